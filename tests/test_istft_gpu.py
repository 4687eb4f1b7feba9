"""GPU checks of the ISTFT (gdsp_istft_batch_device, gdsp_istft_batch, Istft,
IstftBatch) against the numpy model of istft_ref.py.

Metric. Near a zero of the window out = y / w amplifies the transform's
roundoff by 1 / w, so the engine is held to istft_ref.weighted_err < EXACT (the
error times sqrt(D / max D) over the row's largest sample, bounded by the
transform's roundoff whatever the window) and to TOL unweighted over D > 0.
test_istft_host.py proves on the CPU that the model itself sits 300 and 5
times inside the two.

Shapes: the smallest that reach each way the kernel can go wrong. F = 64, 256
and 1024 run S = 16, 4 and 1 packed pairs per wave and F = 2048 the two-wave
worker; a group is 2 S segments. Segments per channel 1, 2 S, 2 S + 1 and
4 S + 3; no overlap, half, NFFT // 3, 75 % and Pad = 2 NFFT; 1, 2 and 5
channels scaled by 10^(c mod 4). Inputs are numpy.fft.rfft of windowed Gaussian
segments in a buffer with ld_seg = lp + 3, a spare row per channel and NaN in
every gap; outputs are views with ldo = n + 3 inside a guarded allocation
(guarded.py) whose gaps and pads must come back as GUARD bit for bit."""
import importlib

import numpy as np
import pytest

import istft_ref as R
from guarded import GUARD, guarded, pad_for

pytestmark = pytest.mark.gpu

TOL = 1e-9     # unweighted, over D > 0
EXACT = 1e-13  # weighted (istft_ref.weighted_err)

# (nfft, noverlap, pad) from F
OPTS = {
    "nov0": lambda f: (f, 0, f),
    "half": lambda f: (f, f // 2, f),
    "odd": lambda f: (f, f // 3, f),            # divides nothing
    "q75": lambda f: (f, 3 * f // 4, f),
    "pad2": lambda f: (f // 2, f // 8, f),      # Pad = 2 NFFT: the PAD variant
}
SEGS = {"one": lambda s: 1, "g": lambda s: 2 * s, "g1": lambda s: 2 * s + 1,
        "g3": lambda s: 4 * s + 3}

# (F, options, segments, channels, window): every F with every option kind and
# every segment count, every channel count with every F; Hann on all, Hamming
# and Rectangular on one row per F
TABLE = [
    (64, "nov0", "one", 1, "Hann"), (64, "half", "g", 2, "Hann"), (64, "odd", "g1", 5, "Hann"),
    (64, "q75", "g3", 5, "Hann"), (64, "pad2", "g3", 2, "Hann"),
    (64, "q75", "g1", 2, "Hamming"), (64, "half", "g3", 1, "Rectangular"),
    (256, "nov0", "g3", 5, "Hann"), (256, "half", "one", 2, "Hann"), (256, "odd", "g", 1, "Hann"),
    (256, "q75", "g1", 2, "Hann"), (256, "pad2", "g1", 5, "Hann"),
    (256, "odd", "g3", 2, "Hamming"), (256, "nov0", "g1", 1, "Rectangular"),
    (1024, "nov0", "g1", 2, "Hann"), (1024, "half", "g3", 5, "Hann"),
    (1024, "odd", "one", 5, "Hann"), (1024, "q75", "g", 1, "Hann"), (1024, "pad2", "g3", 2, "Hann"),
    (1024, "q75", "g3", 2, "Hamming"), (1024, "odd", "g1", 1, "Rectangular"),
    (2048, "nov0", "g", 5, "Hann"), (2048, "half", "g1", 1, "Hann"), (2048, "odd", "g3", 2, "Hann"),
    (2048, "q75", "g3", 2, "Hann"), (2048, "pad2", "one", 2, "Hann"),
    (2048, "half", "g3", 2, "Hamming"), (2048, "q75", "g1", 1, "Rectangular"),
]
IDS = ["-".join(str(v) for v in row) for row in TABLE]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


def _pairs(f):
    return max(1, 1024 // f)  # S: packed pairs side by side in a worker


def _make(gdsp, f, opt, nsegs, channels, win="Hann", seed=0):
    """A case: options, the signal x[channels, n_full], its rows X, the model's
    result and D."""
    nfft, nov, pad = OPTS[opt](f) if isinstance(opt, str) else opt
    stride = nfft - nov
    w = np.asarray(getattr(gdsp.window, win)(pad), dtype=np.float64)
    n = R.n_full(nsegs, nfft, stride)
    rng = np.random.default_rng(1000 * f + 7 * nsegs + channels + seed)
    x = (10.0 ** (np.arange(channels) % 4))[:, None] * rng.standard_normal((channels, n))
    X = R.stft_rows(x, w, nfft, stride, pad, nsegs)
    ref, Dw = R.istft_batch(X, w, nfft, stride, pad)
    o = gdsp.spectral.PwelchOptions(NFFT=nfft, Noverlap=nov, Pad=pad,
                                    Window=getattr(gdsp.window, win))
    return dict(nfft=nfft, nov=nov, pad=pad, stride=stride, w=w, n=n, x=x, X=X, ref=ref, D=Dw,
                o=o, nsegs=nsegs, channels=channels)


def _rows_on_device(X):
    """X[channels, rows, lp] in a buffer with ld_seg = lp + 3, a spare row per
    channel and NaN in every gap."""
    import torch
    channels, rows, lp = X.shape
    nan = complex(float("nan"), float("nan"))
    buf = torch.full((channels, rows + 1, lp + 3), nan, dtype=torch.complex128, device="cuda")
    view = buf[:, :rows, :lp]
    view.copy_(torch.from_numpy(np.ascontiguousarray(X)).cuda())
    return view


def _guarded_out(channels, n, fill=GUARD):
    """A (channels, n) view with ldo = n + 3 inside a guarded allocation; check()
    asserts that the pads and the gaps hold GUARD's bits."""
    import torch
    whole, check_pads = guarded(torch.full((channels, n + 3), GUARD, dtype=torch.float64,
                                           device="cuda"), GUARD, pad_for(n + 3))
    view = whole[:, :n]
    if fill != GUARD:
        view.fill_(fill)

    def check():
        torch.cuda.synchronize()
        check_pads("istft output")
        assert bool((whole[:, n:] == GUARD).all()), "the gap behind a row changed"

    return view, check


def _run(D, c, X=None, stream=None, fill=GUARD, **kw):
    """One device call on the rows in a NaN-gapped buffer into a guarded output."""
    Xd = _rows_on_device(c["X"] if X is None else X)
    n = kw.get("n", None) or c["n"]
    b, e = kw.get("out_begin", 0), kw.get("out_end", None)
    e = n if e is None else e
    out, check = _guarded_out(Xd.shape[0], e - b, fill)
    r = D.istft_batch(Xd, c["o"], out=out, stream=stream, **kw)
    if stream is not None:
        stream.synchronize()
    check()
    assert r.data_ptr() == out.data_ptr()
    return out.contiguous().cpu().numpy()


class _no_fused:
    """The materialised form for the calls inside the block."""

    def __init__(self, gdsp):
        self.F = gdsp.fft

    def __enter__(self):
        self.prev = self.F.Algorithm()
        self.F.SetAlgorithm(self.prev | self.F.ALGO_NO_FUSED_ISTFT)

    def __exit__(self, *exc):
        self.F.SetAlgorithm(self.prev)
        return False


def _fused(gdsp, c):
    return gdsp.spectral.istft_batch_fused(c["channels"], c["nsegs"], c["nfft"], c["pad"], c["nov"])


def _check_against(got, ref, Dw, what, bound_w=EXACT, bound_p=TOL):
    """Every channel row: weighted EXACT, unweighted TOL, exact zeros where D == 0."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for c in range(ref.shape[0]):
        ew, ep = R.weighted_err(got[c], ref[c], Dw), R.plain_err(got[c], ref[c], Dw)
        print(what, "channel", c, "weighted %.2e plain %.2e" % (ew, ep))
        assert ew < bound_w and ep < bound_p, (what, c, ew, ep)
    assert np.all(got[:, Dw == 0] == 0.0), what + ": a sample without weight is not 0"


_cache: dict = {}


def _case(gdsp, D, i):
    """The inputs, the model and the fused kernel's result of TABLE[i], once."""
    if i not in _cache:
        f, opt, seg, channels, win = TABLE[i]
        c = _make(gdsp, f, opt, SEGS[seg](_pairs(f)), channels, win)
        assert _fused(gdsp, c), TABLE[i]
        c["got"] = _run(D, c)
        _cache[i] = c
    return _cache[i]


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_fused_kernel_vs_model_and_signal(gdsp, D, i):
    c = _case(gdsp, D, i)
    assert c["got"].shape == (c["channels"], c["n"])  # n_out = n_full
    _check_against(c["got"], c["ref"], c["D"], "model")
    # the round trip: the signal wherever a sample has weight
    _check_against(c["got"], np.where(c["D"] > 0, c["x"], 0.0), c["D"], "signal")


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_materialised_form_agrees_with_fused_kernel(gdsp, D, i):
    c = _case(gdsp, D, i)
    with _no_fused(gdsp):
        assert not _fused(gdsp, c)
        mat = _run(D, c)
    for ch in range(c["channels"]):
        e = R.weighted_err(mat[ch], c["got"][ch], c["D"], scale=np.max(np.abs(c["ref"][ch])))
        print("materialised against fused, channel", ch, "%.2e" % e)
        assert e < EXACT
    assert np.all(mat[:, c["D"] == 0] == 0.0)


@pytest.mark.parametrize("nfft,nov", [(32, 16), (100, 30), (64, 63), (3000, 1000), (4096, 2048)])
def test_materialised_form_vs_model(gdsp, D, nfft, nov):
    c = _make(gdsp, nfft, (nfft, nov, nfft), 7, 2)
    assert not _fused(gdsp, c)
    got = _run(D, c)
    _check_against(got, c["ref"], c["D"], "model")
    _check_against(got, np.where(c["D"] > 0, c["x"], 0.0), c["D"], "signal")


@pytest.mark.parametrize("f,opt", [(64, "half"), (64, "q75"), (1024, "odd"), (2048, "q75")])
def test_sample_ranges_give_the_whole_calls_bits(gdsp, D, f, opt):
    import torch
    s = _pairs(f)
    c = _make(gdsp, f, opt, 4 * s + 3, 2)
    whole = _run(D, c)
    stride, n, nsegs, nfft = c["stride"], c["n"], c["nsegs"], c["nfft"]
    Xd = _rows_on_device(c["X"])
    for k in (2 * stride * (s + 1), 3 * stride, 2 * stride * s + stride // 2 + 1):
        assert 0 < k < n
        out, check = _guarded_out(2, n)
        D.istft_batch(Xd, c["o"], out=out[:, :k], out_begin=0, out_end=k)
        check()
        assert bool((out[:, k:] == GUARD).all()), "the first call wrote the second range"
        first = out[:, :k].cpu().numpy()
        out[:, :k] = GUARD
        D.istft_batch(Xd, c["o"], out=out[:, k:], out_begin=k, out_end=n)
        check()
        assert bool((out[:, :k] == GUARD).all()), "the second call wrote the first range"
        assert np.array_equal(first, whole[:, :k]), k
        assert np.array_equal(out[:, k:].cpu().numpy(), whole[:, k:]), k
    # only the needed rows present: seg_row0 > 0. The fused kernel transforms rows
    # (2p, 2p + 1) together, so the range's rows are needed as whole pairs; Hamming
    # gives every sample of every row a weight.
    c = _make(gdsp, f, opt, 4 * s + 3, 2, win="Hamming")
    whole = _run(D, c)
    G = gdsp._lib
    win = torch.from_numpy(c["w"]).cuda()
    null = G._P()

    def call(k, row0, X):
        out, check = _guarded_out(2, n - k)
        st = G.lib().gdsp_istft_batch_device(
            G._P(X.data_ptr()), X.stride(1), X.stride(0), 2, nsegs, row0, nsegs - row0, nfft,
            c["pad"], c["nov"], G._P(win.data_ptr()), k, n, G._P(out.data_ptr()), out.stride(0),
            null)
        check()
        return st, out

    # the first needed row is 4 S, the first of its pair
    k = n - 2 * stride - 1
    slo = (k - nfft) // stride + 1
    assert slo == nsegs - 3 and slo % 2 == 0 and np.all(c["D"][k:] > 0)
    st, out = call(k, slo, _rows_on_device(c["X"][:, slo:]))
    assert st == G.GDSP_OK
    assert np.array_equal(out.cpu().numpy(), whole[:, k:])
    # the first needed row is 4 S + 1, the second of its pair: with its partner the
    # whole call's bits, without it refused (as is a missing needed row), nothing written
    k = n - stride - 1
    assert (k - nfft) // stride + 1 == slo + 1
    st, out = call(k, slo, _rows_on_device(c["X"][:, slo:]))
    assert st == G.GDSP_OK
    assert np.array_equal(out.cpu().numpy(), whole[:, k:])
    for row0 in (slo + 1, slo + 2):
        st, out = call(k, row0, _rows_on_device(c["X"][:, row0:]))
        assert st == G.GDSP_ERR_INVALID, row0
        assert bool((out == GUARD).all())
    # the materialised form transforms every row alone: the needed rows suffice
    with _no_fused(gdsp):
        mat = _run(D, c)
        st, out = call(k, slo + 1, _rows_on_device(c["X"][:, slo + 1:]))
        assert st == G.GDSP_OK
        assert np.array_equal(out.cpu().numpy(), mat[:, k:])


def test_ranges_inside_a_gap_between_segments_are_zeros(gdsp, D):
    """A negative Noverlap leaves gaps (the materialised form): a range that no
    segment covers, a range that begins in a gap, and the whole call."""
    c = _make(gdsp, 64, (64, -64, 64), 5, 2, win="Hamming")
    assert not _fused(gdsp, c)
    got = _run(D, c)
    _check_against(got, c["ref"], c["D"], "model")
    assert np.all(got[:, 64:128] == 0.0)
    gap = _run(D, c, out_begin=64, out_end=128)
    assert gap.shape == (2, 64) and np.all(gap == 0.0)
    assert np.array_equal(_run(D, c, out_begin=70, out_end=300), got[:, 70:300])
    host = gdsp.spectral.IstftBatch(c["X"], c["o"])
    assert np.array_equal(host, got)


@pytest.mark.parametrize("f,opt,m", [(64, "half", 4), (64, "q75", 4), (2048, "half", 4),
                                     (2048, "q75", 4), (2048, "q75", 12), (1024, "q75", 12)])
def test_worker_boundaries_inside_a_channel(gdsp, D, f, opt, m):
    """One channel of m * 2 S + 3 segments: two workers at m = 4, four at m = 12
    (where a group is one pair and the halo two groups, a worker's halo begins
    inside its predecessor's run), each after the first with a halo to recompute."""
    s = _pairs(f)
    c = _make(gdsp, f, opt, m * 2 * s + 3, 1)
    before = gdsp.fft.LoopStats()["multi_unit_launches"]
    got = _run(D, c)
    assert gdsp.fft.LoopStats()["multi_unit_launches"] == before + 1  # groups per worker >= 2
    _check_against(got, c["ref"], c["D"], "model")


def test_channel_count_and_grid_change_no_bit(gdsp, D):
    """Row r alone, inside a 5-channel batch and inside a 2048-channel batch (F =
    64, 35 segments, half overlap: one worker per channel, several groups)."""
    c = _make(gdsp, 64, "half", 35, 2048)
    big = _run(D, c)
    _check_against(big, c["ref"], c["D"], "model")
    for r in (0, 3, 2047):
        alone = _run(D, c, X=c["X"][r:r + 1])
        assert np.array_equal(alone[0], big[r]), r
    five = _run(D, c, X=c["X"][1:6])
    assert np.array_equal(five, big[1:6])


@pytest.mark.parametrize("f,fused", [(64, True), (256, True), (2048, True), (256, False)])
def test_quiet_row_keeps_its_digits(gdsp, D, f, fused):
    """Row 0 of every channel times 2^-40: the samples only segment 0 covers are
    judged on their own scale."""
    s = _pairs(f)
    c = _make(gdsp, f, "half", 2 * s + 1, 2)
    X = c["X"].copy()
    X[:, 0] *= 2.0 ** -40
    ref, Dw = R.istft_batch(X, c["w"], c["nfft"], c["stride"], c["pad"])
    if fused:
        got = _run(D, c, X=X)
    else:
        with _no_fused(gdsp):
            got = _run(D, c, X=X)
    k = c["stride"]
    for ch in range(2):
        own = R.weighted_err(got[ch, :k], ref[ch, :k], Dw[:k])
        rest = R.weighted_err(got[ch], ref[ch], Dw)
        print("quiet row", f, fused, "own scale %.2e whole row %.2e" % (own, rest))
        assert own < EXACT and rest < EXACT
        assert np.max(np.abs(ref[ch, :k])) < 2.0 ** -30 * np.max(np.abs(ref[ch]))


@pytest.mark.parametrize("f", [64, 1024, 2048])
def test_zero_row_adds_exact_zeros(gdsp, D, f):
    s = _pairs(f)
    for opt in ("nov0", "half"):
        c = _make(gdsp, f, opt, 4 * s + 1, 2)
        clean = _run(D, c)
        stride, nfft = c["stride"], c["nfft"]
        # the first of a pair, the second, the unpartnered last
        for row in (2, 3, 4 * s):
            X = c["X"].copy()
            X[0, row] = 0.0
            ref, Dw = R.istft_batch(X, c["w"], nfft, stride, c["pad"])
            got = _run(D, c, X=X)
            lo = row * stride + (nfft - stride if row > 0 else 0)
            hi = (row + 1) * stride if row < c["nsegs"] - 1 else c["n"]
            assert hi > lo or (opt == "half" and row < c["nsegs"] - 1)
            assert np.all(got[0, lo:max(lo, hi)] == 0.0), (opt, row)   # covered by it alone
            assert R.weighted_err(got[0], ref[0], Dw) < EXACT, (opt, row)
            assert np.array_equal(got[1], clean[1]), (opt, row)


def _bad_samples(c, row):
    i = np.arange(c["n"])
    return (i >= row * c["stride"]) & (i < row * c["stride"] + c["nfft"]) & (c["D"] > 0)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "materialised"])
@pytest.mark.parametrize("opt", ["nov0", "half", "q75"])
@pytest.mark.parametrize("f", [64, 1024, 2048])
def test_non_finite_rows_stay_in_their_samples(gdsp, D, f, opt, fused):
    s = _pairs(f)
    c = _make(gdsp, f, opt, 4 * s + 1, 2)

    def run(X):
        if fused:
            return _run(D, c, X=X)
        with _no_fused(gdsp):
            return _run(D, c, X=X)

    clean = run(c["X"])
    # an odd row of the first group, an even row of a later one, the unpartnered last
    for row in (1, 2 * s, 4 * s):
        # in the real part of bin 0, then of bin F / 2: the elements with a weight
        # in every sample of the segment (the cosine or sine of another bin is
        # exactly 0 at some samples, and whether a NaN reaches those is an
        # accident of a transform's arithmetic: numpy's irfft leaves them finite)
        for bad, j in ((float("nan"), 0), (float("inf"), c["pad"] // 2)):
            X = c["X"].copy()
            X[0, row, j] = complex(bad, X[0, row, j].imag)
            got = run(X)
            want = _bad_samples(c, row)
            assert np.array_equal(~np.isfinite(got[0]), want), (row, bad)
            e = R.weighted_err(got[0][~want], clean[0][~want], c["D"][~want],
                               scale=np.max(np.abs(c["ref"][0])))
            assert e < EXACT, (row, bad, e)
            assert np.array_equal(got[1], clean[1]), (row, bad)
    # the ignored imaginary parts of bins 0 and F / 2
    X = c["X"].copy()
    X[0, 1, 0] = complex(X[0, 1, 0].real, float("nan"))
    X[1, 2 * s, c["pad"] // 2] = complex(X[1, 2 * s, c["pad"] // 2].real, float("nan"))
    assert np.array_equal(run(X), clean)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "materialised"])
@pytest.mark.parametrize("opt", ["nov0", "q75"])
@pytest.mark.parametrize("f", [64, 1024, 2048])
def test_non_finite_in_any_bin_stays_in_its_segment(gdsp, D, f, opt, fused):
    """A NaN or an Inf in the real or the imaginary part of bins inside a row (an
    even row, an odd row, the unpartnered last, at F = 2048 through the two-wave
    worker's re-runs): non-finite samples only among the promised ones, every
    other sample within EXACT of the clean run, the other channel unchanged. The
    elements of bin 0 and F / 2 that reach every sample must make all the
    promised samples non-finite (test_non_finite_rows_stay_in_their_samples)."""
    s = _pairs(f)
    c = _make(gdsp, f, opt, 4 * s + 1, 2)

    def run(X):
        if fused:
            return _run(D, c, X=X)
        with _no_fused(gdsp):
            return _run(D, c, X=X)

    clean = run(c["X"])
    lp = c["pad"] // 2 + 1
    # (row, bin, part): bins of lane 0 and of other lanes, low and high registers
    spots = ((1, 5, 0), (1, lp - 2, 1), (2 * s, f // 16 + 3, 1), (2 * s, 1, 0),
             (4 * s, lp // 2, 0), (4 * s, 7 * (f // 16) + 2, 1), (2 * s + 1, f // 4, 1))
    for n_spot, (row, j, part) in enumerate(spots):
        bad = float("nan") if n_spot % 2 == 0 else float("-inf")
        X = c["X"].copy()
        z = X[0, row, j]
        X[0, row, j] = complex(bad, z.imag) if part == 0 else complex(z.real, bad)
        got = run(X)
        want = _bad_samples(c, row)
        nonfinite = ~np.isfinite(got[0])
        assert nonfinite.any() and not np.any(nonfinite & ~want), (row, j, part)
        ok = ~want
        e = R.weighted_err(got[0][ok], clean[0][ok], c["D"][ok], scale=np.max(np.abs(c["ref"][0])))
        assert e < EXACT, (row, j, part, e)
        assert np.array_equal(got[1], clean[1]), (row, j, part)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "materialised"])
@pytest.mark.parametrize("f,opt", [(64, "q75"), (256, "odd"), (2048, "half")])
def test_scaling_by_a_power_of_two_is_exact(gdsp, D, f, opt, fused):
    c = _make(gdsp, f, opt, 2 * _pairs(f) + 1, 2)

    def run(X):
        if fused:
            return _run(D, c, X=X)
        with _no_fused(gdsp):
            return _run(D, c, X=X)

    assert np.array_equal(run(c["X"] * 1024.0), run(c["X"]) * 1024.0)


@pytest.mark.parametrize("f,opt", [(64, "q75"), (1024, "odd"), (2048, "half")])
def test_repeatable_on_any_stream_and_stale_output(gdsp, D, f, opt):
    import torch
    c = _make(gdsp, f, opt, 4 * _pairs(f) + 3, 2)
    a = _run(D, c)
    assert np.array_equal(_run(D, c), a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert np.array_equal(_run(D, c, stream=side), a)
    assert np.array_equal(_run(D, c, fill=float("nan")), a)
    with _no_fused(gdsp):
        m = _run(D, c)
        assert np.array_equal(_run(D, c, fill=float("nan")), m)


@pytest.mark.parametrize("i", [1, 11, 24, -1], ids=["64-half", "256-pad2", "2048-q75", "100-30"])
def test_host_entries(gdsp, D, i):
    S = gdsp.spectral
    c = _case(gdsp, D, i) if i >= 0 else _make(gdsp, 100, (100, 30, 100), 7, 2)
    dev = c["got"] if i >= 0 else _run(D, c)
    got = S.IstftBatch(c["X"], c["o"])
    assert got.shape == (c["channels"], c["n"]) and got.dtype == np.float64
    assert np.array_equal(got, dev)           # one range: the device call's bits
    short = S.IstftBatch(c["X"], c["o"], n=c["n"] - c["stride"] // 2 - 1)
    assert np.array_equal(short, dev[:, :short.shape[1]])
    one = S.Istft(c["X"][-1], c["o"])
    assert np.array_equal(one, dev[-1])


def test_istft_of_stft_returns_the_signal(gdsp, D):
    S = gdsp.spectral
    rng = np.random.default_rng(5)
    for nfft, nov in ((256, 128), (64, 48), (100, 30)):
        o = S.PwelchOptions(NFFT=nfft, Noverlap=nov, Window=gdsp.window.Hamming)
        stride = nfft - nov
        x = rng.standard_normal(9 * stride + nfft + stride - 1)  # a tail shorter than a stride
        X, _, _ = S.Stft(x, 1.0, o)
        y = S.Istft(X, o)
        assert y.shape == (9 * stride + nfft,)
        Dw = R.weights(np.asarray(gdsp.window.Hamming(nfft)), 10, nfft, stride)
        assert R.weighted_err(y, x[:y.size], Dw) < EXACT and R.plain_err(y, x[:y.size], Dw) < TOL
        # a signal shorter than NFFT: one zero-padded segment, n = len(x)
        x = rng.standard_normal(nfft - 7)
        X, _, _ = S.Stft(x, 1.0, o)
        assert X.shape[0] == 1
        y = S.Istft(X, o, n=x.size)
        assert y.shape == x.shape
        Dw = R.weights(np.asarray(gdsp.window.Hamming(nfft)), 1, nfft, stride)[:x.size]
        assert R.weighted_err(y, x, Dw) < EXACT and R.plain_err(y, x, Dw) < TOL


def test_host_chunk_loop_past_its_first_iteration(gdsp, D):
    """One channel, F = 64, Noverlap 48, rows just over ISTFT_CHUNK_ELEMS: the
    second range of gdsp_istft_batch. Checked around the cut and at the end
    against irfft of the rows that reach those samples."""
    import torch
    S = gdsp.spectral
    nfft, nov, lp, stride = 64, 48, 33, 16
    fit = S.ISTFT_CHUNK_ELEMS // lp
    nsegs = fit + 40
    rng = np.random.default_rng(11)
    X = rng.standard_normal((nsegs, lp, 2)).view(np.complex128).reshape(nsegs, lp)
    o = S.PwelchOptions(NFFT=nfft, Noverlap=nov)
    w = np.asarray(gdsp.window.Hann(nfft), dtype=np.float64)
    before = gdsp.fft.LoopStats()["later_chunks"]
    y = S.Istft(X, o)
    assert gdsp.fft.LoopStats()["later_chunks"] > before
    n = R.n_full(nsegs, nfft, stride)
    assert y.shape == (n,)
    # the cut of gdsp_istft_batch: rows per range from the chunk, whole pairs, less the halo
    cut = ((fit - 4 - 2) & ~1) * stride
    assert 0 < cut < n

    def model(lo, hi):
        a = max(0, (lo - nfft) // stride - 1) & ~1
        b = min(nsegs, hi // stride + 2)
        out, Dw = R.istft(X[a:b], w, nfft, stride, nfft)
        return a, b, out[lo - a * stride:hi - a * stride], Dw[lo - a * stride:hi - a * stride]

    for lo, hi in ((cut - 200, cut + 200), (n - 300, n)):
        a, b, ref, Dw = model(lo, hi)
        if b < nsegs:  # the partial window sums at the slice's ends are not the signal's
            assert lo - a * stride >= nfft and hi <= (b - 1) * stride
        e = R.weighted_err(y[lo:hi], ref, Dw)
        print("chunk loop", lo, hi, "%.2e" % e)
        assert e < EXACT
    assert y[n - 1] == 0.0  # Hann's zero
    # behind the cut: the bits of a device call on that range
    a = max(0, (cut - nfft) // stride - 1) & ~1
    b = min(nsegs, (cut + 400) // stride + 2)
    Xd = _rows_on_device(X[None, a:b])
    win = torch.from_numpy(w).cuda()
    out, check = _guarded_out(1, 400)
    G = gdsp._lib
    st = G.lib().gdsp_istft_batch_device(
        G._P(Xd.data_ptr()), Xd.stride(1), Xd.stride(0), 1, nsegs, a, b - a, nfft, nfft, nov,
        G._P(win.data_ptr()), cut, cut + 400, G._P(out.data_ptr()), out.stride(0), G._P())
    check()
    assert st == G.GDSP_OK
    assert np.array_equal(out.cpu().numpy()[0], y[cut:cut + 400])
