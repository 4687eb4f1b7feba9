"""GPU parity of the per-segment spectra (gdsp_stft_batch_device,
gdsp_spectrogram_batch_device, gdsp_stft_batch, gdsp_spectrogram_batch, Stft,
Spectrogram, SpectrogramChannels).

Two references, built here per segment: the oracle's pieces (its Segment, its
window, zero-padding, its FFTReal, the first lp bins: test_cpsd_gpu._reference's
spectra), held to the suite's 1e-9, and numpy.fft.fft of the exact segments,
held to 1e-13 like every engine-against-engine comparison. Every comparison is
conftest.row_nrel with one row per segment, so a quiet segment is judged on its
own scale. test_stft_host.py proves on the CPU that the two references agree to
1e-14 and that the mean over the segments of the power rows built from them is
the oracle's Pwelch.

Shapes: the smallest that reach each way the kernel can go wrong. F = 64, 256
and 1024 run S = 16, 4 and 1 segment pairs per wave and F = 2048 the two-wave
workgroup with the mirror across its waves; segments per channel 1 (no
partner), 2 S (one exact group), 2 S + 1 (a full group and a masked one holding
one unpartnered segment) and 4 S + 3, with a tail shorter than a stride; 1, 2
and 5 channels scaled by 10^(c mod 4), so a leak between channels shows in the
per-row error. Inputs live in a buffer of row stride n + 3 with NaN in the gaps.
Outputs are views of a guarded allocation (guarded.py) with ld_seg = lp + 3 and a
spare segment row per channel: every gap, spare and pad element must come back
as GUARD, bit for bit."""
import importlib
import io

import numpy as np
import pytest

import test_cpsd_gpu as CP
from conftest import row_nrel
from guarded import GUARD, guarded, pad_for

pytestmark = pytest.mark.gpu

TOL = 1e-9     # north star: within 1e-9 relative
EXACT = 1e-13  # engine against engine, and against numpy on the exact segments
FS = 48000.0
assert (TOL, EXACT, FS) == (CP.TOL, CP.EXACT, CP.FS)

OPTS = CP.OPTS  # nov0, half, odd, pad2 (the PAD variant), padh (pwelch.go:108 quirk)
# segments per channel from S, the pairs side by side in a worker
SEGS = {"one": lambda s: 1, "g": lambda s: 2 * s, "g1": lambda s: 2 * s + 1,
        "g3": lambda s: 4 * s + 3}

# (F, options, segments, channels): every F with every option kind and every
# segment count, every channel count with every F
TABLE = [
    (64, "nov0", "one", 1), (64, "half", "g", 2), (64, "odd", "g1", 5), (64, "pad2", "g3", 5),
    (64, "padh", "g3", 2),
    (256, "nov0", "g3", 5), (256, "half", "one", 2), (256, "odd", "g", 1), (256, "pad2", "g1", 2),
    (256, "padh", "g1", 5),
    (1024, "nov0", "g1", 2), (1024, "half", "g3", 5), (1024, "odd", "one", 5),
    (1024, "pad2", "g", 1), (1024, "padh", "g3", 2),
    (2048, "nov0", "g", 5), (2048, "half", "g1", 1), (2048, "odd", "g3", 2),
    (2048, "pad2", "one", 2), (2048, "padh", "g3", 5),
]
IDS = ["-".join(str(v) for v in row) for row in TABLE]
MODES = ("complex", "power")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


def _shape(row):
    f, opt, seg, channels = row
    nfft, nov, pad = OPTS[opt](f)
    pad = pad or nfft  # the default, spelled out
    s = max(1, 1024 // f)  # pairs side by side in a worker
    nsegs = SEGS[seg](s)
    stride = nfft - nov
    n = (nsegs - 1) * stride + nfft + min(3, stride - 1)  # a tail shorter than a stride
    return nfft, nov, pad, nsegs, n, channels


def _signals(seed, channels, n):
    """Gaussian rows, row c scaled by 10^(c mod 4)."""
    rng = np.random.default_rng(seed)
    return (10.0 ** (np.arange(channels) % 4))[:, None] * rng.standard_normal((channels, n))


def _segments(r, nfft, nov, flen):
    """The exact segments of one row, zero-padded to flen (and the row to nfft)."""
    r = np.asarray(r, dtype=np.float64)
    if r.size < nfft:
        r = np.concatenate([r, np.zeros(nfft - r.size)])
    stride = nfft - nov
    nsegs = 1 if r.size == nfft else (r.size - nfft) // stride + 1
    segs = np.zeros((nsegs, flen))
    for s in range(nsegs):
        segs[s, :nfft] = r[s * stride:s * stride + nfft]
    return segs


def _reference(oracle, x, nfft, nov, pad, win="hann", only=None):
    """(oracle rows, numpy rows), each (channels, nsegs, lp) complex: the first
    lp bins of the transform of every windowed, zero-padded segment. only: the
    segment indices to compute (the others are left zero)."""
    flen, lp = max(pad, nfft), pad // 2 + 1
    w = oracle.window(win, flen)
    ref_o, ref_n = [], []
    for r in x:
        rr = np.asarray(r, dtype=np.float64)
        if rr.size < nfft:
            rr = np.concatenate([rr, np.zeros(nfft - rr.size)])
        segs = oracle.segment(rr, nfft, nov)
        exact = _segments(r, nfft, nov, flen)
        assert len(segs) == len(exact)
        rows = np.zeros((len(segs), lp), np.complex128)
        for s, seg in enumerate(segs):
            if only is not None and s not in only:
                continue
            z = np.zeros(flen)
            z[:nfft] = seg
            rows[s] = oracle.fft_real(z * w)[:lp]
        ref_o.append(rows)
        num = np.zeros((len(segs), lp), np.complex128)
        pick = range(len(segs)) if only is None else sorted(only)
        num[list(pick)] = np.fft.fft(exact[list(pick)] * w[None, :], axis=1)[:, :lp]
        ref_n.append(num)
    return np.stack(ref_o), np.stack(ref_n)


def _power(rows, nfft, pad, fs=FS, window=None):
    """c_j |X|^2 / norm of complex rows (..., lp): Hann (the host table, no GPU)
    unless a window table of nfft is given."""
    lp = pad // 2 + 1
    if window is None:
        window = importlib.import_module("go-dsp_amd").window.Hann(nfft)
    norm = float(np.sum(np.asarray(window, dtype=np.float64) ** 2)) * fs
    cj = np.ones(lp)
    cj[1:lp - 1] = 2.0
    return cj * (rows.real * rows.real + rows.imag * rows.imag) / norm


def _flat(a):
    """One row per segment."""
    return np.ascontiguousarray(a).reshape(-1, a.shape[-1])


def _err(got, ref):
    return row_nrel(_flat(got), _flat(ref))


def _guarded_out(channels, ns, lp, power):
    """A (channels, ns, lp) view with ld_seg = lp + 3 and a spare row per channel
    inside a guarded allocation full of GUARD; check() asserts that everything
    but the view still holds GUARD's bits."""
    import torch
    dt = torch.float64 if power else torch.complex128
    fill = GUARD if power else complex(GUARD, GUARD)
    whole, check_pads = guarded(torch.full((channels, ns + 1, lp + 3), fill, dtype=dt,
                                           device="cuda"), GUARD, pad_for(lp + 3))
    view = whole[:, :ns, :lp]

    def check(untouched=()):
        """untouched: segment rows of the view that must still hold GUARD."""
        torch.cuda.synchronize()
        check_pads("stft output")
        raw = torch.view_as_real(whole) if not power else whole
        assert bool((raw[:, ns] == GUARD).all()), "the spare segment row changed"
        assert bool((raw[:, :, lp:] == GUARD).all()), "the gap behind a row changed"
        for s in untouched:
            assert bool((raw[:, s] == GUARD).all()), "row %d was written" % s

    return view, check


def _run(D, x, o, power, seg_begin=0, seg_end=None, stream=None, nsegs=None, fs=FS):
    """One device call on the rows of x in a NaN-gapped buffer into a guarded
    output: (rows as numpy, freqs, times)."""
    nfft, pad, nov, _, _ = importlib.import_module("go-dsp_amd").spectral.resolve_options(o)
    lp = pad // 2 + 1
    if nsegs is None:
        n = max(x.shape[1], nfft)
        nsegs = 1 if n == nfft else (n - nfft) // (nfft - nov) + 1
    end = nsegs if seg_end is None else seg_end
    out, check = _guarded_out(x.shape[0], end - seg_begin, lp, power)
    xd = CP._strided(x, 3)
    if power:
        r, freqs, times = D.spectrogram_batch(xd, fs, o, out=out, seg_begin=seg_begin,
                                              seg_end=seg_end, stream=stream)
    else:
        r, freqs, times = D.stft_batch(xd, o, out=out, seg_begin=seg_begin, seg_end=seg_end,
                                       stream=stream, Fs=fs)
    if stream is not None:
        stream.synchronize()
    check()
    assert r.data_ptr() == out.data_ptr()
    return out.contiguous().cpu().numpy(), freqs, times


class _no_fused:
    """The materialised form for the calls inside the block."""

    def __init__(self, gdsp):
        self.F = gdsp.fft

    def __enter__(self):
        self.prev = self.F.Algorithm()
        self.F.SetAlgorithm(self.prev | self.F.ALGO_NO_FUSED_STFT)

    def __exit__(self, *exc):
        self.F.SetAlgorithm(self.prev)
        return False


_cache: dict = {}


def _case(gdsp, oracle, D, i):
    """Inputs, both references and the fused kernel's rows of TABLE[i], once."""
    if i not in _cache:
        nfft, nov, pad, nsegs, n, channels = _shape(TABLE[i])
        x = _signals(3000 + i, channels, n)
        o = CP._options(gdsp, nfft, nov, pad)
        assert gdsp.spectral.segment_count(n, nfft, nov) == nsegs
        assert gdsp.spectral.stft_batch_fused(channels, n, nfft, pad, nov)
        ref_o, ref_n = _reference(oracle, x, nfft, nov, pad)
        got = {}
        for mode in MODES:
            got[mode], freqs, times = _run(D, x, o, mode == "power")
        _cache[i] = dict(x=x, o=o, ref_o=ref_o, ref_n=ref_n, got=got, freqs=freqs, times=times)
    return _cache[i]


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_fused_kernel_vs_reference(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    nfft, nov, pad, nsegs, n, channels = _shape(TABLE[i])
    lp = pad // 2 + 1
    X, P = c["got"]["complex"], c["got"]["power"]
    assert X.shape == P.shape == (channels, nsegs, lp)
    for name, ref, bound in (("oracle", c["ref_o"], TOL), ("numpy", c["ref_n"], EXACT)):
        err = _err(X, ref)
        print("complex", IDS[i], name, err)
        assert err < bound, name
        err = _err(P, _power(ref, nfft, pad))
        print("power", IDS[i], name, err)
        assert err < bound, name
    # bins 0 and F / 2 are their own mirrors: real, exactly
    assert np.all(X[:, :, 0].imag == 0)
    if pad // 2 == max(pad, nfft) // 2:
        assert np.all(X[:, :, -1].imag == 0)
    assert np.all(P >= 0)
    assert np.array_equal(c["freqs"], oracle.pwelch(c["x"][0], FS, nfft=nfft, pad=pad,
                                                    noverlap=nov)[1])
    assert np.array_equal(c["times"], (np.arange(nsegs) * (nfft - nov) + nfft / 2) / FS)


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_mean_over_segments_is_pwelch(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    nfft, nov, pad, _, _, _ = _shape(TABLE[i])
    mean = c["got"]["power"].mean(axis=1)
    single = np.stack([gdsp.spectral.Pwelch(r, FS, c["o"])[0] for r in c["x"]])
    err = row_nrel(mean, single)
    print("spectral.Pwelch", IDS[i], err)
    assert err < EXACT
    ref = np.stack([oracle.pwelch(r, FS, nfft=nfft, pad=pad, noverlap=nov)[0] for r in c["x"]])
    err = row_nrel(mean, ref)
    print("oracle.pwelch", IDS[i], err)
    assert err < TOL


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_power_rows_are_the_scaled_squares_of_the_complex_rows(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    nfft, _, pad, _, _, _ = _shape(TABLE[i])
    err = _err(c["got"]["power"], _power(c["got"]["complex"], nfft, pad))
    print("power against complex", IDS[i], err)
    assert err < EXACT


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_materialised_form_agrees_with_fused_kernel(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    nfft, nov, pad, nsegs, n, channels = _shape(TABLE[i])
    with _no_fused(gdsp):
        assert not gdsp.spectral.stft_batch_fused(channels, n, nfft, pad, nov)
        for mode in MODES:
            got, freqs, times = _run(D, c["x"], c["o"], mode == "power")
            err = _err(got, c["got"][mode])
            print("materialised", IDS[i], mode, err)
            assert err < EXACT, mode
            assert np.array_equal(freqs, c["freqs"]) and np.array_equal(times, c["times"])
            if mode == "complex":
                assert np.all(got[:, :, 0].imag == 0)
    assert gdsp.spectral.stft_batch_fused(channels, n, nfft, pad, nov)


@pytest.mark.parametrize("nfft,nov", [(32, 16), (100, 30), (3000, 1000), (4096, 2048)])
def test_other_lengths_vs_reference(gdsp, oracle, D, nfft, nov):
    channels, nsegs = 3, 5
    n = (nsegs - 1) * (nfft - nov) + nfft + 2
    assert not gdsp.spectral.stft_batch_fused(channels, n, nfft, 0, nov)
    x = _signals(nfft, channels, n)
    o = CP._options(gdsp, nfft, nov, 0)
    ref_o, ref_n = _reference(oracle, x, nfft, nov, nfft)
    for mode in MODES:
        got, freqs, _ = _run(D, x, o, mode == "power")
        assert got.shape == (channels, nsegs, nfft // 2 + 1)
        ref = ref_o if mode == "complex" else _power(ref_o, nfft, nfft)
        err = _err(got, ref)
        print("other", nfft, mode, err)
        assert err < TOL, mode
        assert np.array_equal(freqs, oracle.pwelch(x[0], FS, nfft=nfft, noverlap=nov)[1])


RANGES = [(256, 19, 5), (256, 19, 8), (2048, 5, 1), (2048, 5, 2), (100, 7, 3), (100, 7, 4)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f,nsegs,k", RANGES,
                         ids=["%d-%s" % (f, "odd" if k % 2 else "even") for f, _, k in RANGES])
def test_segment_ranges_fill_one_output(gdsp, D, f, nsegs, k, mode):
    """[0, k) and [k, nsegs) into one output against the whole call. An odd k
    pairs the segments of the second range differently, so its rows agree to
    roundoff; an even k gives the same bits. Each partial call leaves the other
    range's rows untouched."""
    import torch
    power = mode == "power"
    nfft, nov, channels = f, (f // 2 if f != 100 else 30), 5
    lp = nfft // 2 + 1
    stride = nfft - nov
    n = (nsegs - 1) * stride + nfft + min(3, stride - 1)
    assert gdsp.spectral.stft_batch_fused(channels, n, nfft, 0, nov) == (f != 100)
    x = _signals(88 + f, channels, n)
    xd = CP._strided(x, 3)
    o = CP._options(gdsp, nfft, nov, 0)
    whole, _, _ = _run(D, x, o, power)
    out, check = _guarded_out(channels, nsegs, lp, power)

    def call(b, e):
        if power:
            return D.spectrogram_batch(xd, FS, o, out=out[:, b:e], seg_begin=b, seg_end=e)
        return D.stft_batch(xd, o, out=out[:, b:e], seg_begin=b, seg_end=e, Fs=FS)

    _, _, t0 = call(0, k)
    check(untouched=range(k, nsegs))
    first = out[:, :k].contiguous().cpu().numpy()
    out[:, :k] = GUARD if power else complex(GUARD, GUARD)
    _, _, t1 = call(k, nsegs)
    check(untouched=range(k))
    got = np.concatenate([first, out[:, k:].contiguous().cpu().numpy()], axis=1)
    torch.cuda.synchronize()
    err = _err(got, whole)
    print("ranges", f, k, mode, err)
    assert err < EXACT
    # the same pairs from the same start: the same bits (segment k - 1 of an odd
    # k has lost its partner)
    assert np.array_equal(got[:, :k - k % 2], whole[:, :k - k % 2])
    if k % 2 == 0 or f == 100:
        assert np.array_equal(got, whole)
    assert np.array_equal(np.concatenate([t0, t1]),
                          (np.arange(nsegs) * stride + nfft / 2) / FS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nfft,nov", [(64, 32), (256, 0), (2048, 1024), (100, 30)],
                         ids=["64", "256", "2048", "100-materialised"])
def test_first_segment_far_below_the_rest(gdsp, oracle, D, nfft, nov, mode):
    """The samples of segment 0 scaled by 1e-12 (a fade-in, a channel switched on
    late): its row is held to TOL on its own scale. A packed pair's roundoff is
    relative to the louder segment, so without the per-pair balance the quiet
    row is off by about 1e-4."""
    channels, nsegs = 2, 2 * max(1, 1024 // nfft) + 2
    stride = nfft - nov
    n = (nsegs - 1) * stride + nfft + 1
    assert gdsp.spectral.stft_batch_fused(channels, n, nfft, 0, nov) == (nfft != 100)
    x = _signals(500 + nfft, channels, n)
    x[:, :nfft] *= 1e-12  # the whole of segment 0
    o = CP._options(gdsp, nfft, nov, 0)
    ref_o, ref_n = _reference(oracle, x, nfft, nov, nfft)
    assert np.abs(ref_o[0, 0]).max() < 1e-9 * np.abs(ref_o[0, -1]).max()
    got, _, _ = _run(D, x, o, mode == "power")
    refs = [("oracle", ref_o, TOL)]
    if nfft != 100:  # the fused kernel against numpy on the exact segments too
        refs.append(("numpy", ref_n, EXACT))
    for name, ref, bound in refs:
        err = _err(got, ref if mode == "complex" else _power(ref, nfft, nfft))
        print("quiet", nfft, mode, name, err)
        assert err < bound, name


@pytest.mark.parametrize("nfft,fused", [(64, True), (256, True), (2048, True), (100, False)],
                         ids=["64", "256", "2048", "100-materialised"])
def test_all_zero_segment_gives_a_row_of_zeros(gdsp, D, nfft, fused):
    """A segment of exact zeros: its row is exact zeros in both modes, not its
    partner's roundoff, and every other row is within EXACT of the clean run."""
    channels, nsegs = 2, 2 * max(1, 1024 // nfft) + 3
    n = nsegs * nfft + 1
    assert gdsp.spectral.stft_batch_fused(channels, n, nfft, 0, 0) == fused
    x = _signals(600 + nfft, channels, n)
    o = CP._options(gdsp, nfft, 0, 0)
    for mode in MODES:
        clean, _, _ = _run(D, x, o, mode == "power")
        for dead in (0, 3, nsegs - 1):  # the first of a pair, the second, the unpartnered last
            y = x.copy()
            y[1, dead * nfft:(dead + 1) * nfft] = 0.0
            got, _, _ = _run(D, y, o, mode == "power")
            assert np.all(got[1, dead] == 0), (mode, dead)
            keep = np.ones((channels, nsegs), bool)
            keep[1, dead] = False
            assert np.isfinite(got).all()
            err = row_nrel(got[keep], clean[keep])
            print("zeros", nfft, mode, dead, err)
            assert err < EXACT, (mode, dead)
            assert np.array_equal(got[0], clean[0])  # the other channel: not a bit


@pytest.mark.parametrize("nfft,nov,fused", [(64, 0, True), (64, 32, True), (256, 128, True),
                                            (2048, 0, True), (2048, 1024, True), (100, 0, False),
                                            (100, 50, False)],
                         ids=["64-nov0", "64-half", "256-half", "2048-nov0", "2048-half",
                              "100-nov0-materialised", "100-half-materialised"])
def test_non_finite_sample_stays_in_its_segments(gdsp, D, nfft, nov, fused):
    """One NaN, then one Inf: exactly the rows of the segments that contain the
    sample are non-finite (every bin), every other row is finite and within
    EXACT of the clean run; the other channel does not change by a bit."""
    channels, nsegs = 2, 4 * max(1, 1024 // nfft) + 3
    stride = nfft - nov
    n = (nsegs - 1) * stride + nfft + 1
    assert gdsp.spectral.stft_batch_fused(channels, n, nfft, 0, nov) == fused
    x = _signals(700 + nfft + nov, channels, n)
    o = CP._options(gdsp, nfft, nov, 0)
    # inside the first group (an odd segment's own half), inside an even segment
    # of the second group, and in the unpartnered last segment
    spots = (stride + nfft - 3, 2 * (nsegs // 4) * stride + 5 * nfft // 8, n - 4)
    for mode in MODES:
        clean, _, _ = _run(D, x, o, mode == "power")
        assert np.isfinite(clean).all()
        for value in (float("nan"), float("inf")):
            for at in spots:
                y = x.copy()
                y[1, at] = value
                hit = [s for s in range(nsegs) if s * stride <= at < s * stride + nfft]
                assert hit and len(hit) <= 2
                got, _, _ = _run(D, y, o, mode == "power")
                bad = np.zeros((channels, nsegs), bool)
                bad[1, hit] = True
                assert not np.isfinite(got[bad]).any(), (mode, value, at, "a bin stayed finite")
                assert np.isfinite(got[~bad]).all(), (mode, value, at, "the sample spread")
                err = row_nrel(got[~bad], clean[~bad])
                print("non-finite", nfft, nov, mode, value, at, hit, err)
                assert err < EXACT, (mode, value, at)
                assert np.array_equal(got[0], clean[0])


@pytest.mark.parametrize("i", [2, 8, 11, 19], ids=[IDS[i] for i in (2, 8, 11, 19)])
def test_scaling_by_a_power_of_two_is_exact(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    x = np.ldexp(c["x"], 10)
    for mode, k in (("complex", 10), ("power", 20)):
        got, _, _ = _run(D, x, c["o"], mode == "power")
        base = c["got"][mode]
        back = np.ldexp(got.view(np.float64), -k).view(got.dtype)
        assert np.array_equal(back, base), (mode, int((back != base).sum()))
        with _no_fused(gdsp):
            m0, _, _ = _run(D, c["x"], c["o"], mode == "power")
            m1, _, _ = _run(D, x, c["o"], mode == "power")
        assert np.array_equal(np.ldexp(m1.view(np.float64), -k).view(m1.dtype), m0), mode


@pytest.mark.parametrize("i", [3, 17], ids=[IDS[i] for i in (3, 17)])
def test_repeated_call_and_side_stream_give_the_same_bits(gdsp, oracle, D, i):
    import torch
    c = _case(gdsp, oracle, D, i)
    for mode in MODES:
        again, _, _ = _run(D, c["x"], c["o"], mode == "power")
        assert np.array_equal(again, c["got"][mode]), mode
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        got, freqs, times = _run(D, c["x"], c["o"], mode == "power", stream=side)
        assert np.array_equal(got, c["got"][mode]), mode
        assert np.array_equal(freqs, c["freqs"]) and np.array_equal(times, c["times"])


def test_host_entries(gdsp, oracle, D):
    S = gdsp.spectral
    for i in (4, 9, 16):
        c = _case(gdsp, oracle, D, i)
        nfft, nov, pad, nsegs, n, channels = _shape(TABLE[i])
        X, fx, tx = S.StftBatch(c["x"], FS, c["o"])
        P, fp, tp = S.SpectrogramBatch(list(c["x"]), FS, c["o"])
        assert X.shape == P.shape == (channels, nsegs, pad // 2 + 1)
        assert _err(X, c["ref_o"]) < TOL and _err(X, c["got"]["complex"]) < EXACT
        assert _err(P, _power(c["ref_o"], nfft, pad)) < TOL
        assert _err(P, c["got"]["power"]) < EXACT
        for f, t in ((fx, tx), (fp, tp)):
            assert np.array_equal(f, c["freqs"]) and np.array_equal(t, c["times"])
        X1, f1, t1 = S.Stft(c["x"][-1], FS, c["o"])
        P1, _, _ = S.Spectrogram(c["x"][-1], FS, c["o"])
        assert X1.shape == (nsegs, pad // 2 + 1) and np.array_equal(t1, c["times"])
        assert _err(X1, c["ref_o"][-1]) < TOL and _err(X1, X[-1]) < EXACT
        assert _err(P1, P[-1]) < EXACT
    # the materialised form through the host staging
    nfft, nov = 100, 30
    x = _signals(9, 3, 4 * 70 + 100 + 2)
    o = CP._options(gdsp, nfft, nov, 0)
    ref_o, _ = _reference(oracle, x, nfft, nov, nfft)
    X, _, _ = S.StftBatch(x, FS, o)
    P, _, _ = S.SpectrogramBatch(x, FS, o)
    assert _err(X, ref_o) < TOL and _err(P, _power(ref_o, nfft, nfft)) < TOL


def test_short_signal_and_empty_input(gdsp, oracle, D):
    import torch
    S = gdsp.spectral
    o = S.PwelchOptions(NFFT=64)
    x = _signals(6, 3, 50)  # shorter than NFFT: zero-padded to NFFT, one segment
    ref_o, ref_n = _reference(oracle, x, 64, 0, 64)
    assert ref_o.shape == (3, 1, 33)
    for mode in MODES:
        power = mode == "power"
        got, freqs, times = _run(D, x, o, power)
        host, hf, ht = (S.SpectrogramBatch if power else S.StftBatch)(x, FS, o)
        ro, rn = (_power(ref_o, 64, 64), _power(ref_n, 64, 64)) if power else (ref_o, ref_n)
        assert got.shape == host.shape == (3, 1, 33)
        assert _err(got, ro) < TOL and _err(got, rn) < EXACT
        assert _err(host, ro) < TOL and _err(host, got) < EXACT
        assert np.array_equal(freqs, hf) and np.array_equal(times, ht)
        assert np.array_equal(times, np.array([32 / FS]))
        assert np.array_equal(freqs, oracle.pwelch(x[0], FS, nfft=64)[1])
    pw = np.stack([S.Pwelch(r, FS, o)[0] for r in x])
    assert row_nrel(S.SpectrogramBatch(x, FS, o)[0][:, 0], pw) < EXACT
    e = torch.zeros((2, 0), dtype=torch.float64, device="cuda")
    r, freqs, times = D.stft_batch(e, o)
    assert tuple(r.shape) == (2, 0, 0) and r.dtype == torch.complex128
    assert freqs.shape == (0,) and times.shape == (0,)
    r, freqs, times = D.spectrogram_batch(e, FS, o)
    assert tuple(r.shape) == (2, 0, 0) and r.dtype == torch.float64
    # no channels, and an empty segment range
    z = torch.zeros((0, 300), dtype=torch.float64, device="cuda")
    r, freqs, times = D.spectrogram_batch(z, FS, o)
    assert tuple(r.shape) == (0, 4, 33) and freqs.shape == (33,) and times.shape == (4,)
    xd = CP._strided(_signals(7, 2, 300), 3)
    r, _, times = D.stft_batch(xd, o, seg_begin=2, seg_end=2)
    assert tuple(r.shape) == (2, 0, 33) and times.shape == (0,)
    r, _, _ = S.StftBatch(np.zeros((0, 300)), FS, o)
    assert r.shape == (0, 4, 33)


def test_host_chunk_loop_past_its_first_iteration(gdsp, D):
    """The smallest host call whose output exceeds the chunk constant: F = 64
    with Noverlap = NFFT - 1 keeps the input near a million samples. The cut
    falls on an even segment, so the rows behind it are, bit for bit, those of a
    device call on the range that starts there. A rectangular window makes norm
    an exact integer, whatever the order it is summed in."""
    S = gdsp.spectral
    nfft, lp = 64, 33
    per = (S.STFT_CHUNK_ELEMS // lp) & ~1  # segments per range of a one-channel call
    assert per * lp <= S.STFT_CHUNK_ELEMS < (per + 2) * lp
    nsegs = per + 67
    n = nsegs - 1 + nfft
    o = S.PwelchOptions(NFFT=nfft, Noverlap=nfft - 1, Window=gdsp.window.Rectangular)
    assert S.stft_batch_fused(1, n, nfft, 0, nfft - 1)
    x = np.random.default_rng(12).standard_normal((1, n))
    before = gdsp.fft.LoopStats()
    P, freqs, times = S.SpectrogramBatch(x, FS, o)
    after = gdsp.fft.LoopStats()
    assert after["later_chunks"] - before["later_chunks"] >= 1
    assert P.shape == (1, nsegs, lp) and times[-1] == (nsegs - 1 + nfft / 2) / FS
    rows = list(range(per - 64, per + 64)) + [nsegs - 1]
    segs = np.stack([x[0, s:s + nfft] for s in rows])
    ref = _power(np.fft.fft(segs, axis=1)[:, :lp], nfft, nfft, window=np.ones(nfft))
    err = row_nrel(P[0, rows], ref)
    print("host chunks", err)
    assert err < EXACT
    tail, _, _ = D.spectrogram_batch(CP._strided(x, 3), FS, o, seg_begin=per, seg_end=nsegs)
    assert np.array_equal(tail.cpu().numpy()[0], P[0, per:])


def test_workers_with_several_groups(gdsp, D):
    """2048 channels share the kernel's 2048 workers one each, and 35 segments at
    F = 64 are two groups of 16 pairs: every worker runs a full group and a
    masked one."""
    nfft, nov, channels, nsegs = 64, 32, 2048, 35
    n = (nsegs - 1) * (nfft - nov) + nfft
    x = np.random.default_rng(13).standard_normal((channels, n))
    o = CP._options(gdsp, nfft, nov, 0)
    import torch
    xd = torch.from_numpy(x).cuda()
    before = gdsp.fft.LoopStats()
    P, _, _ = D.spectrogram_batch(xd, FS, o)
    torch.cuda.synchronize()
    after = gdsp.fft.LoopStats()
    assert after["multi_unit_launches"] - before["multi_unit_launches"] >= 1
    w = np.asarray(gdsp.window.Hann(nfft))
    segs = np.stack([x[:, s * 32:s * 32 + nfft] for s in range(nsegs)], axis=1)
    ref = _power(np.fft.fft(segs * w, axis=2)[:, :, :33], nfft, nfft)
    got = _flat(P.cpu().numpy())
    ref = _flat(ref)
    d = got - ref
    err = max(float((np.linalg.norm(d, axis=1) / np.linalg.norm(ref, axis=1)).max()),
              float((np.abs(d).max(axis=1) / np.abs(ref).max(axis=1)).max()))
    print("several groups", err)
    assert err < EXACT


def test_wav_spectrogram_of_channels(gdsp, oracle):
    W = gdsp.wav
    frames, channels = 5000, 3
    rng = np.random.default_rng(17)
    sig = rng.standard_normal((channels, frames)) * np.array([[1.0], [0.3], [2.0]])
    pcm = np.clip(np.round(sig * 4000.0), -32768, 32767).astype("<i2")
    data = np.ascontiguousarray(pcm.T).tobytes()  # interleaved frames
    want = oracle.wav_floats(data, frames * channels, 1, 16).astype(np.float64)
    rows = np.stack([want[c::channels] for c in range(channels)])
    o = gdsp.spectral.PwelchOptions(NFFT=256, Noverlap=128)
    w = W.New(io.BytesIO(CP._wav(1, 16, channels, data)))
    assert w.NumChannels == channels
    P, freqs, times = W.SpectrogramChannels(w, frames, o)
    ref_o, _ = _reference(oracle, rows, 256, 128, 256)
    nsegs = ref_o.shape[1]
    assert P.shape == (channels, nsegs, 129)
    err = _err(P, _power(ref_o, 256, 256, fs=44100.0))
    print("wav", err)
    assert err < TOL
    assert np.array_equal(freqs, oracle.pwelch(rows[0], 44100.0, nfft=256, noverlap=128)[1])
    assert np.array_equal(times, (np.arange(nsegs) * 128 + 128.0) / 44100.0)
    pw, _ = W.PwelchChannels(W.New(io.BytesIO(CP._wav(1, 16, channels, data))), frames, o)
    assert row_nrel(P.mean(axis=1), pw) < EXACT
    e = W.SpectrogramChannels(W.New(io.BytesIO(CP._wav(1, 16, channels, data))), 0, o)
    assert e[0].shape == (channels, 0, 0) and e[1].shape == (0,) and e[2].shape == (0,)
