"""GPU checks of the chirp-z transform (gdsp_czt_batch, the plan object and
gdsp_czt_batch_device): the fused kernel over its sizes and the composed form
over its own, through both entries.

Accuracy: exact_dft.err_u against the 80-bit Bluestein of czt_ref.py (every
angle reduced in integers), bounded by exact_dft.check with the project's
MARGIN against the float64 statement of the same factorisation on the same
rows in the same run; no other number is fixed. A kernel whose chirp angle is
not reduced, or reduced in float64, lands at 1e4 to 1e8 u and fails.

Shapes: the smallest that reach each way the kernel can go wrong. F = 256 runs
16 rows per workgroup (ragged at 5 and 33 rows), 4096 is the last size with 16
elements per thread, 8192 the first with 32, 16384 the largest fused size (its
postmultiplier follows the transform instead of riding its last pass); every
fused F is hit at n + m - 1 = F (the alias edge) and at F / 2 + 1. (8192, 8194)
and (20000, 5000) are above the fused range; every fused shape runs again under
GDSP_ALGO_NO_FUSED_CZT.

Values: row independence bit for bit, zeros, containment, scaling and history
with the helpers of values.py. Layout: strides above the row lengths with NaN
in the gaps, guard bands (guarded.py), no allocation with out and work given,
a plan across calls and streams. Paths: the flag, the host entry's second row
range, the composed form's second chunk.
"""
import gc
import importlib
import os

import numpy as np
import pytest

import czt_ref as R
import exact_dft as E
import values as V
from conftest import GOLDEN
from guarded import GUARD, NAN, guarded, pad_for

pytestmark = pytest.mark.gpu

# (n, m) -> F
FUSED = [(128, 129), (1, 1), (2, 255), (255, 2), (2048, 2049), (3000, 1000), (4097, 4096),
         (8192, 8193)]
HALF = [(65, 65), (1025, 1025), (2049, 2049), (4097, 4097)]   # n + m - 1 = F / 2 + 1
COMPOSED = [(8192, 8194), (20000, 5000)]

PARAMS = {
    "dft": dict(),
    "zoom": dict(zoom=([0.1234, 0.2345], 2, False)),
    "zoom-endpoint": dict(zoom=([0.1234, 0.2345], 2, True)),
    "step0.37": dict(step_turns=0.37, step_div=1),
    "a0.999": dict(a_abs=0.999, step_turns=0.3, step_div=401, a_turns=0.05),
}


def _kw(name, m):
    p = dict(PARAMS[name])
    if "zoom" in p:
        fn, fs, endpoint = p.pop("zoom")
        at, st, sd = R.zoom_params(fn, m, fs, endpoint)
        p.update(a_turns=at, step_turns=st, step_div=sd)
    return p


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


class Flag:
    """ALGO_NO_FUSED_CZT for the block (composed=True), the path asserted."""

    def __init__(self, gdsp, composed, n, m):
        self.F, self.composed, self.n, self.m = gdsp.fft, composed, n, m

    def __enter__(self):
        F = self.F
        self.prev = F.Algorithm()
        F.SetAlgorithm(self.prev | F.ALGO_NO_FUSED_CZT if self.composed
                       else self.prev & ~F.ALGO_NO_FUSED_CZT)
        length = max(256, E._next_pow2(self.n + self.m - 1))
        assert F.czt_length(self.n, self.m) == (length, length <= 16384 and not self.composed)
        assert F.czt_fused(self.n, self.m) == (length <= 16384 and not self.composed)

    def __exit__(self, *a):
        self.F.SetAlgorithm(self.prev)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_plans: dict = {}


def _plan(D, n, m, kw):
    key = (n, m, tuple(sorted(kw.items())))
    if key not in _plans:
        _plans[key] = D.CztPlan(n, m, **kw)
    return _plans[key]


def _run(D, x, m, kw=None, pad=0, fill=None, stream=None):
    """device.czt_batch on rows ldx = n + pad apart (NaN in the gaps) into rows
    ldo = m + pad apart inside guard bands; fill: what out and a work buffer of
    exactly the stated size hold before. The plan says which form ran."""
    import torch
    x = np.atleast_2d(x)
    rows, n = x.shape
    kw = kw or {}
    plan = _plan(D, n, m, kw)
    wide = np.full((rows, n + pad), complex(NAN, NAN) if np.iscomplexobj(x) else NAN)
    wide[:, :n] = x
    xd = _dev(wide)[:, :n]
    sentinel = GUARD if fill is None else fill
    payload = torch.full((rows, m + pad), sentinel, dtype=torch.complex128, device="cuda")
    out, check = guarded(payload, sentinel, pad_for(m + pad))
    work = None
    if fill is not None and plan.work_bytes(rows):
        work = torch.full((plan.work_bytes(rows) // 8,), fill, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # the fills ran on the default stream
    got = D.czt_batch(xd, plan, out=out[:, :m], work=work, stream=stream)
    torch.cuda.synchronize()
    check("czt n=%d m=%d rows=%d" % (n, m, rows))
    if pad:
        gap = out[:, m:].cpu().numpy()
        assert np.array_equal(gap.view(np.float64), np.full_like(gap, sentinel).view(np.float64),
                              equal_nan=True), "a store between the rows"
    return got.cpu().numpy()


_refs: dict = {}


def _ref(n, m, name, real):
    """(inputs, 80-bit result, err_u of the float64 route) of the standard rows
    (real: their real parts), computed once per shape and parameter set."""
    key = (n, m, name, real)
    if key not in _refs:
        x = E.standard_rows(n)
        x = np.ascontiguousarray(x.real if real else x)
        kw = _kw(name, m)
        ex = R.czt_exact(x, m, **kw)
        ex.setflags(write=False)
        _refs[key] = (x, ex, E.err_u(R.czt_float64(x, m, **kw), ex))
    return _refs[key]


def _accuracy(gdsp, D, n, m, name, forms):
    kw = _kw(name, m)
    got = {}
    for real in (False, True):
        x, ex, e_ref = _ref(n, m, name, real)
        for composed in forms:
            with Flag(gdsp, composed, n, m):
                fused = gdsp.fft.czt_fused(n, m)
                y = _run(D, x, m, kw, pad=3)
            variant = "%s m=%d %s %s" % (name, m, "real" if real else "complex",
                                         "fused" if fused else "composed")
            E.check("czt", n, variant, E.err_u(y, ex), e_ref)
            got[(real, composed)] = y
        if name == "dft" and n == m:
            xf = E.exact_fft(x)
            assert E.err_u(ex, xf) < 0.25  # the reference itself
            for composed in forms:
                E.check("czt", n, "dft against exact_fft " + ("real" if real else "complex"),
                        E.err_u(got[(real, composed)], xf), e_ref)
    return got


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("n,m", FUSED, ids=["%dx%d" % s for s in FUSED])
def test_accuracy_fused_and_under_the_flag(gdsp, D, n, m, name):
    got = _accuracy(gdsp, D, n, m, name, (False, True))
    # the two forms agree within the sum of their bounds
    for real in (False, True):
        _, ex, e_ref = _ref(n, m, name, real)
        d = np.abs(got[(real, False)].astype(E.CLD) - got[(real, True)]).max(axis=1) \
            / np.abs(ex).max(axis=1)
        assert float(d.max() / E.LD(E.U)) <= 2 * E.MARGIN * e_ref


@pytest.mark.parametrize("n,m", HALF, ids=["%dx%d" % s for s in HALF])
def test_accuracy_at_half_the_length_plus_one(gdsp, D, n, m):
    _accuracy(gdsp, D, n, m, "dft", (False, True))


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("n,m", COMPOSED, ids=["%dx%d" % s for s in COMPOSED])
def test_accuracy_above_the_fused_range(gdsp, D, n, m, name):
    assert not gdsp.fft.czt_fused(n, m)
    _accuracy(gdsp, D, n, m, name, (False,))


# ---- values ------------------------------------------------------------------------

VALUE_SHAPES = [(128, 129, False), (3000, 1000, False), (4097, 4096, False),
                (8192, 8193, False), (128, 129, True), (8192, 8194, False)]
_vid = ["%dx%d%s" % (n, m, "-flag" if c else "") for n, m, c in VALUE_SHAPES]
ZOOM = dict(a_turns=0.0617, step_turns=0.05555, step_div=1009)


def _rows(seed, rows, n, real):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (rows, n))
    if not real:
        x = x + 1j * rng.uniform(-1, 1, (rows, n))
    return x * (10.0 ** (np.arange(rows) % 4))[:, None]


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("n,m,composed", VALUE_SHAPES, ids=_vid)
def test_rows_are_independent_bit_for_bit(gdsp, D, n, m, composed, real):
    """A row's output is the same alone or among others, at 1, 2, 5 and 33
    rows, on the device entry and through the host entry; a zero row gives
    zeros."""
    x = _rows(n + m, 33, n, real)
    x[7] = 0.0
    with Flag(gdsp, composed, n, m):
        full = _run(D, x, m, ZOOM, pad=5)
        assert np.isfinite(full.view(np.float64)).all()
        assert np.all(full[7] == 0)
        for r in (1, 2, 5):
            assert np.array_equal(_run(D, x[:r], m, ZOOM), full[:r]), r
        for r in (4, 17, 32):
            assert np.array_equal(_run(D, x[r:r + 1], m, ZOOM)[0], full[r]), r
        assert np.array_equal(_run(D, x[[32, 3, 7]], m, ZOOM, pad=1), full[[32, 3, 7]])
        host = gdsp.fft.CZTBatch(x, m, ZOOM["step_turns"], ZOOM["step_div"], ZOOM["a_turns"])
        assert np.array_equal(host, full)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("n,m,composed", VALUE_SHAPES, ids=_vid)
def test_bad_samples_stay_in_their_row(gdsp, D, n, m, composed, real):
    """A NaN or an Inf sample makes all m outputs of its row non-finite, in
    both parts, and changes no bit of any other row."""
    rows = 18
    x = _rows(n + 2 * m, rows, n, real)
    with Flag(gdsp, composed, n, m):
        clean = _run(D, x, m, ZOOM)
        for name, value, _ in V.bad_values(not real):
            for r, i in ((0, 0), (rows - 1, (2 * n // 3) | 1 if n > 2 else n - 1), (16, n - 1)):
                got = _run(D, V.with_sample(x, (r, i), value), m, ZOOM)
                what = "%s at [%d, %d]" % (name, r, i)
                V.check_contained((got,), (clean,), [V.rows_mask(clean.shape, [r])], what)
                assert (~np.isfinite(got[r].real) & ~np.isfinite(got[r].imag)).all(), what


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("n,m,composed", VALUE_SHAPES, ids=_vid)
def test_scaling_and_stale_buffers(gdsp, D, n, m, composed, real):
    """Inputs times 2^k give outputs times 2^k exactly; what out and work held
    before, NaN included, changes nothing."""
    x = _rows(3 * n + m, 5, n, real)
    nan = np.full((11, n), NAN if real else complex(NAN, NAN))
    with Flag(gdsp, composed, n, m):
        def run(inputs, fill):
            return (_run(D, inputs[0], m, ZOOM, pad=2, fill=fill),)

        V.check_equivariant(run, (x,), (((200,), (200,)), ((-200,), (-200,))), "czt")
        V.check_history(run, (x,), (nan,), "czt")


# ---- layout --------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,composed", [(600, 425, False), (600, 425, True)])
def test_no_allocation_with_out_and_work_given(gdsp, D, n, m, composed):
    import torch
    x = _dev(_rows(n, 6, n, True))
    with Flag(gdsp, composed, n, m):
        plan = D.CztPlan(n, m, **ZOOM)
        assert plan.fused == (not composed) and plan.F == 1024
        assert plan.work_bytes(6) == (6 * 1024 * 16 if composed else 0)
        out = torch.empty((6, m), dtype=torch.complex128, device="cuda")
        work = torch.empty(6 * 1024 * 2, dtype=torch.float64, device="cuda")
        D.czt_batch(x, plan, out=out, work=work)  # the F-point plan's own first use
        torch.cuda.synchronize()
        gc.collect()
        before = torch.cuda.memory_allocated()
        got = D.czt_batch(x, plan, out=out, work=work)
        assert torch.cuda.memory_allocated() == before
        assert got is out
        torch.cuda.synchronize()
        if composed:  # a work buffer below the stated size is refused
            with pytest.raises(gdsp.GDSPError) as e:
                D.czt_batch(x, plan, out=out, work=work[:-2])
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID


def test_plan_is_reused_across_calls_and_streams(gdsp, D):
    import torch
    n, m = 3000, 1000
    x = _rows(9, 7, n, False)
    with Flag(gdsp, False, n, m):
        first = _run(D, x, m, ZOOM)
        handle = _plan(D, n, m, ZOOM).handle.value
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a = _run(D, x, m, ZOOM, stream=s1)
        b = _run(D, x[:3], m, ZOOM, stream=s2)
        assert np.array_equal(a, first) and np.array_equal(b, first[:3])
        assert np.array_equal(_run(D, x, m, ZOOM), first)
        assert _plan(D, n, m, ZOOM).handle.value == handle


def test_device_entry_rejects_overlap(gdsp, D):
    import torch
    plan = D.CztPlan(256, 128, **ZOOM)
    buf = torch.zeros(4096, dtype=torch.complex128, device="cuda")
    x = buf[:512].view(2, 256)
    for out in (buf[:256].view(2, 128), buf[500:756].view(2, 128)):
        with pytest.raises(gdsp.GDSPError) as e:
            D.czt_batch(x, plan, out=out)
        assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    D.czt_batch(x, plan, out=buf[512:768].view(2, 128))
    torch.cuda.synchronize()


# ---- paths reached -------------------------------------------------------------------

def test_host_call_crosses_a_row_range(gdsp, D):
    """2^24 div F rows a range: 1024 of F = 16384, so 1026 rows take a second
    range of two. One row per transform: the bits are those of one device call
    over all rows."""
    F = gdsp.fft
    n, m, rows = 8192, 8193, 1026
    x = np.random.default_rng(5).uniform(-1, 1, (rows, n))
    with Flag(gdsp, False, n, m):
        before = F.LoopStats()["later_chunks"]
        got = F.CZTBatch(x, m, ZOOM["step_turns"], ZOOM["step_div"], ZOOM["a_turns"])
        assert F.LoopStats()["later_chunks"] - before == 1
        before = F.LoopStats()["later_chunks"]
        F.CZTBatch(x[:1024], m, ZOOM["step_turns"], ZOOM["step_div"], ZOOM["a_turns"])
        assert F.LoopStats()["later_chunks"] == before
        assert np.array_equal(got, _run(D, x, m, ZOOM))


def test_composed_form_crosses_a_chunk(gdsp, D):
    """The composed form's chunks are 2^24 div F rows: 512 of F = 32768, so 514
    rows run a second chunk of two, with the bits they have in a call of their
    own."""
    F = gdsp.fft
    n, m, rows = 8192, 8194, 514
    x = np.random.default_rng(6).uniform(-1, 1, (rows, n))
    before = F.LoopStats()["later_chunks"]
    got = _run(D, x, m, ZOOM)
    assert F.LoopStats()["later_chunks"] - before == 1
    assert np.array_equal(got[512:], _run(D, x[512:], m, ZOOM))
    assert np.array_equal(got[:3], _run(D, x[:3], m, ZOOM))


# ---- the wrappers ---------------------------------------------------------------------

def test_python_wrappers_and_a_tone_between_bins(gdsp, D):
    F = gdsp.fft
    n, fs = 1000, 8000.0
    f0 = 1234.5678  # between the DFT bins 154 and 155 (8 Hz apart)
    t = np.arange(n)
    x = np.cos(2 * np.pi * f0 / fs * t) + 0.01 * np.random.default_rng(1).uniform(-1, 1, n)
    fn, m = [1200.0, 1260.0], 601
    z = F.ZoomFFT(x, fn, m, fs=fs, endpoint=True)
    freqs = F.zoom_freqs(fn, m, fs=fs, endpoint=True)
    assert abs(freqs[np.argmax(np.abs(z))] - f0) <= 0.1 + 1e-9      # the grid is 0.1 Hz
    at, st, sd = R.zoom_params(fn, m, fs, True)
    ex = R.czt_exact(x, m, st, sd, at)
    e_ref = E.err_u(R.czt_float64(x, m, st, sd, at), ex)
    E.check("czt", n, "ZoomFFT", E.err_u(z, ex), e_ref)
    assert np.array_equal(F.ZoomFFTBatch(np.stack([x, 2 * x]), fn, m, fs, True)[1], 2 * z)
    assert np.array_equal(F.CZT(x, m, st, sd, at), z)
    # the default is the DFT
    xc = E.standard_rows(300)[0]
    E.check("czt", 300, "CZT default", E.err_u(F.CZT(xc), E.exact_fft(xc[None, :])),
            E.err_u(R.czt_float64(xc), E.exact_fft(xc[None, :])))
    # the device wrappers
    xd = _dev(np.stack([x, 2 * x]))
    assert np.array_equal(D.zoom_fft_batch(xd, fn, m, fs, True).cpu().numpy()[0], z)
    plan = D.CztPlan(n, m, st, sd, at)
    assert (plan.n, plan.m, plan.F, plan.fused) == (n, m, 2048, True)
    assert np.array_equal(D.czt_batch(xd, plan).cpu().numpy()[1], 2 * z)


def test_wav_zoom_channels(gdsp):
    W, F = gdsp.wav, gdsp.fft
    path = os.path.join(GOLDEN, "wav", "small.wav")
    with open(path, "rb") as f:
        w = W.New(f)
        C, rate = w.NumChannels, float(w.SampleRate)
        frames = min(w.Samples // C, 5000)
        dec = w.ReadFloats(frames * C).astype(np.float64)
    chans = np.stack([dec[c::C] for c in range(C)])
    fn = [0.05 * rate, 0.07 * rate]
    for m in (None, 700):
        with open(path, "rb") as f:
            got = W.ZoomChannels(W.New(f), frames, fn, m)
        assert got.shape == (C, m or frames)
        assert np.array_equal(got, F.ZoomFFTBatch(chans, fn, m or frames, rate))
