"""GPU checks of polyphase resampling (gdsp_upfirdn_batch,
gdsp_upfirdn_batch_device, ResamplePoly): the fused kernel over its shapes and
the plain form as a second opinion and beyond them, strides and stray writes,
output ranges, rows that must not see each other, scaling and non-finite
samples, the resample_poly composition, the host chunk loop and the wav entry.

The reference is the definition in np.longdouble rounded to float64
(resample_ref.upfirdn: zero-stuff, np.convolve, slice), compared with
conftest.row_nrel at test_fir_gpu.EXACT = 1e-13, the bound FIR is held to. A
float64 numpy model of the polyphase sum stays at or below 1.9e-15 on every
shape below: a failure is a bug, not roundoff."""
import contextlib
import importlib
import os

import numpy as np
import pytest

import resample_ref as R
from conftest import GOLDEN, row_nrel
from guarded import GUARD, guarded
from test_fir_gpu import EXACT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


@contextlib.contextmanager
def _plain(gdsp):
    """The plain form: the fused kernel switched off for the calls inside."""
    F = gdsp.fft
    prev = F.Algorithm()
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_UPFIRDN)
    try:
        yield
    finally:
        F.SetAlgorithm(prev)


def _form(gdsp, plain):
    return _plain(gdsp) if plain else contextlib.nullcontext()


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _run(D, x, h, up, down, **kw):
    import torch
    out = D.upfirdn_batch(_cuda(x), _cuda(h), up, down, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# (up, down, m, n, fused)
SHAPES = [(1, 1, 1, 5, True),            # identity
          (1, 2, 3, 9, True),            # decimation
          (2, 1, 4, 7, True),            # interpolation
          (3, 2, 7, 50, True),           # rational ratio
          (8, 1, 3, 20, True),           # phases 3-7 have no tap
          (1, 50, 3, 400, False),        # samples no output reads; a tile's span beyond the LDS
          (5, 7, 200, 3, True),          # n < T
          (7, 3, 64, 1, True),           # one sample
          (160, 147, 3218, 3000, True),  # audio rate pair, T = 21
          (147, 160, 3361, 3000, True),  # audio rate pair, T = 23
          (1, 4, 1001, 1500, True),      # T beyond any register block
          (1, 16, 337, 70000, True),     # lane stride 16, several tiles, last one partial
          (4, 1, 81, 20000, True),       # several tiles
          (1024, 1023, 9000, 40, False)]  # table beyond the fused budget: plain only


@pytest.mark.parametrize("up,down,m,n,fused", SHAPES,
                         ids=["%d-%d-%d-%d" % s[:4] for s in SHAPES])
def test_definition(gdsp, D, up, down, m, n, fused):
    F = gdsp.fft
    x, h, ref = R.case(up + down + m + n, 3, n, m, up, down)
    L = F.upfirdn_length(n, m, up, down)
    assert ref.shape == (3, L)
    assert F.upfirdn_fused(m, up, down) == fused
    got = _run(D, x, h, up, down)
    with _plain(gdsp):
        assert not F.upfirdn_fused(m, up, down)
        plain = _run(D, x, h, up, down)
    assert F.upfirdn_fused(m, up, down) == fused
    assert got.shape == plain.shape == (3, L)
    e1, e2 = row_nrel(got, ref), row_nrel(plain, ref)
    print(f"{up}/{down} m={m} n={n}: default {e1:.3e} plain {e2:.3e}")
    assert e1 < EXACT and e2 < EXACT
    # one fused multiply-add per term in ascending t in both forms
    assert _same_bits(got, plain)
    if (up, m) == (8, 3):
        idle = (np.arange(L) * down) % up >= m
        assert idle.sum() == L - 3 * n
        for o in (got, plain):
            assert np.all(o[:, idle] == 0.0) and not np.any(np.signbit(o[:, idle]))


@pytest.mark.parametrize("plain", [False, True], ids=["fused", "plain"])
def test_strides_and_stray_writes(gdsp, D, plain):
    """x is a row-strided view, out a view into a sentinel-filled buffer whose
    padding columns and guard row keep their bits; an exact-size work buffer
    between guard bands stays intact."""
    import torch
    channels, up, down, m, n = 17, 3, 2, 7, 300
    x, h, ref = R.case(2000, channels, n, m, up, down)
    L = ref.shape[1]
    xb = torch.full((channels, n + 5), 3.5, dtype=torch.float64, device="cuda")
    xb[:, :n] = _cuda(x)
    ob = torch.full((channels + 1, L + 3), GUARD, dtype=torch.float64, device="cuda")
    xv, ov = xb[:, :n], ob[:channels, :L]
    assert xv.stride(0) == n + 5 and ov.stride(0) == L + 3
    T = -(-m // up)
    work, check = guarded(torch.zeros(up * T, dtype=torch.float64, device="cuda"), GUARD, 1024)
    with _form(gdsp, plain):
        assert gdsp.fft.upfirdn_fused(m, up, down) == (not plain)
        got = D.upfirdn_batch(xv, _cuda(h), up, down, out=ov, work=work)
        torch.cuda.synchronize()
    assert got is ov
    o = ob.cpu().numpy()
    assert row_nrel(o[:channels, :L], ref) < EXACT
    assert np.all(o[:, L:] == GUARD) and np.all(o[channels] == GUARD)
    check("work")
    # the phase-major taps, as the header describes the scratch
    want = np.zeros(up * T)
    for k in range(m):
        want[(k % up) * T + k // up] = h[k]
    assert np.array_equal(work.cpu().numpy(), want)


@pytest.mark.parametrize("plain", [False, True], ids=["fused", "plain"])
@pytest.mark.parametrize("up,down,m,n,cuts", [(160, 147, 3218, 3000, (777, 2603)),
                                              (1, 16, 337, 70000, (301, 3001))],
                         ids=["160-147", "1-16"])
def test_ranges(gdsp, D, up, down, m, n, cuts, plain):
    """[0, L) cut at two odd points that are no tile boundaries: the first
    range's window starts before sample 0, the last one's ends past n."""
    x, h, ref = R.case(up + down + m + n, 3, n, m, up, down)
    L = ref.shape[1]
    a, b = cuts
    assert 0 < a < b < L and a % 256 and b % 256
    assert -(-m // up) > 1                # output 0 reads samples before the row
    assert (L - 1) * down // up >= n      # the last window reaches past the row
    with _form(gdsp, plain):
        whole = _run(D, x, h, up, down)
        parts = [_run(D, x, h, up, down, out_begin=lo, out_end=hi)
                 for lo, hi in ((0, a), (a, b), (b, L))]
    assert [p.shape[1] for p in parts] == [a, b - a, L - b]
    assert _same_bits(np.concatenate(parts, axis=1), whole)
    assert row_nrel(whole, ref) < EXACT


@pytest.mark.parametrize("plain", [False, True], ids=["fused", "plain"])
@pytest.mark.parametrize("up,down,m,n", [(3, 2, 7, 300), (160, 147, 3218, 3000)],
                         ids=["3-2", "160-147"])
def test_rows_alone(gdsp, D, up, down, m, n, plain):
    rng = np.random.default_rng(77)
    x, h = rng.standard_normal((5, n)), rng.standard_normal(m)
    with _form(gdsp, plain):
        got = _run(D, x, h, up, down)
        for c in range(5):
            assert _same_bits(got[c:c + 1], _run(D, x[c:c + 1], h, up, down)), c


VALUE_SHAPES = [(3, 2, 7, 50), (160, 147, 3218, 3000)]


@pytest.mark.parametrize("plain", [False, True], ids=["fused", "plain"])
@pytest.mark.parametrize("up,down,m,n", VALUE_SHAPES, ids=["3-2", "160-147"])
def test_scaling_zeros_and_stale_buffers(gdsp, D, up, down, m, n, plain):
    import torch
    x, h, ref = R.case(up + down + m + n, 3, n, m, up, down)
    L = ref.shape[1]
    T = -(-m // up)
    with _form(gdsp, plain):
        clean = _run(D, x, h, up, down)
        for a, b in ((7, -3), (-40, 12), (100, 100)):
            got = _run(D, x * 2.0 ** a, h * 2.0 ** b, up, down)
            assert _same_bits(got, clean * 2.0 ** (a + b)), (a, b)
        zeros = _run(D, np.zeros_like(x), h, up, down)
        assert np.all(zeros == 0.0)
        out = torch.full((3, L), float("nan"), dtype=torch.float64, device="cuda")
        work = torch.full((up * T,), float("nan"), dtype=torch.float64, device="cuda")
        assert _same_bits(_run(D, x, h, up, down, out=out, work=work), clean)
    assert row_nrel(clean, ref) < EXACT


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("plain", [False, True], ids=["fused", "plain"])
@pytest.mark.parametrize("up,down,m,n", VALUE_SHAPES, ids=["3-2", "160-147"])
def test_non_finite_sample(gdsp, D, up, down, m, n, plain, bad):
    x, h, _ = R.case(up + down + m + n, 3, n, m, up, down)
    L = gdsp.fft.upfirdn_length(n, m, up, down)
    T = -(-m // up)
    c, i = 1, n // 3
    xb = np.array(x)
    xb[c, i] = bad
    with _form(gdsp, plain):
        clean = _run(D, x, h, up, down)
        got = _run(D, xb, h, up, down)
    k = np.arange(L) * down - i * up
    must = (k >= 0) & (k < m)
    may = (k >= 0) & (k < T * up)
    assert must.any() and (~may).any()
    assert not np.any(np.isfinite(got[c, must]))
    assert np.all(np.isfinite(got[c, ~may]))
    assert _same_bits(got[c, ~may], clean[c, ~may])
    for r in (0, 2):
        assert _same_bits(got[r], clean[r]), r


RATIOS = ((160, 147), (147, 160), (1, 8), (3, 1), (2, 3), (48, 44))


def _poly_case(up, down):
    rng = np.random.default_rng(up * 1000 + down)
    return rng.standard_normal((3, 1000))


@pytest.mark.parametrize("up,down", RATIOS, ids=["%d-%d" % r for r in RATIOS])
def test_resample_poly(gdsp, D, up, down):
    import torch
    F = gdsp.fft
    x = _poly_case(up, down)
    ref = R.resample_poly(x, up, down)
    assert ref.shape == (3, -(-1000 * up // down))
    dev = D.resample_poly_batch(_cuda(x), up, down)
    torch.cuda.synchronize()
    dev = dev.cpu().numpy()
    host = F.ResamplePolyBatch(x, up, down)
    e1, e2 = row_nrel(dev, ref), row_nrel(host, ref)
    print(f"{up}/{down}: device {e1:.3e} host {e2:.3e}")
    assert dev.shape == host.shape == ref.shape
    assert e1 < EXACT and e2 < EXACT
    assert _same_bits(dev, host)
    assert _same_bits(F.ResamplePoly(x[1], up, down), host[1])


@pytest.mark.parametrize("up,down", RATIOS, ids=["%d-%d" % r for r in RATIOS])
def test_resample_poly_against_scipy(gdsp, D, up, down):
    ss = pytest.importorskip("scipy.signal")
    x = _poly_case(up, down)
    want = ss.resample_poly(x, up, down, axis=1)
    got = gdsp.fft.ResamplePolyBatch(x, up, down)
    err = row_nrel(got, want)
    print(f"{up}/{down}: {err:.3e}")
    assert got.shape == want.shape and err < EXACT


def test_resample_poly_with_given_taps(gdsp, D):
    import torch
    F = gdsp.fft
    rng = np.random.default_rng(9)
    x, taps = rng.standard_normal((3, 1000)), rng.standard_normal(42)
    for up, down in ((3, 2), (1, 5), (7, 1), (6, 4)):
        u, d, pre, post, rem, n_out = R.plan(1000, 42, up, down)
        hh = np.concatenate([np.zeros(pre), taps, np.zeros(post)])
        want = F.UpfirdnBatch(x, hh, u, d, rem, rem + n_out)
        assert want.shape == (3, n_out)
        assert _same_bits(F.ResamplePolyBatch(x, up, down, taps=taps), want)
        for t in (taps, _cuda(taps)):
            got = D.resample_poly_batch(_cuda(x), up, down, taps=t)
            torch.cuda.synchronize()
            assert _same_bits(got.cpu().numpy(), want)
        assert row_nrel(want, R.resample_poly(x, up, down, taps)) < EXACT
    same = D.resample_poly_batch(_cuda(x), 5, 5)
    assert _same_bits(same.cpu().numpy(), x)


def test_host_chunk_loop(gdsp, D):
    """One row past UPFIRDN_CHUNK_ELEMS = 2^25 outputs: the host entry cuts the
    job once; the outputs around the cut are those of a device call whose range
    does not cut there."""
    import torch
    F = gdsp.fft
    cut, m = 1 << 25, 5
    n = cut + 1000
    rng = np.random.default_rng(123)
    x = rng.standard_normal(n).reshape(1, n)
    h = rng.standard_normal(m)
    before = F.LoopStats()["later_chunks"]
    got = F.UpfirdnBatch(x, h, 1, 1)
    assert F.LoopStats()["later_chunks"] - before == 1
    L = n + m - 1
    assert got.shape == (1, L)
    for lo, hi in ((0, 3000), (cut - 2000, cut + 1000), (L - 3000, L)):
        a = max(lo - (m - 1), 0)
        full = R.upfirdn(x[:, a:min(hi, n)], h, 1, 1)   # outputs a ... of the job
        want = full[:, lo - a:hi - a]
        assert want.shape == (1, hi - lo)
        assert row_nrel(got[:, lo:hi], want) < EXACT, (lo, hi)
    dev = D.upfirdn_batch(_cuda(x), _cuda(h), 1, 1, out_begin=cut - 2000, out_end=cut + 1000)
    torch.cuda.synchronize()
    assert _same_bits(dev.cpu().numpy(), got[:, cut - 2000:cut + 1000])


def test_wav_resample_channels(gdsp):
    W, F = gdsp.wav, gdsp.fft
    path = os.path.join(GOLDEN, "wav", "small.wav")
    with open(path, "rb") as f:
        w = W.New(f)
        C, rate = w.NumChannels, w.SampleRate
        frames = min(w.Samples // C, 20000)
        dec = w.ReadFloats(frames * C).astype(np.float64)
    chans = np.stack([dec[c::C] for c in range(C)])
    assert rate != 48000
    with open(path, "rb") as f:
        got = W.ResampleChannels(W.New(f), frames, 48000)
    want = F.ResamplePolyBatch(chans, 48000, rate)
    assert got.shape == want.shape == (C, -(-frames * 48000 // rate))
    assert _same_bits(got, want)
    assert row_nrel(got, R.resample_poly(chans, 48000, rate)) < EXACT


def test_device_entry_refuses_in_place(gdsp, D):
    import torch
    x = torch.zeros((2, 1000), dtype=torch.float64, device="cuda")
    h = torch.ones(1, dtype=torch.float64, device="cuda")
    with pytest.raises(gdsp.GDSPError) as e:
        D.upfirdn_batch(x, h, 1, 1, out=x)
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
