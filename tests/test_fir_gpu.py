"""GPU checks of FIR filtering (gdsp_fir_batch, gdsp_fir_batch_device): the
fused overlap-save kernel over its block lengths, the composed form beyond
them and as a second opinion, strides and empty workgroup slots, taps per row,
rows that must not see each other, exact cases, the default block, a chunked
stream, and the host and wav entries.

The reference is np.convolve on np.longdouble copies, rounded to float64; the
measures are conftest.row_nrel (normwise, and max|err| / max|row|), both below
the 1e-13 the fused convolution is held to. A numpy model of this scheme
(paired blocks, float64 FFT) stays at <= 5.2e-16 normwise and <= 5.6e-16
elementwise on every shape below: a failure is a bug, not roundoff."""
import functools
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, row_nrel

pytestmark = pytest.mark.gpu

EXACT = 1e-13  # the bound test_convolve_batch_gpu.py holds the fused convolution to


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


def _gauss(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape)


def _ref(x, h, full):
    """np.convolve per row in extended precision, rounded to float64."""
    x, h = np.atleast_2d(x), np.asarray(h)
    n = x.shape[1]
    rows = []
    for c in range(x.shape[0]):
        hc = h if h.ndim == 1 else h[c]
        y = np.convolve(x[c].astype(np.longdouble), hc.astype(np.longdouble))
        rows.append((y if full else y[:n]).astype(np.float64))
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def _case(seed, channels, n, m):
    """Gaussian rows and taps with their full reference, computed once."""
    x, h = _gauss(seed, channels, n), _gauss(seed + 1, m)
    ref = _ref(x, h, True)
    for a in (x, h, ref):
        a.setflags(write=False)
    return x, h, ref


def _run(D, x, h, full=False, block=0, **kw):
    import torch
    out = D.fir_batch(torch.from_numpy(np.array(x)).cuda(),
                      torch.from_numpy(np.array(h)).cuda(), full=full, block=block,
                      **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


FUSED = [(256, 1, 700),        # no halo, L = F
         (256, 2, 255),        # one partial block, lonely partner
         (256, 128, 392),      # m = F/2, odd block count
         (256, 128, 40),       # n < m
         (4096, 2048, 6154),
         (4096, 65, 12000),
         (8192, 4096, 8195),   # LOG2E = 5
         (16384, 8192, 24590),
         (16384, 3, 40000)]


@pytest.mark.parametrize("full", [False, True], ids=["causal", "full"])
@pytest.mark.parametrize("F,m,n", FUSED)
def test_fused_range(gdsp, D, F, m, n, full):
    assert gdsp.fft.fir_block(m, F) == (F, True)
    x, h, ref = _case(F + m + n, 1, n, m)
    got = _run(D, x, h, full, F)
    want = ref if full else ref[:, :n]
    assert got.shape == want.shape
    err = row_nrel(got, want)
    print(f"F={F} m={m} n={n} full={full}: {err:.3e}")
    assert err < EXACT


@pytest.mark.parametrize("full", [False, True], ids=["causal", "full"])
@pytest.mark.parametrize("F", [256, 512])
def test_slots_and_strides(gdsp, D, F, full):
    """17 rows of one transform each: the last workgroup has empty slots. x is
    a row-strided view, out a view into a buffer whose padding columns and
    guard row must keep their sentinel bit for bit."""
    import torch
    channels, n, m, guard = 17, 300, 9, -7.25
    assert gdsp.fft.fir_block(m, F) == (F, True)
    x, h, ref = _case(1000 + F, channels, n, m)
    out_len = n + m - 1 if full else n
    xb = torch.full((channels, n + 5), 3.5, dtype=torch.float64, device="cuda")
    xb[:, :n] = torch.from_numpy(np.array(x)).cuda()
    ob = torch.full((channels + 1, out_len + 3), guard, dtype=torch.float64, device="cuda")
    xv, ov = xb[:, :n], ob[:channels, :out_len]
    assert xv.stride(0) == n + 5 and ov.stride(0) == out_len + 3
    got = D.fir_batch(xv, torch.from_numpy(np.array(h)).cuda(), out=ov, full=full, block=F)
    torch.cuda.synchronize()
    assert got is ov
    o = ob.cpu().numpy()
    assert row_nrel(o[:channels, :out_len], ref[:, :out_len]) < EXACT
    assert np.all(o[:, out_len:] == guard) and np.all(o[channels] == guard)


def test_per_row_taps(D):
    channels, n, m = 3, 3000, 33
    x, h = _gauss(21, channels, n), _gauss(22, channels, m)
    for full in (False, True):
        got = _run(D, x, h, full)
        assert row_nrel(got, _ref(x, h, full)) < EXACT
        for c in range(channels):
            assert np.array_equal(got[c], _run(D, x[c:c + 1], h[c], full)[0]), c


def test_no_cross_talk(D):
    x, h, _ = _case(31, 5, 2500, 40)
    for block in (256, 1024):
        got = _run(D, x, h, True, block)
        for c in range(5):
            assert np.array_equal(got[c], _run(D, x[c:c + 1], h, True, block)[0]), (block, c)


def test_both_paths_agree(gdsp, D):
    F = gdsp.fft
    x, h, ref = _case(41, 3, 12000, 65)
    hr = _gauss(43, 3, 65)
    assert F.fir_block(65, 4096) == (4096, True)
    fused = [_run(D, x, h, True, 4096), _run(D, x, hr, True, 4096)]
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_FIR)
        assert F.fir_block(65, 4096) == (4096, False)
        composed = [_run(D, x, h, True, 4096), _run(D, x, hr, True, 4096)]
    finally:
        F.SetAlgorithm(prev)
    assert F.fir_block(65, 4096) == (4096, True)
    for a, b in zip(fused, composed):
        assert row_nrel(a, b) < EXACT
    assert row_nrel(composed[0], ref) < EXACT
    assert row_nrel(composed[1], _ref(x, hr, True)) < EXACT


@pytest.mark.parametrize("m,n,block,F", [(8193, 40000, 0, 32768), (100, 40000, 32768, 32768)])
def test_composed_range(gdsp, D, m, n, block, F):
    assert gdsp.fft.fir_block(m, block) == (F, False)
    x, h, ref = _case(51 + m, 1, n, m)
    for full in (False, True):
        err = row_nrel(_run(D, x, h, full, block), ref if full else ref[:, :n])
        print(f"composed m={m} n={n} full={full}: {err:.3e}")
        assert err < EXACT


@pytest.mark.parametrize("s", [0, 5, 76])
def test_delay(D, s):
    m, n = 77, 5000
    x = _gauss(61, 2, n)
    h = np.zeros(m)
    h[s] = 1.0
    want = np.zeros((2, n + m - 1))
    want[:, s:s + n] = x
    assert row_nrel(_run(D, x, h, True), want) < EXACT
    assert row_nrel(_run(D, x, h, False), want[:, :n]) < EXACT


def test_integers(gdsp, D):
    rng = np.random.default_rng(71)
    x = rng.integers(-100, 101, (2, 5000))
    h = rng.integers(-100, 101, 300)
    assert gdsp.fft.fir_block(300, 1024) == (1024, True)
    want = np.stack([np.convolve(r, h) for r in x])
    assert want.dtype == np.int64
    got = _run(D, x.astype(np.float64), h.astype(np.float64), True, 1024)
    dev = float(np.max(np.abs(got - np.rint(got))))
    print(f"integer deviation {dev:.3e}")
    assert np.array_equal(np.rint(got).astype(np.int64), want)
    assert dev < 1e-6


def test_zero_input(D):
    h = _gauss(81, 50)
    for block in (0, 256, 8192, 32768):
        got = _run(D, np.zeros((3, 4000)), h, True, block)
        assert got.shape == (3, 4049) and not got.any()


@pytest.mark.parametrize("m", [31, 2047])
def test_default_block(gdsp, D, m):
    F, fused = gdsp.fft.fir_block(m)
    assert fused and F >= 2 * m
    x, h, ref = _case(91 + m, 2, 3 * F + 17, m)
    got = _run(D, x, h, True)
    assert row_nrel(got, ref) < EXACT
    # the block the library chose is the one fir_block reports
    assert np.array_equal(got, _run(D, x, h, True, F))


def test_chunked_stream(D):
    m, n, cut = 65, 5000, 2300
    x, h, ref = _case(101, 2, n, m)
    a, b = _run(D, x[:, :cut], h, True), _run(D, x[:, cut:], h, True)
    y = np.zeros((2, n + m - 1))
    y[:, :cut + m - 1] += a
    y[:, cut:] += b
    whole = _run(D, x, h, True)
    assert row_nrel(y, whole) < EXACT
    assert row_nrel(whole, ref) < EXACT


def test_host_entry_equals_device_entry(gdsp, D):
    F = gdsp.fft
    x, h, ref = _case(111, 3, 2000, 20)
    hr = _gauss(113, 3, 20)
    for full in (False, True):
        assert np.array_equal(F.FIRFilterBatch(x, h, full=full), _run(D, x, h, full))
        assert np.array_equal(F.FIRFilterBatch(x, hr, full=full, block=512),
                              _run(D, x, hr, full, 512))
    # list input, and a strided array
    assert np.array_equal(F.FIRFilterBatch([r for r in x], h), _run(D, x, h))
    wide = np.zeros((3, 2007))
    wide[:, :2000] = x
    assert np.array_equal(F.FIRFilterBatch(wide[:, :2000], h), _run(D, x, h))
    assert np.array_equal(F.FIRFilter(x[0], h), _run(D, x[:1], h)[0])
    assert np.array_equal(F.ConvolveLinear(x[1], h), _run(D, x[1:2], h, True)[0])
    assert row_nrel(F.ConvolveLinear(x[1], h), ref[1]) < EXACT


def test_host_entry_in_place(gdsp):
    """The C entry's out may alias x: the caller's memory is only touched by
    host memcpy."""
    G = gdsp._lib
    x, h, ref = _case(121, 2, 1500, 12)
    buf = x.copy()
    p = buf.ctypes.data_as(G._P)
    G.check(G.lib().gdsp_fir_batch(p, 1500, h.ctypes.data_as(G._P), 1, 12, 2, 1500, 0, 0, p, 1500),
            "fir_batch")
    assert row_nrel(buf, ref[:, :1500]) < EXACT


def test_wav_filter_channels(gdsp):
    W, F = gdsp.wav, gdsp.fft
    path = os.path.join(GOLDEN, "wav", "small.wav")
    with open(path, "rb") as f:
        w = W.New(f)
        C = w.NumChannels
        frames = min(w.Samples // C, 20000)
        dec = w.ReadFloats(frames * C).astype(np.float64)
    chans = np.stack([dec[c::C] for c in range(C)])
    h = _gauss(131, 25)
    for full in (False, True):
        with open(path, "rb") as f:
            got = W.FilterChannels(W.New(f), frames, h, full=full)
        assert got.shape == (C, frames + 24 if full else frames)
        assert np.array_equal(got, F.FIRFilterBatch(chans, h, full=full))
    assert row_nrel(got, _ref(chans, h, True)) < EXACT


def test_device_entry_refuses_in_place(gdsp, D):
    import torch
    x = torch.zeros((2, 1000), dtype=torch.float64, device="cuda")
    h = torch.ones(5, dtype=torch.float64, device="cuda")
    with pytest.raises(gdsp.GDSPError) as e:
        D.fir_batch(x, h, out=x)
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID


def test_stream_and_work_buffer(gdsp, D):
    """With the caller's work buffer and stream, fused and composed."""
    import torch
    x, h, ref = _case(141, 2, 9000, 65)
    xt, ht = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(h)).cuda()
    # the taps' spectrum; composed: plus its chunk of both rows' one transform
    for block, rows in ((4096, 1), (32768, 1 + 2)):
        work = torch.empty(rows * block, dtype=torch.complex128, device="cuda")
        out = torch.empty((2, 9064), dtype=torch.float64, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        D.fir_batch(xt, ht, out=out, full=True, block=block, work=work, stream=st)
        st.synchronize()
        assert row_nrel(out.cpu().numpy(), ref) < EXACT
