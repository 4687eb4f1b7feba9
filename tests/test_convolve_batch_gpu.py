"""GPU parity of the batched Convolve (gdsp_convolve_batch,
gdsp_convolve_batch_device): rows against one y or one y per row, on the fused
one-kernel convolution (powers of 2, 256 ... 16384) and on the composed FFT,
multiply, IFFT chain (every other length), checked row by row against the
oracle's fft.Convolve within the suite's 1e-9, and the two paths against each
other within the 1e-13 the parity suite holds the engine to."""
import importlib

import numpy as np
import pytest

from conftest import row_nrel

pytestmark = pytest.mark.gpu

TOL = 1e-9     # north star: within 1e-9 relative for complex128
EXACT = 1e-13  # the engine against the exact DFT (test_parity_gpu.py)

# rows per workgroup of the fused kernel (256 threads, 16 points per thread)
TPW = {256: 16, 512: 8, 4096: 1, 8192: 1, 16384: 1}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


def _rows(seed, batch, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))


def _ref(oracle, x, y):
    return np.stack([oracle.convolve(x[g], y if y.ndim == 1 else y[g])
                     for g in range(x.shape[0])])


def _run(D, x, y, **kw):
    import torch
    out = D.convolve_batch(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "perrow"])
@pytest.mark.parametrize("n,batch", [(n, b) for n in TPW for b in (1, TPW[n] + 1)])
def test_fused_range(gdsp, oracle, D, n, batch, per_row):
    # batch TPW + 1: the last workgroup's other slots are empty
    assert D.plan(n).kind == 1 and D.convolve_fused(n)
    x = _rows(n + batch, batch, n)
    y = _rows(7 * n + batch, batch, n) if per_row else _rows(7 * n, 1, n)[0]
    assert row_nrel(_run(D, x, y), _ref(oracle, x, y)) < TOL


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "perrow"])
@pytest.mark.parametrize("n", [1, 2, 8, 128, 3, 5, 12, 257, 3000, 3001, 32768])
def test_composed_range(gdsp, oracle, D, n, per_row):
    assert not D.convolve_fused(n)
    x = _rows(n, 3, n)
    y = _rows(11 * n, 3, n) if per_row else _rows(11 * n, 1, n)[0]
    assert row_nrel(_run(D, x, y), _ref(oracle, x, y)) < TOL


def test_both_paths_agree(gdsp, D):
    F = gdsp.fft
    x, y = _rows(1, 5, 4096), _rows(2, 5, 4096)
    assert D.convolve_fused(4096)
    fused = [_run(D, x, y[0]), _run(D, x, y)]
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_CONVOLVE)
        assert not D.convolve_fused(4096)
        composed = [_run(D, x, y[0]), _run(D, x, y)]
    finally:
        F.SetAlgorithm(prev)
    assert D.convolve_fused(4096)
    for a, b in zip(fused, composed):
        assert row_nrel(a, b) < EXACT


def test_unit_impulse_rolls_the_rows(D):
    # y = delta(k - 5): the circular convolution is a rotation by 5
    n, batch, s = 512, 9, 5
    x = _rows(3, batch, n)
    y = np.zeros(n, np.complex128)
    y[s] = 1.0
    assert row_nrel(_run(D, x, y), np.roll(x, s, axis=1)) < EXACT


@pytest.mark.parametrize("n", [4096, 3000])  # fused, composed
def test_in_place_equals_out_of_place(D, n):
    import torch
    assert D.convolve_fused(n) == (n == 4096)
    x, y = _rows(n, 2, n), _rows(n + 1, 2, n)
    for yy in (y[0], y):
        want = _run(D, x, yy)
        xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(yy).cuda()
        got = D.convolve_batch(xt, yt, out=xt)
        torch.cuda.synchronize()
        assert got is xt
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("n", [4096, 3000])
def test_stream_and_work_buffer(D, n):
    import torch
    x, y = _rows(n + 2, 3, n), _rows(n + 3, 3, n)
    for yy in (y[0], y):
        want = _run(D, x, yy)
        xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(yy).cuda()
        work = torch.empty_like(yt)
        out = torch.empty_like(xt)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        D.convolve_batch(xt, yt, out=out, work=work, stream=st)
        st.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)


def test_host_entry_matches_convolve(gdsp):
    F = gdsp.fft
    x, y = _rows(4, 3, 1024), _rows(5, 3, 1024)
    one = np.stack([F.Convolve(x[g], y[0]) for g in range(3)])
    each = np.stack([F.Convolve(x[g], y[g]) for g in range(3)])
    assert row_nrel(F.ConvolveBatch(x, y[0]), one) < EXACT
    assert row_nrel(F.ConvolveBatch(x, y), each) < EXACT
