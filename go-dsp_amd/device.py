"""Device-pointer entry points of libgdspfft for callers that hold HBM-resident
data in torch tensors (bench.py, distributed.py). torch provides device memory,
streams and torch.distributed only; the transforms are the library's HIP
kernels. Each call is stream-ordered on torch's current stream of the tensor's
device (or the given stream)."""
from __future__ import annotations

import ctypes

from . import _lib
from ._lib import check, lib


def _torch():
    import torch
    return torch


def _stream_ptr(stream, device):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return ctypes.c_void_p(s.cuda_stream)


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


class Plan:
    """Cached device plan for transform length n on the current device
    (gdsp_plan_create). kind: 0 trivial, 1 LDS Stockham, 2 multi-pass
    Stockham, 3 fused Bluestein, 4 composed Bluestein, 5 mixed radix,
    6 mixed four-step, 7 Rader (a prime n <= 8193 whose n - 1 has a radix
    list; m = n - 1, the cyclic convolution's length), 8 prime-factor Rader
    (composite n = n1 * n2 <= 8192, n2 the prime; m = n2 - 1).
    chirpz=True forces the reference's Bluestein algorithm
    (gdsp_plan_create_chirpz) for a non-trivial length."""

    def __init__(self, n: int, chirpz: bool = False):
        self.n = int(n)
        self.chirpz = bool(chirpz)
        self.handle = ctypes.c_void_p()
        if self.chirpz:
            check(lib().gdsp_plan_create_chirpz(self.n, ctypes.byref(self.handle)),
                  "plan_create_chirpz")
        else:
            check(lib().gdsp_plan_create(self.n, ctypes.byref(self.handle)), "plan_create")
        self.kind = int(lib().gdsp_plan_kind(self.handle))
        v = [ctypes.c_int64() for _ in range(4)]
        rc = ctypes.c_int()
        check(lib().gdsp_plan_info(self.handle, *v, rc), "plan_info")
        # chirp-z convolution length; four-step split; runtime-compiled?
        self.m, self.n1, self.n2 = v[1].value, v[2].value, v[3].value
        self.runtime_compiled = bool(rc.value)
        # output parts of the chirp-z kernel (> 1: n in (8192, 14563] on M = 16384)
        self.parts = int(lib().gdsp_plan_parts(self.handle))
        # the mixed-radix passes (kind 5: the transform; 7 / 8: the Rader
        # convolution's; kind 3 on the smooth-L chirp-z kernel: those of its
        # convolution length m), () for the other plans
        r = (ctypes.c_int * 16)()
        k = int(lib().gdsp_plan_radices(self.handle, r, 16))
        self.radices = tuple(r[:min(k, 16)])


_plans: dict = {}


def plan(n: int, chirpz: bool = False) -> Plan:
    torch = _torch()
    # the library caches plans per (device, n, algorithm flags): so does this
    key = (torch.cuda.current_device(), int(n), bool(chirpz), int(lib().gdsp_get_algorithm()))
    if key not in _plans:
        _plans[key] = Plan(n, chirpz)
    return _plans[key]


def fft_batch(x, out=None, inverse: bool = False, stream=None, chirpz: bool = False):
    """Batched FFT/IFFT of the rows of a (batch, n) complex128 CUDA tensor
    (chirpz=True: through the forced-Bluestein plan)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.complex128 and x.dim() == 2 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
    with torch.cuda.device(x.device):
        p = plan(x.shape[1], chirpz)
        check(lib().gdsp_fft_batch_device(p.handle, _ptr(x), _ptr(out), x.shape[0], int(inverse),
                                          _stream_ptr(stream, x.device)), "fft_batch_device")
    return out


def convolve_fused(n: int) -> bool:
    """Whether convolve_batch runs rows of n on the fused one-kernel
    convolution under the current algorithm flags (gdsp_convolve_fused)."""
    return bool(lib().gdsp_convolve_fused(plan(n).handle))


def convolve_batch(x, y, out=None, work=None, stream=None):
    """fft.Convolve of every row of a (batch, n) complex128 CUDA tensor with y:
    a 1-D tensor of n (one y for all rows) or a tensor of x's shape (row by
    row). out may be x itself. work: scratch of y's size (complex128) for the
    spectrum of y; with it the call does not allocate
    (gdsp_convolve_batch_device)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.complex128 and x.dim() == 2 and x.is_contiguous()
    assert y.is_cuda and y.dtype == torch.complex128 and y.is_contiguous()
    assert y.device == x.device
    if tuple(y.shape) != tuple(x.shape) and tuple(y.shape) != (x.shape[1],):
        raise _lib.Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
    if work is not None:
        assert work.is_cuda and work.dtype == torch.complex128 and work.is_contiguous()
        assert work.numel() >= y.numel()
    y_rows = 1 if y.dim() == 1 else x.shape[0]
    with torch.cuda.device(x.device):
        p = plan(x.shape[1])
        wp = _ptr(work) if work is not None else ctypes.c_void_p()
        check(lib().gdsp_convolve_batch_device(p.handle, _ptr(x), _ptr(y), y_rows, _ptr(out),
                                               x.shape[0], wp, _stream_ptr(stream, x.device)),
              "convolve_batch_device")
    return out


def fir_batch(x, h, out=None, full: bool = False, block: int = 0, work=None, stream=None):
    """fft.FIRFilterBatch on float64 CUDA tensors: every row of x (channels,
    n; unit inner stride, any row stride) filtered with the taps h, (m,) or
    (channels, m) contiguous, into out (channels, n, or n + m - 1 with
    full=True; unit inner stride, any row stride), which must not overlap x.
    block: the overlap-save block length (0: fft.fir_block's choice). work:
    scratch (complex128) as gdsp_fir_batch_device sizes it; with it the fused
    form does not allocate (gdsp_fir_batch_device)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    assert h.is_cuda and h.dtype == torch.float64 and h.device == x.device and h.is_contiguous()
    channels, n = x.shape
    if h.dim() not in (1, 2) or (h.dim() == 2 and h.shape[0] != channels):
        raise _lib.Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    m = h.shape[-1]
    out_len = n + m - 1 if full else n
    if out is None:
        out = torch.empty((channels, max(out_len, 0)), dtype=torch.float64, device=x.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.device == x.device
    assert tuple(out.shape) == (channels, max(out_len, 0))
    assert n == 0 or x.stride(1) == 1, "rows must have unit inner stride"
    assert out_len <= 0 or out.stride(1) == 1, "rows must have unit inner stride"
    ldx = x.stride(0) if channels > 1 else n
    ldo = out.stride(0) if channels > 1 else out_len
    if work is not None:
        assert work.is_cuda and work.dtype == torch.complex128 and work.is_contiguous()
    h_rows = 1 if h.dim() == 1 else channels
    with torch.cuda.device(x.device):
        wp = _ptr(work) if work is not None else ctypes.c_void_p()
        check(lib().gdsp_fir_batch_device(_ptr(x), ldx, _ptr(h), h_rows, m, channels, n,
                                          int(bool(full)), int(block), _ptr(out), ldo, wp,
                                          _stream_ptr(stream, x.device)), "fir_batch_device")
    return out


def upfirdn_batch(x, h, up: int = 1, down: int = 1, out=None, out_begin: int = 0, out_end=None,
                  work=None, stream=None):
    """fft.UpfirdnBatch on float64 CUDA tensors: every row of x (channels, n;
    unit inner stride, any row stride) zero-stuffed by up, filtered with the
    taps h (m,) and decimated by down (scipy.signal.upfirdn(h, x, up, down)).
    Outputs [out_begin, out_end) of every row (out_end None: to the end,
    fft.upfirdn_length) go into out (channels, out_end - out_begin; unit inner
    stride, any row stride), which must not overlap x. work: scratch (float64)
    of up * ceil(m / up) elements for the phase-major taps; with it the call
    neither allocates nor synchronises (gdsp_upfirdn_batch_device)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    assert h.is_cuda and h.dtype == torch.float64 and h.device == x.device
    assert h.dim() == 1 and h.is_contiguous()
    channels, n = x.shape
    m = h.shape[0]
    up, down = int(up), int(down)
    L = int(lib().gdsp_upfirdn_length(n, m, up, down))
    end = L if out_end is None else int(out_end)
    cnt = max(end - int(out_begin), 0)
    if out is None:
        out = torch.empty((channels, cnt), dtype=torch.float64, device=x.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.device == x.device
    assert tuple(out.shape) == (channels, cnt)
    assert n == 0 or x.stride(1) == 1, "rows must have unit inner stride"
    assert cnt == 0 or out.stride(1) == 1, "rows must have unit inner stride"
    ldx = x.stride(0) if channels > 1 else n
    ldo = out.stride(0) if channels > 1 else cnt
    if work is not None:
        assert work.is_cuda and work.dtype == torch.float64 and work.is_contiguous()
        assert work.numel() >= up * -(-m // up)
    with torch.cuda.device(x.device):
        wp = _ptr(work) if work is not None else ctypes.c_void_p()
        check(lib().gdsp_upfirdn_batch_device(_ptr(x), ldx, _ptr(h), m, up, down, channels, n,
                                              int(out_begin), end, _ptr(out), ldo, wp,
                                              _stream_ptr(stream, x.device)),
              "upfirdn_batch_device")
    return out


_HILBERT_KINDS = {"analytic": _lib.GDSP_HILBERT_ANALYTIC, "quadrature": _lib.GDSP_HILBERT_QUADRATURE,
                  "envelope": _lib.GDSP_HILBERT_ENVELOPE}


def hilbert_batch(x, N=None, kind: str = "analytic", out=None, work=None, stream=None):
    """fft.HilbertBatch on a float64 CUDA tensor (rows, n; unit inner stride,
    any row stride): every row cut or zero-padded to N samples (None: n) and
    its analytic signal x + i h (kind "analytic": complex128), h alone
    ("quadrature": float64) or sqrt(fma(x, x, h h)) ("envelope": float64) into
    out (rows, N; unit inner stride, any row stride), which must not overlap
    x and is allocated only when not given. work: scratch (any dtype) of the
    bytes gdsp_hilbert_batch_device states for the composed form; the fused
    form (fft.hilbert_fused(N)) takes none, and with work given neither
    allocates nor synchronises."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    k = _HILBERT_KINDS[kind]
    rows, n = x.shape
    nfft = n if N is None else int(N)
    dt = torch.complex128 if k == _lib.GDSP_HILBERT_ANALYTIC else torch.float64
    if out is None:
        out = torch.empty((rows, max(nfft, 0)), dtype=dt, device=x.device)
    assert out.is_cuda and out.dtype == dt and out.device == x.device
    assert tuple(out.shape) == (rows, max(nfft, 0))
    assert n == 0 or x.stride(1) == 1, "rows must have unit inner stride"
    assert nfft <= 0 or out.stride(1) == 1, "rows must have unit inner stride"
    ldx = x.stride(0) if rows > 1 else n
    ldo = out.stride(0) if rows > 1 else nfft
    if work is not None:
        assert work.is_cuda and work.device == x.device and work.is_contiguous()
        if nfft > 0 and not lib().gdsp_hilbert_fused(nfft):
            need = min(rows, max(1, (1 << 24) // nfft)) * nfft * 24
            assert work.numel() * work.element_size() >= need and work.data_ptr() % 16 == 0
    with torch.cuda.device(x.device):
        wp = _ptr(work) if work is not None else ctypes.c_void_p()
        check(lib().gdsp_hilbert_batch_device(_ptr(x), ldx, rows, n, nfft, k, _ptr(out), ldo, wp,
                                              _stream_ptr(stream, x.device)),
              "hilbert_batch_device")
    return out


def dct_batch(x, n=None, type=2, norm=None, inverse: bool = False, out=None, work=None,
              stream=None):
    """fft.DCTBatch (inverse: fft.IDCTBatch) on a float64 CUDA tensor (rows,
    nx; unit inner stride, any row stride): every row cut or zero-padded to n
    samples (None: nx) and its cosine transform of type 2 or 3 under scipy's
    norm into out (rows, n; float64, unit inner stride, any row stride). out
    may be x itself (n <= nx; the same row stride), nothing else that overlaps
    it, and is allocated only when not given. work: scratch (any dtype) of
    gdsp_dct_work_doubles(rows, n) float64 for the composed form; the fused
    form (fft.dct_fused(n)) takes none, and with work given a call neither
    allocates nor synchronises."""
    from .fft import dct_kind, dct_length
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    t, k = dct_kind(type, norm, inverse, "dct_batch")
    nfft = dct_length(n, "dct_batch")  # ValueError below 1, as scipy
    rows, nx = x.shape
    nfft = nx if nfft is None else nfft
    if out is None:
        out = torch.empty((rows, max(nfft, 0)), dtype=torch.float64, device=x.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.device == x.device
    assert tuple(out.shape) == (rows, max(nfft, 0))
    assert nx == 0 or x.stride(1) == 1, "rows must have unit inner stride"
    assert nfft <= 0 or out.stride(1) == 1, "rows must have unit inner stride"
    ldx = x.stride(0) if rows > 1 else nx
    ldo = out.stride(0) if rows > 1 else nfft
    if work is not None:
        assert work.is_cuda and work.device == x.device and work.is_contiguous()
        need = int(lib().gdsp_dct_work_doubles(rows, nfft)) * 8
        assert work.numel() * work.element_size() >= need and work.data_ptr() % 16 == 0
    with torch.cuda.device(x.device):
        wp = _ptr(work) if work is not None else ctypes.c_void_p()
        check(lib().gdsp_dct_batch_device(_ptr(x), ldx, rows, nx, nfft, t, k, _ptr(out), ldo, wp,
                                          _stream_ptr(stream, x.device)),
              "dct_batch_device")
    return out


class CztPlan:
    """A chirp-z plan on the current device (gdsp_czt_plan_create): X[k] =
    sum_j x[j] z_k^-j on the m points z_k = a_abs exp(2 pi i (a_turns + k
    step_turns / step_div)) for rows of n samples, as fft.CZTBatch (by default
    m = n and the DFT's step). Owns the device tables; reusable across calls
    and streams of its device. F: the convolution length; fused: whether a
    call made now runs the fused kernel."""

    def __init__(self, n: int, m=None, step_turns=None, step_div=None, a_turns: float = 0.0,
                 a_abs: float = 1.0):
        from .fft import _czt_step
        self.n = int(n)
        self.m, st, sd = _czt_step(self.n, m, step_turns, step_div)
        self.handle = ctypes.c_void_p()
        self.device = _torch().cuda.current_device()
        check(lib().gdsp_czt_plan_create(self.n, self.m, float(a_abs), float(a_turns), st, sd,
                                         ctypes.byref(self.handle)), "czt_plan_create")
        v = [ctypes.c_int64() for _ in range(3)]
        check(lib().gdsp_czt_plan_info(self.handle, *v, None), "czt_plan_info")
        self.F = v[2].value

    @property
    def fused(self) -> bool:
        f = ctypes.c_int()
        check(lib().gdsp_czt_plan_info(self.handle, None, None, None, f), "czt_plan_info")
        return bool(f.value)

    def work_bytes(self, rows: int) -> int:
        """Bytes of `work` czt_batch takes for `rows` rows under the current
        flags (0 in the fused form)."""
        return int(lib().gdsp_czt_work_bytes(self.handle, int(rows)))

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                lib().gdsp_czt_plan_destroy(h)
            except Exception:
                pass


def czt_batch(x, plan: CztPlan, out=None, work=None, stream=None):
    """fft.CZTBatch on a float64 or complex128 CUDA tensor (rows, n; unit
    inner stride, any row stride) through a CztPlan: m complex128 per row into
    out (rows, m; unit inner stride, any row stride), which must not overlap x
    and is allocated only when not given. work: scratch (any dtype) of
    plan.work_bytes(rows) bytes for the composed form; the fused form takes
    none, and with work given a call neither allocates nor synchronises."""
    torch = _torch()
    assert x.is_cuda and x.dim() == 2 and x.dtype in (torch.float64, torch.complex128)
    rows, n = x.shape
    assert n == plan.n and x.device.index == plan.device
    if out is None:
        out = torch.empty((rows, plan.m), dtype=torch.complex128, device=x.device)
    assert out.is_cuda and out.dtype == torch.complex128 and out.device == x.device
    assert tuple(out.shape) == (rows, plan.m)
    assert x.stride(1) == 1 and out.stride(1) == 1, "rows must have unit inner stride"
    ldx = x.stride(0) if rows > 1 else n
    ldo = out.stride(0) if rows > 1 else plan.m
    wp, wb = ctypes.c_void_p(), 0
    if work is not None:
        assert work.is_cuda and work.device == x.device and work.is_contiguous()
        wp, wb = _ptr(work), work.numel() * work.element_size()
    with torch.cuda.device(x.device):
        check(lib().gdsp_czt_batch_device(plan.handle, _ptr(x), ldx, int(x.dtype == torch.float64),
                                          rows, _ptr(out), ldo, wp, wb,
                                          _stream_ptr(stream, x.device)), "czt_batch_device")
    return out


def zoom_fft_batch(x, fn, m=None, fs: float = 2, endpoint: bool = False, out=None):
    """fft.ZoomFFTBatch on a CUDA tensor (rows, n): the spectrum of every row
    at m frequencies from f1 to f2 (scipy.signal.zoom_fft), through a CztPlan
    built for the call."""
    from .fft import _zoom_params
    torch = _torch()
    m = x.shape[1] if m is None else int(m)
    _, _, at, st, sd = _zoom_params(fn, m, fs, endpoint)
    with torch.cuda.device(x.device):
        p = CztPlan(x.shape[1], m, st, sd, at)
        out = czt_batch(x, p, out=out)
        torch.cuda.current_stream(x.device).synchronize()  # before the plan's tables go
    return out


def _host_sos(sos):
    import numpy as np
    if _torch().is_tensor(sos):
        sos = sos.detach().cpu().numpy()
    s = np.ascontiguousarray(np.asarray(sos, dtype=np.float64))
    assert s.ndim == 2 and s.shape[1] == 6, "sos must have the shape (S, 6)"
    return s, s.ctypes.data_as(_lib._P)


def sosfilt_batch(x, sos, zi=None, out=None, work=None, stream=None, return_zf: bool = False):
    """fft.SosFiltBatch on a float64 CUDA tensor (channels, n; unit inner
    stride, any row stride): every row through the sections sos ((S, 6), a host
    array: the kernels' tables are host arithmetic) from the states zi
    ((channels, S, 2) contiguous CUDA tensor; None: zeros) into out (same shape;
    may be x itself, no other overlap). return_zf: also the final states as a
    (channels, S, 2) tensor. work: float64 scratch of
    gdsp_sosfilt_work_doubles(S, channels, n) elements; with it the call
    neither allocates nor synchronises (gdsp_sosfilt_batch_device)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    s, sp = _host_sos(sos)
    S = s.shape[0]
    channels, n = x.shape
    if out is None:
        out = torch.empty((channels, n), dtype=torch.float64, device=x.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.device == x.device
    assert tuple(out.shape) == (channels, n)
    assert n == 0 or (x.stride(1) == 1 and out.stride(1) == 1), "rows must have unit inner stride"
    ldx = x.stride(0) if channels > 1 else n
    ldo = out.stride(0) if channels > 1 else n
    if zi is not None:
        assert zi.is_cuda and zi.dtype == torch.float64 and zi.device == x.device
        assert tuple(zi.shape) == (channels, S, 2) and zi.is_contiguous()
    zf = torch.empty((channels, S, 2), dtype=torch.float64, device=x.device) if return_zf else None
    if work is not None:
        assert work.is_cuda and work.dtype == torch.float64 and work.is_contiguous()
        assert work.numel() >= int(lib().gdsp_sosfilt_work_doubles(S, channels, n))
    null = ctypes.c_void_p()
    with torch.cuda.device(x.device):
        check(lib().gdsp_sosfilt_batch_device(_ptr(x), ldx, sp, S,
                                              _ptr(zi) if zi is not None else null, channels, n,
                                              _ptr(out), ldo, _ptr(zf) if return_zf else null,
                                              _ptr(work) if work is not None else null,
                                              _stream_ptr(stream, x.device)),
              "sosfilt_batch_device")
    return (out, zf) if return_zf else out


def sosfiltfilt_batch(x, sos, padlen=None, out=None, work=None, stream=None):
    """fft.SosFiltFiltBatch on a float64 CUDA tensor (channels, n): zero-phase
    filtering as scipy.signal.sosfiltfilt(sos, x, axis=1, padlen=padlen) into
    out (same shape, no overlap with x). work: float64 scratch of
    gdsp_sosfiltfilt_work_doubles(S, channels, n, padlen) elements, which holds
    the forward pass's result (gdsp_sosfiltfilt_batch_device)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    s, sp = _host_sos(sos)
    S = s.shape[0]
    channels, n = x.shape
    pl = -1 if padlen is None else int(padlen)
    assert padlen is None or pl >= 0
    if out is None:
        out = torch.empty((channels, n), dtype=torch.float64, device=x.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.device == x.device
    assert tuple(out.shape) == (channels, n)
    assert n == 0 or (x.stride(1) == 1 and out.stride(1) == 1), "rows must have unit inner stride"
    ldx = x.stride(0) if channels > 1 else n
    ldo = out.stride(0) if channels > 1 else n
    if work is not None:
        assert work.is_cuda and work.dtype == torch.float64 and work.is_contiguous()
        p = pl if pl >= 0 else int(lib().gdsp_sosfiltfilt_padlen(sp, S))
        assert work.numel() >= int(lib().gdsp_sosfiltfilt_work_doubles(S, channels, n, p))
    with torch.cuda.device(x.device):
        check(lib().gdsp_sosfiltfilt_batch_device(_ptr(x), ldx, sp, S, pl, channels, n, _ptr(out),
                                                  ldo, _ptr(work) if work is not None
                                                  else ctypes.c_void_p(),
                                                  _stream_ptr(stream, x.device)),
              "sosfiltfilt_batch_device")
    return out


def resample_poly_batch(x, up: int, down: int, taps=None, out=None, stream=None):
    """fft.ResamplePolyBatch on a float64 CUDA tensor (channels, n):
    scipy.signal.resample_poly(x, up, down, axis=1) with its default zero
    padding, ceil(n up / down) samples per row. taps: the low-pass as it is, a
    1-D array or tensor (None: fft.resample_taps). One upfirdn_batch call on
    the padded taps whose range starts after the dropped outputs; up == down
    copies."""
    torch = _torch()
    import numpy as np

    from . import fft
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    u, d = fft._rate_pair(up, down)
    channels, n = x.shape
    if taps is None:
        h = fft.resample_taps(u, d)
    elif torch.is_tensor(taps):
        h = taps.detach().cpu().numpy()
    else:
        h = taps
    if np.iscomplexobj(h):
        raise TypeError("resample_poly_batch: complex taps are not supported")
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    pl = fft.resample_plan(n, u, d, h.size)
    if out is None:
        out = torch.empty((channels, pl["n_out"]), dtype=torch.float64, device=x.device)
    assert tuple(out.shape) == (channels, pl["n_out"])
    if u == d:
        out.copy_(x)
        return out
    if channels == 0 or n == 0:
        return out
    hh = np.concatenate([np.zeros(pl["pre"]), h, np.zeros(pl["post"])])
    return upfirdn_batch(x, torch.from_numpy(hh).to(x.device), u, d, out=out,
                         out_begin=pl["rem"], out_end=pl["rem"] + pl["n_out"], stream=stream)


def fft_real_batch(x, out=None, inverse: bool = False, stream=None, chirpz: bool = False):
    """fft.FFTReal / IFFTReal of the rows of a (batch, n) float64 CUDA tensor
    into a complex128 tensor (gdsp_fft_real_batch_device: the kernels read the
    real rows themselves)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.complex128, device=x.device)
    assert out.shape == x.shape and out.dtype == torch.complex128 and out.is_contiguous()
    with torch.cuda.device(x.device):
        p = plan(x.shape[1], chirpz)
        check(lib().gdsp_fft_real_batch_device(p.handle, _ptr(x), _ptr(out), x.shape[0],
                                               int(inverse), _stream_ptr(stream, x.device)),
              "fft_real_batch_device")
    return out


def fft2(x, out=None, inverse: bool = False, work=None, stream=None):
    """FFT2/IFFT2 of a (rows, cols) complex128 CUDA tensor."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.complex128 and x.dim() == 2 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        wp = _ptr(work) if work is not None else ctypes.c_void_p()
        check(lib().gdsp_fft2_device(_ptr(x), _ptr(out), x.shape[0], x.shape[1], int(inverse), wp,
                                     _stream_ptr(stream, x.device)), "fft2_device")
    return out


def fftn(x, out=None, inverse: bool = False, stream=None):
    """FFTN/IFFTN (fft/fft.go:157-192) of a contiguous complex128 CUDA tensor
    of any rank: every axis in turn (gdsp_fftn_device)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.complex128 and x.is_contiguous() and x.dim() >= 1
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.is_contiguous()
    if x.numel() == 0:
        return out
    dims = (ctypes.c_int64 * x.dim())(*x.shape)
    with torch.cuda.device(x.device):
        check(lib().gdsp_fftn_device(_ptr(x), _ptr(out), dims, x.dim(), int(inverse),
                                     _stream_ptr(stream, x.device)), "fftn_device")
    return out


def fft_axis(x, axis: int, out=None, inverse: bool = False, stream=None):
    """The 1-D FFT/IFFT along one axis of a contiguous complex128 CUDA tensor
    (gdsp_fft_axis_device; axis 0 of a matrix = computeFFT2's column pass)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.complex128 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.is_contiguous()
    if x.numel() == 0:
        return out
    dims = (ctypes.c_int64 * x.dim())(*x.shape)
    with torch.cuda.device(x.device):
        check(lib().gdsp_fft_axis_device(_ptr(x), _ptr(out), dims, x.dim(), axis % x.dim(),
                                         int(inverse), _stream_ptr(stream, x.device)),
              "fft_axis_device")
    return out


def fill_uniform(t, seed: int, offset: int = 0, stream=None):
    """Fill a float64 (or complex128, as interleaved pairs) CUDA tensor with the
    counter-based uniform[-1,1) generator."""
    torch = _torch()
    assert t.is_cuda and t.is_contiguous()
    count = t.numel() * (2 if t.dtype == torch.complex128 else 1)
    with torch.cuda.device(t.device):
        check(lib().gdsp_fill_uniform_device(_ptr(t), count, seed, offset,
                                             _stream_ptr(stream, t.device)), "fill_uniform")
    return t


def pwelch_accumulate(x, nfft: int, pad: int, noverlap: int, seg_begin: int, seg_end: int,
                      win_seg, acc, stream=None):
    """Adds the per-bin power sums of segments [seg_begin, seg_end) of the
    float64 CUDA signal x into acc (float64, max(pad, nfft) entries)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and acc.dtype == torch.float64
    with torch.cuda.device(x.device):
        check(lib().gdsp_pwelch_accumulate_device(
            _ptr(x), x.numel(), nfft, pad, noverlap, seg_begin, seg_end, _ptr(win_seg), _ptr(acc),
            _stream_ptr(stream, x.device)), "pwelch_accumulate")
    return acc


def pwelch_batch_accumulate(x, nfft: int, pad: int, noverlap: int, seg_begin: int, seg_end: int,
                            win_seg, acc, stream=None):
    """pwelch_accumulate over the rows of a 2-D float64 CUDA tensor (channels,
    n) with unit inner stride and any row stride: adds the sums of segments
    [seg_begin, seg_end) of row c into acc[c] (acc: (channels, max(pad, nfft))
    float64, contiguous). One fused kernel over all rows where
    spectral.pwelch_batch_fused says so (gdsp_pwelch_batch_accumulate_device)."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    channels, n = x.shape
    assert n == 0 or x.stride(1) == 1, "rows must have unit inner stride"
    ldx = x.stride(0) if channels > 1 else n
    assert ldx >= n, "rows overlap"
    flen = max(pad, nfft)
    assert acc.is_cuda and acc.dtype == torch.float64 and acc.is_contiguous()
    assert acc.numel() >= channels * flen
    assert win_seg.is_cuda and win_seg.dtype == torch.float64 and win_seg.numel() >= flen
    with torch.cuda.device(x.device):
        check(lib().gdsp_pwelch_batch_accumulate_device(
            _ptr(x), channels, n, ldx, nfft, pad, noverlap, seg_begin, seg_end, _ptr(win_seg),
            _ptr(acc), _stream_ptr(stream, x.device)), "pwelch_batch_accumulate")
    return acc


def _cpsd_rows(x, y):
    """(channels, n, ldx, ldy, y_rows) of a cross-spectral pair of float64
    CUDA tensors: x (channels, n), y (n,) or x's shape; unit inner strides."""
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    assert y.is_cuda and y.dtype == torch.float64 and y.device == x.device
    channels, n = x.shape
    if tuple(y.shape) != (n,) and tuple(y.shape) != (channels, n):
        raise _lib.Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    assert n == 0 or (x.stride(1) == 1 and y.stride(-1) == 1), "rows must have unit inner stride"
    ldx = x.stride(0) if channels > 1 else n
    y_rows = 1 if y.dim() == 1 else channels
    ldy = y.stride(0) if y_rows > 1 else n
    assert ldx >= n and ldy >= n, "rows overlap"
    return channels, n, ldx, ldy, y_rows


def cpsd_batch_accumulate(x, y, nfft: int, pad: int, noverlap: int, seg_begin: int, seg_end: int,
                          win_seg, acc, stream=None):
    """Adds the cross-spectral sums of segments [seg_begin, seg_end) of every
    row of x (channels, n) against y ((n,): one for all rows, or x's shape:
    row by row) into acc: (channels, 4, max(pad, nfft) // 2 + 1) float64,
    contiguous, planes Sxx, Syy, Re Sxy, Im Sxy with Sxy = sum conj(X_s) Y_s.
    The true sums of the range: ranges add in any split. float64 CUDA tensors,
    unit inner stride, any row stride (gdsp_cpsd_batch_accumulate_device)."""
    torch = _torch()
    channels, n, ldx, ldy, y_rows = _cpsd_rows(x, y)
    hb = max(pad, nfft) // 2 + 1
    assert acc.is_cuda and acc.dtype == torch.float64 and acc.is_contiguous()
    assert acc.numel() >= channels * 4 * hb
    assert win_seg.is_cuda and win_seg.dtype == torch.float64 and win_seg.numel() >= max(pad, nfft)
    with torch.cuda.device(x.device):
        check(lib().gdsp_cpsd_batch_accumulate_device(
            _ptr(x), ldx, _ptr(y), ldy, y_rows, channels, n, nfft, pad, noverlap, seg_begin,
            seg_end, _ptr(win_seg), _ptr(acc), _stream_ptr(stream, x.device)),
            "cpsd_batch_accumulate")
    return acc


def cpsd_batch(x, y, Fs: float, o, acc=None, stream=None, out=None):
    """spectral.CpsdBatch on float64 CUDA tensors (unit inner stride, any row
    stride), device-resident end to end: x (channels, n) against y, (n,) or
    x's shape. Returns spectral.CrossSpectra(Pxy complex128, Pxx, Pyy, Cxy
    float64, each (channels, pad // 2 + 1) on x's device, freqs numpy).
    acc: the caller's accumulator ((channels, 4, max(pad, nfft) // 2 + 1)
    float64, contiguous; overwritten); out: the caller's (Pxy, Pxx, Pyy, Cxy)
    tensors, contiguous, any of them None."""
    import contextlib

    import numpy as np

    from . import distributed, spectral
    torch = _torch()
    channels, n, _, _, _ = _cpsd_rows(x, y)
    dev = x.device
    if n == 0:  # pwelch.go:75-77
        e = torch.zeros((channels, 0), dtype=torch.float64, device=dev)
        return spectral.CrossSpectra(e.to(torch.complex128), e, e.clone(), e.clone(), np.zeros(0))
    nfft, pad, noverlap, wf, scaling = spectral.resolve_options(o)
    flen, lp = max(pad, nfft), pad // 2 + 1
    hb = flen // 2 + 1
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with torch.cuda.device(dev), ctx:
        if n < nfft:  # pwelch.go:97-99: zero-padded to nfft
            x = torch.nn.functional.pad(x, (0, nfft - n))
            y = torch.nn.functional.pad(y, (0, nfft - n))
        nsegs = spectral.segment_count(x.shape[1], nfft, noverlap)
        win_seg = distributed._device_window(wf, flen, dev, torch)
        if acc is None:
            acc = torch.zeros((channels, 4, hb), dtype=torch.float64, device=dev)
        else:
            assert acc.is_cuda and acc.dtype == torch.float64 and acc.is_contiguous()
            assert acc.numel() >= channels * 4 * hb
            acc.view(-1)[:channels * 4 * hb].zero_()
        outs = list(out) if out is not None else [None] * 4
        assert len(outs) == 4
        for i, dt in enumerate((torch.complex128, torch.float64, torch.float64, torch.float64)):
            if outs[i] is None:
                outs[i] = torch.empty((channels, lp), dtype=dt, device=dev)
            assert outs[i].is_cuda and outs[i].dtype == dt and outs[i].is_contiguous()
            assert outs[i].numel() >= channels * lp
        if nsegs > 0:
            cpsd_batch_accumulate(x, y, nfft, pad, noverlap, 0, nsegs, win_seg, acc, stream)
        win_nfft = np.ascontiguousarray(wf(nfft), dtype=np.float64)
        freqs = np.empty(lp, np.float64)
        check(lib().gdsp_cpsd_batch_finalize_device(
            _ptr(acc), channels, flen, nsegs, nfft, pad, win_nfft.ctypes.data_as(_lib._P),
            float(Fs), int(not scaling), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
            _ptr(outs[3]), freqs.ctypes.data_as(_lib._P), _stream_ptr(stream, dev)),
            "cpsd_batch_finalize")
    return spectral.CrossSpectra(outs[0], outs[1], outs[2], outs[3], freqs)


def _segment_rows(power: bool, x, Fs: float, o, out, seg_begin: int, seg_end, stream):
    """stft_batch / spectrogram_batch: the rows of segments [seg_begin, seg_end)
    of every row of x into out, (channels, seg_end - seg_begin, lp)."""
    import contextlib

    import numpy as np

    from . import distributed, spectral
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    channels, n = x.shape
    dev = x.device
    dtype = torch.float64 if power else torch.complex128
    if n == 0:  # pwelch.go:75-77
        return torch.zeros((channels, 0, 0), dtype=dtype, device=dev), np.zeros(0), np.zeros(0)
    assert x.stride(1) == 1, "rows must have unit inner stride"
    nfft, pad, noverlap, wf, scaling = spectral.resolve_options(o)
    flen, lp = max(pad, nfft), pad // 2 + 1
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with torch.cuda.device(dev), ctx:
        if n < nfft:  # pwelch.go:97-99: zero-padded to nfft
            x = torch.nn.functional.pad(x, (0, nfft - n))
        n = x.shape[1]
        ldx = x.stride(0) if channels > 1 else n
        assert ldx >= n, "rows overlap"
        nsegs = spectral.segment_count(n, nfft, noverlap)
        seg_end = nsegs if seg_end is None else int(seg_end)
        seg_begin = int(seg_begin)
        assert 0 <= seg_begin <= seg_end <= nsegs, (seg_begin, seg_end, nsegs)
        ns = seg_end - seg_begin
        if out is None:
            out = torch.empty((channels, ns, lp), dtype=dtype, device=dev)
        assert out.is_cuda and out.dtype == dtype and out.device == dev
        assert tuple(out.shape) == (channels, ns, lp), (tuple(out.shape), (channels, ns, lp))
        assert lp == 1 or out.stride(2) == 1, "rows must have unit inner stride"
        ld_seg = out.stride(1) if ns > 1 else lp
        ld_chan = out.stride(0) if channels > 1 else ns * ld_seg
        freqs = spectral.stft_freqs(pad, Fs)
        times = spectral.stft_times(seg_begin, seg_end, nfft, noverlap, Fs)
        if channels == 0 or ns == 0:
            return out, freqs, times
        win_seg = distributed._device_window(wf, flen, dev, torch)
        sp = _stream_ptr(stream, dev)
        if power:
            # gdsp_pwelch_finalize's norm: the window's squares summed in order
            w = np.ascontiguousarray(wf(nfft), dtype=np.float64)
            norm = float(np.cumsum(w * w)[-1]) if w.size else 0.0
            if scaling:
                norm *= float(Fs)
            check(lib().gdsp_spectrogram_batch_device(
                _ptr(x), ldx, channels, n, nfft, pad, noverlap, seg_begin, seg_end, _ptr(win_seg),
                norm, _ptr(out), ld_seg, ld_chan, sp), "spectrogram_batch_device")
        else:
            check(lib().gdsp_stft_batch_device(
                _ptr(x), ldx, channels, n, nfft, pad, noverlap, seg_begin, seg_end, _ptr(win_seg),
                _ptr(out), ld_seg, ld_chan, sp), "stft_batch_device")
    return out, freqs, times


def stft_batch(x, o, out=None, seg_begin: int = 0, seg_end=None, stream=None, Fs: float = 1.0):
    """spectral.StftBatch on a (channels, n) float64 CUDA tensor (unit inner
    stride, any row stride), device-resident: the complex128 rows of segments
    [seg_begin, seg_end) (None: all) of every channel. Returns (X, freqs,
    times) with X (channels, seg_end - seg_begin, pad // 2 + 1) on x's device
    and numpy freqs and times (of Fs; the default 1.0 gives cycles per sample
    and sample counts). out: any view of that shape whose last dimension is
    contiguous; its strides are the rows' (gdsp_stft_batch_device), and nothing
    between the rows is written."""
    return _segment_rows(False, x, Fs, o, out, seg_begin, seg_end, stream)


def spectrogram_batch(x, Fs: float, o, out=None, seg_begin: int = 0, seg_end=None, stream=None):
    """spectral.SpectrogramBatch on a (channels, n) float64 CUDA tensor: the
    float64 power rows c_j |X|^2 / norm of segments [seg_begin, seg_end) of
    every channel, as stft_batch (gdsp_spectrogram_batch_device). The mean of
    all rows of channel c over the segments is pwelch_batch's row c."""
    return _segment_rows(True, x, Fs, o, out, seg_begin, seg_end, stream)


def istft_batch(X, o, out=None, n=None, out_begin: int = 0, out_end=None, stream=None):
    """spectral.IstftBatch on a (channels, nsegs, pad // 2 + 1) complex128 CUDA
    tensor, device-resident (gdsp_istft_batch_device): samples [out_begin,
    out_end) (None: n, itself None for all (nsegs - 1) * stride + nfft) of
    every channel, as a (channels, out_end - out_begin) float64 tensor. X may
    be any view whose last dimension is contiguous; out any view of the
    result's shape with unit inner stride: nothing between its rows is written.
    Every range gives the bits of the whole call."""
    import contextlib

    from . import distributed, spectral
    torch = _torch()
    assert X.is_cuda and X.dtype == torch.complex128 and X.dim() == 3
    channels, nsegs, lpx = X.shape
    dev = X.device
    if nsegs == 0 or lpx == 0:
        return torch.zeros((channels, 0), dtype=torch.float64, device=dev)
    nfft, pad, noverlap, wf, _ = spectral.resolve_options(o)
    if pad < nfft:
        raise _lib.Panic(_lib.GDSP_ERR_INVALID,
                         "Pad below NFFT: a truncated spectrum has no inverse")
    lp = pad // 2 + 1
    if lpx != lp:
        raise _lib.Panic(_lib.GDSP_ERR_INVALID,
                         "rows of %d bins, Pad / 2 + 1 = %d expected" % (lpx, lp))
    assert X.stride(2) == 1, "rows must have unit inner stride"
    n_full = spectral.istft_length(nsegs, nfft, noverlap) if nsegs > 1 else nfft
    n = n_full if n is None else int(n)
    out_end = n if out_end is None else int(out_end)
    out_begin = int(out_begin)
    assert 0 <= out_begin <= out_end <= n <= n_full, (out_begin, out_end, n, n_full)
    length = out_end - out_begin
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with torch.cuda.device(dev), ctx:
        if out is None:
            out = torch.empty((channels, length), dtype=torch.float64, device=dev)
        assert out.is_cuda and out.dtype == torch.float64 and out.device == dev
        assert tuple(out.shape) == (channels, length), (tuple(out.shape), (channels, length))
        assert length <= 1 or out.stride(1) == 1, "rows must have unit inner stride"
        if channels == 0 or length == 0:
            return out
        ld_seg = X.stride(1) if nsegs > 1 else lp
        ld_chan = X.stride(0) if channels > 1 else nsegs * ld_seg
        ldo = out.stride(0) if channels > 1 else length
        win_seg = distributed._device_window(wf, pad, dev, torch)
        check(lib().gdsp_istft_batch_device(
            _ptr(X), ld_seg, ld_chan, channels, nsegs, 0, nsegs, nfft, pad, noverlap,
            _ptr(win_seg), out_begin, out_end, _ptr(out), ldo, _stream_ptr(stream, dev)),
            "istft_batch_device")
    return out


def pwelch_batch(x, Fs: float, o, out=None, acc=None, stream=None):
    """spectral.Pwelch of every row of a (channels, n) float64 CUDA tensor
    (unit inner stride, any row stride), device-resident end to end: returns
    the (channels, pad // 2 + 1) PSD tensor on x's device and freqs (numpy).
    Row c equals spectral.Pwelch(x[c], Fs, o). out / acc: caller's result and
    accumulator tensors ((channels, lp) and (channels, max(pad, nfft))
    float64, contiguous); acc is overwritten."""
    import contextlib

    import numpy as np

    from . import distributed, spectral
    torch = _torch()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2
    channels, n = x.shape
    dev = x.device
    if n == 0:  # pwelch.go:75-77
        return torch.zeros((channels, 0), dtype=torch.float64, device=dev), np.zeros(0)
    nfft, pad, noverlap, wf, scaling = spectral.resolve_options(o)
    flen, lp = max(pad, nfft), pad // 2 + 1
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with torch.cuda.device(dev), ctx:
        if n < nfft:  # pwelch.go:97-99: zero-padded to nfft
            x = torch.nn.functional.pad(x, (0, nfft - n))
        nsegs = spectral.segment_count(x.shape[1], nfft, noverlap)
        win_seg = distributed._device_window(wf, flen, dev, torch)
        if acc is None:
            acc = torch.zeros((channels, flen), dtype=torch.float64, device=dev)
        else:
            assert acc.is_cuda and acc.dtype == torch.float64 and acc.is_contiguous()
            assert acc.numel() >= channels * flen
            acc.view(-1)[:channels * flen].zero_()
        if out is None:
            out = torch.empty((channels, lp), dtype=torch.float64, device=dev)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
        assert out.numel() >= channels * lp
        if nsegs > 0:
            pwelch_batch_accumulate(x, nfft, pad, noverlap, 0, nsegs, win_seg, acc, stream)
        win_nfft = np.ascontiguousarray(wf(nfft), dtype=np.float64)
        freqs = np.empty(lp, np.float64)
        check(lib().gdsp_pwelch_batch_finalize_device(
            _ptr(acc), channels, flen, nsegs, nfft, pad, win_nfft.ctypes.data_as(_lib._P),
            float(Fs), int(not scaling), _ptr(out), freqs.ctypes.data_as(_lib._P),
            _stream_ptr(stream, dev)), "pwelch_batch_finalize")
    return out, freqs
