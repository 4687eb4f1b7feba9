"""Host mirror of go-dsp's `fft` package (fft/fft.go, fft/radix2.go,
fft/bluestein.go) over the libgdspfft C ABI. Same names, argument meaning and
panics as the Go API; slices become numpy arrays. Every transform runs on the
GPU (gfx950 kernels); nothing here computes a transform on the CPU.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import Panic, check, lib


def _p(a: np.ndarray):
    return a.ctypes.data_as(_lib._P)


def _as_c(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.complex128).reshape(-1))


def _as_f(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))


def FFT(x) -> np.ndarray:
    """fft.FFT — fft/fft.go:72-87. Returns a new array; x is not modified."""
    x = _as_c(x)
    out = np.empty_like(x)
    check(lib().gdsp_fft(_p(x), _p(out), x.size), "FFT")
    return out


def IFFT(x) -> np.ndarray:
    """fft.IFFT — fft/fft.go:35-52. Panics (index out of range) on len 0."""
    x = _as_c(x)
    if x.size == 0:
        raise Panic(_lib.GDSP_ERR_EMPTY, "runtime error: index out of range [0] with length 0")
    out = np.empty_like(x)
    check(lib().gdsp_ifft(_p(x), _p(out), x.size), "IFFT")
    return out


def FFTReal(x) -> np.ndarray:
    """fft.FFTReal — fft/fft.go:25-27 (full N-point complex spectrum)."""
    x = _as_f(x)
    out = np.empty(x.size, np.complex128)
    check(lib().gdsp_fft_real(_p(x), _p(out), x.size), "FFTReal")
    return out


def IFFTReal(x) -> np.ndarray:
    """fft.IFFTReal — fft/fft.go:30-32."""
    x = _as_f(x)
    if x.size == 0:
        raise Panic(_lib.GDSP_ERR_EMPTY, "runtime error: index out of range [0] with length 0")
    out = np.empty(x.size, np.complex128)
    check(lib().gdsp_ifft_real(_p(x), _p(out), x.size), "IFFTReal")
    return out


def Convolve(x, y) -> np.ndarray:
    """fft.Convolve — fft/fft.go:55-69."""
    x, y = _as_c(x), _as_c(y)
    if x.size != y.size:
        raise Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    out = np.empty_like(x)
    check(lib().gdsp_convolve(_p(x), _p(y), _p(out), x.size), "Convolve")
    return out


def ConvolveBatch(x, y) -> np.ndarray:
    """Additive batched Convolve: every row of the (batch, n) array x
    convolved with y — one y of n for all rows, or a (batch, n) array, row by
    row. fft.Convolve (fft/fft.go:55-69) per row, with its panic for any
    other shape of y."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex128))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.complex128))
    if x.ndim != 2:
        raise ValueError("ConvolveBatch expects a 2-D (batch, n) array")
    if y.shape != x.shape and y.shape != (x.shape[1],):
        raise Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    out = np.empty_like(x)
    y_rows = 1 if y.ndim == 1 else x.shape[0]
    check(lib().gdsp_convolve_batch(_p(x), _p(y), _p(out), x.shape[1], x.shape[0], y_rows),
          "ConvolveBatch")
    return out


def _real_rows(x, what: str) -> np.ndarray:
    """A list of real rows as a (channels, n) float64 array: ragged rows
    panic, complex samples are refused (never cast)."""
    if not isinstance(x, np.ndarray):
        rows = [np.asarray(r) for r in x]
        if any(r.ndim != 1 or r.size != rows[0].size for r in rows):
            raise Panic(_lib.GDSP_ERR_RAGGED, "ragged input array")
        if any(np.iscomplexobj(r) for r in rows):
            raise TypeError(f"{what}: complex input is not supported")
        x = np.asarray(rows, dtype=np.float64).reshape(len(rows), rows[0].size if rows else 0)
    if np.iscomplexobj(x):
        raise TypeError(f"{what}: complex input is not supported")
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f"{what} expects a 2-D (channels, n) array")
    return np.ascontiguousarray(x)


def fir_block(m: int, block: int = 0) -> tuple[int, bool]:
    """(F, fused): the overlap-save block length FIRFilterBatch uses for m taps
    (block=0: the library's choice; F = 0 where the call would fail) and
    whether the fused kernel runs it under the current algorithm flags
    (gdsp_fir_block; host arithmetic)."""
    fused = _lib._I(0)
    f = int(lib().gdsp_fir_block(int(m), int(block), fused))
    return f, bool(fused.value)


def FIRFilterBatch(rows, h, full: bool = False, block: int = 0) -> np.ndarray:
    """Additive FIR filter of every row of the real (channels, n) array (or
    list of rows) with the real taps h — (m,): one filter for all rows, or
    (channels, m): row by row: out[c, i] = sum_k h[k] rows[c, i - k], rows
    taken as zero outside [0, n). full=False: n samples per row
    (scipy.signal.lfilter(h, 1, x)); full=True: n + m - 1 (numpy.convolve).
    block: the overlap-save block length (0: the library's choice)."""
    x = _real_rows(rows, "FIRFilterBatch")
    if np.iscomplexobj(h):
        raise TypeError("FIRFilterBatch: complex taps are not supported")
    h = np.asarray(h, dtype=np.float64)  # (ascontiguousarray would make a scalar 1-D)
    channels, n = x.shape
    if h.ndim == 0 or h.ndim > 2 or (h.ndim == 2 and h.shape[0] != channels):
        raise Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    h = np.ascontiguousarray(h)
    m = h.shape[-1]
    out_len = n + m - 1 if full else n
    out = np.empty((channels, max(out_len, 0)), np.float64)
    if channels == 0:
        return out
    h_rows = 1 if h.ndim == 1 else channels
    check(lib().gdsp_fir_batch(_p(x), n, _p(h), h_rows, m, channels, n, int(bool(full)),
                               int(block), _p(out), out_len), "FIRFilterBatch")
    return out


def FIRFilter(x, h) -> np.ndarray:
    """The causal FIR filter of the real signal x with the real taps h: n
    samples, scipy.signal.lfilter(h, 1, x) (FIRFilterBatch of one row)."""
    if np.iscomplexobj(x):
        raise TypeError("FIRFilter: complex input is not supported")
    return FIRFilterBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), h)[0]


def ConvolveLinear(x, h) -> np.ndarray:
    """The linear convolution of the real vectors x and h: n + m - 1 samples,
    numpy.convolve(x, h) (FIRFilterBatch of one row, full)."""
    if np.iscomplexobj(x):
        raise TypeError("ConvolveLinear: complex input is not supported")
    return FIRFilterBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), h, full=True)[0]


def upfirdn_length(n: int, m: int, up: int = 1, down: int = 1) -> int:
    """L = ((n - 1) up + m - 1) div down + 1, the outputs per row of UpfirdnBatch;
    0 for n = 0 or m = 0, -1 where the call would be refused
    (gdsp_upfirdn_length; host arithmetic)."""
    return int(lib().gdsp_upfirdn_length(int(n), int(m), int(up), int(down)))


def upfirdn_fused(m: int, up: int = 1, down: int = 1) -> bool:
    """Whether UpfirdnBatch runs m taps at up/down on the fused polyphase
    kernel under the current algorithm flags (gdsp_upfirdn_fused; host
    arithmetic)."""
    return bool(lib().gdsp_upfirdn_fused(int(m), int(up), int(down)))


def UpfirdnBatch(rows, h, up: int = 1, down: int = 1, out_begin: int = 0,
                 out_end: int | None = None) -> np.ndarray:
    """Additive polyphase resampling of every row of the real (channels, n)
    array (or list of rows) with the real taps h (one set for all rows):
    scipy.signal.upfirdn(h, rows, up, down) — zero-stuff by up, filter, keep
    every down-th sample: out[c, j] = sum_i h[j down - i up] rows[c, i], j in
    [0, upfirdn_length(n, m, up, down)). out_begin, out_end: only that range
    of the outputs (out_end None: to the end)."""
    x = _real_rows(rows, "UpfirdnBatch")
    if np.iscomplexobj(h):
        raise TypeError("UpfirdnBatch: complex taps are not supported")
    h = np.asarray(h, dtype=np.float64)
    if h.ndim != 1:
        raise Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    h = np.ascontiguousarray(h)
    channels, n = x.shape
    m = h.size
    L = upfirdn_length(n, m, up, down)
    end = L if out_end is None else int(out_end)
    out = np.empty((channels, max(end - int(out_begin), 0)), np.float64)
    check(lib().gdsp_upfirdn_batch(_p(x), n, _p(h), m, int(up), int(down), channels, n,
                                   int(out_begin), end, _p(out), out.shape[1]), "UpfirdnBatch")
    return out


def Upfirdn(x, h, up: int = 1, down: int = 1) -> np.ndarray:
    """scipy.signal.upfirdn(h, x, up, down) of the real signal x (UpfirdnBatch
    of one row)."""
    if np.iscomplexobj(x):
        raise TypeError("Upfirdn: complex input is not supported")
    return UpfirdnBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), h, up, down)[0]


def hilbert_fused(N: int) -> bool:
    """Whether HilbertBatch runs transform length N on the fused
    analytic-signal kernel under the current algorithm flags
    (gdsp_hilbert_fused; host arithmetic)."""
    return bool(lib().gdsp_hilbert_fused(int(N)))


def _hilbert(rows, N, kind: int, what: str) -> np.ndarray:
    x = _real_rows(rows, what)
    r, n = x.shape
    nfft = n if N is None else int(N)
    if nfft < 0:
        raise _lib.GDSPError(_lib.GDSP_ERR_INVALID, "negative size")
    out = np.empty((r, nfft), np.complex128 if kind == _lib.GDSP_HILBERT_ANALYTIC else np.float64)
    check(lib().gdsp_hilbert_batch(_p(x), n, r, n, nfft, kind, _p(out), nfft), what)
    return out


def HilbertBatch(rows, N=None) -> np.ndarray:
    """Additive analytic signal of every row of the real (rows, n) array (or
    list of rows): scipy.signal.hilbert(rows, N, axis=1) — each row cut or
    zero-padded to N samples (None: n), x + i h with h the row's Hilbert
    transform; complex128 (rows, N). The real part is the input's own bits."""
    return _hilbert(rows, N, _lib.GDSP_HILBERT_ANALYTIC, "HilbertBatch")


def Hilbert(x, N=None) -> np.ndarray:
    """scipy.signal.hilbert(x, N) of the real signal x (HilbertBatch of one
    row)."""
    if np.iscomplexobj(x):
        raise TypeError("Hilbert: complex input is not supported")
    return HilbertBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), N)[0]


def EnvelopeBatch(rows, N=None) -> np.ndarray:
    """abs(scipy.signal.hilbert(rows, N, axis=1)) as sqrt(fma(x, x, h h)):
    float64 (rows, N), computed where the analytic signal is, without storing
    it."""
    return _hilbert(rows, N, _lib.GDSP_HILBERT_ENVELOPE, "EnvelopeBatch")


def Envelope(x, N=None) -> np.ndarray:
    """The envelope of the real signal x (EnvelopeBatch of one row)."""
    if np.iscomplexobj(x):
        raise TypeError("Envelope: complex input is not supported")
    return EnvelopeBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), N)[0]


def dct_fused(N: int) -> bool:
    """Whether DCTBatch / IDCTBatch run transform length N on the fused
    cosine-transform kernel under the current algorithm flags (gdsp_dct_fused;
    host arithmetic)."""
    return bool(lib().gdsp_dct_fused(int(N)))


_DCT_NORMS = {None: _lib.GDSP_DCT_BACKWARD, "backward": _lib.GDSP_DCT_BACKWARD,
              "ortho": _lib.GDSP_DCT_ORTHO, "forward": _lib.GDSP_DCT_FORWARD}
_DCT_OPPOSITE = {_lib.GDSP_DCT_BACKWARD: _lib.GDSP_DCT_FORWARD,
                 _lib.GDSP_DCT_ORTHO: _lib.GDSP_DCT_ORTHO,
                 _lib.GDSP_DCT_FORWARD: _lib.GDSP_DCT_BACKWARD}


def dct_kind(type, norm, inverse: bool = False, what: str = "DCT"):
    """(type, norm) of the C ABI for scipy's arguments. The inverse of (2, norm)
    is (3, the opposite norm) and the other way round; opposite swaps backward
    and forward and keeps ortho."""
    if isinstance(type, bool) or type not in (2, 3):
        raise ValueError(f"{what}: type must be 2 or 3, not {type!r}")
    if not (norm is None or isinstance(norm, str)) or norm not in _DCT_NORMS:
        raise ValueError(f"{what}: norm must be None, 'backward', 'ortho' or 'forward', "
                         f"not {norm!r}")
    t, k = int(type), _DCT_NORMS[norm]
    return (5 - t, _DCT_OPPOSITE[k]) if inverse else (t, k)


def dct_length(n, what: str = "DCT"):
    """scipy's n= as a transform length: None (the row length) or an integer of
    at least 1. scipy.fft.dct raises ValueError below 1; so does this, before
    anything is allocated: the C ABI reads nfft = 0 as "the row length", which
    an output of n = 0 columns would not hold."""
    if n is None:
        return None
    if isinstance(n, bool) or int(n) != n or int(n) < 1:
        raise ValueError(f"{what}: invalid number of data points ({n!r}) specified")
    return int(n)


def _dct(rows, type, n, norm, inverse: bool, what: str) -> np.ndarray:
    t, k = dct_kind(type, norm, inverse, what)
    nfft = dct_length(n, what)
    x = _real_rows(rows, what)
    r, nx = x.shape
    nfft = nx if nfft is None else nfft
    out = np.empty((r, nfft), np.float64)
    check(lib().gdsp_dct_batch(_p(x), nx, r, nx, nfft, t, k, _p(out), nfft), what)
    return out


def DCTBatch(rows, type=2, n=None, norm=None) -> np.ndarray:
    """Additive cosine transform of every row of the real (rows, nx) array (or
    list of rows): scipy.fft.dct(rows, type, n=n, axis=1, norm=norm) for type
    2 or 3 — each row cut or zero-padded to n samples (None: nx); float64
    (rows, n)."""
    return _dct(rows, type, n, norm, False, "DCTBatch")


def IDCTBatch(rows, type=2, n=None, norm=None) -> np.ndarray:
    """scipy.fft.idct(rows, type, n=n, axis=1, norm=norm): the DCT of the other
    type under the opposite norm (dct_kind)."""
    return _dct(rows, type, n, norm, True, "IDCTBatch")


def DCT(x, type=2, n=None, norm=None) -> np.ndarray:
    """scipy.fft.dct(x, type, n=n, norm=norm) of the real signal x (DCTBatch
    of one row)."""
    if np.iscomplexobj(x):
        raise TypeError("DCT: complex input is not supported")
    return _dct(np.asarray(x, dtype=np.float64).reshape(1, -1), type, n, norm, False, "DCT")[0]


def IDCT(x, type=2, n=None, norm=None) -> np.ndarray:
    """scipy.fft.idct(x, type, n=n, norm=norm) of the real signal x (IDCTBatch
    of one row)."""
    if np.iscomplexobj(x):
        raise TypeError("IDCT: complex input is not supported")
    return _dct(np.asarray(x, dtype=np.float64).reshape(1, -1), type, n, norm, True, "IDCT")[0]


def _sos(sos, what: str) -> np.ndarray:
    """Sections as a contiguous (S, 6) float64 array."""
    if np.iscomplexobj(sos):
        raise TypeError(f"{what}: complex coefficients are not supported")
    s = np.ascontiguousarray(np.asarray(sos, dtype=np.float64))
    if s.ndim != 2 or s.shape[1] != 6:
        raise _lib.GDSPError(_lib.GDSP_ERR_INVALID, "sos must have the shape (S, 6)")
    return s


def czt_length(n: int, m: int) -> tuple[int, bool]:
    """(F, fused): the convolution length CZTBatch uses for n samples and m
    points (0 where n + m - 1 exceeds 2^20: the call would fail) and whether
    the fused chirp-z kernel runs it under the current algorithm flags
    (gdsp_czt_length; host arithmetic)."""
    fused = _lib._I(0)
    f = int(lib().gdsp_czt_length(int(n), int(m), fused))
    return f, bool(fused.value)


def czt_fused(n: int, m: int) -> bool:
    """Whether CZTBatch runs (n, m) on the fused chirp-z kernel under the
    current algorithm flags (gdsp_czt_fused; host arithmetic)."""
    return bool(lib().gdsp_czt_fused(int(n), int(m)))


def _czt_step(n: int, m, step_turns, step_div):
    m = int(n) if m is None else int(m)
    if step_turns is None and step_div is None:
        return m, 1.0, max(m, 1)  # the DFT grid of m points
    return m, float(1.0 if step_turns is None else step_turns), int(1 if step_div is None else step_div)


def czt_points(m: int, step_turns=None, step_div=None, a_turns: float = 0.0,
               a_abs: float = 1.0) -> np.ndarray:
    """The m points z_k = a_abs exp(2 pi i (a_turns + k step_turns / step_div))
    CZT evaluates on (scipy.signal.czt_points with w = exp(-2 pi i step), a =
    a_abs exp(2 pi i a_turns)); by default the DFT's. Host arithmetic in
    float64, for plotting: the transform itself takes every angle exactly."""
    m, st, sd = _czt_step(m, m, step_turns, step_div)
    k = np.arange(m, dtype=np.float64)
    return float(a_abs) * np.exp(2j * np.pi * (float(a_turns) + k * st / sd))


def CZTBatch(rows, m=None, step_turns=None, step_div=None, a_turns: float = 0.0,
             a_abs: float = 1.0) -> np.ndarray:
    """Additive chirp-z transform of every row of the real or complex (rows,
    n) array on m points of a circle: X[k] = sum_j x[j] z_k^-j with z_k = a_abs
    exp(2 pi i (a_turns + k step_turns / step_div)), angles in turns, the step
    the exact rational step_turns / step_div (an int64 divisor). By default m =
    n and the step is 1 / m: the DFT. scipy.signal.czt(rows, m, w, a, axis=1)
    with w = exp(-2 pi i step), a = a_abs exp(2 pi i a_turns); spirals (|w| !=
    1) are not offered. complex128 (rows, m). Real rows stay real on the way
    to the GPU."""
    x = np.asarray(rows)
    if x.ndim != 2:
        raise ValueError("CZTBatch expects a 2-D (rows, n) array")
    real = not np.iscomplexobj(x)
    x = np.ascontiguousarray(x, dtype=np.float64 if real else np.complex128)
    r, n = x.shape
    m, st, sd = _czt_step(n, m, step_turns, step_div)
    if m < 0:
        raise _lib.GDSPError(_lib.GDSP_ERR_INVALID, "negative size")
    out = np.empty((r, m), np.complex128)
    check(lib().gdsp_czt_batch(_p(x), n, int(real), r, n, m, float(a_abs), float(a_turns), st, sd,
                               _p(out), m), "CZTBatch")
    return out


def CZT(x, m=None, step_turns=None, step_div=None, a_turns: float = 0.0,
        a_abs: float = 1.0) -> np.ndarray:
    """scipy.signal.czt of the signal x on an arc of a circle (CZTBatch of one
    row); by default its DFT."""
    x = np.asarray(x).reshape(1, -1)
    return CZTBatch(x, m, step_turns, step_div, a_turns, a_abs)[0]


def _zoom_params(fn, m: int, fs: float, endpoint: bool):
    f = np.atleast_1d(np.asarray(fn, dtype=np.float64))
    if f.size == 1:
        f1, f2 = 0.0, float(f[0])
    elif f.size == 2:
        f1, f2 = float(f[0]), float(f[1])
    else:
        raise ValueError("fn must be a scalar or a pair")
    m = int(m)
    div = m - 1 if endpoint else m
    return f1, f2, f1 / fs, (f2 - f1) / fs, max(div, 1)


def zoom_freqs(fn, m: int, fs: float = 2, endpoint: bool = False) -> np.ndarray:
    """The m frequencies ZoomFFT(x, fn, m, fs, endpoint) evaluates:
    numpy.linspace(f1, f2, m, endpoint=endpoint)."""
    f1, f2, _, _, _ = _zoom_params(fn, m, fs, endpoint)
    return np.linspace(f1, f2, int(m), endpoint=bool(endpoint))


def ZoomFFTBatch(rows, fn, m=None, fs: float = 2, endpoint: bool = False) -> np.ndarray:
    """scipy.signal.zoom_fft(rows, fn, m, fs=fs, endpoint=endpoint, axis=1):
    the spectrum of every row at m frequencies from f1 to f2 (fn = [f1, f2],
    or a scalar f2 with f1 = 0), at the sampling rate fs. CZTBatch with a_turns
    = f1 / fs and the exact step ((f2 - f1) / fs) / m (or m - 1 with
    endpoint)."""
    x = np.asarray(rows)
    if x.ndim != 2:
        raise ValueError("ZoomFFTBatch expects a 2-D (rows, n) array")
    m = x.shape[1] if m is None else int(m)
    _, _, at, st, sd = _zoom_params(fn, m, fs, endpoint)
    return CZTBatch(x, m, st, sd, at)


def ZoomFFT(x, fn, m=None, fs: float = 2, endpoint: bool = False) -> np.ndarray:
    """scipy.signal.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint) of one signal
    (ZoomFFTBatch of one row)."""
    return ZoomFFTBatch(np.asarray(x).reshape(1, -1), fn, m, fs, endpoint)[0]


def sosfilt_fused(sos) -> bool:
    """Whether SosFiltBatch runs these sections on the time-parallel kernel
    under the current algorithm flags: 1 to 8 sections, each strictly inside
    the stability triangle (gdsp_sosfilt_fused; host arithmetic)."""
    s = _sos(sos, "sosfilt_fused")
    return bool(lib().gdsp_sosfilt_fused(_p(s), s.shape[0]))


def sosfilt_granule(S: int) -> int:
    """G: a row cut at a multiple of G into calls chained by zi = zf gives the
    bits of one call (gdsp_sosfilt_granule; host arithmetic)."""
    return int(lib().gdsp_sosfilt_granule(int(S)))


def sosfilt_zi(sos) -> np.ndarray:
    """scipy.signal.sosfilt_zi(sos): the (S, 2) states of the settled unit step
    response (gdsp_sosfilt_zi; host arithmetic in long double)."""
    s = _sos(sos, "sosfilt_zi")
    zi = np.empty((s.shape[0], 2), np.float64)
    check(lib().gdsp_sosfilt_zi(_p(s), s.shape[0], _p(zi)), "sosfilt_zi")
    return zi


def sosfiltfilt_padlen(sos) -> int:
    """scipy's default padlen of sosfiltfilt, 3 (2 S + 1 - min(#{b2 == 0},
    #{a2 == 0})) (gdsp_sosfiltfilt_padlen)."""
    s = _sos(sos, "sosfiltfilt_padlen")
    return int(lib().gdsp_sosfiltfilt_padlen(_p(s), s.shape[0]))


def butter_sos(order: int, Wn: float, btype: str = "low") -> np.ndarray:
    """Butterworth low-pass or high-pass of the given order with its -3 dB edge
    at Wn (1 = Nyquist), as (ceil(order / 2), 6) second-order sections, in
    closed form: the analog poles w exp(i pi (2 k + order + 1) / (2 order)),
    w = 2 tan(pi Wn / 2) the prewarped edge, each conjugate pair through the
    bilinear transform s = 2 (z - 1) / (z + 1). An odd order gives a
    first-order first section (b2 = a2 = 0); the pairs follow by increasing a2
    (scipy's order). Every section has unit gain at DC (low) or at Nyquist
    (high), where scipy.signal.butter(..., output="sos") puts the whole gain
    into section 0: same denominators, same response."""
    order = int(order)
    if btype not in ("low", "high"):
        raise ValueError("butter_sos: btype must be 'low' or 'high'")
    if order < 1 or not (0.0 < float(Wn) < 1.0):
        raise _lib.GDSPError(_lib.GDSP_ERR_INVALID, "order >= 1 and 0 < Wn < 1")
    high = btype == "high"
    w = 2.0 * np.tan(np.pi * float(Wn) / 2.0)
    secs = []
    if order % 2:
        a0 = 2.0 + w
        b = (2.0 / a0, -2.0 / a0, 0.0) if high else (w / a0, w / a0, 0.0)
        secs.append([*b, 1.0, (w - 2.0) / a0, 0.0])
    pairs = []
    for k in range(order // 2):
        c = -2.0 * np.cos(np.pi * (2 * k + order + 1) / (2 * order)) * w  # s^2 + c s + w^2
        a0 = 4.0 + 2.0 * c + w * w
        g = 4.0 / a0 if high else w * w / a0
        pairs.append([g, (-2.0 if high else 2.0) * g, g, 1.0, (2.0 * w * w - 8.0) / a0,
                      (4.0 - 2.0 * c + w * w) / a0])
    pairs.sort(key=lambda q: q[5])
    return np.array(secs + pairs, dtype=np.float64)


def SosFiltBatch(rows, sos, zi=None, return_zf: bool = False):
    """Additive recursive (IIR) filtering of every row of the real (channels,
    n) array (or list of rows): scipy.signal.sosfilt(sos, rows, axis=1, zi=zi)
    with one set of sections (S, 6) for all rows, a0 == 1. zi: (channels, S, 2)
    initial states (None: zeros). return_zf: also the final states, so that a
    recording can be filtered piece by piece (gdsp_sosfilt_batch)."""
    x = _real_rows(rows, "SosFiltBatch")
    s = _sos(sos, "SosFiltBatch")
    channels, n = x.shape
    S = s.shape[0]
    x = np.ascontiguousarray(x)
    z = None
    if zi is not None:
        z = np.ascontiguousarray(np.asarray(zi, dtype=np.float64))
        if z.shape != (channels, S, 2):
            raise _lib.GDSPError(_lib.GDSP_ERR_INVALID, "zi must have the shape (channels, S, 2)")
    out = np.empty((channels, n), np.float64)
    zf = np.zeros((channels, S, 2), np.float64) if return_zf else None
    check(lib().gdsp_sosfilt_batch(_p(x), n, _p(s), S, _p(z) if z is not None else None, channels,
                                   n, _p(out), n, _p(zf) if zf is not None else None),
          "SosFiltBatch")
    return (out, zf) if return_zf else out


def SosFilt(x, sos, zi=None, return_zf: bool = False):
    """scipy.signal.sosfilt(sos, x) of the real signal x (SosFiltBatch of one
    row); zi and the returned zf are (S, 2)."""
    if np.iscomplexobj(x):
        raise TypeError("SosFilt: complex input is not supported")
    z = None if zi is None else np.asarray(zi, dtype=np.float64)[None]
    r = SosFiltBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), sos, z, return_zf)
    return (r[0][0], r[1][0]) if return_zf else r[0]


def SosFiltFiltBatch(rows, sos, padlen=None) -> np.ndarray:
    """Zero-phase filtering of every row: scipy.signal.sosfiltfilt(sos, rows,
    axis=1, padtype="odd", padlen=padlen), forward and backward over the odd
    extension of each row (padlen None: scipy's default, sosfiltfilt_padlen);
    rows must be longer than padlen (gdsp_sosfiltfilt_batch)."""
    x = np.ascontiguousarray(_real_rows(rows, "SosFiltFiltBatch"))
    s = _sos(sos, "SosFiltFiltBatch")
    channels, n = x.shape
    pl = -1 if padlen is None else int(padlen)
    if pl < 0 and padlen is not None:
        raise _lib.GDSPError(_lib.GDSP_ERR_INVALID, "negative size")
    out = np.empty((channels, n), np.float64)
    check(lib().gdsp_sosfiltfilt_batch(_p(x), n, _p(s), s.shape[0], pl, channels, n, _p(out), n),
          "SosFiltFiltBatch")
    return out


def SosFiltFilt(x, sos, padlen=None) -> np.ndarray:
    """scipy.signal.sosfiltfilt(sos, x) of the real signal x (SosFiltFiltBatch
    of one row)."""
    if np.iscomplexobj(x):
        raise TypeError("SosFiltFilt: complex input is not supported")
    return SosFiltFiltBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), sos, padlen)[0]


def _rate_pair(up: int, down: int) -> tuple[int, int]:
    import math
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise _lib.GDSPError(_lib.GDSP_ERR_INVALID, "up and down must be at least 1")
    g = math.gcd(up, down)
    return up // g, down // g


def resample_taps(up: int, down: int) -> np.ndarray:
    """The anti-alias low-pass ResamplePoly uses by default, scipy's
    firwin(2 half + 1, 1 / R, window=('kaiser', 5.0)) * up with R = max(up,
    down) after the gcd reduction and half = 10 R: h[k] = (1 / R) sinc((k -
    half) / R) kaiser(2 half + 1, 5.0)[k], divided by its sum, times up."""
    up, down = _rate_pair(up, down)
    R = max(up, down)
    half = 10 * R
    k = np.arange(2 * half + 1) - half
    h = (1.0 / R) * np.sinc(k / R) * np.kaiser(2 * half + 1, 5.0)
    h /= h.sum()
    return h * up


def resample_plan(n: int, up: int, down: int, m: int | None = None) -> dict:
    """The arithmetic of ResamplePoly (scipy.signal.resample_poly's) for rows
    of n samples and m taps (None: resample_taps'): the reduced up and down,
    half = (m - 1) div 2, pre zeros in front of the taps and post behind them,
    rem outputs dropped in front and n_out = ceil(n up / down) kept."""
    up, down = _rate_pair(up, down)
    if m is None:
        m = 20 * max(up, down) + 1
    half = (int(m) - 1) // 2
    n_out = -(-int(n) * up // down)
    pre = down - half % down
    rem = (half + pre) // down
    post = 0
    while n > 0 and ((n - 1) * up + m + pre + post - 1) // down + 1 < n_out + rem:
        post += 1
    return {"up": up, "down": down, "half": half, "pre": pre, "post": post, "rem": rem,
            "n_out": n_out}


def ResamplePolyBatch(rows, up: int, down: int, taps=None) -> np.ndarray:
    """scipy.signal.resample_poly(rows, up, down, axis=1) with its default
    zero padding: every row of the real (channels, n) array at up / down
    times its rate, ceil(n up / down) samples, the filter's delay removed.
    taps: the low-pass to use as it is (None: resample_taps(up, down)); its
    centre is tap (len - 1) div 2. One UpfirdnBatch call on the padded taps
    whose range starts after the dropped outputs; up == down returns a copy."""
    x = _real_rows(rows, "ResamplePolyBatch")
    if taps is not None and np.iscomplexobj(taps):
        raise TypeError("ResamplePolyBatch: complex taps are not supported")
    u, d = _rate_pair(up, down)
    if u == d:
        return x.copy()
    h = resample_taps(u, d) if taps is None else np.asarray(taps, dtype=np.float64).reshape(-1)
    pl = resample_plan(x.shape[1], u, d, h.size)
    if x.shape[0] == 0 or x.shape[1] == 0:
        return np.empty((x.shape[0], pl["n_out"]), np.float64)
    hh = np.concatenate([np.zeros(pl["pre"]), h, np.zeros(pl["post"])])
    return UpfirdnBatch(x, hh, u, d, pl["rem"], pl["rem"] + pl["n_out"])


def ResamplePoly(x, up: int, down: int, taps=None) -> np.ndarray:
    """scipy.signal.resample_poly(x, up, down) of the real signal x
    (ResamplePolyBatch of one row)."""
    if np.iscomplexobj(x):
        raise TypeError("ResamplePoly: complex input is not supported")
    return ResamplePolyBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), up, down, taps)[0]


def FFTBatch(x, inverse: bool = False) -> np.ndarray:
    """Additive batched entry point: FFT (or IFFT) of every row
    of a (batch, n) complex array, in one GPU launch."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex128))
    if x.ndim != 2:
        raise ValueError("FFTBatch expects a 2-D (batch, n) array")
    out = np.empty_like(x)
    check(lib().gdsp_fft_batch(_p(x), _p(out), x.shape[1], x.shape[0], int(inverse)), "FFTBatch")
    return out


def FFTRealBatch(x) -> np.ndarray:
    """FFTReal of every row of a (batch, n) float64 array."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if x.ndim != 2:
        raise ValueError("FFTRealBatch expects a 2-D (batch, n) array")
    out = np.empty(x.shape, np.complex128)
    check(lib().gdsp_fft_real_batch(_p(x), _p(out), x.shape[1], x.shape[0]), "FFTRealBatch")
    return out


def _matrix(x, dtype) -> np.ndarray:
    """Flatten [][]T after the reference's checks (fft/fft.go:124-136)."""
    if isinstance(x, np.ndarray):
        if x.ndim != 2 or x.shape[0] == 0:
            if x.ndim == 2 or x.size == 0:
                raise Panic(_lib.GDSP_ERR_EMPTY, "empty input array")
            raise ValueError("expected a 2-D matrix")
        return np.ascontiguousarray(x, dtype=dtype)
    rows = list(x)
    if len(rows) == 0:
        raise Panic(_lib.GDSP_ERR_EMPTY, "empty input array")
    cols = len(rows[0])
    for r in rows:
        if len(r) != cols:
            raise Panic(_lib.GDSP_ERR_RAGGED, "ragged input array")
    return np.ascontiguousarray(np.asarray(rows, dtype=dtype).reshape(len(rows), cols))


def _fft2(x, real: bool, inverse: bool) -> np.ndarray:
    m = _matrix(x, np.float64 if real else np.complex128)
    out = np.empty(m.shape, np.complex128)
    fn = lib().gdsp_fft2_real if real else lib().gdsp_fft2
    check(fn(_p(m), _p(out), m.shape[0], m.shape[1], int(inverse)), "FFT2")
    return out


def FFT2(x) -> np.ndarray:
    """fft.FFT2 — fft/fft.go:109-111 (computeFFT2 :123-154)."""
    return _fft2(x, False, False)


def IFFT2(x) -> np.ndarray:
    """fft.IFFT2 — fft/fft.go:119-121."""
    return _fft2(x, False, True)


def FFT2Real(x) -> np.ndarray:
    """fft.FFT2Real — fft/fft.go:104-106."""
    return _fft2(x, True, False)


def IFFT2Real(x) -> np.ndarray:
    """fft.IFFT2Real — fft/fft.go:114-116."""
    return _fft2(x, True, True)


def _fftn(m, inverse: bool):
    from .dsputils import MakeMatrix
    x = np.ascontiguousarray(m.list, dtype=np.complex128)
    dims = np.ascontiguousarray(np.asarray(m.dims, dtype=np.int64))
    out = np.empty_like(x)
    check(lib().gdsp_fftn(_p(x), _p(out), _p(dims), dims.size, int(inverse)), "FFTN")
    return MakeMatrix(out, list(m.dims))


def FFTN(m):
    """fft.FFTN — fft/fft.go:157-159 (computeFFTN :166-192): N-D DFT of a
    dsputils.Matrix; returns a new Matrix."""
    return _fftn(m, False)


def IFFTN(m):
    """fft.IFFTN — fft/fft.go:162-164."""
    return _fftn(m, True)


def SetWorkerPoolSize(n: int) -> None:
    """fft.SetWorkerPoolSize — fft/fft.go:95-101 (recorded; the GPU path has no
    goroutine pool)."""
    lib().gdsp_set_worker_pool_size(int(n))


def EnsureRadix2Factors(input_len: int) -> None:
    """fft.EnsureRadix2Factors — fft/radix2.go:35-37: pre-build the device plan
    (twiddle table, and for non-powers of 2 the Bluestein tables)."""
    check(lib().gdsp_ensure_plan(int(input_len)), "EnsureRadix2Factors")


# ---- multi-device (include/gdsp_fft.h "multi-device") ---------------------
# The reference hides its parallelism inside each call (radix2.go:89-151);
# these select and use the GPUs of the node the same way.

def _dev_array(devices):
    import ctypes
    if devices is None:
        return None, 0
    ids = [int(d) for d in devices]
    return (ctypes.c_int * len(ids))(*ids), len(ids)


def SetDevices(devices=None) -> None:
    """Device set of the host-pointer calls (gdsp_set_devices): once set to
    more than one entry, large FFTBatch / FFTRealBatch / spectral.Pwelch calls
    split over it. A device may repeat (its shards then share it on separate
    streams). None or [] restores the default: the calling thread's current
    device (or GDSP_DEVICES), i.e. no automatic split."""
    arr, n = _dev_array(devices or [])
    check(lib().gdsp_set_devices(arr, n), "SetDevices")


def Devices() -> list[int]:
    """The current device set (gdsp_get_devices); [] without a GPU."""
    import ctypes
    n = int(lib().gdsp_get_devices(None, 0))
    arr = (ctypes.c_int * max(n, 1))()
    n = int(lib().gdsp_get_devices(arr, n))
    return list(arr[:n])


# algorithm selection (gdsp_set_algorithm, include/gdsp_fft.h)
ALGO_DEFAULT = 0
ALGO_GENERIC_MIXED = 1
ALGO_NO_CHIRPZ_PARTS = 2
ALGO_CHIRPZ_POW2 = 4
ALGO_CHIRPZ_UNFUSED = 8
ALGO_NO_RADER = 16
ALGO_NO_RACE = 32
ALGO_NO_FUSED_CONVOLVE = 64
ALGO_NO_FUSED_PWELCH_BATCH = 128
ALGO_NO_FUSED_CPSD = 256
ALGO_NO_FUSED_FIR = _lib.GDSP_ALGO_NO_FUSED_FIR
ALGO_NO_FUSED_STFT = 1024
ALGO_NO_FUSED_ISTFT = 4096  # 2048 is not a flag
ALGO_NO_FUSED_UPFIRDN = 8192
ALGO_NO_FUSED_HILBERT = 32768  # 16384 is not a flag
ALGO_NO_FUSED_SOSFILT = 65536
ALGO_NO_FUSED_CZT = 262144  # 131072 is not a flag
ALGO_NO_FUSED_DCT = 1 << 21  # 1 << 19 and 1 << 20 are not flags


def SetAlgorithm(flags: int = ALGO_DEFAULT) -> None:
    """Select alternative paths of the engine (same DFT) for plans built and
    Pwelch calls made after this call (gdsp_set_algorithm)."""
    check(lib().gdsp_set_algorithm(int(flags)), "SetAlgorithm")


def Algorithm() -> int:
    return int(lib().gdsp_get_algorithm())


def MultiStats() -> dict:
    """gdsp_multi_stats: calls split over a device set since process start,
    and how Pwelch accumulators were combined."""
    import ctypes
    v = [ctypes.c_int64() for _ in range(4)]
    check(lib().gdsp_multi_stats(*[ctypes.byref(a) for a in v]), "MultiStats")
    return dict(zip(("batch_calls", "pwelch_calls", "rccl_reduces", "host_reduces"),
                    (a.value for a in v)))


def LoopStats() -> dict:
    """gdsp_loop_stats: second-or-later iterations of the host chunk loops, and
    Pwelch / Cpsd / STFT / ISTFT launches whose workers took two or more pairs or groups,
    since process start."""
    import ctypes
    v = [ctypes.c_int64() for _ in range(2)]
    check(lib().gdsp_loop_stats(*[ctypes.byref(a) for a in v]), "LoopStats")
    return dict(zip(("later_chunks", "multi_unit_launches"), (a.value for a in v)))


def FFTBatchMulti(x, inverse: bool = False, devices=None) -> np.ndarray:
    """FFTBatch split over `devices` (None: the device set): contiguous row
    shards, one per device, no collective (gdsp_fft_batch_multi)."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex128))
    if x.ndim != 2:
        raise ValueError("FFTBatchMulti expects a 2-D (batch, n) array")
    out = np.empty_like(x)
    arr, n = _dev_array(devices)
    check(lib().gdsp_fft_batch_multi(_p(x), _p(out), x.shape[1], x.shape[0], int(inverse),
                                     arr, n), "FFTBatchMulti")
    return out


def batch_shard(batch: int, ndev: int, i: int) -> tuple[int, int]:
    """Rows [lo, hi) of shard i of ndev (gdsp_batch_shard; host arithmetic)."""
    lo, hi = _lib._I64(0), _lib._I64(0)
    check(lib().gdsp_batch_shard(int(batch), int(ndev), int(i), lo, hi), "batch_shard")
    return lo.value, hi.value
