"""The reference of the DCT tests (test_dct_host.py, test_dct_gpu.py): types
II and III of every row, cut or zero-padded to N, under scipy's three norms,
by two routes — 80-bit through exact_dft.exact_fft (what the errors are
measured against) and float64 (the reference level the accuracy bound is
relative to: scipy.fft.dct where scipy imports, else Makhoul's statement
through numpy.fft).

80-bit, with no private function of exact_dft:
  II   y = 2 Re(FFT_4N(u)[:N]),  u[2j+1] = x[j]: the angle 2 pi k (2j+1) / (4N)
       is pi k (2j+1) / (2N)
  III  y = Re(FFT_4N(g)[1:2N:2]),  g[0] = x[0], g[k] = 2 x[k] (k < N): bin 2j+1
       of g has the angle pi k (2j+1) / (2N)
"""
import numpy as np

import exact_dft as E

NORMS = (None, "ortho", "forward")

try:
    from scipy import fft as _sfft
except ImportError:  # the float64 level then comes from numpy.fft
    _sfft = None


def padded(x, N=None):
    """The rows of x as (rows, N) float64 (np.longdouble rows stay so): cut to
    N samples or zero-padded."""
    x = np.atleast_2d(np.asarray(x))
    if x.dtype != E.LD:
        x = x.astype(np.float64)
    N = x.shape[1] if N is None else int(N)
    out = np.zeros((x.shape[0], N), x.dtype)
    k = min(N, x.shape[1])
    out[:, :k] = x[:, :k]
    return out


def _norm(norm):
    assert norm in (None, "backward", "ortho", "forward"), norm
    return "backward" if norm is None else norm


def opposite(norm):
    return {"backward": "forward", "ortho": "ortho", "forward": "backward"}[_norm(norm)]


def dct_exact(x, type=2, N=None, norm=None):
    """80-bit route: (rows, N) np.longdouble."""
    p = padded(x, N).astype(E.LD)
    rows, N = p.shape
    norm = _norm(norm)
    n2 = E.LD(2) * E.LD(N)
    f = {"backward": E.LD(1), "forward": 1 / n2, "ortho": np.sqrt(1 / n2)}[norm]
    if type == 2:
        u = np.zeros((rows, 4 * N), E.LD)
        u[:, 1:2 * N:2] = p
        y = 2 * E.exact_fft(u)[:, :N].real * f
        if norm == "ortho":
            y[:, 0] = y[:, 0] * np.sqrt(E.LD(1) / E.LD(2))
        return y
    assert type == 3, type
    g = np.zeros((rows, 4 * N), E.LD)
    g[:, :N] = 2 * p
    g[:, 0] = p[:, 0] * (np.sqrt(E.LD(2)) if norm == "ortho" else E.LD(1))
    return E.exact_fft(g)[:, 1:2 * N:2].real * f


def idct_exact(x, type=2, N=None, norm=None):
    return dct_exact(x, 5 - type, N, opposite(norm))


def _makhoul64(p, type, norm):
    rows, N = p.shape
    k = np.arange(N)
    w = np.exp(-1j * np.pi * k / (2 * N))
    f = {"backward": 1.0, "forward": 1 / (2.0 * N), "ortho": np.sqrt(1 / (2.0 * N))}[norm]
    h = (N + 1) // 2
    if type == 2:
        v = np.empty_like(p)
        v[:, :h] = p[:, 0::2]
        v[:, h:] = p[:, 1::2][:, ::-1]
        y = 2 * (np.fft.fft(v, axis=1) * w).real * f
        if norm == "ortho":
            y[:, 0] *= np.sqrt(0.5)
        return y
    q = p.copy()
    if norm == "ortho":
        q[:, 0] *= np.sqrt(2.0)
    xr = np.zeros_like(q)
    xr[:, 1:] = q[:, :0:-1]
    W = (q - 1j * xr) * np.conj(w)
    W[:, 0] = q[:, 0]
    v = np.fft.ifft(W, axis=1).real * N
    y = np.empty_like(p)
    y[:, 0::2] = v[:, :h]
    y[:, 1::2] = v[:, h:][:, ::-1]
    return y * f


def dct64(x, type=2, N=None, norm=None):
    """float64 route: scipy.fft.dct, or Makhoul through numpy.fft."""
    p = padded(x, N)
    if _sfft is not None:
        return _sfft.dct(p, type=type, axis=1, norm=_norm(norm))
    return _makhoul64(p, type, _norm(norm))


def idct64(x, type=2, N=None, norm=None):
    p = padded(x, N)
    if _sfft is not None:
        return _sfft.idct(p, type=type, axis=1, norm=_norm(norm))
    return _makhoul64(p, 5 - type, opposite(norm))


def twiddles_exact(N):
    """(cos, sin) of pi k / (2N), k < N, np.longdouble, every angle evaluated at
    most pi/4: past N/2 through the complement pi (N - k) / (2N)."""
    k = np.arange(N, dtype=np.int64)
    low = 2 * k <= N
    a = np.where(low, k, N - k).astype(E.LD) * (E.PI / E.LD(2 * N))
    c, s = np.cos(a), np.sin(a)
    return np.where(low, c, s), np.where(low, s, c)
