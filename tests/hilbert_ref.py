"""The reference of the Hilbert tests (test_hilbert_host.py,
test_hilbert_gpu.py): h = IFFT_N(m FFT_N(x)) of every row, cut or zero-padded
to N, by two routes — float64 through numpy.fft (the float64 reference level
the accuracy bound is relative to; scipy.signal.hilbert where scipy imports is
the same arithmetic) and 80-bit through exact_dft.exact_fft (what the errors
are measured against).
"""
import numpy as np

import exact_dft as E


def padded(x, N=None):
    """The rows of x as (rows, N) float64: cut to N samples or zero-padded."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    N = x.shape[1] if N is None else int(N)
    out = np.zeros((x.shape[0], N))
    k = min(N, x.shape[1])
    out[:, :k] = x[:, :k]
    return out


def multiplier(N):
    """m[f]: -i for 0 < f < N/2, +i for N/2 < f < N, 0 at f = 0 and f = N/2."""
    f = np.arange(N)
    m = np.zeros(N, np.complex128)
    m[(f > 0) & (2 * f < N)] = -1j
    m[2 * f > N] = 1j
    return m


def quadrature64(x, N=None):
    """float64 route: numpy FFT, multiplier, IFFT; (rows, N) float64."""
    p = padded(x, N)
    return np.fft.ifft(np.fft.fft(p, axis=1) * multiplier(p.shape[1])[None, :], axis=1).real


def analytic64(x, N=None):
    return padded(x, N) + 1j * quadrature64(x, N)


def quadrature_exact(x, N=None):
    """80-bit route: (rows, N) np.longdouble."""
    p = padded(x, N)
    m = multiplier(p.shape[1]).astype(E.CLD)
    return E.exact_fft(E.exact_fft(p) * m[None, :], inverse=True).real
