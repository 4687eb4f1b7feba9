"""Extended-precision reference of the chirp-z transform on a circle's arc
(test_czt_host.py, test_czt_gpu.py), built on exact_dft.py:

    z_k  = a_abs exp(2 pi i (a_turns + k step)),  step = step_turns / step_div
    X[k] = sum_{j<n} x[j] z_k^-j,                 k < m

with the step taken as the exact rational number. Every angle is reduced
modulo one turn in Python integers on the parameters' significands
(float.as_integer_ratio) before any sine or cosine is taken, in np.longdouble.

czt_exact: all m bins by Bluestein on a power of 2 in np.longdouble.
czt_bins: direct O(n) sums for a few bins, only there to pin czt_exact.
czt_float64: the same statement in float64 through numpy.fft with tables
rounded from the extended ones: the float64 level the GPU bound is relative to.
Nothing here calls the engine or scipy.
"""
from __future__ import annotations

import numpy as np

import exact_dft as E

LD, CLD = E.LD, E.CLD
_TWO_PI = 2 * E.PI


def defaults(n: int, m=None, step_turns=None, step_div=None):
    """(m, step_turns, step_div) as fft.CZT fills them in: the DFT grid."""
    m = int(n) if m is None else int(m)
    if step_turns is None and step_div is None:
        return m, 1.0, m
    return m, float(1.0 if step_turns is None else step_turns), int(1 if step_div is None else step_div)


def zoom_params(fn, m: int, fs: float = 2, endpoint: bool = False):
    """(a_turns, step_turns, step_div) of scipy.signal.zoom_fft(x, fn, m, fs=fs,
    endpoint=endpoint), the divisions made in float64 as fft.ZoomFFT makes them."""
    f = np.atleast_1d(np.asarray(fn, dtype=np.float64))
    f1, f2 = (0.0, float(f[0])) if f.size == 1 else (float(f[0]), float(f[1]))
    return f1 / fs, (f2 - f1) / fs, max(m - 1 if endpoint else m, 1)


def _frac_ld(r: int, den: int):
    """r / den for 0 <= r < den as a np.longdouble in [-1/2, 1/2] (modulo 1),
    within 2^-80: the quotient as an 80-bit integer, taken in two 40-bit
    halves a double holds exactly."""
    neg = 2 * r > den
    if neg:
        r = den - r
    q = (r << 80) // den
    f = (LD(float(q >> 40)) * LD(2.0 ** 40) + LD(float(q & ((1 << 40) - 1)))) * LD(2.0 ** -80)
    return -f if neg else f


def reduced_turns(mults, x: float, div: int = 1) -> np.ndarray:
    """(mult x / div) turns modulo 1 in [-1/2, 1/2] for every integer mult, x
    the exact value of the float64."""
    p, q = float(x).as_integer_ratio()
    den = q * int(div)
    return np.array([_frac_ld((int(k) * p) % den, den) for k in mults], LD)


def _cis_turns(f: np.ndarray) -> np.ndarray:
    """exp(2 pi i f) in extended precision."""
    a = f.astype(LD) * _TWO_PI
    out = np.empty(a.shape, CLD)
    out.real = np.cos(a)
    out.imag = np.sin(a)
    return out


_tables: dict = {}


def tables(n: int, m: int, F: int, a_abs=1.0, a_turns=0.0, step_turns=1.0, step_div=1):
    """(A, v, P) of the issue's factorisation in np.clongdouble: A[j] = a_abs^-j
    exp(-2 pi i j a_turns) c(j), v[d mod F] = conj(c(d)) for -(n-1) <= d <= m-1,
    P[k] = c(k), c(j) = exp(-pi i step j^2). Memoised, read-only."""
    key = (n, m, F, float(a_abs), float(a_turns), float(step_turns), int(step_div))
    if key not in _tables:
        assert F >= n + m - 1
        top = max(n, m)
        j = np.arange(top)
        fc = reduced_turns([int(i) * int(i) for i in j], step_turns, 2 * int(step_div))
        c = _cis_turns(-fc)
        fa = reduced_turns(range(n), a_turns, 1)
        mag = np.power(LD(a_abs), -np.arange(n).astype(LD)) if a_abs != 1.0 else np.ones(n, LD)
        A = mag * _cis_turns(-(fa + fc[:n]))
        v = np.zeros(F, CLD)
        v[:m] = np.conj(c[:m])
        if n > 1:
            v[F - n + 1:] = np.conj(c[1:n][::-1])
        P = c[:m].copy()
        for t in (A, v, P):
            t.setflags(write=False)
        _tables[key] = (A, v, P)
    return _tables[key]


def _length(n: int, m: int) -> int:
    return max(256, E._next_pow2(n + m - 1))


def czt_exact(x, m=None, step_turns=None, step_div=None, a_turns=0.0, a_abs=1.0) -> np.ndarray:
    """All m bins of every row of x, in extended precision."""
    x = np.atleast_2d(np.asarray(x)).astype(CLD)
    n = x.shape[1]
    m, st, sd = defaults(n, m, step_turns, step_div)
    F = _length(n, m)
    A, v, P = tables(n, m, F, a_abs, a_turns, st, sd)
    a = np.zeros((x.shape[0], F), CLD)
    a[:, :n] = x * A
    vh = E._radix2(v[None, :])[0]
    c = np.conj(E._radix2(np.conj(E._radix2(a) * vh))) / LD(F)
    return c[:, :m] * P


def czt_bins(x, ks, m=None, step_turns=None, step_div=None, a_turns=0.0, a_abs=1.0) -> np.ndarray:
    """Bins ks by the direct sum, the angle j a_turns + j k step of every term
    reduced in integers. Only there to check czt_exact."""
    x = np.atleast_2d(np.asarray(x)).astype(CLD)
    n = x.shape[1]
    m, st, sd = defaults(n, m, step_turns, step_div)
    pa, qa = float(a_turns).as_integer_ratio()
    ps, qs = float(st).as_integer_ratio()
    den = qa * qs * int(sd)
    mag = np.power(LD(a_abs), -np.arange(n).astype(LD)) if a_abs != 1.0 else np.ones(n, LD)
    out = np.empty((x.shape[0], len(ks)), CLD)
    for i, k in enumerate(ks):
        k = int(k)
        num = pa * qs * int(sd) + k * ps * qa
        f = np.array([_frac_ld((j * num) % den, den) for j in range(n)], LD)
        out[:, i] = (x * (mag * _cis_turns(-f))).sum(axis=1)
    return out


def czt_float64(x, m=None, step_turns=None, step_div=None, a_turns=0.0, a_abs=1.0) -> np.ndarray:
    """The same factorisation in float64 through numpy.fft, its tables rounded
    once from the extended ones."""
    x = np.atleast_2d(np.asarray(x))
    n = x.shape[1]
    m, st, sd = defaults(n, m, step_turns, step_div)
    F = _length(n, m)
    A, v, P = (t.astype(np.complex128) for t in tables(n, m, F, a_abs, a_turns, st, sd))
    spec = np.fft.fft(x.astype(np.complex128) * A, F, axis=1) * np.fft.fft(v)
    return np.fft.ifft(spec, axis=1)[:, :m] * P
