"""Extended-precision reference for the accuracy tests (test_accuracy_host.py,
test_accuracy_gpu.py, scripts/measure_accuracy.py).

Everything here is numpy in np.longdouble / np.clongdouble, the x86 80-bit
type (64-bit significand, eps 1.08e-19): about 2000 times finer than the
float64 results it judges, so a float64 transform's own rounding error is
measured, in units of u = 2**-53, instead of being compared with another
float64 transform's.

exact_fft: recursive radix-2 for powers of 2, Bluestein on a power of 2 for
every other length with the chirp angle reduced in integers ((k*k) % (2n)
before the multiplication by pi/n, the reduction fft/bluestein.go:53 lacks).
exact_bins: direct O(n) sums for a few bins, to check exact_fft.

The module also holds what the accuracy tests share: the standard rows of a
length, the error metric err_u, the bound check() and the record of what it
measured.
"""
from __future__ import annotations

import numpy as np
import pytest

LD = np.longdouble
CLD = np.clongdouble

if np.finfo(LD).eps != LD(2) ** -63:
    pytest.skip("np.longdouble is not the x86 80-bit type here (eps %g): no extended-precision "
                "reference" % float(np.finfo(LD).eps), allow_module_level=True)

U = 2.0 ** -53            # unit roundoff of float64
MARGIN = 16               # err_u(kernel) <= MARGIN * err_u(float64 reference)
PI = LD("3.14159265358979323846264338327950288")
assert abs(4 * np.arctan(LD(1)) - PI) <= 2 * np.finfo(LD).eps


def _is_pow2(n: int) -> bool:
    return n > 0 and n & (n - 1) == 0


def _next_pow2(n: int) -> int:
    m = 1
    while m < n:
        m *= 2
    return m


def _cis(num: np.ndarray, den: int) -> np.ndarray:
    """exp(-i * pi * num / den) for int64 num, cos/sin of extended arguments."""
    a = num.astype(LD) * (PI / LD(den))
    out = np.empty(a.shape, CLD)
    out.real = np.cos(a)
    out.imag = -np.sin(a)
    return out


_tw: dict = {}


def _twiddles(n: int) -> np.ndarray:
    """exp(-2 pi i k / n), k < n / 2."""
    if n not in _tw:
        _tw[n] = _cis(2 * np.arange(n // 2, dtype=np.int64), n)
    return _tw[n]


def _radix2(x: np.ndarray) -> np.ndarray:
    """Recursive decimation in time; the even and the odd half go down as one
    array of twice the rows, so a call per level is all the Python there is."""
    rows, n = x.shape
    if n == 1:
        return x.copy()
    y = _radix2(np.concatenate([x[:, 0::2], x[:, 1::2]], axis=0))
    e, o = y[:rows], y[rows:] * _twiddles(n)
    return np.concatenate([e + o, e - o], axis=1)


_chirp: dict = {}


def _bluestein_tables(n: int):
    if n not in _chirp:
        k = np.arange(n, dtype=np.int64)
        w = _cis((k * k) % (2 * n), n)          # exp(-i pi k^2 / n), angle reduced exactly
        m = _next_pow2(2 * n - 1)
        b = np.zeros(m, CLD)
        b[:n] = np.conj(w)
        b[m - n + 1:] = np.conj(w[1:][::-1])
        _chirp[n] = (w, m, _radix2(b[None, :])[0])
    return _chirp[n]


def exact_fft(x, inverse: bool = False) -> np.ndarray:
    """The DFT (inverse: the 1/n-scaled inverse DFT) of every row of a 2-D
    array, in extended precision."""
    x = np.asarray(x)
    assert x.ndim == 2
    x = x.astype(CLD)
    n = x.shape[1]
    if n == 0:
        return x
    if inverse:
        return np.conj(exact_fft(np.conj(x))) / LD(n)
    if _is_pow2(n):
        return _radix2(x)
    w, m, bhat = _bluestein_tables(n)
    a = np.zeros((x.shape[0], m), CLD)
    a[:, :n] = x * w
    c = np.conj(_radix2(np.conj(_radix2(a) * bhat))) / LD(m)
    return c[:, :n] * w


def exact_bins(x, ks) -> np.ndarray:
    """Bins ks of the forward DFT of every row of x by the direct sum, the
    exponent (j * k) % n reduced in int64. Only there to check exact_fft."""
    x = np.asarray(x).astype(CLD)
    n = x.shape[1]
    j = np.arange(n, dtype=np.int64)
    out = np.empty((x.shape[0], len(ks)), CLD)
    for i, k in enumerate(ks):
        out[:, i] = (x * _cis(2 * ((j * int(k)) % n), n)).sum(axis=1)
    return out


def exact_fftn(x, dims=None, inverse: bool = False) -> np.ndarray:
    """exact_fft along every axis of x (reshaped to dims where given)."""
    x = np.asarray(x).astype(CLD)
    if dims is not None:
        x = x.reshape(tuple(int(d) for d in dims))
    for ax in range(x.ndim):
        x = exact_fft_axis(x, ax, inverse)
    return x


def exact_fft_axis(x, axis: int, inverse: bool = False) -> np.ndarray:
    x = np.moveaxis(np.asarray(x).astype(CLD), axis, -1)
    y = exact_fft(x.reshape(-1, x.shape[-1]), inverse).reshape(x.shape)
    return np.moveaxis(y, -1, axis)


def exact_convolve(x, y) -> np.ndarray:
    """fft.Convolve (fft/fft.go:55-69) of the rows of x with y (one row for
    all, or row by row)."""
    return exact_fft(exact_fft(x) * exact_fft(np.atleast_2d(y)), inverse=True)


def segment_count(lx: int, size: int, noverlap: int) -> int:
    """spectral.Segment's count (spectral/spectral.go:22-33; gdsp_segment_count)."""
    stride = size - noverlap
    assert stride > 0
    return 0 if lx < size else (lx - size) // stride + 1


def _pwelch(x, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off, real, fft):
    """spectral/pwelch.go:74-145 in the type `real`, transforms by `fft`."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size < nfft:
        x = np.concatenate([x, np.zeros(nfft - x.size)])
    flen, lp = max(pad, nfft), pad // 2 + 1
    nsegs = segment_count(x.size, nfft, noverlap)
    stride = nfft - noverlap
    segs = np.zeros((nsegs, flen), real)
    for s in range(nsegs):
        segs[s, :nfft] = x[s * stride:s * stride + nfft]
    spec = fft(segs * np.asarray(win_seg, dtype=np.float64).astype(real)[None, :])
    acc = (spec.real * spec.real + spec.imag * spec.imag).sum(axis=0)
    w = np.asarray(win_nfft, dtype=np.float64).astype(real)
    norm = (w * w).sum()
    if not scale_off:
        norm = norm * real(fs)
    j = np.arange(lp)
    # gdsp_pwelch_finalize: pxx[j] = c_j (acc[j] + acc[(flen - j) % flen]) / 2 / nsegs / norm
    c = np.where((j > 0) & (j < lp - 1), 2, 1).astype(real)
    if nsegs == 0:
        return np.zeros(lp, real)
    return c * (acc[j] + acc[(flen - j) % flen]) / real(2) / real(nsegs) / norm


def exact_pwelch(x, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off=False) -> np.ndarray:
    """spectral.Pwelch's Pxx in extended precision from the float64 window
    tables win_seg (max(pad, nfft) entries) and win_nfft (nfft entries)."""
    return _pwelch(x, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off, LD, exact_fft)


def numpy_pwelch(x, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off=False) -> np.ndarray:
    """The same statement in float64 through numpy.fft: the float64 reference
    level of Pwelch."""
    return _pwelch(x, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off, np.float64,
                   lambda s: np.fft.fft(s, axis=1))


# ---- the metric -------------------------------------------------------------

def err_u(y, ex) -> float:
    """Per row max_k |y_k - ex_k| / max_k |ex_k|, the largest row, in units of
    u = 2**-53. Elementwise, so one bad bin cannot hide in a norm; relative to
    the row's largest exact output, so impulse, tone and noise rows are on one
    scale."""
    ex = np.asarray(ex)
    ex = ex.reshape(-1, ex.shape[-1]) if ex.ndim > 1 else ex.reshape(1, -1)
    y = np.asarray(y).reshape(ex.shape)
    d = np.abs(y.astype(ex.dtype) - ex).max(axis=1)
    top = np.abs(ex).max(axis=1)
    assert np.all(top > 0)
    return float((d / top).max() / LD(U))


def err_u_all(y, ex) -> float:
    """err_u with the whole array as one row (FFT2 / FFTN results)."""
    return err_u(np.asarray(y).reshape(1, -1), np.asarray(ex).reshape(1, -1))


def err_u_per_bin(p, ex) -> float:
    """max_k |p_k - ex_k| / ex_k in u: Pwelch's second metric."""
    ex = np.asarray(ex).reshape(-1)
    p = np.asarray(p).reshape(-1)
    assert np.all(ex > 0)
    return float((np.abs(p.astype(ex.dtype) - ex) / ex).max() / LD(U))


# ---- the standard rows and their memoised exact results --------------------------

def uniform_rows(seed: int, batch: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (batch, n)) + 1j * rng.uniform(-1, 1, (batch, n))


_rows: dict = {}


def standard_rows(n: int) -> np.ndarray:
    """The five rows of length n, rng seeded by n: complex noise; real noise;
    an impulse 1-2j at an odd index near 3n/7; the tone of bin n // 3 (phase
    index reduced mod n in integers) plus 1e-3 of row 0; row 0 again (batch 5
    leaves a ragged last workgroup). Read-only."""
    if n not in _rows:
        rng = np.random.default_rng(n)
        x = np.zeros((5, n), np.complex128)
        x[0] = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
        x[1] = rng.uniform(-1, 1, n)
        x[2, min(n - 1, (3 * n // 7) | 1)] = 1 - 2j
        j = np.arange(n, dtype=np.int64)
        ph = 2 * np.pi * ((j * (n // 3)) % n) / n
        x[3] = np.cos(ph) + 1j * np.sin(ph) + 1e-3 * x[0]
        x[4] = x[0]
        x.setflags(write=False)
        _rows[n] = x
    return _rows[n]


_memo: dict = {}


def memo(key, fn):
    """Exact results are computed once per key and shared (read-only) by the
    forward, inverse, real and flag variants of a family."""
    if key not in _memo:
        v = fn()
        v.setflags(write=False)
        _memo[key] = v
    return _memo[key]


def exact_standard(n: int, inverse: bool = False, real: bool = False, rows=None) -> np.ndarray:
    """exact_fft of the standard rows (real: of the real parts of rows 0-2),
    or of the listed rows, each row computed once per (n, direction, real)."""
    rows = tuple(range(3 if real else 5)) if rows is None else tuple(rows)
    src = [0 if r == 4 else r for r in rows]  # row 4 is row 0
    todo = sorted(r for r in set(src) if ("std", n, inverse, real, r) not in _memo)
    if todo:
        x = standard_rows(n)
        y = exact_fft((x.real if real else x)[todo], inverse)
        for r, v in zip(todo, y):
            memo(("std", n, inverse, real, r), lambda v=v: v.copy())
    return np.stack([_memo[("std", n, inverse, real, r)] for r in src])


def input_rows(n: int, real: bool = False, rows=None) -> np.ndarray:
    """The inputs exact_standard(n, ..., real, rows) transforms, as a fresh
    contiguous float64 / complex128 array."""
    rows = tuple(range(3 if real else 5)) if rows is None else tuple(rows)
    x = standard_rows(n)
    return np.ascontiguousarray((x.real if real else x)[list(rows)])


# ---- the bound and the record ---------------------------------------------------

RECORDS: list = []


def check(family: str, n, variant: str, got: float, e_ref: float, margin: float = MARGIN,
          record: bool = True):
    """The accuracy bound of every case: `got` (err_u of the code under test)
    against `e_ref` (err_u of the float64 reference of the same operation on
    the same rows, measured in the same run). Prints and records the
    measurement, then asserts."""
    ratio = got / e_ref if e_ref > 0 else (0.0 if got == 0 else float("inf"))
    if record:  # (a negative control is no measurement of the engine)
        RECORDS.append({"family": family, "n": n, "variant": variant,
                        "err_u": round(got, 3), "e_ref": round(e_ref, 3),
                        "ratio": round(ratio, 3), "margin": margin})
    print("accuracy: %s n=%s %s err_u=%.3g e_ref=%.3g ratio=%.3g (margin %g)"
          % (family, n, variant, got, e_ref, ratio, margin))
    assert got <= margin * e_ref, \
        "%s n=%s %s: %.4g u against %.4g u of the float64 reference (x%.3g > %g)" \
        % (family, n, variant, got, e_ref, ratio, margin)
