"""Shapes and references of test_seams_gpu.py (and test_seams_host.py, which
proves them on the CPU): the smallest calls that reach the second iteration
of a host chunk loop or the second unit of a persistent worker.

Every shape is computed here from the constants of the code it is meant for,
restated with the place they come from; gdsp_loop_stats then tells the GPU
test whether the call really crossed its seam, so a constant restated wrongly
fails the test instead of passing it on the first iteration.

Reference for the Welch family: numpy's rfft of the exact windowed segments
(a strided view of the signal, in chunks), |.|^2 or conj(X) Y summed per bin
in np.longdouble and rounded to float64 once. float64 rfft is good to about
1e-16 of a segment's largest bin and the errors of different segments do not
add up coherently, so the sums are far inside the 1e-13 they are compared at;
test_seams_host.py holds this reference to exact_dft.exact_pwelch at 1e-15.
"""
from collections import namedtuple

import numpy as np

LD = np.longdouble
EXACT = 1e-13  # test_segment_ranges_gpu.EXACT, test_guard_bands_gpu.EXACT, test_fir_gpu.EXACT

WMUL = 2048                  # welch.hip: at most 2048 workers per workgroup slot (wmul)
MAT_BYTES_LOG2 = 25          # welch.hip: 2^25 complex128 (512 MiB) of rows per chunk
KRPP = 64                    # welch.hip: rows per part of the partial sums (kRpp)
GRID_LIMIT = 65535           # a grid's y / z extent
PARTIALS_LOG2 = 26           # welch.hip channels_per_launch: 2^26 doubles of partials
FIR_CHUNK_LOG2 = 24          # gdsp_api.hip fir_chunk_rows: 2^24 complex128 per chunk
ZERO_COPY_MAX = 512 << 10    # gdsp_api.hip kZeroCopyMax: in + out bytes of one call
STAGING_HALF = 8 << 20       # gdsp_api.hip: bytes of one pinned staging half

# The fused Pwelch's own radix lists of the lengths used here
# (GDSP_SPEC_GROUP(specspw), fft_specs0.hip); the plan reports the FFT's list.
PW_LISTS = {3000: (15, 5, 5, 8), 6000: (15, 5, 5, 16)}


def pow2_tpw(f):
    """Geo<log2 f>::TPW (fft_device.hpp): 256 threads, f / 16 per transform."""
    return max(1, 256 // max(1, f // 16))


def hamming(n):
    """No zero at the ends, so a segment's first and last sample count."""
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / (n - 1))


def segments(x, nfft, stride, a, b):
    """Segments [a, b) of x as a read-only strided view, a row each."""
    x = np.ascontiguousarray(x)
    assert a >= 0 and b >= a and (b == a or (b - 1) * stride + nfft <= len(x))
    return np.lib.stride_tricks.as_strided(x[a * stride:], (b - a, nfft),
                                           (stride * x.itemsize, x.itemsize), writeable=False)


def _chunks(count, flen):
    step = max(1, (1 << 22) // flen)  # 2^22 points of spectra at a time
    return [(lo, min(lo + step, count)) for lo in range(0, count, step)]


def welch_sums(x, nfft, flen, stride, a, b, win):
    """sum over segments s in [a, b) of |FFT_flen(win x_s, zero-padded)[j]|^2,
    j = 0 .. flen / 2, summed in extended precision (np.longdouble, flen / 2 +
    1 entries). What gdsp_pwelch_finalize reads: 0.5 (acc[j] + acc[flen - j])."""
    segs = segments(x, nfft, stride, a, b)
    w = np.asarray(win)[:nfft]
    total = np.zeros(flen // 2 + 1, LD)
    for lo, hi in _chunks(b - a, flen):
        spec = np.fft.rfft(segs[lo:hi] * w, n=flen, axis=1)
        total += (spec.real * spec.real + spec.imag * spec.imag).sum(axis=0, dtype=LD)
    return total


def cross_sums(x, y, nfft, flen, stride, a, b, win):
    """The four planes of gdsp_cpsd_batch_accumulate_device for one channel:
    Sxx, Syy, Re Sxy, Im Sxy with Sxy = sum conj(X_s) Y_s, flen / 2 + 1 bins
    each, in extended precision."""
    sx, sy = segments(x, nfft, stride, a, b), segments(y, nfft, stride, a, b)
    w = np.asarray(win)[:nfft]
    out = np.zeros((4, flen // 2 + 1), LD)
    for lo, hi in _chunks(b - a, flen):
        X = np.fft.rfft(sx[lo:hi] * w, n=flen, axis=1)
        Y = np.fft.rfft(sy[lo:hi] * w, n=flen, axis=1)
        out[0] += (X.real * X.real + X.imag * X.imag).sum(axis=0, dtype=LD)
        out[1] += (Y.real * Y.real + Y.imag * Y.imag).sum(axis=0, dtype=LD)
        out[2] += (X.real * Y.real + X.imag * Y.imag).sum(axis=0, dtype=LD)
        out[3] += (X.real * Y.imag - X.imag * Y.real).sum(axis=0, dtype=LD)
    return out


def unfold(half, flen):
    """The flen entries 0.5 (acc[j] + acc[(flen - j) mod flen]) from the
    flen / 2 + 1 sums of a real signal."""
    j = np.arange(flen)
    return np.asarray(half)[..., np.minimum(j, flen - j)]


def fold(acc):
    acc = np.asarray(acc)
    f = acc.shape[-1]
    return 0.5 * (acc + acc[..., (f - np.arange(f)) % f])


def finalize(total, nsegs, nfft, pad, win_nfft, fs):
    """gdsp_pwelch_finalize on the sums of welch_sums, in their precision."""
    lp = pad // 2 + 1
    j = np.arange(lp)
    w = np.asarray(win_nfft).astype(LD)
    norm = (w * w).sum() * LD(fs)
    cj = np.where((j > 0) & (j < lp - 1), 2, 1).astype(LD)
    return cj * np.asarray(total)[:lp] / LD(nsegs) / norm


def signal_len(nseg, nfft, stride):
    return (nseg - 1) * stride + nfft


def noise(seed, *shape):
    return np.random.default_rng(seed).uniform(-1, 1, shape)


# ---- A. worker loops: npairs = target + 1, so ppw = 2 and the last worker one pair ----
# path as test_segment_ranges_gpu.Case (its _assert_path checks the branch);
# tpw: workers per workgroup, None where it comes from the plan's radix list
W = namedtuple("W", "path nfft stride pad flags tpw", defaults=((), None))


def worker_cases():
    cs = [W("generic", 16, 3, 0, (), pow2_tpw(16)), W("generic", 32, 3, 0, (), pow2_tpw(32)),
          W("generic", 8192, 3, 0, (), pow2_tpw(8192)),
          W("generic", 16384, 3, 0, (), pow2_tpw(16384)),
          W("generic", 4000, 3, 4096, (), pow2_tpw(4096)),
          W("half", 32, 16, 0, (), pow2_tpw(32)), W("row", 4096, 2048, 0, (), pow2_tpw(4096)),
          W("half", 8192, 4096, 0, (), pow2_tpw(8192)),
          W("half", 16384, 8192, 0, (), pow2_tpw(16384)),
          W("rowg", 4096, 3, 0, (), pow2_tpw(4096))]
    # (12 has no compiled list: the planner compiles one at run time, and the
    # fused Pwelch runs on it as on a compiled one)
    for n in (12, 480, 2000, 3000, 3200, 6000):
        path = "pw-list" if n in PW_LISTS else "hiprtc" if n == 12 else "fft-list"
        cs += [W(path, n, 3, 0), W(path, n, n // 2, 0)]
    cs += [W("hiprtc", 2275, 3, 0), W("hiprtc", 810, 3, 0)]
    # launch_pwelch_mixed: wmul workers, one per workgroup slot (welch.hip)
    cs += [W("runtime-radix", 1000, 3, 0, ("GENERIC_MIXED",), 1)]
    return cs


def worker_id(c):
    return "-".join([c.path, str(c.nfft), "s%d" % c.stride, str(c.pad)] + list(c.flags))


def worker_nseg(tpw):
    """An odd count: target + 1 pairs, the last of one segment."""
    return 2 * (WMUL * tpw + 1) - 1


# The wave kernels (pwelch_wave_geometry, pwelch_wave.hip) take pair groups of
# S = 64 / (F / 16) pairs (1 from F = 2048), `target` workers: 1024 two-wave
# workers at 2048, else 2048 (3072 at half overlap from F = 128: not here).
def wave_groups(f):
    t = f // 16
    return (64 // t if t <= 64 else 1), (2048 if t <= 64 else 1024)


def wave_nseg(f):
    """ngroups = target + 1 (gpw = 2), the last group of one pair of one segment."""
    s, target = wave_groups(f)
    return 2 * (target * s + 1) - 1


# ---- B. chunk loops -----------------------------------------------------------------
def materialised_rows(flen, npairs):
    """Pairs per chunk of the materialised Pwelch (welch.hip)."""
    return min(max(1, (1 << MAT_BYTES_LOG2) // flen), GRID_LIMIT * KRPP, npairs)


# name, nfft, noverlap, pad, segments
M = namedtuple("M", "name nfft nov pad nseg")
MATERIALISED = [
    # (a) kind 2 at Pad 32768: 2^25 / 32768 = 1024 pairs a chunk; 2049 + 2 segments are 1026
    M("a-pad32768", 100, 99, 32768, 2049 + 2),
    # (b) the grid-limit cap: 2^25 / 8 = 4194304 pairs > 65535 * 64 = 4194240, one pair more
    M("b-grid-limit", 8, 6, 0, 2 * (GRID_LIMIT * KRPP + 1) - 1),
    # (c) a prime (chirp-z): 2^25 / 1031 = 32545 pairs a chunk, one pair more
    M("c-prime1031", 1031, 1031 - 8, 0, 2 * (((1 << MAT_BYTES_LOG2) // 1031) + 1) - 1),
]

LARGEST_NSEG = max([m.nseg for m in MATERIALISED] +
                   [worker_nseg(c.tpw) for c in worker_cases() if c.tpw])
