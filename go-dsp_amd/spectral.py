"""Host mirror of go-dsp's `spectral` package (spectral/pwelch.go,
spectral/spectral.go). Pwelch runs the fused GPU kernel (window +
packed-pair FFT + |X|^2 accumulation) through gdsp_pwelch."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, NamedTuple, Optional

import numpy as np

from . import _lib, window
from ._lib import Panic, check, lib


@dataclass
class PwelchOptions:
    """spectral/pwelch.go:28-65 (zero values select the defaults)."""
    NFFT: int = 0
    Window: Optional[Callable[[int], np.ndarray]] = None
    Pad: int = 0
    Noverlap: int = 0
    Scale_off: bool = False


def _p(a: np.ndarray):
    return a.ctypes.data_as(_lib._P)


def segment_count(lx: int, size: int, noverlap: int) -> int:
    """Segment count of spectral.Segment (spectral/spectral.go:22-33)."""
    c = _lib._I64(0)
    check(lib().gdsp_segment_count(lx, size, noverlap, c), "Segment")
    return int(c.value)


def Segment(x, size: int, noverlap: int):
    """spectral.Segment — spectral/spectral.go:22-47: copies of each segment
    (the GPU path never materialises them; this is the host API)."""
    x = np.asarray(x, dtype=np.float64)
    n = segment_count(x.size, size, noverlap)
    stride = size - noverlap
    return [x[i * stride:i * stride + size].copy() for i in range(n)]


def resolve_options(o: Optional[PwelchOptions]):
    """Defaults of spectral/pwelch.go:79-95; a nil options pointer panics."""
    if o is None:
        raise Panic(_lib.GDSP_ERR_INVALID,
                    "runtime error: invalid memory address or nil pointer dereference")
    nfft = o.NFFT or 256
    pad = o.Pad or nfft
    wf = o.Window or window.Hann
    return nfft, pad, o.Noverlap, wf, not o.Scale_off


def _welch_args(o: Optional[PwelchOptions]):
    """(nfft, pad, noverlap, win_seg, win_nfft, lp, scale_off) of a Welch call:
    the resolved options, the window at max(pad, nfft) and at nfft, Pad / 2 + 1
    and the C ABI's scale_off. Callers return on an empty input before this."""
    nfft, pad, noverlap, wf, scaling = resolve_options(o)
    win_seg = np.ascontiguousarray(wf(max(pad, nfft)), dtype=np.float64)
    win_nfft = np.ascontiguousarray(wf(nfft), dtype=np.float64)
    return nfft, pad, noverlap, win_seg, win_nfft, pad // 2 + 1, int(not scaling)


def Pwelch(x, Fs: float, o: Optional[PwelchOptions]):
    """spectral.Pwelch — spectral/pwelch.go:74-145. Returns (Pxx, freqs)."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    if x.size == 0:
        return np.zeros(0), np.zeros(0)
    nfft, pad, noverlap, win_seg, win_nfft, lp, scale_off = _welch_args(o)
    pxx = np.empty(lp, np.float64)
    freqs = np.empty(lp, np.float64)
    lpo = _lib._I64(0)
    check(lib().gdsp_pwelch(_p(x), x.size, float(Fs), nfft, pad, noverlap, _p(win_seg),
                            _p(win_nfft), scale_off, _p(pxx), _p(freqs), lpo), "Pwelch")
    return pxx[:lpo.value], freqs[:lpo.value]


def _rows(rows):
    """A (channels, n) float64 array of equal-length rows, or the ragged panic."""
    if isinstance(rows, np.ndarray) and rows.ndim == 2:
        return np.ascontiguousarray(rows, dtype=np.float64)
    rs = [np.asarray(r, dtype=np.float64).reshape(-1) for r in rows]
    if any(r.size != rs[0].size for r in rs):
        raise Panic(_lib.GDSP_ERR_RAGGED, "ragged input array")
    return np.ascontiguousarray(rs, dtype=np.float64).reshape(len(rs), rs[0].size if rs else 0)


def pwelch_batch_fused(channels: int, n: int, nfft: int = 0, pad: int = 0,
                       noverlap: int = 0) -> bool:
    """Whether a batched Pwelch of this shape runs the kernel over all
    channels (True) or the loop over the channels (gdsp_pwelch_batch_fused)."""
    return bool(lib().gdsp_pwelch_batch_fused(int(channels), int(n), int(nfft), int(pad),
                                              int(noverlap)))


def PwelchBatch(rows, Fs: float, o: Optional[PwelchOptions]):
    """spectral.Pwelch of every row of `rows` (equal lengths: the channels of
    a recording) in one call (gdsp_pwelch_batch). Returns (Pxx[channels, lp],
    freqs); row c equals Pwelch(rows[c], Fs, o)."""
    x = _rows(rows)
    channels, n = x.shape
    if n == 0:  # pwelch.go:75-77, before the options are looked at
        return np.zeros((channels, 0)), np.zeros(0)
    nfft, pad, noverlap, win_seg, win_nfft, lp, scale_off = _welch_args(o)
    pxx = np.empty((channels, lp), np.float64)
    freqs = np.empty(lp, np.float64)
    lpo = _lib._I64(0)
    check(lib().gdsp_pwelch_batch(_p(x), channels, n, n, float(Fs), nfft, pad, noverlap,
                                  _p(win_seg), _p(win_nfft), scale_off, _p(pxx),
                                  _p(freqs), lpo), "PwelchBatch")
    return pxx, freqs


class CrossSpectra(NamedTuple):
    """What CpsdBatch / device.cpsd_batch return: row c of Pxy, Pxx, Pyy and
    Cxy belongs to x row c against its y."""
    Pxy: Any
    Pxx: Any
    Pyy: Any
    Cxy: Any
    freqs: Any


def cpsd_batch_fused(channels: int, n: int, nfft: int = 0, pad: int = 0,
                     noverlap: int = 0) -> bool:
    """Whether cross spectra of this shape run the fused kernel over all
    channels (True) or the materialised form (gdsp_cpsd_batch_fused)."""
    return bool(lib().gdsp_cpsd_batch_fused(int(channels), int(n), int(nfft), int(pad),
                                            int(noverlap)))


def CpsdBatch(x_rows, y, Fs: float, o: Optional[PwelchOptions]) -> CrossSpectra:
    """Welch cross spectra of every row of `x_rows` (equal lengths n) against
    y: one row of n for all, or an array of x_rows' shape, row by row
    (gdsp_cpsd_batch). Options, segments, windows, scaling and freqs are
    Pwelch's. With X_s, Y_s the windowed spectra of segment s,
    Pxy = c_j sum_s conj(X_s) Y_s / nsegs / norm (complex; MATLAB cpsd's and
    scipy.signal.csd's sign), Pxx and Pyy the same of |X_s|^2 and |Y_s|^2, so
    Pxx row c equals Pwelch(x_rows[c], Fs, o), and Cxy = |Sxy|^2 / (Sxx Syy),
    the magnitude-squared coherence (mscohere, scipy.signal.coherence). Cxy is
    the plain quotient: NaN in a bin that holds no power. One transform carries
    a segment of x and of y; y's is packed times a power of 2 chosen from that
    segment's two levels and taken out again exactly, so a difference in level
    between the signals costs neither of them digits (include/gdsp_fft.h)."""
    x = _rows(x_rows)
    channels, n = x.shape
    try:
        yy = np.ascontiguousarray(y, dtype=np.float64)
    except ValueError:  # a ragged y
        raise Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size") from None
    if yy.shape != (n,) and yy.shape != (channels, n):
        raise Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    if n == 0:  # pwelch.go:75-77, before the options are looked at
        e = np.zeros((channels, 0))
        return CrossSpectra(e.astype(np.complex128), e, e.copy(), e.copy(), np.zeros(0))
    nfft, pad, noverlap, win_seg, win_nfft, lp, scale_off = _welch_args(o)
    pxy = np.empty((channels, lp), np.complex128)
    pxx, pyy, coh = (np.empty((channels, lp), np.float64) for _ in range(3))
    freqs = np.empty(lp, np.float64)
    lpo = _lib._I64(0)
    check(lib().gdsp_cpsd_batch(_p(x), n, _p(yy), n, 1 if yy.ndim == 1 else channels, channels, n,
                                float(Fs), nfft, pad, noverlap, _p(win_seg), _p(win_nfft),
                                scale_off, _p(pxy), _p(pxx), _p(pyy), _p(coh), _p(freqs),
                                lpo), "CpsdBatch")
    return CrossSpectra(pxy, pxx, pyy, coh, freqs)


def _one_pair(x, y):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.size != y.size:
        raise Panic(_lib.GDSP_ERR_UNEQUAL, "arrays not of equal size")
    return x.reshape(1, -1), y


def Cpsd(x, y, Fs: float, o: Optional[PwelchOptions]):
    """The Welch cross power spectral density of two signals of equal length
    (MATLAB cpsd, scipy.signal.csd): CpsdBatch of one row. Returns (Pxy,
    freqs); Cpsd(x, x) is Pwelch(x)."""
    x, y = _one_pair(x, y)
    r = CpsdBatch(x, y, Fs, o)
    return r.Pxy[0], r.freqs


def Coherence(x, y, Fs: float, o: Optional[PwelchOptions]):
    """The magnitude-squared coherence |Pxy|^2 / (Pxx Pyy) of two signals of
    equal length (MATLAB mscohere, scipy.signal.coherence). Returns (Cxy,
    freqs); NaN in a bin that holds no power."""
    x, y = _one_pair(x, y)
    r = CpsdBatch(x, y, Fs, o)
    return r.Cxy[0], r.freqs


# elements of the device output of one StftBatch / SpectrogramBatch call: longer
# results are computed as ranges of segments (include/gdsp_fft.h, gdsp_stft_batch)
STFT_CHUNK_ELEMS = 1 << 25


def stft_batch_fused(channels: int, n: int, nfft: int = 0, pad: int = 0,
                     noverlap: int = 0) -> bool:
    """Whether per-segment spectra of this shape run the fused kernel over all
    channels (True) or the materialised form (gdsp_stft_batch_fused)."""
    return bool(lib().gdsp_stft_batch_fused(int(channels), int(n), int(nfft), int(pad),
                                            int(noverlap)))


def stft_freqs(pad: int, Fs: float) -> np.ndarray:
    """Pwelch's frequencies of the Pad / 2 + 1 bins (pwelch.go:138-142)."""
    return np.arange(pad // 2 + 1, dtype=np.float64) * (float(Fs) / float(pad))


def stft_times(seg_begin: int, seg_end: int, nfft: int, noverlap: int, Fs: float) -> np.ndarray:
    """The centres of segments [seg_begin, seg_end) in seconds: (s * stride +
    NFFT / 2) / Fs, the convention of scipy.signal.spectrogram."""
    s = np.arange(seg_begin, seg_end, dtype=np.int64) * (nfft - noverlap)
    return (s.astype(np.float64) + 0.5 * nfft) / float(Fs)


def StftBatch(rows, Fs: float, o: Optional[PwelchOptions]):
    """The short-time Fourier transform of every row of `rows` (equal lengths)
    in one call (gdsp_stft_batch). Options, segments and the window are
    Pwelch's. Returns (X[channels, nsegs, lp] complex128, freqs, times): X[c, s]
    is the first lp = Pad / 2 + 1 bins of the transform of segment s of row c,
    windowed and zero-padded to max(Pad, NFFT) — pwelch.go:111's pgram —
    unscaled; times are the segments' centres."""
    x = _rows(rows)
    channels, n = x.shape
    if n == 0:  # pwelch.go:75-77, before the options are looked at
        return np.zeros((channels, 0, 0), np.complex128), np.zeros(0), np.zeros(0)
    nfft, pad, noverlap, win_seg, _, lp, _ = _welch_args(o)
    nsegs = segment_count(max(n, nfft), nfft, noverlap)
    out = np.empty((channels, nsegs, lp), np.complex128)
    nso, lpo = _lib._I64(0), _lib._I64(0)
    check(lib().gdsp_stft_batch(_p(x), channels, n, n, nfft, pad, noverlap, _p(win_seg), _p(out),
                                nso, lpo), "StftBatch")
    return out, stft_freqs(pad, Fs), stft_times(0, nsegs, nfft, noverlap, Fs)


def SpectrogramBatch(rows, Fs: float, o: Optional[PwelchOptions]):
    """The spectrogram of every row of `rows` (equal lengths) in one call
    (gdsp_spectrogram_batch). Returns (P[channels, nsegs, lp] float64, freqs,
    times): P[c, s, j] = c_j |X[c, s, j]|^2 / norm of StftBatch's X with
    Pwelch's scaling, so P[c].mean(axis=0) is Pwelch(rows[c], Fs, o)."""
    x = _rows(rows)
    channels, n = x.shape
    if n == 0:  # pwelch.go:75-77, before the options are looked at
        return np.zeros((channels, 0, 0)), np.zeros(0), np.zeros(0)
    nfft, pad, noverlap, win_seg, win_nfft, lp, scale_off = _welch_args(o)
    nsegs = segment_count(max(n, nfft), nfft, noverlap)
    out = np.empty((channels, nsegs, lp), np.float64)
    freqs = np.empty(lp, np.float64)
    times = np.empty(nsegs, np.float64)
    nso, lpo = _lib._I64(0), _lib._I64(0)
    check(lib().gdsp_spectrogram_batch(_p(x), channels, n, n, float(Fs), nfft, pad, noverlap,
                                       _p(win_seg), _p(win_nfft), scale_off, _p(out), _p(freqs),
                                       _p(times), nso, lpo), "SpectrogramBatch")
    return out, freqs, times


def Stft(x, Fs: float, o: Optional[PwelchOptions]):
    """The short-time Fourier transform of one signal (MATLAB stft,
    scipy.signal.stft without its scaling): StftBatch of one row. Returns
    (X[nsegs, lp], freqs, times)."""
    X, freqs, times = StftBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), Fs, o)
    return X[0], freqs, times


# complex elements of the device copy of X in one IstftBatch call: longer inputs
# are inverted as ranges of samples (include/gdsp_fft.h, gdsp_istft_batch)
ISTFT_CHUNK_ELEMS = 1 << 25


def istft_batch_fused(channels: int, nsegs: int, nfft: int = 0, pad: int = 0,
                      noverlap: int = 0) -> bool:
    """Whether the inverse of per-segment spectra of this shape runs the fused
    overlap-add kernel (True) or the materialised form (gdsp_istft_batch_fused)."""
    return bool(lib().gdsp_istft_batch_fused(int(channels), int(nsegs), int(nfft), int(pad),
                                             int(noverlap)))


def istft_length(nsegs: int, nfft: int, noverlap: int) -> int:
    """The samples nsegs segments span: (nsegs - 1) * stride + NFFT (0: none)."""
    return (nsegs - 1) * (nfft - noverlap) + nfft if nsegs > 0 else 0


def IstftBatch(X, o: Optional[PwelchOptions], n: Optional[int] = None):
    """The inverse of StftBatch by weighted overlap-add (gdsp_istft_batch;
    MATLAB istft, scipy.signal.istft): X[channels, nsegs, Pad / 2 + 1]
    complex128 -> rows[channels, n], n = (nsegs - 1) * stride + NFFT unless a
    shorter n is given. rows[c, i] = sum_s w y_s / sum_s w^2 over the segments
    that cover i, exactly 0 where the window leaves a sample without weight.
    Pad >= NFFT is required."""
    X = np.asarray(X)
    if X.ndim != 3:
        raise Panic(_lib.GDSP_ERR_INVALID, "X must be channels x nsegs x (Pad/2+1)")
    channels, nsegs = X.shape[:2]
    if nsegs == 0 or X.shape[2] == 0:  # what StftBatch returns for an empty signal
        return np.zeros((channels, 0))
    nfft, pad, noverlap, win_seg, _, lp, _ = _welch_args(o)
    if pad < nfft:
        raise Panic(_lib.GDSP_ERR_INVALID, "Pad below NFFT: a truncated spectrum has no inverse")
    if X.shape[2] != lp:
        raise Panic(_lib.GDSP_ERR_INVALID,
                    "rows of %d bins, Pad / 2 + 1 = %d expected" % (X.shape[2], lp))
    X = np.ascontiguousarray(X, dtype=np.complex128)
    if nfft == noverlap and nsegs > 1:
        raise Panic(_lib.GDSP_ERR_DIVIDE_BY_ZERO, "runtime error: integer divide by zero")
    n_full = istft_length(nsegs, nfft, noverlap) if nsegs > 1 else nfft
    n = n_full if n is None else int(n)
    if n < 0 or n > n_full:
        raise Panic(_lib.GDSP_ERR_INVALID, "n = %d outside [0, %d]" % (n, n_full))
    out = np.empty((channels, n), np.float64)
    if n == 0 or channels == 0:
        return out
    no = _lib._I64(0)
    check(lib().gdsp_istft_batch(_p(X), channels, nsegs, nfft, pad, noverlap, _p(win_seg), n,
                                 _p(out), n, no), "IstftBatch")
    return out


def Istft(X, o: Optional[PwelchOptions], n: Optional[int] = None):
    """The inverse of Stft: X[nsegs, Pad / 2 + 1] -> x[n] (IstftBatch of one
    channel). Istft(Stft(x)[0], o, n=len(x)) is x wherever the window gives a
    sample weight."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise Panic(_lib.GDSP_ERR_INVALID, "X must be nsegs x (Pad/2+1)")
    return IstftBatch(X.reshape((1,) + X.shape), o, n)[0]


def Spectrogram(x, Fs: float, o: Optional[PwelchOptions]):
    """The spectrogram of one signal (MATLAB spectrogram's ps, scipy.signal.
    spectrogram): SpectrogramBatch of one row. Returns (P[nsegs, lp], freqs,
    times); P.mean(axis=0) is Pwelch(x, Fs, o)."""
    P, freqs, times = SpectrogramBatch(np.asarray(x, dtype=np.float64).reshape(1, -1), Fs, o)
    return P[0], freqs, times


def finalize(acc: np.ndarray, nsegs: int, nfft: int, pad: int, win_nfft: np.ndarray, Fs: float,
             scale_off: bool):
    """Host finalisation (gdsp_pwelch_finalize, spectral/pwelch.go:113-142) of
    summed accumulators acc[0..flen)."""
    acc = np.ascontiguousarray(acc, dtype=np.float64)
    win_nfft = np.ascontiguousarray(win_nfft, dtype=np.float64)
    lp = pad // 2 + 1
    pxx = np.empty(lp, np.float64)
    freqs = np.empty(lp, np.float64)
    check(lib().gdsp_pwelch_finalize(_p(acc), acc.size, nsegs, nfft, pad, _p(win_nfft),
                                     float(Fs), int(scale_off), _p(pxx), _p(freqs)),
          "pwelch_finalize")
    return pxx, freqs


def PwelchMulti(x, Fs: float, o: Optional[PwelchOptions], devices=None):
    """spectral.Pwelch split over `devices` (None: the library's device set):
    segment shards with their halos, per-device accumulation and one
    in-process RCCL reduce of the per-bin sums (gdsp_pwelch_multi)."""
    from .fft import _dev_array
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    if x.size == 0:
        return np.zeros(0), np.zeros(0)
    nfft, pad, noverlap, win_seg, win_nfft, lp, scale_off = _welch_args(o)
    pxx = np.empty(lp, np.float64)
    freqs = np.empty(lp, np.float64)
    lpo = _lib._I64(0)
    arr, n = _dev_array(devices)
    check(lib().gdsp_pwelch_multi(_p(x), x.size, float(Fs), nfft, pad, noverlap, _p(win_seg),
                                  _p(win_nfft), scale_off, _p(pxx), _p(freqs), lpo,
                                  arr, n), "PwelchMulti")
    return pxx[:lpo.value], freqs[:lpo.value]


def pwelch_shard(nsegs: int, nfft: int, noverlap: int, ndev: int, i: int):
    """(seg_lo, seg_hi, x_lo, x_hi) of device shard i (gdsp_pwelch_shard)."""
    v = [_lib._I64(0) for _ in range(4)]
    check(lib().gdsp_pwelch_shard(int(nsegs), int(nfft), int(noverlap), int(ndev), int(i), *v),
          "pwelch_shard")
    return tuple(a.value for a in v)
