"""The numpy model of gdsp_istft_batch (include/gdsp_fft.h) that the ISTFT
tests compare the engine with, and their metric.

For one channel with rows X_s, s < nsegs, of lp = F / 2 + 1 bins:

    y_s    = numpy.fft.irfft(X_s, n=F)[:NFFT]
    num[i] = sum_s w[i - s stride] y_s[i - s stride]     ascending s
    D[i]   = sum_s w[i - s stride]^2                      ascending s
    out[i] = num[i] / D[i] where D[i] > 0, exactly 0 where D[i] == 0

numpy's irfft ignores the imaginary parts of bins 0 and F / 2, as the engine
does. Both sums start from +0 and add their terms one segment at a time.
"""
import numpy as np


def n_full(nsegs: int, nfft: int, stride: int) -> int:
    return (nsegs - 1) * stride + nfft if nsegs > 0 else 0


def weights(w: np.ndarray, nsegs: int, nfft: int, stride: int) -> np.ndarray:
    """D[i], i < n_full, summed in ascending s."""
    D = np.zeros(n_full(nsegs, nfft, stride))
    w2 = w[:nfft] * w[:nfft]
    for s in range(nsegs):
        D[s * stride:s * stride + nfft] += w2
    return D


def istft(X: np.ndarray, w: np.ndarray, nfft: int, stride: int, F: int):
    """(out, D) of rows X[nsegs, lp] under the window w (its first nfft entries)."""
    X = np.asarray(X, dtype=np.complex128)
    nsegs = X.shape[0]
    assert X.shape[1] == F // 2 + 1 and F >= nfft
    num = np.zeros(n_full(nsegs, nfft, stride))
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.fft.irfft(X, n=F, axis=1)[:, :nfft]
        for s in range(nsegs):
            num[s * stride:s * stride + nfft] += w[:nfft] * y[s]
    D = weights(w, nsegs, nfft, stride)
    out = np.zeros_like(num)
    pos = D > 0
    with np.errstate(invalid="ignore", over="ignore"):
        out[pos] = num[pos] / D[pos]
    return out, D


def istft_batch(X: np.ndarray, w: np.ndarray, nfft: int, stride: int, F: int):
    """(out[channels, n_full], D) of X[channels, nsegs, lp]."""
    rows = [istft(x, w, nfft, stride, F) for x in X]
    return np.stack([r[0] for r in rows]), rows[0][1]


def stft_rows(x: np.ndarray, w: np.ndarray, nfft: int, stride: int, F: int, nsegs: int):
    """numpy.fft.rfft of the windowed segments of x[channels, n]: the input of
    the tests, X[channels, nsegs, lp]."""
    idx = np.arange(nsegs)[:, None] * stride + np.arange(nfft)[None, :]
    return np.fft.rfft(x[:, idx] * w[:nfft], n=F, axis=2)


def weighted_err(got: np.ndarray, ref: np.ndarray, D: np.ndarray, scale=None) -> float:
    """max_i |got - ref| sqrt(D / max D) / max |ref| of one row (or of the part
    given): the numerator's roundoff is about eps w max |y| and w <= sqrt D, so
    this is bounded by the transform's roundoff whatever the window."""
    scale = np.max(np.abs(ref)) if scale is None else scale
    if got.size == 0 or scale == 0:
        return 0.0 if np.array_equal(got, ref) else float("inf")
    return float(np.max(np.abs(got - ref) * np.sqrt(D / np.max(D))) / scale)


def plain_err(got: np.ndarray, ref: np.ndarray, D: np.ndarray) -> float:
    """The unweighted error over D > 0 relative to the row's largest sample."""
    pos = D > 0
    if not pos.any():
        return 0.0
    return float(np.max(np.abs(got[pos] - ref[pos])) / np.max(np.abs(ref)))
