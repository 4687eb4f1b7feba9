"""The reference of the resampling tests (test_resample_host.py,
test_resample_gpu.py): scipy.signal.upfirdn's definition in np.longdouble —
zero-stuff by up, np.convolve, keep every down-th sample — rounded to float64,
and scipy.signal.resample_poly's composition on top of it. Nothing here calls
the library."""
import functools
import math

import numpy as np


def out_len(n, m, up, down):
    return ((n - 1) * up + m - 1) // down + 1 if n > 0 and m > 0 else 0


STUFFED_MAX = 30_000_000  # products of the literal form beyond which the zeros are left out


def upfirdn(x, h, up, down, literal=None):
    """Rows of out_len(n, m, up, down) float64. The literal form multiplies
    ((n - 1) up + 1) m pairs, all but one in `up` of them with a stuffed zero;
    past STUFFED_MAX products (the audio rate pairs: 1.5e9 per row) the same
    sums are taken without the zero terms: np.convolve of the row with each
    phase's taps h[p::up], still in np.longdouble, output j read from phase (j
    down) mod up at (j down) div up. test_resample_host.py holds the two forms
    against each other."""
    x = np.atleast_2d(x)
    n = x.shape[1]
    hl = np.asarray(h).astype(np.longdouble)
    m = hl.size
    if literal is None:
        literal = ((n - 1) * up + 1) * m <= STUFFED_MAX
    rows = []
    for r in x:
        rl = r.astype(np.longdouble)
        if literal:
            xu = np.zeros((n - 1) * up + 1, np.longdouble)
            xu[::up] = rl
            rows.append(np.convolve(xu, hl)[::down].astype(np.float64))
            continue
        T = -(-m // up)
        y = np.zeros((up, n + T - 1), np.longdouble)
        for p in range(min(up, m)):
            hp = hl[p::up]
            y[p, :n + hp.size - 1] = np.convolve(rl, hp)
        a = np.arange(out_len(n, m, up, down)) * down
        rows.append(y[a % up, a // up].astype(np.float64))
    return np.stack(rows)


def taps(up, down):
    """The written formula of fft.resample_taps."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    R = max(up, down)
    half = 10 * R
    k = np.arange(2 * half + 1)
    h = (1.0 / R) * np.sinc((k - half) / R) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def plan(n, m, up, down):
    """(up, down, pre, post, rem, n_out) as scipy.signal.resample_poly computes
    them for rows of n samples and m taps."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    half = (m - 1) // 2
    n_out = -(-n * up // down)
    pre = down - half % down
    rem = (half + pre) // down
    post = 0
    while out_len(n, m + pre + post, up, down) < n_out + rem:
        post += 1
    return up, down, pre, post, rem, n_out


def resample_poly(x, up, down, h=None):
    """The composition in extended precision; h None: taps(up, down)."""
    x = np.atleast_2d(x)
    h = taps(up, down) if h is None else np.asarray(h)
    u, d, pre, post, rem, n_out = plan(x.shape[1], h.size, up, down)
    hh = np.concatenate([np.zeros(pre), h, np.zeros(post)])
    return upfirdn(x, hh, u, d)[:, rem:rem + n_out]


@functools.lru_cache(maxsize=None)
def case(seed, channels, n, m, up, down):
    """Gaussian rows and taps with their reference, computed once and shared
    read-only."""
    rng = np.random.default_rng(seed)
    x, h = rng.standard_normal((channels, n)), rng.standard_normal(m)
    ref = upfirdn(x, h, up, down)
    for a in (x, h, ref):
        a.setflags(write=False)
    return x, h, ref
