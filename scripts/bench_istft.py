#!/usr/bin/env python3
"""The ISTFT (device.istft_batch: one fused overlap-add kernel over all
channels) against the library's own other route and against the only route
there was before. Per shape, in one run:

  (a) ms_fused:        gdsp_istft_batch_device as it is;
  (b) ms_materialised: the same call under ALGO_NO_FUSED_ISTFT (rows completed
                       to dense complex rows of F, the plan's batched inverse
                       transform, a kernel with one thread per output sample);
  (c) ms_composed:     outside the spectral API: torch Hermitian completion,
                       device.fft_batch(inverse=True), slice and window,
                       index_add_ fold, divide by the window sums (computed
                       once, outside the timing); in chunks of 2^24 elements.

2^28 output samples in all, over 2 / 256 / 4096 channels, NFFT 256 / 1024 /
2048, overlap half, 75 % and none. The rows are uniform random numbers in HBM
(device.fill_uniform). HIP events on one stream, 3 warm-ups and the median of
10 runs, the three taking turns within a run; spread_* is (max - min) / median
of a route's 10 runs. `fused` is what gdsp_istft_batch_fused says of the shape.
max_weighted_diff is the worst difference of (a) from (c) and from (b), times
sqrt(D / max D), over the largest sample; share_of_8TBs is the algorithmic
bytes of (a), 16 lp per segment plus 8 per output sample, over its time, as a
share of 8 TB/s. One JSON line per record; --out also writes {"stamp":
tools/source_stamp.py's, "records": [...]}."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
D = importlib.import_module("go-dsp_amd.device")
F = importlib.import_module("go-dsp_amd.fft")
G = importlib.import_module("go-dsp_amd._lib")
S = importlib.import_module("go-dsp_amd.spectral")
W = importlib.import_module("go-dsp_amd.window")

WARMUP, RUNS = 3, 10
CHANNELS = [2, 256, 4096]
NFFTS = [256, 1024, 2048]
CHUNK = 1 << 24  # complex elements per chunk of the composed form


def timed(fns, s):
    """(median ms, spread) of each callable: WARMUP calls each, then RUNS rounds
    in which they take turns, every call between its own pair of events."""
    for f in fns:
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(RUNS)] for _ in fns]
    for r in range(RUNS):
        for i, f in enumerate(fns):
            ev[i][r][0].record(s)
            f()
            ev[i][r][1].record(s)
    torch.cuda.synchronize()
    out = []
    for e in ev:
        t = [a.elapsed_time(b) for a, b in e]
        m = statistics.median(t)
        out.append((m, (max(t) - min(t)) / m))
    return out


def composed(X, nfft, stride, win, dsum, out, s):
    """out[c] = fold(w * irfft(X[c, j])[:nfft]) / D by torch and the batched inverse FFT."""
    channels, ns, lp = X.shape
    n = out.shape[1]
    base = torch.arange(nfft, device="cuda")

    def fold(c0, cc, j0, k):
        a = X[c0:c0 + cc, j0:j0 + k]
        head = a[..., :1].real.to(torch.complex128)
        tail = a[..., lp - 1:].real.to(torch.complex128)
        full = torch.cat([head, a[..., 1:lp - 1], tail, a[..., 1:lp - 1].flip(-1).conj()], dim=-1)
        y = D.fft_batch(full.reshape(cc * k, nfft).contiguous(), inverse=True, stream=s)
        y = (y.real * win).view(cc, k * nfft)
        idx = (torch.arange(j0, j0 + k, device="cuda")[:, None] * stride + base).reshape(-1)
        out[c0:c0 + cc].index_add_(1, idx, y)

    with torch.cuda.stream(s):
        out.zero_()
        if ns * nfft <= CHUNK:
            cc = max(1, CHUNK // (ns * nfft))
            for c0 in range(0, channels, cc):
                fold(c0, min(cc, channels - c0), 0, ns)
        else:
            k = max(1, CHUNK // nfft)
            for c in range(channels):
                for j0 in range(0, ns, k):
                    fold(c, 1, j0, min(k, ns - j0))
        out.div_(dsum)
        out.masked_fill_(dsum == 0, 0.0)
    assert n == dsum.shape[0]


def run(channels, nsegs, nfft, nov):
    lp, stride = nfft // 2 + 1, nfft - nov
    n = (nsegs - 1) * stride + nfft
    X = torch.empty((channels, nsegs, lp), dtype=torch.complex128, device="cuda")
    D.fill_uniform(X, 0x5EED)
    wn = np.ascontiguousarray(W.Hann(nfft))
    win = torch.from_numpy(wn).cuda()
    dsum = torch.zeros(n, dtype=torch.float64, device="cuda")
    idx = (torch.arange(nsegs, device="cuda")[:, None] * stride +
           torch.arange(nfft, device="cuda")).reshape(-1)
    dsum.index_add_(0, idx, (win * win).repeat(nsegs))
    out_a = torch.empty((channels, n), dtype=torch.float64, device="cuda")
    out_b = torch.empty_like(out_a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    lib, P = G.lib(), ctypes.c_void_p
    sp = P(s.cuda_stream)

    def call(out):
        G.check(lib.gdsp_istft_batch_device(
            P(X.data_ptr()), lp, nsegs * lp, channels, nsegs, 0, nsegs, nfft, nfft, nov,
            P(win.data_ptr()), 0, n, P(out.data_ptr()), n, sp), "istft_batch_device")

    def fused():
        call(out_a)

    def materialised():
        prev = F.Algorithm()
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_ISTFT)
        try:
            call(out_b)
        finally:
            F.SetAlgorithm(prev)

    def comp():
        composed(X, nfft, stride, win, dsum, out_b, s)

    wgt = (dsum / dsum.max()).sqrt()

    def diff(u, v):
        return float((((u - v).abs() * wgt).amax(dim=1) / v.abs().amax(dim=1)).max().item())

    fused()
    materialised()
    s.synchronize()
    diff_b = diff(out_a, out_b)
    comp()
    s.synchronize()
    diff_c = diff(out_a, out_b)
    (ma, sa), (mb, sb), (mc, sc) = timed([fused, materialised, comp], s)
    nbytes = 16 * lp * nsegs * channels + 8 * n * channels
    return {"channels": channels, "n": n, "nfft": nfft, "noverlap": nov,
            "segments_per_channel": nsegs,
            "fused": bool(S.istft_batch_fused(channels, nsegs, nfft, 0, nov)),
            "max_weighted_diff": diff_c, "max_weighted_diff_materialised": diff_b,
            "ms_fused": round(ma, 4), "ms_materialised": round(mb, 4), "ms_composed": round(mc, 4),
            "spread_fused": round(sa, 4), "spread_materialised": round(sb, 4),
            "spread_composed": round(sc, 4),
            "fused_over_materialised": round(ma / mb, 4), "fused_over_composed": round(ma / mc, 4),
            "share_of_8TBs": round(nbytes / (ma * 1e-3) / 8e12, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the stamp and the records to this JSON file")
    ap.add_argument("--log2-samples", type=int, default=28, help="output samples in all (2^28)")
    a = ap.parse_args()
    import source_stamp
    torch.cuda.set_device(0)
    total = 1 << a.log2_samples
    recs = []
    for channels in CHANNELS:
        for nfft in NFFTS:
            for nov in (nfft // 2, 3 * nfft // 4, 0):
                stride = nfft - nov
                nsegs = max(1, (total // channels - nfft) // stride + 1)
                recs.append(run(channels, nsegs, nfft, nov))
                print(json.dumps(recs[-1]), flush=True)
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"stamp": source_stamp.stamp(), "records": recs}, f, indent=1)
            f.write("\n")
