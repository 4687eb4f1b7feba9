#!/usr/bin/env python3
"""Batched cross-spectral accumulation (device.cpsd_batch_accumulate: one fused
kernel over all channel pairs) against the only route the library offered
before it, and against the batched Pwelch of the same rows. Per shape, in one
run:

  (a) ms_fused:    device.cpsd_batch_accumulate of x (channels, n) against y
                   (channels, n): Sxx, Syy and Sxy of every pair;
  (b) ms_composed: the same sums outside the spectral API: torch unfold and
                   window, device.fft_real_batch of both signals, torch
                   multiply and sum, in chunks of 2^24 segment samples;
  (c) ms_pwelch:   device.pwelch_batch_accumulate over the same 2 * channels
                   rows. It computes less (no cross term); the ratio (a) / (c)
                   is what the mirror exchange and the four sums per bin cost
                   over the batched Pwelch kernel.

2^28 samples in all, x and y together. Device-resident rows
(device.fill_uniform), HIP events on one stream, 3 warm-ups and the median of
10 runs, the three taking turns within the run. `fused` is what
gdsp_cpsd_batch_fused says of the shape. One JSON line per shape; --out also
writes {"stamp": tools/source_stamp.py's, "records": [...]}."""
import argparse
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
S = importlib.import_module("go-dsp_amd.spectral")
W = importlib.import_module("go-dsp_amd.window")

WARMUP, RUNS = 3, 10
CHANNELS = [2, 256, 4096]
OPTIONS = [(256, 128), (1024, 512), (2048, 1024)]
CHUNK = 1 << 24  # segment samples per chunk of the composed form


def medians(fns, s):
    """Median ms of each callable: WARMUP calls each, then RUNS rounds in which
    they take turns, every call between its own pair of events."""
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
    return [statistics.median(a.elapsed_time(b) for a, b in e) for e in ev]


def composed(x, y, nfft, nov, win, out, s):
    """out[c] = (Sxx, Syy, Re Sxy, Im Sxy)[: nfft // 2 + 1] of x[c] against y[c]."""
    hb = nfft // 2 + 1
    vx, vy = x.unfold(1, nfft, nfft - nov), y.unfold(1, nfft, nfft - nov)
    channels, ns, _ = vx.shape

    def sums(a, b):  # (cc, k, nfft) windowed segments -> (cc, 4, hb)
        cc, k, _ = a.shape
        X = D.fft_real_batch(a.reshape(cc * k, nfft), stream=s).view(cc, k, nfft)[..., :hb]
        Y = D.fft_real_batch(b.reshape(cc * k, nfft), stream=s).view(cc, k, nfft)[..., :hb]
        P = torch.conj(X) * Y
        return torch.stack([(X.real ** 2 + X.imag ** 2).sum(1), (Y.real ** 2 + Y.imag ** 2).sum(1),
                            P.real.sum(1), P.imag.sum(1)], dim=1)

    with torch.cuda.stream(s):
        out.zero_()
        if ns * nfft <= CHUNK:
            cc = max(1, CHUNK // (ns * nfft))
            for c0 in range(0, channels, cc):
                out[c0:c0 + cc] = sums(vx[c0:c0 + cc] * win, vy[c0:c0 + cc] * win)
        else:
            k = max(1, CHUNK // nfft)
            for c in range(channels):
                for j0 in range(0, ns, k):
                    out[c:c + 1] += sums(vx[c:c + 1, j0:j0 + k] * win, vy[c:c + 1, j0:j0 + k] * win)


def run(xy, channels, n, nfft, nov):
    rows = xy.view(2 * channels, n)
    x, y = rows[:channels], rows[channels:]
    hb = nfft // 2 + 1
    win = torch.from_numpy(np.ascontiguousarray(W.Hann(nfft))).cuda()
    nsegs = S.segment_count(n, nfft, nov)
    acc_a = torch.zeros((channels, 4, hb), dtype=torch.float64, device="cuda")
    acc_b = torch.zeros((channels, 4, hb), dtype=torch.float64, device="cuda")
    acc_c = torch.zeros((2 * channels, nfft), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def fused():
        D.cpsd_batch_accumulate(x, y, nfft, nfft, nov, 0, nsegs, win, acc_a, stream=s)

    def comp():
        composed(x, y, nfft, nov, win, acc_b, s)

    def pwelch():
        D.pwelch_batch_accumulate(rows, nfft, nfft, nov, 0, nsegs, win, acc_c, stream=s)

    acc_a.zero_()
    s.wait_stream(torch.cuda.current_stream())
    fused()
    comp()
    s.synchronize()

    def rel(u, v):
        return float(((u - v).norm(dim=-1) / v.norm(dim=-1)).max().item())

    diff = max(rel(acc_a[:, 0], acc_b[:, 0]), rel(acc_a[:, 1], acc_b[:, 1]),
               rel(torch.complex(acc_a[:, 2], acc_a[:, 3]), torch.complex(acc_b[:, 2], acc_b[:, 3])))
    ma, mb, mc = medians([fused, comp, pwelch], s)
    return {"channels": channels, "n": n, "nfft": nfft, "noverlap": nov,
            "segments_per_channel": nsegs,
            "fused": bool(S.cpsd_batch_fused(channels, n, nfft, 0, nov)),
            "max_row_rel_diff": diff, "ms_fused": round(ma, 4), "ms_composed": round(mb, 4),
            "ms_pwelch": round(mc, 4), "fused_over_composed": round(ma / mb, 4),
            "fused_over_pwelch": round(ma / mc, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the stamp and the records to this JSON file")
    ap.add_argument("--log2-samples", type=int, default=28,
                    help="samples in all, x and y together (default 2^28)")
    a = ap.parse_args()
    import source_stamp
    torch.cuda.set_device(0)
    total = 1 << a.log2_samples
    xy = torch.empty(total, dtype=torch.float64, device="cuda")
    D.fill_uniform(xy, 0x5EED)
    recs = []
    for channels in CHANNELS:
        n = total // (2 * channels)
        for nfft, nov in OPTIONS:
            recs.append(run(xy, channels, n, nfft, nov))
            print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"stamp": source_stamp.stamp(), "records": recs}, f, indent=1)
            f.write("\n")
