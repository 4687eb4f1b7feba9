#!/usr/bin/env python3
"""Batched Pwelch accumulation (device.pwelch_batch_accumulate: one fused
kernel over all channels) against what the library offered before it for the
same job, and against the kernel family's ceiling. Per shape, in one run:

  (a) ms_batch:   device.pwelch_batch_accumulate over the (channels, n) rows;
  (b) ms_loop:    a Python loop of device.pwelch_accumulate over the rows into
                  the rows of one acc;
  (c) ms_ceiling: one device.pwelch_accumulate over the same channels * n
                  samples as a single signal, same options. It computes
                  something else (segments run across the row boundaries); it
                  is the rate the kernels reach with launch and grid effects
                  gone.

Device-resident rows (device.fill_uniform), HIP events on one stream, 3
warm-ups and the median of 20 runs, the three taking turns within the run.
`fused` is what gdsp_pwelch_batch_fused says of the shape: where it is false,
(a) is the library's own loop over the channels. One JSON line per shape;
--out also writes them as one JSON list."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
D = importlib.import_module("go-dsp_amd.device")
S = importlib.import_module("go-dsp_amd.spectral")
W = importlib.import_module("go-dsp_amd.window")

WARMUP, RUNS = 3, 20
SHAPES = [(4096, 1 << 16), (256, 1 << 20), (8, 1 << 25), (2, 1 << 27)]
OPTIONS = [(256, 0), (1024, 512), (2048, 1024)]


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


def run(x, channels, n, nfft, nov):
    rows = x.view(channels, n)
    flat = x.view(-1)
    win = torch.from_numpy(np.ascontiguousarray(W.Hann(nfft))).cuda()
    nsegs = S.segment_count(n, nfft, nov)
    nsegs_flat = S.segment_count(channels * n, nfft, nov)
    acc_a = torch.zeros((channels, nfft), dtype=torch.float64, device="cuda")
    acc_b = torch.zeros((channels, nfft), dtype=torch.float64, device="cuda")
    acc_c = torch.zeros(nfft, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def batch():
        D.pwelch_batch_accumulate(rows, nfft, nfft, nov, 0, nsegs, win, acc_a, stream=s)

    def loop():
        for c in range(channels):
            D.pwelch_accumulate(rows[c], nfft, nfft, nov, 0, nsegs, win, acc_b[c], stream=s)

    def ceiling():
        D.pwelch_accumulate(flat, nfft, nfft, nov, 0, nsegs_flat, win, acc_c, stream=s)

    batch()
    loop()
    s.synchronize()
    diff = float(((acc_a - acc_b).norm(dim=1) / acc_b.norm(dim=1)).max().item())
    ma, mb, mc = medians([batch, loop, ceiling], s)
    return {"channels": channels, "n": n, "nfft": nfft, "noverlap": nov,
            "segments_per_channel": nsegs,
            "fused": bool(S.pwelch_batch_fused(channels, n, nfft, 0, nov)),
            "max_row_rel_diff": diff, "ms_batch": round(ma, 4), "ms_loop": round(mb, 4),
            "ms_ceiling": round(mc, 4), "batch_over_loop": round(ma / mb, 4),
            "batch_over_ceiling": round(ma / mc, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the records to this JSON file")
    ap.add_argument("--log2-samples", type=int, default=28, help="samples in all (default 2^28)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    total = 1 << a.log2_samples
    x = torch.empty(total, dtype=torch.float64, device="cuda")
    D.fill_uniform(x, 0x5EED)
    recs = []
    for channels, n in SHAPES:
        n = n * total >> 28
        for nfft, nov in OPTIONS:
            recs.append(run(x, channels, n, nfft, nov))
            print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")
