#!/usr/bin/env python3
"""Batched Convolve (device.convolve_batch: the fused one-kernel convolution
for powers of 2 from 256 to 16384) against what the library offered before it
for the same job: device.fft_batch, a torch broadcast multiply by a
precomputed spectrum of y, device.fft_batch(inverse=True). Device-resident
rows (device.fill_uniform), one y for all rows and one y per row, HIP events
on one stream, 3 warm-ups and the median of 20 runs, the two alternating
within the run. The new call computes the spectrum of y itself, every call;
`ms_base_with_yfft` adds that transform to the baseline for the per-row case,
where it is a pass over as much data as x. `ms_composed` is the new call
with ALGO_NO_FUSED_CONVOLVE. One JSON line per shape; --out also writes them
as one JSON list."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
D = importlib.import_module("go-dsp_amd.device")
F = importlib.import_module("go-dsp_amd.fft")

WARMUP, RUNS = 3, 20


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


def run(n, batch, per_row):
    x = torch.empty((batch, n), dtype=torch.complex128, device="cuda")
    D.fill_uniform(x, 0x5EED)
    y = torch.empty((batch, n) if per_row else (n,), dtype=torch.complex128, device="cuda")
    D.fill_uniform(y, 0xC0DE)
    y2 = y if per_row else y.view(1, n)
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    work, yhat = torch.empty_like(y2), torch.empty_like(y2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    D.fft_batch(y2, yhat, stream=s)

    def base():
        D.fft_batch(x, tmp, stream=s)
        with torch.cuda.stream(s):
            torch.mul(tmp, yhat, out=tmp)
        D.fft_batch(tmp, out, inverse=True, stream=s)

    def base_yfft():
        D.fft_batch(y2, yhat, stream=s)
        base()

    def new():
        D.convolve_batch(x, y, out=out, work=work, stream=s)

    rec = {"n": n, "batch": batch, "y": "per_row" if per_row else "shared",
           "fused": bool(D.convolve_fused(n))}
    base()
    s.synchronize()
    want = out[:4].clone()
    new()
    s.synchronize()
    rec["max_rel_diff"] = float(((out[:4] - want).abs().max() / want.abs().max()).item())
    mb, mf, my = medians([base, new, base_yfft], s)
    prev = F.Algorithm()
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_CONVOLVE)
    try:
        mc, = medians([new], s)
    finally:
        F.SetAlgorithm(prev)
    rec.update(ms_base=round(mb, 4), ms_new=round(mf, 4), ms_base_with_yfft=round(my, 4),
               ms_composed=round(mc, 4), speedup=round(mb / mf, 3),
               speedup_with_yfft=round(my / mf, 3),
               new_tb_s=round(32 * batch * n / mf / 1e9, 3))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the records to this JSON file")
    ap.add_argument("--samples", type=int, default=1 << 27)
    ap.add_argument("n", nargs="*", type=int, help="row lengths (default: 65536 x 4096, then "
                    "--samples at each 2^8 ... 2^14)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    shapes = [(n, max(1, a.samples // n)) for n in a.n] or \
        [(4096, 65536)] + [(1 << k, a.samples >> k) for k in range(8, 15)]
    recs = []
    for n, batch in shapes:
        for per_row in (False, True):
            recs.append(run(n, batch, per_row))
            print(json.dumps(recs[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")
