#!/usr/bin/env python3
"""Analytic signal and envelope (device.hilbert_batch: the fused one-kernel
form for powers of 2 from 256 to 16384) against the two other routes to the
same result: the same call under ALGO_NO_FUSED_HILBERT (the composed form), and
what the library offered before it — device.fft_real_batch, a torch multiply by
the Hilbert multiplier (with the 1 + i m of scipy.signal.hilbert, so one
inverse transform gives x + i h), device.fft_batch(inverse=True), then nothing
more (analytic) or torch.abs (envelope). Device-resident rows
(device.fill_uniform), HIP events on one stream, 3 warm-ups and the median of
20 runs, the routes alternating within the run. tb_s: the algorithmic bytes (8
in, 16 or 8 out per sample) over the fused call's time. One JSON line per
shape and kind; --out also writes them as one JSON list."""
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


def run(n, rows, kind):
    x = torch.empty((rows, n), dtype=torch.float64, device="cuda")
    D.fill_uniform(x, 0x5EED)
    dt = torch.complex128 if kind == "analytic" else torch.float64
    out = torch.empty((rows, n), dtype=dt, device="cuda")
    spec = torch.empty((rows, n), dtype=torch.complex128, device="cuda")
    ana = torch.empty_like(spec)
    work = torch.empty(min(rows, max(1, (1 << 24) // n)) * n * 3, dtype=torch.float64,
                       device="cuda")
    f = torch.arange(n, device="cuda")
    # 1 + i m: 1 at 0 and n / 2, 2 below n / 2, 0 above
    mask = torch.where(2 * f < n, 2.0, 0.0).to(torch.float64)
    mask[0] = 1.0
    mask[n // 2] = 1.0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def base():
        D.fft_real_batch(x, spec, stream=s)
        with torch.cuda.stream(s):
            torch.mul(spec, mask, out=spec)
        D.fft_batch(spec, ana if kind == "envelope" else out, inverse=True, stream=s)
        if kind == "envelope":
            with torch.cuda.stream(s):
                torch.abs(ana, out=out)

    def new():
        D.hilbert_batch(x, kind=kind, out=out, work=work, stream=s)

    rec = {"n": n, "rows": rows, "kind": kind, "fused": bool(F.hilbert_fused(n))}
    base()
    s.synchronize()
    want = out[:4].clone()
    new()
    s.synchronize()
    rec["max_rel_diff"] = float(((out[:4] - want).abs().max() / want.abs().max()).item())
    mb, mf = medians([base, new], s)
    prev = F.Algorithm()
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_HILBERT)
    try:
        mc, = medians([new], s)
    finally:
        F.SetAlgorithm(prev)
    nbytes = (8 + (16 if kind == "analytic" else 8)) * rows * n
    rec.update(ms_fused=round(mf, 4), ms_composed=round(mc, 4), ms_base=round(mb, 4),
               speedup_vs_composed=round(mc / mf, 3), speedup_vs_base=round(mb / mf, 3),
               fused_tb_s=round(nbytes / mf / 1e9, 3))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the records to this JSON file")
    ap.add_argument("--samples", type=int, default=1 << 27)
    ap.add_argument("n", nargs="*", type=int, help="row lengths (default: 256, 1024, 4096, 16384)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    recs = []
    for n in a.n or [256, 1024, 4096, 16384]:
        for kind in ("analytic", "envelope"):
            recs.append(run(n, max(1, a.samples // n), kind))
            print(json.dumps(recs[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")
