#!/usr/bin/env python3
"""Chirp-z transform of rows (device.czt_batch through a device.CztPlan: the
fused one-kernel form for convolution lengths F from 256 to 16384) against the
two other routes to the same result: the same call under ALGO_NO_FUSED_CZT (the
composed form), and what the library offered before it, the "before": a torch
multiply by the premultiplier into a zero-padded (rows, F) buffer,
device.fft_batch, a torch multiply by the chirp's spectrum,
device.fft_batch(inverse=True), a slice and a torch multiply by the
postmultiplier. Device-resident rows (device.fill_uniform), 2^27 input samples
in all, a zoom on the band 0.1234 ... 0.2345 of fs = 2. HIP events on one
stream, 3 warm-ups and the median of 20 runs, the routes alternating within
the run. tb_s: the algorithmic bytes (8 or 16 in per sample, 16 out per point)
over the fused call's time. One JSON line per shape and row type; --out also
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
F = importlib.import_module("go-dsp_amd.fft")
L = importlib.import_module("go-dsp_amd._lib")

WARMUP, RUNS = 3, 20
# F = 256, 1024, 4096, 8192, 16384, 4096; then 512 and 2048, so that every
# fused length has its own line
SHAPES = [(128, 128), (512, 512), (2048, 2048), (4096, 4097), (8192, 8192), (3000, 1000),
          (256, 256), (1024, 1024)]
FN, FS = [0.1234, 0.2345], 2.0


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


def host_tables(n, m, length, at, st, sd):
    A, v, P = (np.empty(k, np.complex128) for k in (n, length, m))
    p = L._P
    L.check(L.lib().gdsp_czt_tables(n, m, length, 1.0, at, st, sd, A.ctypes.data_as(p),
                                    v.ctypes.data_as(p), P.ctypes.data_as(p)), "czt_tables")
    return A, v, P


def run(n, m, rows, real):
    at, st, sd = FN[0] / FS, (FN[1] - FN[0]) / FS, m
    length, fused = F.czt_length(n, m)
    x = torch.empty((rows, n), dtype=torch.float64 if real else torch.complex128, device="cuda")
    D.fill_uniform(x, 0x5EED)
    out = torch.empty((rows, m), dtype=torch.complex128, device="cuda")
    plan = D.CztPlan(n, m, st, sd, at)
    prev = F.Algorithm()
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_CZT)
    wbytes = plan.work_bytes(rows)
    F.SetAlgorithm(prev)
    work = torch.empty(wbytes // 8, dtype=torch.float64, device="cuda")
    # the "before": tables on the device, the chirp's spectrum by the engine
    A, v, P = (torch.from_numpy(t).cuda() for t in host_tables(n, m, length, at, st, sd))
    vhat = D.fft_batch(v[None, :].contiguous())[0]
    pad = torch.zeros((rows, length), dtype=torch.complex128, device="cuda")
    spec = torch.empty_like(pad)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def base():
        with torch.cuda.stream(s):
            torch.mul(x, A, out=pad[:, :n])
        D.fft_batch(pad, spec, stream=s)
        with torch.cuda.stream(s):
            torch.mul(spec, vhat, out=spec)
        D.fft_batch(spec, spec, inverse=True, stream=s)
        with torch.cuda.stream(s):
            torch.mul(spec[:, :m], P, out=out)

    def new():
        D.czt_batch(x, plan, out=out, work=work, stream=s)

    rec = {"n": n, "m": m, "F": length, "rows": rows, "real": real, "fused": fused}
    base()
    s.synchronize()
    want = out[:4].clone()
    new()
    s.synchronize()
    rec["max_rel_diff"] = float(((out[:4] - want).abs().max() / want.abs().max()).item())
    mb, mf = medians([base, new], s)
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_CZT)
    try:
        mc, = medians([new], s)
    finally:
        F.SetAlgorithm(prev)
    nbytes = ((8 if real else 16) * n + 16 * m) * rows
    rec.update(ms_fused=round(mf, 4), ms_composed=round(mc, 4), ms_base=round(mb, 4),
               speedup_vs_composed=round(mc / mf, 3), speedup_vs_base=round(mb / mf, 3),
               fused_tb_s=round(nbytes / mf / 1e9, 3))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the stamp and the records to this JSON file")
    ap.add_argument("--samples", type=int, default=1 << 27, help="input samples in all")
    a = ap.parse_args()
    import source_stamp
    torch.cuda.set_device(0)
    recs = []
    for n, m in SHAPES:
        for real in (True, False):
            recs.append(run(n, m, max(1, a.samples // n), real))
            print(json.dumps(recs[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"stamp": source_stamp.stamp(), "records": recs}, f, indent=1)
            f.write("\n")
