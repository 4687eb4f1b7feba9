#!/usr/bin/env python3
"""Cosine transforms of types II and III (device.dct_batch: the fused
one-kernel form for powers of 2 from 256 to 16384) against the two other routes
to the same result: the same call under ALGO_NO_FUSED_DCT (the composed form),
and what the library offered before it — for type II a torch index-permute,
device.fft_real_batch, a torch multiply by w_k and twice the real part; for
type III its mirror: torch builds (x[k] - i x[N-k]) conj(w_k), then
device.fft_batch(inverse=True), the real part times N and the un-permute.
Device-resident rows (device.fill_uniform), 2^27 samples a shape (2 GiB of
algorithmic traffic, far above the Infinity Cache), HIP events on one stream, 3
warm-ups and the median of 20 runs, the three routes taking turns within every
round. tb_s: the algorithmic 16 bytes per sample (8 in, 8 out) over the fused call's
time. spread: the largest interquartile range over the median among the three
routes of the line, the session's own run-to-run spread; beats: the fused form
is faster than both other routes by more than that. One JSON line per shape and
type; --out also writes {"stamp": tools/source_stamp.py's, "records": [...]}."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
D = importlib.import_module("go-dsp_amd.device")
F = importlib.import_module("go-dsp_amd.fft")
L = importlib.import_module("go-dsp_amd._lib")

WARMUP, RUNS = 3, 20


def timings(fns, s):
    """(median ms, interquartile range / median) of each callable: WARMUP calls
    each, then RUNS rounds in which they take turns, every call between its own
    pair of events."""
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
    res = []
    for e in ev:
        t = sorted(a.elapsed_time(b) for a, b in e)
        q = statistics.quantiles(t, n=4)
        med = statistics.median(t)
        res.append((med, (q[2] - q[0]) / med))
    return res


def run(n, rows, type):
    x = torch.empty((rows, n), dtype=torch.float64, device="cuda")
    D.fill_uniform(x, 0x5EED)
    out = torch.empty((rows, n), dtype=torch.float64, device="cuda")
    real = torch.empty((rows, n), dtype=torch.float64, device="cuda")
    spec = torch.empty((rows, n), dtype=torch.complex128, device="cuda")
    prev = F.Algorithm()
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_DCT)
    work = torch.empty(max(int(L.lib().gdsp_dct_work_doubles(rows, n)), 2), dtype=torch.float64,
                       device="cuda")
    F.SetAlgorithm(prev)
    k = torch.arange(n, device="cuda")
    w = torch.polar(torch.ones(n, dtype=torch.float64, device="cuda"),
                    -math.pi * k.to(torch.float64) / (2 * n))
    wc = w.conj().resolve_conj()
    h = (n + 1) // 2
    src = torch.where(k < h, 2 * k, 2 * (n - 1 - k) + 1)      # v[i] = x[src[i]]
    pos = torch.where(k % 2 == 1, n - 1 - k // 2, k // 2)     # y[i] = v[pos[i]]
    rev = (n - k) % n
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def base2():
        with torch.cuda.stream(s):
            torch.index_select(x, 1, src, out=real)
        D.fft_real_batch(real, spec, stream=s)
        with torch.cuda.stream(s):
            torch.mul(spec, w, out=spec)
            torch.mul(spec.real, 2.0, out=out)

    def base3():
        with torch.cuda.stream(s):
            torch.index_select(x, 1, rev, out=real)
            real[:, 0] = 0.0
            torch.complex(x, real.neg_(), out=spec)
            torch.mul(spec, wc, out=spec)
        D.fft_batch(spec, spec, inverse=True, stream=s)
        with torch.cuda.stream(s):
            torch.index_select(spec.real, 1, pos, out=out)
            out.mul_(float(n))

    base = base2 if type == 2 else base3

    def new():
        D.dct_batch(x, type=type, out=out, work=work, stream=s)

    rec = {"n": n, "rows": rows, "type": type, "fused": bool(F.dct_fused(n))}
    base()
    s.synchronize()
    want = out[:4].clone()
    new()
    s.synchronize()
    rec["max_rel_diff"] = float(((out[:4] - want).abs().max() / want.abs().max()).item())

    def composed():  # the same call under the flag (host arithmetic, read at the call)
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_DCT)
        try:
            new()
        finally:
            F.SetAlgorithm(prev)

    (mb, sb), (mf, sf), (mc, sc) = timings([base, new, composed], s)
    spread = max(sb, sf, sc)
    rec.update(ms_fused=round(mf, 4), ms_composed=round(mc, 4), ms_base=round(mb, 4),
               speedup_vs_composed=round(mc / mf, 3), speedup_vs_base=round(mb / mf, 3),
               fused_tb_s=round(16 * rows * n / mf / 1e9, 3), spread=round(spread, 4),
               beats=bool(min(mc, mb) / mf > 1 + spread))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the records to this JSON file")
    ap.add_argument("--samples", type=int, default=1 << 27)
    ap.add_argument("n", nargs="*", type=int,
                    help="row lengths (default: 256, 1024, 4096, 8192, 16384)")
    a = ap.parse_args()
    import source_stamp
    torch.cuda.set_device(0)
    recs = []
    for n in a.n or [256, 1024, 4096, 8192, 16384]:
        for type in (2, 3):
            recs.append(run(n, max(1, a.samples // n), type))
            print(json.dumps(recs[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"stamp": source_stamp.stamp(), "records": recs}, f, indent=1)
            f.write("\n")
