#!/usr/bin/env python3
"""FIR filtering of long rows (device.fir_batch: the fused overlap-save kernel
for block lengths 256 ... 16384) against the composed form of the same call
(ALGO_NO_FUSED_FIR) and against what the library offered before it for the
same job, written with torch glue on the public API: pad, unfold into blocks,
device.fft_batch, multiply by the taps' spectrum, device.fft_batch(inverse=
True), slice the valid parts. --samples float64 samples in all (default 2^28:
2 GiB in, 2 GiB out, beyond the 256 MiB Infinity Cache), over 1 / 8 / 4096
channels, m = 31 / 255 / 2047 / 8192 taps, every admissible block length F
for each m. Device-resident rows (device.fill_uniform), one stream; each
figure is the median of WINDOWS timed windows of back-to-back calls between
two HIP events (the window's average per call) after WARMUP calls, the fused
call and the torch-glue form taking turns, the composed form on its own.
`tb_s` is the fused call's rate on the algorithmic bytes 8 (n F / L + out_len) per row. One JSON line per shape;
--out also writes them as one JSON list, followed by the per-F cost table
(ms per 2^27 points through the transform pair) that gdsp_fir_block's
constants are set from."""
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

WARMUP, WINDOWS = 2, 3
CHANNELS = (1, 8, 4096)
TAPS = (31, 255, 2047, 8192)
BLOCKS = tuple(1 << k for k in range(8, 15))


def windows(fns, calls, s):
    """Median over WINDOWS windows of each callable's average ms per call:
    calls[i] back-to-back calls of fns[i] between two events, the callables
    taking turns."""
    for f in fns:
        for _ in range(WARMUP):
            f()
    s.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(WINDOWS)] for _ in fns]
    for w in range(WINDOWS):
        for i, f in enumerate(fns):
            ev[i][w][0].record(s)
            for _ in range(calls[i]):
                f()
            ev[i][w][1].record(s)
    s.synchronize()
    return [statistics.median(a.elapsed_time(b) for a, b in e) / c for e, c in zip(ev, calls)]


def run(samples, channels, m, block):
    n = samples // channels
    L = block - m + 1
    nb = -(-n // L)
    x = torch.empty((channels, n), dtype=torch.float64, device="cuda")
    D.fill_uniform(x, 0x5EED)
    h = torch.empty(m, dtype=torch.float64, device="cuda")
    D.fill_uniform(h, 0xC0DE)
    out = torch.empty_like(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    hp = torch.zeros((1, block), dtype=torch.complex128, device="cuda")
    hp[0, :m] = h
    torch.cuda.synchronize()
    hspec = D.fft_batch(hp, stream=s)
    glue_out = [None]

    def glue():
        with torch.cuda.stream(s):
            xp = torch.nn.functional.pad(x, (m - 1, nb * L - n))
            rows = xp.unfold(1, block, L).to(torch.complex128).reshape(channels * nb, block)
        D.fft_batch(rows, rows, stream=s)
        with torch.cuda.stream(s):
            rows.mul_(hspec)
        D.fft_batch(rows, rows, inverse=True, stream=s)
        with torch.cuda.stream(s):
            y = rows.view(channels, nb, block)[:, :, m - 1:].real
            glue_out[0] = y.reshape(channels, nb * L)[:, :n].contiguous()

    def new():
        D.fir_batch(x, h, out=out, block=block, stream=s)

    rec = {"channels": channels, "n": n, "m": m, "F": block,
           "fused": bool(F.fir_block(m, block)[1])}
    glue()
    new()
    s.synchronize()
    want = glue_out[0][:2, :1 << 16]
    rec["max_rel_diff"] = float(((out[:2, :1 << 16] - want).abs().max() / want.abs().max()).item())
    mf, mg = windows([new, glue], [50, 5], s)
    glue_out[0] = None
    prev = F.Algorithm()
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_FIR)
    try:
        mc, = windows([new], [10], s)
    finally:
        F.SetAlgorithm(prev)
    bytes_alg = 8.0 * (n * block / L + n) * channels
    rec.update(ms_fused=round(mf, 4), ms_composed=round(mc, 4), ms_glue=round(mg, 4),
               speedup_composed=round(mc / mf, 3), speedup_glue=round(mg / mf, 3),
               tb_s=round(bytes_alg / mf / 1e9, 3),
               # ms per 2^27 points through FFT_F, multiply, inverse FFT_F
               cost=round(mf * (L / block) * (1 << 27) / samples, 4))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the records to this JSON file")
    ap.add_argument("--samples", type=int, default=1 << 28)
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    ap.add_argument("--taps", type=int, nargs="*", default=list(TAPS))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    recs = []
    for channels in a.channels:
        for m in a.taps:
            for block in BLOCKS:
                if block < 2 * m:
                    continue
                recs.append(run(a.samples, channels, m, block))
                print(json.dumps(recs[-1]), flush=True)
                torch.cuda.empty_cache()
    table = {str(b): round(statistics.median(r["cost"] for r in recs if r["F"] == b), 4)
             for b in BLOCKS if any(r["F"] == b for r in recs)}
    print(json.dumps({"cost_table": table}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs + [{"cost_table": table}], f, indent=1)
            f.write("\n")
