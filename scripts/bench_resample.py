#!/usr/bin/env python3
"""Polyphase resampling of long rows (device.upfirdn_batch on fft.resample_taps'
filter, padded and ranged as device.resample_poly_batch does: the fused
polyphase kernel) against the plain form of the same call
(ALGO_NO_FUSED_UPFIRDN) and against what the library offered before it for the
same job, written with torch glue on the public API: zero-stuff by `up` into a
buffer `up` times the size, device.fir_batch(full=True) over all of it, a
strided slice by `down`. --samples float64 input samples in all (default 2^28:
2 GiB in, beyond the 256 MiB Infinity Cache), over 2 / 256 / 4096 channels, at
160/147, 147/160, 1/8, 4/1 and 2/3. Device-resident rows (device.fill_uniform),
one stream; each figure is the median of WINDOWS timed windows of back-to-back
calls between two HIP events (the window's average per call) after WARMUP
calls, the forms taking turns. The glue's stuffed buffer holds at most
--glue-doubles (default 2^29: 4 GiB, and as much again for its output): where
the job needs more, the glue runs on `glue_samples` input samples and
`ms_glue` is that time times samples / glue_samples (`glue_scaled`). `tb_s` is
the fused call's rate on the algorithmic bytes 8 (n + n_out) per row. One JSON
line per shape; --out also writes them as one JSON list."""
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
F = importlib.import_module("go-dsp_amd.fft")

WARMUP, WINDOWS = 2, 3
CHANNELS = (2, 256, 4096)
RATIOS = ((160, 147), (147, 160), (1, 8), (4, 1), (2, 3))


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


def padded_taps(n, up, down):
    pl = F.resample_plan(n, up, down)
    h = np.concatenate([np.zeros(pl["pre"]), F.resample_taps(up, down), np.zeros(pl["post"])])
    return h, pl["rem"], pl["n_out"]


def run(samples, channels, up, down, glue_doubles):
    n = samples // channels
    hh, rem, n_out = padded_taps(n, up, down)
    m = hh.size
    x = torch.empty((channels, n), dtype=torch.float64, device="cuda")
    D.fill_uniform(x, 0x5EED)
    h = torch.from_numpy(hh).cuda()
    out = torch.empty((channels, n_out), dtype=torch.float64, device="cuda")
    work = torch.empty(up * -(-m // up), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()

    def new():
        D.upfirdn_batch(x, h, up, down, out=out, out_begin=rem, out_end=rem + n_out, work=work,
                        stream=s)

    # the parent's route on the first ng samples of every row
    ng = min(n, max(glue_doubles // (up * channels), 1))
    hg, remg, n_outg = padded_taps(ng, up, down)
    hgd = torch.from_numpy(hg).cuda()
    xg = x[:, :ng]
    glue_out = [None]

    def glue():
        with torch.cuda.stream(s):
            xu = torch.zeros((channels, ng * up), dtype=torch.float64, device="cuda")
            xu[:, ::up] = xg
        y = D.fir_batch(xu, hgd, full=True, stream=s)
        with torch.cuda.stream(s):
            glue_out[0] = y[:, remg * down::down][:, :n_outg].contiguous()

    rec = {"channels": channels, "n": n, "up": up, "down": down, "m": m, "n_out": n_out,
           "fused": bool(F.upfirdn_fused(m, up, down)), "glue_samples": ng * channels,
           "glue_scaled": ng < n}
    prev = F.Algorithm()
    new()
    s.synchronize()
    head = out[:2, :1 << 15].clone()
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_UPFIRDN)
    try:
        new()
        s.synchronize()
        rec["plain_same_bits"] = bool(torch.equal(head.view(torch.int64),
                                                  out[:2, :1 << 15].view(torch.int64)))
    finally:
        F.SetAlgorithm(prev)
    glue()
    s.synchronize()
    k = min(1 << 15, n_outg, n_out) - 64  # the glue's short rows end earlier: compare inside them
    want = glue_out[0][:2, :k]
    rec["max_rel_diff_glue"] = float(((head[:, :k] - want).abs().max() / want.abs().max()).item())

    def plain():
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_UPFIRDN)
        try:
            new()
        finally:
            F.SetAlgorithm(prev)

    mf, mp, mg = windows([new, plain, glue], [20, 5, 2], s)
    glue_out[0] = None
    mg *= n / ng
    bytes_alg = 8.0 * (n + n_out) * channels
    rec.update(ms_fused=round(mf, 4), ms_plain=round(mp, 4), ms_glue=round(mg, 3),
               speedup_plain=round(mp / mf, 3), speedup_glue=round(mg / mf, 1),
               speedup_glue_plain=round(mg / mp, 1), tb_s=round(bytes_alg / mf / 1e9, 3))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the records to this JSON file")
    ap.add_argument("--samples", type=int, default=1 << 28)
    ap.add_argument("--glue-doubles", type=int, default=1 << 29)
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    recs = []
    for channels in a.channels:
        for up, down in RATIOS:
            recs.append(run(a.samples, channels, up, down, a.glue_doubles))
            print(json.dumps(recs[-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")
