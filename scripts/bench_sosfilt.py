#!/usr/bin/env python3
"""Recursive filtering (device.sosfilt_batch, device.sosfiltfilt_batch): the
time-parallel form against the plain form (the same call under
ALGO_NO_FUSED_SOSFILT) and, where scipy is present, against
scipy.signal.sosfilt on 16 host threads, one row per thread. 2^28 samples in
all over 2, 256 and 4096 channels, a Butterworth low-pass at 0.1 of 1, 2, 4 and
8 sections. Device-resident rows (device.fill_uniform), out and work given,
HIP events on one stream, 3 warm-ups and the median of 20 runs.

The plain form runs one thread per row, so its time is the row length times
the time per sample whatever the channel count; at these sizes that is seconds
to minutes. It is therefore timed on rows cut to 2^15 samples (1 warm-up, 3
runs) and ms_plain is that time scaled by the row length; plain_row says on
what it was measured. scipy is timed on 16 rows of 2^20 samples and scaled to
the line's samples over min(16, channels) threads. tb_s: the algorithmic 16
bytes per sample over the time-parallel call's time; frac_8tbs: that over 8
TB/s. One JSON line per shape; --out also writes them as one JSON list."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
D = importlib.import_module("go-dsp_amd.device")
F = importlib.import_module("go-dsp_amd.fft")
L = importlib.import_module("go-dsp_amd._lib").lib()

PLAIN_ROW = 1 << 15


def median_ms(f, s, warmup=3, runs=20):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(runs)]
    for a, b in ev:
        a.record(s)
        f()
        b.record(s)
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def scipy_ns_per_sample(sos):
    """ns per sample and row of scipy.signal.sosfilt with 16 rows in flight on
    16 threads (None without scipy)."""
    try:
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        from scipy.signal import sosfilt
    except ImportError:
        return None
    rows = np.random.default_rng(0).standard_normal((16, 1 << 20))
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda r: sosfilt(sos, r), rows))
        t = time.perf_counter()
        list(ex.map(lambda r: sosfilt(sos, r), rows))
        dt = time.perf_counter() - t
    return dt * 1e9 / rows.shape[1]     # 16 rows side by side: per sample of one thread's row


def run(channels, n, S, zero_phase, sci):
    sos = F.butter_sos(2 * S if S > 1 else 2, 0.1)[:S]
    assert len(sos) == S and F.sosfilt_fused(sos)
    x = torch.empty((channels, n), dtype=torch.float64, device="cuda")
    D.fill_uniform(x, 0x5EED)
    out = torch.empty_like(x)
    pl = F.sosfiltfilt_padlen(sos)
    need = (L.gdsp_sosfiltfilt_work_doubles(S, channels, n, pl) if zero_phase
            else L.gdsp_sosfilt_work_doubles(S, channels, n))
    work = torch.empty(int(need), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def call(xx, oo):
        if zero_phase:
            D.sosfiltfilt_batch(xx, sos, out=oo, work=work, stream=s)
        else:
            D.sosfilt_batch(xx, sos, out=oo, work=work, stream=s)

    ms = median_ms(lambda: call(x, out), s)
    m = min(n, PLAIN_ROW)
    xs, os_ = x[:, :m], out[:, :m]
    call(xs, os_)
    s.synchronize()
    want = os_[:2].clone()
    prev = F.Algorithm()
    F.SetAlgorithm(prev | F.ALGO_NO_FUSED_SOSFILT)
    try:
        mp = median_ms(lambda: call(xs, os_), s, warmup=1, runs=3)
        s.synchronize()
        diff = float(((os_[:2] - want).abs().max() / want.abs().max()).item())
    finally:
        F.SetAlgorithm(prev)
    rec = {"op": "sosfiltfilt" if zero_phase else "sosfilt", "channels": channels, "n": n, "S": S,
           "ms": round(ms, 4), "tb_s": round(16.0 * channels * n / ms / 1e9, 3),
           "frac_8tbs": round(16.0 * channels * n / ms / 1e9 / 8.0, 4),
           "plain_row": m, "ms_plain": round(mp * n / m, 2), "speedup_vs_plain": round(mp * n / m / ms, 1),
           "max_rel_diff_forms": diff}
    if sci is not None and not zero_phase:
        host = sci * n * -(-channels // 16) / 1e6
        rec.update(ms_scipy_16_threads=round(host, 1), speedup_vs_scipy=round(host / ms, 1))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the records to this JSON file")
    ap.add_argument("--samples", type=int, default=1 << 28)
    ap.add_argument("--channels", type=int, nargs="*", default=[2, 256, 4096])
    ap.add_argument("--sections", type=int, nargs="*", default=[1, 2, 4, 8])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    recs = []
    for S in a.sections:
        sci = scipy_ns_per_sample(F.butter_sos(2 * S if S > 1 else 2, 0.1)[:S])
        for ch in a.channels:
            for zp in (False, True):
                recs.append(run(ch, a.samples // ch, S, zp, sci))
                print(json.dumps(recs[-1]), flush=True)
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")
