#!/usr/bin/env python3
"""Per-segment spectra (device.stft_batch / device.spectrogram_batch: one fused
kernel over all channels) against the library's own other route and against the
only route it offered before. Per shape and mode (complex rows, power rows), in
one run:

  (a) ms_fused:        the device entry (gdsp_stft_batch_device /
                       gdsp_spectrogram_batch_device) as it is;
  (b) ms_materialised: the same call under ALGO_NO_FUSED_STFT (gathered real
                       rows, the plan's batched transform, a kernel that writes
                       the first lp bins or their scaled powers);
  (c) ms_composed:     outside the spectral API: torch unfold and window,
                       device.fft_real_batch (all F bins of every segment),
                       slice to lp bins and copy into the result, plus abs^2
                       and the scaling for power rows; in chunks of 2^24
                       segment samples.

2^28 input samples in all. Device-resident rows (device.fill_uniform), HIP
events on one stream, 3 warm-ups and the median of 10 runs, the three taking
turns within a run. `fused` is what gdsp_stft_batch_fused says of the shape.
max_row_rel_diff is the worst per-row difference of (a) from (c); share_of_8TBs
is the algorithmic bytes of (a), 8 per input sample plus the output, over its
time, as a share of 8 TB/s. One JSON line per record; --out also writes
{"stamp": tools/source_stamp.py's, "records": [...]}."""
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
FS = 48000.0
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


def composed(x, nfft, nov, win, power, scale, out, s):
    """out[c, j] = the first lp bins of FFTReal(w x_j), or their scaled powers."""
    lp = nfft // 2 + 1
    v = x.unfold(1, nfft, nfft - nov)
    channels, ns, _ = v.shape

    def rows(a):  # (cc, k, nfft) segments -> (cc, k, lp)
        cc, k, _ = a.shape
        X = D.fft_real_batch((a * win).reshape(cc * k, nfft), stream=s).view(cc, k, nfft)[..., :lp]
        return (X.real ** 2 + X.imag ** 2) * scale if power else X

    with torch.cuda.stream(s):
        if ns * nfft <= CHUNK:
            cc = max(1, CHUNK // (ns * nfft))
            for c0 in range(0, channels, cc):
                out[c0:c0 + cc] = rows(v[c0:c0 + cc])
        else:
            k = max(1, CHUNK // nfft)
            for c in range(channels):
                for j0 in range(0, ns, k):
                    out[c:c + 1, j0:j0 + k] = rows(v[c:c + 1, j0:j0 + k])


def run(x, nfft, nov, power):
    channels, n = x.shape
    lp = nfft // 2 + 1
    nsegs = S.segment_count(n, nfft, nov)
    wn = np.ascontiguousarray(W.Hann(nfft))
    win = torch.from_numpy(wn).cuda()
    cj = torch.full((lp,), 2.0, dtype=torch.float64, device="cuda")
    cj[0] = cj[-1] = 1.0
    scale = cj / (float(np.sum(wn * wn)) * FS)
    dt = torch.float64 if power else torch.complex128
    out_a = torch.empty((channels, nsegs, lp), dtype=dt, device="cuda")
    out_b = torch.empty_like(out_a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    # the device entries as device.stft_batch / spectrogram_batch call them, without
    # their host work per call (freqs, and times: a numpy array of nsegs entries,
    # milliseconds of host time at a million segments, which the events would count)
    lib, P = G.lib(), ctypes.c_void_p
    norm = float(np.cumsum(wn * wn)[-1]) * FS
    sp = P(s.cuda_stream)

    def call(out):
        if power:
            G.check(lib.gdsp_spectrogram_batch_device(
                P(x.data_ptr()), n, channels, n, nfft, nfft, nov, 0, nsegs, P(win.data_ptr()), norm,
                P(out.data_ptr()), lp, nsegs * lp, sp), "spectrogram_batch_device")
        else:
            G.check(lib.gdsp_stft_batch_device(
                P(x.data_ptr()), n, channels, n, nfft, nfft, nov, 0, nsegs, P(win.data_ptr()),
                P(out.data_ptr()), lp, nsegs * lp, sp), "stft_batch_device")

    def fused():
        call(out_a)

    def materialised():
        prev = F.Algorithm()
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_STFT)
        try:
            call(out_b)
        finally:
            F.SetAlgorithm(prev)

    def comp():
        composed(x, nfft, nov, win, power, scale, out_b, s)

    def rel(u, v):
        u, v = u.reshape(-1, lp), v.reshape(-1, lp)
        return float(((u - v).norm(dim=-1) / v.norm(dim=-1)).max().item())

    fused()
    materialised()
    s.synchronize()
    diff_b = rel(out_a, out_b)
    comp()
    s.synchronize()
    diff_c = rel(out_a, out_b)
    ma, mb, mc = medians([fused, materialised, comp], s)
    nbytes = 8 * channels * n + out_a.numel() * out_a.element_size()
    return {"mode": "power" if power else "complex", "channels": channels, "n": n, "nfft": nfft,
            "noverlap": nov, "segments_per_channel": nsegs,
            "fused": bool(S.stft_batch_fused(channels, n, nfft, 0, nov)),
            "max_row_rel_diff": diff_c, "max_row_rel_diff_materialised": diff_b,
            "ms_fused": round(ma, 4), "ms_materialised": round(mb, 4), "ms_composed": round(mc, 4),
            "fused_over_materialised": round(ma / mb, 4), "fused_over_composed": round(ma / mc, 4),
            "share_of_8TBs": round(nbytes / (ma * 1e-3) / 8e12, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the stamp and the records to this JSON file")
    ap.add_argument("--log2-samples", type=int, default=28, help="input samples in all (2^28)")
    a = ap.parse_args()
    import source_stamp
    torch.cuda.set_device(0)
    total = 1 << a.log2_samples
    buf = torch.empty(total, dtype=torch.float64, device="cuda")
    D.fill_uniform(buf, 0x5EED)
    recs = []
    for channels in CHANNELS:
        x = buf.view(channels, total // channels)
        for nfft in NFFTS:
            for nov in (nfft // 2, 0):
                for power in (False, True):
                    recs.append(run(x, nfft, nov, power))
                    print(json.dumps(recs[-1]), flush=True)
                    torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"stamp": source_stamp.stamp(), "records": recs}, f, indent=1)
            f.write("\n")
