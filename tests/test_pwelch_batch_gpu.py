"""GPU parity of the batched Pwelch (gdsp_pwelch_batch,
gdsp_pwelch_batch_accumulate_device, gdsp_pwelch_batch_finalize_device) and of
the planar WAV decode that feeds it: every row of a batch against the oracle's
spectral.Pwelch of that row within the suite's 1e-9, and against the engine's
single-signal Pwelch and its loop fallback within 1e-13 (a batch row and the
single-signal result differ only in the order of a sum of non-negative terms).

Shapes: the smallest that reach each way the kernel can go wrong. F = 64, 256,
1024 run S = 16, 4, 1 transforms per wave and F = 2048 the two-wave workgroup;
segments per channel 1 (a lone segment), 2 (one exact pair), 2S + 1 (a full
group and a partnerless tail) and 4S + 2 (two groups and a partial one);
1, 2 and 5 channels (five: one more than the waves of a workgroup). Rows are
scaled by 10^(c mod 4) so a leak between channels shows in the per-row error,
live in a buffer of row stride n + 3 with NaN in the gaps, and the accumulators
and results carry a guard row that must come back untouched."""
import importlib
import io
import struct

import numpy as np
import pytest

from conftest import row_nrel

pytestmark = pytest.mark.gpu

TOL = 1e-9     # north star: within 1e-9 relative
EXACT = 1e-13  # engine against engine (test_parity_gpu.py)
GUARD = -12345.0
FS = 48000.0

# option kinds: (Noverlap, Pad) from NFFT; F = max(Pad, NFFT)
OPTS = {
    "half": lambda f: (f, f // 2, 0),            # the HALF variant
    "nov0": lambda f: (f, 0, 0),                 # plain
    "odd": lambda f: (f, f // 4 + 1, 0),         # plain, odd overlap
    "pad2": lambda f: (f // 2, f // 8, f),       # Pad = 2 NFFT: the PAD variant
    "padh": lambda f: (f, f // 2 - 3, f // 2),   # Pad = NFFT / 2 (pwelch.go:108 quirk)
}
SEGS = {"one": lambda s: 1, "pair": lambda s: 2, "g1": lambda s: 2 * s + 1,
        "g2": lambda s: 4 * s + 2}

# (F, options, segments, channels, window): every F x option kind twice, every
# segment count and channel count with every F, every variant with every S
TABLE = [
    (64, "half", "one", 1, "hann"), (64, "half", "g2", 5, "hann"),
    (64, "nov0", "pair", 2, "hann"), (64, "nov0", "g1", 5, "hann"),
    (64, "odd", "g1", 1, "hann"), (64, "odd", "g2", 2, "hann"),
    (64, "pad2", "g2", 5, "hann"), (64, "pad2", "one", 2, "hann"),
    (64, "padh", "pair", 1, "hann"), (64, "padh", "g1", 5, "hann"),
    (256, "half", "g1", 5, "hann"), (256, "half", "pair", 2, "hamming"),
    (256, "nov0", "g2", 1, "hann"), (256, "nov0", "one", 5, "hann"),
    (256, "odd", "pair", 5, "hann"), (256, "odd", "g2", 2, "hann"),
    (256, "pad2", "g1", 2, "hann"), (256, "pad2", "g2", 1, "hann"),
    (256, "padh", "g2", 5, "hann"), (256, "padh", "one", 1, "hann"),
    (1024, "half", "g2", 2, "hann"), (1024, "half", "g1", 5, "hann"),
    (1024, "nov0", "one", 2, "hann"), (1024, "nov0", "g2", 5, "hann"),
    (1024, "odd", "g1", 5, "hann"), (1024, "odd", "pair", 1, "hann"),
    (1024, "pad2", "pair", 5, "hann"), (1024, "pad2", "g1", 1, "hann"),
    (1024, "padh", "g1", 2, "hann"), (1024, "padh", "g2", 5, "hann"),
    (2048, "half", "pair", 5, "hann"), (2048, "half", "g2", 1, "hann"),
    (2048, "nov0", "g1", 2, "hann"), (2048, "nov0", "g2", 5, "hann"),
    (2048, "odd", "one", 5, "hann"), (2048, "odd", "g2", 2, "hann"),
    (2048, "pad2", "g2", 2, "hann"), (2048, "pad2", "g1", 5, "hann"),
    (2048, "padh", "one", 1, "hann"), (2048, "padh", "pair", 5, "hann"),
]
WIN = {"hann": "Hann", "hamming": "Hamming"}
IDS = ["-".join(str(v) for v in row) for row in TABLE]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


def _shape(row):
    f, opt, seg, channels, win = row
    nfft, nov, pad = OPTS[opt](f)
    pad = pad or nfft  # the default, spelled out
    s = max(1, 1024 // f)  # transforms side by side in a worker
    nsegs = SEGS[seg](s)
    stride = nfft - nov
    n = (nsegs - 1) * stride + nfft + min(3, stride - 1)  # a tail shorter than a stride
    return nfft, nov, pad, nsegs, n, channels, win


def _options(gdsp, nfft, nov, pad, win="hann"):
    return gdsp.spectral.PwelchOptions(NFFT=nfft, Noverlap=nov, Pad=pad,
                                       Window=getattr(gdsp.window, WIN[win]))


def _signal(seed, channels, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((channels, n)) * (10.0 ** (np.arange(channels) % 4))[:, None]


def _strided(x):
    """The rows of x on the device in a buffer of row stride n + 3, NaN between."""
    import torch
    channels, n = x.shape
    buf = torch.full((channels, n + 3), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(x).cuda()
    return buf[:, :n]


def _run_guarded(D, xd, o, flen, lp, **kw):
    """device.pwelch_batch into caller tensors with a guard row each."""
    import torch
    channels = xd.shape[0]
    acc = torch.full((channels + 1, flen), GUARD, dtype=torch.float64, device="cuda")
    out = torch.full((channels + 1, lp), GUARD, dtype=torch.float64, device="cuda")
    res, freqs = D.pwelch_batch(xd, FS, o, out=out[:channels], acc=acc[:channels], **kw)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert bool((acc[channels] == GUARD).all()) and bool((out[channels] == GUARD).all())
    return out[:channels].cpu().numpy(), freqs, acc[:channels].cpu().numpy()


_cache: dict = {}


def _case(gdsp, oracle, D, i):
    """Inputs, the oracle's rows and the batched kernel's result of TABLE[i],
    computed once."""
    if i not in _cache:
        nfft, nov, pad, nsegs, n, channels, win = _shape(TABLE[i])
        x = _signal(1000 + i, channels, n)
        o = _options(gdsp, nfft, nov, pad, win)
        assert gdsp.spectral.segment_count(n, nfft, nov) == nsegs
        ref = [oracle.pwelch(r, FS, nfft=nfft, pad=pad, noverlap=nov, window_kind=win) for r in x]
        assert gdsp.spectral.pwelch_batch_fused(channels, n, nfft, pad, nov)
        pxx, freqs, acc = _run_guarded(D, _strided(x), o, max(pad, nfft), pad // 2 + 1)
        _cache[i] = dict(x=x, o=o, ref=np.stack([p for p, _ in ref]), ref_freqs=ref[0][1],
                         pxx=pxx, freqs=freqs, acc=acc, nsegs=nsegs)
    return _cache[i]


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_batched_kernel_vs_oracle_and_single(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    err = row_nrel(c["pxx"], c["ref"])
    print("oracle", IDS[i], err)
    assert err < TOL
    assert np.array_equal(c["freqs"], c["ref_freqs"])
    single = [gdsp.spectral.Pwelch(r, FS, c["o"]) for r in c["x"]]
    err = row_nrel(c["pxx"], np.stack([p for p, _ in single]))
    print("single", IDS[i], err)
    assert err < EXACT
    assert np.array_equal(c["freqs"], single[0][1])


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_loop_fallback_agrees_with_batched_kernel(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    F = gdsp.fft
    nfft, nov, pad, nsegs, n, channels, _ = _shape(TABLE[i])
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_PWELCH_BATCH)
        assert not gdsp.spectral.pwelch_batch_fused(channels, n, nfft, pad, nov)
        pxx, freqs, _ = _run_guarded(D, _strided(c["x"]), c["o"], max(pad, nfft), pad // 2 + 1)
    finally:
        F.SetAlgorithm(prev)
    err = row_nrel(pxx, c["pxx"])
    print("loop", IDS[i], err)
    assert err < EXACT
    assert np.array_equal(freqs, c["freqs"])


@pytest.mark.parametrize("nfft,nov", [(32, 16), (4096, 2048), (3000, 1000), (100, 30)])
def test_fallback_lengths_vs_oracle(gdsp, oracle, D, nfft, nov):
    channels, nsegs = 3, 5
    n = (nsegs - 1) * (nfft - nov) + nfft + 2
    assert not gdsp.spectral.pwelch_batch_fused(channels, n, nfft, 0, nov)
    x = _signal(nfft, channels, n)
    o = _options(gdsp, nfft, nov, 0)
    pxx, freqs, _ = _run_guarded(D, _strided(x), o, nfft, nfft // 2 + 1)
    ref = [oracle.pwelch(r, FS, nfft=nfft, noverlap=nov) for r in x]
    assert row_nrel(pxx, np.stack([p for p, _ in ref])) < TOL
    assert np.array_equal(freqs, ref[0][1])


@pytest.mark.parametrize("k", [5, 8], ids=["odd", "even"])
def test_accumulation_adds(gdsp, D, k):
    import torch
    nfft, nov, channels, nsegs = 256, 128, 5, 18  # 4 S + 2 segments
    n = (nsegs - 1) * (nfft - nov) + nfft
    xd = _strided(_signal(77, channels, n))
    win = torch.from_numpy(np.ascontiguousarray(gdsp.window.Hann(nfft))).cuda()
    whole = torch.zeros((channels + 1, nfft), dtype=torch.float64, device="cuda")
    parts = torch.zeros((channels + 1, nfft), dtype=torch.float64, device="cuda")
    whole[channels] = GUARD
    parts[channels] = GUARD
    D.pwelch_batch_accumulate(xd, nfft, nfft, nov, 0, nsegs, win, whole[:channels])
    D.pwelch_batch_accumulate(xd, nfft, nfft, nov, 0, k, win, parts[:channels])
    D.pwelch_batch_accumulate(xd, nfft, nfft, nov, k, nsegs, win, parts[:channels])
    torch.cuda.synchronize()
    assert bool((whole[channels] == GUARD).all()) and bool((parts[channels] == GUARD).all())
    # A packed pair's |FFT(x_s + i x_(s+1))_k|^2 holds a cross term that only
    # cancels between bins k and F - k, so which segments are paired (an odd k
    # shifts the pairing) moves power between acc[k] and acc[F - k]: what the
    # accumulators define, and finalisation reads, is the folded sum.
    def fold(a):
        a = a[:channels].cpu().numpy()
        return a + a[:, (nfft - np.arange(nfft)) % nfft]
    err = row_nrel(fold(parts), fold(whole))
    print("adds", k, err)
    assert err < EXACT


@pytest.mark.parametrize("i,scale_off", [(10, False), (18, True), (36, False)])
def test_device_finalize_equals_host_finalize(gdsp, oracle, D, i, scale_off):
    import torch
    c = _case(gdsp, oracle, D, i)
    nfft, nov, pad, nsegs, n, channels, win = _shape(TABLE[i])
    G = gdsp._lib
    flen, lp = max(pad, nfft), pad // 2 + 1
    wn = np.ascontiguousarray(getattr(gdsp.window, WIN[win])(nfft), dtype=np.float64)
    acc = torch.from_numpy(c["acc"]).cuda()
    out = torch.full((channels + 1, lp), GUARD, dtype=torch.float64, device="cuda")
    freqs = np.empty(lp)
    G.check(G.lib().gdsp_pwelch_batch_finalize_device(
        G._P(acc.data_ptr()), channels, flen, nsegs, nfft, pad, wn.ctypes.data_as(G._P), FS,
        int(scale_off), G._P(out.data_ptr()), freqs.ctypes.data_as(G._P),
        G._P(torch.cuda.current_stream().cuda_stream)), "finalize")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[channels] == GUARD)
    for ch in range(channels):
        p, f = gdsp.spectral.finalize(c["acc"][ch], nsegs, nfft, pad, wn, FS, scale_off)
        assert np.array_equal(got[ch], p), ch
        assert np.array_equal(freqs, f)


def test_host_entry(gdsp, oracle, D):
    S = gdsp.spectral
    c = _case(gdsp, oracle, D, 10)
    pxx, freqs = S.PwelchBatch(c["x"], FS, c["o"])
    assert row_nrel(pxx, c["ref"]) < TOL and row_nrel(pxx, c["pxx"]) < EXACT
    assert np.array_equal(freqs, c["ref_freqs"])
    # shorter than NFFT: every channel zero-padded to NFFT
    o = S.PwelchOptions(NFFT=64)
    x = _signal(5, 3, 50)
    pxx, freqs = S.PwelchBatch(list(x), FS, o)
    ref = [oracle.pwelch(r, FS, nfft=64) for r in x]
    assert pxx.shape == (3, 33)
    assert row_nrel(pxx, np.stack([p for p, _ in ref])) < TOL
    assert row_nrel(pxx, np.stack([S.Pwelch(r, FS, o)[0] for r in x])) < EXACT
    assert np.array_equal(freqs, ref[0][1])
    pxx, freqs = S.PwelchBatch(np.zeros((3, 0)), FS, o)
    assert pxx.shape == (3, 0) and freqs.shape == (0,)


def test_device_entry_short_and_empty(gdsp, oracle, D):
    import torch
    o = gdsp.spectral.PwelchOptions(NFFT=64)
    x = _signal(6, 2, 50)
    pxx, freqs = D.pwelch_batch(_strided(x), FS, o)
    ref = [oracle.pwelch(r, FS, nfft=64) for r in x]
    assert row_nrel(pxx.cpu().numpy(), np.stack([p for p, _ in ref])) < TOL
    pxx, freqs = D.pwelch_batch(torch.zeros((2, 0), dtype=torch.float64, device="cuda"), FS, o)
    assert tuple(pxx.shape) == (2, 0) and freqs.shape == (0,)


def test_stream_and_caller_buffers_give_the_same_bits(gdsp, oracle, D):
    import torch
    c = _case(gdsp, oracle, D, 21)  # caller's acc and out, the current stream
    xd = _strided(c["x"])
    pxx, freqs = D.pwelch_batch(xd, FS, c["o"])
    torch.cuda.synchronize()
    assert np.array_equal(pxx.cpu().numpy(), c["pxx"]) and np.array_equal(freqs, c["freqs"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    pxx, freqs = D.pwelch_batch(xd, FS, c["o"], stream=side)
    side.synchronize()
    assert np.array_equal(pxx.cpu().numpy(), c["pxx"]) and np.array_equal(freqs, c["freqs"])


def _wav(audio_format, bits, channels, data):
    """A 44-byte canonical header and the data chunk."""
    block = channels * bits // 8
    return (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " +
            struct.pack("<IHHIIHH", 16, audio_format, channels, 44100, 44100 * block, block, bits) +
            b"data" + struct.pack("<I", len(data)) + data)


@pytest.mark.parametrize("audio_format,bits,channels", [(1, 16, 3), (3, 32, 2)],
                         ids=["pcm16x3", "float32x2"])
def test_wav_planar_decode_and_channel_spectra(gdsp, oracle, audio_format, bits, channels):
    import torch
    W = gdsp.wav
    frames = 5000
    rng = np.random.default_rng(bits + channels)
    if audio_format == 1:
        data = rng.integers(-32768, 32768, frames * channels).astype("<i2").tobytes()
    else:
        data = rng.standard_normal(frames * channels).astype("<f4").tobytes()
    blob = _wav(audio_format, bits, channels, data)
    assert len(blob) == 44 + len(data)
    want = oracle.wav_floats(data, frames * channels, audio_format, bits)
    # the planar decode, into rows of stride frames + 3 with a guard row
    raw = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    buf = torch.full((channels + 1, frames + 3), GUARD, dtype=torch.float64, device="cuda")
    W.device_floats_planar(raw, frames, channels, audio_format, bits, out=buf[:channels, :frames])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    for c in range(channels):
        assert np.array_equal(got[c, :frames], want[c::channels].astype(np.float64)), c
    assert np.all(got[:, frames:] == GUARD) and np.all(got[channels] == GUARD)
    # the feeder end to end
    w = W.New(io.BytesIO(blob))
    assert w.NumChannels == channels
    o = gdsp.spectral.PwelchOptions(NFFT=256, Noverlap=128)
    pxx, freqs = W.PwelchChannels(w, frames, o)
    ref = [oracle.pwelch(want[c::channels].astype(np.float64), 44100.0, nfft=256, noverlap=128)
           for c in range(channels)]
    assert pxx.shape == (channels, 129)
    assert row_nrel(pxx, np.stack([p for p, _ in ref])) < TOL
    assert np.array_equal(freqs, ref[0][1])
