"""CPU-only checks of the per-segment spectra's boundary (Stft, Spectrogram,
StftBatch, SpectrogramBatch): the five entry points are declared, exported and
bound alike; their argument checks answer before any device call; the flag that
turns the fused kernel off is a known algorithm bit; gdsp_stft_batch_fused (host
arithmetic) says which shapes take the kernel; freqs and times follow their
formulas; the Python mirrors panic like Pwelch and return shaped empties; and
the two references the GPU tests use (the oracle's pieces, numpy on the exact
segments) agree with each other and with the oracle's Pwelch far inside the
GPU tests' bounds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_stft_gpu as SG
from conftest import REPO, row_nrel

NAMES = ("gdsp_stft_batch", "gdsp_spectrogram_batch", "gdsp_stft_batch_fused",
         "gdsp_stft_batch_device", "gdsp_spectrogram_batch_device")


def test_header_exports_and_signatures_agree(gdsp):
    declared = set(gdsp._lib.header_functions())
    out = subprocess.run(["nm", "-D", "--defined-only",
                          os.path.join(REPO, "go-dsp_amd", "lib", "libgdspfft.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NAMES:
        assert name in declared, name
        assert name in exported, name
        assert name in gdsp._lib.SIGNATURES, name
    S = gdsp._lib.SIGNATURES
    P, I64, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    PI64 = ctypes.POINTER(I64)
    # (x, channels, n, ldx, nfft, pad, noverlap, win_seg, out, nsegs, lp)
    assert S["gdsp_stft_batch"] == (I, [P, I64, I64, I64, I64, I64, I64, P, P, PI64, PI64])
    # (x, channels, n, ldx, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off, out, freqs,
    #  times, nsegs, lp)
    assert S["gdsp_spectrogram_batch"] == (I, [P, I64, I64, I64, D, I64, I64, I64, P, P, I, P, P, P,
                                               PI64, PI64])
    assert S["gdsp_stft_batch_fused"] == (I, [I64, I64, I64, I64, I64])
    # (d_x, ldx, channels, n, nfft, pad, noverlap, seg_begin, seg_end, d_win_seg, [norm,] d_out,
    #  ld_seg, ld_chan, stream)
    assert S["gdsp_stft_batch_device"] == (I, [P, I64, I64, I64, I64, I64, I64, I64, I64, P, P,
                                               I64, I64, P])
    assert S["gdsp_spectrogram_batch_device"] == (I, [P, I64, I64, I64, I64, I64, I64, I64, I64, P,
                                                      D, P, I64, I64, P])
    hdr = open(os.path.join(REPO, "include", "gdsp_fft.h")).read()
    assert "GDSP_ALGO_NO_FUSED_STFT = 1024" in hdr


def _device_entries(gdsp):
    """Both device entries behind one signature (the power entry with norm 1)."""
    L = gdsp._lib.lib()

    def power(x, ldx, channels, n, nfft, pad, nov, b, e, win, out, ld_seg, ld_chan, stream):
        return L.gdsp_spectrogram_batch_device(x, ldx, channels, n, nfft, pad, nov, b, e, win, 1.0,
                                               out, ld_seg, ld_chan, stream)

    return L.gdsp_stft_batch_device, power


def test_device_entries_status_codes_before_any_device_call(gdsp):
    G = gdsp._lib
    buf = np.zeros(4096)
    p = buf.ctypes.data_as(G._P)
    null = G._P()
    for f in _device_entries(gdsp):
        def call(x=p, ldx=200, channels=2, n=200, nfft=64, pad=64, nov=0, b=0, e=1, win=p, out=p,
                 ld_seg=33, ld_chan=33):
            return f(x, ldx, channels, n, nfft, pad, nov, b, e, win, out, ld_seg, ld_chan, null)

        assert call(nfft=0) == G.GDSP_ERR_INVALID
        assert call(nfft=-64) == G.GDSP_ERR_INVALID
        assert call(pad=0) == G.GDSP_ERR_INVALID
        assert call(b=-1) == G.GDSP_ERR_INVALID
        assert call(b=2, e=1) == G.GDSP_ERR_INVALID
        assert call(channels=-1) == G.GDSP_ERR_INVALID
        assert call(n=-1) == G.GDSP_ERR_INVALID
        assert call(ldx=199) == G.GDSP_ERR_INVALID
        # rows of lp = 33: a row stride below them, a channel stride below its rows
        assert call(ld_seg=32) == G.GDSP_ERR_INVALID
        assert call(pad=128, ld_seg=64, ld_chan=64) == G.GDSP_ERR_INVALID   # lp = 65
        assert call(ld_chan=32) == G.GDSP_ERR_INVALID
        assert call(e=3, ld_chan=98) == G.GDSP_ERR_INVALID                   # 3 rows of 33
        assert call(b=1, e=3, ld_seg=40, ld_chan=79) == G.GDSP_ERR_INVALID   # 2 rows of 40
        # segments beyond the signal
        assert call(e=4, ld_chan=4 * 33) == G.GDSP_ERR_INVALID
        assert call(nov=-140, e=2, ld_chan=66) == G.GDSP_ERR_INVALID         # stride 204
        assert call(nov=100, e=2, ld_chan=66) == G.GDSP_ERR_INVALID          # a negative stride
        # a needed NULL pointer
        assert call(x=null) == G.GDSP_ERR_INVALID
        assert call(win=null) == G.GDSP_ERR_INVALID
        assert call(out=null) == G.GDSP_ERR_INVALID
        # a zero stride: Segment's integer divide, only past one segment
        assert call(nov=64, e=2, ld_chan=66) == G.GDSP_ERR_DIVIDE_BY_ZERO
        # nothing to do: nothing is looked at
        assert call(x=null, win=null, out=null, channels=0) == G.GDSP_OK
        assert call(x=null, win=null, out=null, b=1, e=1, ld_chan=0) == G.GDSP_OK
        assert call(x=null, win=null, out=null, b=0, e=0, ld_chan=0) == G.GDSP_OK
        if gdsp.device_count() == 0:
            assert call() == G.GDSP_ERR_NO_DEVICE
            assert call(e=3, ld_chan=99) == G.GDSP_ERR_NO_DEVICE


def test_host_entries_status_codes_before_any_device_call(gdsp):
    G = gdsp._lib
    L = G.lib()
    buf = np.zeros(8192)
    p = buf.ctypes.data_as(G._P)
    null = G._P()
    ns, lp = G._I64(-1), G._I64(-1)

    def power(x=p, channels=2, n=100, ldx=100, fs=1.0, nfft=64, pad=0, nov=0, out=p, freqs=p,
              times=p, nso=ns, lpo=lp):
        return L.gdsp_spectrogram_batch(x, channels, n, ldx, fs, nfft, pad, nov, null, null, 0, out,
                                        freqs, times, nso, lpo)

    def cplx(x=p, channels=2, n=100, ldx=100, fs=1.0, nfft=64, pad=0, nov=0, out=p, freqs=p,
             times=p, nso=ns, lpo=lp):
        return L.gdsp_stft_batch(x, channels, n, ldx, nfft, pad, nov, null, out, nso, lpo)

    for host in (power, cplx):
        assert host(nso=None) == G.GDSP_ERR_INVALID
        assert host(lpo=None) == G.GDSP_ERR_INVALID
        assert host(channels=-1) == G.GDSP_ERR_INVALID
        assert host(n=-1) == G.GDSP_ERR_INVALID
        assert host(ldx=99) == G.GDSP_ERR_INVALID
        assert host(nfft=-64) == G.GDSP_ERR_INVALID
        assert host(pad=-64) == G.GDSP_ERR_INVALID
        assert host(x=null) == G.GDSP_ERR_INVALID
        assert host(out=null) == G.GDSP_ERR_INVALID
        # a zero stride: Segment's integer divide
        assert host(nov=64) == G.GDSP_ERR_DIVIDE_BY_ZERO
        # n == 0: empty results, whatever else is passed
        ns.value = lp.value = -1
        assert host(x=null, n=0, ldx=0, channels=3, out=null, freqs=null, times=null) == G.GDSP_OK
        assert ns.value == 0 and lp.value == 0
        if gdsp.device_count() == 0:
            assert host() == G.GDSP_ERR_NO_DEVICE
            assert host(n=40) == G.GDSP_ERR_NO_DEVICE  # shorter than NFFT: one zero-padded segment
    assert power(freqs=null) == G.GDSP_ERR_INVALID
    assert power(times=null) == G.GDSP_ERR_INVALID
    # channels == 0: only freqs, times and the counts are written
    out = np.full(80, -7.0)
    freqs, times = np.full(40, -7.0), np.full(8, -7.0)
    ns.value = lp.value = -1
    assert power(x=null, channels=0, n=200, ldx=0, nov=24, fs=8.0, out=out.ctypes.data_as(G._P),
                 freqs=freqs.ctypes.data_as(G._P), times=times.ctypes.data_as(G._P)) == G.GDSP_OK
    assert ns.value == 4 and lp.value == 33        # (200 - 64) // 40 + 1
    assert np.array_equal(freqs[:33], np.arange(33) * (8.0 / 64)) and np.all(freqs[33:] == -7.0)
    assert np.array_equal(times[:4], (np.arange(4) * 40 + 32.0) / 8.0) and np.all(times[4:] == -7.0)
    assert np.all(out == -7.0)
    assert power(x=null, channels=0, freqs=null) == G.GDSP_ERR_INVALID
    ns.value = lp.value = -1
    assert cplx(x=null, channels=0, n=200, ldx=0, nov=24, out=null) == G.GDSP_OK
    assert ns.value == 4 and lp.value == 33
    # Pad below NFFT: lp follows Pad (pwelch.go:108), a short signal is one segment
    assert power(x=null, channels=0, n=10, ldx=0, nfft=64, pad=32, out=null) == G.GDSP_OK
    assert ns.value == 1 and lp.value == 17


def test_no_fused_stft_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_STFT == 1024
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_STFT)
        assert F.Algorithm() == F.ALGO_NO_FUSED_STFT
        F.SetAlgorithm(F.ALGO_NO_FUSED_STFT | F.ALGO_NO_FUSED_CPSD | F.ALGO_NO_FUSED_FIR)
        assert F.Algorithm() == F.ALGO_NO_FUSED_STFT | F.ALGO_NO_FUSED_CPSD | F.ALGO_NO_FUSED_FIR
        for bad in (1 << 20, 2048):
            with pytest.raises(gdsp.GDSPError) as e:
                F.SetAlgorithm(bad)
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == F.ALGO_NO_FUSED_STFT | F.ALGO_NO_FUSED_CPSD | F.ALGO_NO_FUSED_FIR
    finally:
        F.SetAlgorithm(prev)


FUSED = ((64, 0, 0), (128, 0, 64), (256, 0, 128), (512, 1024, 256), (1024, 0, 1), (2048, 0, 1024),
         (100, 256, 0))
MATERIALISED = ((32, 0, 0), (4096, 0, 2048), (2048, 4096, 0), (100, 0, 30), (3000, 0, 0),
                (256, 0, 256 - (1 << 22) - 1))


def test_fused_query_is_host_arithmetic(gdsp):
    F = gdsp.fft
    q = gdsp.spectral.stft_batch_fused
    for nfft, pad, nov in FUSED:
        assert q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    for nfft, pad, nov in MATERIALISED:
        assert not q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    assert q(5, 4096)  # the defaults: NFFT 256
    assert q(5, 4096, 256, 0, 256 - (1 << 22))  # the last stride the kernel addresses
    assert not q(-1, 4096) and not q(5, -1) and not q(5, 4096, -256)
    prev = F.Algorithm()
    try:
        # the flags of the other fused kernels do not touch this one, its own does
        F.SetAlgorithm(F.ALGO_NO_FUSED_PWELCH_BATCH | F.ALGO_NO_FUSED_CPSD)
        assert q(5, 4096, 256, 0, 128)
        F.SetAlgorithm(F.ALGO_NO_FUSED_STFT)
        assert gdsp.spectral.pwelch_batch_fused(5, 4096, 256, 0, 128)
        assert gdsp.spectral.cpsd_batch_fused(5, 4096, 256, 0, 128)
        for nfft, pad, nov in FUSED + MATERIALISED:
            assert not q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    finally:
        F.SetAlgorithm(prev)
    for nfft, pad, nov in FUSED:
        assert q(5, 4096, nfft, pad, nov), (nfft, pad, nov)


def test_freqs_and_times_follow_their_formulas(gdsp, oracle):
    S = gdsp.spectral
    for nfft, pad, nov, fs in ((256, 0, 128, 48000.0), (100, 0, 30, 1.0), (64, 128, 63, 8.0),
                               (64, 32, 0, 44100.0), (75, 0, 11, 3.0)):
        p = pad or nfft
        assert np.array_equal(S.stft_freqs(p, fs), oracle.pwelch(np.ones(4 * nfft), fs, nfft=nfft,
                                                                 pad=pad, noverlap=nov)[1])
        t = S.stft_times(0, 9, nfft, nov, fs)
        assert np.array_equal(t, np.array([(s * (nfft - nov) + nfft / 2) / fs for s in range(9)]))
        assert np.array_equal(S.stft_times(3, 7, nfft, nov, fs), t[3:7])
        # the C entry writes the same bits
        G = gdsp._lib
        n = 8 * (nfft - nov) + nfft
        fr, tm = np.empty(p // 2 + 1), np.empty(9)
        ns, lp = G._I64(0), G._I64(0)
        G.check(G.lib().gdsp_spectrogram_batch(G._P(), 0, n, 0, fs, nfft, pad, nov, G._P(), G._P(),
                                               0, G._P(), fr.ctypes.data_as(G._P),
                                               tm.ctypes.data_as(G._P), ns, lp), "spectrogram")
        assert ns.value == 9 and lp.value == p // 2 + 1
        assert np.array_equal(fr, S.stft_freqs(p, fs)) and np.array_equal(tm, t)


def test_python_panics_and_empty_shapes(gdsp):
    S = gdsp.spectral
    o = S.PwelchOptions(NFFT=64)
    for batch in (S.StftBatch, S.SpectrogramBatch):
        with pytest.raises(gdsp.Panic, match="ragged input array") as e:
            batch([np.zeros(100), np.zeros(99)], 1.0, o)
        assert e.value.status == gdsp._lib.GDSP_ERR_RAGGED
        with pytest.raises(gdsp.Panic, match="nil pointer dereference"):
            batch(np.zeros((2, 100)), 1.0, None)
        with pytest.raises(gdsp.Panic, match="integer divide by zero"):
            batch(np.zeros((2, 100)), 1.0, S.PwelchOptions(NFFT=64, Noverlap=64))
        r, freqs, times = batch(np.zeros((3, 0)), 1.0, o)
        assert r.shape == (3, 0, 0) and freqs.shape == (0,) and times.shape == (0,)
        r, freqs, times = batch([[], []], 1.0, None)  # empty before the options are looked at
        assert r.shape == (2, 0, 0)
    assert S.StftBatch(np.zeros((3, 0)), 1.0, o)[0].dtype == np.complex128
    assert S.SpectrogramBatch(np.zeros((3, 0)), 1.0, o)[0].dtype == np.float64
    for one in (S.Stft, S.Spectrogram):
        with pytest.raises(gdsp.Panic, match="nil pointer dereference"):
            one(np.zeros(100), 1.0, None)
        r, freqs, times = one([], 1.0, o)
        assert r.shape == (0, 0) and freqs.shape == (0,) and times.shape == (0,)
    assert S.STFT_CHUNK_ELEMS == 1 << 25


# one shape of every class of the GPU table, and the materialised lengths
REFERENCE_SHAPES = [SG._shape(row)[:5] for row in SG.TABLE[::2]] + \
    [(100, 30, 100, 5, 4 * 70 + 102), (4096, 2048, 4096, 5, 4 * 2048 + 4098)]


@pytest.mark.parametrize("nfft,nov,pad,nsegs,n", REFERENCE_SHAPES,
                         ids=["%d-%d-%d-%d" % s[:4] for s in REFERENCE_SHAPES])
def test_the_two_references_agree(gdsp, oracle, nfft, nov, pad, nsegs, n):
    """The oracle's per-segment rows against numpy's on the exact segments, and
    the mean over segments of c_j |X|^2 / norm built from them against the
    oracle's Pwelch. Both are float64 transforms of the same rows: a power of 2
    differs by a few eps log2 F (2.7e-15 at F = 4096) and stays below 1e-14; the
    oracle's chirp-z for NFFT 100 (three transforms of 256 points and two chirp
    products, the worst row at 1.0e-14) below 1e-13: the oracle, which the GPU
    tests hold to TOL = 1e-9, sits four orders inside it, and numpy, which they
    hold to EXACT, is the other side of this comparison."""
    x = SG._signals(77, 2, n)
    ref_o, ref_n = SG._reference(oracle, x, nfft, nov, pad)
    assert ref_o.shape == (2, nsegs, pad // 2 + 1)
    err = row_nrel(SG._flat(ref_o), SG._flat(ref_n))
    print("oracle against numpy", nfft, err)
    assert err < (1e-14 if max(pad, nfft) & (max(pad, nfft) - 1) == 0 else 1e-13)
    for rows in (ref_o, ref_n):
        mean = SG._power(rows, nfft, pad).mean(axis=1)
        want = np.stack([oracle.pwelch(r, SG.FS, nfft=nfft, pad=pad, noverlap=nov)[0] for r in x])
        err = row_nrel(mean, want)
        print("mean against oracle.pwelch", nfft, err)
        assert err < 1e-14
