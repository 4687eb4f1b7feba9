"""CPU-only checks of the batched Pwelch boundary: the new entry points are
declared, exported and bound alike; their argument checks answer before any
device call; the flag that turns the batched kernel off is a known algorithm
bit; gdsp_pwelch_batch_fused (host arithmetic) says which shapes take the
kernel; and the Python mirror panics like Pwelch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

NAMES = ("gdsp_pwelch_batch", "gdsp_pwelch_batch_accumulate_device",
         "gdsp_pwelch_batch_finalize_device", "gdsp_pwelch_batch_fused",
         "gdsp_wav_read_floats_planar_device")


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
    # (x, channels, n, ldx, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off, pxx, freqs, lp)
    assert S["gdsp_pwelch_batch"] == (I, [P, I64, I64, I64, D, I64, I64, I64, P, P, I, P, P,
                                          ctypes.POINTER(I64)])
    # (d_x, channels, n, ldx, nfft, pad, noverlap, seg_begin, seg_end, d_win_seg, d_acc, stream)
    assert S["gdsp_pwelch_batch_accumulate_device"] == (
        I, [P, I64, I64, I64, I64, I64, I64, I64, I64, P, P, P])
    # (d_acc, channels, flen, nsegs, nfft, pad, win_nfft, fs, scale_off, d_pxx, freqs, stream)
    assert S["gdsp_pwelch_batch_finalize_device"] == (
        I, [P, I64, I64, I64, I64, I64, P, D, I, P, P, P])
    assert S["gdsp_pwelch_batch_fused"] == (I, [I64, I64, I64, I64, I64])
    # (d_in, frames, channels, audio_format, bits, d_out, ld_out, stream)
    assert S["gdsp_wav_read_floats_planar_device"] == (I, [P, I64, I64, I, I, P, I64, P])


def test_status_codes_before_any_device_call(gdsp):
    L = gdsp._lib.lib()
    G = gdsp._lib
    buf = np.zeros(4096)
    p = buf.ctypes.data_as(G._P)
    null = G._P()
    lp = G._I64(-1)
    f = L.gdsp_pwelch_batch
    # (x, channels, n, ldx, fs, nfft, pad, noverlap, wseg, wnfft, scale_off, pxx, freqs, lp)
    assert f(p, 2, 100, 100, 1.0, 64, 0, 0, null, null, 0, p, p, None) == G.GDSP_ERR_INVALID
    assert f(p, -1, 100, 100, 1.0, 64, 0, 0, null, null, 0, p, p, lp) == G.GDSP_ERR_INVALID
    assert f(p, 2, -1, 100, 1.0, 64, 0, 0, null, null, 0, p, p, lp) == G.GDSP_ERR_INVALID
    assert f(p, 2, 100, 99, 1.0, 64, 0, 0, null, null, 0, p, p, lp) == G.GDSP_ERR_INVALID
    assert f(p, 2, 100, 100, 1.0, -64, 0, 0, null, null, 0, p, p, lp) == G.GDSP_ERR_INVALID
    assert f(null, 2, 100, 100, 1.0, 64, 0, 0, null, null, 0, p, p, lp) == G.GDSP_ERR_INVALID
    assert f(p, 2, 100, 100, 1.0, 64, 0, 0, null, null, 0, null, p, lp) == G.GDSP_ERR_INVALID
    assert f(p, 2, 100, 100, 1.0, 64, 0, 0, null, null, 0, p, null, lp) == G.GDSP_ERR_INVALID
    # a zero stride: Segment's integer divide
    assert f(p, 2, 100, 100, 1.0, 64, 0, 64, null, null, 0, p, p, lp) == G.GDSP_ERR_DIVIDE_BY_ZERO
    # n == 0: empty results, whatever else is passed
    lp.value = -1
    assert f(null, 3, 0, 0, 1.0, 64, 0, 0, null, null, 0, null, null, lp) == G.GDSP_OK
    assert lp.value == 0
    # channels == 0: only freqs and the count are written
    pxx = np.full(40, -7.0)
    freqs = np.full(40, -7.0)
    assert f(null, 0, 100, 100, 8.0, 64, 0, 0, null, null, 0, pxx.ctypes.data_as(G._P),
             freqs.ctypes.data_as(G._P), lp) == G.GDSP_OK
    assert lp.value == 33
    assert np.array_equal(freqs[:33], np.arange(33) * (8.0 / 64)) and np.all(freqs[33:] == -7.0)
    assert np.all(pxx == -7.0)
    assert f(null, 0, 100, 100, 8.0, 64, 0, 0, null, null, 0, null, null, lp) == G.GDSP_ERR_INVALID

    a = L.gdsp_pwelch_batch_accumulate_device
    # (d_x, channels, n, ldx, nfft, pad, noverlap, seg_begin, seg_end, d_win, d_acc, stream)
    assert a(p, 2, 100, 100, 0, 64, 0, 0, 1, p, p, null) == G.GDSP_ERR_INVALID    # nfft <= 0
    assert a(p, 2, 100, 100, 64, 0, 0, 0, 1, p, p, null) == G.GDSP_ERR_INVALID    # pad <= 0
    assert a(p, 2, 100, 100, 64, 64, 0, -1, 1, p, p, null) == G.GDSP_ERR_INVALID  # seg_begin < 0
    assert a(p, 2, 100, 100, 64, 64, 0, 2, 1, p, p, null) == G.GDSP_ERR_INVALID   # end < begin
    assert a(p, -1, 100, 100, 64, 64, 0, 0, 1, p, p, null) == G.GDSP_ERR_INVALID  # channels < 0
    assert a(p, 2, -1, 100, 64, 64, 0, 0, 1, p, p, null) == G.GDSP_ERR_INVALID    # n < 0
    assert a(p, 2, 100, 99, 64, 64, 0, 0, 1, p, p, null) == G.GDSP_ERR_INVALID    # ldx < n
    assert a(p, 2, 100, 100, 64, 64, 0, 0, 3, p, p, null) == G.GDSP_ERR_INVALID   # past the signal
    assert a(null, 2, 100, 100, 64, 64, 0, 0, 1, p, p, null) == G.GDSP_ERR_INVALID
    assert a(p, 2, 100, 100, 64, 64, 0, 0, 1, null, p, null) == G.GDSP_ERR_INVALID
    assert a(p, 2, 100, 100, 64, 64, 0, 0, 1, p, null, null) == G.GDSP_ERR_INVALID
    assert a(null, 0, 100, 100, 64, 64, 0, 0, 1, null, null, null) == G.GDSP_OK   # no channels
    assert a(null, 2, 100, 100, 64, 64, 0, 1, 1, null, null, null) == G.GDSP_OK   # no segments

    z = L.gdsp_pwelch_batch_finalize_device
    # (d_acc, channels, flen, nsegs, nfft, pad, win_nfft, fs, scale_off, d_pxx, freqs, stream)
    assert z(p, -1, 64, 1, 64, 64, null, 1.0, 0, p, null, null) == G.GDSP_ERR_INVALID
    assert z(p, 2, 0, 1, 64, 64, null, 1.0, 0, p, null, null) == G.GDSP_ERR_INVALID
    assert z(p, 2, 64, 1, 0, 64, null, 1.0, 0, p, null, null) == G.GDSP_ERR_INVALID
    assert z(p, 2, 64, 1, 64, 0, null, 1.0, 0, p, null, null) == G.GDSP_ERR_INVALID
    assert z(null, 2, 64, 1, 64, 64, null, 1.0, 0, p, null, null) == G.GDSP_ERR_INVALID
    assert z(p, 2, 64, 1, 64, 64, null, 1.0, 0, null, null, null) == G.GDSP_ERR_INVALID
    fr = np.full(40, -7.0)
    assert z(null, 0, 64, 1, 64, 64, null, 8.0, 0, null, fr.ctypes.data_as(G._P),
             null) == G.GDSP_OK
    assert np.array_equal(fr[:33], np.arange(33) * (8.0 / 64)) and np.all(fr[33:] == -7.0)

    w = L.gdsp_wav_read_floats_planar_device
    # (d_in, frames, channels, audio_format, bits, d_out, ld_out, stream)
    assert w(p, -1, 2, 1, 16, p, 10, null) == G.GDSP_ERR_INVALID
    assert w(p, 10, -1, 1, 16, p, 10, null) == G.GDSP_ERR_INVALID
    assert w(p, 10, 2, 1, 16, p, 9, null) == G.GDSP_ERR_INVALID       # rows would overlap
    assert w(null, 10, 2, 1, 16, p, 10, null) == G.GDSP_ERR_INVALID
    assert w(p, 10, 2, 1, 16, null, 10, null) == G.GDSP_ERR_INVALID
    assert w(p, 10, 2, 1, 24, p, 10, null) == G.GDSP_ERR_UNSUPPORTED  # unknown bits per sample
    assert w(p, 10, 2, 2, 16, p, 10, null) == G.GDSP_ERR_UNSUPPORTED  # unknown audio format
    assert w(null, 0, 2, 1, 16, null, 0, null) == G.GDSP_OK
    assert w(null, 10, 0, 3, 32, null, 10, null) == G.GDSP_OK


def test_no_fused_pwelch_batch_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_PWELCH_BATCH == 128
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_PWELCH_BATCH)
        assert F.Algorithm() == F.ALGO_NO_FUSED_PWELCH_BATCH
        F.SetAlgorithm(F.ALGO_NO_FUSED_PWELCH_BATCH | F.ALGO_NO_FUSED_CONVOLVE)
        assert F.Algorithm() == F.ALGO_NO_FUSED_PWELCH_BATCH | F.ALGO_NO_FUSED_CONVOLVE
        with pytest.raises(gdsp.GDSPError) as e:
            F.SetAlgorithm(1 << 20)
        assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == F.ALGO_NO_FUSED_PWELCH_BATCH | F.ALGO_NO_FUSED_CONVOLVE
    finally:
        F.SetAlgorithm(prev)


FUSED = ((64, 0, 0), (256, 0, 128), (512, 1024, 256), (2048, 0, 1024), (1024, 512, 0))
LOOP = ((32, 0, 0), (4096, 0, 2048), (3000, 0, 0), (100, 0, 0), (16, 32, 0), (512, 4096, 0),
        (256, 0, 256 - (1 << 23)))


def test_fused_query_is_host_arithmetic(gdsp):
    F = gdsp.fft
    q = gdsp.spectral.pwelch_batch_fused
    for nfft, pad, nov in FUSED:
        assert q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    for nfft, pad, nov in LOOP:
        assert not q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    assert q(5, 4096)  # the defaults: NFFT 256
    # a stride of exactly 2^22 is the last one the kernels address
    assert q(5, 4096, 256, 0, 256 - (1 << 22)) and not q(5, 4096, 256, 0, 255 - (1 << 22))
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_PWELCH_BATCH)
        for nfft, pad, nov in FUSED + LOOP:
            assert not q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    finally:
        F.SetAlgorithm(prev)
    for nfft, pad, nov in FUSED:
        assert q(5, 4096, nfft, pad, nov), (nfft, pad, nov)


def test_python_panics_and_empty_rows(gdsp):
    S = gdsp.spectral
    o = S.PwelchOptions(NFFT=64)
    with pytest.raises(gdsp.Panic, match="ragged input array") as e:
        S.PwelchBatch([np.zeros(100), np.zeros(99)], 1.0, o)
    assert e.value.status == gdsp._lib.GDSP_ERR_RAGGED
    with pytest.raises(gdsp.Panic, match="nil pointer dereference"):
        S.PwelchBatch(np.zeros((2, 100)), 1.0, None)
    pxx, freqs = S.PwelchBatch(np.zeros((3, 0)), 1.0, o)
    assert pxx.shape == (3, 0) and freqs.shape == (0,)
    pxx, freqs = S.PwelchBatch([[], []], 1.0, o)
    assert pxx.shape == (2, 0) and freqs.shape == (0,)
    with pytest.raises(gdsp.Panic, match="integer divide by zero"):
        S.PwelchBatch(np.zeros((2, 100)), 1.0, S.PwelchOptions(NFFT=64, Noverlap=64))
