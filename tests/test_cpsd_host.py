"""CPU-only checks of the cross-spectral boundary (Cpsd, Coherence, CpsdBatch):
the four entry points are declared, exported and bound alike; their argument
checks answer before any device call; the flag that turns the fused kernel off
is a known algorithm bit; gdsp_cpsd_batch_fused (host arithmetic) says which
shapes take the kernel; and the Python mirror panics like Pwelch and
Convolve."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

NAMES = ("gdsp_cpsd_batch", "gdsp_cpsd_batch_accumulate_device",
         "gdsp_cpsd_batch_finalize_device", "gdsp_cpsd_batch_fused")


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
    # (x, ldx, y, ldy, y_rows, channels, n, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off,
    #  pxy, pxx, pyy, coh, freqs, lp)
    assert S["gdsp_cpsd_batch"] == (I, [P, I64, P, I64, I64, I64, I64, D, I64, I64, I64, P, P, I,
                                        P, P, P, P, P, ctypes.POINTER(I64)])
    # (d_x, ldx, d_y, ldy, y_rows, channels, n, nfft, pad, noverlap, seg_begin, seg_end,
    #  d_win_seg, d_acc, stream)
    assert S["gdsp_cpsd_batch_accumulate_device"] == (
        I, [P, I64, P, I64, I64, I64, I64, I64, I64, I64, I64, I64, P, P, P])
    # (d_acc, channels, flen, nsegs, nfft, pad, win_nfft, fs, scale_off, d_pxy, d_pxx, d_pyy,
    #  d_coh, freqs, stream)
    assert S["gdsp_cpsd_batch_finalize_device"] == (
        I, [P, I64, I64, I64, I64, I64, P, D, I, P, P, P, P, P, P])
    assert S["gdsp_cpsd_batch_fused"] == (I, [I64, I64, I64, I64, I64])


def test_status_codes_before_any_device_call(gdsp):
    L = gdsp._lib.lib()
    G = gdsp._lib
    buf = np.zeros(4096)
    p = buf.ctypes.data_as(G._P)
    null = G._P()
    lp = G._I64(-1)
    f = L.gdsp_cpsd_batch

    def host(x=p, ldx=100, y=p, ldy=100, y_rows=2, channels=2, n=100, nfft=64, pad=0, nov=0,
             pxy=p, pxx=p, pyy=p, coh=p, freqs=p, lpo=lp, fs=1.0):
        return f(x, ldx, y, ldy, y_rows, channels, n, fs, nfft, pad, nov, null, null, 0, pxy, pxx,
                 pyy, coh, freqs, lpo)

    assert host(lpo=None) == G.GDSP_ERR_INVALID
    assert host(channels=-1, y_rows=1) == G.GDSP_ERR_INVALID
    assert host(n=-1) == G.GDSP_ERR_INVALID
    assert host(ldx=99) == G.GDSP_ERR_INVALID
    assert host(ldy=99) == G.GDSP_ERR_INVALID
    assert host(nfft=-64) == G.GDSP_ERR_INVALID
    assert host(pad=-64) == G.GDSP_ERR_INVALID
    assert host(x=null) == G.GDSP_ERR_INVALID
    assert host(y=null) == G.GDSP_ERR_INVALID
    assert host(pxy=null) == G.GDSP_ERR_INVALID
    assert host(freqs=null) == G.GDSP_ERR_INVALID
    # y is one row or one per channel
    assert host(y_rows=3) == G.GDSP_ERR_UNEQUAL
    assert host(y_rows=0) == G.GDSP_ERR_UNEQUAL
    assert host(channels=3, y_rows=2) == G.GDSP_ERR_UNEQUAL
    # a zero stride: Segment's integer divide
    assert host(nov=64) == G.GDSP_ERR_DIVIDE_BY_ZERO
    # n == 0: empty results, whatever else is passed
    lp.value = -1
    assert host(x=null, y=null, n=0, ldx=0, ldy=0, channels=3, y_rows=7, pxy=null, pxx=null,
                pyy=null, coh=null, freqs=null) == G.GDSP_OK
    assert lp.value == 0
    # channels == 0: only freqs and the count are written
    outs = [np.full(80, -7.0) for _ in range(4)]
    freqs = np.full(40, -7.0)
    ptrs = [o.ctypes.data_as(G._P) for o in outs]
    for y_rows in (0, 1):
        lp.value = -1
        freqs[:] = -7.0
        assert host(x=null, y=null, channels=0, y_rows=y_rows, pxy=ptrs[0], pxx=ptrs[1],
                    pyy=ptrs[2], coh=ptrs[3], freqs=freqs.ctypes.data_as(G._P),
                    fs=8.0) == G.GDSP_OK
        assert lp.value == 33
        assert np.array_equal(freqs[:33], np.arange(33) * (8.0 / 64)) and np.all(freqs[33:] == -7.0)
        assert all(np.all(o == -7.0) for o in outs)
    assert host(x=null, y=null, channels=0, y_rows=1, freqs=null) == G.GDSP_ERR_INVALID

    a = L.gdsp_cpsd_batch_accumulate_device

    def accum(x=p, ldx=100, y=p, ldy=100, y_rows=2, channels=2, n=100, nfft=64, pad=64, nov=0,
              b=0, e=1, win=p, acc=p):
        return a(x, ldx, y, ldy, y_rows, channels, n, nfft, pad, nov, b, e, win, acc, null)

    assert accum(nfft=0) == G.GDSP_ERR_INVALID
    assert accum(pad=0) == G.GDSP_ERR_INVALID
    assert accum(b=-1) == G.GDSP_ERR_INVALID
    assert accum(b=2, e=1) == G.GDSP_ERR_INVALID
    assert accum(channels=-1, y_rows=1) == G.GDSP_ERR_INVALID
    assert accum(n=-1) == G.GDSP_ERR_INVALID
    assert accum(ldx=99) == G.GDSP_ERR_INVALID
    assert accum(ldy=99) == G.GDSP_ERR_INVALID
    assert accum(e=3) == G.GDSP_ERR_INVALID                    # past the signal
    assert accum(nov=-36, e=2) == G.GDSP_ERR_INVALID           # stride 100: segment 1 past it
    assert accum(x=null) == G.GDSP_ERR_INVALID
    assert accum(y=null) == G.GDSP_ERR_INVALID
    assert accum(win=null) == G.GDSP_ERR_INVALID
    assert accum(acc=null) == G.GDSP_ERR_INVALID
    assert accum(y_rows=3) == G.GDSP_ERR_UNEQUAL
    assert accum(channels=3, y_rows=2) == G.GDSP_ERR_UNEQUAL
    assert accum(nov=64, e=2) == G.GDSP_ERR_DIVIDE_BY_ZERO
    assert accum(x=null, y=null, win=null, acc=null, channels=0, y_rows=1) == G.GDSP_OK
    assert accum(x=null, y=null, win=null, acc=null, b=1, e=1) == G.GDSP_OK  # no segments

    z = L.gdsp_cpsd_batch_finalize_device

    def fin(acc=p, channels=2, flen=64, nsegs=1, nfft=64, pad=64, pxy=p, freqs=null, fs=1.0):
        return z(acc, channels, flen, nsegs, nfft, pad, null, fs, 0, pxy, null, null, null, freqs,
                 null)

    assert fin(channels=-1) == G.GDSP_ERR_INVALID
    assert fin(flen=0) == G.GDSP_ERR_INVALID
    assert fin(nfft=0) == G.GDSP_ERR_INVALID
    assert fin(pad=0) == G.GDSP_ERR_INVALID
    assert fin(nsegs=-1) == G.GDSP_ERR_INVALID
    assert fin(acc=null) == G.GDSP_ERR_INVALID
    assert fin(flen=64, pad=128) == G.GDSP_ERR_INVALID  # accumulators shorter than Pad / 2 + 1
    fr = np.full(40, -7.0)
    assert fin(acc=null, channels=0, pxy=null, freqs=fr.ctypes.data_as(G._P), fs=8.0) == G.GDSP_OK
    assert np.array_equal(fr[:33], np.arange(33) * (8.0 / 64)) and np.all(fr[33:] == -7.0)
    # every output NULL: nothing to do, the frequencies still written
    fr[:] = -7.0
    assert fin(pxy=null, freqs=fr.ctypes.data_as(G._P), fs=8.0) == G.GDSP_OK
    assert np.array_equal(fr[:33], np.arange(33) * (8.0 / 64))


def test_no_fused_cpsd_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_CPSD == 256
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_CPSD)
        assert F.Algorithm() == F.ALGO_NO_FUSED_CPSD
        F.SetAlgorithm(F.ALGO_NO_FUSED_CPSD | F.ALGO_NO_FUSED_PWELCH_BATCH)
        assert F.Algorithm() == F.ALGO_NO_FUSED_CPSD | F.ALGO_NO_FUSED_PWELCH_BATCH
        with pytest.raises(gdsp.GDSPError) as e:
            F.SetAlgorithm(1 << 20)
        assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == F.ALGO_NO_FUSED_CPSD | F.ALGO_NO_FUSED_PWELCH_BATCH
    finally:
        F.SetAlgorithm(prev)


FUSED = ((64, 0, 0), (256, 0, 128), (512, 1024, 256), (2048, 0, 1024))
MATERIALISED = ((32, 0, 0), (4096, 0, 2048), (3000, 0, 0), (256, 0, 256 - (1 << 22) - 1))


def test_fused_query_is_host_arithmetic(gdsp):
    F = gdsp.fft
    q = gdsp.spectral.cpsd_batch_fused
    for nfft, pad, nov in FUSED:
        assert q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    for nfft, pad, nov in MATERIALISED:
        assert not q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    assert q(5, 4096)  # the defaults: NFFT 256
    assert q(5, 4096, 256, 0, 256 - (1 << 22))  # the last stride the kernel addresses
    prev = F.Algorithm()
    try:
        # the Pwelch flag does not touch the cross spectra, the Cpsd flag does
        F.SetAlgorithm(F.ALGO_NO_FUSED_PWELCH_BATCH)
        assert q(5, 4096, 256, 0, 128) and not gdsp.spectral.pwelch_batch_fused(5, 4096, 256, 0, 128)
        F.SetAlgorithm(F.ALGO_NO_FUSED_CPSD)
        assert gdsp.spectral.pwelch_batch_fused(5, 4096, 256, 0, 128)
        for nfft, pad, nov in FUSED + MATERIALISED:
            assert not q(5, 4096, nfft, pad, nov), (nfft, pad, nov)
    finally:
        F.SetAlgorithm(prev)
    for nfft, pad, nov in FUSED:
        assert q(5, 4096, nfft, pad, nov), (nfft, pad, nov)


def test_python_panics_and_empty_shapes(gdsp):
    S = gdsp.spectral
    o = S.PwelchOptions(NFFT=64)
    with pytest.raises(gdsp.Panic, match="ragged input array") as e:
        S.CpsdBatch([np.zeros(100), np.zeros(99)], np.zeros(100), 1.0, o)
    assert e.value.status == gdsp._lib.GDSP_ERR_RAGGED
    for y in (np.zeros(99), np.zeros((3, 100)), np.zeros((2, 99)), np.zeros((1, 100)),
              [np.zeros(100), np.zeros(99)]):
        with pytest.raises(gdsp.Panic, match="arrays not of equal size") as e:
            S.CpsdBatch(np.zeros((2, 100)), y, 1.0, o)
        assert e.value.status == gdsp._lib.GDSP_ERR_UNEQUAL
    with pytest.raises(gdsp.Panic, match="arrays not of equal size"):
        S.Cpsd(np.zeros(100), np.zeros(99), 1.0, o)
    with pytest.raises(gdsp.Panic, match="arrays not of equal size"):
        S.Coherence(np.zeros(100), np.zeros(101), 1.0, o)
    for call in (lambda: S.CpsdBatch(np.zeros((2, 100)), np.zeros(100), 1.0, None),
                 lambda: S.Cpsd(np.zeros(100), np.zeros(100), 1.0, None),
                 lambda: S.Coherence(np.zeros(100), np.zeros(100), 1.0, None)):
        with pytest.raises(gdsp.Panic, match="nil pointer dereference"):
            call()
    r = S.CpsdBatch(np.zeros((3, 0)), np.zeros(0), 1.0, o)
    assert isinstance(r, S.CrossSpectra)
    assert r.Pxy.shape == (3, 0) and r.Pxy.dtype == np.complex128
    assert r.Pxx.shape == r.Pyy.shape == r.Cxy.shape == (3, 0) and r.freqs.shape == (0,)
    r = S.CpsdBatch([[], []], [[], []], 1.0, None)  # empty before the options are looked at
    assert r.Pxy.shape == (2, 0) and r.freqs.shape == (0,)
    pxy, freqs = S.Cpsd([], [], 1.0, o)
    assert pxy.shape == (0,) and pxy.dtype == np.complex128 and freqs.shape == (0,)
    cxy, freqs = S.Coherence([], [], 1.0, o)
    assert cxy.shape == (0,) and freqs.shape == (0,)
    with pytest.raises(gdsp.Panic, match="integer divide by zero"):
        S.CpsdBatch(np.zeros((2, 100)), np.zeros(100), 1.0, S.PwelchOptions(NFFT=64, Noverlap=64))
