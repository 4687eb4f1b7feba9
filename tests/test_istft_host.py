"""CPU-only checks of the ISTFT's boundary (Istft, IstftBatch, gdsp_istft_batch,
gdsp_istft_batch_device, gdsp_istft_batch_fused): the entry points are declared,
exported and bound alike; their argument checks answer before any device call;
GDSP_ALGO_NO_FUSED_ISTFT is the known bit 4096 and 2048 stays unknown; the
fused query is host arithmetic; the Python mirrors panic and return shaped
empties; and the numpy model the GPU tests compare with (istft_ref.py) returns
its own input far inside the GPU tests' two bounds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import istft_ref as R
from conftest import REPO

TOL = 1e-9     # the unweighted error over D > 0
EXACT = 1e-13  # the weighted error (istft_ref.weighted_err)

NAMES = ("gdsp_istft_batch", "gdsp_istft_batch_device", "gdsp_istft_batch_fused")


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
    P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    PI64 = ctypes.POINTER(I64)
    # (X, channels, nsegs, nfft, pad, noverlap, win_seg, n, out, ldo, n_out)
    assert S["gdsp_istft_batch"] == (I, [P, I64, I64, I64, I64, I64, P, I64, P, I64, PI64])
    assert S["gdsp_istft_batch_fused"] == (I, [I64, I64, I64, I64, I64])
    # (d_X, ld_seg, ld_chan, channels, nsegs, seg_row0, seg_rows, nfft, pad, noverlap, d_win_seg,
    #  out_begin, out_end, d_out, ldo, stream)
    assert S["gdsp_istft_batch_device"] == (I, [P, I64, I64, I64, I64, I64, I64, I64, I64, I64, P,
                                                I64, I64, P, I64, P])
    hdr = open(os.path.join(REPO, "include", "gdsp_fft.h")).read()
    assert "GDSP_ALGO_NO_FUSED_ISTFT = 4096" in hdr
    assert "2048" in hdr.split("GDSP_ALGO_NO_FUSED_ISTFT = 4096")[0].rsplit("/*", 1)[1]
    assert "ISTFT" in hdr.split("---- values")[1].split("---- fft package")[0]


def test_device_entry_status_codes_before_any_device_call(gdsp):
    G = gdsp._lib
    f = G.lib().gdsp_istft_batch_device
    buf = np.zeros(4096)
    p = buf.ctypes.data_as(G._P)
    null = G._P()

    # 2 channels of 4 rows of lp = 33 (NFFT 64, stride 32): n_full = 160
    def call(X=p, ld_seg=33, ld_chan=4 * 33, channels=2, nsegs=4, row0=0, rows=4, nfft=64, pad=64,
             nov=32, win=p, b=0, e=160, out=p, ldo=160):
        return f(X, ld_seg, ld_chan, channels, nsegs, row0, rows, nfft, pad, nov, win, b, e, out,
                 ldo, null)

    assert call(nfft=0) == G.GDSP_ERR_INVALID
    assert call(nfft=-64) == G.GDSP_ERR_INVALID
    assert call(pad=32) == G.GDSP_ERR_INVALID            # Pad below NFFT: no inverse
    assert call(pad=0) == G.GDSP_ERR_INVALID             # the device entry takes no defaults
    assert call(channels=-1) == G.GDSP_ERR_INVALID
    assert call(nsegs=-1) == G.GDSP_ERR_INVALID
    assert call(row0=-1) == G.GDSP_ERR_INVALID
    assert call(rows=-1) == G.GDSP_ERR_INVALID
    assert call(row0=1, rows=4) == G.GDSP_ERR_INVALID    # rows past nsegs
    assert call(ld_seg=32) == G.GDSP_ERR_INVALID         # rows of lp = 33
    assert call(pad=128, ld_seg=64, ld_chan=256) == G.GDSP_ERR_INVALID  # lp = 65
    assert call(ld_chan=4 * 33 - 1) == G.GDSP_ERR_INVALID
    assert call(ld_seg=40, ld_chan=159) == G.GDSP_ERR_INVALID
    assert call(ldo=159) == G.GDSP_ERR_INVALID
    assert call(b=-1) == G.GDSP_ERR_INVALID
    assert call(b=100, e=99) == G.GDSP_ERR_INVALID       # reversed
    assert call(e=161) == G.GDSP_ERR_INVALID             # past n_full
    assert call(nov=100, e=10) == G.GDSP_ERR_INVALID     # a negative stride with nsegs > 1
    # missing rows: sample 63 needs row 0, sample 128 needs row 3
    assert call(row0=1, rows=3, ld_chan=3 * 33, b=63, e=100) == G.GDSP_ERR_INVALID
    assert call(row0=0, rows=3, ld_chan=3 * 33, b=0, e=129) == G.GDSP_ERR_INVALID
    # this shape runs the fused kernel, which needs whole pairs (2p, 2p + 1): sample
    # 64 needs row 1 and with it row 0, sample 95 needs row 2 and with it row 3
    assert call(row0=1, rows=3, ld_chan=3 * 33, b=64, e=160) == G.GDSP_ERR_INVALID
    assert call(row0=0, rows=3, ld_chan=3 * 33, b=0, e=96) == G.GDSP_ERR_INVALID
    assert call(X=null) == G.GDSP_ERR_INVALID
    assert call(win=null) == G.GDSP_ERR_INVALID
    assert call(out=null) == G.GDSP_ERR_INVALID
    # a zero stride: only past one segment
    assert call(nov=64, e=64) == G.GDSP_ERR_DIVIDE_BY_ZERO
    # nothing to do: nothing is looked at
    assert call(X=null, win=null, out=null, channels=0) == G.GDSP_OK
    assert call(X=null, win=null, out=null, nsegs=0, rows=0, e=0, ldo=0) == G.GDSP_OK
    assert call(X=null, win=null, out=null, b=77, e=77, ldo=0) == G.GDSP_OK
    assert call(nsegs=0, rows=0, e=1) == G.GDSP_ERR_INVALID
    if gdsp.device_count() == 0:
        assert call() == G.GDSP_ERR_NO_DEVICE
        assert call(row0=2, rows=2, ld_chan=2 * 33, b=96, e=160) == G.GDSP_ERR_NO_DEVICE
        assert call(row0=0, rows=2, ld_chan=2 * 33, b=0, e=64) == G.GDSP_ERR_NO_DEVICE
        # the materialised form (NFFT 100) transforms every row alone: the needed rows suffice
        assert call(row0=1, rows=3, ld_seg=51, ld_chan=3 * 51, nfft=100, pad=100, nov=50, b=100,
                    e=250, ldo=150) == G.GDSP_ERR_NO_DEVICE
        # a range inside a gap between segments needs no row
        assert call(row0=3, rows=1, ld_chan=33, nov=-64, b=64, e=128, ldo=64) == G.GDSP_ERR_NO_DEVICE
        assert call(nsegs=1, rows=1, ld_chan=33, nov=64, e=64, ldo=64) == G.GDSP_ERR_NO_DEVICE


def test_host_entry_status_codes_before_any_device_call(gdsp):
    G = gdsp._lib
    f = G.lib().gdsp_istft_batch
    buf = np.zeros(8192)
    p = buf.ctypes.data_as(G._P)
    null = G._P()
    no = G._I64(-1)

    def call(X=p, channels=2, nsegs=4, nfft=64, pad=0, nov=32, n=0, out=p, ldo=160, n_out=no):
        return f(X, channels, nsegs, nfft, pad, nov, null, n, out, ldo, n_out)

    assert call(n_out=None) == G.GDSP_ERR_INVALID
    assert call(channels=-1) == G.GDSP_ERR_INVALID
    assert call(nsegs=-1) == G.GDSP_ERR_INVALID
    assert call(n=-1) == G.GDSP_ERR_INVALID
    assert call(nfft=-64) == G.GDSP_ERR_INVALID
    assert call(pad=-64) == G.GDSP_ERR_INVALID
    assert call(pad=32) == G.GDSP_ERR_INVALID            # Pad below NFFT
    assert call(nfft=0, pad=128) == G.GDSP_ERR_INVALID   # NFFT 256 by default
    assert call(n=161) == G.GDSP_ERR_INVALID             # n_full = 160
    assert call(ldo=159) == G.GDSP_ERR_INVALID
    assert call(n=100, ldo=99) == G.GDSP_ERR_INVALID
    assert call(X=null) == G.GDSP_ERR_INVALID
    assert call(out=null) == G.GDSP_ERR_INVALID
    assert call(nov=100) == G.GDSP_ERR_INVALID           # a negative stride
    assert call(nov=64) == G.GDSP_ERR_DIVIDE_BY_ZERO
    # the counts written on the OK paths
    no.value = -1
    assert call(X=null, out=null, nsegs=0) == G.GDSP_OK
    assert no.value == 0
    no.value = -1
    assert call(X=null, out=null, channels=0) == G.GDSP_OK
    assert no.value == 160
    no.value = -1
    assert call(X=null, out=null, channels=0, n=100) == G.GDSP_OK
    assert no.value == 100
    no.value = -1
    assert call(X=null, out=null, channels=0, nsegs=1, nov=64) == G.GDSP_OK  # one segment
    assert no.value == 64
    assert call(X=null, out=null, channels=0, nfft=0, nov=128) == G.GDSP_OK  # NFFT 256, Pad 256
    assert no.value == 3 * 128 + 256
    assert call(nsegs=0, n=1) == G.GDSP_ERR_INVALID
    if gdsp.device_count() == 0:
        assert call() == G.GDSP_ERR_NO_DEVICE
        assert call(n=100, ldo=100) == G.GDSP_ERR_NO_DEVICE


def test_no_fused_istft_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_ISTFT == 4096
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_ISTFT)
        assert F.Algorithm() == 4096
        F.SetAlgorithm(F.ALGO_NO_FUSED_ISTFT | F.ALGO_NO_FUSED_STFT)
        assert F.Algorithm() == 4096 | 1024
        for bad in (2048, 1 << 20, 4096 | 2048):
            with pytest.raises(gdsp.GDSPError) as e:
                F.SetAlgorithm(bad)
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == 4096 | 1024
    finally:
        F.SetAlgorithm(prev)


# (nfft, pad, noverlap)
FUSED = ((64, 0, 0), (256, 0, 128), (256, 0, 192), (512, 1024, 256), (2048, 0, 1024))
MATERIALISED = ((256, 0, 193), (32, 0, 0), (4096, 0, 2048), (100, 0, 30), (64, 0, 63))


def test_fused_query_is_host_arithmetic(gdsp):
    F = gdsp.fft
    S = gdsp.spectral
    q = S.istft_batch_fused
    for nfft, pad, nov in FUSED:
        assert q(5, 11, nfft, pad, nov), (nfft, pad, nov)
    for nfft, pad, nov in MATERIALISED:
        assert not q(5, 11, nfft, pad, nov), (nfft, pad, nov)
    assert q(5, 11)                          # the defaults: NFFT 256, no overlap
    assert not q(5, 11, 256, 128, 0)         # Pad below NFFT
    assert not q(5, 11, 256, 0, -1)          # gaps between the segments
    assert not q(5, 11, 256, 0, 256)         # a zero stride
    assert not q(-1, 11) and not q(5, -1) and not q(5, 11, -256)
    prev = F.Algorithm()
    try:
        # the flags of the other fused kernels do not touch this one, its own does
        F.SetAlgorithm(F.ALGO_NO_FUSED_STFT | F.ALGO_NO_FUSED_PWELCH_BATCH | F.ALGO_NO_FUSED_CPSD)
        assert q(5, 11, 256, 0, 128)
        F.SetAlgorithm(F.ALGO_NO_FUSED_ISTFT)
        assert S.stft_batch_fused(5, 4096, 256, 0, 128)
        assert S.pwelch_batch_fused(5, 4096, 256, 0, 128)
        assert S.cpsd_batch_fused(5, 4096, 256, 0, 128)
        for nfft, pad, nov in FUSED + MATERIALISED:
            assert not q(5, 11, nfft, pad, nov), (nfft, pad, nov)
    finally:
        F.SetAlgorithm(prev)
    for nfft, pad, nov in FUSED:
        assert q(5, 11, nfft, pad, nov), (nfft, pad, nov)


def test_python_panics_and_empty_shapes(gdsp):
    S = gdsp.spectral
    o = S.PwelchOptions(NFFT=64, Noverlap=32)
    X = np.zeros((2, 4, 33), np.complex128)
    with pytest.raises(gdsp.Panic, match="nil pointer dereference"):
        S.IstftBatch(X, None)
    with pytest.raises(gdsp.Panic, match="Pad below NFFT") as e:
        S.IstftBatch(np.zeros((2, 4, 17), np.complex128), S.PwelchOptions(NFFT=64, Pad=32))
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    with pytest.raises(gdsp.Panic, match="33 expected") as e:
        S.IstftBatch(np.zeros((2, 4, 32), np.complex128), o)
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    with pytest.raises(gdsp.Panic, match="65 expected"):
        S.Istft(np.zeros((4, 33), np.complex128), S.PwelchOptions(NFFT=64, Pad=128))
    with pytest.raises(gdsp.Panic, match="integer divide by zero"):
        S.IstftBatch(X, S.PwelchOptions(NFFT=64, Noverlap=64))
    with pytest.raises(gdsp.Panic, match="outside"):
        S.IstftBatch(X, o, n=161)
    with pytest.raises(gdsp.Panic):
        S.IstftBatch(np.zeros((4, 33), np.complex128), o)   # not three axes
    with pytest.raises(gdsp.Panic):
        S.Istft(X, o)                                        # not two axes
    # what StftBatch / Stft return for an empty signal, options not looked at
    r = S.IstftBatch(np.zeros((3, 0, 0), np.complex128), None)
    assert r.shape == (3, 0) and r.dtype == np.float64
    assert S.IstftBatch(S.StftBatch(np.zeros((3, 0)), 1.0, o)[0], o).shape == (3, 0)
    assert S.Istft(S.Stft([], 1.0, o)[0], o).shape == (0,)
    assert S.IstftBatch(np.zeros((0, 4, 33), np.complex128), o).shape == (0, 160)
    assert S.IstftBatch(X, o, n=0).shape == (2, 0)
    assert S.ISTFT_CHUNK_ELEMS == 1 << 25
    assert S.istft_length(4, 64, 32) == 160 and S.istft_length(0, 64, 32) == 0


# (nfft, noverlap, pad): NFFT 64 to 4096, also 100 and Pad = 2 NFFT; no overlap,
# half, odd and 75 %
MODEL_SHAPES = ((64, 0, 64), (64, 32, 64), (64, 48, 64), (64, 17, 64), (100, 30, 100),
                (256, 128, 256), (256, 192, 512), (1024, 512, 1024), (1024, 257, 1024),
                (2048, 1024, 2048), (2048, 1536, 2048), (4096, 2048, 4096), (4096, 0, 4096))
MODEL_SEGS = 11


@pytest.mark.parametrize("win", ("Hann", "Rectangular", "Hamming"))
def test_the_model_returns_its_input(gdsp, win):
    """The reference's own error, with the library's window tables: the round
    trip of istft_ref.istft on numpy.fft.rfft of the windowed segments against
    the signal. Measured at most 3.6e-16 weighted and 2.0e-10 unweighted (Hann
    at 4096 without overlap, whose second sample has the weight 5.9e-7^2 alone):
    about 300 and 5 times inside the two bounds the GPU tests hold the engine to."""
    worst_w = worst_p = 0.0
    for k, (nfft, nov, pad) in enumerate(MODEL_SHAPES):
        stride = nfft - nov
        w = np.asarray(getattr(gdsp.window, win)(pad), dtype=np.float64)
        n = gdsp.spectral.istft_length(MODEL_SEGS, nfft, nov)
        assert n == R.n_full(MODEL_SEGS, nfft, stride)
        x = np.random.default_rng(100 + k).standard_normal((1, n))
        X = R.stft_rows(x, w, nfft, stride, pad, MODEL_SEGS)
        out, D = R.istft(X[0], w, nfft, stride, pad)
        assert out.shape == (n,)
        assert np.all(out[D == 0] == 0.0)
        want = np.where(D > 0, x[0], 0.0)
        ew, ep = R.weighted_err(out, want, D), R.plain_err(out, want, D)
        print(win, nfft, nov, pad, "weighted %.2e plain %.2e zeros %d" % (ew, ep, int((D == 0).sum())))
        worst_w, worst_p = max(worst_w, ew), max(worst_p, ep)
        if win == "Hann":  # zero at both ends (of F: a window cut at NFFT < F has one zero)
            assert D[0] == 0 and (D[-1] == 0 or pad > nfft)
            if nov == 0 and pad == nfft:
                assert int((D == 0).sum()) == 2 * MODEL_SEGS
    assert worst_w < EXACT and worst_p < TOL, (worst_w, worst_p)
