"""CPU-only checks of the batched Convolve boundary: the three entry points are
declared, exported and bound alike; their argument checks answer before any
device call; the Python mirror panics like fft.Convolve on mismatched shapes;
and the flag that turns the fused kernel off is a known algorithm bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

NAMES = ("gdsp_convolve_batch", "gdsp_convolve_batch_device", "gdsp_convolve_fused")


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
    assert S["gdsp_convolve_batch"] == (I, [P, P, P, I64, I64, I64])
    assert S["gdsp_convolve_batch_device"] == (I, [P, P, P, I64, P, I64, P, P])
    assert S["gdsp_convolve_fused"] == (I, [P])


def test_status_codes_before_any_device_call(gdsp):
    L = gdsp._lib.lib()
    G = gdsp._lib
    buf = np.zeros(64)
    p = buf.ctypes.data_as(G._P)
    null = G._P()
    f = L.gdsp_convolve_batch
    assert f(p, p, p, -1, 2, 1) == G.GDSP_ERR_INVALID       # n < 0
    assert f(p, p, p, 4, -1, 1) == G.GDSP_ERR_INVALID       # batch < 0
    assert f(p, p, p, 4, 3, 2) == G.GDSP_ERR_INVALID        # y_rows neither 1 nor batch
    assert f(p, p, p, 4, 3, 0) == G.GDSP_ERR_INVALID
    assert f(null, p, p, 4, 2, 1) == G.GDSP_ERR_INVALID     # NULL with batch > 0
    assert f(p, null, p, 4, 2, 2) == G.GDSP_ERR_INVALID
    assert f(p, p, null, 4, 2, 1) == G.GDSP_ERR_INVALID
    assert f(p, p, p, 0, 2, 1) == G.GDSP_ERR_EMPTY          # the reference's IFFT panics
    assert f(p, p, p, 0, 2, 2) == G.GDSP_ERR_EMPTY
    assert f(p, p, p, 4, 0, 1) == G.GDSP_OK                 # nothing to do
    assert f(null, null, null, 4, 0, 0) == G.GDSP_OK
    assert f(null, null, null, 0, 0, 1) == G.GDSP_OK
    # the device entry takes n from its plan: without one it is invalid, and
    # no plan is "not fused"
    d = L.gdsp_convolve_batch_device
    assert d(null, p, p, 1, p, 2, null, null) == G.GDSP_ERR_INVALID
    assert L.gdsp_convolve_fused(null) == 0


def test_python_panics_on_mismatched_shapes(gdsp):
    F = gdsp.fft
    x = np.zeros((3, 8), np.complex128)
    for y in (np.zeros(7), np.zeros(9), np.zeros((2, 8)), np.zeros((3, 7)), np.zeros((1, 8)),
              np.zeros((3, 8, 1)), np.zeros(())):
        with pytest.raises(gdsp.Panic, match="arrays not of equal size"):
            F.ConvolveBatch(x, y)
    # an empty batch asks nothing of the device
    assert F.ConvolveBatch(np.zeros((0, 8)), np.zeros(8)).shape == (0, 8)


def test_no_fused_convolve_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_CONVOLVE == 64
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_CONVOLVE)
        assert F.Algorithm() == F.ALGO_NO_FUSED_CONVOLVE
        F.SetAlgorithm(F.ALGO_NO_FUSED_CONVOLVE | F.ALGO_NO_RACE)
        assert F.Algorithm() == F.ALGO_NO_FUSED_CONVOLVE | F.ALGO_NO_RACE
        with pytest.raises(gdsp.GDSPError) as e:
            F.SetAlgorithm(1 << 20)
        assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == F.ALGO_NO_FUSED_CONVOLVE | F.ALGO_NO_RACE
    finally:
        F.SetAlgorithm(prev)
