"""CPU-only checks of the FIR filtering boundary: the three entry points are
declared, exported and bound alike; every status code of the header's table
answers before any device call; gdsp_fir_block is deterministic host
arithmetic with the documented range; the Python mirrors panic or raise like
the existing ones; and the flag that turns the fused kernel off is a known
algorithm bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

NAMES = ("gdsp_fir_block", "gdsp_fir_batch", "gdsp_fir_batch_device")


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
    assert S["gdsp_fir_block"] == (I64, [I64, I64, ctypes.POINTER(I)])
    assert S["gdsp_fir_batch"] == (I, [P, I64, P, I64, I64, I64, I64, I, I64, P, I64])
    assert S["gdsp_fir_batch_device"] == (I, [P, I64, P, I64, I64, I64, I64, I, I64, P, I64, P, P])
    hdr = open(os.path.join(REPO, "include", "gdsp_fft.h")).read()
    assert "GDSP_ALGO_NO_FUSED_FIR = 512" in hdr


def _entries(gdsp):
    """Both entries behind one signature: (x, ldx, h, h_rows, m, channels, n,
    full, block, out, ldo) -> status."""
    L = gdsp._lib.lib()
    null = gdsp._lib._P()
    return (L.gdsp_fir_batch,
            lambda *a: L.gdsp_fir_batch_device(*a, null, null))


def test_status_codes_before_any_device_call(gdsp):
    G = gdsp._lib
    buf, obuf = np.zeros(4096), np.zeros(4096)
    p, o = buf.ctypes.data_as(G._P), obuf.ctypes.data_as(G._P)
    null = G._P()
    for f in _entries(gdsp):
        # negative sizes
        assert f(p, 8, p, 1, -1, 2, 8, 0, 0, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 1, 3, -1, 8, 0, 0, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 1, 3, 2, -1, 0, 0, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 1, 3, 2, 8, 0, -256, o, 8) == G.GDSP_ERR_INVALID
        # h_rows neither 1 nor channels
        assert f(p, 8, p, 2, 3, 3, 8, 0, 0, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 0, 3, 3, 8, 0, 0, o, 8) == G.GDSP_ERR_INVALID
        # row strides below the row lengths with more than one channel
        assert f(p, 7, p, 1, 3, 2, 8, 0, 0, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 1, 3, 2, 8, 0, 0, o, 7) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 1, 3, 2, 8, 1, 0, o, 9) == G.GDSP_ERR_INVALID  # out_len = 10
        # bad block: no power of 2, out of range, below 2 m
        for block in (300, 128, 1 << 21, 255):
            assert f(p, 8, p, 1, 3, 2, 8, 0, block, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 1, 129, 1, 8, 0, 256, o, 8) == G.GDSP_ERR_INVALID
        # full neither 0 nor 1
        assert f(p, 8, p, 1, 3, 2, 8, 2, 0, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 1, 3, 2, 8, -1, 0, o, 8) == G.GDSP_ERR_INVALID
        # a needed NULL pointer
        assert f(null, 8, p, 1, 3, 2, 8, 0, 0, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, null, 1, 3, 2, 8, 0, 0, o, 8) == G.GDSP_ERR_INVALID
        assert f(p, 8, p, 1, 3, 2, 8, 0, 0, null, 8) == G.GDSP_ERR_INVALID
        # nothing to do
        assert f(null, 0, null, 1, 3, 0, 8, 0, 0, null, 0) == G.GDSP_OK
        assert f(null, 0, null, 0, 0, 0, 0, 1, 0, null, 0) == G.GDSP_OK
        # empty input, as np.convolve refuses it
        assert f(p, 8, p, 1, 3, 2, 0, 0, 0, o, 8) == G.GDSP_ERR_EMPTY
        assert f(p, 8, p, 1, 0, 2, 8, 0, 0, o, 8) == G.GDSP_ERR_EMPTY
        assert f(p, 8, p, 1, 0, 1, 0, 1, 0, o, 8) == G.GDSP_ERR_EMPTY
        # taps beyond the composed form's range (before the pointers are looked at)
        assert f(p, 8, p, 1, (1 << 19) + 1, 1, 8, 0, 0, o, 8) == G.GDSP_ERR_UNSUPPORTED
        assert f(null, 8, null, 1, (1 << 19) + 1, 1, 8, 0, 0, null, 8) == G.GDSP_ERR_UNSUPPORTED


def test_device_entry_rejects_overlapping_ranges(gdsp):
    """The overlap rule is arithmetic on the two address ranges: fake pointers
    suffice, no device is touched."""
    G = gdsp._lib
    d = gdsp._lib.lib().gdsp_fir_batch_device
    null = G._P()
    base = 1 << 40
    h = G._P(1 << 30)

    def call(xa, oa, channels=2, n=100, ldx=128, ldo=128, m=5, full=0):
        return d(G._P(xa), ldx, h, 1, m, channels, n, full, 0, G._P(oa), ldo, null, null)

    assert call(base, base) == G.GDSP_ERR_INVALID                    # in place
    assert call(base, base + 8 * 50) == G.GDSP_ERR_INVALID           # out starts inside x
    assert call(base + 8 * 50, base) == G.GDSP_ERR_INVALID           # x starts inside out
    # x spans (channels - 1) ldx + n = 228 doubles: the last one still collides
    assert call(base, base + 8 * 227) == G.GDSP_ERR_INVALID
    assert call(base + 8 * 227, base) == G.GDSP_ERR_INVALID
    # full: out spans 128 + 104 = 232 doubles
    assert call(base + 8 * 231, base, full=1) == G.GDSP_ERR_INVALID
    # one channel: the strides do not count, the rows' own lengths do
    assert call(base, base + 8 * 99, channels=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID


GRID = sorted(set([1, 2, 128, 129, 8192] + list(range(3, 8192, 97)) +
                  [(1 << k) + d for k in range(1, 13) for d in (-1, 0, 1)]))


def test_fir_block_is_deterministic_and_in_range(gdsp):
    F = gdsp.fft
    assert GRID[0] == 1 and GRID[-1] == 8192
    for m in GRID:
        f, fused = F.fir_block(m)
        assert 256 <= f <= 16384 and f & (f - 1) == 0, (m, f)
        assert f >= 2 * m and fused, (m, f, fused)
        assert F.fir_block(m) == (f, fused)
        assert F.fir_block(m, 0) == (f, fused)


def test_fir_block_beyond_the_fused_range(gdsp):
    F = gdsp.fft
    assert F.fir_block(8193) == (32768, False)
    assert F.fir_block((1 << 19) + 1) == (0, False)
    assert F.fir_block(0) == (0, False)
    assert F.fir_block(-3) == (0, False)
    # NULL for the fused answer
    L = gdsp._lib.lib()
    assert L.gdsp_fir_block(8193, 0, None) == 32768
    assert L.gdsp_fir_block(31, 0, None) == F.fir_block(31)[0]


def test_fir_block_forced(gdsp):
    F = gdsp.fft
    for block in (256, 512, 4096, 16384):
        assert F.fir_block(5, block) == (block, True)
    for block in (32768, 1 << 20):
        assert F.fir_block(5, block) == (block, False)
    assert F.fir_block(128, 256) == (256, True)
    assert F.fir_block(8192, 16384) == (16384, True)
    assert F.fir_block(100, 32768) == (32768, False)
    assert F.fir_block(1 << 19, 1 << 20) == (1 << 20, False)
    # no power of 2, out of range, below 2 m
    for m, block in ((5, 300), (5, 128), (5, 1 << 21), (5, 255), (129, 256), (8193, 16384),
                     ((1 << 19) + 1, 1 << 20), (5, -256)):
        assert F.fir_block(m, block) == (0, False), (m, block)


def test_flag_clears_fused_and_keeps_the_block(gdsp):
    F = gdsp.fft
    prev = F.Algorithm()
    want = {m: F.fir_block(m)[0] for m in (1, 31, 255, 2047, 8192)}
    try:
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_FIR)
        for m, f in want.items():
            assert F.fir_block(m) == (f, False)
        assert F.fir_block(65, 4096) == (4096, False)
    finally:
        F.SetAlgorithm(prev)
    assert F.fir_block(65, 4096) == (4096, True)


def test_no_fused_fir_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_FIR == 512 == gdsp._lib.GDSP_ALGO_NO_FUSED_FIR
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_FIR)
        assert F.Algorithm() == F.ALGO_NO_FUSED_FIR
        F.SetAlgorithm(F.ALGO_NO_FUSED_FIR | F.ALGO_NO_FUSED_CONVOLVE | F.ALGO_NO_RACE)
        assert F.Algorithm() == F.ALGO_NO_FUSED_FIR | F.ALGO_NO_FUSED_CONVOLVE | F.ALGO_NO_RACE
        with pytest.raises(gdsp.GDSPError) as e:
            F.SetAlgorithm(1 << 20)
        assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == F.ALGO_NO_FUSED_FIR | F.ALGO_NO_FUSED_CONVOLVE | F.ALGO_NO_RACE
    finally:
        F.SetAlgorithm(prev)


def test_python_mirrors_panic_and_refuse(gdsp):
    F = gdsp.fft
    with pytest.raises(gdsp.Panic, match="ragged input array"):
        F.FIRFilterBatch([np.zeros(8), np.zeros(7)], np.ones(3))
    x = np.zeros((3, 8))
    for h in (np.zeros((2, 3)), np.zeros((4, 3)), np.zeros((3, 3, 1)), np.zeros(())):
        with pytest.raises(gdsp.Panic, match="arrays not of equal size"):
            F.FIRFilterBatch(x, h)
    # complex input is refused, never cast
    with pytest.raises(TypeError):
        F.FIRFilterBatch(x.astype(np.complex128), np.ones(3))
    with pytest.raises(TypeError):
        F.FIRFilterBatch(x, np.ones(3, np.complex128))
    with pytest.raises(TypeError):
        F.FIRFilterBatch([np.zeros(8), np.zeros(8, np.complex64)], np.ones(3))
    with pytest.raises(TypeError):
        F.FIRFilter(np.zeros(8, np.complex128), np.ones(3))
    with pytest.raises(TypeError):
        F.FIRFilter(np.zeros(8), 1j * np.ones(3))
    with pytest.raises(TypeError):
        F.ConvolveLinear(np.zeros(8, np.complex128), np.ones(3))
    # an empty batch asks nothing of the device
    assert F.FIRFilterBatch(np.zeros((0, 8)), np.ones(3)).shape == (0, 8)
    assert F.FIRFilterBatch(np.zeros((0, 8)), np.ones(3), full=True).shape == (0, 10)
    assert F.FIRFilterBatch(np.zeros((0, 8)), np.zeros((0, 3)), full=True).shape == (0, 10)
