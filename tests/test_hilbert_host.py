"""CPU-only checks of the Hilbert boundary (gdsp_hilbert_batch,
gdsp_hilbert_batch_device, gdsp_hilbert_fused): the entry points are declared,
exported and bound alike; GDSP_ALGO_NO_FUSED_HILBERT is the known bit 32768
while 2048, 16384 and 1 << 20 stay unknown; every status code of the header's
table answers in its order before any device call, through both entries, with
pointers that would fault if touched; the fused query is host arithmetic; and
the reference the GPU tests compare with (hilbert_ref.py) agrees with scipy and
with itself across its two routes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import exact_dft as E
import hilbert_ref as H
from conftest import REPO

NAMES = ("gdsp_hilbert_batch", "gdsp_hilbert_batch_device", "gdsp_hilbert_fused")


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
    # (x, ldx, rows, n, nfft, kind, out, ldo[, work, stream])
    assert S["gdsp_hilbert_batch"] == (I, [P, I64, I64, I64, I64, I, P, I64])
    assert S["gdsp_hilbert_batch_device"] == (I, [P, I64, I64, I64, I64, I, P, I64, P, P])
    assert S["gdsp_hilbert_fused"] == (I, [I64])
    hdr = open(os.path.join(REPO, "include", "gdsp_fft.h")).read()
    assert "GDSP_ALGO_NO_FUSED_HILBERT = 32768" in hdr
    assert "16384" in hdr.split("GDSP_ALGO_NO_FUSED_HILBERT = 32768")[0].rsplit("/*", 1)[1]
    for name, v in (("ANALYTIC", 0), ("QUADRATURE", 1), ("ENVELOPE", 2)):
        assert "GDSP_HILBERT_%s = %d" % (name, v) in hdr
        assert getattr(gdsp._lib, "GDSP_HILBERT_" + name) == v
    assert "Hilbert" in hdr.split("---- values")[1].split("---- fft package")[0]
    assert "gdsp_hilbert_batch" in hdr.split("later_chunks:")[1].split("gdsp_loop_stats(")[0]


def test_no_fused_hilbert_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_HILBERT == 32768
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_HILBERT)
        assert F.Algorithm() == 32768
        F.SetAlgorithm(F.ALGO_NO_FUSED_HILBERT | F.ALGO_NO_FUSED_UPFIRDN | F.ALGO_NO_FUSED_FIR)
        assert F.Algorithm() == 32768 | 8192 | 512
        for bad in (2048, 16384, 32768 | 16384, 32768 | 2048, 1 << 20):
            with pytest.raises(gdsp.GDSPError) as e:
                F.SetAlgorithm(bad)
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == 32768 | 8192 | 512
    finally:
        F.SetAlgorithm(prev)


def test_fused_query_is_host_arithmetic(gdsp):
    F = gdsp.fft
    prev = F.Algorithm()
    fused = [1 << k for k in range(8, 15)]
    try:
        F.SetAlgorithm(prev & ~F.ALGO_NO_FUSED_HILBERT)
        for n in fused:
            assert F.hilbert_fused(n) is True, n
        for n in (0, 1, 2, 128, 255, 257, 3000, 4095, 16383, 32768, 1 << 20, -256):
            assert F.hilbert_fused(n) is False, n
        # exactly those seven below 2^16
        assert [n for n in range(1, 1 << 16) if F.hilbert_fused(n)] == fused
        # other flags do not matter; this one turns every length off
        F.SetAlgorithm(F.ALGO_NO_FUSED_FIR | F.ALGO_NO_FUSED_CONVOLVE | F.ALGO_NO_FUSED_STFT)
        assert all(F.hilbert_fused(n) for n in fused)
        F.SetAlgorithm(F.ALGO_NO_FUSED_HILBERT)
        for n in fused + [128, 255, 3000, 32768]:
            assert F.hilbert_fused(n) is False, n
    finally:
        F.SetAlgorithm(prev)


def _entries(gdsp):
    """Both entries behind one signature: (x, ldx, rows, n, nfft, kind, out,
    ldo) -> status."""
    L = gdsp._lib.lib()
    null = gdsp._lib._P()
    return (L.gdsp_hilbert_batch, lambda *a: L.gdsp_hilbert_batch_device(*a, null, null))


def test_status_codes_in_order_before_any_device_call(gdsp):
    G = gdsp._lib
    null = G._P()
    # far apart, unmapped: a call that touched either would fault
    px, po = G._P(1 << 44), G._P(1 << 45)
    for f in _entries(gdsp):
        def call(x=px, ldx=300, rows=3, n=300, nfft=256, kind=0, out=po, ldo=256):
            return f(x, ldx, rows, n, nfft, kind, out, ldo)

        # 1. negative sizes, the kind, the strides
        assert call(rows=-1) == G.GDSP_ERR_INVALID
        assert call(n=-1) == G.GDSP_ERR_INVALID
        assert call(nfft=-1) == G.GDSP_ERR_INVALID
        assert call(kind=-1) == G.GDSP_ERR_INVALID
        assert call(kind=3) == G.GDSP_ERR_INVALID
        assert call(ldx=299) == G.GDSP_ERR_INVALID
        assert call(ldo=255) == G.GDSP_ERR_INVALID
        assert call(nfft=0, ldo=299) == G.GDSP_ERR_INVALID       # N = n
        assert call(nfft=512, ldo=511) == G.GDSP_ERR_INVALID
        # ... all before the later ones: no rows, no samples, no pointers
        assert call(rows=0, kind=3) == G.GDSP_ERR_INVALID
        assert call(rows=0, n=-1) == G.GDSP_ERR_INVALID
        assert call(n=0, ldx=0, kind=7) == G.GDSP_ERR_INVALID
        assert call(x=null, out=null, ldx=1) == G.GDSP_ERR_INVALID
        assert call(x=null, n=0, nfft=0, ldx=-1, ldo=0) == G.GDSP_ERR_INVALID  # ldx < n
        # 2. no rows: nothing is looked at
        assert call(x=null, out=null, rows=0) == G.GDSP_OK
        assert call(x=null, out=null, rows=0, n=0, nfft=0, ldx=0, ldo=0) == G.GDSP_OK
        # 3. empty input, before the pointers are looked at
        assert call(n=0, ldx=0) == G.GDSP_ERR_EMPTY
        assert call(n=0, nfft=0, ldx=0, ldo=0) == G.GDSP_ERR_EMPTY
        assert call(x=null, out=null, n=0, ldx=0) == G.GDSP_ERR_EMPTY
        assert call(x=null, rows=1, n=0, nfft=0, ldx=0, ldo=0) == G.GDSP_ERR_EMPTY
        # 4. a NULL pointer; one row needs no stride
        assert call(x=null) == G.GDSP_ERR_INVALID
        assert call(out=null) == G.GDSP_ERR_INVALID
        assert call(x=null, rows=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID
        for kind in (0, 1, 2):
            assert call(out=null, kind=kind, nfft=1000, ldo=1000) == G.GDSP_ERR_INVALID
        if gdsp.device_count() == 0:
            assert call() == G.GDSP_ERR_NO_DEVICE
            assert call(rows=1, ldx=0, ldo=0, kind=2) == G.GDSP_ERR_NO_DEVICE
            assert call(nfft=1000, ldo=1000, kind=1) == G.GDSP_ERR_NO_DEVICE


def test_device_entry_rejects_overlapping_ranges(gdsp):
    """The overlap rule is arithmetic on the two address ranges, after every
    other check: fake pointers suffice, no device is touched."""
    G = gdsp._lib
    d = G.lib().gdsp_hilbert_batch_device
    null = G._P()
    base = 1 << 44

    # 2 rows of 100 at stride 128 into N = 64 at stride 80
    def call(xa, oa, kind=1, rows=2, n=100, nfft=64, ldx=128, ldo=80):
        return d(G._P(xa), ldx, rows, n, nfft, kind, G._P(oa), ldo, null, null)

    assert call(base, base) == G.GDSP_ERR_INVALID                    # in place
    assert call(base, base + 8 * 50) == G.GDSP_ERR_INVALID           # out starts inside x
    assert call(base + 8 * 50, base) == G.GDSP_ERR_INVALID           # x starts inside out
    assert call(base, base + 8 * 227) == G.GDSP_ERR_INVALID          # x spans 228 doubles
    assert call(base + 8 * 143, base) == G.GDSP_ERR_INVALID          # out spans 144 doubles
    assert call(base + 8 * 287, base, kind=0) == G.GDSP_ERR_INVALID  # ... 144 complex128
    assert call(base, base + 8 * 99, rows=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID
    # the earlier checks come first
    assert call(base, base, kind=5) == G.GDSP_ERR_INVALID
    assert call(base, base, rows=0) == G.GDSP_OK
    assert call(base, base, n=0, ldx=0) == G.GDSP_ERR_EMPTY
    if gdsp.device_count() == 0:  # apart: the call goes on to the device
        assert call(base, base + 8 * 228) == G.GDSP_ERR_NO_DEVICE
        assert call(base + 8 * 144, base) == G.GDSP_ERR_NO_DEVICE
        assert call(base + 8 * 288, base, kind=0) == G.GDSP_ERR_NO_DEVICE


def test_python_wrappers_refuse_what_the_library_would(gdsp):
    F = gdsp.fft
    with pytest.raises(TypeError):
        F.Hilbert(np.ones(8, np.complex128))
    with pytest.raises(TypeError):
        F.EnvelopeBatch(np.ones((2, 8), np.complex128))
    with pytest.raises(gdsp.Panic):
        F.HilbertBatch([np.ones(4), np.ones(5)])
    with pytest.raises(gdsp.GDSPError) as e:
        F.Envelope(np.zeros(0))
    assert e.value.status == gdsp._lib.GDSP_ERR_EMPTY
    assert F.HilbertBatch(np.zeros((0, 16))).shape == (0, 16)
    assert F.EnvelopeBatch(np.zeros((0, 16)), 32).dtype == np.float64


# ---- the reference ---------------------------------------------------------------

def test_reference_agrees_with_scipy():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(7)
    for n, N in ((255, None), (256, None), (1000, None), (200, 256), (300, 256), (1, None)):
        x = rng.uniform(-1, 1, (3, n))
        want = signal.hilbert(x, N, axis=1)
        got = H.analytic64(x, N)
        assert got.shape == want.shape
        assert np.array_equal(got.real, H.padded(x, N))
        assert np.max(np.abs(got - want)) <= 1e-13 * max(1.0, np.max(np.abs(want)))


def test_reference_routes_agree_at_roundoff():
    """The float64 route against the 80-bit one on the standard rows: a few u,
    the level the GPU bound is relative to; a tone's quadrature is its sine."""
    for N in (255, 256, 1000):
        x = E.input_rows(N, real=True)
        e = E.err_u(H.quadrature64(x), H.quadrature_exact(x))
        print("hilbert_ref N=%d float64 route %.3g u" % (N, e))
        assert 0 < e < 64
    # a tone on a bin: its sine. The float64 samples carry u / 2 of rounding each,
    # and the transform's infinity norm is below (2 / pi) (ln N + 2) = 5.3 at 512
    ang = 2 * E.PI * ((9 * np.arange(512, dtype=np.int64)) % 512).astype(E.LD) / 512
    q = H.quadrature_exact(np.cos(ang).astype(np.float64))[0]
    d = float(np.max(np.abs(q - np.sin(ang))) / E.U)
    print("hilbert_ref tone: %.3g u" % d)
    assert d < 0.5 * 5.3 + 0.1
    assert np.all(H.quadrature64(np.ones((1, 1)))[0] == 0.0)   # N = 1: h = 0
    assert H.multiplier(6).tolist() == [0, -1j, -1j, 0, 1j, 1j]
    assert H.multiplier(5).tolist() == [0, -1j, -1j, 1j, 1j]
