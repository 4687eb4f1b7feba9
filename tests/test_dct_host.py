"""CPU-only checks of the DCT boundary (gdsp_dct_batch, gdsp_dct_batch_device,
gdsp_dct_fused, gdsp_dct_work_doubles, gdsp_dct_twiddles): the entry points are
declared, exported and bound alike; GDSP_ALGO_NO_FUSED_DCT is the known bit
1 << 21 while 2048, 16384, 131072, 1 << 19 and 1 << 20 stay unknown; every
status code of the header's table answers in its order before any device call,
through both entries, with pointers that would fault if touched; the fused
query, the work size and the w_k table are host arithmetic; the Python wrappers
refuse bad arguments; and the reference the GPU tests compare with (dct_ref.py)
agrees with itself across its routes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dct_ref as R
import exact_dft as E
from conftest import REPO

NAMES = ("gdsp_dct_batch", "gdsp_dct_batch_device", "gdsp_dct_fused", "gdsp_dct_work_doubles",
         "gdsp_dct_twiddles")
FLAG = 1 << 21


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
    # (x, ldx, rows, n, nfft, type, norm, out, ldo[, work, stream])
    assert S["gdsp_dct_batch"] == (I, [P, I64, I64, I64, I64, I, I, P, I64])
    assert S["gdsp_dct_batch_device"] == (I, [P, I64, I64, I64, I64, I, I, P, I64, P, P])
    assert S["gdsp_dct_fused"] == (I, [I64])
    assert S["gdsp_dct_work_doubles"] == (I64, [I64, I64])
    assert S["gdsp_dct_twiddles"] == (I, [I64, P])
    hdr = open(os.path.join(REPO, "include", "gdsp_fft.h")).read()
    assert "GDSP_ALGO_NO_FUSED_DCT = 2097152" in hdr
    note = hdr.split("GDSP_ALGO_NO_FUSED_DCT = 2097152")[0].rsplit("/*", 1)[1]
    assert "1 << 19" in note and "1 << 20" in note  # the bits it could not take
    for name, v in (("BACKWARD", 0), ("ORTHO", 1), ("FORWARD", 2)):
        assert "GDSP_DCT_%s = %d" % (name, v) in hdr
        assert getattr(gdsp._lib, "GDSP_DCT_" + name) == v
    assert "DCT" in hdr.split("---- values")[1].split("---- fft package")[0]
    assert "gdsp_dct_batch" in hdr.split("later_chunks:")[1].split("gdsp_loop_stats(")[0]


def test_no_fused_dct_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_DCT == FLAG == 2097152
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_DCT)
        assert F.Algorithm() == FLAG
        F.SetAlgorithm(F.ALGO_NO_FUSED_DCT | F.ALGO_NO_FUSED_HILBERT | F.ALGO_NO_FUSED_CZT)
        assert F.Algorithm() == FLAG | 32768 | 262144
        for bad in (2048, 16384, 131072, 1 << 19, 1 << 20, 1 << 22, FLAG | 2048, FLAG | (1 << 20)):
            with pytest.raises(gdsp.GDSPError) as e:
                F.SetAlgorithm(bad)
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == FLAG | 32768 | 262144
    finally:
        F.SetAlgorithm(prev)


def test_fused_query_is_host_arithmetic(gdsp):
    F = gdsp.fft
    prev = F.Algorithm()
    fused = [1 << k for k in range(8, 15)]
    try:
        F.SetAlgorithm(prev & ~F.ALGO_NO_FUSED_DCT)
        for n, want in ((0, False), (1, False), (128, False), (255, False), (256, True),
                        (257, False), (3000, False), (16384, True), (32768, False),
                        (1 << 20, False), (-256, False)):
            assert F.dct_fused(n) is want, n
        assert [n for n in range(1, 1 << 16) if F.dct_fused(n)] == fused
        # other flags do not matter; this one turns every length off
        F.SetAlgorithm(F.ALGO_NO_FUSED_HILBERT | F.ALGO_NO_FUSED_CONVOLVE | F.ALGO_NO_FUSED_CZT)
        assert all(F.dct_fused(n) for n in fused)
        F.SetAlgorithm(F.ALGO_NO_FUSED_DCT)
        for n in fused + [128, 255, 3000, 32768]:
            assert F.dct_fused(n) is False, n
    finally:
        F.SetAlgorithm(prev)


def test_work_doubles_follow_the_documented_formula(gdsp):
    F = gdsp.fft
    w = gdsp._lib.lib().gdsp_dct_work_doubles

    def formula(rows, N, fused):
        if rows <= 0 or N <= 1 or N > 1 << 20 or fused:
            return 0
        return 3 * min(rows, max(1, (1 << 24) // N)) * N

    prev = F.Algorithm()
    try:
        for flags in (prev & ~F.ALGO_NO_FUSED_DCT, prev | F.ALGO_NO_FUSED_DCT):
            F.SetAlgorithm(flags)
            for N in (-4, 0, 1, 2, 255, 256, 1000, 3001, 4096, 16384, 32768, 1 << 20,
                      (1 << 20) + 1):
                for rows in (-1, 0, 1, 5, 511, 512, 513, 70000, 1 << 25):
                    assert w(rows, N) == formula(rows, N, F.dct_fused(N)), (rows, N, flags)
        F.SetAlgorithm(prev & ~F.ALGO_NO_FUSED_DCT)
        assert w(7, 4096) == 0 and w(7, 1000) == 21000 and w(1 << 25, 1 << 20) == 3 * 16 << 20
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_DCT)
        assert w(7, 4096) == 3 * 7 * 4096
    finally:
        F.SetAlgorithm(prev)


@pytest.mark.parametrize("N", [1, 2, 256, 3001, 16384])
def test_twiddle_table_is_within_one_u_of_long_double(gdsp, N):
    """Each component against the 80-bit cosine and sine of pi k / (2N), relative
    to the component itself: the table is the long-double value rounded once
    (0.5 u), the 80-bit evaluation adds 2^-11 u."""
    G = gdsp._lib
    t = np.full(2 * N + 2, 7.0)
    assert G.lib().gdsp_dct_twiddles(N, t.ctypes.data_as(G._P)) == G.GDSP_OK
    assert np.all(t[2 * N:] == 7.0)
    c, s = R.twiddles_exact(N)
    for got, want in ((t[0:2 * N:2], c), (t[1:2 * N:2], -s)):
        nz = want != 0
        assert np.all(got[~nz] == 0)
        rel = float(np.max(np.abs(got[nz].astype(E.LD) - want[nz]) / np.abs(want[nz])) / E.U) \
            if nz.any() else 0.0
        print("dct twiddles N=%d: %.3g u" % (N, rel))
        assert rel <= 1.0
    assert t[0] == 1.0 and t[1] == 0.0
    # the same angles without the complement: equal to 1 u of the unit circle
    k = np.arange(N).astype(E.LD)
    a = k * (E.PI / E.LD(2 * N))
    assert np.max(np.abs(t[0:2 * N:2] - np.cos(a))) <= E.U and \
        np.max(np.abs(t[1:2 * N:2] + np.sin(a))) <= E.U


def test_twiddle_status_codes(gdsp):
    G = gdsp._lib
    f = G.lib().gdsp_dct_twiddles
    buf = np.zeros(8)
    p = buf.ctypes.data_as(G._P)
    assert f(-1, p) == G.GDSP_ERR_INVALID
    assert f(0, p) == G.GDSP_ERR_EMPTY
    assert f(4, G._P()) == G.GDSP_ERR_INVALID
    assert f((1 << 20) + 1, p) == G.GDSP_ERR_UNSUPPORTED
    assert f(4, p) == G.GDSP_OK


def _entries(gdsp):
    """Both entries behind one signature: (x, ldx, rows, n, nfft, type, norm,
    out, ldo) -> status."""
    L = gdsp._lib.lib()
    null = gdsp._lib._P()
    return (L.gdsp_dct_batch, lambda *a: L.gdsp_dct_batch_device(*a, null, null))


def test_status_codes_in_order_before_any_device_call(gdsp):
    G = gdsp._lib
    null = G._P()
    # far apart, unmapped: a call that touched either would fault
    px, po = G._P(1 << 44), G._P(1 << 45)
    big = (1 << 20) + 1
    for f in _entries(gdsp):
        def call(x=px, ldx=300, rows=3, n=300, nfft=256, type=2, norm=0, out=po, ldo=256):
            return f(x, ldx, rows, n, nfft, type, norm, out, ldo)

        # 1. negative sizes, the type, the norm, the strides
        assert call(rows=-1) == G.GDSP_ERR_INVALID
        assert call(n=-1) == G.GDSP_ERR_INVALID
        assert call(nfft=-1) == G.GDSP_ERR_INVALID
        for t in (-1, 0, 1, 4):
            assert call(type=t) == G.GDSP_ERR_INVALID
        assert call(norm=-1) == G.GDSP_ERR_INVALID
        assert call(norm=3) == G.GDSP_ERR_INVALID
        assert call(ldx=255) == G.GDSP_ERR_INVALID               # min(n, N) = 256
        assert call(ldo=255) == G.GDSP_ERR_INVALID
        assert call(nfft=0, ldo=299) == G.GDSP_ERR_INVALID       # N = n
        assert call(nfft=512, ldx=299) == G.GDSP_ERR_INVALID     # min(n, N) = 300
        assert call(nfft=512, ldo=511) == G.GDSP_ERR_INVALID
        # ... all before the later ones: no rows, no samples, no pointers, too long
        assert call(rows=0, type=4) == G.GDSP_ERR_INVALID
        assert call(rows=0, norm=3) == G.GDSP_ERR_INVALID
        assert call(rows=0, n=-1) == G.GDSP_ERR_INVALID
        assert call(n=0, ldx=0, type=7) == G.GDSP_ERR_INVALID
        assert call(x=null, out=null, ldo=1) == G.GDSP_ERR_INVALID
        assert call(nfft=big, ldo=big, norm=5) == G.GDSP_ERR_INVALID
        assert call(nfft=big, ldo=big - 1) == G.GDSP_ERR_INVALID
        # 2. no rows: nothing is looked at
        assert call(x=null, out=null, rows=0) == G.GDSP_OK
        assert call(x=null, out=null, rows=0, n=0, nfft=0, ldx=0, ldo=0) == G.GDSP_OK
        assert call(rows=0, nfft=big, ldo=big) == G.GDSP_OK
        # 3. empty input, before the pointers are looked at
        assert call(n=0, ldx=0) == G.GDSP_ERR_EMPTY
        assert call(n=0, nfft=0, ldx=0, ldo=0) == G.GDSP_ERR_EMPTY
        assert call(x=null, out=null, n=0, ldx=0) == G.GDSP_ERR_EMPTY
        assert call(x=null, rows=1, n=0, nfft=0, ldx=0, ldo=0) == G.GDSP_ERR_EMPTY
        assert call(n=0, ldx=0, nfft=big, ldo=big) == G.GDSP_ERR_EMPTY
        # 4. a NULL pointer, before the length limit; one row needs no stride
        assert call(x=null) == G.GDSP_ERR_INVALID
        assert call(out=null) == G.GDSP_ERR_INVALID
        assert call(x=null, rows=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID
        assert call(out=null, nfft=big, ldo=big) == G.GDSP_ERR_INVALID
        for t in (2, 3):
            for norm in (0, 1, 2):
                assert call(out=null, type=t, norm=norm, nfft=1000, ldo=1000) == G.GDSP_ERR_INVALID
        # 5. too long a transform
        assert call(nfft=big, ldo=big) == G.GDSP_ERR_UNSUPPORTED
        assert call(n=big, ldx=big, nfft=0, ldo=big) == G.GDSP_ERR_UNSUPPORTED
        assert call(rows=1, nfft=1 << 21, ldx=0, ldo=0, type=3, norm=1) == G.GDSP_ERR_UNSUPPORTED
        if gdsp.device_count() == 0:
            assert call() == G.GDSP_ERR_NO_DEVICE
            assert call(rows=1, ldx=0, ldo=0, type=3) == G.GDSP_ERR_NO_DEVICE
            assert call(nfft=1 << 20, ldo=1 << 20, norm=2) == G.GDSP_ERR_NO_DEVICE


def test_device_entry_allows_exactly_in_place_and_no_other_overlap(gdsp):
    """The overlap rule is arithmetic on the two address ranges, after every
    other check: fake pointers suffice, no device is touched."""
    G = gdsp._lib
    d = G.lib().gdsp_dct_batch_device
    null = G._P()
    base = 1 << 44
    nodev = gdsp.device_count() == 0

    # 2 rows of 100 at stride 128 into N = 64 at stride 80
    def call(xa, oa, rows=2, n=100, nfft=64, ldx=128, ldo=80, type=2):
        return d(G._P(xa), ldx, rows, n, nfft, type, 0, G._P(oa), ldo, null, null)

    assert call(base, base) == G.GDSP_ERR_INVALID                    # same pointer, other stride
    assert call(base, base, nfft=128, ldo=128) == G.GDSP_ERR_INVALID  # same stride, N > n
    assert call(base, base + 8 * 50) == G.GDSP_ERR_INVALID           # out starts inside x
    assert call(base + 8 * 50, base) == G.GDSP_ERR_INVALID           # x starts inside out
    assert call(base, base + 8 * 191) == G.GDSP_ERR_INVALID          # x reads 128 + 64 doubles
    assert call(base + 8 * 143, base) == G.GDSP_ERR_INVALID          # out spans 144 doubles
    assert call(base, base + 8, ldo=128) == G.GDSP_ERR_INVALID       # shifted by one sample
    assert call(base, base + 8 * 63, rows=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID
    # the earlier checks come first
    assert call(base, base, type=5) == G.GDSP_ERR_INVALID
    assert call(base, base, rows=0) == G.GDSP_OK
    assert call(base, base, n=0, ldx=0) == G.GDSP_ERR_EMPTY
    if nodev:  # exactly in place, or apart: the call goes on to the device
        assert call(base, base, ldo=128) == G.GDSP_ERR_NO_DEVICE
        assert call(base, base, ldo=128, nfft=100, type=3) == G.GDSP_ERR_NO_DEVICE
        assert call(base, base, rows=1, ldx=0, ldo=0) == G.GDSP_ERR_NO_DEVICE
        assert call(base, base + 8 * 192) == G.GDSP_ERR_NO_DEVICE
        assert call(base + 8 * 144, base) == G.GDSP_ERR_NO_DEVICE


def test_python_wrappers_refuse_what_the_library_would(gdsp):
    F = gdsp.fft
    x = np.ones(8)
    for fn in (F.DCT, F.IDCT):
        for t in (1, 4, 0, "2", None, True):
            with pytest.raises(ValueError):
                fn(x, type=t)
        for norm in ("orth", "Ortho", 1, b"ortho"):
            with pytest.raises(ValueError):
                fn(x, norm=norm)
        with pytest.raises(TypeError):
            fn(np.ones(8, np.complex128))
        for bad in (0, -1, -256):
            with pytest.raises(ValueError):
                fn(x, n=bad)
    for fn in (F.DCTBatch, F.IDCTBatch):
        with pytest.raises(ValueError):
            fn(np.ones((2, 8)), type=1)
        with pytest.raises(ValueError):
            fn(np.ones((2, 8)), norm="none")
        with pytest.raises(TypeError):
            fn(np.ones((2, 8), np.complex128))
        with pytest.raises(gdsp.Panic):
            fn([np.ones(4), np.ones(5)])
        assert fn(np.zeros((0, 16))).shape == (0, 16)
        assert fn(np.zeros((0, 16)), n=32, norm="ortho").dtype == np.float64
        # n below 1 is scipy's ValueError, for one row too (the C ABI reads nfft = 0
        # as "the row length", which an output of no columns would not hold)
        for rows in (1, 2):
            for bad in (0, -1, 1.5, True):
                with pytest.raises(ValueError):
                    fn(np.ones((rows, 8)), n=bad)
        with pytest.raises(gdsp.GDSPError) as e:
            fn(np.ones((1, 8)), n=(1 << 20) + 1)
        assert e.value.status == gdsp._lib.GDSP_ERR_UNSUPPORTED
    with pytest.raises(gdsp.GDSPError) as e:
        F.DCT(np.zeros(0))
    assert e.value.status == gdsp._lib.GDSP_ERR_EMPTY
    assert F.dct_length(None) is None and F.dct_length(8) == 8 and F.dct_length(np.int64(3)) == 3
    # the inverse is the other type under the opposite norm
    assert F.dct_kind(2, None) == (2, 0) and F.dct_kind(3, "forward") == (3, 2)
    assert F.dct_kind(2, None, True) == (3, 2) and F.dct_kind(2, "forward", True) == (3, 0)
    assert F.dct_kind(3, "ortho", True) == (2, 1) and F.dct_kind(3, "backward", True) == (2, 2)


# ---- the reference ---------------------------------------------------------------

def _direct(p, type):
    """The definition's sums in long double (small N)."""
    N = p.shape[1]
    j = np.arange(N, dtype=np.int64)
    ang = ((np.outer(j, 2 * j + 1)) % (4 * N)).astype(E.LD) * (E.PI / E.LD(2 * N))
    C = np.cos(ang)  # C[k, j] = cos(pi k (2j+1) / (2N))
    p = p.astype(E.LD)
    if type == 2:
        return 2 * p @ C.T
    return p[:, :1] + 2 * p[:, 1:] @ C[1:, :]


@pytest.mark.parametrize("N", [1, 2, 3, 8, 255, 256])
def test_exact_route_is_the_definition(N):
    x = np.random.default_rng(N).uniform(-1, 1, (3, N))
    n2 = E.LD(2 * N)
    for type in (2, 3):
        want = _direct(x, type)
        top = float(np.max(np.abs(want)))
        got = R.dct_exact(x, type)
        assert float(np.max(np.abs(got - want))) <= 2.0 ** -58 * top, (N, type)
        assert float(np.max(np.abs(R.dct_exact(x, type, norm="forward") - want / n2))) \
            <= 2.0 ** -58 * top / (2 * N)
    o2 = _direct(x, 2) * np.sqrt(1 / n2)
    o2[:, 0] /= np.sqrt(E.LD(2))
    assert float(np.max(np.abs(R.dct_exact(x, 2, norm="ortho") - o2))) <= 2.0 ** -58 * N
    xs = x.astype(E.LD)
    xs[:, 0] *= np.sqrt(E.LD(2))
    o3 = _direct(xs, 3) * np.sqrt(1 / n2)
    assert float(np.max(np.abs(R.dct_exact(x, 3, norm="ortho") - o3))) <= 2.0 ** -58 * N


@pytest.mark.parametrize("N", [1, 2, 3, 8, 255, 256, 1000, 3001, 4096])
def test_reference_routes_agree_at_roundoff(N):
    """The float64 route against the 80-bit one on the standard rows: a few u,
    the level the GPU bound is relative to; the inverse undoes the transform;
    cut and padded rows are the padded row's."""
    x = E.input_rows(N, real=True)
    for type in (2, 3):
        for norm in R.NORMS:
            ex = R.dct_exact(x, type, norm=norm)
            e = E.err_u(R.dct64(x, type, norm=norm), ex)
            print("dct_ref N=%d type %d %s: float64 route %.3g u" % (N, type, norm, e))
            assert e < 64
            back = R.idct_exact(ex, type, norm=norm)
            # 80-bit roundoff is 2^-10 u; two transforms of 4N points keep it below 2^-4 u
            assert E.err_u(back, x.astype(E.LD)) < 2.0 ** -4
            assert E.err_u(R.idct64(R.dct64(x, type, norm=norm), type, norm=norm),
                           x.astype(E.LD)) < 256
    if N >= 8:
        y = np.random.default_rng(N).uniform(-1, 1, (2, N))
        cut = R.dct_exact(y, 2, N - 3)
        assert np.array_equal(cut, R.dct_exact(y[:, :N - 3], 2))
        assert np.array_equal(R.dct_exact(y[:, :N - 3], 3, N),
                              R.dct_exact(np.pad(y[:, :N - 3], ((0, 0), (0, 3))), 3))


def test_makhoul_statement_agrees_with_the_exact_route():
    """The fallback of the float64 route (and the statement the kernels
    implement), odd lengths included."""
    for N in (1, 2, 3, 8, 255, 256, 1000, 3001):
        x = E.input_rows(N, real=True)
        for type in (2, 3):
            for norm in R.NORMS:
                e = E.err_u(R._makhoul64(R.padded(x), type, R._norm(norm)),
                            R.dct_exact(x, type, norm=norm))
                assert e < 64, (N, type, norm, e)
