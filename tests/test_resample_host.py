"""CPU-only checks of the resampling boundary (gdsp_upfirdn_length,
gdsp_upfirdn_fused, gdsp_upfirdn_batch, gdsp_upfirdn_batch_device): the entry
points are declared, exported and bound alike; GDSP_ALGO_NO_FUSED_UPFIRDN is the
known bit 8192; every status code of the header's table answers before any
device call, through both entries; the length and the fused query are host
arithmetic; resample_taps is the written formula (and scipy's firwin);
ResamplePoly's pre / rem / post arithmetic is scipy's; and the reference the
GPU tests compare with (resample_ref.py) gives the same sums in both its forms."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import resample_ref as R
from conftest import REPO, row_nrel

NAMES = ("gdsp_upfirdn_length", "gdsp_upfirdn_fused", "gdsp_upfirdn_batch",
         "gdsp_upfirdn_batch_device")


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
    assert S["gdsp_upfirdn_length"] == (I64, [I64, I64, I64, I64])
    assert S["gdsp_upfirdn_fused"] == (I, [I64, I64, I64])
    # (x, ldx, h, m, up, down, channels, n, out_begin, out_end, out, ldo)
    assert S["gdsp_upfirdn_batch"] == (I, [P, I64, P, I64, I64, I64, I64, I64, I64, I64, P, I64])
    assert S["gdsp_upfirdn_batch_device"] == (I, [P, I64, P, I64, I64, I64, I64, I64, I64, I64, P,
                                                  I64, P, P])
    hdr = open(os.path.join(REPO, "include", "gdsp_fft.h")).read()
    assert "GDSP_ALGO_NO_FUSED_UPFIRDN = 8192" in hdr
    assert "resampling" in hdr.split("---- values")[1].split("---- fft package")[0]
    assert "gdsp_upfirdn_batch" in hdr.split("later_chunks:")[1].split("gdsp_loop_stats(")[0]


def test_no_fused_upfirdn_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_UPFIRDN == 8192
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_UPFIRDN)
        assert F.Algorithm() == 8192
        F.SetAlgorithm(F.ALGO_NO_FUSED_UPFIRDN | F.ALGO_NO_FUSED_ISTFT | F.ALGO_NO_FUSED_FIR)
        assert F.Algorithm() == 8192 | 4096 | 512
        for bad in (2048, 8192 | 2048, 16384, 1 << 20):
            with pytest.raises(gdsp.GDSPError) as e:
                F.SetAlgorithm(bad)
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == 8192 | 4096 | 512
    finally:
        F.SetAlgorithm(prev)


def _entries(gdsp):
    """Both entries behind one signature: (x, ldx, h, m, up, down, channels, n,
    out_begin, out_end, out, ldo) -> status."""
    L = gdsp._lib.lib()
    null = gdsp._lib._P()
    return (L.gdsp_upfirdn_batch, lambda *a: L.gdsp_upfirdn_batch_device(*a, null, null))


def test_status_codes_before_any_device_call(gdsp):
    G = gdsp._lib
    buf, obuf, hbuf = np.zeros(4096), np.zeros(4096), np.zeros(64)
    p, o, h = (a.ctypes.data_as(G._P) for a in (buf, obuf, hbuf))
    null = G._P()
    big = 1 << 62
    for f in _entries(gdsp):
        # 2 rows of 8 samples, 3 taps, 3/2: L = (7 * 3 + 2) div 2 + 1 = 12
        def call(x=p, ldx=8, hh=h, m=3, up=3, down=2, channels=2, n=8, b=0, e=-1, out=o, ldo=12):
            return f(x, ldx, hh, m, up, down, channels, n, b, e, out, ldo)

        # 1. negative sizes, rates below 1, ranges, strides
        assert call(m=-1) == G.GDSP_ERR_INVALID
        assert call(n=-1) == G.GDSP_ERR_INVALID
        assert call(channels=-1) == G.GDSP_ERR_INVALID
        assert call(up=0) == G.GDSP_ERR_INVALID
        assert call(down=0) == G.GDSP_ERR_INVALID
        assert call(up=-3) == G.GDSP_ERR_INVALID
        assert call(b=-1) == G.GDSP_ERR_INVALID
        assert call(b=5, e=4) == G.GDSP_ERR_INVALID          # reversed
        assert call(e=13) == G.GDSP_ERR_INVALID              # past L
        assert call(b=13, e=13) == G.GDSP_ERR_INVALID
        assert call(e=-2) == G.GDSP_ERR_INVALID
        assert call(n=0, e=1) == G.GDSP_ERR_INVALID          # L = 0
        assert call(ldx=7) == G.GDSP_ERR_INVALID
        assert call(ldo=11) == G.GDSP_ERR_INVALID
        assert call(b=2, e=9, ldo=6) == G.GDSP_ERR_INVALID
        # ... all before the later ones: a bad range with no channels, no samples, rates too high
        assert call(channels=0, e=13) == G.GDSP_ERR_INVALID
        assert call(n=0, up=0) == G.GDSP_ERR_INVALID
        assert call(up=1 << 17, ldx=7) == G.GDSP_ERR_INVALID
        assert call(n=big, up=65536, ldx=big, b=-1) == G.GDSP_ERR_INVALID
        # 2. no channels: nothing is looked at
        assert call(x=null, hh=null, out=null, channels=0) == G.GDSP_OK
        assert call(x=null, hh=null, out=null, channels=0, n=0, m=0, ldx=0, ldo=0) == G.GDSP_OK
        assert call(x=null, hh=null, out=null, channels=0, up=1 << 20) == G.GDSP_OK
        # 3. empty input, before the rates and the pointers are looked at
        assert call(n=0, ldx=0, ldo=0) == G.GDSP_ERR_EMPTY
        assert call(m=0, ldo=0) == G.GDSP_ERR_EMPTY
        assert call(n=0, m=0, e=0, ldo=0) == G.GDSP_ERR_EMPTY
        assert call(x=null, n=0, up=1 << 17, e=0, ldo=0) == G.GDSP_ERR_EMPTY
        # 4. beyond the supported sizes, before the pointers are looked at
        assert call(up=65537, e=0) == G.GDSP_ERR_UNSUPPORTED
        assert call(down=65537, e=0) == G.GDSP_ERR_UNSUPPORTED
        assert call(m=(1 << 24) + 1, e=0) == G.GDSP_ERR_UNSUPPORTED
        assert call(x=null, hh=null, out=null, up=65537, e=0) == G.GDSP_ERR_UNSUPPORTED
        assert call(n=big, up=65536, ldx=big, e=0) == G.GDSP_ERR_UNSUPPORTED  # (n - 1) up overflows
        assert call(channels=1, n=big, up=65536, b=7, e=9) == G.GDSP_ERR_UNSUPPORTED
        # 5. a needed NULL pointer, also for an empty range
        assert call(x=null) == G.GDSP_ERR_INVALID
        assert call(hh=null) == G.GDSP_ERR_INVALID
        assert call(out=null) == G.GDSP_ERR_INVALID
        assert call(out=null, b=4, e=4) == G.GDSP_ERR_INVALID
        # 6. an empty range
        assert call(b=0, e=0) == G.GDSP_OK
        assert call(b=12, e=12) == G.GDSP_OK
        assert call(b=5, e=5, ldo=0) == G.GDSP_OK
        if gdsp.device_count() == 0:
            assert call() == G.GDSP_ERR_NO_DEVICE
            assert call(b=3, e=4) == G.GDSP_ERR_NO_DEVICE
            assert call(up=65536, down=65536, ldo=8) == G.GDSP_ERR_NO_DEVICE
    # the limits themselves are served
    F = gdsp.fft
    assert F.upfirdn_length(8, 1 << 24, 65536, 65536) == (7 * 65536 + (1 << 24) - 1) // 65536 + 1


def test_device_entry_rejects_overlapping_ranges(gdsp):
    """The overlap rule is arithmetic on the two address ranges: fake pointers
    suffice, no device is touched. It stands before the empty range."""
    G = gdsp._lib
    d = G.lib().gdsp_upfirdn_batch_device
    null = G._P()
    base = 1 << 40
    h = G._P(1 << 30)

    # 2 rows of 100 at stride 128, 5 taps, 1/1: L = 104
    def call(xa, oa, channels=2, n=100, ldx=128, ldo=128, b=0, e=-1):
        return d(G._P(xa), ldx, h, 5, 1, 1, channels, n, b, e, G._P(oa), ldo, null, null)

    assert call(base, base) == G.GDSP_ERR_INVALID                    # in place
    assert call(base, base + 8 * 50) == G.GDSP_ERR_INVALID           # out starts inside x
    assert call(base + 8 * 50, base) == G.GDSP_ERR_INVALID           # x starts inside out
    assert call(base, base + 8 * 227) == G.GDSP_ERR_INVALID          # x spans 228 doubles
    assert call(base + 8 * 231, base) == G.GDSP_ERR_INVALID          # out spans 232
    # a range of 10 outputs per row spans 138: its last double still collides
    assert call(base + 8 * 137, base, b=20, e=30) == G.GDSP_ERR_INVALID
    assert call(base, base + 8 * 99, channels=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID
    assert call(base, base + 8 * 300, b=7, e=7) == G.GDSP_OK         # apart, and empty


def _count(n, m, up, down):
    """The definition, counted: the n samples stuffed to (n - 1) up + 1, the full
    convolution with m taps, every down-th of its samples."""
    if n == 0 or m == 0:
        return 0
    stuffed = np.zeros((n - 1) * up + 1)
    return len(np.convolve(stuffed, np.zeros(m))[::down])


def test_length_against_a_brute_force_count(gdsp):
    F = gdsp.fft
    for up in range(1, 6):
        for down in range(1, 6):
            for n in range(13):
                for m in range(13):
                    want = _count(n, m, up, down)
                    assert F.upfirdn_length(n, m, up, down) == want, (n, m, up, down)
                    assert R.out_len(n, m, up, down) == want
    for bad in ((-1, 3, 1, 1), (3, -1, 1, 1), (3, 3, 0, 1), (3, 3, 1, 0), (0, 0, 0, 1),
                (3, 3, 65537, 1), (3, 3, 1, 65537), (3, (1 << 24) + 1, 1, 1), (1 << 62, 3, 4, 1)):
        assert F.upfirdn_length(*bad) == -1, bad
    assert F.upfirdn_length(0, 3, 65537, 1) == 0
    assert F.upfirdn_length(1 << 62, 3, 1, 1) == (1 << 62) + 2


# (m, up, down): the shapes the fused kernel is promised for
def _promised():
    yield 3218, 160, 147
    yield 3361, 147, 160
    yield 20 * 160 + 1, 160, 147   # resample_taps' own lengths
    yield 20 * 160 + 1, 147, 160
    for r in range(2, 17):
        yield 20 * r + 1, r, 1
        yield 20 * r + 1, 1, r
        yield 20 * r + 1 + r, 1, r  # with ResamplePoly's zeros in front
        yield 20 * r + 2, r, 1
    for m in (1, 3, 4, 7, 64, 81, 200, 337, 1001):
        yield m, 1, 1


def test_fused_query_is_host_arithmetic(gdsp):
    F = gdsp.fft
    q = F.upfirdn_fused
    for m, up, down in _promised():
        assert q(m, up, down), (m, up, down)
    assert q(7, 3, 2) and q(3, 8, 1) and q(200, 5, 7) and q(64, 7, 3)
    assert not q(9000, 1024, 1023)       # the table alone is beyond the LDS budget
    assert not q(9000, 1, 1)
    assert not q(3, 1, 50)               # the samples of the smallest tile are
    assert not q(0, 1, 1) and not q(3, 0, 1) and not q(3, 1, 0) and not q(-1, 1, 1)
    assert not q(3, 65537, 1) and not q((1 << 24) + 1, 1, 1)
    prev = F.Algorithm()
    try:
        # the flags of the other fused kernels do not touch this one, its own does
        F.SetAlgorithm(F.ALGO_NO_FUSED_FIR | F.ALGO_NO_FUSED_ISTFT | F.ALGO_NO_FUSED_CONVOLVE)
        assert q(3218, 160, 147)
        F.SetAlgorithm(F.ALGO_NO_FUSED_UPFIRDN)
        assert F.fir_block(31)[1]
        for m, up, down in list(_promised()) + [(7, 3, 2), (9000, 1024, 1023)]:
            assert not q(m, up, down), (m, up, down)
    finally:
        F.SetAlgorithm(prev)
    assert q(3218, 160, 147)


RATIOS = ((160, 147), (147, 160), (1, 8), (3, 1), (2, 3), (48, 44))


def test_resample_taps_are_the_written_formula(gdsp):
    for up, down in RATIOS + ((1, 1), (441, 480), (6, 4)):
        h = gdsp.fft.resample_taps(up, down)
        want = R.taps(up, down)
        assert h.dtype == np.float64 and h.shape == want.shape
        assert np.max(np.abs(h - want)) <= 1e-14 * np.max(np.abs(want)), (up, down)
        assert np.max(np.abs(h - h[::-1])) < 1e-15
    assert gdsp.fft.resample_taps(6, 4).size == 20 * 3 + 1
    with pytest.raises(gdsp.GDSPError):
        gdsp.fft.resample_taps(0, 3)


def test_resample_taps_against_scipy_firwin(gdsp):
    ss = pytest.importorskip("scipy.signal")
    for up, down in RATIOS:
        h = gdsp.fft.resample_taps(up, down)
        u, d = R.plan(1000, h.size, up, down)[:2]
        want = ss.firwin(h.size, 1.0 / max(u, d), window=("kaiser", 5.0)) * u
        diff = np.max(np.abs(h - want))
        print(f"{up}/{down}: {diff:.2e} of {np.max(np.abs(want)):.3f}")
        assert diff <= 1e-14 * np.max(np.abs(want)), (up, down)


def test_resample_poly_arithmetic(gdsp):
    F = gdsp.fft
    n = 1000
    found = []
    for up, down in RATIOS:
        pl = F.resample_plan(n, up, down)
        u, d, pre, post, rem, n_out = R.plan(n, 20 * max(pl["up"], pl["down"]) + 1, up, down)
        assert (pl["up"], pl["down"], pl["pre"], pl["post"], pl["rem"], pl["n_out"]) == \
            (u, d, pre, post, rem, n_out), (up, down)
        m = 20 * max(u, d) + 1
        assert pl["half"] == 10 * max(u, d) and pl["n_out"] == -(-n * u // d)
        assert pl["pre"] == d - pl["half"] % d and pl["rem"] == (pl["half"] + pl["pre"]) // d
        # the padded taps reach exactly far enough: one zero less behind them would not
        assert F.upfirdn_length(n, m + pre + post, u, d) >= rem + n_out
        assert post == 0 or F.upfirdn_length(n, m + pre + post - 1, u, d) < rem + n_out
        found.append((pre, post))
    assert found == [(17, 0), (160, 0), (8, 0), (1, 0), (3, 0), (1, 0)]
    # taps given: their own length counts; trailing zeros only where L would be short
    pl = F.resample_plan(10, 1, 3, 2)
    assert (pl["half"], pl["pre"], pl["rem"], pl["n_out"], pl["post"]) == (0, 3, 1, 4, 0)
    pl = F.resample_plan(10, 5, 1, 1)
    assert (pl["half"], pl["pre"], pl["rem"], pl["n_out"], pl["post"]) == (0, 1, 1, 50, 4)
    assert F.upfirdn_length(10, 1 + 1 + 4, 5, 1) == 51
    assert F.upfirdn_length(10, 1 + 1 + 3, 5, 1) == 50


def test_python_mirrors_refuse_before_any_device_call(gdsp):
    F = gdsp.fft
    x = np.zeros((2, 8))
    with pytest.raises(TypeError):
        F.UpfirdnBatch(x.astype(np.complex128), np.ones(3), 2, 1)
    with pytest.raises(TypeError):
        F.UpfirdnBatch(x, np.ones(3, np.complex128), 2, 1)
    with pytest.raises(TypeError):
        F.Upfirdn(np.zeros(8, np.complex128), np.ones(3))
    with pytest.raises(TypeError):
        F.ResamplePoly(np.zeros(8, np.complex128), 2, 1)
    with pytest.raises(TypeError):
        F.ResamplePolyBatch(x, 2, 1, taps=np.ones(3, np.complex128))
    with pytest.raises(gdsp.Panic):
        F.UpfirdnBatch(x, np.ones((2, 3)), 2, 1)
    with pytest.raises(gdsp.Panic):
        F.UpfirdnBatch(np.zeros((2, 0)), np.ones(3), 2, 1)          # GDSP_ERR_EMPTY
    with pytest.raises(gdsp.GDSPError) as e:
        F.UpfirdnBatch(x, np.ones(3), 0, 1)
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    with pytest.raises(gdsp.GDSPError) as e:
        F.UpfirdnBatch(x, np.ones(3), 1, 1, 4, 20)
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    assert F.UpfirdnBatch(np.zeros((0, 8)), np.ones(3), 3, 2).shape == (0, 12)
    # up == down copies, whatever the taps; no device is needed
    y = np.arange(12.0).reshape(2, 6)
    for got in (F.ResamplePolyBatch(y, 3, 3), F.ResamplePolyBatch(y, 44, 44, taps=np.ones(5))):
        assert np.array_equal(got, y) and got is not y
    assert np.array_equal(F.ResamplePoly(y[0], 7, 7), y[0])
    assert F.ResamplePolyBatch(np.zeros((3, 0)), 2, 3).shape == (3, 0)
    assert F.ResamplePolyBatch(np.zeros((0, 9)), 2, 3).shape == (0, 6)


def test_reference_forms_agree():
    """resample_ref.upfirdn with and without the stuffed zeros: the same sums in
    np.longdouble, far inside the GPU tests' bound."""
    rng = np.random.default_rng(5)
    for up, down, m, n in ((3, 2, 7, 50), (8, 1, 3, 20), (5, 7, 200, 3), (7, 3, 64, 1),
                           (16, 15, 330, 200), (1, 4, 101, 150)):
        x, h = rng.standard_normal((2, n)), rng.standard_normal(m)
        a, b = R.upfirdn(x, h, up, down, literal=True), R.upfirdn(x, h, up, down, literal=False)
        assert a.shape == b.shape == (2, R.out_len(n, m, up, down))
        assert row_nrel(b, a) < 1e-15, (up, down, m, n, row_nrel(b, a))
