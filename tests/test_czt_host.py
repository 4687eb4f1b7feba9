"""CPU-only checks of the chirp-z boundary (gdsp_czt_tables, gdsp_czt_length,
gdsp_czt_fused, gdsp_czt_batch, the plan object and gdsp_czt_batch_device): the
entry points are declared, exported and bound alike; GDSP_ALGO_NO_FUSED_CZT is
the known bit 262144 while 2048, 16384 and 131072 stay unknown; the length and
fused queries are host arithmetic; every status code that answers before a
device is touched, through every entry, with pointers that would fault if
touched; the host tables against an evaluation at 50 digits, every angle
reduced exactly; and the reference the GPU tests compare with (czt_ref.py)
against direct sums, against scipy and against itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import czt_ref as R
import exact_dft as E
from conftest import REPO

NAMES = ("gdsp_czt_tables", "gdsp_czt_length", "gdsp_czt_fused", "gdsp_czt_batch",
         "gdsp_czt_plan_create", "gdsp_czt_plan_destroy", "gdsp_czt_plan_info",
         "gdsp_czt_work_bytes", "gdsp_czt_batch_device")


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
    PI64, PI = ctypes.POINTER(I64), ctypes.POINTER(I)
    # (n, m, F, a_abs, a_turns, step_turns, step_div, A, v, P)
    assert S["gdsp_czt_tables"] == (I, [I64, I64, I64, D, D, D, I64, P, P, P])
    assert S["gdsp_czt_length"] == (I64, [I64, I64, PI])
    assert S["gdsp_czt_fused"] == (I, [I64, I64])
    # (x, ldx, is_real, rows, n, m, a_abs, a_turns, step_turns, step_div, out, ldo)
    assert S["gdsp_czt_batch"] == (I, [P, I64, I, I64, I64, I64, D, D, D, I64, P, I64])
    assert S["gdsp_czt_plan_create"] == (I, [I64, I64, D, D, D, I64, ctypes.POINTER(P)])
    assert S["gdsp_czt_plan_destroy"] == (I, [P])
    assert S["gdsp_czt_plan_info"] == (I, [P, PI64, PI64, PI64, PI])
    assert S["gdsp_czt_work_bytes"] == (I64, [P, I64])
    # (plan, x, ldx, is_real, rows, out, ldo, work, work_bytes, stream)
    assert S["gdsp_czt_batch_device"] == (I, [P, P, I64, I, I64, P, I64, P, I64, P])
    hdr = open(os.path.join(REPO, "include", "gdsp_fft.h")).read()
    assert "GDSP_ALGO_NO_FUSED_CZT = 262144" in hdr
    assert "131072" in hdr.split("GDSP_ALGO_NO_FUSED_CZT = 262144")[0].rsplit("/*", 1)[1]
    values = hdr.split("---- values")[1].split("---- fft package")[0]
    assert "CZT" in values and "zero row gives zeros" in values
    assert "gdsp_czt_batch" in hdr.split("later_chunks:")[1].split("gdsp_loop_stats(")[0]
    doc = hdr.split("int gdsp_czt_tables(")[0].rsplit("/* The chirp-z transform", 1)[1]
    assert "EXACTLY" in doc and "Spirals" in doc and "NOT offered" in doc


def test_no_fused_czt_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_CZT == 262144
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_CZT)
        assert F.Algorithm() == 262144
        F.SetAlgorithm(F.ALGO_NO_FUSED_CZT | F.ALGO_NO_FUSED_HILBERT | F.ALGO_NO_FUSED_SOSFILT)
        assert F.Algorithm() == 262144 | 32768 | 65536
        for bad in (2048, 16384, 131072, 262144 | 131072, 262144 | 2048, 1 << 19, 1 << 20):
            with pytest.raises(gdsp.GDSPError) as e:
                F.SetAlgorithm(bad)
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == 262144 | 32768 | 65536
    finally:
        F.SetAlgorithm(prev)


def test_length_and_fused_are_host_arithmetic(gdsp):
    F = gdsp.fft
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(prev & ~F.ALGO_NO_FUSED_CZT)
        # n + m - 1 = 256, 257, 16384, 16385, 2^20, 2^20 + 1
        table = (((128, 129), 256, True), ((1, 256), 256, True), ((129, 129), 512, True),
                 ((257, 1), 512, True), ((1, 1), 256, True), ((2, 255), 256, True),
                 ((8192, 8193), 16384, True), ((16384, 1), 16384, True),
                 ((8193, 8193), 32768, False), ((1, 16385), 32768, False),
                 ((1 << 19, (1 << 19) + 1), 1 << 20, False), ((1 << 20, 1), 1 << 20, False),
                 (((1 << 19) + 1, (1 << 19) + 1), 0, False), ((1 << 20, 2), 0, False),
                 ((1, (1 << 20) + 1), 0, False), ((0, 5), 0, False), ((5, 0), 0, False),
                 ((-1, 5), 0, False), ((3000, 1000), 4096, True), ((4097, 4096), 8192, True))
        for (n, m), want, fused in table:
            assert F.czt_length(n, m) == (want, fused), (n, m)
            assert F.czt_fused(n, m) is fused, (n, m)
        assert gdsp._lib.lib().gdsp_czt_length(100, 100, None) == 256  # fused may be NULL
        # other flags do not matter; this one turns every length off
        F.SetAlgorithm(F.ALGO_NO_FUSED_HILBERT | F.ALGO_NO_FUSED_CONVOLVE)
        assert F.czt_length(128, 129) == (256, True)
        F.SetAlgorithm(F.ALGO_NO_FUSED_CZT)
        for (n, m), want, _ in table:
            assert F.czt_length(n, m) == (want, False), (n, m)
            assert F.czt_fused(n, m) is False
    finally:
        F.SetAlgorithm(prev)


def test_status_codes_in_order_before_any_device_call(gdsp):
    G = gdsp._lib
    L = G.lib()
    null = G._P()
    # far apart, unmapped: a call that touched either would fault
    px, po = G._P(1 << 44), G._P(1 << 45)
    nan, inf = float("nan"), float("inf")

    def call(x=px, ldx=300, is_real=1, rows=3, n=300, m=200, a_abs=1.0, a_turns=0.1, st=0.05,
             sd=200, out=po, ldo=200):
        return L.gdsp_czt_batch(x, ldx, is_real, rows, n, m, a_abs, a_turns, st, sd, out, ldo)

    # 1. sizes, is_real, strides, parameters
    for kw in (dict(rows=-1), dict(n=-1), dict(m=-1), dict(is_real=2), dict(is_real=-1),
               dict(ldx=299), dict(ldo=199), dict(a_abs=0.0), dict(a_abs=-1.0), dict(a_abs=nan),
               dict(a_abs=inf), dict(a_turns=nan), dict(a_turns=inf), dict(st=nan), dict(st=-inf),
               dict(sd=0), dict(sd=-5),
               # ... all before the later ones: no rows, no samples, no pointers
               dict(rows=0, sd=0), dict(rows=0, n=-1), dict(n=0, ldx=0, is_real=7),
               dict(x=null, out=null, ldx=1), dict(n=0, ldx=0, a_abs=0.0)):
        assert call(**kw) == G.GDSP_ERR_INVALID, kw
    # 2. no rows: nothing is looked at
    assert call(x=null, out=null, rows=0) == G.GDSP_OK
    assert call(x=null, out=null, rows=0, n=0, m=0, ldx=0, ldo=0) == G.GDSP_OK
    # 3. empty input, before the pointers are looked at
    assert call(n=0, ldx=0) == G.GDSP_ERR_EMPTY
    assert call(m=0, ldo=0) == G.GDSP_ERR_EMPTY
    assert call(x=null, out=null, n=0, ldx=0) == G.GDSP_ERR_EMPTY
    # 4. a NULL pointer; one row needs no stride
    assert call(x=null) == G.GDSP_ERR_INVALID
    assert call(out=null) == G.GDSP_ERR_INVALID
    assert call(x=null, rows=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID
    # 5. a convolution above 2^20
    big = 1 << 20
    assert call(n=big, ldx=big, m=2, ldo=2) == G.GDSP_ERR_UNSUPPORTED
    assert call(n=(1 << 19) + 1, ldx=big, m=(1 << 19) + 1, ldo=big) == G.GDSP_ERR_UNSUPPORTED
    # 6. a circle whose a_abs^-(n-1) leaves the double range
    assert call(a_abs=0.9, n=8000, ldx=8000) == G.GDSP_ERR_INVALID
    assert call(a_abs=1.1, n=8000, ldx=8000) == G.GDSP_ERR_INVALID   # underflow: not normal
    if gdsp.device_count() == 0:
        assert call() == G.GDSP_ERR_NO_DEVICE
        assert call(is_real=0, rows=1, ldx=0, ldo=0, a_abs=0.999) == G.GDSP_ERR_NO_DEVICE

    # the plan: the same parameter checks, in the same order
    h = ctypes.c_void_p()

    def create(n=300, m=200, a_abs=1.0, a_turns=0.1, st=0.05, sd=200, ref=ctypes.byref(h)):
        return L.gdsp_czt_plan_create(n, m, a_abs, a_turns, st, sd, ref)

    assert create(ref=None) == G.GDSP_ERR_INVALID
    for kw in (dict(n=-1), dict(m=-1), dict(a_abs=0.0), dict(a_abs=nan), dict(a_turns=inf),
               dict(st=nan), dict(sd=0), dict(n=0, sd=0), dict(m=0, a_abs=-2.0)):
        assert create(**kw) == G.GDSP_ERR_INVALID, kw
        assert h.value is None
    assert create(n=0) == G.GDSP_ERR_EMPTY
    assert create(m=0) == G.GDSP_ERR_EMPTY
    assert create(n=big, m=2) == G.GDSP_ERR_UNSUPPORTED
    assert create(n=8000, a_abs=0.9) == G.GDSP_ERR_INVALID
    if gdsp.device_count() == 0:
        assert create() == G.GDSP_ERR_NO_DEVICE
        assert h.value is None
    # without a plan the plan's entries answer at once
    assert L.gdsp_czt_plan_destroy(null) == G.GDSP_OK
    assert L.gdsp_czt_plan_info(null, None, None, None, None) == G.GDSP_ERR_INVALID
    assert L.gdsp_czt_work_bytes(null, 5) == 0
    assert L.gdsp_czt_batch_device(null, px, 300, 1, 3, po, 200, null, 0, null) == G.GDSP_ERR_INVALID


def _tables(gdsp, n, m, F, a_abs, a_turns, st, sd):
    A, v, P = (np.empty(k, np.complex128) for k in (n, F, m))
    p = gdsp._lib._P
    status = gdsp._lib.lib().gdsp_czt_tables(n, m, F, a_abs, a_turns, st, sd, A.ctypes.data_as(p),
                                             v.ctypes.data_as(p), P.ctypes.data_as(p))
    return status, A, v, P


def _mp_tables(n, m, F, a_abs, a_turns, st, sd):
    """The three tables at 50 digits, each angle reduced modulo one turn as an
    exact rational (Python integers) first; as pairs of lists of mpf."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    ps, qs = float(st).as_integer_ratio()
    pa, qa = float(a_turns).as_integer_ratio()
    den_c, two_pi = 2 * qs * int(sd), 2 * mp.pi

    def cis(num, den):  # exp(-2 pi i num / den)
        ang = two_pi * mp.mpf(num % den) / mp.mpf(den)
        return mp.cos(ang), -mp.sin(ang)

    c = [cis(j * j * ps, den_c) for j in range(max(n, m))]
    A = []
    mag, inv = mp.mpf(1), 1 / mp.mpf(a_abs)
    for j in range(n):
        re, im = cis(j * j * ps * qa + 2 * j * pa * qs * int(sd), den_c * qa)
        A.append((mag * re, mag * im))
        mag *= inv
    zero = (mp.mpf(0), mp.mpf(0))
    v = [zero] * F
    for d in range(-(n - 1), m):
        re, im = c[abs(d)]
        v[d % F] = (re, -im)
    return A, v, c[:m]


TABLE_SETS = [
    ("dft-3000", 3000, 3000, 1.0, 0.0, 1.0, 3000),
    # j^2 step / 2 reaches 10^3 turns
    ("zoom-8192", 8192, 8193, 1.0, 0.1234 / 2, 0.1111 / 2, 8193),
    # ... 10^7 turns
    ("step0.37-16000", 16000, 300, 1.0, 0.25, 0.37, 1),
    ("step1e-300", 700, 500, 1.0, 0.3, 1e-300, 3),
    ("negative-step", 1500, 1200, 1.0, -0.2, -0.123, 911),
    ("a0.999-4000", 4000, 4000, 0.999, 0.05, 0.3, 4001),
]


@pytest.mark.parametrize("case", TABLE_SETS, ids=[c[0] for c in TABLE_SETS])
def test_tables_within_one_u_of_fifty_digits(gdsp, case):
    """Every component of every entry within 1 u of the entry's modulus."""
    _, n, m, a_abs, a_turns, st, sd = case
    F = gdsp.fft.czt_length(n, m)[0]
    status, A, v, P = _tables(gdsp, n, m, F, a_abs, a_turns, st, sd)
    assert status == gdsp._lib.GDSP_OK
    try:
        import mpmath as mp
        ref = _mp_tables(n, m, F, a_abs, a_turns, st, sd)
    except ImportError:  # the extended tables of czt_ref, 2^-63 instead of 50 digits
        mp = None
        ref = R.tables(n, m, F, a_abs, a_turns, st, sd)
    worst = 0.0
    for name, got, want in zip("AvP", (A, v, P), ref):
        assert len(got) == len(want)
        if mp is None:
            mod = np.abs(want)
            d = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
            assert np.all(got[mod == 0] == 0)
            e = float((d[mod > 0] / mod[mod > 0]).max() / E.LD(E.U))
        else:
            e = 0.0
            for g, (re, im) in zip(got, want):
                mod = mp.sqrt(re * re + im * im)
                if mod == 0:
                    assert g == 0
                    continue
                d = max(abs(mp.mpf(float(g.real)) - re), abs(mp.mpf(float(g.imag)) - im))
                e = max(e, float(d / mod / mp.mpf(E.U)))
        print("czt tables %s %s: %.4f u" % (case[0], name, e))
        worst = max(worst, e)
    assert worst <= 1.0
    # the extended tables the GPU tests' reference uses are the same tables
    for got, want in zip((A, v, P), R.tables(n, m, F, a_abs, a_turns, st, sd)):
        assert E.err_u(got, want) <= 1.0


def test_tables_refuse_what_leaves_the_double_range(gdsp):
    G = gdsp._lib
    # 0.9^-7999 overflows; 1.1^-7999 is subnormal and then zero
    assert _tables(gdsp, 8000, 100, 8192, 0.9, 0.0, 1.0, 8000)[0] == G.GDSP_ERR_INVALID
    assert _tables(gdsp, 8000, 100, 8192, 1.1, 0.0, 1.0, 8000)[0] == G.GDSP_ERR_INVALID
    assert _tables(gdsp, 4000, 100, 8192, 0.9, 0.0, 1.0, 8000)[0] == G.GDSP_OK  # 0.9^-3999 = 1e183
    nan = float("nan")
    for kw in (dict(n=0), dict(m=0), dict(F=298), dict(F=(1 << 20) + 1), dict(a_abs=0.0),
               dict(a_abs=nan), dict(a_turns=nan), dict(st=float("inf")), dict(sd=0)):
        a = dict(n=200, m=100, F=300, a_abs=1.0, a_turns=0.0, st=0.5, sd=3)
        a.update(kw)
        assert _tables(gdsp, a["n"], a["m"], a["F"], a["a_abs"], a["a_turns"], a["st"],
                       a["sd"])[0] == G.GDSP_ERR_INVALID, kw
    p = G._P
    buf = np.empty(512, np.complex128).ctypes.data_as(p)
    L = G.lib()
    assert L.gdsp_czt_tables(10, 10, 256, 1.0, 0.0, 1.0, 10, None, buf, buf) == G.GDSP_ERR_INVALID
    # any F >= n + m - 1 is a table length, not only the engine's own
    assert _tables(gdsp, 200, 100, 299, 1.0, 0.0, 0.5, 3)[0] == G.GDSP_OK


# ---- the reference ---------------------------------------------------------------

PARAMS = [
    ("dft", dict()),
    ("zoom", dict(zoom=([0.1234, 0.2345], 2, False))),
    ("zoom-endpoint", dict(zoom=([0.1234, 0.2345], 2, True))),
    ("step0.37", dict(step_turns=0.37, step_div=1)),
    ("a0.999", dict(a_abs=0.999, step_turns=0.3, step_div=401, a_turns=0.05)),
]


def _kw(p, m):
    p = dict(p)
    if "zoom" in p:
        fn, fs, endpoint = p.pop("zoom")
        at, st, sd = R.zoom_params(fn, m, fs, endpoint)
        p.update(a_turns=at, step_turns=st, step_div=sd)
    return p


@pytest.mark.parametrize("name,p", PARAMS, ids=[c[0] for c in PARAMS])
@pytest.mark.parametrize("n,m", [(300, 257), (1000, 1000)])
def test_reference_against_direct_sums(name, p, n, m):
    x = E.standard_rows(n)
    kw = _kw(p, m)
    ex = R.czt_exact(x, m, **kw)
    ks = [0, 1, m // 3, m - 2, m - 1]
    # err_u's metric, the scale a row's largest output or the 2-norm of its
    # terms x[j] a_abs^-j, whichever is larger: the rounding error of a sum is
    # relative to its terms, not to a result cancellation made small (the step
    # 0.37 = 37/100 puts every point on a null of the tone row's kernel: its
    # largest output is 0.03 against terms of size 1)
    terms = np.abs(x) * kw.get("a_abs", 1.0) ** -np.arange(n)
    scale = np.maximum(np.abs(ex).max(axis=1), np.sqrt((terms * terms).sum(axis=1)).astype(E.LD))
    d = np.abs(ex[:, ks] - R.czt_bins(x, ks, m, **kw)).max(axis=1) / scale
    e = float(d.max() / E.LD(E.U))
    print("czt_ref %s n=%d m=%d: exact against direct sums %.3g u" % (name, n, m, e))
    # 2^-63 arithmetic over log2 F passes, about 2000 times finer than float64
    assert e < 0.25
    f = E.err_u(R.czt_float64(x, m, **kw), ex)
    print("czt_ref %s n=%d m=%d: float64 route %.3g u" % (name, n, m, f))
    assert 0 < f < 1e4


def test_reference_default_is_the_dft():
    for n in (255, 256, 1000):
        x = E.standard_rows(n)
        assert E.err_u(R.czt_exact(x), E.exact_fft(x)) < 0.25


def test_float64_route_against_scipy():
    """The triangle inequality and no new number: our float64 statement is as
    near scipy's result as both are near the exact one."""
    signal = pytest.importorskip("scipy.signal")
    if not hasattr(signal, "zoom_fft"):
        pytest.skip("scipy.signal has no zoom_fft")
    n, m = 300, 257
    x = E.standard_rows(n)
    for endpoint in (False, True):
        fn = [0.1234, 0.2345]
        kw = _kw(dict(zoom=(fn, 2, endpoint)), m)
        ex = R.czt_exact(x, m, **kw)
        ours = R.czt_float64(x, m, **kw)
        theirs = signal.zoom_fft(x, fn, m, fs=2, endpoint=endpoint, axis=1)
        bound = E.err_u(theirs, ex) + E.MARGIN * E.err_u(ours, ex)
        got = E.err_u(ours, theirs.astype(E.CLD))
        print("zoom_fft endpoint=%s: ours - scipy %.3g u, bound %.3g u" % (endpoint, got, bound))
        assert got <= bound
    for name, p in PARAMS[3:]:
        kw = _kw(p, m)
        ex = R.czt_exact(x, m, **kw)
        ours = R.czt_float64(x, m, **kw)
        step = kw["step_turns"] / kw["step_div"]
        w = np.exp(-2j * np.pi * step)
        a = kw.get("a_abs", 1.0) * np.exp(2j * np.pi * kw.get("a_turns", 0.0))
        theirs = signal.czt(x, m, w, a, axis=1)
        bound = E.err_u(theirs, ex) + E.MARGIN * E.err_u(ours, ex)
        got = E.err_u(ours, theirs.astype(E.CLD))
        print("czt %s: ours - scipy %.3g u, bound %.3g u" % (name, got, bound))
        assert got <= bound


def test_python_wrappers(gdsp):
    F = gdsp.fft
    assert np.array_equal(F.zoom_freqs([1.0, 2.0], 4), [1.0, 1.25, 1.5, 1.75])
    assert np.array_equal(F.zoom_freqs(2.0, 5, endpoint=True), [0.0, 0.5, 1.0, 1.5, 2.0])
    z = F.czt_points(8)
    assert np.allclose(z, np.exp(2j * np.pi * np.arange(8) / 8))
    z = F.czt_points(3, 0.25, 2, a_turns=0.5, a_abs=2.0)
    assert np.allclose(z, 2.0 * np.exp(2j * np.pi * (0.5 + np.arange(3) * 0.125)))
    with pytest.raises(ValueError):
        F.CZTBatch(np.ones(8))
    with pytest.raises(ValueError):
        F.ZoomFFT(np.ones(8), [1, 2, 3])
    with pytest.raises(gdsp.GDSPError) as e:
        F.CZT(np.zeros(0))
    assert e.value.status == gdsp._lib.GDSP_ERR_EMPTY
    with pytest.raises(gdsp.GDSPError) as e:
        F.CZT(np.ones(8), step_turns=0.5, step_div=0)
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    assert F.CZTBatch(np.zeros((0, 16)), 5).shape == (0, 5)
