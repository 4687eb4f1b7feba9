"""CPU-only checks of the recursive-filter boundary (gdsp_sosfilt_batch,
gdsp_sosfiltfilt_batch, their device entries, gdsp_sosfilt_fused,
gdsp_sosfilt_granule, gdsp_sosfilt_zi, gdsp_sosfiltfilt_padlen): the entries are
declared, exported and bound alike; GDSP_ALGO_NO_FUSED_SOSFILT is the known bit
65536 while 2048 and 16384 stay unknown; which filters the time-parallel form
takes is host arithmetic; sosfilt_zi, padlen and butter_sos follow their written
formulas (and scipy, where present); every status code answers in its order
before any device call; and the numpy model of the time-parallel decomposition
(sos_ref.model) stays within the bound the GPU tests hold the kernel to, so
that the bound itself is checked without a GPU.

The model against the long-double recurrence, rows of 3 tiles, noise and noise
plus a DC of 100 (e = max|a - ref| / max|ref|, ratio = e / max(e_seq, 8 * 2^-53)):
butter8_0.2 1.00, butter6_band 1.14, cheby1_8_high 1.14, ellip8_0.05 1.16,
butter8_0.01 1.88, butter2_0.001 3.32; butter12_0.002 e = 4.1e-12."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sos_ref as R
from conftest import REPO

NAMES = ("gdsp_sosfilt_batch", "gdsp_sosfilt_batch_device", "gdsp_sosfiltfilt_batch",
         "gdsp_sosfiltfilt_batch_device", "gdsp_sosfilt_fused", "gdsp_sosfilt_granule",
         "gdsp_sosfilt_zi", "gdsp_sosfiltfilt_padlen", "gdsp_sosfilt_work_doubles",
         "gdsp_sosfiltfilt_work_doubles")


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
    # (x, ldx, sos, S, zi, channels, n, out, ldo, zf[, work, stream])
    assert S["gdsp_sosfilt_batch"] == (I, [P, I64, P, I64, P, I64, I64, P, I64, P])
    assert S["gdsp_sosfilt_batch_device"] == (I, [P, I64, P, I64, P, I64, I64, P, I64, P, P, P])
    # (x, ldx, sos, S, padlen, channels, n, out, ldo[, work, stream])
    assert S["gdsp_sosfiltfilt_batch"] == (I, [P, I64, P, I64, I64, I64, I64, P, I64])
    assert S["gdsp_sosfiltfilt_batch_device"] == (I, [P, I64, P, I64, I64, I64, I64, P, I64, P, P])
    assert S["gdsp_sosfilt_fused"] == (I, [P, I64])
    assert S["gdsp_sosfilt_granule"] == (I64, [I64])
    hdr = open(os.path.join(REPO, "include", "gdsp_fft.h")).read()
    assert "GDSP_ALGO_NO_FUSED_SOSFILT = 65536" in hdr
    assert "recursive filters" in hdr.split("---- values")[1].split("---- fft package")[0]
    assert "gdsp_sosfilt_batch" in hdr.split("later_chunks:")[1].split("gdsp_loop_stats(")[0]


def test_no_fused_sosfilt_flag_round_trips(gdsp):
    F = gdsp.fft
    assert F.ALGO_NO_FUSED_SOSFILT == 65536
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(F.ALGO_NO_FUSED_SOSFILT)
        assert F.Algorithm() == 65536
        F.SetAlgorithm(F.ALGO_NO_FUSED_SOSFILT | F.ALGO_NO_FUSED_HILBERT | F.ALGO_NO_FUSED_FIR)
        assert F.Algorithm() == 65536 | 32768 | 512
        for bad in (2048, 16384, 65536 | 16384, 65536 | 2048, 1 << 17, 1 << 20):
            with pytest.raises(gdsp.GDSPError) as e:
                F.SetAlgorithm(bad)
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        assert F.Algorithm() == 65536 | 32768 | 512
    finally:
        F.SetAlgorithm(prev)


def _sec(a1, a2, b=(1.0, 0.5, 0.25)):
    return [b[0], b[1], b[2], 1.0, a1, a2]


def test_fused_query_is_host_arithmetic(gdsp):
    F, G = gdsp.fft, gdsp._lib
    L = G.lib()
    prev = F.Algorithm()
    stable = _sec(-1.2, 0.5)
    try:
        F.SetAlgorithm(prev & ~F.ALGO_NO_FUSED_SOSFILT)
        for S in (1, 2, 7, 8):
            assert F.sosfilt_fused([stable] * S) is True, S
        for name, sos in R.FILTERS.items():
            assert F.sosfilt_fused(sos) is True, name
        assert F.sosfilt_fused([_sec(0.3, 0.0, (1.0, 1.0, 0.0))]) is True      # first order
        assert F.sosfilt_fused([_sec(1.9999, 0.99995)]) is True                # just inside
        # the edge of the triangle and beyond it
        for a1, a2 in ((0.0, 1.0), (0.0, -1.0), (2.0, 1.0), (-1.5, 0.5), (1.5, 0.5), (0.0, 1.01),
                       (-1.0, 0.0), (1.0, 0.0), (0.5, -0.5), (3.0, 0.5), (float("nan"), 0.5)):
            assert F.sosfilt_fused([_sec(a1, a2)]) is False, (a1, a2)
            assert F.sosfilt_fused([stable, _sec(a1, a2), stable]) is False, (a1, a2)
        assert F.sosfilt_fused([[1.0, 0.0, 0.0, 2.0, 0.0, 0.0]]) is False      # a0 != 1
        # S = 0, 9, 65, and a NULL pointer
        assert F.sosfilt_fused(np.zeros((0, 6))) is False
        assert F.sosfilt_fused([stable] * 9) is False
        assert F.sosfilt_fused([stable] * 65) is False
        assert L.gdsp_sosfilt_fused(G._P(), 4) == 0
        assert L.gdsp_sosfilt_fused(G._P(1 << 44), -1) == 0
        F.SetAlgorithm(F.ALGO_NO_FUSED_SOSFILT)
        for S in (1, 8):
            assert F.sosfilt_fused([stable] * S) is False, S
    finally:
        F.SetAlgorithm(prev)


def test_granule_is_a_multiple_of_the_tile(gdsp):
    F = gdsp.fft
    for S in (1, 2, 8, 9, 64):
        G = F.sosfilt_granule(S)
        assert G > 0 and G % R.TILE == 0, S
    for S in (0, -1, 65):
        assert F.sosfilt_granule(S) == 0
    L = gdsp._lib.lib()
    assert L.gdsp_sosfilt_work_doubles(0, 1, 1) == -1
    assert L.gdsp_sosfilt_work_doubles(2, 3, R.TILE + 1) >= 3 * 5 * 4
    assert L.gdsp_sosfiltfilt_work_doubles(2, 3, 100, 15) >= 3 * 130
    assert L.gdsp_sosfiltfilt_work_doubles(2, 3, 100, -1) == -1


def test_zi_and_padlen_follow_their_formulas(gdsp):
    F = gdsp.fft
    for name, sos in R.FILTERS.items():
        want = R.sosfilt_zi(sos)
        got = F.sosfilt_zi(sos)
        assert got.shape == (len(sos), 2)
        # both are long double rounded once, by two routes
        assert np.max(np.abs(got - want.astype(np.float64))) <= 2.0 ** -52 * np.max(np.abs(want)), name
        assert F.sosfiltfilt_padlen(sos) == R.padlen(sos), name
    assert F.sosfiltfilt_padlen(F.butter_sos(3, 0.2)) == 3 * (2 * 2 + 1 - 1)
    assert F.sosfiltfilt_padlen(F.butter_sos(4, 0.2)) == 15
    # the settled step response: a step filtered from zi stays at the gain
    sos = R.FILTERS["butter8_0.2"]
    y, zf = R.seq(sos, np.ones((1, 50)), R.LD, F.sosfilt_zi(sos)[None])
    assert np.max(np.abs(y - y[0, 0])) < 1e-14
    with pytest.raises(gdsp.GDSPError) as e:
        F.sosfilt_zi([[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]])   # a pole at z = 1
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    with pytest.raises(gdsp.GDSPError):
        F.sosfilt_zi([[1.0, 0.0, 0.0, 0.5, 0.0, 0.0]])
    assert F.sosfilt_zi(np.zeros((0, 6))).shape == (0, 2)


def test_zi_and_padlen_agree_with_scipy(gdsp):
    signal = pytest.importorskip("scipy.signal")
    F = gdsp.fft
    for name, sos in R.FILTERS.items():
        want = signal.sosfilt_zi(sos)
        assert np.max(np.abs(F.sosfilt_zi(sos) - want)) <= 1e-9 * np.max(np.abs(want)), name
    x = np.random.default_rng(3).standard_normal((2, 200))
    for name in ("butter8_0.2", "cheby1_8_high"):
        sos = R.FILTERS[name]
        want = signal.sosfiltfilt(sos, x, axis=1)
        assert R.err(R.sosfiltfilt(sos, x), want) < 1e-12, name
        assert R.err(R.sosfiltfilt(sos, x, 40), signal.sosfiltfilt(sos, x, axis=1, padlen=40)) < 1e-12
        assert R.err(R.seq(sos, x)[0], signal.sosfilt(sos, x, axis=1)) < 1e-13, name


def _butter_formula(order, Wn, high):
    """The written formula in long double."""
    LD = R.LD
    w = 2 * np.tan(LD(np.pi) * LD(Wn) / 2)
    secs = []
    if order % 2:
        a0 = 2 + w
        b = [2 / a0, -2 / a0, LD(0)] if high else [w / a0, w / a0, LD(0)]
        secs.append(b + [LD(1), (w - 2) / a0, LD(0)])
    pairs = []
    for k in range(order // 2):
        c = -2 * np.cos(LD(np.pi) * (2 * k + order + 1) / (2 * order)) * w
        a0 = 4 + 2 * c + w * w
        g = 4 / a0 if high else w * w / a0
        pairs.append([g, (-2 if high else 2) * g, g, LD(1), (2 * w * w - 8) / a0,
                      (4 - 2 * c + w * w) / a0])
    pairs.sort(key=lambda q: q[5])
    return np.array(secs + pairs, dtype=LD)


def _response(sos, w):
    z = np.exp(-1j * w)
    h = np.ones_like(z)
    for b0, b1, b2, _, a1, a2 in np.asarray(sos, dtype=np.float64):
        h = h * (b0 + b1 * z + b2 * z * z) / (1 + a1 * z + a2 * z * z)
    return h


def test_butter_sos_follows_its_formula(gdsp):
    F = gdsp.fft
    for order in range(1, 9):
        for Wn in (0.01, 0.2, 0.7):
            for bt in ("low", "high"):
                s = F.butter_sos(order, Wn, bt)
                assert s.shape == ((order + 1) // 2, 6) and s.dtype == np.float64
                want = _butter_formula(order, Wn, bt == "high")
                assert np.max(np.abs(s - want)) <= 8 * 2.0 ** -53 * 2, (order, Wn, bt)
                assert np.all(s[:, 3] == 1.0)
                if order % 2:
                    assert s[0, 2] == 0.0 and s[0, 5] == 0.0
                assert np.all(np.diff(s[order % 2:, 5]) > 0)
                # unit gain per section at DC or at Nyquist, -3 dB at the edge
                sign = np.array([1.0, -1.0, 1.0]) if bt == "high" else np.ones(3)
                gain = (s[:, :3] @ sign) / (s[:, 3:] @ sign)
                assert np.max(np.abs(gain - 1)) < 1e-10, (order, Wn, bt)
                assert abs(abs(_response(s, np.array([np.pi * Wn]))[0]) - 0.5 ** 0.5) < 1e-10
                assert F.sosfilt_fused(s)
    with pytest.raises(ValueError):
        F.butter_sos(4, 0.2, "band")
    for order, Wn in ((0, 0.2), (4, 0.0), (4, 1.0), (4, -0.1)):
        with pytest.raises(gdsp.GDSPError):
            F.butter_sos(order, Wn)


def test_butter_sos_agrees_with_scipy(gdsp):
    signal = pytest.importorskip("scipy.signal")
    F = gdsp.fft
    w = np.linspace(0, np.pi, 512, endpoint=False)
    for order in range(1, 9):
        for Wn in (0.01, 0.2, 0.7):
            for bt in ("low", "high"):
                mine = F.butter_sos(order, Wn, bt)
                ref = signal.butter(order, Wn, bt, output="sos")
                assert np.max(np.abs(mine[:, 3:] - ref[:, 3:])) <= 1e-15, (order, Wn, bt)
                assert np.max(np.abs(_response(mine, w) - _response(ref, w))) <= 1e-12


def _entries(gdsp, kind):
    """Host and device entry behind one signature. kind "filt": (x, ldx, sos,
    S, channels, n, out, ldo); "filtfilt": the same and padlen."""
    L = gdsp._lib.lib()
    null = gdsp._lib._P()
    if kind == "filt":
        return (lambda x, ldx, sos, S, pl, ch, n, out, ldo:
                L.gdsp_sosfilt_batch(x, ldx, sos, S, null, ch, n, out, ldo, null),
                lambda x, ldx, sos, S, pl, ch, n, out, ldo:
                L.gdsp_sosfilt_batch_device(x, ldx, sos, S, null, ch, n, out, ldo, null, null, null))
    return (lambda x, ldx, sos, S, pl, ch, n, out, ldo:
            L.gdsp_sosfiltfilt_batch(x, ldx, sos, S, pl, ch, n, out, ldo),
            lambda x, ldx, sos, S, pl, ch, n, out, ldo:
            L.gdsp_sosfiltfilt_batch_device(x, ldx, sos, S, pl, ch, n, out, ldo, null, null))


@pytest.mark.parametrize("kind", ["filt", "filtfilt"])
def test_status_codes_in_order_before_any_device_call(gdsp, kind):
    G = gdsp._lib
    null = G._P()
    # far apart, unmapped: a call that touched either would fault
    px, po = G._P(1 << 44), G._P(1 << 45)
    good = np.ascontiguousarray(R.FILTERS["butter8_0.2"])
    bad_a0 = good.copy()
    bad_a0[2, 3] = 1.5
    nonfinite = good.copy()
    nonfinite[1, 0] = np.inf
    many = np.ascontiguousarray(np.tile(good[:1], (65, 1)))
    ptr = lambda a: a.ctypes.data_as(G._P)
    for f in _entries(gdsp, kind):
        def call(x=px, ldx=300, sos=good, S=4, pl=-1, ch=3, n=300, out=po, ldo=300):
            return f(x, ldx, ptr(sos) if sos is not None else null, S, pl, ch, n, out, ldo)

        # 1. negative sizes, the strides
        assert call(S=-1) == G.GDSP_ERR_INVALID
        assert call(ch=-1) == G.GDSP_ERR_INVALID
        assert call(n=-1) == G.GDSP_ERR_INVALID
        assert call(ldx=299) == G.GDSP_ERR_INVALID
        assert call(ldo=299) == G.GDSP_ERR_INVALID
        if kind == "filtfilt":
            assert call(pl=-2) == G.GDSP_ERR_INVALID
            assert call(pl=-2, ch=0) == G.GDSP_ERR_INVALID
        # ... before the later ones
        assert call(ch=0, n=-1) == G.GDSP_ERR_INVALID
        assert call(x=null, out=null, sos=None, ldx=1) == G.GDSP_ERR_INVALID
        # 2. no rows: nothing is looked at
        assert call(x=null, out=null, sos=None, ch=0) == G.GDSP_OK
        assert call(ch=0, S=100) == G.GDSP_OK
        # 3. empty input, before the section count and the pointers
        assert call(n=0, ldx=0, ldo=0) == G.GDSP_ERR_EMPTY
        assert call(S=0) == G.GDSP_ERR_EMPTY
        assert call(x=null, out=null, sos=None, n=0, ldx=0, ldo=0, S=65) == G.GDSP_ERR_EMPTY
        # 4. too many sections, before the pointers
        assert call(sos=many, S=65) == G.GDSP_ERR_UNSUPPORTED
        assert call(x=null, sos=None, S=65) == G.GDSP_ERR_UNSUPPORTED
        # 5. a NULL pointer; one row needs no stride
        assert call(x=null) == G.GDSP_ERR_INVALID
        assert call(out=null) == G.GDSP_ERR_INVALID
        assert call(sos=None) == G.GDSP_ERR_INVALID
        assert call(x=null, ch=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID
        # 6. the coefficients
        assert call(sos=bad_a0) == G.GDSP_ERR_INVALID
        assert call(sos=nonfinite) == G.GDSP_ERR_INVALID
        # 7. sosfiltfilt: rows no longer than padlen (the default here is 27)
        if kind == "filtfilt":
            assert call(n=27, ldx=27, ldo=27) == G.GDSP_ERR_INVALID
            assert call(pl=300) == G.GDSP_ERR_INVALID
            assert call(n=5, ldx=5, ldo=5, pl=5) == G.GDSP_ERR_INVALID
        if gdsp.device_count() == 0:
            assert call() == G.GDSP_ERR_NO_DEVICE
            assert call(sos=many, S=64, pl=10) == G.GDSP_ERR_NO_DEVICE
            assert call(ch=1, ldx=0, ldo=0) == G.GDSP_ERR_NO_DEVICE
            if kind == "filtfilt":
                assert call(n=28, ldx=28, ldo=28) == G.GDSP_ERR_NO_DEVICE
                assert call(n=6, ldx=6, ldo=6, pl=5) == G.GDSP_ERR_NO_DEVICE
                assert call(pl=0) == G.GDSP_ERR_NO_DEVICE


def test_device_entries_overlap_rules(gdsp):
    """Arithmetic on the two address ranges, after every other check: fake
    pointers suffice. sosfilt takes out == x exactly; sosfiltfilt nothing."""
    G = gdsp._lib
    L = G.lib()
    null = G._P()
    sos = np.ascontiguousarray(R.FILTERS["butter8_0.2"])
    sp = sos.ctypes.data_as(G._P)
    base = 1 << 44

    def filt(xa, oa, ch=2, n=100, ldx=128, ldo=128):
        return L.gdsp_sosfilt_batch_device(G._P(xa), ldx, sp, 4, null, ch, n, G._P(oa), ldo, null,
                                           null, null)

    def ff(xa, oa, ch=2, n=100, ldx=128, ldo=128):
        return L.gdsp_sosfiltfilt_batch_device(G._P(xa), ldx, sp, 4, -1, ch, n, G._P(oa), ldo, null,
                                               null)

    for f in (filt, ff):
        assert f(base, base + 8 * 50) == G.GDSP_ERR_INVALID        # out starts inside x
        assert f(base + 8 * 50, base) == G.GDSP_ERR_INVALID
        assert f(base, base + 8 * 227) == G.GDSP_ERR_INVALID       # x spans 228 doubles
        assert f(base, base, ldo=130) == G.GDSP_ERR_INVALID        # same start, other stride
        assert f(base, base + 8 * 99, ch=1, ldx=0, ldo=0) == G.GDSP_ERR_INVALID
        assert f(base, base + 8 * 50, ch=0) == G.GDSP_OK           # the earlier checks first
    assert ff(base, base) == G.GDSP_ERR_INVALID
    if gdsp.device_count() == 0:
        assert filt(base, base) == G.GDSP_ERR_NO_DEVICE            # in place: allowed
        assert filt(base, base, ch=1, ldx=0, ldo=0) == G.GDSP_ERR_NO_DEVICE
        assert filt(base, base + 8 * 228) == G.GDSP_ERR_NO_DEVICE
        assert ff(base, base + 8 * 228) == G.GDSP_ERR_NO_DEVICE


def test_python_wrappers_refuse_what_the_library_would(gdsp):
    F = gdsp.fft
    sos = R.FILTERS["butter8_0.2"]
    with pytest.raises(TypeError):
        F.SosFilt(np.ones(8, np.complex128), sos)
    with pytest.raises(TypeError):
        F.SosFiltFiltBatch(np.ones((2, 80), np.complex128), sos)
    with pytest.raises(gdsp.Panic):
        F.SosFiltBatch([np.ones(4), np.ones(5)], sos)
    with pytest.raises(gdsp.GDSPError) as e:
        F.SosFilt(np.zeros(0), sos)
    assert e.value.status == gdsp._lib.GDSP_ERR_EMPTY
    with pytest.raises(gdsp.GDSPError):
        F.SosFiltBatch(np.zeros((2, 8)), sos[:, :5])
    with pytest.raises(gdsp.GDSPError):
        F.SosFiltBatch(np.zeros((2, 8)), sos, zi=np.zeros((2, 3, 2)))
    with pytest.raises(gdsp.GDSPError) as e:
        F.SosFiltFilt(np.zeros(27), sos)
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    assert F.SosFiltBatch(np.zeros((0, 16)), sos).shape == (0, 16)
    assert F.SosFiltFiltBatch(np.zeros((0, 16)), sos).shape == (0, 16)


# ---- the bound, on the CPU ----------------------------------------------------------

@pytest.mark.parametrize("name", R.BOUNDED + [R.ILL])
def test_model_of_the_decomposition_is_within_the_bound(name):
    """tile 4096, E = 16, float64, tables from long double, against the
    long-double recurrence: noise, and noise on a DC of 100."""
    sos = R.FILTERS[name]
    rng = np.random.default_rng(1)
    n = 3 * R.TILE
    x = np.stack([rng.standard_normal(n), rng.standard_normal(n) + 100.0])
    ref, _ = R.seq(sos, x)
    e_seq = R.err(R.seq(sos, x, np.float64)[0], ref)
    for r in range(2):
        e = R.err(R.model(sos, x[r]), ref[r])
        ratio = e / max(e_seq, R.FLOOR)
        print("sos model %s row %d: e_seq %.3g e %.3g ratio %.2f" % (name, r, e_seq, e, ratio))
        if name == R.ILL:
            assert e <= 1e-9
        else:
            assert e <= R.K_BOUND * max(e_seq, R.FLOOR)
