"""GPU checks of the recursive filters (gdsp_sosfilt_batch,
gdsp_sosfiltfilt_batch and their device entries): the time-parallel form and
the plain form, each wherever it serves.

Accuracy: e = max|a - ref| / max|ref| per row against the long-double
recurrence of sos_ref.py. For the six filters of sos_ref.BOUNDED both forms are
held to e <= K max(e_seq, 8 * 2^-53), K = 8, e_seq being the float64 run of the
same recurrence on the same rows; butter12_0.002 is held to 1e-9 and its ratio
printed. The filters of the definition test (butter_sos of orders 2, 3, 8 and
16) are held to the same K. Measured ratios on one MI355X (rows of 3 tiles + 17,
noise and noise on a DC of 100; time-parallel / plain):
  butter8_0.2 0.66 / 0.64, butter6_band 0.92 / 0.71, cheby1_8_high 1.08 / 0.95,
  ellip8_0.05 0.48 / 0.61, butter8_0.01 1.11 / 0.53, butter2_0.001 6.23 / 0.80;
  butter12_0.002 e = 5.0e-12 / 1.4e-12 (ratio 1.55 / 0.43).
butter2_0.001 has both poles at 0.998: a rounding of a state is amplified some
1e4 times (e_seq itself is 1e4 u), and the time-parallel form rounds a thread's
entry state in up to 16 more products (the scan, M^lane, the waves) than the
numpy model of sos_ref.py, which has 3.3.

Shapes: tile = 4096 samples, E = 16 a thread; n = 1, E - 1, tile - 1, tile, tile +
1, 3 tile + 17 and 2 G + 5 reach a lone thread, a partial tile, the scan with
and without a ragged last tile, and zf from pass 2 (n on a tile) and from pass
3's last thread (elsewhere).
"""
import importlib
import os

import numpy as np
import pytest

import sos_ref as R
from conftest import GOLDEN
from guarded import GUARD, NAN, guarded, pad_for

pytestmark = pytest.mark.gpu

TILE, E = R.TILE, R.E
FORMS = ("parallel", "plain")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


class Form:
    """ALGO_NO_FUSED_SOSFILT for the block (form "plain"); the path asserted."""

    def __init__(self, gdsp, form, sos, serves=True):
        self.F, self.plain, self.sos, self.serves = gdsp.fft, form == "plain", sos, serves

    def __enter__(self):
        F = self.F
        self.prev = F.Algorithm()
        F.SetAlgorithm(self.prev | F.ALGO_NO_FUSED_SOSFILT if self.plain
                       else self.prev & ~F.ALGO_NO_FUSED_SOSFILT)
        assert F.sosfilt_fused(self.sos) == (self.serves and not self.plain)

    def __exit__(self, *a):
        self.F.SetAlgorithm(self.prev)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _filt(D, x, sos, zi=None, zf=True):
    """device.sosfilt_batch of host rows: (y, zf) as numpy."""
    import torch
    r = D.sosfilt_batch(_dev(np.atleast_2d(x)), sos, zi=None if zi is None else _dev(zi),
                        return_zf=zf)
    torch.cuda.synchronize()
    return (r[0].cpu().numpy(), r[1].cpu().numpy()) if zf else r.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case_sos(gdsp, case):
    F = gdsp.fft
    return {"S1": F.butter_sos(2, 0.05), "S2_first_order": F.butter_sos(3, 0.2, "high"),
            "S4": F.butter_sos(8, 0.2), "S8": F.butter_sos(16, 0.3)}[case]


_cache: dict = {}


def _rows(n, rows=3, seed=11):
    rng = np.random.default_rng(seed + n)
    x = rng.standard_normal((rows, n))
    x[-1] += 100.0
    return x


def _ref(key, sos, x, zi):
    """(long-double y, zf, e_seq of y, e_seq of zf), once per key."""
    if key not in _cache:
        y, zf = R.seq(sos, x, R.LD, zi)
        y64, zf64 = R.seq(sos, x, np.float64, zi)
        _cache[key] = (y, zf, R.err(y64, y), R.err(zf64.reshape(len(x), -1), zf.reshape(len(x), -1)))
    return _cache[key]


def _bound(e_seq):
    return R.K_BOUND * max(e_seq, R.FLOOR)


@pytest.mark.parametrize("case", ["S1", "S2_first_order", "S4", "S8"])
@pytest.mark.parametrize("form", FORMS)
def test_definition(gdsp, D, form, case):
    sos = _case_sos(gdsp, case)
    S = len(sos)
    assert S == {"S1": 1, "S2_first_order": 2, "S4": 4, "S8": 8}[case]
    if case == "S2_first_order":
        assert sos[0, 2] == 0 and sos[0, 5] == 0
    G = gdsp.fft.sosfilt_granule(S)
    with Form(gdsp, form, sos):
        for n in (1, E - 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 2 * G + 5):
            x = _rows(n)
            # random zi everywhere; zeros (NULL) where a row is one thread, and
            # where pass 2 starts from them
            for with_zi in ((False, True) if n in (1, TILE + 1) else (True,)):
                zi = np.random.default_rng(n).standard_normal((3, S, 2)) if with_zi else None
                y, zf, es, ez = _ref((case, n, with_zi), sos, x, zi)
                got, gzf = _filt(D, x, sos, zi)
                e = R.err(got, y)
                z = R.err(gzf.reshape(3, -1), zf.reshape(3, -1))
                print("sosfilt %s %s n=%d zi=%d: e %.3g (seq %.3g) zf %.3g (seq %.3g)"
                      % (form, case, n, with_zi, e, es, z, ez))
                assert e <= _bound(es), (n, with_zi)
                assert z <= _bound(ez), (n, with_zi)
                # without zf the same samples
                assert _same(_filt(D, x, sos, zi, zf=False), got)


@pytest.mark.parametrize("name", R.BOUNDED + [R.ILL])
def test_accuracy_against_the_sequential_error(gdsp, D, name):
    sos = R.FILTERS[name]
    n = 3 * TILE + 17
    rng = np.random.default_rng(1)
    x = np.stack([rng.standard_normal(n), rng.standard_normal(n) + 100.0])
    y, zf, es, _ = _ref(("acc", name), sos, x, None)
    for form in FORMS:
        with Form(gdsp, form, sos):
            got, _ = _filt(D, x, sos)
        e = R.err(got, y)
        print("sosfilt accuracy %s %s: e_seq %.3g e %.3g ratio %.2f"
              % (name, form, es, e, e / max(es, R.FLOOR)))
        if name == R.ILL:
            assert e <= 1e-9
        else:
            assert e <= _bound(es)


@pytest.mark.parametrize("form", FORMS)
def test_strides_and_guard_bands(gdsp, D, form):
    import torch
    sos = _case_sos(gdsp, "S4")
    S, rows, n, gap = 4, 3, 2 * TILE + 33, 40
    x = _rows(n)
    zi = np.random.default_rng(5).standard_normal((rows, S, 2))
    y, zf, es, ez = _ref(("guard", n), sos, x, zi)
    wide = np.full((rows + 1, n + gap), NAN)      # a guard row and guard columns
    wide[:rows, :n] = x
    xv, xcheck = guarded(_dev(wide), NAN, pad_for(n + gap))
    ov, ocheck = guarded(torch.full((rows + 1, n + gap), GUARD, dtype=torch.float64, device="cuda"),
                         GUARD, pad_for(n + gap))
    need = int(gdsp._lib.lib().gdsp_sosfilt_work_doubles(S, rows, n))
    wv, wcheck = guarded(torch.full((need,), NAN, dtype=torch.float64, device="cuda"), GUARD,
                         pad_for(need, 1))
    with Form(gdsp, form, sos):
        got, gzf = D.sosfilt_batch(xv[:rows, :n], sos, zi=_dev(zi), out=ov[:rows, :n], work=wv,
                                   return_zf=True)
        torch.cuda.synchronize()
    xcheck("x"), ocheck("out"), wcheck("work")
    full = ov.cpu().numpy()
    assert np.all(full[rows] == GUARD) and np.all(full[:, n:] == GUARD), "a store between the rows"
    assert np.array_equal(_bits(xv.cpu().numpy()), _bits(wide))
    assert R.err(full[:rows, :n], y) <= _bound(es)
    assert R.err(gzf.cpu().numpy().reshape(rows, -1), zf.reshape(rows, -1)) <= _bound(ez)
    # the same bits as the dense call with the library's workspace
    with Form(gdsp, form, sos):
        dense, dzf = _filt(D, x, sos, zi)
    assert _same(full[:rows, :n], dense) and _same(gzf.cpu().numpy(), dzf)


@pytest.mark.parametrize("form", FORMS)
def test_in_place_and_refused_overlap(gdsp, D, form):
    import torch
    sos = _case_sos(gdsp, "S4")
    n = 2 * TILE + 5
    x = _rows(n)
    with Form(gdsp, form, sos):
        want, _ = _filt(D, x, sos)
        xd = _dev(x)
        got = D.sosfilt_batch(xd, sos, out=xd)
        torch.cuda.synchronize()
        assert got.data_ptr() == xd.data_ptr()
        assert _same(xd.cpu().numpy(), want)
        buf = torch.zeros(3 * n + 64, dtype=torch.float64, device="cuda")
        a = buf[:3 * n].view(3, n)
        for off in (8, n, 3 * n - 1):
            b = buf[off:off + 3 * n]
            if b.numel() < 3 * n:
                continue
            with pytest.raises(gdsp.GDSPError) as e:
                D.sosfilt_batch(a, sos, out=b.view(3, n))
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
        with pytest.raises(gdsp.GDSPError):
            D.sosfiltfilt_batch(a, sos, out=a)


@pytest.mark.parametrize("form", FORMS)
def test_cuts_in_time(gdsp, D, form):
    sos = _case_sos(gdsp, "S4")
    G = gdsp.fft.sosfilt_granule(4)
    n = 3 * G + 100
    x = _rows(n)
    zi = np.random.default_rng(9).standard_normal((3, 4, 2))
    with Form(gdsp, form, sos):
        whole, zf = _filt(D, x, sos, zi)
        for k in (1, 2):
            a, za = _filt(D, x[:, :k * G], sos, zi)
            b, zb = _filt(D, x[:, k * G:], sos, za)
            assert _same(np.concatenate([a, b], axis=1), whole), k
            assert _same(zb, zf), k
        # three pieces chained by zf -> zi
        a, za = _filt(D, x[:, :G], sos, zi)
        b, zb = _filt(D, x[:, G:3 * G], sos, za)
        c, zc = _filt(D, x[:, 3 * G:], sos, zb)
        assert _same(np.concatenate([a, b, c], axis=1), whole) and _same(zc, zf)
        # a cut off the granule: the same filter, equal within the bound
        y, _, es, _ = _ref(("cuts", n), sos, x, zi)
        a, za = _filt(D, x[:, :G + 7], sos, zi)
        b, zb = _filt(D, x[:, G + 7:], sos, za)
        assert R.err(np.concatenate([a, b], axis=1), y) <= _bound(es)
        if form == "plain":   # sample by sample: every cut is exact
            assert _same(np.concatenate([a, b], axis=1), whole) and _same(zb, zf)


@pytest.mark.parametrize("form", FORMS)
def test_rows_alone(gdsp, D, form):
    sos = _case_sos(gdsp, "S8")
    n = 2 * TILE + 100
    x = _rows(n, rows=5)
    x[1] *= 1e-6
    x[3] = 0.0
    zi = np.random.default_rng(2).standard_normal((5, 8, 2))
    zi[3] = 0.0
    with Form(gdsp, form, sos):
        got, zf = _filt(D, x, sos, zi)
        for r in range(5):
            one, z1 = _filt(D, x[r:r + 1], sos, zi[r:r + 1])
            assert _same(one[0], got[r]) and _same(z1[0], zf[r]), r
    assert np.all(_bits(got[3]) == 0) and np.all(_bits(zf[3]) == 0)   # exact +0.0


@pytest.mark.parametrize("form", FORMS)
def test_scaling_zeros_and_stale_buffers(gdsp, D, form):
    import torch
    sos = _case_sos(gdsp, "S4")
    S, n = 4, 2 * TILE + 77
    x = _rows(n)
    zi = np.random.default_rng(4).standard_normal((3, S, 2))
    need = int(gdsp._lib.lib().gdsp_sosfilt_work_doubles(S, 3, n))
    with Form(gdsp, form, sos):
        base, zf = _filt(D, x, sos, zi)
        for k in (-40, 3, 200):
            s = 2.0 ** k
            got, gz = _filt(D, x * s, sos, zi * s)
            assert _same(got, base * s) and _same(gz, zf * s), k
        z, zz = _filt(D, np.zeros((3, n)), sos)
        assert np.all(_bits(z) == 0) and np.all(_bits(zz) == 0)
        for fill in (NAN, 1e300, GUARD):
            out = torch.full((3, n), fill, dtype=torch.float64, device="cuda")
            work = torch.full((need,), fill, dtype=torch.float64, device="cuda")
            D.sosfilt_batch(_dev(x), sos, zi=_dev(zi), out=out, work=work)
            torch.cuda.synchronize()
            assert _same(out.cpu().numpy(), base), fill
        ff = D.sosfiltfilt_batch(_dev(x), sos).cpu().numpy()
        needf = int(gdsp._lib.lib().gdsp_sosfiltfilt_work_doubles(S, 3, n, R.padlen(sos)))
        out = torch.full((3, n), NAN, dtype=torch.float64, device="cuda")
        work = torch.full((needf,), NAN, dtype=torch.float64, device="cuda")
        D.sosfiltfilt_batch(_dev(x), sos, out=out, work=work)
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), ff)
        assert _same(D.sosfiltfilt_batch(_dev(x * 8.0), sos).cpu().numpy(), ff * 8.0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("form", FORMS)
def test_non_finite_sample(gdsp, D, form, bad):
    sos = R.FILTERS["cheby1_8_high"]          # every coefficient non-zero
    assert np.all(sos != 0)
    n = 3 * TILE + 17
    j = n // 3                                # inside the middle tile
    assert TILE < j < 2 * TILE
    x = _rows(n)
    with Form(gdsp, form, sos):
        clean, czf = _filt(D, x, sos)
        xb = x.copy()
        xb[1, j] = bad
        got, zf = _filt(D, xb, sos)
    assert _same(got[0], clean[0]) and _same(got[2], clean[2])
    assert _same(zf[0], czf[0]) and _same(zf[2], czf[2])
    assert _same(got[1, :j], clean[1, :j])
    assert not np.any(np.isfinite(got[1, j:]))
    assert not np.any(np.isfinite(zf[1]))


@pytest.mark.parametrize("case", ["S2_first_order", "S4"])
@pytest.mark.parametrize("form", FORMS)
def test_sosfiltfilt(gdsp, D, form, case):
    import torch
    sos = _case_sos(gdsp, case)
    pl = R.padlen(sos)
    assert gdsp.fft.sosfiltfilt_padlen(sos) == pl
    with Form(gdsp, form, sos):
        for n in (pl + 1, TILE, 2 * TILE + 3):
            x = _rows(n, rows=3)
            for padlen in (None, 7, 0):
                if padlen is not None and n == TILE:
                    continue
                key = ("ff", case, n, padlen)
                if key not in _cache:
                    ref = R.sosfiltfilt(sos, x, padlen)
                    _cache[key] = (ref, R.err(R.sosfiltfilt(sos, x, padlen, np.float64), ref))
                ref, es = _cache[key]
                got = D.sosfiltfilt_batch(_dev(x), sos, padlen=padlen).cpu().numpy()
                e = R.err(got, ref)
                print("sosfiltfilt %s %s n=%d padlen=%s: e %.3g (seq %.3g)"
                      % (form, case, n, padlen, e, es))
                assert e <= _bound(es), (n, padlen)
                for r in range(3):   # rows alone
                    one = D.sosfiltfilt_batch(_dev(x[r:r + 1]), sos, padlen=padlen).cpu().numpy()
                    assert _same(one[0], got[r])
                if n == 2 * TILE + 3 and padlen is None:
                    xb = x.copy()
                    xb[1, n // 2] = NAN
                    b = D.sosfiltfilt_batch(_dev(xb), sos).cpu().numpy()
                    assert not np.any(np.isfinite(b[1]))
                    assert _same(b[0], got[0]) and _same(b[2], got[2])
                    # the host entry: the same bits
                    assert _same(gdsp.fft.SosFiltFiltBatch(x, sos), got)
        # refused sizes
        for n, padlen in ((pl, None), (5, 5), (3, 7)):
            with pytest.raises(gdsp.GDSPError) as e:
                D.sosfiltfilt_batch(torch.zeros((2, n), dtype=torch.float64, device="cuda"), sos,
                                    padlen=padlen)
            assert e.value.status == gdsp._lib.GDSP_ERR_INVALID


def test_sosfiltfilt_agrees_with_scipy(gdsp, D):
    signal = pytest.importorskip("scipy.signal")
    sos = _case_sos(gdsp, "S4")
    x = _rows(2 * TILE + 3)
    got = D.sosfiltfilt_batch(_dev(x), sos).cpu().numpy()
    assert R.err(got, signal.sosfiltfilt(sos, x, axis=1)) < 1e-11
    y, zf = _filt(D, x, sos)
    assert R.err(y, signal.sosfilt(sos, x, axis=1)) < 1e-12


def test_nine_sections_take_the_plain_form(gdsp, D):
    F = gdsp.fft
    sos = F.butter_sos(18, 0.3)
    assert len(sos) == 9 and not F.sosfilt_fused(sos) and F.sosfilt_fused(sos[:8])
    n = TILE + 50
    x = _rows(n)
    zi = np.random.default_rng(6).standard_normal((3, 9, 2))
    y, zf, es, ez = _ref(("S9", n), sos, x, zi)
    got, gzf = _filt(D, x, sos, zi)
    assert R.err(got, y) <= _bound(es)
    assert R.err(gzf.reshape(3, -1), zf.reshape(3, -1)) <= _bound(ez)
    with Form(gdsp, "plain", sos, serves=False):
        again, _ = _filt(D, x, sos, zi)
    assert _same(again, got)


def test_unstable_section_takes_the_plain_form(gdsp, D):
    F = gdsp.fft
    sos = np.array(F.butter_sos(4, 0.2))
    sos[1, 5] = 1.01
    assert not F.sosfilt_fused(sos)
    n = TILE + 50
    x = _rows(n)
    y, zf, es, _ = _ref(("unstable", n), sos, x, None)
    assert np.all(np.isfinite(y.astype(np.float64)))      # grows, and stays in range here
    got, _ = _filt(D, x, sos)
    assert np.all(np.isfinite(got))
    assert R.err(got, y) <= _bound(es)


def test_host_chunk_loop(gdsp, D):
    """One row of 2^25 + 1000 samples: the host entry cuts it once, at a
    multiple of the granule; a device call on the whole row does not cut."""
    import torch
    F = gdsp.fft
    sos = F.butter_sos(4, 0.1)
    n = (1 << 25) + 1000
    x = np.random.default_rng(8).standard_normal((1, n))
    before = F.LoopStats()["later_chunks"]
    host, hzf = F.SosFiltBatch(x, sos, return_zf=True)
    assert F.LoopStats()["later_chunks"] == before + 1
    dev, dzf = D.sosfilt_batch(_dev(x), sos, return_zf=True)
    torch.cuda.synchronize()
    dev = dev.cpu().numpy()
    cut = 1 << 25
    assert _same(host[:, cut - 2 * TILE:cut + 1000], dev[:, cut - 2 * TILE:cut + 1000])
    assert _same(host, dev) and _same(hzf, dzf.cpu().numpy())
    # the start of the row against the reference
    m = 2 * TILE
    y, _ = R.seq(sos, x[:, :m])
    assert R.err(host[:, :m], y) <= _bound(R.err(R.seq(sos, x[:, :m], np.float64)[0], y))


def test_wav_iir_filter_channels(gdsp):
    W, F = gdsp.wav, gdsp.fft
    sos = F.butter_sos(6, 0.25)
    path = os.path.join(GOLDEN, "wav", "small.wav")
    with open(path, "rb") as f:
        w = W.New(f)
        C = w.NumChannels
        frames = min(w.Samples // C, 5000)
        dec = w.ReadFloats(frames * C).astype(np.float64)
    chans = np.stack([dec[c::C] for c in range(C)])
    with open(path, "rb") as f:
        got = W.IIRFilterChannels(W.New(f), frames, sos)
    assert got.shape == (C, frames)
    assert _same(got, F.SosFiltBatch(chans, sos))
    with open(path, "rb") as f:
        got = W.IIRFilterChannels(W.New(f), frames, sos, zero_phase=True)
    assert _same(got, F.SosFiltFiltBatch(chans, sos))
