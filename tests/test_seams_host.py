"""The instruments of test_seams_gpu.py, proved on the CPU: its Welch reference
against exact_dft.exact_pwelch, the sensitivity of its bound to one segment in
the largest count it uses, and the arithmetic of its shapes against the rules
they restate."""
import numpy as np
import pytest

import exact_dft as E
import seams as S
from conftest import row_nrel


@pytest.mark.parametrize("nfft,stride,pad,nseg", [(64, 3, 0, 41), (48, 24, 64, 9),
                                                  (100, 1, 256, 33)])
def test_reference_is_pwelch(nfft, stride, pad, nseg):
    """welch_sums over [0, N), finalised as gdsp_pwelch_finalize does, is
    exact_pwelch of the same signal to 1e-15."""
    flen, padv = max(pad, nfft), pad or nfft
    x = S.noise([nfft, stride, flen], S.signal_len(nseg, nfft, stride))
    assert E.segment_count(len(x), nfft, nfft - stride) == nseg
    win, wn = S.hamming(flen), S.hamming(nfft)
    total = S.welch_sums(x, nfft, flen, stride, 0, nseg, win)
    mine = S.finalize(total, nseg, nfft, padv, wn, 48000.0)
    ex = E.exact_pwelch(x, 48000.0, nfft, padv, nfft - stride, win, wn)
    err = row_nrel(mine.astype(np.float64), ex.astype(np.float64))
    print("seams reference %d/%d/%d: %.3g" % (nfft, stride, pad, err))
    assert err < 1e-15
    # a range is the difference of two prefixes
    part = S.welch_sums(x, nfft, flen, stride, 3, nseg - 2, win)
    rest = S.welch_sums(x, nfft, flen, stride, 0, 3, win) + \
        S.welch_sums(x, nfft, flen, stride, nseg - 2, nseg, win)
    assert row_nrel((part + rest).astype(np.float64), total.astype(np.float64)) < 1e-15


def test_cross_sums_are_welch_sums():
    """Planes 0 and 1 are welch_sums of x and y; Sxy of x with itself is Sxx."""
    x, y = S.noise(1, 500), S.noise(2, 500)
    win = S.hamming(64)
    c = S.cross_sums(x, y, 60, 64, 7, 1, 60, win)
    assert np.array_equal(c[0], S.welch_sums(x, 60, 64, 7, 1, 60, win))
    assert np.array_equal(c[1], S.welch_sums(y, 60, 64, 7, 1, 60, win))
    d = S.cross_sums(x, x, 60, 64, 7, 1, 60, win)
    assert np.array_equal(d[2], d[0]) and not d[3].any()
    # conj(X) Y: y = x delayed by one sample turns bin j by exp(-2 pi i j / F)
    z = S.cross_sums(x[1:], x[:-1], 64, 64, 64, 0, 7, np.ones(64))
    ang = np.angle((z[2] + 1j * z[3]).astype(np.complex128)[1:8])
    assert np.all(ang < 0)


def test_one_segment_in_the_largest_count_fails_the_bound():
    """Dropping or repeating one segment of the largest count the GPU tests
    use moves the sums by about 1 / nseg: seven orders above the 1e-13 they
    are held to. Asserted, so that neither the bound nor the counts can be
    changed into a check that one lost pair would pass."""
    m = max(S.MATERIALISED, key=lambda m: m.nseg)
    assert m.nseg == S.LARGEST_NSEG and m.nseg > 8_000_000
    stride = m.nfft - m.nov
    x = S.noise(m.nseg, S.signal_len(m.nseg, m.nfft, stride))
    win = S.hamming(m.nfft)
    total = S.welch_sums(x, m.nfft, m.nfft, stride, 0, m.nseg, win)
    ref = S.unfold(total, m.nfft).astype(np.float64)
    worst = np.inf
    for s in (0, m.nseg // 2, m.nseg - 1):
        one = S.welch_sums(x, m.nfft, m.nfft, stride, s, s + 1, win)
        for changed in (total - one, total + one):
            d = row_nrel(S.unfold(changed, m.nfft).astype(np.float64), ref)
            worst = min(worst, d)
    print("seams: one segment of %d moves the sums by >= %.3g" % (m.nseg, worst))
    assert worst > 1e4 * S.EXACT
    assert S.EXACT == 1e-13


def test_shapes_cross_their_seams():
    """pair_workers, pwelch_wave_geometry and the materialised chunk rule
    (welch.hip, pwelch_wave.hip), restated, on the shapes of the GPU tests."""
    for c in S.worker_cases():
        if c.tpw is None:
            continue
        nseg = S.worker_nseg(c.tpw)
        npairs, target = (nseg + 1) // 2, S.WMUL * c.tpw
        ppw = -(-npairs // min(target, npairs))
        nworkers = -(-npairs // ppw)
        assert nseg % 2 == 1 and ppw == 2 and npairs - (nworkers - 1) * ppw == 1, c
    for f in (64, 2048):
        s, target = S.wave_groups(f)
        nseg = S.wave_nseg(f)
        ngroups = -(-((nseg + 1) // 2) // s)
        assert nseg % 2 == 1 and ngroups == target + 1 and -(-ngroups // target) == 2
    assert S.wave_groups(64) == (16, 2048) and S.wave_groups(2048) == (1, 1024)
    for m in S.MATERIALISED:
        npairs = (m.nseg + 1) // 2
        rows = S.materialised_rows(max(m.pad, m.nfft), npairs)
        assert m.nseg % 2 == 1 and rows < npairs <= rows + 2, m
    assert S.materialised_rows(8, 1 << 30) == 65535 * 64
    assert [S.pow2_tpw(f) for f in (16, 32, 4096, 8192, 16384)] == [256, 128, 1, 1, 1]


def test_loop_stats_readable_without_gpu(gdsp):
    """gdsp_loop_stats reads host counters: no device call, any pointer NULL,
    and they never run backwards."""
    L = gdsp._lib
    a = gdsp.fft.LoopStats()
    assert set(a) == {"later_chunks", "multi_unit_launches"} and min(a.values()) >= 0
    v = L._I64(-1)
    assert L.lib().gdsp_loop_stats(None, None) == L.GDSP_OK
    assert L.lib().gdsp_loop_stats(v, None) == L.GDSP_OK and v.value >= a["later_chunks"]
    assert L.lib().gdsp_loop_stats(None, v) == L.GDSP_OK and v.value >= a["multi_unit_launches"]


def test_segments_view():
    x = np.arange(20.0)
    v = S.segments(x, 4, 3, 1, 5)
    assert v.shape == (4, 4) and np.array_equal(v[0], [3, 4, 5, 6]) and v[3, 3] == 15
    with pytest.raises(AssertionError):
        S.segments(x, 4, 3, 0, 7)  # segment 6 ends at sample 22
    acc = np.arange(8.0)
    assert np.array_equal(S.fold(acc), 0.5 * (acc + acc[[0, 7, 6, 5, 4, 3, 2, 1]]))
    assert np.array_equal(S.unfold(np.arange(5.0), 8), [0, 1, 2, 3, 4, 3, 2, 1])
