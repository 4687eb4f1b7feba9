"""The instruments of test_segment_ranges_gpu.py and test_guard_bands_gpu.py,
proved on the CPU (no GPU needed): the range-sum reference against
exact_dft.exact_pwelch, controls that an off-by-one range or a read of a
poisoned sample cannot pass, and the guard-band checker."""
import numpy as np
import pytest

import exact_dft as E
import test_segment_ranges_gpu as R
from conftest import row_nrel
from guarded import GUARD, NAN, guarded, pad_for

# the 80-bit reference of every case is computed here as on the GPU machine;
# the longest (32768 x 5, 16384 x 7) take about a second each
CASES = R.CASES


def _hamming(n):
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / (n - 1))


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_range_reference_is_pwelch(c):
    """The reference over [0, N), finalised as gdsp_pwelch_finalize does,
    is exact_pwelch of the same signal to 1e-15."""
    x, n, f = R.signal(c), R.nsegs(c), R.flen(c)
    pad = c.pad or c.nfft
    lp = pad // 2 + 1
    total = R.powers(c).sum(axis=0)  # extended
    j = np.arange(lp)
    w = _hamming(c.nfft).astype(E.LD)
    norm = (w * w).sum() * E.LD(48000.0)
    cj = np.where((j > 0) & (j < lp - 1), 2, 1).astype(E.LD)
    mine = cj * (total[j] + total[(f - j) % f]) / E.LD(2) / E.LD(n) / norm
    ex = E.exact_pwelch(x, 48000.0, c.nfft, pad, c.nov, R.window(c), _hamming(c.nfft))
    err = row_nrel(mine.astype(np.float64), ex.astype(np.float64))
    print("reference %s: %.3g" % (R.case_id(c), err))
    assert err < 1e-15
    # and the float64 the GPU test compares with is that sum, rounded once
    assert np.array_equal(R.reference(c, 0, n), total.astype(np.float64))


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_control_off_by_one_range_fails(c):
    """[a + 1, b + 1) and [a, b - 1) differ from [a, b) by more than 1e-3: a
    kernel that is one segment off cannot pass 1e-13."""
    a, b = 1, R.nsegs(c) - 1
    ref = R.reference(c, a, b)
    for a2, b2 in ((a + 1, b + 1), (a, b - 1)):
        d = row_nrel(R.reference(c, a2, b2), ref)
        assert d > 1e-3, (R.case_id(c), a2, b2, d)


@pytest.mark.parametrize("c", [c for c in CASES if R.flen(c) <= 4096], ids=R.case_id)
def test_control_poisoned_signal(c):
    """The poisoned signal leaves the reference of its range finite and
    unchanged; one segment further and it is not."""
    x = R.signal(c)
    for a, b in R.ranges(c):
        p = R.segment_powers(c, R.poisoned(c, x, a, b), a, b)
        assert np.isfinite(p).all()
        assert np.array_equal(p, R.powers(c)[a:b])
    a, b = 2, 2 + R.group(c) + 1
    y = R.poisoned(c, x, a, b)
    assert not np.isfinite(R.segment_powers(c, y, a, b + 1)).all()
    assert not np.isfinite(R.segment_powers(c, y, a - 1, b)).all()
    assert np.isnan(R.poisoned(c, x, 2, 2)).all()


def test_ranges_and_splits():
    for c in CASES:
        n, g = R.nsegs(c), R.group(c)
        assert n == (5 if R.flen(c) == 32768 else 2 * g + 3)
        rs = R.ranges(c)
        assert all(0 <= a < b <= n for a, b in rs) and rs[0] == (0, n)
        assert rs[2][0] % 2 == 1 and (rs[2][1] - rs[2][0]) % 2 == 0  # odd start, even count
        assert sorted(k % 2 for k in R.splits(c)) == [0, 1]
        assert all(0 < k < n for k in R.splits(c))


def test_fold():
    acc = np.arange(8.0)
    assert np.array_equal(R.fold(acc), 0.5 * (acc + acc[[0, 7, 6, 5, 4, 3, 2, 1]]))


@pytest.mark.parametrize("complex_", [False, True], ids=["float64", "complex128"])
@pytest.mark.parametrize("fill", [GUARD, NAN], ids=["sentinel", "nan"])
def test_guard_checker_reports_one_changed_element(fill, complex_):
    import torch
    dtype = torch.complex128 if complex_ else torch.float64
    payload = torch.arange(15, dtype=torch.float64).reshape(3, 5).to(dtype)
    pad = pad_for(5)
    assert pad % 32 == 0 and pad >= 1024
    view, check = guarded(payload, fill, pad)
    assert view.shape == payload.shape and torch.equal(view, payload)
    base = view.untyped_storage()
    assert base.nbytes() == (2 * pad + 15) * payload.element_size()
    assert view.data_ptr() - base.data_ptr() == pad * payload.element_size()
    check()
    view.mul_(2)  # writing the payload is no violation
    check()
    flat = torch.empty(0, dtype=dtype).set_(base)
    for at in (0, pad - 1, pad + 15, 2 * pad + 14):
        old = flat[at].clone()
        flat[at] = 1.0 if at % 2 else fill + 1  # (NaN + 1: another value only for the sentinel)
        if fill != fill and not at % 2:
            flat[at] = 0.0
        with pytest.raises(AssertionError, match="1 pad element"):
            check()
        flat[at] = old
        check()
    if complex_:  # the imaginary part alone
        torch.view_as_real(flat)[pad + 15, 1] = 3.0
        with pytest.raises(AssertionError):
            check()
