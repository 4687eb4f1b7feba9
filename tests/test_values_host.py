"""CPU proof of what test_values_gpu.py relies on (values.py).

The float64 numpy model of every case (numpy.fft, ifft(fft * fft),
numpy.convolve, the numpy Welch and Cpsd models) is itself exactly equivariant
under the powers of 2 of test B, on the very inputs of the GPU test, and never
produces a subnormal or a non-finite value there: bit equality is a fair demand
of arithmetic without absolute thresholds, and the exponents leave the normal
range nowhere. And every checker rejects a planted fault: a stale finite addend
(A and B), a flush of small values to zero (B), a finite row for a NaN input
and a NaN in a neighbouring row (C).
"""
import numpy as np
import pytest

import values as V

IDS = [c.ident() for c in V.CASES]


def test_every_entry_has_a_case():
    assert {c.entry for c in V.CASES} == set(V.COVERAGE)
    assert len(set(IDS)) == len(IDS)
    assert {c.c.path for c in V.CASES if isinstance(c, V.PwelchAccumulate)} == set(V.SR.PATHS)


def _model(case, size):
    return lambda inputs, fill: case.model(inputs, size)


@pytest.mark.parametrize("case", V.CASES, ids=IDS)
def test_model_is_exactly_equivariant(case):
    for size in case.sizes:
        V.check_equivariant(_model(case, size), case.clean(size), case.scalings,
                            "%s %s" % (case.ident(), size), normal=True)


@pytest.mark.parametrize("case", V.CASES, ids=IDS)
def test_poison_is_larger_and_masks_are_sound(case):
    """The NaN call of A is at least as large in every dimension; the masks of
    C fit the outputs, never overlap, and leave the bad sample in the inputs."""
    for size in case.sizes:
        clean, (poison, _) = case.clean(size), case.poison(size)
        for p, c in zip(poison, clean):
            assert np.isnan(p).all() and p.ndim == c.ndim
            assert all(a >= b for a, b in zip(p.shape, c.shape))
    size = case.sizes[-1]
    clean = case.clean(size)
    outs = case.model(clean, size)
    runs = list(case.bad_runs(size))
    assert {label.split()[0] for label, _, _, _ in runs} == {"nan", "inf"}
    for label, inputs, masks, both in runs:
        # one finite sample became non-finite, nothing else moved (a Pwelch
        # range's own NaN samples outside the range stay)
        assert sum(int((np.isfinite(b) & ~np.isfinite(a)).sum())
                   for a, b in zip(inputs, clean)) == 1, label
        assert sum(int((np.isfinite(b) & (a != b)).sum())
                   for a, b in zip(inputs, clean)) == 1, label
        assert len(masks) == len(outs)
        for (bad, keep), o in zip(masks, outs):
            for m in (bad, keep):
                assert m is None or np.broadcast_to(m, o.shape).shape == o.shape
            if bad is not None and keep is not None:
                assert not (bad & keep).any(), label
        assert any(bad is not None for bad, _ in masks), label


# ---- planted faults ---------------------------------------------------------------------

def _first(cls, **kw):
    return next(c for c in V.CASES if isinstance(c, cls)
                and all(getattr(c, k) == v for k, v in kw.items()))


CONTROLS = [_first(V.Transform, variant="forward"), _first(V.Transform, variant="real"),
            _first(V.Convolve), _first(V.Fir), _first(V.Nd, entry="fft2"),
            _first(V.Nd, entry="fft_axis"), _first(V.PwelchAccumulate), _first(V.PwelchBatch),
            _first(V.Cpsd, one=False), _first(V.Cpsd, one=True)]
CIDS = [c.ident() for c in CONTROLS]


class Stale:
    """An engine that adds what its previous call left behind (a finite value)
    to one output element."""

    def __init__(self, case, size):
        self.case, self.size, self.left = case, size, 0.0

    def __call__(self, inputs, fill):
        outs = [np.array(o) for o in self.case.model(inputs, self.size)]
        outs[0].flat[outs[0].size // 2] += self.left
        self.left = 1e-9
        return tuple(outs)


def _flushing(case, size):
    """An engine with an absolute threshold: |v| < 1e-30 is zero, on the way in
    and on the way out."""
    def flush(a):
        a = np.array(a)
        v = a.view(np.float64) if np.iscomplexobj(a) else a
        v[np.abs(v) < 1e-30] = 0.0
        return a
    return lambda inputs, fill: tuple(flush(o) for o in case.model(
        tuple(flush(np.ascontiguousarray(x)) for x in inputs), size))


@pytest.mark.parametrize("case", CONTROLS, ids=CIDS)
def test_control_stale_value_fails_history_and_equivariance(case):
    size = case.sizes[-1]
    clean = case.clean(size)
    V.check_history(_model(case, size), clean, clean, case.ident())  # the honest engine passes
    with pytest.raises(AssertionError, match="changed after the NaN call"):
        V.check_history(Stale(case, size), clean, clean, case.ident())
    with pytest.raises(AssertionError, match="differs from the unscaled run"):
        V.check_equivariant(Stale(case, size), clean, case.scalings, case.ident())


@pytest.mark.parametrize("case", CONTROLS, ids=CIDS)
def test_control_flush_to_zero_fails_equivariance(case):
    size = case.sizes[-1]
    with pytest.raises(AssertionError, match="differs from the unscaled run"):
        V.check_equivariant(_flushing(case, size), case.clean(size), case.scalings, case.ident())


@pytest.mark.parametrize("case", CONTROLS, ids=CIDS)
def test_control_containment(case):
    """An ideal engine (the clean result, non-finite exactly under the bad
    masks) passes; one that hands back the clean, finite values for the
    poisoned part fails, and so does one with a NaN outside it."""
    size = case.sizes[-1]
    clean = case.model(case.clean(size), size)
    for label, _, masks, both in case.bad_runs(size):
        ideal = []
        for o, (bad, _) in zip(clean, masks):
            o = np.array(o)
            if bad is not None:
                o[np.broadcast_to(bad, o.shape)] = complex(V.NAN, V.NAN) if np.iscomplexobj(o) \
                    else V.NAN
            ideal.append(o)
        V.check_contained(ideal, clean, masks, label, both)
        with pytest.raises(AssertionError, match="came out"):
            V.check_contained(clean, clean, masks, label, both)
        if both:  # NaN in one part only is not enough for a complex NaN input
            half = [np.array(o) for o in ideal]
            i = next(i for i, (bad, _) in enumerate(masks) if bad is not None)
            half[i][np.broadcast_to(masks[i][0], half[i].shape)] = complex(V.NAN, 0.0)
            with pytest.raises(AssertionError, match="not NaN"):
                V.check_contained(half, clean, masks, label, both)
        kept = [i for i, (_, keep) in enumerate(masks) if keep is not None and keep.any()]
        if kept:
            leak = [np.array(o) for o in ideal]
            where = np.argwhere(np.broadcast_to(masks[kept[0]][1], leak[kept[0]].shape))[0]
            leak[kept[0]][tuple(where)] = V.NAN
            with pytest.raises(AssertionError, match="outside the poisoned part changed"):
                V.check_contained(leak, clean, masks, label, both)


def test_ldexp_is_exact_on_both_parts():
    z = np.array([1.5 - 0.75j, 3e-5 + 7j])
    assert np.array_equal(V.ldexp(z, 10), z * 1024) and np.array_equal(V.ldexp(z, 0), z)
    assert np.array_equal(V.ldexp(V.ldexp(z, -200), 200), z)
    with pytest.raises(AssertionError, match="subnormal"):
        V.assert_normal((np.array([1.0, 1e-310]),), "x")
    with pytest.raises(AssertionError, match="not finite"):
        V.assert_normal((np.array([1.0, V.INF]),), "x")
