"""Scaling, non-finite samples and stale state in every kernel family (values.py
has the cases and the checkers, test_values_host.py proves both on the CPU).

  A  test_history       a clean call before and after a larger all-NaN call of
                        the same entry, every caller buffer full of NaN: the
                        same bits
  B  test_equivariance  inputs times 2^k: outputs times the matching power of
                        2, bit for bit; the coherence unchanged
  C  test_containment   one NaN / +Inf sample: its row, channel or FIR blocks
                        non-finite, every other output bit for bit
     test_zeros         all-zero inputs: exact zeros (the coherence NaN)
  D  test_cpsd_extremes the ends of the Cpsd balance against the 80-bit reference
  E  test_fir_locality  FIR rows whose level alternates by 2^40 from block to
                        block, per output against an extended-precision direct
                        convolution, bounded by 16 times the error of a float64
                        numpy model of the same paired overlap-save

Every case asserts its path before it runs (Case.setup: the plan kind, the
fused / composed queries, test_segment_ranges_gpu._assert_path).
"""
import importlib

import numpy as np
import pytest

import exact_dft as E
import values as V
from conftest import row_nrel
from test_accuracy_gpu import algorithm

pytestmark = pytest.mark.gpu

EXACT = 1e-13  # test_cpsd_gpu.py's bar, engine against the exact reference here
IDS = [c.ident() for c in V.CASES]
CP_NAMES = ("Pxy", "Pxx", "Pyy", "Cxy")


@pytest.fixture(scope="module")
def env(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")
    return V.environment(gdsp, importlib.import_module("go-dsp_amd.device"))


def test_every_entry_has_a_case():
    """A, B, C and the zero test run every case of the one table, and every
    case asserts its path (Pwelch: _assert_path) before it runs."""
    assert {c.entry for c in V.CASES} == set(V.COVERAGE)
    assert len(set(IDS)) == len(IDS)
    for c in V.CASES:
        assert c.scalings and c.sizes, c.ident()
        assert any(True for _ in c.bad_runs(c.sizes[-1])), c.ident()


def _runner(env, case, size):
    return lambda inputs, fill, size=size: case.run(env, inputs, fill, size)


@pytest.mark.parametrize("case", V.CASES, ids=IDS)
def test_history(env, case):
    with algorithm(env.gdsp, case.flags):
        case.setup(env)
        for size in case.sizes:
            poison, psize = case.poison(size)
            clean = case.clean(size)
            for p, c in zip(poison, clean):
                assert np.isnan(p).all() and p.ndim == c.ndim
                assert all(a >= b for a, b in zip(p.shape, c.shape)), (p.shape, c.shape)

            def run(inputs, fill, poisoned=poison, size=size, psize=psize):
                return case.run(env, inputs, fill, psize if inputs is poisoned else size)

            V.check_history(run, clean, poison, "%s %s" % (case.ident(), size))


@pytest.mark.parametrize("case", V.CASES, ids=IDS)
def test_equivariance(env, case):
    with algorithm(env.gdsp, case.flags):
        case.setup(env)
        for size in case.sizes:
            V.check_equivariant(_runner(env, case, size), case.clean(size), case.scalings,
                                "%s %s" % (case.ident(), size))


@pytest.mark.parametrize("case", V.CASES, ids=IDS)
def test_containment(env, case):
    size = case.sizes[-1]
    fails = []
    with algorithm(env.gdsp, case.flags):
        case.setup(env)
        clean = case.run(env, case.clean(size), 0.0, size)
        for label, inputs, masks, both in case.bad_runs(size):
            got = case.run(env, inputs, 0.0, size)
            try:
                V.check_contained(got, clean, masks, "%s %s" % (case.ident(), label), both)
            except AssertionError as e:
                fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", V.CASES, ids=IDS)
def test_zeros(env, case):
    with algorithm(env.gdsp, case.flags):
        case.setup(env)
        for size in case.sizes:
            outs = case.run(env, case.zeros(size), V.NAN, size)
            for i, a in enumerate(outs):
                if i in case.coherence:
                    assert np.isnan(a).all(), "%s: a coherence of no power" % case.ident()
                else:
                    assert not np.any(a), "%s %s: output %d of zero input: %d nonzero" \
                        % (case.ident(), size, i, int(np.count_nonzero(a)))


# ---- D: the ends of the Cpsd balance ---------------------------------------------------

def _exact_cpsd(case, x, y):
    key = ("values-cpsd", case.ident(), hash(x.tobytes()), hash(y.tobytes()))
    ref = E.memo(key, lambda: np.stack([np.asarray(a, np.complex128) for a in case.model(
        (x, y), None, real=E.LD, fft=E.exact_fft)]))
    return ref[0], ref[1].real, ref[2].real, ref[3].real


CPSD_D = [c for c in V.CASES if isinstance(c, V.Cpsd) and not c.host
          and c.row[:3] == (64, "odd", "s1")]


@pytest.mark.parametrize("case", CPSD_D, ids=[c.ident() for c in CPSD_D])
def test_cpsd_extremes(env, case):
    assert not case.one
    x, y = case.clean(None)
    stride = case.nfft - case.nov
    fails = []

    def bar(what, name, got, ref):
        err = row_nrel(got, ref)
        print("values: cpsd %s %s %s %.3g" % (case.ident(), what, name, err))
        if not err < EXACT:
            fails.append("%s %s: %.3g" % (what, name, err))

    with algorithm(env.gdsp, case.flags):
        case.setup(env)
        # y identically zero
        pxy, pxx, pyy, cxy = case.run(env, (x, np.zeros_like(y)), V.NAN, None)
        assert not np.any(pxy) and not np.any(pyy), "zero y: Pxy and Pyy are exact zeros"
        assert np.isnan(cxy).all(), "zero y: the coherence of no power is NaN"
        bar("zero-y", "Pxx", pxx, _exact_cpsd(case, x, y)[1])
        # and the other way round
        pxy, pxx, pyy, cxy = case.run(env, (np.zeros_like(x), y), V.NAN, None)
        assert not np.any(pxy) and not np.any(pxx), "zero x: Pxy and Pxx are exact zeros"
        assert np.isnan(cxy).all(), "zero x: the coherence of no power is NaN"
        bar("zero-x", "Pyy", pyy, _exact_cpsd(case, x, y)[2])
        # y zero in one segment (the balance of that segment is off: alpha = 1)
        y1 = np.array(y)
        y1[:, 2 * stride:2 * stride + case.nfft] = 0.0
        got = case.run(env, (x, y1), V.NAN, None)
        for name, a, b in zip(CP_NAMES, got, _exact_cpsd(case, x, y1)):
            assert np.isfinite(a).all(), name
            bar("zero-segment", name, a, b)
        # max |w y| subnormal
        ys = np.ldexp(y, -1060)
        assert 0 < np.abs(ys).max() < V.TINY
        pxy, pxx, pyy, cxy = case.run(env, (x, ys), V.NAN, None)
        assert np.isfinite(pxy).all() and np.isfinite(pxx).all() and np.isfinite(pyy).all()
        assert (np.isfinite(cxy) | (pyy == 0)).all(), "non-finite coherence where Syy is not 0"
        bar("subnormal-y", "Pxx", pxx, _exact_cpsd(case, x, y)[1])
        # x times 2^200 against y times 2^-200: 400 binary orders apart. Nothing
        # is non-finite, the coherence included, and Pxx is at the bar. The
        # balance spans every difference two normal doubles can have (+-1022),
        # so this is B's property as well: the clean run's bits, rescaled
        base = case.run(env, (x, y), V.NAN, None)
        got = case.run(env, (np.ldexp(x, 200), np.ldexp(y, -200)), V.NAN, None)
        for name, a, b, e in zip(CP_NAMES, got, base, (0, 400, -400, 0)):
            bad = ~np.isfinite(a)
            assert not bad.any(), "400 orders apart: %d of %d values of %s are not finite, at %s" \
                % (int(bad.sum()), a.size, name, np.argwhere(bad)[:6].tolist())
            assert np.array_equal(V.ldexp(a, -e), b), "400 orders apart: %s x 2^%d" % (name, -e)
        bar("400-apart", "Pxx", np.ldexp(got[1], -400), _exact_cpsd(case, x, y)[1])
    assert not fails, "; ".join(fails)


# ---- E: FIR error locality ---------------------------------------------------------------

def _fir_pairs_model(x, h, F, out_len):
    """The float64 model of fir.hip's packing: blocks 2p and 2p + 1 of a row as
    a + i b through numpy.fft, times the taps' spectrum, back, the valid parts."""
    n, m = x.shape[1], len(h)
    L = F - m + 1
    tpr = (-(-out_len // L) + 1) // 2
    xp = np.zeros((x.shape[0], (m - 1) + (2 * tpr + 1) * L + F))
    xp[:, m - 1:m - 1 + n] = x
    hs = np.fft.fft(np.concatenate([h, np.zeros(F - m)]))
    out = np.zeros((x.shape[0], 2 * tpr * L))
    for p in range(tpr):
        a = xp[:, 2 * p * L:2 * p * L + F]
        b = xp[:, (2 * p + 1) * L:(2 * p + 1) * L + F]
        z = np.fft.ifft(np.fft.fft(a + 1j * b, axis=1) * hs[None, :], axis=1)
        out[:, 2 * p * L:(2 * p + 1) * L] = z.real[:, m - 1:]
        out[:, (2 * p + 1) * L:(2 * p + 2) * L] = z.imag[:, m - 1:]
    return out[:, :out_len]


def _pair_level(x, L, m, out_len):
    """Per output i the largest |sample| the pair of blocks that produced it
    reads: x[2 p L - (m - 1) : 2 p L + 2 L], p = i // 2 L, clipped to the row."""
    n = x.shape[1]
    out = np.zeros((x.shape[0], out_len))
    for p in range(-(-out_len // (2 * L))):
        a, b = max(2 * p * L - (m - 1), 0), min(2 * p * L + 2 * L, n)
        if b > a:
            out[:, 2 * p * L:2 * p * L + 2 * L] = np.abs(x[:, a:b]).max(axis=1)[:, None]
    return out


def _own_level(x, m):
    """Per output i of the full convolution the largest of the m samples it sums."""
    pad = np.zeros((x.shape[0], m - 1))
    w = np.lib.stride_tricks.sliding_window_view(np.hstack([pad, np.abs(x), pad]), m, axis=1)
    return w.max(axis=2)


@pytest.mark.parametrize("F,n,m", [(256, 1700, 9), (4096, 6 * 4096 + 37, 100)])
def test_fir_locality(env, F, n, m):
    channels = 2
    L = F - m + 1
    rng = np.random.default_rng([F, m])
    h = rng.standard_normal(m)
    level = np.ldexp(1.0, 40 * ((np.arange(n) // F) % 2))  # 1, 2^40, 1, ... from block to block
    x = rng.uniform(-1, 1, (channels, n)) * level[None, :]
    x[1] = x[1] / 2.0 ** 40  # the second row: 2^-40, 1, 2^-40, ...
    out_len = n + m - 1
    exact = E.memo(("values-fir", F, n, m), lambda: np.stack(
        [np.convolve(r.astype(E.LD), h.astype(E.LD)) for r in x]))
    assert env.gdsp.fft.fir_block(m, F) == (F, True)
    import torch
    got = env.D.fir_batch(torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda(), full=True,
                          block=F)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    ref = _fir_pairs_model(x, h, F, out_len)
    sum_h = np.abs(h).sum()
    pair = _pair_level(x, L, m, out_len) * sum_h
    assert np.all(pair > 0)

    def err(y, scale, sel=None):
        d = np.abs(y.astype(E.LD) - exact) / scale
        return float((d if sel is None else d[sel]).max() / E.LD(E.U))

    e_got, e_ref = err(got, pair), err(ref, pair)
    # not asserted: the error against the level of the m samples an output sums
    # (a quiet block packed beside a loud one pays the pair's roundoff)
    own = _own_level(x, m) * sum_h
    quiet = own < pair * 2.0 ** -20
    assert quiet.any()
    print("values: fir F=%d err_u=%.3g e_ref=%.3g ratio=%.3g; quiet outputs against their own "
          "level: engine %.3g u, model %.3g u"
          % (F, e_got, e_ref, e_got / e_ref, err(got, own, quiet), err(ref, own, quiet)))
    assert e_got <= E.MARGIN * e_ref, "F=%d: %.4g u against %.4g u of the float64 model" \
        % (F, e_got, e_ref)
