"""GPU checks of the cosine transforms (gdsp_dct_batch, gdsp_dct_batch_device):
the fused kernel over its sizes and the composed form over its own, types II
and III, the three norms, through both entries.

Accuracy: exact_dft.err_u against the 80-bit route of dct_ref.py, bounded by
exact_dft.check with the project's MARGIN against the float64 route's err_u
(scipy.fft.dct) on the same rows in the same run; no other number is fixed. A
round trip is bounded by twice the forward case's bound.

Structure: an impulse gives a sampled cosine in every bin (bins 0, N/2 and
N-1, the kernel's special cases, included), a constant row gives 2 N c in bin
0 and roundoff of it elsewhere, and ortho keeps the squared 2-norm to 64 u.
The bound of the first two, in u = 2^-53 of the row's largest output as err_u
measures: a transform of N = 2^m points is, in radix-2 terms, m stages of one
rounded complex product and one sum, at most 4 u a stage in the worst case;
w_k, the product with it and the scale add two stages' worth: 4 (m + 2) u.
Other N run a chirp-z or mixed-radix plan: two transforms of the next power of
2 above 2 N at the most, so twice the bound of that length plus its chirp
products (m = 2 (ceil(log2 2N) + 2)). A wrong mirror, permutation or special
bin is wrong by the size of the output itself, 2^53 u.

Shapes: the smallest that reach each way the kernel can go wrong. N = 256 runs
16 rows per workgroup (T = 16 threads a row, four rows a wave), 2048 two rows
of two waves, 4096 one row of four waves, 8192 the first with 32 elements per
thread and 16384 eight waves a row (w_k after the transform, not as its
epilogue). Composed: 1 (no transform), 2, 255 (odd), 1000, 3001 (a prime, odd
ceil(N/2)), 32768, and 4096 under the flag. Row counts 1, 2, 5 and 33 (a
ragged last workgroup at N = 256).
"""
import gc
import importlib
import math

import numpy as np
import pytest

import dct_ref as R
import exact_dft as E
import values as V
from guarded import GUARD, NAN, guarded, pad_for

pytestmark = pytest.mark.gpu

FUSED_N = (256, 2048, 4096, 8192, 16384)
COMPOSED_N = (1, 2, 255, 1000, 3001, 32768)
TYPES = (2, 3)
KINDS = [(t, n) for t in TYPES for n in R.NORMS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


def _pow2_fused(N):
    return N & (N - 1) == 0 and 256 <= N <= 16384


class Flag:
    """ALGO_NO_FUSED_DCT for the block (composed=True), the path asserted."""

    def __init__(self, gdsp, composed, N):
        self.F, self.composed, self.N = gdsp.fft, composed, N

    def __enter__(self):
        F = self.F
        self.prev = F.Algorithm()
        F.SetAlgorithm(self.prev | F.ALGO_NO_FUSED_DCT if self.composed
                       else self.prev & ~F.ALGO_NO_FUSED_DCT)
        assert F.dct_fused(self.N) == (_pow2_fused(self.N) and not self.composed)

    def __exit__(self, *a):
        self.F.SetAlgorithm(self.prev)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _work_doubles(gdsp, rows, N):
    return int(gdsp._lib.lib().gdsp_dct_work_doubles(rows, N))


def _run(gdsp, D, x, type=2, norm=None, N=None, inverse=False, pad=0, fill=None):
    """device.dct_batch on rows ldx = n + pad apart (NaN in the gaps) into rows
    ldo = N + pad apart; fill: what out (and a work buffer) hold before."""
    import torch
    x = np.atleast_2d(x)
    rows, n = x.shape
    N = n if N is None else N
    wide = np.full((rows, n + pad), NAN)
    wide[:, :n] = x
    xd = _dev(wide)[:, :n]
    out = torch.full((rows, N + pad), GUARD if fill is None else fill, dtype=torch.float64,
                     device="cuda")
    work = None
    if fill is not None:
        work = torch.full((max(_work_doubles(gdsp, rows, N), 2),), fill, dtype=torch.float64,
                          device="cuda")
    got = D.dct_batch(xd, N, type=type, norm=norm, inverse=inverse, out=out[:, :N], work=work)
    torch.cuda.synchronize()
    full = out.cpu().numpy()
    if pad and fill is None:
        assert np.all(full[:, N:] == GUARD), "a store between the rows"
    return got.cpu().numpy()


_exact: dict = {}


def _std(N):
    """The standard real rows (noise, noise, an impulse at an odd index), then
    row 0 and row 1 again: five rows, an odd count."""
    if ("x", N) not in _exact:
        x = E.input_rows(N, real=True)
        x = np.concatenate([x, x[:2]])
        x.setflags(write=False)
        _exact[("x", N)] = x
    return _exact[("x", N)]


def _refs(N, type, norm):
    """(80-bit result, err_u of the float64 route) on _std(N), once per case."""
    key = (N, type, norm)
    if key not in _exact:
        x = _std(N)
        ex3 = R.dct_exact(x[:3], type, norm=norm)
        ex = np.concatenate([ex3, ex3[:2]])
        ex.setflags(write=False)
        _exact[key] = (ex, E.err_u(R.dct64(x, type, norm=norm), ex))
    return _exact[key]


def _stages(N):
    """The stages the bound of the structure tests counts (module docstring)."""
    if N <= 1:
        return 0
    if N & (N - 1) == 0:
        return int(math.log2(N))
    return 2 * (math.ceil(math.log2(2 * N)) + 2)  # (chirp-z: two transforms of >= 2N)


def _struct_bound(N):
    return 4.0 * (_stages(N) + 2)


# ---- accuracy ----------------------------------------------------------------------

CASES = [(n, False) for n in FUSED_N] + [(n, True) for n in COMPOSED_N] + [(4096, True)]
IDS = ["%d-%s" % (n, "composed" if c else "fused") for n, c in CASES]


@pytest.mark.parametrize("N,composed", CASES, ids=IDS)
def test_accuracy_on_the_standard_rows(gdsp, D, N, composed):
    """Both types, the three norms; three rows, then the 5-row batch."""
    variant = "composed" if composed else "fused"
    x = _std(N)
    with Flag(gdsp, composed, N):
        for type, norm in KINDS:
            ex, e_ref = _refs(N, type, norm)
            for rows in (3, 5):
                got = _run(gdsp, D, x[:rows], type, norm, pad=3)
                E.check("dct", N, "%s-type%d-%s-%d" % (variant, type, norm or "backward", rows),
                        E.err_u(got, ex[:rows]), e_ref)


@pytest.mark.parametrize("N,composed", CASES, ids=IDS)
def test_round_trip(gdsp, D, N, composed):
    """IDCT(DCT(x)) = x for each type and norm, within twice the forward
    case's bound (MARGIN times the float64 route's err_u of the forward
    transform); the float64 route's own round trip is printed beside it."""
    x = _std(N)[:3]
    with Flag(gdsp, composed, N):
        for type, norm in KINDS:
            _, e_ref = _refs(N, type, norm)
            y = _run(gdsp, D, x, type, norm)
            back = _run(gdsp, D, y, type, norm, inverse=True)
            e64 = E.err_u(R.idct64(R.dct64(x, type, norm=norm), type, norm=norm), x.astype(E.LD))
            print("round trip N=%d type %d %s: float64 route %.3g u" % (N, type, norm, e64))
            E.check("dct", N, "round-trip-type%d-%s" % (type, norm or "backward"),
                    E.err_u(back, x.astype(E.LD)), 2 * e_ref)


def test_flag_results_agree_with_the_fused_ones(gdsp, D):
    x = _std(4096)[:3]
    for type, norm in KINDS:
        ex, e_ref = _refs(4096, type, norm)
        with Flag(gdsp, False, 4096):
            a = _run(gdsp, D, x, type, norm)
        with Flag(gdsp, True, 4096):
            b = _run(gdsp, D, x, type, norm)
        # each within MARGIN e_ref of the exact result: within twice that of each other
        E.check("dct", 4096, "flag-against-fused-type%d-%s" % (type, norm or "backward"),
                E.err_u(b, a.astype(E.LD)), 2 * e_ref)


# ---- structure -----------------------------------------------------------------------

STRUCT_N = FUSED_N + COMPOSED_N


def _cos_table(N, js):
    """cos(pi k (2j+1) / (2N)) for every k and the listed j, np.longdouble, the
    angle reduced mod 4N in integers."""
    k = np.arange(N, dtype=np.int64)
    m = np.outer(np.asarray(js, np.int64) * 2 + 1, k) % (4 * N)
    return np.cos(m.astype(E.LD) * (E.PI / E.LD(2 * N)))


@pytest.mark.parametrize("N", STRUCT_N)
def test_impulse_gives_a_sampled_cosine(gdsp, D, N):
    """Type II of an impulse at j0 is 2 cos(pi k (2 j0 + 1) / (2N)) in every
    bin, 0, N/2 and N-1 included; type III of an impulse at k0 is the same
    table read the other way (1 for k0 = 0). Impulses at the first, an even, an
    odd, the middle and the last index."""
    js = sorted({min(j, N - 1) for j in (0, 1, 2, N // 2, max(N // 2 - 1, 0), (3 * N // 7) | 1,
                                         N - 1)})
    x = np.zeros((len(js), N))
    x[np.arange(len(js)), js] = 1.0
    C = _cos_table(N, js)                         # C[r, k]: j = js[r]
    want2 = 2 * C
    got2 = _run(gdsp, D, x, 2)
    e2 = E.err_u(got2, want2)
    print("impulse N=%d type II: %.3g u (bound %g)" % (N, e2, _struct_bound(N)))
    assert e2 <= _struct_bound(N)
    for r in range(len(js)):   # the special bins, one by one
        for k in {0, N // 2, N - 1}:
            assert abs(float(got2[r, k] - want2[r, k])) <= _struct_bound(N) * E.U * 2, (js[r], k)
    # type III: y[j] = 2 cos(pi k0 (2j+1) / (2N)), or 1 for k0 = 0
    k0s = np.asarray(js, np.int64)
    j = np.arange(N, dtype=np.int64)
    m = np.outer(k0s, 2 * j + 1) % (4 * N)
    want3 = 2 * np.cos(m.astype(E.LD) * (E.PI / E.LD(2 * N)))
    want3[k0s == 0] = 1
    got3 = _run(gdsp, D, x, 3)
    e3 = E.err_u(got3, want3)
    print("impulse N=%d type III: %.3g u (bound %g)" % (N, e3, _struct_bound(N)))
    assert e3 <= _struct_bound(N)


@pytest.mark.parametrize("N", STRUCT_N)
def test_constant_row_gives_one_bin(gdsp, D, N):
    c = np.array([[1.0], [-3.0], [0.37]]) * np.ones((3, N))
    got = _run(gdsp, D, c, 2)
    want = np.zeros((3, N), E.LD)
    want[:, 0] = 2 * E.LD(N) * c[:, 0].astype(E.LD)
    e = E.err_u(got, want)
    print("constant N=%d: %.3g u (bound %g)" % (N, e, _struct_bound(N)))
    assert e <= _struct_bound(N)
    # and back: type III of one bin is a constant row
    one = np.zeros((2, N))
    one[:, 0] = (1.0, -2.5)
    back = _run(gdsp, D, one, 3)
    assert E.err_u(back, np.array([[1.0], [-2.5]], E.LD) * np.ones((2, N), E.LD)) <= _struct_bound(N)


@pytest.mark.parametrize("N", STRUCT_N)
def test_ortho_keeps_the_two_norm(gdsp, D, N):
    x = np.random.default_rng(N).uniform(-1, 1, (5, N))
    for type in TYPES:
        y = _run(gdsp, D, x, type, "ortho")
        nx = np.sum(x.astype(E.LD) ** 2, axis=1)
        ny = np.sum(y.astype(E.LD) ** 2, axis=1)
        rel = float(np.max(np.abs(ny - nx) / nx) / E.U)
        print("ortho N=%d type %d: ||y||^2 within %.3g u of ||x||^2" % (N, type, rel))
        assert rel <= 64


# ---- nfft ----------------------------------------------------------------------------

@pytest.mark.parametrize("n,N", [(200, 256), (300, 256), (5000, 4096), (10000, 16384),
                                 (200, 255), (300, 1000), (7, 1), (1, 2)])
def test_cut_and_padded_rows_through_both_entries(gdsp, D, n, N):
    """N < n cuts, N > n pads with zeros (what lies beyond n, here NaN in the
    stride gap, is not read): the result is the padded row's, bit for bit, and
    within the accuracy bound; the host entry's bits are the device entry's."""
    F = gdsp.fft
    x = V.real_rows(n + N, 5, n)
    p = R.padded(x, N)
    for type, norm in KINDS:
        got = _run(gdsp, D, x, type, norm, N=N, pad=5)
        assert np.array_equal(got, _run(gdsp, D, p, type, norm)), (type, norm)
        ex = R.dct_exact(x, type, N, norm)
        E.check("dct", N, "n%d-type%d-%s" % (n, type, norm or "backward"), E.err_u(got, ex),
                E.err_u(R.dct64(x, type, N, norm), ex))
        h = F.DCTBatch(x, type, N, norm)
        assert h.shape == (5, N) and h.dtype == np.float64
        assert np.array_equal(h, got), "the host entry's bits differ from the device entry's"
        assert np.array_equal(F.DCT(x[1], type, N, norm), got[1])
        inv = F.IDCTBatch(x, type, N, norm)
        assert np.array_equal(inv, _run(gdsp, D, x, type, norm, N=N, inverse=True))
        assert np.array_equal(F.IDCT(x[4], type, N, norm), inv[4])


def test_length_one_and_two(gdsp, D):
    x = np.array([[3.0], [-2.0], [0.5]])
    assert np.array_equal(_run(gdsp, D, x, 2), 2 * x)
    assert np.array_equal(_run(gdsp, D, x, 2, "forward"), x)
    assert np.array_equal(_run(gdsp, D, x, 2, "ortho"), x)
    assert np.array_equal(_run(gdsp, D, x, 3), x)
    assert np.array_equal(_run(gdsp, D, x, 3, "forward"), x / 2)
    assert np.max(np.abs(_run(gdsp, D, x, 3, "ortho") - x)) <= 2 * E.U * 3
    x2 = np.array([[1.0, 2.0], [0.5, -0.25]])
    for type, norm in KINDS:
        ex = R.dct_exact(x2, type, norm=norm)
        assert E.err_u(_run(gdsp, D, x2, type, norm), ex) <= 8


# ---- bit-level independence ----------------------------------------------------------

INDEP = [(256, False), (2048, False), (16384, False), (255, True), (4096, True)]
INDEP_IDS = ["%d-%s" % (n, "composed" if c else "fused") for n, c in INDEP]


@pytest.mark.parametrize("N,composed", INDEP, ids=INDEP_IDS)
def test_a_row_depends_on_itself_alone(gdsp, D, N, composed):
    """A row's bits are the same alone, in a batch of 33 (at any slot of a
    workgroup), beside a row of 1e200 and beside a NaN row."""
    rows = 33 if N <= 2048 else 5
    x = V.real_rows(N + 1, rows, N)
    with Flag(gdsp, composed, N):
        for type, norm in ((2, None), (3, None), (2, "ortho"), (3, "ortho")):
            batch = _run(gdsp, D, x, type, norm)
            for r in (0, 1, rows // 2, rows - 1):
                alone = _run(gdsp, D, x[r], type, norm)
                assert np.array_equal(alone[0], batch[r]), (type, norm, r)
            loud = x.copy()
            loud[1] = 1e200 * x[1]
            loud[rows - 2] = NAN
            got = _run(gdsp, D, loud, type, norm)
            keep = [r for r in range(rows) if r not in (1, rows - 2)]
            assert np.array_equal(got[keep], batch[keep]), (type, norm)
            assert np.all(np.isfinite(got[1])) and not np.any(np.isfinite(got[rows - 2]))


@pytest.mark.parametrize("N,composed", INDEP, ids=INDEP_IDS)
def test_zero_row_gives_exact_zeros(gdsp, D, N, composed):
    x = V.real_rows(N, 5, N)
    with Flag(gdsp, composed, N):
        for type, norm in KINDS:
            clean = _run(gdsp, D, x, type, norm)
            for dead in (0, 3, 4):
                y = x.copy()
                y[dead] = 0.0
                got = _run(gdsp, D, y, type, norm)
                assert np.all(got[dead] == 0), (type, norm, dead)
                live = [r for r in range(5) if r != dead]
                assert np.array_equal(got[live], clean[live])


CONTAIN = [(256, 33, False), (2048, 5, False), (8192, 3, False), (16384, 3, False),
           (255, 5, True), (2, 3, True)]


@pytest.mark.parametrize("N,rows,composed", CONTAIN,
                         ids=["%d-%s" % (c[0], "composed" if c[2] else "fused") for c in CONTAIN])
def test_non_finite_sample_stays_in_its_row(gdsp, D, N, rows, composed):
    """One NaN, then one Inf, at the first, a middle and the last sample of a
    row: every output of that row is non-finite and every other row keeps the
    clean run's bits, for both types."""
    x = V.real_rows(N + rows, rows, N)
    with Flag(gdsp, composed, N):
        for type in TYPES:
            clean = _run(gdsp, D, x, type)
            for name, value, _ in V.bad_values(False):
                for r, j in ((rows - 1, 0), (rows // 2, N // 2 + 1 if N > 2 else 1), (0, N - 1)):
                    got = _run(gdsp, D, V.with_sample(x, (r, j), value), type)
                    V.check_contained((got,), (clean,), [V.rows_mask(clean.shape, [r])],
                                      "%s at (%d, %d), type %d" % (name, r, j, type))


SCALE = [(256, 5, False), (8192, 3, False), (16384, 2, False), (1000, 3, True), (1, 3, True)]


@pytest.mark.parametrize("N,rows,composed", SCALE,
                         ids=["%d-%s" % (c[0], "composed" if c[2] else "fused") for c in SCALE])
def test_scaling_by_powers_of_two_is_exact(gdsp, D, N, rows, composed):
    x = np.random.default_rng(N).uniform(-1, 1, (rows, N))
    n_out = len(KINDS)
    with Flag(gdsp, composed, N):
        V.check_equivariant(
            lambda ins, fill: tuple(_run(gdsp, D, ins[0], t, nm) for t, nm in KINDS), (x,),
            [((300,), (300,) * n_out), ((-300,), (-300,) * n_out)], "dct %d" % N)


@pytest.mark.parametrize("N,rows,composed", SCALE,
                         ids=["%d-%s" % (c[0], "composed" if c[2] else "fused") for c in SCALE])
def test_poisoned_out_and_work_change_nothing(gdsp, D, N, rows, composed):
    x = V.real_rows(N, rows, N)
    poison = np.full((2 * rows + 1, N), NAN)

    def run(ins, fill):
        return tuple(_run(gdsp, D, ins[0], t, nm, fill=fill) for t, nm in ((2, None), (3, "ortho")))

    with Flag(gdsp, composed, N):
        first = V.check_history(run, (x,), (poison,), "dct %d" % N)
        assert np.array_equal(first[0], _run(gdsp, D, x, 2))


# ---- layout --------------------------------------------------------------------------

LAYOUT = [(256, False, 1), (256, False, 2), (256, False, 5), (256, False, 33), (2048, False, 3),
          (8192, False, 3), (255, True, 1), (255, True, 5), (1, True, 5)]


@pytest.mark.parametrize("N,composed,rows", LAYOUT,
                         ids=["%d-%s-%d" % (c[0], "composed" if c[1] else "fused", c[2])
                              for c in LAYOUT])
def test_strides_and_guard_bands(gdsp, D, N, composed, rows):
    import torch
    n = N + 40  # cut to N: the samples past it are NaN and must not be read
    x = V.real_rows(N + rows, rows, n)
    x[:, N:] = NAN
    ldx, ldo = n + 5, N + 7
    with Flag(gdsp, composed, N):
        for type in TYPES:
            dense = _run(gdsp, D, x[:, :N], type)
            wide = torch.full((rows, ldx), NAN, dtype=torch.float64, device="cuda")
            wide[:, :n] = _dev(x)
            payload = torch.full((rows, ldo), GUARD, dtype=torch.float64, device="cuda")
            view, check = guarded(payload, GUARD, pad_for(ldo))
            D.dct_batch(wide[:, :n], N, type=type, out=view[:, :N])
            torch.cuda.synchronize()
            check("dct type %d N=%d rows=%d" % (type, N, rows))
            got = view.cpu().numpy()
            assert np.all(got[:, N:] == GUARD)
            assert np.array_equal(got[:, :N], dense), type


INPLACE = [(256, False, 33), (2048, False, 5), (16384, False, 2), (255, True, 5), (4096, True, 3),
           (1, True, 3)]


@pytest.mark.parametrize("N,composed,rows", INPLACE,
                         ids=["%d-%s" % (c[0], "composed" if c[1] else "fused") for c in INPLACE])
def test_exactly_in_place_equals_out_of_place(gdsp, D, N, composed, rows):
    """d_out == d_x with the same stride and N <= n: the same bits as out of
    place, rows wider than N keep their tails."""
    import torch
    n = N + 9
    x = V.real_rows(N + 3, rows, n)
    with Flag(gdsp, composed, N):
        for type, norm in ((2, None), (3, None), (3, "ortho")):
            want = _run(gdsp, D, x, type, norm, N=N)
            buf = _dev(x)
            got = D.dct_batch(buf, N, type=type, norm=norm, out=buf[:, :N])
            torch.cuda.synchronize()
            full = buf.cpu().numpy()
            assert got.data_ptr() == buf.data_ptr()
            assert np.array_equal(full[:, :N], want), (type, norm)
            assert np.array_equal(full[:, N:], x[:, N:])
            # N == n, dense rows
            dense = _dev(x[:, :N])
            D.dct_batch(dense, type=type, norm=norm, out=dense)
            torch.cuda.synchronize()
            assert np.array_equal(dense.cpu().numpy(), want), (type, norm)


def test_device_entry_refuses_partial_overlap(gdsp, D):
    import torch
    buf = torch.zeros(4 * 300, dtype=torch.float64, device="cuda")
    x = buf[:600].view(2, 300)
    bad = [buf[1:601].view(2, 300)[:, :256],            # shifted by one sample
           buf[500:500 + 512].view(2, 256),            # starts inside x
           buf[:512].view(2, 256)]                     # the same start, another stride
    for out in bad:
        with pytest.raises(gdsp.GDSPError) as e:
            D.dct_batch(x, 256, out=out)
        assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    with pytest.raises(gdsp.GDSPError) as e:           # in place but N > n
        D.dct_batch(buf[:512].view(2, 256)[:, :200], 256, out=buf[:512].view(2, 256))
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    D.dct_batch(x, 256, out=buf[600:600 + 512].view(2, 256))
    D.dct_batch(x, 256, out=x[:, :256])
    torch.cuda.synchronize()


def test_device_wrapper_refuses_a_length_below_one(gdsp, D):
    """n = 0 is scipy's ValueError, not "the row length" of the C ABI: a
    zero-width view of a live tensor as out is not written past."""
    import torch
    buf = torch.full((3, 64), GUARD, dtype=torch.float64, device="cuda")
    x = _dev(V.real_rows(3, 1, 32))
    for n in (0, -1):
        with pytest.raises(ValueError):
            D.dct_batch(x, n)
    with pytest.raises(ValueError):
        D.dct_batch(x, 0, out=buf[1:2, :0])
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())


@pytest.mark.parametrize("N,composed", [(1024, False), (1000, True)])
def test_no_allocation_with_out_and_work_given(gdsp, D, N, composed):
    """With out and work given the allocator's counters do not move (the fused
    form needs no work at all: none is passed there)."""
    import torch
    x = _dev(V.real_rows(N, 6, N))
    with Flag(gdsp, composed, N):
        for type in TYPES:
            out = torch.empty((6, N), dtype=torch.float64, device="cuda")
            work = torch.empty(_work_doubles(gdsp, 6, N), dtype=torch.float64,
                               device="cuda") if composed else None
            assert composed == (work is not None and work.numel() == 18 * N)
            D.dct_batch(x, type=type, out=out, work=work)  # the plan and the table, once
            torch.cuda.synchronize()
            gc.collect()  # (tensors an earlier test's garbage still holds go now, not mid-count)
            before = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
            got = D.dct_batch(x, type=type, out=out, work=work)
            assert (torch.cuda.memory_allocated(), torch.cuda.memory_reserved()) == before
            assert got is out
            del got  # (it would keep this round's out alive into the next round's count)
            torch.cuda.synchronize()


# ---- paths reached -------------------------------------------------------------------

def test_host_call_crosses_a_row_range(gdsp, D):
    """2^24 samples a range: 1024 rows of 16384, so 1026 rows take a second
    range of two. The bits are those of one device call over all rows."""
    F = gdsp.fft
    N, rows = 16384, 1026
    x = np.random.default_rng(5).uniform(-1, 1, (rows, N))
    with Flag(gdsp, False, N):
        before = F.LoopStats()["later_chunks"]
        got = F.DCTBatch(x, 2, norm="ortho")
        assert F.LoopStats()["later_chunks"] - before == 1
        before = F.LoopStats()["later_chunks"]
        F.DCTBatch(x[:1024], 3)
        assert F.LoopStats()["later_chunks"] == before
        assert np.array_equal(got, _run(gdsp, D, x, 2, "ortho"))
        assert np.array_equal(got[1024:], F.DCTBatch(x[1024:], 2, norm="ortho"))


def test_composed_form_crosses_a_chunk(gdsp, D):
    """The composed form's chunks are 2^24 div N rows: 512 of 32768, so 514
    rows run a second chunk of two. The rows of the second chunk have the bits
    they have in a call of their own."""
    F = gdsp.fft
    N, rows = 32768, 514
    x = np.random.default_rng(6).uniform(-1, 1, (rows, N))
    for type in TYPES:
        before = F.LoopStats()["later_chunks"]
        got = _run(gdsp, D, x, type)
        assert F.LoopStats()["later_chunks"] - before == 1
        assert np.array_equal(got[512:], _run(gdsp, D, x[512:], type))
        assert np.array_equal(got[:3], _run(gdsp, D, x[:3], type))


def test_fused_query_reports_the_path_that_ran(gdsp, D):
    """A work buffer filled with a sentinel tells which form ran: the fused
    kernel takes no work and leaves every element of it alone, the composed
    form writes its chunk's rows into it. Where dct_fused(N) says fused the
    sentinel survives, where it says composed (the flag, or a size no kernel
    serves) it does not; the host entry gives the bits of the form the query
    names, and the two forms' bits differ somewhere."""
    import torch
    F = gdsp.fft
    x = _std(4096)[:3]
    xd = _dev(x)
    res = {}
    for composed in (False, True):
        with Flag(gdsp, composed, 4096):
            assert F.dct_fused(4096) == (not composed)
            assert _work_doubles(gdsp, 3, 4096) == (9 * 4096 if composed else 0)
            for type in TYPES:
                work = torch.full((9 * 4096,), GUARD, dtype=torch.float64, device="cuda")
                got = D.dct_batch(xd, type=type, work=work)
                torch.cuda.synchronize()
                untouched = bool((work == GUARD).all())
                assert untouched == F.dct_fused(4096), (composed, type)
                res[composed, type] = got.cpu().numpy()
                assert np.array_equal(res[composed, type], F.DCTBatch(x, type))
    for type in TYPES:
        differ = int((res[False, type] != res[True, type]).sum())
        print("fused against composed at 4096, type %d: %d element(s) differ" % (type, differ))
        assert differ > 0
    # a size no kernel serves is composed with the flag clear, and says so
    with Flag(gdsp, False, 1000):
        work = torch.full((9 * 1000,), GUARD, dtype=torch.float64, device="cuda")
        D.dct_batch(_dev(_std(1000)[:3]), work=work)
        torch.cuda.synchronize()
        assert not F.dct_fused(1000) and not bool((work == GUARD).all())
