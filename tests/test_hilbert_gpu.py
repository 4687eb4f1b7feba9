"""GPU checks of the analytic signal (gdsp_hilbert_batch,
gdsp_hilbert_batch_device): the fused kernel over its sizes and the composed
form over its own, through both entries.

Accuracy: exact_dft.err_u of the quadrature against the 80-bit route of
hilbert_ref.py, bounded by exact_dft.check with the project's MARGIN against
the float64 route's err_u on the same rows in the same run; no other number is
fixed. The analytic real part is the input's bits; the envelope is within
4 * 2^-53 relative of np.hypot of the analytic parts (2 u from the fma and the
product, halved by the root, plus 1 u for the root, plus 1 u for hypot).

Shapes: the smallest that reach each way the kernel can go wrong. N = 256 runs
16 rows per workgroup (T = 16 threads a row, four rows a wave), 2048 two rows
of two waves, 4096 one row of four waves, 8192 the first with 32 elements per
thread and 16384 eight waves a row (and the inputs read again at the store).
Row counts 1, 2, 5 and 33 (a ragged last workgroup at N = 256).

Values: balance, zeros, containment, scaling and history with the helpers of
values.py. Layout: strides above the row lengths, guard bands (guarded.py),
overlap, no allocation with out and work given. Paths: the flag, and the host
entry's second row range.
"""
import gc
import importlib
import os

import numpy as np
import pytest

import exact_dft as E
import hilbert_ref as H
import values as V
from conftest import GOLDEN
from guarded import GUARD, NAN, guarded, pad_for

pytestmark = pytest.mark.gpu

KINDS = ("analytic", "quadrature", "envelope")
FUSED_N = (256, 4096, 8192, 16384)
COMPOSED_N = (255, 1000, 3001, 32768)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


class Flag:
    """ALGO_NO_FUSED_HILBERT for the block (composed=True), the path asserted."""

    def __init__(self, gdsp, composed, N):
        self.F, self.composed, self.N = gdsp.fft, composed, N

    def __enter__(self):
        F = self.F
        self.prev = F.Algorithm()
        F.SetAlgorithm(self.prev | F.ALGO_NO_FUSED_HILBERT if self.composed
                       else self.prev & ~F.ALGO_NO_FUSED_HILBERT)
        pow2 = self.N & (self.N - 1) == 0 and 256 <= self.N <= 16384
        assert F.hilbert_fused(self.N) == (pow2 and not self.composed)

    def __exit__(self, *a):
        self.F.SetAlgorithm(self.prev)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(D, x, N=None, kind="quadrature", pad=0, fill=None):
    """device.hilbert_batch on rows ldx = n + pad apart (NaN in the gaps) into
    rows ldo = N + pad apart; fill: what out (and a work buffer) hold before."""
    import torch
    x = np.atleast_2d(x)
    rows, n = x.shape
    N = n if N is None else N
    wide = np.full((rows, n + pad), NAN)
    wide[:, :n] = x
    xd = _dev(wide)[:, :n]
    dt = torch.complex128 if kind == "analytic" else torch.float64
    out = torch.full((rows, N + pad), GUARD if fill is None else fill, dtype=dt, device="cuda")
    work = None
    if fill is not None:
        work = torch.full((min(rows, max(1, (1 << 24) // N)) * N * 3,), fill,
                          dtype=torch.float64, device="cuda")
    got = D.hilbert_batch(xd, N, kind=kind, out=out[:, :N], work=work)
    torch.cuda.synchronize()
    full = out.cpu().numpy()
    if pad and fill is None:
        assert np.all(full[:, N:] == GUARD), "a store between the rows"
    return got.cpu().numpy()


_exact: dict = {}


def _refs(N, rows=(0, 1, 2, 3, 4)):
    """(inputs, 80-bit quadrature, float64-route quadrature) of the real parts
    of the standard rows, computed once per N."""
    if N not in _exact:
        x = E.input_rows(N, real=True, rows=(0, 1, 2, 3))
        x = np.concatenate([x, x[:1]])
        ex = H.quadrature_exact(x)
        ex.setflags(write=False)
        _exact[N] = (x, ex, H.quadrature64(x))
    x, ex, f64 = _exact[N]
    r = list(rows)
    return x[r], ex[r], f64[r]


def _check_envelope(env, a, what):
    """Within 4 u of np.hypot of the same inputs' analytic parts (the module
    docstring's derivation); exact zeros where both parts are."""
    hyp = np.hypot(a.real, a.imag)
    rel = float(np.max(np.abs(env - hyp) / np.where(hyp > 0, hyp, 1.0)) / E.U)
    print("envelope %s: %.3g u of hypot" % (what, rel))
    assert rel <= 4.0 and np.all(env[hyp == 0] == 0)


def _check_kinds(D, x, N, variant, pad=3):
    """All three kinds of one shape against the references; returns the
    quadrature."""
    ex, f64 = H.quadrature_exact(x, N), H.quadrature64(x, N)
    e_ref = E.err_u(f64, ex)
    q = _run(D, x, N, "quadrature", pad)
    E.check("hilbert", N, variant, E.err_u(q, ex), e_ref)
    a = _run(D, x, N, "analytic", pad)
    assert np.array_equal(a.real.view(np.int64), H.padded(x, N).view(np.int64)), \
        "the real part is not the input's bits"
    E.check("hilbert", N, variant + "-analytic", E.err_u(a.imag, ex), e_ref)
    _check_envelope(_run(D, x, N, "envelope", pad), a, "N=%d %s" % (N, variant))
    return q


# ---- accuracy ----------------------------------------------------------------------

CASES = [(n, False) for n in FUSED_N] + [(n, True) for n in COMPOSED_N] + [(4096, True)]


@pytest.mark.parametrize("N,composed", CASES,
                         ids=["%d-%s" % (n, "composed" if c else "fused") for n, c in CASES])
def test_accuracy_on_the_standard_rows(gdsp, D, N, composed):
    """Rows 0-2, then the 5-row batch (an odd last row; at N = 256 it shares a
    workgroup with nothing else, at 16384 every pair has its own)."""
    variant = "composed" if composed else "fused"
    with Flag(gdsp, composed, N):
        for rows in ((0, 1, 2), (0, 1, 2, 3, 4)):
            x, ex, f64 = _refs(N, rows)
            e_ref = E.err_u(f64, ex)
            for kind in KINDS if len(rows) == 3 else ("quadrature",):
                got = _run(D, x, N, kind, pad=3)
                if kind == "analytic":
                    assert np.array_equal(got.real.view(np.int64), x.view(np.int64))
                    got = got.imag
                if kind == "envelope":
                    _check_envelope(got, _run(D, x, N, "analytic"), "N=%d %s" % (N, variant))
                    continue
                E.check("hilbert", N, "%s-%s-%d" % (variant, kind, len(rows)),
                        E.err_u(got, ex), e_ref)


def test_flag_results_agree_with_the_fused_ones(gdsp, D):
    x, ex, f64 = _refs(4096, (0, 1, 2))
    with Flag(gdsp, False, 4096):
        a = _run(D, x, 4096)
    with Flag(gdsp, True, 4096):
        b = _run(D, x, 4096)
    e_ref = E.err_u(f64, ex)
    E.check("hilbert", 4096, "fused", E.err_u(a, ex), e_ref)
    E.check("hilbert", 4096, "flag", E.err_u(b, ex), e_ref)
    # each within MARGIN e_ref of the exact result: within twice that of each other
    E.check("hilbert", 4096, "flag-against-fused", E.err_u(b, a.astype(E.LD)), 2 * e_ref)


@pytest.mark.parametrize("n,N", [(200, 256), (300, 256), (200, 255), (300, 1000)])
def test_padding_and_truncation_through_both_entries(gdsp, D, n, N):
    x = V.real_rows(n + N, 5, n)
    q = _check_kinds(D, x, N, "device-n%d" % n)
    F = gdsp.fft
    a = F.HilbertBatch(x, N)
    assert a.shape == (5, N) and a.dtype == np.complex128
    assert np.array_equal(a.real.view(np.int64), H.padded(x, N).view(np.int64))
    assert np.array_equal(a.imag, q), "the host entry's bits differ from the device entry's"
    assert np.array_equal(F.EnvelopeBatch(x, N), _run(D, x, N, "envelope"))
    # one row per transform: alone or in a batch, the same bits
    assert np.array_equal(F.Hilbert(x[1], N), a[1])
    ex = H.quadrature_exact(x[1], N)
    E.check("hilbert", N, "host-one-row", E.err_u(F.Hilbert(x[1], N).imag, ex),
            E.err_u(H.quadrature64(x[1], N), ex))
    assert np.array_equal(F.Envelope(x[1], N), F.EnvelopeBatch(x[1:2], N)[0])


def test_length_one_gives_zero(gdsp, D):
    x = np.array([[3.0], [-2.0], [0.5]])
    assert np.array_equal(_run(D, x, 1, "quadrature"), np.zeros((3, 1)))
    assert np.array_equal(_run(D, x, 1, "analytic"), x.astype(np.complex128))
    assert np.array_equal(_run(D, x, 1, "envelope"), np.abs(x))
    assert np.array_equal(gdsp.fft.HilbertBatch(np.ones((2, 7)), 1), np.ones((2, 1), np.complex128))


# ---- value properties ----------------------------------------------------------------

@pytest.mark.parametrize("N", [256, 2048, 16384])
def test_balance_keeps_a_quiet_row_beside_a_loud_one(gdsp, D, N):
    """A row times 2^40 beside a row of level 1, in both orders: each row's
    own err_u passes the bound of the accuracy test (two rows packed into one
    transform without a balance would leave the quiet one at 1.4e12 u; the
    kernel runs one row per transform, so a neighbour's level cannot reach it)."""
    x, ex, f64 = _refs(N, (0, 1, 1, 0, 0))
    k = np.array([40, 0, 0, 40, -40])[:, None]
    xs = np.ldexp(x, k)
    with Flag(gdsp, False, N):
        got = _run(D, xs, N)
    for r in range(5):
        E.check("hilbert", N, "balance-row%d" % r, E.err_u(np.ldexp(got[r], -k[r]), ex[r]),
                E.err_u(f64[r], ex[r]))


@pytest.mark.parametrize("N,composed", [(256, False), (4096, False), (255, True)])
def test_zero_row_gives_exact_zeros(gdsp, D, N, composed):
    x = V.real_rows(N, 5, N)
    with Flag(gdsp, composed, N):
        clean = _run(D, x, N)
        for dead in (0, 3, 4):  # the first of a pair, the second, the unpartnered last
            y = x.copy()
            y[dead] = 0.0
            for kind in KINDS:
                got = _run(D, y, N, kind)
                assert np.all(got[dead] == 0), (kind, dead)
                assert np.all(np.isfinite(got))
            q = _run(D, y, N)
            live = [r for r in range(5) if r // 2 != dead // 2]
            assert np.array_equal(q[live], clean[live])


CONTAIN = [(256, 33, 3, False), (2048, 5, 0, False), (16384, 3, 0, False), (255, 5, 1, True)]


def _contain(gdsp, D, N, rows, p, composed):
    """Yields (what, bad row, kind, clean outputs, outputs with the sample)."""
    x = V.real_rows(N + rows, rows, N)
    with Flag(gdsp, composed, N):
        clean = {k: _run(D, x, N, k) for k in KINDS}
        for name, value, _ in V.bad_values(False):
            for r in (2 * p, 2 * p + 1):
                y = V.with_sample(x, (r, N // 2 + 1), value)
                for k in KINDS:
                    yield "%s in row %d, %s" % (name, r, k), r, k, clean[k], _run(D, y, N, k)


@pytest.mark.parametrize("N,rows,p,composed", CONTAIN,
                         ids=["%d-%s" % (c[0], "composed" if c[3] else "fused") for c in CONTAIN])
def test_non_finite_sample_stays_in_its_row(gdsp, D, N, rows, p, composed):
    """One NaN, then one Inf, at a middle sample of row 2p and then of row
    2p + 1 (33 rows at N = 256: 15 other rows share the workgroup): that
    row's outputs are all non-finite (analytic: the imaginary parts; the real
    parts are the input's bits), every other row keeps the clean run's bits,
    and its neighbour stays within the accuracy bound of its own reference
    (test_partner_of_a_bad_row_keeps_its_bits asserts the neighbour's bits)."""
    x = V.real_rows(N + rows, rows, N)
    for what, r, kind, clean, got in _contain(gdsp, D, N, rows, p, composed):
        mate = r ^ 1
        bad = np.zeros(clean.shape, bool)
        bad[r] = True
        keep = ~bad
        if mate < rows:
            keep[mate] = False
        g = got.imag if kind == "analytic" else got
        c = clean.imag if kind == "analytic" else clean
        V.check_contained((g,), (c,), [(bad, keep)], what)
        if kind == "analytic":
            assert np.array_equal(got.real[keep], clean.real[keep])
        if mate < rows:
            assert np.all(np.isfinite(got[mate])), what
            if kind == "quadrature":
                ex = H.quadrature_exact(x[mate], N)
                E.check("hilbert", N, "partner of " + what, E.err_u(got[mate], ex),
                        E.err_u(H.quadrature64(x[mate], N), ex), record=False)


@pytest.mark.parametrize("N,rows,p,composed", CONTAIN,
                         ids=["%d-%s" % (c[0], "composed" if c[3] else "fused") for c in CONTAIN])
def test_partner_of_a_bad_row_keeps_its_bits(gdsp, D, N, rows, p, composed):
    """Every other row, the neighbour a packed kernel would pair it with
    included, is bit-identical to the clean run: a row's outputs depend on
    that row alone in both forms. (An earlier form of the fused kernel carried
    rows 2p and 2p + 1 in one transform; the partner of a bad row, recomputed
    alone, then moved by 4.8-12.3 u at N = 256 ... 16384, which is why the
    kernel runs one row per transform.)"""
    worst = 0.0
    fails = []
    for what, r, kind, clean, got in _contain(gdsp, D, N, rows, p, composed):
        mate = r ^ 1
        if mate >= rows:
            continue
        g = got.imag if kind == "analytic" else got
        c = clean.imag if kind == "analytic" else clean
        d = float(np.max(np.abs(g[mate] - c[mate])) / np.max(np.abs(c[mate])) / E.U)
        worst = max(worst, d)
        if not np.array_equal(g[mate], c[mate]):
            fails.append("%s: %d element(s), %.3g u" % (what, int((g[mate] != c[mate]).sum()), d))
    print("partner N=%d %s: worst %.3g u" % (N, "composed" if composed else "fused", worst))
    assert not fails, "; ".join(fails)


SCALE = [(256, 5, False), (8192, 3, False), (1000, 3, True)]


@pytest.mark.parametrize("N,rows,composed", SCALE,
                         ids=["%d-%s" % (c[0], "composed" if c[2] else "fused") for c in SCALE])
def test_scaling_by_powers_of_two_is_exact(gdsp, D, N, rows, composed):
    x = V.real_rows(N, rows, N)
    with Flag(gdsp, composed, N):
        V.check_equivariant(lambda ins, fill: tuple(_run(D, ins[0], N, k) for k in KINDS), (x,),
                            [((200,), (200, 200, 200)), ((-200,), (-200, -200, -200))],
                            "hilbert %d" % N)


@pytest.mark.parametrize("N,rows,composed", SCALE,
                         ids=["%d-%s" % (c[0], "composed" if c[2] else "fused") for c in SCALE])
def test_poisoned_out_and_work_change_nothing(gdsp, D, N, rows, composed):
    x = V.real_rows(N, rows, N)
    poison = np.full((2 * rows + 1, N), NAN)

    def run(ins, fill):
        return tuple(_run(D, ins[0], N, k, fill=fill) for k in KINDS)

    with Flag(gdsp, composed, N):
        first = V.check_history(run, (x,), (poison,), "hilbert %d" % N)
        assert np.array_equal(first[1], _run(D, x, N))


# ---- layout --------------------------------------------------------------------------

LAYOUT = [(256, False, 1), (256, False, 2), (256, False, 5), (256, False, 33), (8192, False, 3),
          (255, True, 1), (255, True, 5)]


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
        for kind in KINDS:
            dense = _run(D, x[:, :N], N, kind)
            wide = torch.full((rows, ldx), NAN, dtype=torch.float64, device="cuda")
            wide[:, :n] = _dev(x)
            dt = torch.complex128 if kind == "analytic" else torch.float64
            payload = torch.full((rows, ldo), GUARD, dtype=dt, device="cuda")
            view, check = guarded(payload, GUARD, pad_for(ldo))
            D.hilbert_batch(wide[:, :n], N, kind=kind, out=view[:, :N])
            torch.cuda.synchronize()
            check("hilbert %s N=%d rows=%d" % (kind, N, rows))
            got = view.cpu().numpy()
            assert np.all(got[:, N:] == GUARD)
            assert np.array_equal(got[:, :N], dense), kind


def test_device_entry_refuses_overlap(gdsp, D):
    import torch
    buf = torch.zeros(4 * 300, dtype=torch.float64, device="cuda")
    x = buf[:600].view(2, 300)
    for out in (x[:, :256], buf[500:500 + 512].view(2, 256)):
        with pytest.raises(gdsp.GDSPError) as e:
            D.hilbert_batch(x, 256, kind="quadrature", out=out)
        assert e.value.status == gdsp._lib.GDSP_ERR_INVALID
    D.hilbert_batch(x, 256, kind="quadrature", out=buf[600:600 + 512].view(2, 256))
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,composed", [(1024, False), (1000, True)])
def test_no_allocation_with_out_and_work_given(gdsp, D, N, composed):
    import torch
    x = _dev(V.real_rows(N, 6, N))
    with Flag(gdsp, composed, N):
        for kind in KINDS:
            dt = torch.complex128 if kind == "analytic" else torch.float64
            out = torch.empty((6, N), dtype=dt, device="cuda")
            work = torch.empty(6 * N * 3, dtype=torch.float64, device="cuda")
            D.hilbert_batch(x, N, kind=kind, out=out, work=work)  # the plan, once
            torch.cuda.synchronize()
            gc.collect()  # (tensors an earlier test's garbage still holds go now, not mid-count)
            before = torch.cuda.memory_allocated()
            got = D.hilbert_batch(x, N, kind=kind, out=out, work=work)
            assert torch.cuda.memory_allocated() == before
            assert got is out
            del got  # (it would keep this round's out alive into the next round's count)
            torch.cuda.synchronize()


# ---- paths reached -------------------------------------------------------------------

def test_host_call_crosses_a_row_range(gdsp, D):
    """2^24 samples a range: 1024 rows of 16384, so 1026 rows take a second
    range of one pair. The ranges start at even rows, so the bits are those of
    one device call over all rows (the unchunked computation)."""
    F = gdsp.fft
    N, rows = 16384, 1026
    x = np.random.default_rng(5).uniform(-1, 1, (rows, N))
    with Flag(gdsp, False, N):
        before = F.LoopStats()["later_chunks"]
        got = F.EnvelopeBatch(x)
        assert F.LoopStats()["later_chunks"] - before == 1
        before = F.LoopStats()["later_chunks"]
        F.EnvelopeBatch(x[:1024])
        assert F.LoopStats()["later_chunks"] == before
        assert np.array_equal(got, _run(D, x, N, "envelope"))


def test_composed_form_crosses_a_chunk(gdsp, D):
    """The composed form's chunks are 2^24 div N rows: 512 of 32768, so 514
    rows run a second chunk of two. One row per transform: the rows of the
    second chunk have the bits they have in a call of their own."""
    F = gdsp.fft
    N, rows = 32768, 514
    x = np.random.default_rng(6).uniform(-1, 1, (rows, N))
    before = F.LoopStats()["later_chunks"]
    got = _run(D, x, N, "quadrature")
    assert F.LoopStats()["later_chunks"] - before == 1
    assert np.array_equal(got[512:], _run(D, x[512:], N, "quadrature"))
    assert np.array_equal(got[:3], _run(D, x[:3], N, "quadrature"))


def test_wav_envelope_channels(gdsp):
    W, F = gdsp.wav, gdsp.fft
    path = os.path.join(GOLDEN, "wav", "small.wav")
    with open(path, "rb") as f:
        w = W.New(f)
        C = w.NumChannels
        frames = min(w.Samples // C, 5000)
        dec = w.ReadFloats(frames * C).astype(np.float64)
    chans = np.stack([dec[c::C] for c in range(C)])
    for N in (None, 4096):
        with open(path, "rb") as f:
            got = W.EnvelopeChannels(W.New(f), frames, N)
        assert got.shape == (C, N or frames)
        assert np.array_equal(got, F.EnvelopeBatch(chans, N))
