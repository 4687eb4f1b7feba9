"""Stray reads and writes, and cross-talk between rows, of the device entries:
fft_batch, fft_real_batch, convolve_batch, fir_batch, fft2, fftn, fft_axis.

Many kernels run several transforms per workgroup; a store from an empty slot
of the last workgroup lands in the allocator's padding and nothing notices.
Here every input lives between NaN guard bands (a read outside the payload
that reaches a result gives a non-finite output), every output and every
caller-supplied work buffer, sized exactly as include/gdsp_fft.h documents,
between sentinel bands that must come back bit for bit (guarded.py). The
bands belong to the same allocation, so a stray access stays in owned memory.

Rows are uniform noise scaled by 10^(r mod 4), and every row is judged on its
own: conftest.row_nrel < 1e-13 against numpy.fft on the same rows (the
project's EXACT; the documented worst family error is 1.2e-14 of a row's
largest output, numpy's own about 1e-15). The value check is there to catch
cross-talk between rows of different level; roundoff is held in
test_accuracy_gpu.py. Bitwise equality of a row in a batch and alone is not
promised (exec_fourstep splits by batch) and not asked.

Batches: 1 and TPW + 1, TPW the transforms per workgroup of the kernel (tpws()
below restates the geometry of each family from the code); 1 and 3 where a
kernel has no such notion. Every band is at least TPW rows long (and two rows,
and 1024 elements), so the stores of a whole workgroup of empty slots would
still land inside it.
"""
import importlib
from collections import namedtuple

import numpy as np
import pytest

from conftest import row_nrel
from guarded import GUARD, NAN, guarded, pad_for
from test_accuracy_gpu import _smooth_m, algorithm

pytestmark = pytest.mark.gpu

EXACT = 1e-13


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


# smooth: whether a kind-3 plan must run the smooth-M kernels of chirpz6k.hpp
T = namedtuple("T", "kind n flags chirpz batches c6multi smooth",
               defaults=((), False, None, False, None))
NR = ("NO_RACE",)

TRANSFORMS = (
    [T(1, n) for n in (2, 16, 256, 2048, 4096, 16384)]
    # 2^17 on both sides of exec_fourstep's split by batch (batch * 16 <= 256)
    + [T(2, 1 << 15, batches=(1, 3)), T(2, 1 << 17, batches=(16, 17))]
    + [T(5, n) for n in (12, 375, 3000, 4095, 5000, 5400)]
    + [T(5, 3000, flags=("GENERIC_MIXED",))]
    + [T(6, n, batches=(1, 3)) for n in (10000, 8505, 9889, 20014)]
    # kind 3: bluestein_kernel forced on 100; c6_fft_multi (M = 768 = 16 3 16, five
    # transforms per workgroup) forced on 300; the smooth-M kernels; the power of 2
    # under CHIRPZ_POW2; the output parts
    + [T(3, 100, chirpz=True, smooth=False), T(3, 300, chirpz=True, c6multi=True, smooth=True),
       T(3, 2062, smooth=True), T(3, 3000, chirpz=True, smooth=True), T(3, 5003, smooth=True),
       T(3, 3000, flags=("CHIRPZ_POW2",), chirpz=True, smooth=False),
       T(3, 8209, smooth=False), T(3, 14563, smooth=False)]
    + [T(4, 16411, batches=(1, 2))]
    + [T(7, n, flags=NR) for n in (17, 257, 3001, 8161)]
    + [T(8, n, flags=NR) for n in (74, 481, 4097)]
)
KINDS = (1, 2, 3, 4, 5, 6, 7, 8)


def _tid(c):
    return "-".join(["k%d" % c.kind, str(c.n)] + list(c.flags) + (["cz"] if c.chirpz else []))


def test_every_kind_has_a_case():
    """test_transform asserts the plan kind of every case before it runs it."""
    assert {c.kind for c in TRANSFORMS} == set(KINDS)


def _need(n, radices):
    """Threads per transform that a radix list needs: a thread takes up to 16
    points of a pass (make_mixed_desc, plan.hip; FixedGeo::need, mixed_fixed.hpp)."""
    need = 1
    for r in radices:
        jmax = 1 if r > 16 else 16 // r
        need = max(need, (n // r + jmax - 1) // jmax)
    return need


def _fixed_tpw(need, lds_bytes_per_row):
    """FixedGeo::tpw / RaderGeo::tpw: about 256 threads within 64 KiB of LDS."""
    t = max(1, 256 // need)
    while t > 1 and t * lds_bytes_per_row > 65536:
        t -= 1
    return t


def tpws(p):
    """The transforms per workgroup of the kernels a plan may run (a kind-5
    plan: the compiled or runtime-compiled specialisation and the runtime-radix
    kernel, which the plan does not tell apart), empty where a kernel has no
    such notion."""
    n = p.n
    if p.kind == 1:    # Geo<>::TPW (fft_device.hpp): 256 threads, n / 16 per transform
        return [max(1, 256 // max(1, n // 16))]
    if p.kind == 5:
        need = _need(n, p.radices)
        t1 = 1
        while t1 < need:
            t1 *= 2
        t1 = t1 if t1 <= 64 else (need + 63) // 64 * 64
        # d.tpw (make_mixed_desc; kMixedMax = 4096) and FixedGeo::TPW
        return [max(1, min(256 // t1, 4096 // n)), _fixed_tpw(need, ((n + 7) & ~7) * 16)]
    if p.kind == 7:    # RaderGeo::TPW on the list of n - 1
        slots = (n + 7) & ~7
        return [_fixed_tpw(_need(n - 1, p.radices), (slots if n - 1 > 4096 else 2 * slots) * 8)]
    if p.kind == 3 and p.m % 256 == 0 and p.m // 256 <= 8 and p.m & (p.m - 1):
        return [256 // (p.m // 16)]  # C6Geo::TPW (chirpz6k.hpp): NA = M / 16 < 256
    if p.kind == 3 and p.m & (p.m - 1) == 0 and p.parts == 1:
        return [max(1, 256 // (p.m // 16))]  # bluestein_kernel: Geo<log2 M>::TPW
    return []


def _rows(seed, batch, n, real=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (batch, n))
    if not real:
        x = x + 1j * rng.uniform(-1, 1, (batch, n))
    return x * (10.0 ** (np.arange(batch) % 4))[:, None]


def _in(x, rows=2):
    """x on the device between NaN bands."""
    import torch
    return guarded(torch.from_numpy(np.array(x)).cuda(), NAN,
                   pad_for(x.shape[-1], rows))


def _out(shape, complex_=True, row=None, rows=2):
    """An output or work tensor of this shape between sentinel bands of
    `rows` rows of `row` elements (the last axis by default)."""
    import torch
    t = torch.full(tuple(shape), 7.0, dtype=torch.complex128 if complex_ else torch.float64,
                   device="cuda")
    return guarded(t, GUARD, pad_for(row or shape[-1], rows))


def _slots(n):
    """Rows a band holds for the entries that run power-of-2 kernels of n
    points with several rows per workgroup (Geo<>::TPW, as tpws() below)."""
    return max(2, 256 // max(1, n // 16)) if n & (n - 1) == 0 else 2


class Fails(list):
    def judge(self, what, got, ref, chks):
        import torch
        torch.cuda.synchronize()
        got = got.cpu().numpy() if hasattr(got, "cpu") else got
        try:
            for chk in chks:
                chk(what)
            assert np.isfinite(got).all(), "%s: non-finite output" % what
            err = row_nrel(got, ref)
            print("guard: %s %.3g" % (what, err))
            assert err < EXACT, "%s: %.3g" % (what, err)
        except AssertionError as e:
            self.append(str(e))

    def done(self):
        assert not self, "\n".join(self)


@pytest.mark.parametrize("c", TRANSFORMS, ids=_tid)
def test_transform(gdsp, D, c):
    n, fails = c.n, Fails()
    with algorithm(gdsp, c.flags):
        p = D.plan(n, c.chirpz)
        assert p.kind == c.kind, (n, p.kind)
        if n == 5400:
            assert p.runtime_compiled
        if c.c6multi:  # c6_fft_multi: RB = M / 256 <= 8
            assert _smooth_m(gdsp, p) and p.m // 256 <= 8 and tpws(p)[0] > 1, p.m
        if c.smooth is not None:
            assert _smooth_m(gdsp, p) == c.smooth, (n, p.m)
        if n in (8209, 14563):
            assert p.parts > 1
        ts = [t for t in tpws(p) if t > 1]
        batches = c.batches or ((1,) + tuple(sorted({t + 1 for t in ts})) if ts else (1, 3))
        band = max([2] + ts)
        for batch in batches:
            x = _rows(n + batch, batch, n)
            ref = np.fft.fft(x, axis=1)
            tag = "%s b%d " % (_tid(c), batch)
            # out of place
            xd, cx = _in(x, band)
            out, co = _out(x.shape, rows=band)
            D.fft_batch(xd, out=out, chirpz=c.chirpz)
            fails.judge(tag + "forward", out, ref, (cx, co))
            # in place: one buffer, NaN on both sides of it
            xd, cx = _in(x, band)
            D.fft_batch(xd, out=xd, chirpz=c.chirpz)
            fails.judge(tag + "in-place", xd, ref, (cx,))
            # real input
            xr = _rows(n + batch + 1, batch, n, real=True)
            xd, cx = _in(xr, band)
            out, co = _out(x.shape, rows=band)
            D.fft_real_batch(xd, out=out, chirpz=c.chirpz)
            fails.judge(tag + "real", out, np.fft.fft(xr, axis=1), (cx, co))
        # one inverse, the larger batch
        xd, cx = _in(x, band)
        out, co = _out(x.shape, rows=band)
        D.fft_batch(xd, out=out, inverse=True, chirpz=c.chirpz)
        fails.judge(tag + "inverse", out, np.fft.ifft(x, axis=1), (cx, co))
    fails.done()


# ---- Convolve -----------------------------------------------------------------------
# fused: 16 rows per workgroup at 256, one at 4096; composed: 3000

@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "perrow"])
@pytest.mark.parametrize("n,batch,fused", [(256, 17, True), (4096, 2, True), (3000, 3, False)])
def test_convolve(D, n, batch, fused, per_row):
    assert D.convolve_fused(n) == fused
    fails = Fails()
    x = _rows(n, batch, n)
    y = _rows(n + 1, batch if per_row else 1, n)
    ref = np.fft.ifft(np.fft.fft(x, axis=1) * np.fft.fft(y, axis=1), axis=1)
    tag = "convolve %d x %d %s " % (n, batch, "perrow" if per_row else "shared")
    band = _slots(n)
    for in_place in (False, True):
        xd, cx = _in(x, band)
        yd, cy = _in(y if per_row else y[0], band)
        # work: exactly y's size
        work, cw = _out(yd.shape, row=n, rows=band)
        out, co = (xd, cx) if in_place else _out(x.shape, rows=band)
        D.convolve_batch(xd, yd, out=out, work=work)
        fails.judge(tag + ("in-place" if in_place else "forward"), out, ref, (cx, cy, cw, co))
    fails.done()


# ---- FIR ----------------------------------------------------------------------------

def _fir_ref(x, h):
    return np.stack([np.convolve(x[c].astype(np.longdouble),
                                 (h if h.ndim == 1 else h[c]).astype(np.longdouble))
                     .astype(np.float64) for c in range(x.shape[0])])


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "perrow"])
@pytest.mark.parametrize("F,channels,n,m,fused", [(256, 17, 300, 9, True),
                                                  (32768, 2, 40000, 100, False)])
def test_fir(gdsp, D, F, channels, n, m, fused, per_row):
    """work of exactly the documented size: 16 F h_rows bytes for the taps'
    spectra, and in the composed form 16 F min(T, max(1, 2^24 / F)) more, T =
    channels * ceil(ceil(output length / (F - m + 1)) / 2)."""
    assert gdsp.fft.fir_block(m, F) == (F, fused)
    fails = Fails()
    x = _rows(F + channels, channels, n, real=True)
    h = np.random.default_rng(m).standard_normal((channels, m) if per_row else (m,))
    h_rows = channels if per_row else 1
    ref = _fir_ref(x, h)
    for full in (False, True):
        out_len = n + m - 1 if full else n
        blocks = -(-out_len // (F - m + 1))
        total = channels * ((blocks + 1) // 2)
        rows = h_rows + (0 if fused else min(total, max(1, (1 << 24) // F)))
        xd, cx = _in(x)
        hd, ch = _in(h)
        work, cw = _out((rows * F,), row=F, rows=_slots(F))
        out, co = _out((channels, out_len), complex_=False)
        D.fir_batch(xd, hd, out=out, full=full, block=F, work=work)
        fails.judge("fir F=%d x %d %s %s" % (F, channels, "perrow" if per_row else "shared",
                                             "full" if full else "causal"),
                    out, ref[:, :out_len], (cx, ch, cw, co))
    fails.done()


# ---- FFT2, FFTN, one axis -------------------------------------------------------------

def _nd(shape):
    rng = np.random.default_rng(list(shape))
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


def _flat(a):
    return np.asarray(a).reshape(1, -1)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("shape", [(64, 48), (37, 41), (1024, 20)], ids=str)
def test_fft2(D, shape, inverse):
    fails = Fails()
    x = _nd(shape)
    ref = (np.fft.ifft2 if inverse else np.fft.fft2)(x)
    for given in (True, False):
        xd, cx = _in(x)
        out, co = _out(shape)
        chks = [cx, co]
        work = None
        if given:  # exactly rows * cols
            work, cw = _out((shape[0] * shape[1],), row=shape[1])
            chks.append(cw)
        D.fft2(xd, out=out, inverse=inverse, work=work)
        fails.judge("fft2 %s %s" % (shape, "work" if given else "no work"), _flat(out.cpu().numpy()),
                    _flat(ref), chks)
    fails.done()


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_fftn(D, inverse):
    fails = Fails()
    x = _nd((8, 6, 5))
    xd, cx = _in(x, rows=30)
    out, co = _out(x.shape, row=30)
    D.fftn(xd, out=out, inverse=inverse)
    fails.judge("fftn 8x6x5", _flat(out.cpu().numpy()),
                _flat((np.fft.ifftn if inverse else np.fft.fftn)(x)), (cx, co))
    fails.done()


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_fft_axis(D, inverse):
    fails = Fails()
    x = _nd((3, 1024, 7))
    xd, cx = _in(x, rows=1024)
    out, co = _out(x.shape, row=7 * 1024)
    D.fft_axis(xd, 1, out=out, inverse=inverse)
    ref = (np.fft.ifft if inverse else np.fft.fft)(x, axis=1)
    # every line along the axis is a row of its own
    got = np.moveaxis(out.cpu().numpy(), 1, -1).reshape(-1, 1024)
    fails.judge("fft_axis 3x1024x7 axis 1", got, np.moveaxis(ref, 1, -1).reshape(-1, 1024),
                (cx, co))
    fails.done()
