"""Every host chunk loop and persistent-worker loop past its first iteration.

Between the C ABI and the kernels a call is cut into pieces in about a dozen
places: workers that take several segment pairs, launches of at most so many
channels, chunks of at most so many transforms, pieces of 65535 rows. The
rest of the suite stays inside the first piece of almost all of them. Each
test here runs the smallest valid call that reaches the second piece, reads
gdsp_loop_stats before and after it and asserts that the counter it targets
moved (seams.py derives the shapes from the code's constants; a constant
restated wrongly fails here instead of passing on the first iteration).

References and bounds are the suite's own: for the Welch family numpy's rfft
of the exact segments summed per bin in np.longdouble (seams.py, proved on
the CPU in test_seams_host.py) at 1e-13 (test_segment_ranges_gpu.EXACT); for
transforms numpy on the compared rows at 1e-13 (test_guard_bands_gpu.EXACT);
for FIR np.convolve in extended precision at test_fir_gpu.EXACT. Where a row
must not depend on where the cut falls, it is compared bit for bit with the
same row in a call that the cut does not reach. Inputs are uniform or
Gaussian noise; segment counts are odd.
"""
import ctypes
import importlib

import numpy as np
import pytest

import seams as S
import test_guard_bands_gpu as G
import test_segment_ranges_gpu as R
from conftest import row_nrel
from guarded import GUARD, guarded, pad_for
from test_accuracy_gpu import algorithm
from test_fir_gpu import EXACT as FIR_EXACT

pytestmark = pytest.mark.gpu

EXACT = S.EXACT
assert EXACT == R.EXACT == G.EXACT == FIR_EXACT


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


class Counted:
    """gdsp_loop_stats around a block: .later and .multi are what it added."""

    def __init__(self, gdsp):
        self.stats = gdsp.fft.LoopStats

    def __enter__(self):
        self.before = self.stats()
        return self

    def __exit__(self, *exc):
        after = self.stats()
        self.later = after["later_chunks"] - self.before["later_chunks"]
        self.multi = after["multi_unit_launches"] - self.before["multi_unit_launches"]
        return False


def rows_err(got, ref):
    """conftest.row_nrel (worst row, normwise and max|d| / max|ref|), vectorised
    for tens of thousands of rows."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    d = got - ref
    e1 = np.linalg.norm(d, axis=1) / np.linalg.norm(ref, axis=1)
    e2 = np.abs(d).max(axis=1) / np.abs(ref).max(axis=1)
    return float(max(e1.max(), e2.max()))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def zeros(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.float64, device="cuda")


def host_finalize(gdsp, acc, nsegs, nfft, pad, win_nfft, fs):
    """gdsp_pwelch_finalize of a host accumulator."""
    L = gdsp._lib
    acc = np.ascontiguousarray(acc)
    lp = pad // 2 + 1
    pxx, freqs = np.empty(lp), np.empty(lp)
    wn = np.ascontiguousarray(win_nfft)
    L.check(L.lib().gdsp_pwelch_finalize(acc.ctypes.data_as(L._P), acc.size, nsegs, nfft, pad,
                                         wn.ctypes.data_as(L._P), float(fs), 0,
                                         pxx.ctypes.data_as(L._P), freqs.ctypes.data_as(L._P)),
            "pwelch_finalize")
    return pxx


def check_sums(gdsp, what, acc, x, nfft, flen, stride, a, b, win):
    """The folded accumulator against welch_sums of [a, b), and the spectrum
    gdsp_pwelch_finalize makes of it against the finalised reference."""
    got = acc.cpu().numpy()
    assert np.isfinite(got).all(), what
    total = S.welch_sums(x, nfft, flen, stride, a, b, win)
    err = row_nrel(S.fold(got), S.unfold(total, flen).astype(np.float64))
    pad = flen
    wn = S.hamming(nfft)
    pxx = host_finalize(gdsp, got, b - a, nfft, pad, wn, 48000.0)
    errf = row_nrel(pxx, S.finalize(total, b - a, nfft, pad, wn, 48000.0).astype(np.float64))
    print("seams: %s: sums %.3g, finalised %.3g" % (what, err, errf))
    assert err < EXACT and errf < EXACT, (what, err, errf)


# ---- A. worker loops ------------------------------------------------------------------

def _list_tpw(p, f):
    """FixedGeo::TPW (mixed_fixed.hpp; fixed_geo, mixed_jit.hip) of the list the
    fused Pwelch of f runs: its own where it has one, else the plan's."""
    rad = S.PW_LISTS.get(f, p.radices)
    return G._fixed_tpw(G._need(f, rad), ((f + 7) & ~7) * 16)


@pytest.mark.parametrize("c", S.worker_cases(), ids=S.worker_id)
def test_worker_loop(gdsp, D, c):
    """npairs = 2048 * workers per workgroup + 1: every worker but the last
    runs two pairs (accumulators and the half-overlap carry go from one to the
    next), the last runs one pair of one segment."""
    f, nov = max(c.pad, c.nfft), c.nfft - c.stride
    with algorithm(gdsp, c.flags):
        p = D.plan(f)
        tpw = c.tpw or _list_tpw(p, f)
        nseg = S.worker_nseg(tpw)
        n = S.signal_len(nseg, c.nfft, c.stride)
        R._assert_path(gdsp, D, R.Case(c.path, c.nfft, nov, c.pad, c.flags), n)
        x = S.noise([c.nfft, c.stride, f], n)
        win = S.hamming(f)
        acc = zeros(f)
        with Counted(gdsp) as k:
            D.pwelch_accumulate(dev(x), c.nfft, f, nov, 0, nseg, dev(win), acc)
        what = "%s tpw %d, %d segments" % (S.worker_id(c), tpw, nseg)
        print("seams: %s: multi-unit launches +%d, later chunks +%d" % (what, k.multi, k.later))
        assert (k.multi, k.later) == (1, 0), (what, k.multi, k.later)
        check_sums(gdsp, what, acc, x, c.nfft, f, c.stride, 0, nseg, win)


@pytest.mark.parametrize("nfft,f", [(60, 64), (2000, 2048)])
def test_wave_masked_loop(gdsp, D, nfft, f):
    """The wave kernels' PAD variant (Pad > NFFT: the masked load loop) at
    stride 3 with ngroups = target + 1: two groups per worker, the last worker
    one group of one pair of one segment."""
    nseg, stride = S.wave_nseg(f), 3
    n = S.signal_len(nseg, nfft, stride)
    R._assert_path(gdsp, D, R.Case("wave", nfft, nfft - stride, f), n)
    x, win, acc = S.noise([nfft, f], n), S.hamming(f), zeros(f)
    with Counted(gdsp) as k:
        D.pwelch_accumulate(dev(x), nfft, f, nfft - stride, 0, nseg, dev(win), acc)
    what = "wave %d pad %d, %d segments" % (nfft, f, nseg)
    print("seams: %s: multi-unit launches +%d" % (what, k.multi))
    assert (k.multi, k.later) == (1, 0), (what, k.multi, k.later)
    check_sums(gdsp, what, acc, x, nfft, f, stride, 0, nseg, win)


def _odd_ld(n):
    return n + 1 if n % 2 == 0 else n + 2


def _wide(seed, channels, n):
    """(device view (channels, n) at an odd row stride, host rows)."""
    import torch
    ld = _odd_ld(n)
    buf = torch.full((channels, ld), float("nan"), dtype=torch.float64, device="cuda")
    x = S.noise(seed, channels, n)
    buf[:, :n] = dev(x)
    return buf[:, :n], x


@pytest.mark.parametrize("f", [64, 2048])
def test_batched_pwelch_groups(gdsp, D, f):
    """pwelch_batch_geometry (pwelch_batch.hip): 3 channels share the target
    (2048 waves, 1024 two-wave workers at 2048), so want = target / 3 workers
    a channel; one group more gives gpw = 2."""
    channels, stride = 3, 3
    s, target = S.wave_groups(f)
    npairs = (target // channels) * s + 1
    nseg = 2 * npairs - 1
    n = S.signal_len(nseg, f, stride)
    assert gdsp.spectral.pwelch_batch_fused(channels, n, f, 0, f - stride)
    xd, x = _wide([f, 1], channels, n)
    win, acc = S.hamming(f), zeros(channels, f)
    with Counted(gdsp) as k:
        D.pwelch_batch_accumulate(xd, f, f, f - stride, 0, nseg, dev(win), acc)
    print("seams: batched Pwelch %d, %d segments: multi-unit launches +%d" % (f, nseg, k.multi))
    assert (k.multi, k.later) == (1, 0), (k.multi, k.later)
    for ch in range(channels):
        check_sums(gdsp, "batched Pwelch %d channel %d" % (f, ch), acc[ch], x[ch], f, f, stride,
                   0, nseg, win)


def _check_cross(what, acc, x, y, nfft, f, stride, a, b, win):
    """acc (channels, 4, hb) against cross_sums, plane by plane; returns the
    reference (channels, 4, hb) in extended precision."""
    got = acc.cpu().numpy()
    assert np.isfinite(got).all(), what
    ref = np.stack([S.cross_sums(x[ch], y if y.ndim == 1 else y[ch], nfft, f, stride, a, b, win)
                    for ch in range(x.shape[0])])
    errs = [rows_err(got[:, pl], ref[:, pl].astype(np.float64)) for pl in range(4)]
    print("seams: %s: Sxx %.3g Syy %.3g Re Sxy %.3g Im Sxy %.3g" % ((what,) + tuple(errs)))
    assert max(errs) < EXACT, (what, errs)
    return ref


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared-y", "y-per-channel"])
@pytest.mark.parametrize("f", [64, 2048])
def test_batched_cpsd_groups(gdsp, D, f, per_channel):
    """cpsd_batch_geometry (cpsd_batch.hip): groups of S segments, want =
    target / 3 workers a channel; one group more gives gpw = 2."""
    channels, stride = 3, 3
    s, target = S.wave_groups(f)
    nseg = (target // channels) * s + 1
    nseg += 1 - nseg % 2  # odd
    n = S.signal_len(nseg, f, stride)
    assert gdsp.spectral.cpsd_batch_fused(channels, n, f, 0, f - stride)
    xd, x = _wide([f, 2], channels, n)
    yd, y = _wide([f, 3], channels if per_channel else 1, n)
    if not per_channel:
        yd, y = yd[0], y[0]
    win, acc = S.hamming(f), zeros(channels, 4, f // 2 + 1)
    with Counted(gdsp) as k:
        D.cpsd_batch_accumulate(xd, yd, f, f, f - stride, 0, nseg, dev(win), acc)
    print("seams: batched Cpsd %d, %d segments: multi-unit launches +%d" % (f, nseg, k.multi))
    assert (k.multi, k.later) == (1, 0), (k.multi, k.later)
    _check_cross("batched Cpsd %d" % f, acc, x, y, f, f, stride, 0, nseg, win)


# ---- B. chunk loops -------------------------------------------------------------------

@pytest.mark.parametrize("m", S.MATERIALISED, ids=lambda m: m.name)
def test_materialised_pwelch_chunks(gdsp, D, m):
    """The r0 loop of the materialised Pwelch (welch.hip): one pair more than
    a chunk holds, so the second chunk starts at segment seg_begin + 2 rows."""
    f, stride = max(m.pad, m.nfft), m.nfft - m.nov
    n = S.signal_len(m.nseg, m.nfft, stride)
    R._assert_path(gdsp, D, R.Case("materialised", m.nfft, m.nov, m.pad), n)
    x, win = S.noise([m.nfft, f], n), S.hamming(f)
    xd, wd = dev(x), dev(win)
    ranges = [(0, m.nseg)]
    if m.name.startswith("a-"):
        # an odd seg_begin, the range still one pair longer than a chunk
        ranges.append((1, m.nseg))
    for a, b in ranges:
        rows = S.materialised_rows(f, 1 << 40)
        assert rows < (b - a + 1) // 2 <= rows + 2  # two chunks
        acc = zeros(f)
        with Counted(gdsp) as k:
            D.pwelch_accumulate(xd, m.nfft, f, m.nov, a, b, wd, acc)
        what = "materialised %s [%d, %d)" % (m.name, a, b)
        print("seams: %s: later chunks +%d" % (what, k.later))
        assert (k.later, k.multi) == (1, 0), (what, k.later, k.multi)
        check_sums(gdsp, what, acc, x, m.nfft, f, stride, a, b, win)


def _cpsd_finalize(gdsp, D, acc, channels, f, nsegs, nfft, win_nfft, fs):
    """gdsp_cpsd_batch_finalize_device of acc: (Pxy, Pxx, Pyy, Cxy) as numpy."""
    import torch
    L = gdsp._lib
    lp = f // 2 + 1
    pxy = torch.empty((channels, lp), dtype=torch.complex128, device="cuda")
    outs = [torch.empty((channels, lp), dtype=torch.float64, device="cuda") for _ in range(3)]
    wn = np.ascontiguousarray(win_nfft)
    freqs = np.empty(lp)
    L.check(L.lib().gdsp_cpsd_batch_finalize_device(
        D._ptr(acc), channels, f, nsegs, nfft, f, wn.ctypes.data_as(L._P), float(fs), 0,
        D._ptr(pxy), D._ptr(outs[0]), D._ptr(outs[1]), D._ptr(outs[2]),
        freqs.ctypes.data_as(L._P), D._stream_ptr(None, acc.device)), "cpsd_batch_finalize")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in [pxy] + outs]


CPSD_MAT = [("c0-shared-y", 7, 300, False), ("c0-y-per-channel", 7, 300, True),
            ("j0", 2, 1025 + 40, True)]


@pytest.mark.parametrize("name,channels,nseg,per_channel", CPSD_MAT, ids=[c[0] for c in CPSD_MAT])
def test_materialised_cpsd_chunks(gdsp, D, name, channels, nseg, per_channel):
    """The c0 and j0 loops of the materialised Cpsd (welch.hip) at Pad 32768:
    1024 rows a chunk, so 300 segments go 3 channels a launch (7 channels: 3,
    3, 1) and 1065 segments go one channel a launch in runs of 1024 and 41."""
    nfft, f, stride = 100, 32768, 3
    maxrows = (1 << S.MAT_BYTES_LOG2) // f
    ns_max = min(nseg, maxrows)
    cpl = min(maxrows // ns_max, channels)
    launches, runs = -(-channels // cpl), -(-nseg // ns_max)
    assert (cpl, launches, runs) == ((3, 3, 1) if channels == 7 else (1, 2, 2))
    n = S.signal_len(nseg, nfft, stride)
    assert not gdsp.spectral.cpsd_batch_fused(channels, n, nfft, f, nfft - stride)
    xd, x = _wide([nseg, 1], channels, n)
    yd, y = _wide([nseg, 2], channels if per_channel else 1, n)
    if not per_channel:
        yd, y = yd[0], y[0]
    win, acc = S.hamming(f), zeros(channels, 4, f // 2 + 1)
    with Counted(gdsp) as k:
        D.cpsd_batch_accumulate(xd, yd, nfft, f, nfft - stride, 0, nseg, dev(win), acc)
    print("seams: materialised Cpsd %s: later chunks +%d" % (name, k.later))
    assert (k.later, k.multi) == (launches - 1 + launches * (runs - 1), 0), (k.later, k.multi)
    ref = _check_cross("materialised Cpsd " + name, acc, x, y, nfft, f, stride, 0, nseg, win)
    # the coherence after finalise: |Sxy|^2 / (Sxx Syy)
    wn = S.hamming(nfft)
    pxy, pxx, pyy, coh = _cpsd_finalize(gdsp, D, acc, channels, f, nseg, nfft, wn, 48000.0)
    want = ((ref[:, 2] ** 2 + ref[:, 3] ** 2) / (ref[:, 0] * ref[:, 1])).astype(np.float64)
    err = rows_err(coh, want)
    scale = np.stack([S.finalize(np.ones(f // 2 + 1, S.LD), nseg, nfft, f, wn, 48000.0)] * channels)
    errx = rows_err(pxx, (ref[:, 0] * scale).astype(np.float64))
    errxy = rows_err(pxy, ((ref[:, 2] + 1j * ref[:, 3]) * scale).astype(np.complex128))
    print("seams: materialised Cpsd %s: coherence %.3g, Pxx %.3g, Pxy %.3g"
          % (name, err, errx, errxy))
    assert max(err, errx, errxy) < EXACT, (err, errx, errxy)


def _batch_sums(x, ld, channels, nfft, stride, nseg, win):
    """welch_sums of every row of a host buffer with rows ld apart:
    (channels, nfft / 2 + 1) float64."""
    v = np.lib.stride_tricks.as_strided(x, (channels, nseg, nfft), (ld * 8, stride * 8, 8),
                                        writeable=False)
    out = np.empty((channels, nfft // 2 + 1))
    step = max(1, (1 << 22) // (nseg * nfft))
    for lo in range(0, channels, step):
        spec = np.fft.rfft(v[lo:lo + step] * win, axis=2)
        out[lo:lo + step] = (spec.real * spec.real + spec.imag * spec.imag).sum(axis=1, dtype=S.LD)
    return out


@pytest.mark.parametrize("f,extra", [(64, 5), (2048, 3)])
def test_fused_batched_pwelch_channel_chunks(gdsp, D, f, extra):
    """The c0 loop of the fused batched Pwelch (welch.hip): 3 segments a
    channel leave `rows` partial rows of f doubles each, and 2^26 doubles of
    partials hold cpl channels; `extra` channels more take a second launch
    whose x and acc start c0 rows further. Every channel is compared, and the
    rows around the cut are bit for bit what they are in the first launch of a
    call of 1024 channels (at 1024 channels and more a channel has one worker,
    so the order of its sums is the same)."""
    nseg = 3
    stride = 3 if f == 64 else f // 2
    s, target = S.wave_groups(f)
    ngroups = -(-((nseg + 1) // 2) // s)
    gpw = ngroups  # want = max(1, target / channels) = 1 worker a channel
    rows = 1 * s
    cpl = (1 << S.PARTIALS_LOG2) // (rows * f)
    assert cpl == (65536 if f == 64 else 32768)
    channels = cpl + extra
    n = S.signal_len(nseg, f, stride)
    ld = _odd_ld(n)
    assert gdsp.spectral.pwelch_batch_fused(channels, n, f, 0, f - stride)
    import torch
    buf = torch.empty((channels, ld), dtype=torch.float64, device="cuda")
    D.fill_uniform(buf, 0x5EA + f)
    xd = buf[:, :n]
    win = S.hamming(f)
    wd, acc = dev(win), zeros(channels, f)
    with Counted(gdsp) as k:
        D.pwelch_batch_accumulate(xd, f, f, f - stride, 0, nseg, wd, acc)
    print("seams: fused batched Pwelch %d x %d: later chunks +%d, multi-unit launches +%d"
          % (f, channels, k.later, k.multi))
    assert (k.later, k.multi) == (1, 2 if gpw >= 2 else 0), (k.later, k.multi)
    got = acc.cpu().numpy()
    assert np.isfinite(got).all()
    ref = _batch_sums(buf.cpu().numpy(), ld, channels, f, stride, nseg, win)
    err = rows_err(S.fold(got), S.unfold(ref, f))
    print("seams: fused batched Pwelch %d x %d: sums %.3g" % (f, channels, err))
    assert err < EXACT, err
    lo = channels - 1024
    acc2 = zeros(1024, f)
    with Counted(gdsp) as k2:
        D.pwelch_batch_accumulate(xd[lo:lo + 1024], f, f, f - stride, 0, nseg, wd, acc2)
    assert k2.later == 0
    assert torch.equal(acc[lo:lo + 1024].view(torch.int64), acc2.view(torch.int64))


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared-y", "y-per-channel"])
def test_fused_batched_cpsd_channel_chunks(gdsp, D, per_channel):
    """The c0 loop of the fused Cpsd (welch.hip) at F = 64: 3 segments leave
    16 partial rows of 4 * 33 doubles a channel, so 2^26 / 2112 = 31775
    channels a launch; 3 more take a second launch."""
    import torch
    f, nseg, stride = 64, 3, 3
    s, _ = S.wave_groups(f)
    hb = f // 2 + 1
    cpl = (1 << S.PARTIALS_LOG2) // (s * 4 * hb)
    assert cpl == 31775
    channels = cpl + 3
    n = S.signal_len(nseg, f, stride)
    ld = _odd_ld(n)
    assert gdsp.spectral.cpsd_batch_fused(channels, n, f, 0, f - stride)
    bx = torch.empty((channels, ld), dtype=torch.float64, device="cuda")
    by = torch.empty((channels if per_channel else 1, ld + 2), dtype=torch.float64, device="cuda")
    D.fill_uniform(bx, 0xC5D)
    D.fill_uniform(by, 0xC5E)
    xd, yd = bx[:, :n], (by[:, :n] if per_channel else by[0, :n])
    win = S.hamming(f)
    wd, acc = dev(win), zeros(channels, 4, hb)
    with Counted(gdsp) as k:
        D.cpsd_batch_accumulate(xd, yd, f, f, f - stride, 0, nseg, wd, acc)
    print("seams: fused batched Cpsd 64 x %d: later chunks +%d" % (channels, k.later))
    assert (k.later, k.multi) == (1, 0), (k.later, k.multi)
    # every channel: the spectra of its 3 segments against those of y's
    hx, hy = bx.cpu().numpy(), by.cpu().numpy()
    X = np.fft.rfft(np.lib.stride_tricks.as_strided(hx, (channels, nseg, f), (ld * 8, 24, 8)) * win,
                    axis=2)
    Y = np.fft.rfft(np.lib.stride_tricks.as_strided(
        hy, (hy.shape[0], nseg, f), ((ld + 2) * 8, 24, 8)) * win, axis=2)
    ref = np.stack([(np.abs(X) ** 2).sum(axis=1, dtype=S.LD),
                    np.broadcast_to((np.abs(Y) ** 2).sum(axis=1, dtype=S.LD), (channels, hb)),
                    (X.real * Y.real + X.imag * Y.imag).sum(axis=1, dtype=S.LD),
                    (X.real * Y.imag - X.imag * Y.real).sum(axis=1, dtype=S.LD)], axis=1)
    got = acc.cpu().numpy()
    assert np.isfinite(got).all()
    errs = [rows_err(got[:, pl], ref[:, pl].astype(np.float64)) for pl in range(4)]
    print("seams: fused batched Cpsd 64 x %d: Sxx %.3g Syy %.3g Re Sxy %.3g Im Sxy %.3g"
          % ((channels,) + tuple(errs)))
    assert max(errs) < EXACT, errs
    # the rows around the cut, bit for bit, in a call the cut does not reach
    lo = channels - 1024
    acc2 = zeros(1024, 4, hb)
    D.cpsd_batch_accumulate(xd[lo:lo + 1024], yd[lo:lo + 1024] if per_channel else yd, f, f,
                            f - stride, 0, nseg, wd, acc2)
    assert torch.equal(acc[lo:lo + 1024].view(torch.int64), acc2.view(torch.int64))


def test_batched_pwelch_fallback_loop(gdsp, D):
    """The channel loop of gdsp_pwelch_batch_accumulate_device where it has no
    fused kernel (4096): channel c reads x + c ldx and adds into acc + c flen,
    bit for bit what the single-signal call gives."""
    import torch
    f, nseg, channels = 4096, 5, 5
    n = S.signal_len(nseg, f, f // 2)
    assert not gdsp.spectral.pwelch_batch_fused(channels, n, f, 0, f // 2)
    xd, x = _wide(4096, channels, n)
    win = S.hamming(f)
    wd, acc = dev(win), zeros(channels, f)
    with Counted(gdsp) as k:
        D.pwelch_batch_accumulate(xd, f, f, f // 2, 0, nseg, wd, acc)
    print("seams: batched Pwelch fallback: later chunks +%d" % k.later)
    assert (k.later, k.multi) == (channels - 1, 0), (k.later, k.multi)
    for ch in range(channels):
        one = zeros(f)
        D.pwelch_accumulate(xd[ch].contiguous(), f, f, f // 2, 0, nseg, wd, one)
        assert torch.equal(acc[ch].view(torch.int64), one.view(torch.int64)), ch
        check_sums(gdsp, "fallback channel %d" % ch, acc[ch], x[ch], f, f, f // 2, 0, nseg, win)


@pytest.mark.parametrize("full", [False, True], ids=["causal", "full"])
@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "perrow"])
def test_composed_fir_chunks(gdsp, D, per_row, full):
    """The g0 loop of the composed FIR (fir_rows, gdsp_api.hip): block 32768
    gives 2^24 / 32768 = 512 transforms a chunk; 3 channels of 171 are 513, so
    the second chunk is the last transform of the last channel, and with taps
    per row the multiply runs are cut there. n: 341 blocks of L = F - m + 1
    outputs a channel, the last of 1000 samples.

    np.convolve in extended precision covers the first outputs, the first
    block boundary and the last 3000 outputs of every channel (the second
    chunk's among them); every channel whole is bit for bit that channel run
    alone (171 transforms: one chunk)."""
    import torch
    F, m, channels = 32768, 100, 3
    assert gdsp.fft.fir_block(m, F) == (F, False)
    rows = (1 << S.FIR_CHUNK_LOG2) // F
    L = F - m + 1
    tpr = rows // channels + 1
    n = (2 * tpr - 2) * L + 1000
    out_len = n + m - 1 if full else n
    assert -(-out_len // L) == 2 * tpr - 1 and (tpr, channels * tpr) == (171, rows + 1)
    x = torch.empty((channels, n), dtype=torch.float64, device="cuda")
    D.fill_uniform(x, 0xF1)
    h = np.random.default_rng(m).standard_normal((channels, m) if per_row else (m,))
    hd = dev(h)
    h_rows = channels if per_row else 1
    alone = [D.fir_batch(x[c:c + 1], hd[c] if per_row else hd, full=full, block=F)
             for c in range(channels)]
    work, chk = guarded(torch.zeros((h_rows + rows) * F, dtype=torch.complex128, device="cuda"),
                        GUARD, pad_for(F, 2))
    wins = [(0, 3000), (L - 1500, L + 1500), (out_len - 3000, out_len)]
    for given in (True, False):
        with Counted(gdsp) as k:
            out = D.fir_batch(x, hd, full=full, block=F, work=work if given else None)
        torch.cuda.synchronize()
        chk("fir work")
        tag = "composed FIR %s %s %s" % ("perrow" if per_row else "shared",
                                         "full" if full else "causal", "work" if given else "no work")
        print("seams: %s: later chunks +%d" % (tag, k.later))
        assert (k.later, k.multi) == (1, 0), (tag, k.later, k.multi)
        worst = 0.0
        for c in range(channels):
            assert torch.equal(out[c].view(torch.int64), alone[c][0].view(torch.int64)), (tag, c)
            hc = (h[c] if per_row else h).astype(S.LD)
            for lo, hi in wins:
                start = max(0, lo - m + 1)
                xs = x[c, start:min(n, hi)].cpu().numpy().astype(S.LD)
                want = np.convolve(xs, hc)[lo - start:hi - start].astype(np.float64)
                worst = max(worst, row_nrel(out[c, lo:hi].cpu().numpy(), want))
        print("seams: %s: %.3g" % (tag, worst))
        assert worst < FIR_EXACT, (tag, worst)


AXIS = [((65537, 16, 3), "one column kernel", 1), ((65537, 1024, 2), "split columns", 1),
        ((65537, 3, 2), "transposes", 2)]


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("shape,branch,later", AXIS, ids=[a[1].replace(" ", "-") for a in AXIS])
def test_fft_axis_outer_pieces(gdsp, D, shape, branch, later, inverse):
    """The o0 loops of fft_axis (gdsp_api.hip): 65537 outer indices are pieces
    of 65535 and 2, in the column kernel (L = 16), the four-step column split
    (L = 1024 = 32 * 32; 2 GiB a buffer) and the transposes around the row
    kernels (L = 3). Lines at both ends, on both sides of the cut and at 8
    random outer indices against numpy; Parseval for every line on the device."""
    import torch
    outer, L, inner = shape
    x = torch.empty(shape, dtype=torch.complex128, device="cuda")
    D.fill_uniform(x, 0xA15 + L)
    with Counted(gdsp) as k:
        out = D.fft_axis(x, 1, inverse=inverse)
    torch.cuda.synchronize()
    print("seams: fft_axis %s (%s): later chunks +%d" % (shape, branch, k.later))
    assert k.later >= later and k.multi == 0, (k.later, k.multi)
    pick = sorted({0, 1, 65534, 65535, 65536} |
                  set(np.random.default_rng(L).integers(2, 65534, 8).tolist()))
    idx = torch.tensor(pick, device="cuda")
    got = np.moveaxis(out[idx].cpu().numpy(), 1, -1).reshape(-1, L)
    src = np.moveaxis(x[idx].cpu().numpy(), 1, -1).reshape(-1, L)
    ref = (np.fft.ifft if inverse else np.fft.fft)(src, axis=1)
    err = row_nrel(got, ref)
    # Parseval: sum |X|^2 = L sum |x|^2 forward, / L inverse, per line
    ein = (x.real ** 2 + x.imag ** 2).sum(dim=1)
    eout = (out.real ** 2 + out.imag ** 2).sum(dim=1)
    pars = float(((eout * (L if inverse else 1.0 / L) - ein).abs() / ein).max())
    print("seams: fft_axis %s %s: lines %.3g, Parseval %.3g"
          % (shape, "inverse" if inverse else "forward", err, pars))
    assert err < EXACT and pars < EXACT, (err, pars)


def test_four_step_mixed_row_pieces(gdsp, D):
    """The b0 loops of the mixed four-step executors (plan kind 6,
    gdsp_api.hip): 65537 rows in place are pieces of 65535 and 2. The smallest
    such length above 8192 is found by search. (Kinds 2 and 4 reach their b0
    loops only at 65536 rows of 2^15 points and more, above 100 GB with the
    scratch: not covered.)"""
    import torch
    n = next((n for n in range(8193, 8449) if D.Plan(n).kind == 6), None)
    assert n is not None, "no kind-6 length in (8192, 8448]"
    batch = 65537
    need = 2 * batch * n * 16  # the rows and the executor's scratch
    free = torch.cuda.mem_get_info()[0]
    if free < 2 * need:
        pytest.skip("kind 6 at %d x %d needs %d bytes, %d free" % (batch, n, need, free))
    x = torch.empty((batch, n), dtype=torch.complex128, device="cuda")
    D.fill_uniform(x, 0x6B0)
    pick = [0, 65534, 65535, 65536]
    src = x[pick].cpu().numpy()
    ein = (x.real ** 2 + x.imag ** 2).sum(dim=1)
    with Counted(gdsp) as k:
        D.fft_batch(x, out=x)
    torch.cuda.synchronize()
    print("seams: kind 6 n = %d x %d in place: later chunks +%d" % (n, batch, k.later))
    assert k.later >= 1 and k.multi == 0, (k.later, k.multi)
    err = row_nrel(x[pick].cpu().numpy(), np.fft.fft(src, axis=1))
    eout = (x.real ** 2 + x.imag ** 2).sum(dim=1)
    pars = float(((eout / n - ein).abs() / ein).max())
    print("seams: kind 6 n = %d: rows %.3g, Parseval %.3g" % (n, err, pars))
    assert err < EXACT and pars < EXACT, (err, pars)


# ---- C. host staging edges ------------------------------------------------------------
# No host loop is cut here, so gdsp_loop_stats must not move: what is checked
# is that the host entry gives the device entry's bits on each side of the edge.

def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("entry,size", [("FFTReal", 21845), ("FFTReal", 21846),
                                        ("FFTBatch", 16384), ("FFTBatch", 16385),
                                        ("FFT", 16384)])
def test_zero_copy_threshold(gdsp, D, entry, size):
    """kZeroCopyMax (gdsp_api.hip): in + out of 512 KiB. FFTReal moves 24 n
    bytes (21845: 524280, 21846: 524304), FFTBatch of n = 1 rows 32 a row
    (16384 rows: 524288, the last call below the staged path) and FFT of
    16384 points 524288."""
    F = gdsp.fft
    assert 24 * 21845 <= S.ZERO_COPY_MAX < 24 * 21846
    assert 32 * 16384 == S.ZERO_COPY_MAX < 32 * 16385
    with Counted(gdsp) as k:
        if entry == "FFTReal":
            x = S.noise(size, size)
            got = F.FFTReal(x)
            want = D.fft_real_batch(dev(x[None, :]))[0].cpu().numpy()
            ref = np.fft.fft(x)
        elif entry == "FFTBatch":
            x = S.noise(size, size, 1) + 1j * S.noise(size + 1, size, 1)
            got = F.FFTBatch(x)
            want = D.fft_batch(dev(x)).cpu().numpy()
            ref = x  # a transform of one point
            assert np.array_equal(got, x)
        else:
            x = S.noise(3, size) + 1j * S.noise(4, size)
            got = F.FFT(x)
            want = D.fft_batch(dev(x[None, :]))[0].cpu().numpy()
            ref = np.fft.fft(x)
    assert np.array_equal(_bits(got), _bits(want)), (entry, size)
    err = row_nrel(got.reshape(1, -1), ref.reshape(1, -1))
    print("seams: %s %d: %.3g" % (entry, size, err))
    assert err < EXACT
    assert (k.later, k.multi) == (0, 0), (k.later, k.multi)


def test_rows_longer_than_the_staging(gdsp, D):
    """stage_rows / unstage_rows (gdsp_api.hip) row by row, each row of 2.3 M
    doubles (18.4 MB) longer than both 8 MiB staging halves: gdsp_fir_batch
    from rows n + 3 apart into rows out_len + 5 apart, and gdsp_pwelch_batch
    from rows n + 3 apart, against the device entries on the same rows."""
    import torch
    L = gdsp._lib
    P = L._P
    channels, n, m = 2, 2_300_000, 31
    assert n * 8 > 2 * S.STAGING_HALF
    ldx = n + 3
    wide = np.full((channels, ldx), np.nan)
    wide[:, :n] = S.noise(23, channels, n)
    x = np.ascontiguousarray(wide[:, :n])
    h = np.random.default_rng(31).standard_normal(m)
    xd = dev(x)
    with Counted(gdsp) as k:
        for full in (0, 1):
            out_len = n + m - 1 if full else n
            ldo = out_len + 5
            out = np.full((channels, ldo), GUARD)
            L.check(L.lib().gdsp_fir_batch(wide.ctypes.data_as(P), ldx, h.ctypes.data_as(P), 1, m,
                                           channels, n, full, 0, out.ctypes.data_as(P), ldo),
                    "fir_batch")
            want = D.fir_batch(xd, dev(h), full=bool(full)).cpu().numpy()
            assert np.array_equal(_bits(out[:, :out_len]), _bits(want)), full
            assert (out[:, out_len:] == GUARD).all(), full
        nfft, nov = 256, 128
        win, wn = S.hamming(nfft), S.hamming(nfft)
        lp = nfft // 2 + 1
        pxx, freqs, lpo = np.empty((channels, lp)), np.empty(lp), L._I64(0)
        L.check(L.lib().gdsp_pwelch_batch(wide.ctypes.data_as(P), channels, n, ldx, 48000.0, nfft,
                                          nfft, nov, win.ctypes.data_as(P), wn.ctypes.data_as(P),
                                          0, pxx.ctypes.data_as(P), freqs.ctypes.data_as(P),
                                          ctypes.byref(lpo)), "pwelch_batch")
        assert lpo.value == lp
        nseg = gdsp.spectral.segment_count(n, nfft, nov)
        acc = zeros(channels, nfft)
        D.pwelch_batch_accumulate(xd, nfft, nfft, nov, 0, nseg, dev(win), acc)
        hacc = acc.cpu().numpy()
        for ch in range(channels):
            want = host_finalize(gdsp, hacc[ch], nseg, nfft, nfft, wn, 48000.0)
            assert np.array_equal(_bits(pxx[ch]), _bits(want)), ch
    torch.cuda.synchronize()
    assert k.later == 0, k.later
