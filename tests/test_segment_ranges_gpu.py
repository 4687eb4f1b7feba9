"""Segment ranges [seg_begin, seg_end) of gdsp_pwelch_accumulate_device on every
kernel behind it, and the refusal of segments that exceed the signal.

Every caller in the library passes seg_begin = 0, and every kernel computes its
own seg_begin + 2 p, has1, npairs, inactive-worker fallback and touch-ahead or
half-overlap carry. Here each kernel runs nonzero, odd, interior and empty
ranges and split accumulations.

Reference: for real x, window w and F = max(Pad, NFFT)

    0.5 (acc[j] + acc[(F - j) mod F]) = sum_{s in [a, b)} |FFT_F(w x_s, zero-padded)[j]|^2

which is what gdsp_pwelch_finalize reads. Only the folded sum is compared:
which segments get packed into a pair moves power between acc[j] and
acc[F - j] (test_pwelch_batch_gpu.test_accumulation_adds), so an odd a
legitimately changes the unfolded accumulators. The right-hand side is
exact_dft.exact_fft (80-bit) of the windowed segments, rounded to float64, and
the bound is conftest.row_nrel < 1e-13 (the suite's engine-level bound; the
README states Pwelch at up to 7e-15 of the largest bin).

The signal is uniform noise of (N - 1) stride + NFFT + min(3, stride - 1)
samples inside NaN guard bands, and for a range [a, b) every sample outside
[a stride, (b - 1) stride + NFFT) is NaN as well: a kernel that loads segment b
and multiplies it by zero gives a non-finite sum and fails, as it should (at
the true end of a signal that load is out of bounds). acc is exactly F doubles
inside sentinel guard bands.

G is the number of segments a worker takes at once (2 max(1, 1024 / F) for the
wave kernels, 2 elsewhere) and N = 2 G + 3 segments (32768: 5).

test_accuracy_host.py's neighbour test_segment_ranges_host.py checks this
reference on the CPU (against exact_dft.exact_pwelch, and that an off-by-one
range cannot pass the bound).
"""
import importlib
from collections import namedtuple

import numpy as np
import pytest

import exact_dft as E
from conftest import row_nrel
from guarded import GUARD, NAN, guarded, pad_for
from test_accuracy_gpu import algorithm

EXACT = 1e-13

# path: the branch of gdsp_pwelch_accumulate_device (welch.hip) the case must
# reach; _assert_path checks it from the plan and the library's queries.
Case = namedtuple("Case", "path nfft nov pad flags nseg", defaults=((), None))

# Lengths of the fused Pwelch's own radix lists (GDSP_SPEC_GROUP(specspw),
# fft_specs0.hip). The plan has no query for md_pw; a kind-5, compiled plan of
# one of these lengths runs it (welch.hip: own = md_pw.n > 0 && !jit).
SPECSPW = (3000, 4000, 6000, 768, 1875, 2250, 2500, 3125, 6400, 5880, 625, 375, 200, 320, 1152,
           735)

CASES = [
    # pwelch_wave_kernel: HALF at S = 16; plain with an odd overlap; the PAD
    # variant; S = 1; the two-wave workgroup, half and plain
    Case("wave", 64, 32, 0), Case("wave", 256, 65, 0), Case("wave", 128, 16, 256),
    Case("wave", 1024, 512, 0), Case("wave", 2048, 1024, 0), Case("wave", 2048, 513, 0),
    # pwelch_half_kernel; pwelch_row_kernel (4096: the carry of the half
    # overlap must start at sample a * 2048)
    Case("half", 32, 16, 0), Case("half", 8192, 4096, 0), Case("half", 16384, 8192, 0),
    Case("row", 4096, 2048, 0),
    Case("rowg", 4096, 1024, 0),
    # the generic pwelch_kernel: log2 F = 4 (below the half kernel's range),
    # Pad > NFFT at 4096, an overlap other than half above 4096
    Case("generic", 16, 8, 0), Case("generic", 2048, 512, 4096), Case("generic", 8192, 2048, 0),
    # compiled specialisations: Pwelch's own list; the FFT's list (1000 = 10 10 10)
    Case("pw-list", 375, 187, 0), Case("pw-list", 3000, 1000, 0),
    Case("fft-list", 1000, 500, 0),
    Case("hiprtc", 810, 405, 0),
    Case("runtime-radix", 3000, 1000, 0, ("GENERIC_MIXED",)),
    # materialised: log2 F < 4; a chirp-z prime; Rader or what the race keeps; kind 2
    Case("materialised", 8, 4, 0), Case("materialised", 1031, 515, 0),
    Case("materialised", 257, 128, 0), Case("materialised", 32768, 16384, 0, (), 5),
]
PATHS = ("wave", "half", "row", "rowg", "generic", "pw-list", "fft-list", "hiprtc",
         "runtime-radix", "materialised")


def case_id(c):
    return "-".join([c.path, str(c.nfft), str(c.nov), str(c.pad)] + list(c.flags))


def flen(c):
    return max(c.pad or c.nfft, c.nfft)


def group(c):
    return 2 * max(1, 1024 // flen(c)) if c.path == "wave" else 2


def nsegs(c):
    return c.nseg or 2 * group(c) + 3


def ranges(c):
    g, n = group(c), nsegs(c)
    return [(0, n), (1, n), (g + 1, n), (2, 2 + g + 1), (n - 1, n)]


def splits(c):
    """An odd and an even split point of [0, N)."""
    g = group(c)
    return [g + 1, g] if nsegs(c) > g + 1 else [1, 2]


def window(c):
    """The segment window, max(Pad, NFFT) entries: Hamming (no zero at the
    ends, so a segment's first and last sample count)."""
    f = flen(c)
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(f) / (f - 1))


def signal(c):
    stride = c.nfft - c.nov
    n = (nsegs(c) - 1) * stride + c.nfft + min(3, stride - 1)
    assert E.segment_count(n, c.nfft, c.nov) == nsegs(c)
    x = np.random.default_rng([c.nfft, c.nov, flen(c)]).uniform(-1, 1, n)
    x.setflags(write=False)
    return x


def poisoned(c, x, a, b):
    """x with NaN in every sample that segments [a, b) do not read."""
    stride = c.nfft - c.nov
    y = np.full_like(x, NAN)
    if b > a:
        lo, hi = a * stride, (b - 1) * stride + c.nfft
        y[lo:hi] = x[lo:hi]
    return y


def segment_powers(c, x, a, b):
    """|FFT_F(w x_s, zero-padded)|^2 of segments s in [a, b) of x, a row each,
    in extended precision."""
    f, stride = flen(c), c.nfft - c.nov
    segs = np.zeros((b - a, f), E.LD)
    for s in range(a, b):
        segs[s - a, :c.nfft] = x[s * stride:s * stride + c.nfft]
    spec = E.exact_fft(segs * window(c).astype(E.LD)[None, :])
    return spec.real * spec.real + spec.imag * spec.imag


def powers(c):
    """segment_powers of the whole clean signal, computed once."""
    return E.memo(("segpow", c.nfft, c.nov, flen(c), nsegs(c)),
                  lambda: segment_powers(c, signal(c), 0, nsegs(c)))


def reference(c, a, b):
    """The folded sum of range [a, b), rounded to float64."""
    return powers(c)[a:b].sum(axis=0).astype(np.float64)


def fold(acc):
    acc = np.asarray(acc)
    f = acc.shape[-1]
    return 0.5 * (acc + acc[..., (f - np.arange(f)) % f])


# ---- the GPU tests ------------------------------------------------------------------

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def D(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")
    return importlib.import_module("go-dsp_amd.device")


def _log2(f):
    return f.bit_length() - 1 if f & (f - 1) == 0 else None


def _assert_path(gdsp, D, c, n):
    """The branch of gdsp_pwelch_accumulate_device that (nfft, nov, pad) takes
    under the current flags, from the plan of F and the library's queries,
    must be c.path. (Strides here are far below the 2^22 that ends fusing.)"""
    f = flen(c)
    p = D.plan(f)
    lg = _log2(f)
    half = 2 * c.nov == c.nfft and f == c.nfft
    # pwelch_wave_applies and pwelch_batch_applies are the same range of
    # log2 F (6 .. 11), and the latter is what the library lets a caller ask
    wave = p.kind == 1 and gdsp.spectral.pwelch_batch_fused(1, n, c.nfft, c.pad, c.nov)
    generic_mixed = bool(gdsp.fft.Algorithm() & gdsp.fft.ALGO_GENERIC_MIXED)
    if wave:
        got = "wave"
    elif p.kind == 1 and lg >= 4:
        if half and lg >= 5:
            got = "row" if lg == 12 else "half"  # launch_pwelch_half: 4096 is pwelch_row_kernel
        elif lg == 12 and f == c.nfft:
            got = "rowg"
        else:
            got = "generic"
    elif p.kind == 5 and generic_mixed:
        assert len(p.radices) >= 2  # md_gen.npass >= 2
        got = "runtime-radix"
    elif p.kind == 5 and p.runtime_compiled:
        got = "hiprtc"
    elif p.kind == 5:
        got = "pw-list" if f in SPECSPW else "fft-list"
        if f == 1000:
            assert p.radices == (10, 10, 10), p.radices  # the compiled list, not the generic one
    else:
        got = "materialised"
    assert got == c.path, (case_id(c), got, p.kind, p.runtime_compiled, p.radices)
    if c.path == "materialised":
        want = {8: (1,), 1031: (3,), 257: (3, 7), 32768: (2,)}[f]
        assert p.kind in want, (f, p.kind)


class _Setup:
    """The device side of a case: the window, and accumulate(x, a, b) into a
    fresh zeroed accumulator of exactly F doubles between sentinel bands, from
    a signal between NaN bands; returns the accumulator as numpy."""

    def __init__(self, D, c):
        import torch
        self.torch, self.D, self.c = torch, D, c
        self.win = torch.from_numpy(window(c)).cuda()
        self.checks = []

    def x(self, x):
        xd, chk = guarded(self.torch.from_numpy(np.array(x)).cuda(), NAN,
                          pad_for(len(x), 1))
        self.checks.append(chk)
        return xd

    def acc(self):
        a, chk = guarded(self.torch.zeros(flen(self.c), dtype=self.torch.float64, device="cuda"),
                         GUARD, pad_for(flen(self.c)))
        self.checks.append(chk)
        return a

    def add(self, xd, a, b, acc):
        c = self.c
        self.D.pwelch_accumulate(xd, c.nfft, c.pad or c.nfft, c.nov, a, b, self.win, acc)

    def done(self):
        self.torch.cuda.synchronize()
        for chk in self.checks:
            chk(case_id(self.c))
        self.checks = []


def test_every_path_has_a_case():
    """Each branch of the dispatch has a case, and test_ranges asserts the
    branch of every case before it runs it (_assert_path)."""
    assert {c.path for c in CASES} == set(PATHS)
    assert len({case_id(c) for c in CASES}) == len(CASES)


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_ranges(gdsp, D, c):
    x, n_seg = signal(c), nsegs(c)
    fails = []
    with algorithm(gdsp, c.flags):
        _assert_path(gdsp, D, c, len(x))
        s = _Setup(D, c)
        for a, b in ranges(c):
            acc = s.acc()
            s.add(s.x(poisoned(c, x, a, b)), a, b, acc)
            s.done()
            got = fold(acc.cpu().numpy())
            finite = bool(np.isfinite(got).all())
            err = row_nrel(got, reference(c, a, b)) if finite else float("inf")
            print("ranges: %s [%d, %d) of %d: %.3g" % (case_id(c), a, b, n_seg, err))
            if not err < EXACT:
                fails.append("[%d, %d): %s" % (a, b, err if finite else "non-finite sums"))
        # an empty range at a > 0 leaves acc as it is: no sample is read (all NaN)
        acc = s.acc()
        before = np.random.default_rng(1).uniform(1, 2, flen(c))
        acc.copy_(s.torch.from_numpy(before).cuda())
        s.add(s.x(poisoned(c, x, 2, 2)), 2, 2, acc)
        s.done()
        assert np.array_equal(acc.cpu().numpy(), before), "an empty range changed acc"
        # [0, k) then [k, N) into one acc, an odd and an even k
        xd = s.x(x)
        for k in splits(c):
            acc = s.acc()
            s.add(xd, 0, k, acc)
            s.add(xd, k, n_seg, acc)
            s.done()
            err = row_nrel(fold(acc.cpu().numpy()), reference(c, 0, n_seg))
            print("ranges: %s [0, %d) + [%d, %d): %.3g" % (case_id(c), k, k, n_seg, err))
            if not err < EXACT:
                fails.append("split at %d: %s" % (k, err))
    assert not fails, case_id(c) + ": " + "; ".join(fails)


@gpu
def test_loop_over_channels(gdsp, D):
    """pwelch_batch_accumulate with a range, at a length it loops over the
    channels for (4096, half overlap: pwelch_row_kernel): 3 channels scaled by
    10^(c mod 4), row stride n + 3 with NaN gaps, range [1, 6)."""
    import torch
    c = Case("row", 4096, 2048, 0)
    channels, a, b = 3, 1, 6
    x = signal(c)
    n = len(x)
    assert not gdsp.spectral.pwelch_batch_fused(channels, n, c.nfft, 0, c.nov)
    scale = 10.0 ** (np.arange(channels) % 4)
    rows = np.full((channels, n + 3), NAN)
    # every channel its own stretch of noise: channel c is x rotated by c * 37
    clean = np.stack([np.roll(x, 37 * ch) * scale[ch] for ch in range(channels)])
    for ch in range(channels):
        rows[ch, :n] = poisoned(c, clean[ch], a, b)
    buf, chk_x = guarded(torch.from_numpy(rows).cuda(), NAN, pad_for(n + 3, 1))
    acc, chk_acc = guarded(torch.zeros((channels, 4096), dtype=torch.float64, device="cuda"),
                           GUARD, pad_for(4096))
    win = torch.from_numpy(window(c)).cuda()
    D.pwelch_batch_accumulate(buf[:, :n], c.nfft, c.nfft, c.nov, a, b, win, acc)
    torch.cuda.synchronize()
    chk_x("loop x")
    chk_acc("loop acc")
    got = fold(acc.cpu().numpy())
    assert np.isfinite(got).all()
    ref = np.stack([segment_powers(c, r, a, b).sum(axis=0).astype(np.float64) for r in clean])
    for ch in range(channels):
        err = row_nrel(got[ch], ref[ch])
        print("ranges: loop channel %d [%d, %d): %.3g" % (ch, a, b, err))
        assert err < EXACT, ch


# ---- segments that exceed the signal --------------------------------------------------

def _refused(gdsp, call):
    with pytest.raises(gdsp._lib.GDSPError) as e:
        call()
    assert e.value.status == gdsp._lib.GDSP_ERR_INVALID, e.value.status


@gpu
@pytest.mark.parametrize("f", [256, 3000])
def test_short_signal_is_refused(gdsp, D, f):
    """A signal of NFFT - 1 samples has no segment: the range [0, 1) is
    GDSP_ERR_INVALID in every accumulate entry (the callers pad to NFFT
    first), and acc keeps its bits. Nothing runs on the short buffer."""
    import torch
    rng = np.random.default_rng(f)
    win = torch.from_numpy(0.5 + 0.5 * rng.uniform(size=f)).cuda()
    x, chk_x = guarded(torch.from_numpy(rng.uniform(-1, 1, (2, f - 1))).cuda(), NAN, pad_for(f))
    y, chk_y = guarded(torch.from_numpy(rng.uniform(-1, 1, (2, f - 1))).cuda(), NAN, pad_for(f))
    hb = f // 2 + 1
    start = rng.uniform(1, 2, 2 * 4 * hb)

    def fresh(count):
        a, chk = guarded(torch.from_numpy(start[:count].copy()).cuda(), GUARD, pad_for(f))
        return a, chk

    calls = [
        ("single", f, lambda a: D.pwelch_accumulate(x[0], f, f, f // 2, 0, 1, win, a)),
        ("batch", 2 * f, lambda a: D.pwelch_batch_accumulate(x, f, f, f // 2, 0, 1, win, a)),
        ("batch-1", f, lambda a: D.pwelch_batch_accumulate(x[:1], f, f, f // 2, 0, 1, win, a)),
        ("cpsd", 2 * 4 * hb, lambda a: D.cpsd_batch_accumulate(x, y, f, f, f // 2, 0, 1, win, a)),
    ]
    for name, count, call in calls:
        acc, chk = fresh(count)
        _refused(gdsp, lambda: call(acc))
        torch.cuda.synchronize()
        chk(name)
        assert np.array_equal(acc.cpu().numpy().view(np.int64), start[:count].view(np.int64)), name
    chk_x("x")
    chk_y("y")
