"""Accuracy of every kernel family at roundoff, against the extended-precision
DFT of exact_dft.py.

The rest of the suite holds the engine to 1e-9 (1e-13 at selected lengths)
against float64 checkers. Here every family's result is compared elementwise
with an 80-bit reference, in units of u = 2**-53 (exact_dft.err_u), and bounded
by MARGIN = 16 times the error of the float64 reference of the same operation
on the same rows, measured in the same run (numpy.fft for transforms,
ifft(fft * fft) for Convolve, exact_dft.numpy_pwelch for Pwelch). A twiddle
taken through float, a constant typed to 12 digits or a recurrence restarted
too rarely costs 1e2 ... 1e5 u (test_accuracy_host.py's controls) and fails.

Why 16: the float64 reference measures 1-8 u on noise rows and 5-16 u on the
impulse row; the engine's documented accuracy (1e-15 = 9 u; 3.7e-15 = 33 u for
the chirp-z) is up to about 8 times that, and 16 leaves a factor of two.

Family margins above 16 (none may pass 64): see FAMILY_MARGIN below.

Every case prints family, n, variant, err_u and e_ref, and adds them to
exact_dft.RECORDS (scripts/measure_accuracy.py writes profiles/accuracy.json
from that; no test reads a bound from it).

Standard rows of a length n (exact_dft.standard_rows): complex noise, real
noise, an impulse 1-2j at an odd index, the tone of bin n // 3 plus 1e-3 of
the noise row, and the noise row again (batch 5: a ragged last workgroup).
Real-input entries get the real parts of rows 0-2.
"""
import contextlib
import importlib
from collections import namedtuple

import numpy as np
import pytest

import exact_dft as E

pytestmark = pytest.mark.gpu

# family -> (margin, measured worst ratio, cause); every other family: exact_dft.MARGIN.
# A family margin is the power of 2 at or above twice the measured ratio, 64 at most.
FAMILY_MARGIN = {
    # 96.0 u against 3.83 u on 3000 (5-10 on the other lengths, where numpy's own
    # chirp-z is the reference). The smooth-M chirp-z kernels (chirpz6k.hpp) multiply
    # by the twiddle powers w^3 .. w^(R-1), R up to 16, of c6_twiddle's three-term
    # recurrence (see pwelch-row below): 65-110 u, against 23 u for bluestein_kernel on
    # M = 8192, which keeps the recurrence to its radix-8 passes. Design: 1.5 % of
    # the chirp-z benchmark. A raced case (kinds 7 and 8) whose race keeps this
    # kernel is measured as this family: 481 and 518 are 16.4-18.1 on it.
    "chirpz6k": (64, 25.1, "three-term twiddle recurrence at radix 16 (c6_twiddle)"),
    # 42.8 u against 2.19 u. pwelch_row_kernel / pwelch_rowg_kernel (F = 4096) take the
    # twiddle powers w^3 .. w^15 of both twiddled radix-16 passes by the three-term
    # recurrence w^(r+2) = 2 cos(2 theta) w^r - w^(r-2) (pass_compute CHEB,
    # fft_device.hpp): for the small angles of a pass's first bases 2 cos(2 theta)
    # rounds away the angle, and the powers end up to 36 u (pass 1) and 78 u (pass 2)
    # off, against 9 and 12 u for the chain of complex products the other kernels use
    # (a numpy model of both chains). Every segment meets the same twiddles, so the
    # error does not average over the segments as the float64 reference's does, and
    # |Z|^2 doubles it. The recurrence is the kernel's design: two FMAs per power
    # instead of four instructions, 2-4 % of the flagship Pwelch; a stable form of it
    # costs what the complex product costs.
    "pwelch-row": (64, 19.5, "three-term twiddle recurrence at radix 16"),
    # 58.9 u against 3.18 u at F = 16384 (3.7 at 8192): pwelch_half_kernel<14> runs 32
    # points per thread, radix 32 32 16, and a radix-32 pass takes w^2 .. w^31 from one
    # table read by two chains of up to 15 complex products (18 u at the chain's end in
    # the same model), coherent over the segments and doubled by |Z|^2 as above.
    "pwelch-half": (64, 18.5, "radix-32 twiddle chains of 15 products from one table read"),
}

FS = 48000.0


def margin(family):
    return FAMILY_MARGIN.get(family, (E.MARGIN,))[0]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


@contextlib.contextmanager
def algorithm(gdsp, flags):
    """The engine under the named ALGO_* flags; restored on the way out."""
    F = gdsp.fft
    prev = F.Algorithm()
    bits = 0
    for name in flags:
        bits |= getattr(F, "ALGO_" + name)
    F.SetAlgorithm(bits)
    try:
        yield
    finally:
        F.SetAlgorithm(prev)


def _dev(fn, x, **kw):
    import torch
    out = fn(torch.from_numpy(np.ascontiguousarray(x)).cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


class Failures(list):
    """Runs every variant of a case before the first failure is raised, so a
    run's log carries all of its measurements."""

    def check(self, *a, **kw):
        try:
            E.check(*a, **kw)
        except AssertionError as e:
            self.append(str(e))

    def done(self):
        assert not self, "\n".join(self)


# ---- transforms ---------------------------------------------------------------------
# kind: the plan kind device.plan(n) must report under the case's flags (a
# tuple where a plan-time race decides). rows: the standard rows of the batch.
T = namedtuple("T", "family n flags chirpz kind rows parts",
               defaults=((), False, None, None, False))

R17 = (0, 2, 3)  # 2^17: the exact reference of three rows only
NR = ("NO_RACE",)

# kind 7: primes whose n - 1 has a radix list (17 -> 16, 257 -> 16 16, 3001 ->
# 25 15 8) and RADER_TOP, the largest below 8193 (8191 stays on chirp-z:
# test_primes_without_radix_list_stay_chirpz)
RADER_TOP = 8161
# kind 6 with neither factor a power of 2 (105 x 81), the smallest such plan found
MIXED4_RADIXCOL = 8505

TRANSFORMS = (
    # kind 1, LDS Stockham
    [T("lds", n, kind=1) for n in (2, 16, 256, 4096, 8192, 16384)]
    # kind 2, global power of 2; 2^17 on both sides of exec_fourstep's split by
    # batch (batch * 2^(17-13) <= 256: rows of 4096, above: of 8192)
    + [T("global", 1 << 15, kind=2), T("global", 1 << 16, kind=2),
       T("global", 1 << 17, kind=2, rows=(0,)),
       T("global", 1 << 17, kind=2, rows=(R17 * 2)[:5]),
       T("global", 1 << 17, kind=2, rows=(R17 * 6)[:17])]
    # kind 5, mixed radix: a pure power of each radix (every hand-typed
    # butterfly), 3000, 4095; the runtime-radix kernel; a compiled
    # specialisation above 4096 (re/im exchange); a hipRTC specialisation
    + [T("mixed", n, kind=5) for n in (2187, 3125, 2401, 1331, 2197, 3000, 4095, 5000, 5400)]
    + [T("mixed-generic", n, flags=("GENERIC_MIXED",), kind=5) for n in (3000, 2197)]
    # kind 6, mixed four-step: power-of-2 columns, 12000, single-radix
    # columns, chirp-z rows (2 x 10007)
    + [T("mixed4", n, kind=6) for n in (10000, 12000, MIXED4_RADIXCOL, 20014)]
    # kind 3, fused chirp-z: forced on 100 (bluestein_kernel, M = 256) and on 3000;
    # the smooth-M kernels (chirpz6k: 3000 and 3067 on M = 6144, 2062 on 4608, 1151 on
    # 2304, 5003 on 10240 = 16 R1 R2 16); the reference's M = 8192 (bluestein_kernel);
    # the two ends of the output-split range
    + [T("chirpz", 100, chirpz=True, kind=3), T("chirpz6k", 3000, chirpz=True, kind=3)]
    + [T("chirpz6k", n, kind=3) for n in (2062, 3067, 5003)]
    # (1151 is a prime with a Rader list, 1150 = 2 25 23, which the race may keep:
    # the chirp-z plan by name)
    + [T("chirpz6k", 1151, flags=("NO_RADER",), kind=3)]
    + [T("chirpz-pow2", 3000, flags=("CHIRPZ_POW2",), chirpz=True, kind=3)]
    + [T("chirpz-parts", n, kind=3, parts=True) for n in (8209, 14563)]
    # kind 4, composed chirp-z
    + [T("chirpz-composed", 16411, kind=4),
       T("chirpz-composed", 16411, flags=("CHIRPZ_UNFUSED",), kind=4),
       T("chirpz-composed", 8209, flags=("NO_CHIRPZ_PARTS",), kind=4)]
    # kind 7, Rader: the kernel itself (no race) and whatever the race keeps
    + [T("rader", n, flags=NR, kind=7) for n in (17, 257, 3001, RADER_TOP)]
    + [T("rader-raced", n, kind=(3, 7)) for n in (17, 257, 3001, RADER_TOP)]
    # kind 8, prime-factor Rader: 17 x 241, and beside P = 37 a native
    # in-register cofactor (2), an odd one (13) and a coprime split (14 = 2 x 7)
    + [T("rader-pfa", n, flags=NR, kind=8) for n in (4097, 74, 481, 518)]
    + [T("rader-pfa-raced", n, kind=(3, 8)) for n in (4097, 74, 481, 518)]
)


def _smooth_m(gdsp, p):
    """Whether a kind-3 plan runs the smooth-M kernels of chirpz6k.hpp: one part
    and M = gdsp::chirpz6k_m(n) (plan.hip)."""
    import ctypes
    m_of = gdsp._lib.lib()["_ZN4gdsp10chirpz6k_mEl"]
    m_of.restype, m_of.argtypes = ctypes.c_int, [ctypes.c_int64]
    return p.kind == 3 and p.parts == 1 and p.m == m_of(p.n)


def _tid(c):
    return "-".join([c.family, str(c.n)] + list(c.flags) + (["cz"] if c.chirpz else [])
                    + (["b%d" % len(c.rows)] if c.rows else []))


@pytest.mark.parametrize("case", TRANSFORMS, ids=_tid)
def test_transform(gdsp, D, case):
    """Forward and inverse through device.fft_batch, real input forward and
    inverse through device.fft_real_batch."""
    n, rows = case.n, case.rows
    rrows = None if rows is None else tuple(r for r in rows if r < 3)
    fam, fails = case.family, Failures()
    with algorithm(gdsp, case.flags):
        p = D.plan(n, case.chirpz)
        kinds = case.kind if isinstance(case.kind, tuple) else (case.kind,)
        assert p.kind in kinds, (n, p.kind, case.kind)
        if case.parts:
            assert p.parts > 1, (n, p.parts)
        if fam in ("chirpz", "chirpz6k", "chirpz-pow2"):
            assert _smooth_m(gdsp, p) == (fam == "chirpz6k"), (n, p.m)
        elif p.kind == 3 and _smooth_m(gdsp, p):
            fam = "chirpz6k"  # the race kept the chirp-z plan: that kernel's family
        if n == MIXED4_RADIXCOL:
            assert p.n1 & (p.n1 - 1) and p.n2 & (p.n2 - 1), (n, p.n1, p.n2)
        for inverse in (False, True):
            x = E.input_rows(n, rows=rows)
            ex = E.exact_standard(n, inverse, rows=rows)
            npf = np.fft.ifft if inverse else np.fft.fft
            tag = "b%d-" % len(x) + ("inverse" if inverse else "forward")
            got = _dev(D.fft_batch, x, inverse=inverse, chirpz=case.chirpz)
            fails.check(fam, n, tag, E.err_u(got, ex), E.err_u(npf(x, axis=1), ex), margin(fam))
            xr = E.input_rows(n, real=True, rows=rrows)
            ex = E.exact_standard(n, inverse, real=True, rows=rrows)
            got = _dev(D.fft_real_batch, xr, inverse=inverse, chirpz=case.chirpz)
            fails.check(fam, n, "real-" + tag, E.err_u(got, ex), E.err_u(npf(xr, axis=1), ex),
                        margin(fam))
    fails.done()


@pytest.mark.parametrize("n", [4096, 3000])
def test_host_entries(gdsp, n):
    """fft.FFT, IFFT, FFTReal, IFFTReal and FFTBatch: the kernels of
    test_transform behind the host staging."""
    F, fails = gdsp.fft, Failures()
    x, xr = E.input_rows(n), E.input_rows(n, real=True)
    for inverse, one, real_one in ((False, F.FFT, F.FFTReal), (True, F.IFFT, F.IFFTReal)):
        npf = np.fft.ifft if inverse else np.fft.fft
        ex, exr = E.exact_standard(n, inverse), E.exact_standard(n, inverse, real=True)
        d = "inverse" if inverse else "forward"
        fails.check("host", n, "batch-" + d, E.err_u(F.FFTBatch(x, inverse=inverse), ex),
                    E.err_u(npf(x, axis=1), ex))
        # the single-signal calls: the tone row, the real noise row
        fails.check("host", n, "one-" + d, E.err_u(one(x[3]), ex[3]), E.err_u(npf(x[3]), ex[3]))
        fails.check("host", n, "real-" + d, E.err_u(real_one(xr[1]), exr[1]),
                    E.err_u(npf(xr[1]), exr[1]))
    fails.done()


# ---- Convolve -----------------------------------------------------------------------
# fused kernel: 256 (16 rows per workgroup), 4096, 16384; the composed chain:
# 3000 (mixed radix), 257 (Rader or chirp-z); 4096 with the fused kernel off
CONVOLVE = [(256, (), True), (4096, (), True), (16384, (), True), (3000, (), False),
            (257, (), False), (4096, ("NO_FUSED_CONVOLVE",), False)]


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "perrow"])
@pytest.mark.parametrize("n,flags,fused", CONVOLVE,
                         ids=["-".join([str(c[0])] + list(c[1])) for c in CONVOLVE])
def test_convolve(gdsp, D, n, flags, fused, per_row):
    import torch
    x = E.input_rows(n)
    y = E.uniform_rows(n + 1, 5, n)
    y = y if per_row else y[0]
    ex = E.memo(("conv", n, per_row), lambda: E.exact_convolve(x, y))
    ref = np.fft.ifft(np.fft.fft(x, axis=1) * np.fft.fft(np.atleast_2d(y), axis=1), axis=1)
    with algorithm(gdsp, flags):
        assert D.convolve_fused(n) == fused
        got = D.convolve_batch(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        torch.cuda.synchronize()
    fam = "convolve-fused" if fused else "convolve-composed"
    E.check(fam, n, "-".join(["perrow" if per_row else "shared"] + list(flags)),
            E.err_u(got.cpu().numpy(), ex), E.err_u(ref, ex), margin(fam))


# ---- FFT2, FFTN, one axis ------------------------------------------------------------

def _nd_input(shape):
    """Uniform noise plus one impulse element."""
    rng = np.random.default_rng(int(np.prod(shape)) + len(shape))
    x = rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)
    x.ravel()[(3 * x.size // 7) | 1] += 8 * (1 - 2j)
    return x


# one-pass column kernel; two-pass column kernel; transposes with Rader and
# mixed rows; mixed rows both ways
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("shape", [(64, 48), (1024, 20), (37, 41), (100, 30)], ids=str)
def test_fft2(D, shape, inverse):
    x = _nd_input(shape)
    ex = E.memo(("fftn", shape, inverse), lambda: E.exact_fftn(x, None, inverse))
    ref = (np.fft.ifft2 if inverse else np.fft.fft2)(x)
    E.check("fft2", "x".join(map(str, shape)), "inverse" if inverse else "forward",
            E.err_u_all(_dev(D.fft2, x, inverse=inverse), ex), E.err_u_all(ref, ex),
            margin("fft2"))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("dims", [(8, 6, 5), (3, 1024, 7)], ids=str)
def test_fftn(D, dims, inverse):
    x = _nd_input(dims)
    ex = E.memo(("fftn", dims, inverse), lambda: E.exact_fftn(x, None, inverse))
    ref = (np.fft.ifftn if inverse else np.fft.fftn)(x)
    E.check("fftn", "x".join(map(str, dims)), "inverse" if inverse else "forward",
            E.err_u_all(_dev(D.fftn, x, inverse=inverse), ex), E.err_u_all(ref, ex),
            margin("fftn"))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_fft_axis(D, inverse):
    dims, axis = (3, 1024, 7), 1
    x = _nd_input(dims)
    ex = E.memo(("axis", dims, axis, inverse), lambda: E.exact_fft_axis(x, axis, inverse))
    ref = (np.fft.ifft if inverse else np.fft.fft)(x, axis=axis)
    import torch
    got = D.fft_axis(torch.from_numpy(x).cuda(), axis, inverse=inverse)
    torch.cuda.synchronize()
    E.check("fft-axis", "x".join(map(str, dims)), "axis1-" + ("inverse" if inverse else "forward"),
            E.err_u_all(got.cpu().numpy(), ex), E.err_u_all(ref, ex), margin("fft-axis"))


# ---- Pwelch -------------------------------------------------------------------------
# (family, NFFT, Noverlap, Pad, segments, window, flags, Scale_off). The input
# is uniform noise of (segments - 1) strides + NFFT + 3 samples; the odd
# segment count leaves a partnerless last segment in the packed pairs.
PW = namedtuple("PW", "family nfft nov pad segs win flags off", defaults=((), False))
PWELCH = [
    # wave kernels, half overlap; Pad > NFFT
    PW("pwelch-wave", 64, 32, 0, 9, "Hann"),
    PW("pwelch-wave", 256, 128, 0, 9, "Hamming"),
    PW("pwelch-wave", 1024, 512, 0, 9, "Blackman"),
    PW("pwelch-wave", 2048, 1024, 0, 9, "FlatTop"),
    PW("pwelch-wave", 1019, 300, 2048, 9, "Hann"),
    PW("pwelch-wave", 256, 128, 0, 9, "Hamming", (), True),  # Scale_off
    # the row kernel, half overlap; pwelch_rowg (any overlap); pwelch_half_kernel
    # at 8192 and 16384
    PW("pwelch-row", 4096, 2048, 0, 5, "Hamming"),
    PW("pwelch-row", 4096, 1024, 0, 5, "Blackman"),
    PW("pwelch-half", 8192, 4096, 0, 5, "FlatTop"),
    PW("pwelch-half", 16384, 8192, 0, 5, "Hann"),
    # mixed radix: compiled specialisations, a hipRTC one, the runtime-radix kernel
    PW("pwelch-mixed", 3000, 1000, 0, 5, "Hamming"),
    PW("pwelch-mixed", 2205, 1102, 0, 9, "Blackman"),
    PW("pwelch-mixed", 5400, 2700, 0, 5, "FlatTop"),
    PW("pwelch-mixed-generic", 3000, 1000, 0, 5, "Hann", ("GENERIC_MIXED",)),
    # a prime: segments materialised, transformed by the plan
    PW("pwelch-prime", 1031, 515, 0, 9, "Hamming"),
]


def _pw_id(c):
    return "-".join([c.family, str(c.nfft), str(c.nov), str(c.pad), c.win] + list(c.flags)
                    + (["scale_off"] if c.off else []))


def _pw_variant(c):
    return "-".join(["nov%d" % c.nov, "pad%d" % (c.pad or c.nfft), c.win] + list(c.flags)
                    + (["scale_off"] if c.off else []))


def _pw_setup(gdsp, c, channels=1):
    pad = c.pad or c.nfft
    n = (c.segs - 1) * (c.nfft - c.nov) + c.nfft + 3
    assert E.segment_count(n, c.nfft, c.nov) == c.segs
    wf = getattr(gdsp.window, c.win)
    x = np.random.default_rng(c.nfft + pad + channels).uniform(-1, 1, (channels, n))
    o = gdsp.spectral.PwelchOptions(NFFT=c.nfft, Window=wf, Pad=c.pad, Noverlap=c.nov,
                                    Scale_off=c.off)
    args = (FS, c.nfft, pad, c.nov, wf(max(pad, c.nfft)), wf(c.nfft), c.off)
    key = ("pwelch", c.nfft, pad, c.nov, c.win, c.off, channels)
    ex = E.memo(key, lambda: np.stack([E.exact_pwelch(r, *args) for r in x]))
    ref = np.stack([E.numpy_pwelch(r, *args) for r in x])
    return x, o, ex, ref


def _pw_check(fails, family, c, variant, got, ex, ref):
    assert got.shape == ex.shape
    m = margin(family)
    fails.check(family, c.nfft, variant + "-max", E.err_u(got, ex), E.err_u(ref, ex), m)
    fails.check(family, c.nfft, variant + "-perbin", E.err_u_per_bin(got, ex),
                E.err_u_per_bin(ref, ex), m)


@pytest.mark.parametrize("case", PWELCH, ids=_pw_id)
def test_pwelch(gdsp, case):
    x, o, ex, ref = _pw_setup(gdsp, case)
    with algorithm(gdsp, case.flags):
        got, _ = gdsp.spectral.Pwelch(x[0], FS, o)
    fails = Failures()
    _pw_check(fails, case.family, case, _pw_variant(case), got[None, :], ex, ref)
    fails.done()


# the kernel over the channels: S = 16, 2 and the two-wave workgroup; 4096: the
# loop over the channels
PWELCH_BATCH = [PW("pwelch-batch", 64, 32, 0, 9, "Hann"),
                PW("pwelch-batch", 512, 256, 0, 9, "Hamming"),
                PW("pwelch-batch", 2048, 1024, 0, 9, "Blackman"),
                PW("pwelch-batch-loop", 4096, 2048, 0, 5, "FlatTop")]


@pytest.mark.parametrize("case", PWELCH_BATCH, ids=_pw_id)
def test_pwelch_batch(gdsp, D, case):
    """3 channels in a buffer of odd row stride through device.pwelch_batch."""
    import torch
    channels = 3
    x, o, ex, ref = _pw_setup(gdsp, case, channels)
    n = x.shape[1]
    ldx = n + 3 if (n + 3) % 2 else n + 4
    buf = torch.full((channels, ldx), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(x).cuda()
    assert gdsp.spectral.pwelch_batch_fused(channels, n, case.nfft, case.pad, case.nov) \
        == (case.family == "pwelch-batch")
    got, _ = D.pwelch_batch(buf[:, :n], FS, o)
    torch.cuda.synchronize()
    fails = Failures()
    _pw_check(fails, case.family, case, _pw_variant(case), got.cpu().numpy(), ex, ref)
    fails.done()


def all_lengths():
    """Every transform length the cases above put through exact_fft (the
    reference's self-check runs at each, test_accuracy_host.py)."""
    ns = {c.n for c in TRANSFORMS} | {4096, 3000} | {c[0] for c in CONVOLVE}
    ns |= {64, 48, 1024, 20, 37, 41, 100, 30, 8, 6, 5, 3, 7}
    ns |= {max(c.pad, c.nfft) for c in PWELCH + PWELCH_BATCH}
    return sorted(ns)
