"""GPU parity of the cross spectra (gdsp_cpsd_batch,
gdsp_cpsd_batch_accumulate_device, gdsp_cpsd_batch_finalize_device, Cpsd,
Coherence, CoherenceChannels).

The reference is built here, per row, from the oracle's pieces: its Segment, its
window, zero-padding, its FFTReal, then the sums and the scaling of
include/gdsp_fft.h in numpy. Every result is held to the suite's 1e-9 against
it (and the Pxx / Pyy planes against the oracle's Pwelch too), and to 1e-13
engine against engine: the fused kernel against the materialised form under
ALGO_NO_FUSED_CPSD, Pxx against spectral.Pwelch, a split accumulation against
the whole.

Shapes: the smallest that reach each way the kernel can go wrong. F = 64, 256,
1024 run S = 16, 4, 1 transforms per wave and F = 2048 the two-wave workgroup
with the mirror across its waves; segments per channel 1, S (one exact group),
S + 1 and 2 S + 2 (full groups and a masked one) with a tail shorter than a
stride; 1, 2 and 5 channels; y as one row for all and row by row. Rows are
scaled by 10^(c mod 4) so a leak between channels shows in the per-row error,
live in buffers of row stride n + 3 (x) and n + 5 (y) with NaN in the gaps, and
the accumulators and every result carry a guard row that must come back
untouched. With one y for all rows the scaled x rows stand up to 1000 times
above it: Pyy is held to spectral.Pwelch(y) at 1e-13 there too, which the packed
transform meets only because the kernels balance every segment's pair by a
power of 2 (cpsd_batch.hip; 1.1e-12 without it); a level that changes by 1e12
after the first segment is held to the same bounds. y is x delayed by 3 samples
plus noise, so the cross spectrum has a definite phase and the coherence lies
strictly between 0 and 1 wherever there is more than one segment."""
import importlib
import io
import struct

import numpy as np
import pytest

from conftest import row_nrel

pytestmark = pytest.mark.gpu

TOL = 1e-9     # north star: within 1e-9 relative
EXACT = 1e-13  # engine against engine (test_parity_gpu.py)
GUARD = -12345.0
FS = 48000.0

# option kinds: (NFFT, Noverlap, Pad) from F = max(Pad, NFFT)
OPTS = {
    "nov0": lambda f: (f, 0, 0),                 # plain
    "half": lambda f: (f, f // 2, 0),            # half overlap
    "odd": lambda f: (f, f // 4 + 1, 0),         # odd overlap
    "pad2": lambda f: (f // 2, f // 8, f),       # Pad = 2 NFFT: the PAD variant
    "padh": lambda f: (f, f // 2 - 3, f // 2),   # Pad = NFFT / 2 (pwelch.go:108 quirk)
}
SEGS = {"one": lambda s: 1, "s": lambda s: s, "s1": lambda s: s + 1, "g2": lambda s: 2 * s + 2}

# (F, options, segments, channels, y as one row?): every F with every option
# kind and every segment count, every channel count and both y forms with every F
TABLE = [
    (64, "nov0", "one", 1, False), (64, "half", "s", 2, True), (64, "odd", "s1", 5, False),
    (64, "pad2", "g2", 5, True), (64, "padh", "g2", 2, False),
    (256, "nov0", "g2", 5, True), (256, "half", "one", 2, False), (256, "odd", "s", 1, True),
    (256, "pad2", "s1", 2, False), (256, "padh", "s1", 5, True),
    (1024, "nov0", "s1", 2, True), (1024, "half", "g2", 5, False), (1024, "odd", "one", 5, True),
    (1024, "pad2", "s", 1, False), (1024, "padh", "g2", 2, True),
    (2048, "nov0", "s", 5, False), (2048, "half", "s1", 1, True), (2048, "odd", "g2", 2, False),
    (2048, "pad2", "one", 2, True), (2048, "padh", "g2", 5, False),
]
IDS = ["-".join(str(v) for v in row[:4]) + ("-y1" if row[4] else "-yc") for row in TABLE]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gdsp):
    if gdsp.device_count() < 1:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("go-dsp_amd.device")


def _shape(row):
    f, opt, seg, channels, one = row
    nfft, nov, pad = OPTS[opt](f)
    pad = pad or nfft  # the default, spelled out
    s = max(1, 1024 // f)  # transforms side by side in a worker
    nsegs = SEGS[seg](s)
    stride = nfft - nov
    n = (nsegs - 1) * stride + nfft + min(3, stride - 1)  # a tail shorter than a stride
    return nfft, nov, pad, nsegs, n, channels, one


def _options(gdsp, nfft, nov, pad, win="Hann"):
    return gdsp.spectral.PwelchOptions(NFFT=nfft, Noverlap=nov, Pad=pad,
                                       Window=getattr(gdsp.window, win))


def _signals(seed, channels, n, one):
    """x rows scaled by 10^(c mod 4); y = x delayed by 3 samples + half-size
    noise: per row, or (one) a single y that every x row leads by 3."""
    rng = np.random.default_rng(seed)
    scale = (10.0 ** (np.arange(channels) % 4))[:, None]
    if one:
        y = rng.standard_normal(n)
        x = scale * (np.roll(y, -3)[None, :] + 0.5 * rng.standard_normal((channels, n)))
        return x, y
    x = scale * rng.standard_normal((channels, n))
    y = np.roll(x, 3, axis=1) + 0.5 * scale * rng.standard_normal((channels, n))
    return x, y


def _strided(a, gap):
    """The rows of a on the device in a buffer of row stride n + gap, NaN between."""
    import torch
    if a.ndim == 1:
        return torch.from_numpy(a).cuda()
    rows, n = a.shape
    buf = torch.full((rows, n + gap), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(a).cuda()
    return buf[:, :n]


def _reference(oracle, x, y, nfft, nov, pad, win="hann", fs=FS):
    """(Pxy, Pxx, Pyy, Cxy) rows by the definition, from the oracle's pieces."""
    flen, lp = max(pad, nfft), pad // 2 + 1
    w = oracle.window(win, flen)
    norm = float(np.sum(oracle.window(win, nfft) ** 2)) * fs
    cj = np.ones(lp)
    cj[1:lp - 1] = 2.0

    def spectra(r):
        r = np.asarray(r, dtype=np.float64)
        if r.size < nfft:
            r = np.concatenate([r, np.zeros(nfft - r.size)])
        out = []
        for seg in oracle.segment(r, nfft, nov):
            z = np.zeros(flen)
            z[:nfft] = seg
            out.append(oracle.fft_real(z * w)[:lp])
        return np.array(out).reshape(len(out), lp)

    ys = [spectra(y)] * len(x) if np.ndim(y) == 1 else [spectra(r) for r in y]
    res = []
    for r, Y in zip(x, ys):
        X = spectra(r)
        nsegs = len(X)
        sxx, syy = np.sum(np.abs(X) ** 2, axis=0), np.sum(np.abs(Y) ** 2, axis=0)
        sxy = np.sum(np.conj(X) * Y, axis=0)
        sc = cj / max(nsegs, 1) / norm
        res.append((sc * sxy, sc * sxx, sc * syy, np.abs(sxy) ** 2 / (sxx * syy)))
    return tuple(np.stack([r[i] for r in res]) for i in range(4))


def _run_guarded(D, xd, yd, o, flen, lp, **kw):
    """device.cpsd_batch into caller tensors with a guard row each; the four
    results as numpy, freqs, and the accumulators."""
    import torch
    channels = xd.shape[0]
    hb = flen // 2 + 1
    acc = torch.full((channels + 1, 4, hb), GUARD, dtype=torch.float64, device="cuda")
    outs = [torch.full((channels + 1, lp), GUARD, dtype=dt, device="cuda")
            for dt in (torch.complex128, torch.float64, torch.float64, torch.float64)]
    r = D.cpsd_batch(xd, yd, FS, o, acc=acc[:channels], out=[t[:channels] for t in outs], **kw)
    torch.cuda.synchronize()
    assert r.Pxy.data_ptr() == outs[0].data_ptr() and r.Cxy.data_ptr() == outs[3].data_ptr()
    assert bool((acc[channels] == GUARD).all())
    for t in outs:
        assert bool((t[channels] == GUARD).all())
    return [t[:channels].cpu().numpy() for t in outs], r.freqs, acc[:channels].cpu().numpy()


_cache: dict = {}


def _case(gdsp, oracle, D, i):
    """Inputs, the reference rows and the fused kernel's result of TABLE[i], once."""
    if i not in _cache:
        nfft, nov, pad, nsegs, n, channels, one = _shape(TABLE[i])
        x, y = _signals(2000 + i, channels, n, one)
        o = _options(gdsp, nfft, nov, pad)
        assert gdsp.spectral.segment_count(n, nfft, nov) == nsegs
        assert gdsp.spectral.cpsd_batch_fused(channels, n, nfft, pad, nov)
        got, freqs, acc = _run_guarded(D, _strided(x, 3), _strided(y, 5), o, max(pad, nfft),
                                       pad // 2 + 1)
        _cache[i] = dict(x=x, y=y, o=o, ref=_reference(oracle, x, y, nfft, nov, pad), got=got,
                         freqs=freqs, acc=acc, nsegs=nsegs)
    return _cache[i]


NAMES = ("Pxy", "Pxx", "Pyy", "Cxy")


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_fused_kernel_vs_reference_and_pwelch(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    nfft, nov, pad, nsegs, n, channels, one = _shape(TABLE[i])
    for name, got, ref in zip(NAMES, c["got"], c["ref"]):
        err = row_nrel(got, ref)
        print("reference", IDS[i], name, err)
        assert err < TOL, name
    pxy, pxx, pyy, cxy = c["got"]
    yrows = [c["y"]] * channels if one else list(c["y"])
    for name, got, rows in (("Pxx", pxx, c["x"]), ("Pyy", pyy, yrows)):
        ref = [oracle.pwelch(r, FS, nfft=nfft, pad=pad, noverlap=nov) for r in rows]
        err = row_nrel(got, np.stack([p for p, _ in ref]))
        print("oracle.pwelch", IDS[i], name, err)
        assert err < TOL, name
        assert np.array_equal(c["freqs"], ref[0][1])
        single = np.stack([gdsp.spectral.Pwelch(r, FS, c["o"])[0] for r in rows])
        err = row_nrel(got, single)
        print("spectral.Pwelch", IDS[i], name, err)
        assert err < EXACT, name
    # bins 0 and F / 2 are their own mirrors: real, exactly
    assert np.all(pxy[:, 0].imag == 0)
    if pad // 2 == max(pad, nfft) // 2:
        assert np.all(pxy[:, -1].imag == 0)
    assert np.all(cxy <= 1 + 1e-12) and np.all(cxy > 0)
    if nsegs > 1:
        assert np.all(cxy[:, 1:-1] < 1)


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_materialised_form_agrees_with_fused_kernel(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    F = gdsp.fft
    nfft, nov, pad, nsegs, n, channels, _ = _shape(TABLE[i])
    prev = F.Algorithm()
    try:
        F.SetAlgorithm(prev | F.ALGO_NO_FUSED_CPSD)
        assert not gdsp.spectral.cpsd_batch_fused(channels, n, nfft, pad, nov)
        got, freqs, _ = _run_guarded(D, _strided(c["x"], 3), _strided(c["y"], 5), c["o"],
                                     max(pad, nfft), pad // 2 + 1)
    finally:
        F.SetAlgorithm(prev)
    for name, a, b in zip(NAMES, got, c["got"]):
        err = row_nrel(a, b)
        print("materialised", IDS[i], name, err)
        assert err < EXACT, name
    assert np.array_equal(freqs, c["freqs"])
    assert np.all(got[0][:, 0].imag == 0)


@pytest.mark.parametrize("i", [2, 8, 11, 17], ids=[IDS[i] for i in (2, 8, 11, 17)])
def test_swapped_arguments_conjugate(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)  # y row by row
    nfft, nov, pad, _, _, _, one = _shape(TABLE[i])
    assert not one
    got, _, _ = _run_guarded(D, _strided(c["y"], 5), _strided(c["x"], 3), c["o"], max(pad, nfft),
                             pad // 2 + 1)
    for name, a, b in (("Pxy", got[0], np.conj(c["got"][0])), ("Pxx", got[1], c["got"][2]),
                       ("Pyy", got[2], c["got"][1]), ("Cxy", got[3], c["got"][3])):
        err = row_nrel(a, b)
        print("swapped", IDS[i], name, err)
        assert err < EXACT, name


@pytest.mark.parametrize("i", [4, 5, 14, 15], ids=[IDS[i] for i in (4, 5, 14, 15)])
def test_cpsd_of_a_signal_with_itself_is_pwelch(gdsp, oracle, D, i):
    c = _case(gdsp, oracle, D, i)
    nfft, nov, pad, _, _, _, _ = _shape(TABLE[i])
    xd = _strided(c["x"], 3)
    (pxy, pxx, pyy, cxy), _, _ = _run_guarded(D, xd, xd, c["o"], max(pad, nfft), pad // 2 + 1)
    single = np.stack([gdsp.spectral.Pwelch(r, FS, c["o"])[0] for r in c["x"]])
    imag = float(np.max(np.max(np.abs(pxy.imag), axis=1) / np.max(np.abs(pxy), axis=1)))
    err = row_nrel(pxy.real, single)
    print("self", IDS[i], "imag", imag, "real", err, "coh", float(np.max(np.abs(cxy - 1))))
    assert imag < EXACT and err < EXACT
    assert row_nrel(pxx, single) < EXACT and row_nrel(pyy, single) < EXACT
    assert np.max(np.abs(cxy - 1)) < 1e-12


@pytest.mark.parametrize("f,nsegs,k", [(256, 18, 5), (256, 18, 8), (2048, 5, 1), (2048, 5, 2)],
                         ids=["256-odd", "256-even", "2048-odd", "2048-even"])
def test_accumulation_adds_without_folding(gdsp, D, f, nsegs, k):
    import torch
    nfft, nov, channels = f, f // 2, 5
    hb = nfft // 2 + 1
    n = (nsegs - 1) * (nfft - nov) + nfft
    x, y = _signals(77, channels, n, False)
    xd, yd = _strided(x, 3), _strided(y, 5)
    win = torch.from_numpy(np.ascontiguousarray(gdsp.window.Hann(nfft))).cuda()
    whole = torch.zeros((channels + 1, 4, hb), dtype=torch.float64, device="cuda")
    parts = torch.zeros((channels + 1, 4, hb), dtype=torch.float64, device="cuda")
    whole[channels] = GUARD
    parts[channels] = GUARD
    D.cpsd_batch_accumulate(xd, yd, nfft, nfft, nov, 0, nsegs, win, whole[:channels])
    D.cpsd_batch_accumulate(xd, yd, nfft, nfft, nov, 0, k, win, parts[:channels])
    D.cpsd_batch_accumulate(xd, yd, nfft, nfft, nov, k, nsegs, win, parts[:channels])
    torch.cuda.synchronize()
    assert bool((whole[channels] == GUARD).all()) and bool((parts[channels] == GUARD).all())
    a, b = parts[:channels].cpu().numpy(), whole[:channels].cpu().numpy()
    # the planes are true sums of their range: they add as they are. Re and Im
    # of Sxy are judged together, as the complex row they are.
    for name, u, v in (("Sxx", a[:, 0], b[:, 0]), ("Syy", a[:, 1], b[:, 1]),
                       ("Sxy", a[:, 2] + 1j * a[:, 3], b[:, 2] + 1j * b[:, 3])):
        err = row_nrel(u, v)
        print("adds", f, k, name, err)
        assert err < EXACT, name


@pytest.mark.parametrize("k", [3, 4], ids=["odd", "even"])
@pytest.mark.parametrize("nfft,nov,no_fused", [(100, 30, False), (4096, 2048, False),
                                               (256, 128, True)],
                         ids=["100", "4096", "256-NO_FUSED_CPSD"])
def test_accumulation_adds_materialised(gdsp, D, nfft, nov, no_fused, k):
    """The same on the materialised form (gather, the plan's transform, partial
    sums), whose gather takes its own first segment: ranges [0, k) and [k, 7)
    against the whole, a tail shorter than a stride behind the last segment."""
    import torch
    F = gdsp.fft
    channels, nsegs = 3, 7
    hb = nfft // 2 + 1
    stride = nfft - nov
    n = (nsegs - 1) * stride + nfft + min(3, stride - 1)
    x, y = _signals(78 + nfft, channels, n, False)
    xd, yd = _strided(x, 3), _strided(y, 5)
    win = torch.from_numpy(np.ascontiguousarray(gdsp.window.Hann(nfft))).cuda()
    whole = torch.zeros((channels + 1, 4, hb), dtype=torch.float64, device="cuda")
    parts = torch.zeros((channels + 1, 4, hb), dtype=torch.float64, device="cuda")
    whole[channels] = GUARD
    parts[channels] = GUARD
    prev = F.Algorithm()
    try:
        if no_fused:
            F.SetAlgorithm(prev | F.ALGO_NO_FUSED_CPSD)
        assert not gdsp.spectral.cpsd_batch_fused(channels, n, nfft, nfft, nov)
        D.cpsd_batch_accumulate(xd, yd, nfft, nfft, nov, 0, nsegs, win, whole[:channels])
        D.cpsd_batch_accumulate(xd, yd, nfft, nfft, nov, 0, k, win, parts[:channels])
        D.cpsd_batch_accumulate(xd, yd, nfft, nfft, nov, k, nsegs, win, parts[:channels])
        torch.cuda.synchronize()
    finally:
        F.SetAlgorithm(prev)
    assert bool((whole[channels] == GUARD).all()) and bool((parts[channels] == GUARD).all())
    a, b = parts[:channels].cpu().numpy(), whole[:channels].cpu().numpy()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    for name, u, v in (("Sxx", a[:, 0], b[:, 0]), ("Syy", a[:, 1], b[:, 1]),
                       ("Sxy", a[:, 2] + 1j * a[:, 3], b[:, 2] + 1j * b[:, 3])):
        err = row_nrel(u, v)
        print("adds materialised", nfft, k, name, err)
        assert err < EXACT, name


@pytest.mark.parametrize("nfft,nov", [(32, 16), (4096, 2048), (3000, 1000), (100, 30)])
@pytest.mark.parametrize("one", [False, True], ids=["yc", "y1"])
def test_other_lengths_vs_reference(gdsp, oracle, D, nfft, nov, one):
    channels, nsegs = 3, 5
    n = (nsegs - 1) * (nfft - nov) + nfft + 2
    assert not gdsp.spectral.cpsd_batch_fused(channels, n, nfft, 0, nov)
    x, y = _signals(nfft, channels, n, one)
    o = _options(gdsp, nfft, nov, 0)
    got, freqs, _ = _run_guarded(D, _strided(x, 3), _strided(y, 5), o, nfft, nfft // 2 + 1)
    ref = _reference(oracle, x, y, nfft, nov, nfft)
    for name, a, b in zip(NAMES, got, ref):
        err = row_nrel(a, b)
        print("other", nfft, name, err)
        assert err < TOL, name
    assert np.array_equal(freqs, oracle.pwelch(x[0], FS, nfft=nfft, noverlap=nov)[1])
    assert np.all(got[0][:, 0].imag == 0)


@pytest.mark.parametrize("quiet", ["x", "y"])
@pytest.mark.parametrize("nfft,nov", [(64, 32), (256, 0), (2048, 1024), (100, 30)],
                         ids=["64", "256", "2048", "100-materialised"])
def test_first_segment_far_below_the_rest(gdsp, oracle, D, nfft, nov, quiet):
    """A level that changes by 1e12 after the first segment (a fade-in, a channel
    switched on late): every segment is balanced by its own level, so neither
    signal's spectrum loses digits to the other's."""
    channels, nsegs = 2, 2 * max(1, 1024 // nfft) + 2
    stride = nfft - nov
    n = (nsegs - 1) * stride + nfft + 1
    x, y = _signals(500 + nfft, channels, n, False)
    (x if quiet == "x" else y)[:, :nfft] *= 1e-12  # the whole of segment 0
    o = _options(gdsp, nfft, nov, 0)
    got, _, _ = _run_guarded(D, _strided(x, 3), _strided(y, 5), o, nfft, nfft // 2 + 1)
    ref = _reference(oracle, x, y, nfft, nov, nfft)
    for name, a, b in zip(NAMES, got, ref):
        err = row_nrel(a, b)
        print("quiet", quiet, nfft, name, err)
        assert err < TOL, name
    for name, a, rows in (("Pxx", got[1], x), ("Pyy", got[2], y)):
        err = row_nrel(a, np.stack([gdsp.spectral.Pwelch(r, FS, o)[0] for r in rows]))
        print("quiet", quiet, nfft, name, "spectral.Pwelch", err)
        assert err < EXACT, name


def test_host_entry_on_the_materialised_form(gdsp, oracle):
    """gdsp_cpsd_batch through its staging where no fused kernel serves the
    length: whole rows in one copy (NFFT 3000), and rows shorter than NFFT,
    staged row by row into zeroed rows of NFFT (n = 70, NFFT 100)."""
    S = gdsp.spectral
    for nfft, nov, n, one in ((3000, 1000, 7002, False), (100, 30, 70, False), (100, 30, 70, True)):
        assert not S.cpsd_batch_fused(3, n, nfft, 0, nov)
        x, y = _signals(nfft + n, 3, n, one)
        o = _options(gdsp, nfft, nov, 0)
        r = S.CpsdBatch(x, y, FS, o)
        ref = _reference(oracle, x, y, nfft, nov, nfft)
        for name, a, b in zip(NAMES, r[:4], ref):
            err = row_nrel(a, b)
            print("host materialised", nfft, n, name, err)
            assert err < TOL, name
        assert np.array_equal(r.freqs, oracle.pwelch(x[0], FS, nfft=nfft, noverlap=nov)[1])


def test_host_entries(gdsp, oracle, D):
    S = gdsp.spectral
    for i in (8, 5):  # y row by row, and one y
        c = _case(gdsp, oracle, D, i)
        r = S.CpsdBatch(c["x"], c["y"], FS, c["o"])
        for name, a, ref, dev in zip(NAMES, r[:4], c["ref"], c["got"]):
            assert row_nrel(a, ref) < TOL and row_nrel(a, dev) < EXACT, name
        assert np.array_equal(r.freqs, c["freqs"])
    c = _case(gdsp, oracle, D, 8)
    pxy, freqs = S.Cpsd(c["x"][1], c["y"][1], FS, c["o"])
    cxy, freqs2 = S.Coherence(c["x"][1], c["y"][1], FS, c["o"])
    assert row_nrel(pxy, c["ref"][0][1]) < TOL and row_nrel(cxy, c["ref"][3][1]) < TOL
    assert np.array_equal(freqs, c["freqs"]) and np.array_equal(freqs2, c["freqs"])
    # only Pxy asked for: the optional outputs may be NULL
    G = gdsp._lib
    x = np.ascontiguousarray(c["x"])
    y = np.ascontiguousarray(c["y"])
    nfft, nov, pad, _, n, channels, _ = _shape(TABLE[8])
    lp = pad // 2 + 1
    out = np.full((channels + 1, lp), GUARD + 0j)
    fr = np.empty(lp)
    lpo = G._I64(0)
    null = G._P()
    G.check(G.lib().gdsp_cpsd_batch(
        x.ctypes.data_as(G._P), n, y.ctypes.data_as(G._P), n, channels, channels, n, FS, nfft, pad,
        nov, null, null, 0, out.ctypes.data_as(G._P), null, null, null, fr.ctypes.data_as(G._P),
        lpo), "cpsd_batch")
    assert lpo.value == lp and np.all(out[channels] == GUARD)
    assert row_nrel(out[:channels], c["got"][0]) < EXACT


def test_short_signal_and_empty_input(gdsp, oracle, D):
    import torch
    S = gdsp.spectral
    o = S.PwelchOptions(NFFT=64)
    x, y = _signals(6, 3, 50, False)  # shorter than NFFT: zero-padded to NFFT
    ref = _reference(oracle, x, y, 64, 0, 64)
    got, freqs, _ = _run_guarded(D, _strided(x, 3), _strided(y, 5), o, 64, 33)
    host = S.CpsdBatch(list(x), list(y), FS, o)
    for name, a, h, b in zip(NAMES, got, host[:4], ref):
        assert row_nrel(a, b) < TOL and row_nrel(h, b) < TOL and row_nrel(h, a) < EXACT, name
    assert host.Pxy.shape == (3, 33)
    assert np.array_equal(freqs, oracle.pwelch(x[0], FS, nfft=64)[1])
    assert row_nrel(got[1], np.stack([S.Pwelch(r, FS, o)[0] for r in x])) < EXACT
    e = torch.zeros((2, 0), dtype=torch.float64, device="cuda")
    r = D.cpsd_batch(e, e, FS, o)
    assert tuple(r.Pxy.shape) == (2, 0) and r.Pxy.dtype == torch.complex128
    assert tuple(r.Cxy.shape) == (2, 0) and r.freqs.shape == (0,)
    r = S.CpsdBatch(np.zeros((3, 0)), np.zeros(0), FS, o)
    assert r.Pxy.shape == (3, 0) and r.freqs.shape == (0,)
    with pytest.raises(gdsp.Panic, match="arrays not of equal size"):
        D.cpsd_batch(_strided(x, 3), _strided(y[:2], 5), FS, o)


def test_side_stream_gives_the_same_bits(gdsp, oracle, D):
    import torch
    c = _case(gdsp, oracle, D, 11)  # caller's acc and outputs, the current stream
    xd, yd = _strided(c["x"], 3), _strided(c["y"], 5)
    r = D.cpsd_batch(xd, yd, FS, c["o"])
    torch.cuda.synchronize()
    for a, b in zip(r[:4], c["got"]):
        assert np.array_equal(a.cpu().numpy(), b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    r = D.cpsd_batch(xd, yd, FS, c["o"], stream=side)
    side.synchronize()
    for a, b in zip(r[:4], c["got"]):
        assert np.array_equal(a.cpu().numpy(), b)
    assert np.array_equal(r.freqs, c["freqs"])


def _wav(audio_format, bits, channels, data):
    """A 44-byte canonical header and the data chunk."""
    block = channels * bits // 8
    return (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " +
            struct.pack("<IHHIIHH", 16, audio_format, channels, 44100, 44100 * block, block, bits) +
            b"data" + struct.pack("<I", len(data)) + data)


def test_wav_coherence_of_channels(gdsp, oracle):
    W = gdsp.wav
    frames, channels = 5000, 3
    rng = np.random.default_rng(16)
    base = rng.standard_normal(frames)
    sig = np.stack([np.roll(base, 2 * c) + 0.5 * rng.standard_normal(frames)
                    for c in range(channels)])
    pcm = np.clip(np.round(sig * 4000.0), -32768, 32767).astype("<i2")
    data = np.ascontiguousarray(pcm.T).tobytes()  # interleaved frames
    want = oracle.wav_floats(data, frames * channels, 1, 16).astype(np.float64)
    rows = np.stack([want[c::channels] for c in range(channels)])
    o = gdsp.spectral.PwelchOptions(NFFT=256, Noverlap=128)
    for ref_ch in (0, 2):
        w = W.New(io.BytesIO(_wav(1, 16, channels, data)))
        assert w.NumChannels == channels
        cxy, freqs = W.CoherenceChannels(w, frames, o, ref=ref_ch)
        ref = _reference(oracle, rows, rows[ref_ch], 256, 128, 256, fs=44100.0)
        assert cxy.shape == (channels, 129)
        err = row_nrel(cxy, ref[3])
        print("wav", ref_ch, err)
        assert err < TOL
        assert np.max(np.abs(cxy[ref_ch] - 1)) < 1e-12
        assert np.array_equal(freqs, oracle.pwelch(rows[0], 44100.0, nfft=256, noverlap=128)[1])
    with pytest.raises(gdsp.GDSPError):
        W.CoherenceChannels(W.New(io.BytesIO(_wav(1, 16, channels, data))), frames, o, ref=3)
