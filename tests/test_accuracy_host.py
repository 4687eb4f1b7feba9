"""The accuracy tests' instrument, proved on the CPU (no GPU needed):

- the extended-precision reference (exact_dft.py) against direct extended sums,
  at every length test_accuracy_gpu.py uses;
- the float64 reference levels (numpy.fft against it) that become the GPU
  tests' bounds, held to [0.25 u, 64 u] so a broken reference cannot silently
  widen every bound;
- negative controls: four subtly wrong transforms, each of which must fail the
  very check() the GPU tests call, and one correct transform (the oracle at
  powers of 2) that must pass it.
"""
import numpy as np
import pytest

import exact_dft as E
import test_accuracy_gpu as G

LENGTHS = G.all_lengths()
LEVEL_LENGTHS = [16, 256, 257, 3000, 3001, 4096, 8209, 10000, 65536]


def test_no_length_beyond_the_reference_reach():
    # the self-check below holds 0.1 u up to these lengths only
    for n in LENGTHS:
        assert n <= (1 << 17 if E._is_pow2(n) else 20014), n


@pytest.mark.parametrize("n", LENGTHS)
def test_reference_self_check(n):
    """exact_fft against the direct sums at bins 0, 1, n // 2, n - 1 and 8
    seeded random bins: within 0.1 u of the row's largest output."""
    rows = (0, 2, 3) if n > 65536 else (0, 1, 2, 3)
    x = E.input_rows(n, rows=rows)
    ex = E.exact_standard(n, rows=rows)
    rnd = np.random.default_rng(n).integers(0, n, 8).tolist()
    ks = sorted({0, 1 % n, n // 2, n - 1} | set(rnd))
    d = np.abs(ex[:, ks] - E.exact_bins(x, ks)).max(axis=1) / np.abs(ex).max(axis=1)
    got = float(d.max() / E.U)
    print("self-check n=%d: %.4f u" % (n, got))
    assert got <= 0.1, (n, got)
    # the inverse is the forward's conjugate form: it must return the rows
    back = E.exact_fft(ex, inverse=True)
    assert E.err_u(x, back) <= 0.51  # x is float64: half an ulp of its largest entry at most


def _level(name, got):
    print("float64 level %s: %.3g u" % (name, got))
    assert 0.25 <= got <= 64, (name, got)


@pytest.mark.parametrize("n", LEVEL_LENGTHS)
def test_float64_reference_levels(n):
    x = E.input_rows(n)
    fwd, inv = E.exact_standard(n), E.exact_standard(n, inverse=True)
    for name, rows in (("noise", [0, 1]), ("impulse", [2]), ("tone", [3])):
        _level("fft %d %s" % (n, name), E.err_u(np.fft.fft(x[rows], axis=1), fwd[rows]))
        _level("ifft %d %s" % (n, name), E.err_u(np.fft.ifft(x[rows], axis=1), inv[rows]))
    xr = E.input_rows(n, real=True)
    _level("fft %d real rows" % n, E.err_u(np.fft.fft(xr, axis=1), E.exact_standard(n, real=True)))


@pytest.mark.parametrize("n", [256, 3000])
def test_float64_convolution_level(n):
    x, y = E.input_rows(n), E.uniform_rows(n + 1, 5, n)
    got = np.fft.ifft(np.fft.fft(x, axis=1) * np.fft.fft(y, axis=1), axis=1)
    _level("convolve %d" % n, E.err_u(got, E.exact_convolve(x, y)))


def test_float64_pwelch_level(gdsp):
    nfft, nov = 256, 128
    x = np.random.default_rng(nfft).uniform(-1, 1, 8 * (nfft - nov) + nfft + 3)
    w = gdsp.window.Hann(nfft)
    ex = E.exact_pwelch(x, 48000.0, nfft, nfft, nov, w, w)
    p = E.numpy_pwelch(x, 48000.0, nfft, nfft, nov, w, w)
    _level("pwelch max", E.err_u(p, ex))
    _level("pwelch per bin", E.err_u_per_bin(p, ex))


def test_exact_pwelch_is_the_reference_pwelch(oracle):
    """exact_pwelch restates spectral/pwelch.go:74-145: the oracle's Pwelch,
    the reference's own statement in float64, agrees with it to the oracle's
    accuracy, odd Pad, Pad < NFFT and scale_off included."""
    for nfft, pad, nov, off in ((64, 0, 32, False), (100, 257, 30, True), (128, 64, 5, False)):
        x = np.random.default_rng(nfft).uniform(-1, 1, 7 * (nfft - nov) + nfft + 3)
        p, _ = oracle.pwelch(x, 2.0, nfft=nfft, pad=pad, noverlap=nov, window_kind="hamming",
                             scale_off=off)
        f = max(pad or nfft, nfft)
        ex = E.exact_pwelch(x, 2.0, nfft, pad or nfft, nov, oracle.window("hamming", f),
                            oracle.window("hamming", nfft), off)
        assert ex.shape == p.shape
        assert E.err_u(p, ex) < 1e-9 / E.U


# ---- negative controls: each must fail the GPU tests' bound ---------------------

def _fails(family, n, got, e_ref):
    with pytest.raises(AssertionError):
        E.check(family, n, "control", got, e_ref, record=False)


@pytest.mark.parametrize("n", [3000, 3001, 8209])
def test_control_oracle_at_bluestein_lengths_fails(oracle, n):
    # the reference's unreduced chirp angle (fft/bluestein.go:53)
    x, ex = E.input_rows(n), E.exact_standard(n)
    _fails("control-oracle", n, E.err_u(oracle.fft_rows(x), ex),
           E.err_u(np.fft.fft(x, axis=1), ex))


@pytest.mark.parametrize("n", [16, 256, 4096, 65536])
def test_control_oracle_at_powers_of_2_passes(oracle, n):
    x, ex = E.input_rows(n), E.exact_standard(n)
    E.check("control-oracle", n, "pow2", E.err_u(oracle.fft_rows(x), ex),
            E.err_u(np.fft.fft(x, axis=1), ex), record=False)


def _radix2_f64(x, spoil_last=False):
    n = x.shape[1]
    if n == 1:
        return x
    k = np.arange(n // 2)
    w = np.exp(-2j * np.pi * k / n)
    if spoil_last:
        w = w.astype(np.complex64).astype(np.complex128)  # the twiddle through float
    e, o = _radix2_f64(x[:, 0::2]), _radix2_f64(x[:, 1::2]) * w
    return np.concatenate([e + o, e - o], axis=1)


def test_control_float_twiddles_in_the_last_stage_fail():
    n = 4096
    x, ex = E.input_rows(n), E.exact_standard(n)
    e_ref = E.err_u(np.fft.fft(x, axis=1), ex)
    E.check("control-radix2", n, "sound", E.err_u(_radix2_f64(x), ex), e_ref, record=False)
    _fails("control-radix2", n, E.err_u(_radix2_f64(x, spoil_last=True), ex), e_ref)


def test_control_dft13_constants_to_12_digits_fail():
    n = 13
    x, ex = E.input_rows(n), E.exact_standard(n)
    jk = np.outer(np.arange(n), np.arange(n)) % n
    w = np.exp(-2j * np.pi * jk / n)
    e_ref = E.err_u(np.fft.fft(x, axis=1), ex)
    E.check("control-dft13", n, "sound", E.err_u(x @ w, ex), e_ref, record=False)

    def digits12(v):
        return np.array([float("%.11e" % t) for t in v.ravel()]).reshape(v.shape)
    _fails("control-dft13", n, E.err_u(x @ (digits12(w.real) + 1j * digits12(w.imag)), ex), e_ref)


def test_control_product_recurrence_twiddles_fail():
    # w_{k+1} = w_k * w_1 over 4096 steps, as the column twiddles of a 4096-point transform
    n = 4096
    x, ex = E.input_rows(n), E.exact_standard(n)
    w = np.empty(n, np.complex128)
    w[0], w1 = 1.0, np.exp(-2j * np.pi / n)
    for k in range(1, n):
        w[k] = w[k - 1] * w1
    jk = np.outer(np.arange(n), np.arange(n)) % n
    _fails("control-recurrence", n, E.err_u(x @ w[jk], ex), E.err_u(np.fft.fft(x, axis=1), ex))
