/*
 * gdsp_fft.h — C ABI of libgdspfft, the MI355X (gfx950) batched-FFT engine for
 * the go-dsp hot path (maddyblue/go-dsp: fft/, spectral/Pwelch, window/Hann).
 *
 * This is the drop-in boundary: each entry point names the reference Go
 * function it replaces (file:line under maddyblue/go-dsp). A Go maintainer
 * binds these through cgo; tests bind them via ctypes.
 *
 * Conventions (mirroring the reference):
 *  - complex data are interleaved (re, im) IEEE float64 pairs, i.e. the memory
 *    layout of Go []complex128 and of C99 double _Complex;
 *  - inputs are never modified; outputs are caller-owned buffers that the
 *    library fills (Go allocates the result slice, C fills it);
 *  - the library never retains a caller pointer after returning (cgo rule);
 *  - every compute runs on the GPU. There is no CPU fallback: without a usable
 *    HIP device the calls return GDSP_ERR_NO_DEVICE;
 *  - the reference's panics become status codes; the Go shim re-panics with
 *    the reference's message (gdsp_status_string);
 *  - host-pointer entry points are synchronous and thread-safe; device-pointer
 *    entry points ("_device") are stream-ordered on the given hipStream_t
 *    (passed as void*; NULL = the null/default stream, as in HIP) and run on
 *    the calling thread's current HIP device.
 */
#ifndef GDSP_FFT_H
#define GDSP_FFT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ------------------------------------------------------------- */
typedef enum {
  GDSP_OK = 0,
  GDSP_ERR_INVALID = 1,        /* bad argument (negative size, NULL pointer, ...) */
  GDSP_ERR_UNEQUAL = 2,        /* "arrays not of equal size"   fft/fft.go:57 */
  GDSP_ERR_EMPTY = 3,          /* "empty input array"          fft/fft.go:126;
                                  IFFT of len 0 (index out of range, fft/fft.go:40) */
  GDSP_ERR_RAGGED = 4,         /* "ragged input array"         fft/fft.go:133 */
  GDSP_ERR_DIVIDE_BY_ZERO = 5, /* Segment stride 0 (integer divide, spectral.go:31) */
  GDSP_ERR_NO_DEVICE = 6,      /* no HIP device / runtime error at init */
  GDSP_ERR_HIP = 7,            /* HIP runtime error during a call */
  GDSP_ERR_NOMEM = 8,          /* device or host allocation failed */
  GDSP_ERR_UNSUPPORTED = 9     /* size beyond what this build implements */
} gdsp_status;

/* Reference panic message (or a description) for a status code. */
const char *gdsp_status_string(int status);
/* Detail of the last error raised on the calling thread ("" if none). */
const char *gdsp_last_error(void);
/* Library version string. */
const char *gdsp_version(void);
/* Runtime compiler (hipRTC specialisations of smooth lengths) since process
 * start: modules compiled, modules loaded from the on-disk code-object cache
 * (GDSP_JIT_CACHE), and compilations that failed — each failure leaves its
 * plan on the slower path it would have replaced, with the same results. The
 * last failure's description is copied into last_failure (cap bytes, NUL-
 * terminated; may be NULL). */
int gdsp_jit_stats(int64_t *built, int64_t *cached, int64_t *failed, char *last_failure,
                   int64_t cap);
/* Number of visible HIP devices (0 without a GPU; never initialises a context
 * beyond hipGetDeviceCount). */
int gdsp_device_count(void);

/* Algorithm selection (no reference equivalent; additive). Every selection
 * computes the same DFT (the reference's results within the 1e-9 bound)
 * by another of the engine's paths; the default (0) takes the measured
 * fastest. Flags apply to plans built after the call (plans are cached per
 * length and flag set) and to Pwelch calls made after it; process-wide. */
enum {
  GDSP_ALGO_DEFAULT = 0,
  /* smooth non-power-of-2 lengths (transforms and fused Pwelch) on the
   * runtime-radix mixed kernels, without the compiled or runtime-compiled
   * (hipRTC) specialisations */
  GDSP_ALGO_GENERIC_MIXED = 1,
  /* primes in (8192, 14563] on the composed chirp-z instead of the
   * output-split fused kernel */
  GDSP_ALGO_NO_CHIRPZ_PARTS = 2,
  /* chirp-z on the reference's M = NextPowerOf2(2n-1) (fft/bluestein.go:70)
   * instead of a smaller smooth M: the composed chirp-z, and the fused one
   * for 129 <= n <= 3200 and 4097 <= n <= 6144 (by default M = 16 * RB * 16
   * or 16 * R1 * R2 * 16, the smallest kept one >= 2n - 1 where not above
   * the power of 2) */
  GDSP_ALGO_CHIRPZ_POW2 = 4,
  /* the composed chirp-z without its fused transposes */
  GDSP_ALGO_CHIRPZ_UNFUSED = 8,
  /* primes n <= 8193 whose n - 1 has a radix list, and the composites of
   * plan kind 8, on the chirp-z kernels instead of Rader's algorithm (plan
   * kinds 7 and 8) */
  GDSP_ALGO_NO_RADER = 16,
  /* no plan-time measurement: where the default races two kernels on
   * synthetic rows when a plan is built (plan kinds 7 and 8, Rader and the
   * prime-factor Rader, each against the chirp-z plan it would replace; the
   * fused chirp-z on a smooth convolution length against the one on a power
   * of 2) and keeps the faster, take the cost model's candidate instead */
  GDSP_ALGO_NO_RACE = 32,
  /* gdsp_convolve_batch / gdsp_convolve_batch_device on the composed path
   * (FFT, row multiply, IFFT: three kernels) also for the powers of 2 the
   * fused one-kernel convolution serves. Read when the call is made, not
   * when the plan is built. */
  GDSP_ALGO_NO_FUSED_CONVOLVE = 64,
  /* gdsp_pwelch_batch / gdsp_pwelch_batch_accumulate_device as a loop of
   * gdsp_pwelch_accumulate_device over the channels also for the lengths the
   * batched kernel serves. Read when the call is made. */
  GDSP_ALGO_NO_FUSED_PWELCH_BATCH = 128,
  /* gdsp_cpsd_batch / gdsp_cpsd_batch_accumulate_device on the materialised
   * form (gathered rows, the plan's batched transform, a kernel over each row
   * and its mirror) also for the lengths the fused cross-spectral kernel
   * serves. Read when the call is made. */
  GDSP_ALGO_NO_FUSED_CPSD = 256,
  /* gdsp_fir_batch / gdsp_fir_batch_device on the composed form (gathered
   * blocks, the plan's batched transform, row multiply, inverse transform,
   * scatter of the valid parts) also for the block lengths the fused
   * overlap-save kernel serves. Read when the call is made. */
  GDSP_ALGO_NO_FUSED_FIR = 512,
  /* gdsp_stft_batch / gdsp_spectrogram_batch and their device entries on the
   * materialised form (gathered real rows, the plan's batched transform, a
   * kernel that writes the first lp bins or their powers) also for the lengths
   * the fused per-segment kernel serves. Read when the call is made. */
  GDSP_ALGO_NO_FUSED_STFT = 1024,
  /* gdsp_istft_batch and its device entry on the materialised form (rows
   * completed to dense complex rows, the plan's batched inverse transform, an
   * overlap-add kernel with one thread per output sample) also for the shapes
   * the fused overlap-add kernel serves. Read when the call is made. The bit
   * 2048 is not used: it stays an unknown bit. */
  GDSP_ALGO_NO_FUSED_ISTFT = 4096,
  /* gdsp_upfirdn_batch / gdsp_upfirdn_batch_device on the plain form (one
   * thread per output, taps and samples from global memory) also for the
   * shapes the fused polyphase kernel serves. Read when the call is made. */
  GDSP_ALGO_NO_FUSED_UPFIRDN = 8192,
  /* gdsp_hilbert_batch / gdsp_hilbert_batch_device on the composed form
   * (gathered real rows, the plan's real-row transform, the multiplier, the
   * plan's inverse, a store kernel) also for the powers of 2 the fused
   * analytic-signal kernel serves. Read when the call is made. The bit 16384
   * is not used, like 2048: both stay unknown bits. */
  GDSP_ALGO_NO_FUSED_HILBERT = 32768,
  /* gdsp_sosfilt_batch, gdsp_sosfiltfilt_batch and their device entries on the
   * plain form (one thread per row, sample by sample from global memory) also
   * for the filters the time-parallel kernel serves; gdsp_sosfilt_fused then
   * reports 0. Read when the call is made. */
  GDSP_ALGO_NO_FUSED_SOSFILT = 65536,
  /* gdsp_czt_batch / gdsp_czt_batch_device on the composed form (a
   * premultiply-and-pad kernel, the plan's transform, the product with the
   * chirp's spectrum, the plan's transform again, a postmultiply-and-store
   * kernel) also for the convolution lengths the fused chirp-z kernel serves;
   * gdsp_czt_fused then reports 0. Read when the call is made. The bit 131072
   * is not used, like 2048 and 16384: all three stay unknown bits. */
  GDSP_ALGO_NO_FUSED_CZT = 262144,
  /* gdsp_dct_batch / gdsp_dct_batch_device on the composed form (type II: a
   * permute-and-pad kernel, the plan's real-row transform, a twiddle-and-store
   * kernel; type III: a kernel that writes the rows of conj W, the plan's
   * transform, an un-permute store) also for the powers of 2 the fused
   * cosine-transform kernel serves; gdsp_dct_fused then reports 0. Read when
   * the call is made. The bits 1 << 19 and 1 << 20 are not used, like 2048,
   * 16384 and 131072: all five stay unknown bits. */
  GDSP_ALGO_NO_FUSED_DCT = 2097152
};
/* Unknown bits → GDSP_ERR_INVALID (the selection is left unchanged). */
int gdsp_set_algorithm(unsigned flags);
unsigned gdsp_get_algorithm(void);

/* ---- values: scale, non-finite samples, earlier calls ----------------------
 * What every entry below, host-pointer or device-pointer, promises about the
 * values it is given (tests/test_values_gpu.py):
 *  - No call depends on an earlier one: workspace, work buffers, accumulators
 *    the library zeroes and outputs may hold anything, NaN included, when a
 *    call starts; the same inputs give the same bits.
 *  - No absolute threshold: inputs times 2^k give outputs times the matching
 *    power of 2 bit for bit (transforms 2^k; Convolve and FIR 2^(a+b) for x
 *    times 2^a and y or h times 2^b; Pwelch 2^2k; cross spectra Pxx 2^2a, Pyy
 *    2^2b, Pxy 2^(a+b), the coherence unchanged; STFT rows 2^k, spectrogram
 *    rows 2^2k), while no intermediate leaves
 *    the normal range and, for cross spectra, the two levels stay within the
 *    balance's range (gdsp_cpsd_batch). All-zero inputs give exact zeros.
 *  - A NaN or an infinity in the input makes non-finite exactly what depends
 *    on it, and nothing else changes by a bit:
 *      transforms, Convolve   every element of that row (a complex NaN: NaN
 *                             in both parts); a y shared by all rows: all rows
 *      FFT2, FFTN             every output; one axis: the lines through it
 *      Pwelch, batched        every bin of that channel
 *      cross spectra          all four results of that channel, the other
 *                             signal's P included: one transform carries a
 *                             segment of both signals (a shared y: all channels)
 *      STFT, spectrogram      every bin of the rows of the segments that hold
 *                             the sample (tests/test_stft_gpu.py)
 *      ISTFT                  a bad used element of row (c, s): non-finite
 *                             samples only among [s*stride, s*stride + nfft)
 *                             of channel c with D > 0; all of those for a bad
 *                             real part of bin 0 or F/2, which has a weight in
 *                             every sample (another bin's cosine or sine is
 *                             exactly 0 at some samples, which the transform
 *                             may or may not reach); zero-weight terms are
 *                             not skipped. Rows times 2^k give samples times
 *                             2^k; every sample is summed over its segments
 *                             in ascending s (tests/test_istft_gpu.py)
 *      FIR                   outputs [j, j + m) of that row for a bad x[j],
 *                             and possibly more of (j - 2F, j + 2F), F =
 *                             gdsp_fir_block's: a transform carries two blocks
 *                             of F - m + 1 outputs and a sample is read by at
 *                             most two transforms. scipy.signal.lfilter would
 *                             confine it to [j, j + m).
 *      resampling            a bad x[c, i] (gdsp_upfirdn_batch and its device
 *                             entry): every output j of row c with 0 <= j*down
 *                             - i*up < m, none outside 0 <= j*down - i*up <
 *                             T*up, T = ceil(m / up) (the taps are padded with
 *                             zeros to T per phase, and zero-weight terms are
 *                             not skipped); x times 2^a and h times 2^b give
 *                             the outputs times 2^(a+b); a phase without a tap
 *                             gives +0.0; every output is summed in ascending t
 *                             with one fused multiply-add per term, so its bits
 *                             do not depend on the range, chunk, tile or form
 *                             that computes it (tests/test_resample_gpu.py)
 *      Hilbert               every output of that row (analytic: the imaginary
 *                             part; the real part is the input's bits), and no
 *                             bit of any other row: both forms run one row
 *                             per transform, so a row's outputs depend on that
 *                             row alone, whatever its neighbours hold and
 *                             however a job is cut into calls. A row of exact
 *                             zeros gives exact zeros; a quiet row beside a
 *                             loud one keeps its own relative accuracy; rows
 *                             times 2^k give outputs times 2^k
 *                             (tests/test_hilbert_gpu.py)
 *      recursive filters     (gdsp_sosfilt_batch, gdsp_sosfiltfilt_batch and
 *                             their device entries, both forms) a row's outputs
 *                             and final state depend on that row alone, bit for
 *                             bit; x times 2^k (and zi times 2^k) gives y and zf
 *                             times 2^k; a zero row with zero zi gives exact
 *                             zeros. A bad x[c, j] makes every output i >= j of
 *                             row c and its zf non-finite (sections whose a1, a2
 *                             are not zero never forget it) and changes no bit of
 *                             the outputs i < j, nor of any other row: every
 *                             step of the scans takes from earlier samples
 *                             only, by a select, never by a zero weight.
 *                             sosfiltfilt: the whole row, and no other row.
 *                             Stale out, work and zf buffers change nothing
 *                             (tests/test_sosfilt_gpu.py)
 *      CZT                   (gdsp_czt_batch, gdsp_czt_batch_device, both forms)
 *                             a row depends on itself alone, bit for bit,
 *                             whatever its neighbours hold and however a job
 *                             is cut into calls, and a zero row gives zeros. A
 *                             NaN or Inf in a row makes all m outputs of that
 *                             row non-finite, in both parts, and changes no bit
 *                             elsewhere; rows times 2^k give outputs times 2^k
 *                             (the inverse's 1 / F is a power of 2, folded into
 *                             the chirp's spectrum) (tests/test_czt_gpu.py)
 *      DCT                   (gdsp_dct_batch, gdsp_dct_batch_device, both types,
 *                             every norm, both forms) a row depends on itself
 *                             alone, bit for bit, whatever its neighbours hold
 *                             and however a job is cut into calls, ranges or
 *                             chunks. A row of zeros gives exact zeros; rows
 *                             times 2^k give outputs times 2^k for every norm
 *                             (each norm is one multiplication by a constant
 *                             after the transform; ortho's type III one more on
 *                             x[0] before it). A NaN or Inf in a row makes
 *                             every output of that row non-finite and changes
 *                             no bit of another row. Stale out and work
 *                             contents change nothing (tests/test_dct_gpu.py) */

/* ---- fft package: host pointers, synchronous ----------------------------- */

/* fft.FFT — fft/fft.go:72-87. n <= 1 copies; power of 2 → Stockham radix-16
 * kernels (reference: radix2FFT, fft/radix2.go:80-154); other n whose prime
 * factors are all <= 13 → a mixed-radix Stockham kernel (n <= 4096) or, above
 * 8192, a four-step over two such factors, computing the same DFT directly;
 * otherwise Bluestein (fft/bluestein.go:68-94).
 * x, out: n complex128. */
int gdsp_fft(const double *x, double *out, int64_t n);

/* fft.IFFT — fft/fft.go:35-52. n == 0 → GDSP_ERR_EMPTY (reference panics). */
int gdsp_ifft(const double *x, double *out, int64_t n);

/* fft.FFTReal — fft/fft.go:25-27. x: n float64; out: n complex128 (full
 * spectrum, as the reference returns). */
int gdsp_fft_real(const double *x, double *out, int64_t n);

/* fft.IFFTReal — fft/fft.go:30-32. */
int gdsp_ifft_real(const double *x, double *out, int64_t n);

/* fft.Convolve — fft/fft.go:55-69 (IFFT(FFT(x)·FFT(y))). The reference's
 * length check ("arrays not of equal size") is the caller's: both are n. */
int gdsp_convolve(const double *x, const double *y, double *out, int64_t n);

/* Additive batched fft.Convolve (no reference equivalent): rows of x (batch ×
 * n complex128) each convolved with y: y_rows == 1 → one y (n complex128) for
 * all rows, y_rows == batch → row by row (y is batch × n). fft.Convolve per
 * row. n < 0, batch < 0, y_rows neither 1 nor batch, or a NULL pointer with
 * batch > 0 → GDSP_ERR_INVALID; n == 0 with batch > 0 → GDSP_ERR_EMPTY (as
 * gdsp_convolve); batch == 0 → GDSP_OK, nothing done. Runs on the current
 * device. */
int gdsp_convolve_batch(const double *x, const double *y, double *out,
                        int64_t n, int64_t batch, int64_t y_rows);

/* Additive FIR filtering of real rows (no reference equivalent; the causal
 * filter of scipy.signal.lfilter(h, 1, x), or numpy.convolve(x, h)): for
 * `channels` rows of n float64, row c at x + c*ldx, and m real taps,
 *   out[c*ldo + i] = sum over k < m of h[k] * x[c*ldx + i - k],
 * x taken as zero outside [0, n); i in [0, n) with full == 0, in
 * [0, n + m - 1) with full == 1 (the tail lets a caller overlap-add the
 * chunks of a stream). h_rows == 1 → one h for all rows, h_rows == channels →
 * row c takes h + c*m. Strides in doubles. Computed by overlap-save on blocks
 * of F = gdsp_fir_block(m, block) points: where that reports `fused`, one
 * kernel per call after the spectrum of the taps (two overlapping blocks of a
 * row per transform as a + i b, FFT_F, times FFT_F(h), inverse FFT_F, the valid
 * parts of Re and Im stored: the samples are read about once and written
 * once); otherwise the composed form in chunks of at most 256 MiB of blocks.
 * out may alias x: the caller's memory is only touched by host memcpy.
 * In this order, before any device call: a negative size, full not 0 or 1,
 * h_rows neither 1 nor channels, a block that gdsp_fir_block rejects for
 * another reason than m's range, ldx < n or ldo < the output length with
 * channels > 1 → GDSP_ERR_INVALID; channels == 0 → GDSP_OK, nothing done;
 * n == 0 or m == 0 → GDSP_ERR_EMPTY (as numpy.convolve refuses empty input);
 * m beyond the composed form's range → GDSP_ERR_UNSUPPORTED; a NULL pointer →
 * GDSP_ERR_INVALID. Runs on the current device. */
int gdsp_fir_batch(const double *x, int64_t ldx, const double *h, int64_t h_rows, int64_t m,
                   int64_t channels, int64_t n, int full, int64_t block, double *out,
                   int64_t ldo);

/* The overlap-save block length F of a gdsp_fir_batch call with m taps (no
 * reference equivalent), or 0 where that call would fail; host arithmetic on
 * a committed cost table, the same answer every time, no GPU needed. block: a
 * power of 2, 256 <= block <= 2^20, block >= 2m, is taken as it is; 0 → the
 * library's choice: for m <= 8192 the F in {256 ... 16384}, F >= 2m, of least
 * cost(F) * F / (F - m + 1); above, the smallest power of 2 >= 4 (m - 1), up
 * to 2^20. *fused (may be NULL): 1 where the fused kernel serves F and m
 * (256 <= F <= 16384, m <= F/2) under the current flags (a call whose grid
 * would pass 2^31 - 1 workgroups still runs composed). */
int64_t gdsp_fir_block(int64_t m, int64_t block, int *fused);

/* Additive polyphase resampling of real rows (no reference equivalent;
 * scipy.signal.upfirdn(h, x, up, down): zero-stuff by up, filter, keep every
 * down-th sample): for `channels` rows of n float64, row c at x + c*ldx, m
 * real taps h (one set for all rows) and integers up, down >= 1,
 *   out[c, j] = sum over i of h[j*down - i*up] * x[c, i],
 *               0 <= j*down - i*up < m, 0 <= i < n,
 *   j in [0, L), L = gdsp_upfirdn_length(n, m, up, down)
 *              = ((n - 1)*up + m - 1) div down + 1,
 * computed in polyphase form: with p = (j*down) mod up, i0 = (j*down) div up,
 * T = ceil(m / up): out[c, j] = sum over t < T of h[p + t*up] * x[c, i0 - t],
 * taps at index >= m and samples outside the row counting as 0, summed in
 * ascending t. Outputs [out_begin, out_end) of every row are written to out +
 * c*ldo (out_end == -1: L). Strides in doubles. Longer jobs are cut into
 * ranges of outputs: the device buffers hold at most 2^25 doubles of output
 * per chunk (UPFIRDN_CHUNK_ELEMS) and the input span that chunk reads.
 * In this order, before any device call: a negative size, up < 1 or down < 1,
 * a range not within 0 <= out_begin <= out_end <= L, or, with channels > 1,
 * ldx < n or ldo < out_end - out_begin -> GDSP_ERR_INVALID; channels == 0 ->
 * GDSP_OK, nothing done; n == 0 or m == 0 -> GDSP_ERR_EMPTY; up or down above
 * 65536, m above 2^24, or (n - 1)*up + m not representable in int64 ->
 * GDSP_ERR_UNSUPPORTED; a NULL pointer -> GDSP_ERR_INVALID; an empty range ->
 * GDSP_OK. Runs on the current device. */
int gdsp_upfirdn_batch(const double *x, int64_t ldx, const double *h, int64_t m, int64_t up,
                       int64_t down, int64_t channels, int64_t n, int64_t out_begin,
                       int64_t out_end, double *out, int64_t ldo);
/* L of gdsp_upfirdn_batch: 0 for n == 0 or m == 0, -1 where the call would be
 * refused for its sizes (GDSP_ERR_INVALID or GDSP_ERR_UNSUPPORTED above). Host
 * arithmetic only. */
int64_t gdsp_upfirdn_length(int64_t n, int64_t m, int64_t up, int64_t down);
/* 1 where the fused polyphase kernel serves m taps at up/down under the
 * current flags (the phase table of up * ceil(m / up) doubles and the samples
 * of the smallest tile fit 64 KiB of LDS), 0 where the plain form runs (also
 * for sizes the call refuses, and under GDSP_ALGO_NO_FUSED_UPFIRDN). Host
 * arithmetic on committed constants, no GPU needed. */
int gdsp_upfirdn_fused(int64_t m, int64_t up, int64_t down);

/* Additive analytic signal of real rows (no reference equivalent;
 * scipy.signal.hilbert(x, N)): for `rows` rows of n float64, row r at x +
 * r*ldx, and a transform length N (nfft; 0: n), row r is cut to N samples or
 * padded with zeros to N, and
 *   h_r = IFFT_N(m * FFT_N(x_r)),  m[f] = -i for 0 < f < N/2, +i for N/2 < f <
 *   N, 0 at f = 0 and (N even) at f = N/2; h_r is real.
 * N elements per row go to out + r*ldo:
 *   GDSP_HILBERT_ANALYTIC    complex128 x_r[i] + i h_r[i]; the real part is the
 *                            input sample's own bits (+0.0 in the padding)
 *   GDSP_HILBERT_QUADRATURE  float64 h_r[i]
 *   GDSP_HILBERT_ENVELOPE    float64 sqrt(fma(x, x, h*h))
 * ldx in doubles, ldo in output elements (complex128 for ANALYTIC). Where
 * gdsp_hilbert_fused(N), one kernel per call: a row as one complex transform
 * (z = x + 0i), the multiplier as a swap of re and im, the inverse, the
 * store; otherwise the composed form (gathered rows, the plan's real-row
 * transform, the multiplier, the plan's inverse, a store kernel) in chunks of
 * at most 2^24 samples. Longer host jobs are cut into ranges of rows that
 * start at even rows, of at most 2^24 samples (HILBERT_CHUNK_ELEMS); a row's
 * bits do not depend on the range it falls in.
 * In this order, before any device call: a negative size, a kind outside
 * 0..2, or, with rows > 1, ldx < n or ldo < N -> GDSP_ERR_INVALID; rows == 0 ->
 * GDSP_OK, nothing done; n == 0 or N == 0 -> GDSP_ERR_EMPTY; a NULL pointer ->
 * GDSP_ERR_INVALID. Runs on the current device. */
enum {
  GDSP_HILBERT_ANALYTIC = 0,
  GDSP_HILBERT_QUADRATURE = 1,
  GDSP_HILBERT_ENVELOPE = 2
};
int gdsp_hilbert_batch(const double *x, int64_t ldx, int64_t rows, int64_t n, int64_t nfft,
                       int kind, double *out, int64_t ldo);
/* 1 where the fused analytic-signal kernel serves transform length nfft under
 * the current flags (a power of 2 from 256 to 16384, without
 * GDSP_ALGO_NO_FUSED_HILBERT), 0 where the composed form runs. Host arithmetic
 * only, no GPU needed. */
int gdsp_hilbert_fused(int64_t nfft);

/* Additive recursive (IIR) filtering of real rows by second-order sections (no
 * reference equivalent; scipy.signal.sosfilt(sos, x, axis=1, zi=zi)): for
 * `channels` rows of n float64, row c at x + c*ldx, and S sections sos[S][6] =
 * (b0, b1, b2, a0, a1, a2) with a0 == 1, one set for all rows, every section
 * is the transposed direct form II
 *   y = b0*x + z0;   z0 = b1*x - a1*y + z1;   z1 = b2*x - a2*y,
 * the sections applied in cascade order. zi[channels][S][2]: the states the
 * rows start from (NULL: zeros); zf, same shape (NULL: not wanted): the states
 * after the last sample, so that filtering [0, n1) and then [n1, n) with zi =
 * zf is filtering [0, n). Strides in doubles.
 * Two forms. Where gdsp_sosfilt_fused(sos, S) — 1 <= S <= 8, every section
 * strictly inside the stability triangle |a2| < 1, |a1| < 1 + a2 — the
 * time-parallel form: rows are cut into tiles of 4096 samples; pass 1 runs
 * every tile from zero state and keeps its end state; pass 2 carries st[k+1] =
 * Phi st[k] + g[k] along each row (Phi = A^4096 of the cascade, 2S x 2S, from
 * the host in long double); pass 3 runs every tile from its true state and
 * stores each sample once. Inside a tile a thread owns 16 samples and the
 * threads' states are scanned through M^(2^k), M = A^16 of a section. A row of
 * one tile runs pass 3 alone. Otherwise the plain form: one thread per row,
 * sample by sample; any S <= 64 and any finite coefficients, unstable ones
 * included. Both follow the recurrence above in fused multiply-adds; the
 * time-parallel form differs from it by a small multiple of the recurrence's
 * own roundoff.
 * Cuts in time: G = gdsp_sosfilt_granule(S). A call on [0, k*G) followed by a
 * call on [k*G, n) with zi = zf gives the bits of one call on [0, n); zf at
 * such a cut is pass 2's value. The host entry cuts rows at multiples of G
 * into chunks of at most 2^25 samples over all rows (SOSFILT_CHUNK_ELEMS), so
 * host and device results are equal bit for bit. A cut elsewhere is equal
 * within the accuracy of the form.
 * In this order, before any device call: a negative size, or, with channels >
 * 1, ldx < n or ldo < n -> GDSP_ERR_INVALID; channels == 0 -> GDSP_OK, nothing
 * done; n == 0 or S == 0 -> GDSP_ERR_EMPTY; S > 64 -> GDSP_ERR_UNSUPPORTED; a
 * NULL x, sos or out -> GDSP_ERR_INVALID; an a0 other than 1 or a coefficient
 * that is not finite -> GDSP_ERR_INVALID. out may alias x: the caller's memory
 * is only touched by host memcpy, chunk by chunk, each read before it is
 * written. Runs on the current device. */
int gdsp_sosfilt_batch(const double *x, int64_t ldx, const double *sos, int64_t S,
                       const double *zi, int64_t channels, int64_t n, double *out, int64_t ldo,
                       double *zf);
/* 1 where the time-parallel kernel serves these sections under the current
 * flags, 0 where the plain form runs (also for arguments the call refuses, and
 * under GDSP_ALGO_NO_FUSED_SOSFILT). Host arithmetic, no GPU needed. */
int gdsp_sosfilt_fused(const double *sos, int64_t S);
/* G of the cuts above: 4096 for 1 <= S <= 64 (pass 2 is sequential over the
 * tiles, so every tile boundary is a cut), 0 otherwise. Host arithmetic. */
int64_t gdsp_sosfilt_granule(int64_t S);
/* scipy.signal.sosfilt_zi(sos): zi[S][2], the states of the settled unit step
 * response — per section, with g = (b0 + b1 + b2) / (1 + a1 + a2): z1 = b2 -
 * a2 g, z0 = b1 - a1 g + z1, times the product of the earlier sections' g —
 * in long double, rounded once. S < 0, a NULL pointer with S > 0, an a0 other
 * than 1, a coefficient that is not finite or a section with 1 + a1 + a2 == 0
 * -> GDSP_ERR_INVALID. Host arithmetic, no GPU needed. */
int gdsp_sosfilt_zi(const double *sos, int64_t S, double *zi);
/* Zero-phase filtering (scipy.signal.sosfiltfilt(sos, x, axis=1, padtype="odd",
 * padlen=padlen)): every row is extended by padlen samples at both ends by odd
 * reflection (2 x[0] - x[padlen - v] before, 2 x[n-1] - x[n-2-v] after),
 * filtered forward from the state gdsp_sosfilt_zi times the extension's first
 * sample, that result filtered backward from gdsp_sosfilt_zi times its last
 * sample, and the middle n samples kept. padlen == -1: scipy's default,
 * gdsp_sosfiltfilt_padlen. Both passes run gdsp_sosfilt_batch's forms; the
 * extension is formed by the kernels' loader and never stored. The host entry
 * cuts both passes in time at multiples of G and holds the intermediate, n + 2
 * padlen doubles per row, in host memory; its results equal the device entry's
 * bit for bit. gdsp_sosfilt_batch's checks in its order, padlen < -1 with the
 * negative sizes; then n <= padlen, or a section with 1 + a1 + a2 == 0 ->
 * GDSP_ERR_INVALID. */
int gdsp_sosfiltfilt_batch(const double *x, int64_t ldx, const double *sos, int64_t S,
                           int64_t padlen, int64_t channels, int64_t n, double *out,
                           int64_t ldo);
/* 3 * (2 S + 1 - min(#{b2 == 0}, #{a2 == 0})), scipy's default padlen; -1 for a
 * NULL sos or S outside 1..64. Host arithmetic. */
int64_t gdsp_sosfiltfilt_padlen(const double *sos, int64_t S);
/* Doubles of d_work a device entry below takes (more than it uses where the
 * plain form runs); -1 for sizes the calls refuse. Host arithmetic. */
int64_t gdsp_sosfilt_work_doubles(int64_t S, int64_t channels, int64_t n);
int64_t gdsp_sosfiltfilt_work_doubles(int64_t S, int64_t channels, int64_t n, int64_t padlen);

/* The chirp-z transform of rows on an arc of a circle (no reference
 * equivalent; scipy.signal.czt with |w| = 1 and scipy.signal.zoom_fft): the
 * z-transform of every row on m points
 *   z_k  = a_abs * exp(2 pi i (a_turns + k * step)),  step = step_turns / step_div
 *   X[k] = sum_{j<n} x[j] * z_k^(-j),                 k = 0 ... m-1
 * (angles in turns; scipy's w = exp(-2 pi i step), a = a_abs exp(2 pi i
 * a_turns)). The step is the rational number step_turns / step_div taken
 * EXACTLY, not the rounded quotient: step_turns = 1, step_div = m = n is the
 * DFT itself, and zoom_fft(fn = [f1, f2], m, fs, endpoint) is a_turns = f1 /
 * fs, step_turns = (f2 - f1) / fs, step_div = m (m - 1 with endpoint). X[k]
 * moves by about 2 pi n m d for an error d in the step, which is why the ABI
 * takes reals and a divisor and no complex w. a_abs != 1 is a circle of
 * another radius (rows damped by a_abs^-j); a_abs^-(n-1) must stay inside the
 * normal double range. Spirals (|w| != 1) are NOT offered: Bluestein's split of
 * |w|^(jk) into |w|^(+-j^2/2) makes the convolution's error relative to the
 * largest of those factors (6e16 u at n = m = 1000 with a chirp range of
 * e^+-40, in scipy as well), and the engine does not offer what it cannot
 * compute.
 * With c(j) = exp(-pi i step j^2) and F = gdsp_czt_length(n, m):
 *   A[j] = a_abs^-j exp(-2 pi i j a_turns) c(j), j < n;  P[k] = c(k), k < m
 *   v[d mod F] = conj(c(d)), -(n-1) <= d <= m-1, zero elsewhere
 *   X[k] = P[k] IFFT_F(FFT_F(x A, zero-padded) FFT_F(v))[k]
 * Every angle (j^2 step_turns / (2 step_div) and j a_turns turns, modulo 1) is
 * reduced exactly in integers on the parameters' significands before any
 * floating-point trigonometry; sine, cosine and a_abs^-j are then taken in long
 * double and rounded once.
 *
 * gdsp_czt_tables: A (n), v (F) and P (m) complex128 for any F >= n + m - 1, F
 * <= 2^20. Host arithmetic, no GPU needed. n < 1, m < 1, F out of range, a NULL
 * pointer, a_abs <= 0, a parameter that is not finite, step_div < 1, or an
 * entry of A whose modulus is not finite and normal -> GDSP_ERR_INVALID. */
int gdsp_czt_tables(int64_t n, int64_t m, int64_t F, double a_abs, double a_turns,
                    double step_turns, int64_t step_div, double *A, double *v, double *P);
/* The convolution length F = max(256, the next power of 2 >= n + m - 1), or 0
 * where it would exceed 2^20 (or n < 1 or m < 1): the entries then return
 * GDSP_ERR_UNSUPPORTED. *fused (may be NULL): 1 where F <= 16384 and
 * GDSP_ALGO_NO_FUSED_CZT is clear. Host arithmetic. */
int64_t gdsp_czt_length(int64_t n, int64_t m, int *fused);
/* 1 where the fused chirp-z kernel serves (n, m) under the current flags, 0
 * where the composed form runs or nothing does. Host arithmetic. */
int gdsp_czt_fused(int64_t n, int64_t m);
/* gdsp_czt_batch: `rows` rows of n float64 (is_real = 1) or complex128
 * (is_real = 0), row r at x + r*ldx elements, m complex128 per row to out +
 * r*ldo complex128. Host pointers, synchronous; builds and frees its plan.
 * Where gdsp_czt_fused(n, m), one kernel per range: a row times A as it is
 * loaded, FFT_F, times FFT_F(v) / F, the second FFT_F as the inverse with P on
 * its last pass, m outputs stored; otherwise the composed form in chunks of at
 * most 2^24 / F rows. Host jobs are cut into ranges of at most 2^24 / F rows; a
 * row's bits do not depend on the range it falls in.
 * In this order, before any device call: a negative size, is_real outside 0..1,
 * with rows > 1 ldx < n or ldo < m, a_abs <= 0, a parameter that is not finite
 * or step_div < 1 -> GDSP_ERR_INVALID; rows == 0 -> GDSP_OK, nothing done; n ==
 * 0 or m == 0 -> GDSP_ERR_EMPTY; a NULL pointer -> GDSP_ERR_INVALID; n + m - 1 >
 * 2^20 -> GDSP_ERR_UNSUPPORTED; a_abs^-(n-1) outside the normal range ->
 * GDSP_ERR_INVALID. Runs on the current device. */
int gdsp_czt_batch(const void *x, int64_t ldx, int is_real, int64_t rows, int64_t n, int64_t m,
                   double a_abs, double a_turns, double step_turns, int64_t step_div, double *out,
                   int64_t ldo);

/* Additive cosine transforms of real rows (no reference equivalent;
 * scipy.fft.dct(x, type, n=N, norm=...), types II and III): for `rows` rows of
 * n float64, row r at x + r*ldx, and a transform length N (nfft; 0: n), row r
 * is cut to N samples or padded with zeros to N, and N float64 go to out +
 * r*ldo:
 *   type 2  y[k] = 2 sum_{j<N} x[j] cos(pi k (2j+1) / (2N))
 *   type 3  y[j] = x[0] + 2 sum_{1<=k<N} x[k] cos(pi k (2j+1) / (2N))
 *   GDSP_DCT_BACKWARD  as written
 *   GDSP_DCT_FORWARD   both types times 1 / (2N)
 *   GDSP_DCT_ORTHO     type 2: y[0] sqrt(1 / (4N)), y[k >= 1] sqrt(1 / (2N));
 *                      type 3: the backward type 3 of (sqrt(2) x[0], x[1], ...)
 *                      times sqrt(1 / (2N))
 * The inverse of (type 2, norm) is (type 3, the opposite norm) and the other
 * way round, where opposite swaps backward and forward and keeps ortho: the
 * callers' mapping, not another entry. One N-point transform per row (Makhoul):
 * v[j] = x[2j], v[N-1-j] = x[2j+1], w_k = exp(-i pi k / (2N)); type 2 is 2
 * Re(w_k FFT_N(v)[k]); type 3 the transform of (x[k] + i x[N-k]) w_k, its real
 * parts un-permuted. Where gdsp_dct_fused(N), one kernel per call: load,
 * permutation, transform, w_k, scale and store in one workgroup; otherwise the
 * composed form around the plan's transform in chunks of at most 2^24 samples
 * (N = 1 needs no transform). Longer host jobs are cut into ranges of rows of
 * at most 2^24 samples; a row's bits do not depend on the range or chunk it
 * falls in.
 * In this order, before any device call: a negative size, a type outside {2,
 * 3}, a norm outside 0..2, or, with rows > 1, ldx < min(n, N) or ldo < N ->
 * GDSP_ERR_INVALID; rows == 0 -> GDSP_OK, nothing done; n == 0 or N == 0 ->
 * GDSP_ERR_EMPTY; a NULL pointer -> GDSP_ERR_INVALID; N > 2^20 ->
 * GDSP_ERR_UNSUPPORTED. Runs on the current device. */
enum { GDSP_DCT_BACKWARD = 0, GDSP_DCT_ORTHO = 1, GDSP_DCT_FORWARD = 2 };
int gdsp_dct_batch(const double *x, int64_t ldx, int64_t rows, int64_t n, int64_t nfft,
                   int type, int norm, double *out, int64_t ldo);
/* 1 where the fused cosine-transform kernel serves transform length nfft under
 * the current flags (a power of 2 from 256 to 16384, without
 * GDSP_ALGO_NO_FUSED_DCT), 0 where the composed form runs or nothing does.
 * Host arithmetic only, no GPU needed. */
int gdsp_dct_fused(int64_t nfft);
/* float64 of d_work for `rows` rows under the current flags: 0 where
 * gdsp_dct_fused(nfft), for nfft <= 1, nfft > 2^20 or rows <= 0; otherwise
 * 3 * R * nfft, R = min(rows, max(1, 2^24 div nfft)): R rows of nfft
 * complex128, then R rows of nfft float64. Host arithmetic. */
int64_t gdsp_dct_work_doubles(int64_t rows, int64_t nfft);
/* The table w_k = exp(-i pi k / (2 nfft)), k < nfft, as the kernels read it:
 * re_im[2k] = cos(pi k / (2 nfft)), re_im[2k+1] = -sin(pi k / (2 nfft)),
 * evaluated in long double on angles of at most pi/4 (past nfft/2 through the
 * complement) and rounded once. Host only. nfft < 0 -> GDSP_ERR_INVALID; 0 ->
 * GDSP_ERR_EMPTY; a NULL pointer -> GDSP_ERR_INVALID; nfft > 2^20 ->
 * GDSP_ERR_UNSUPPORTED. */
int gdsp_dct_twiddles(int64_t nfft, double *re_im);

/* Additive batched entry point (no reference equivalent): the
 * same transform as fft.FFT / fft.IFFT applied to `batch` contiguous rows of n
 * complex128. inverse != 0 → IFFT semantics. */
int gdsp_fft_batch(const double *x, double *out, int64_t n, int64_t batch, int inverse);

/* Real-input batch (FFTReal per row): x is batch*n float64. */
int gdsp_fft_real_batch(const double *x, double *out, int64_t n, int64_t batch);

/* fft.FFT2 / fft.IFFT2 — fft/fft.go:109-121 → computeFFT2 :123-154. x is a
 * row-major rows×cols complex128 matrix (the Go shim flattens [][]complex128
 * after checking raggedness). rows == 0 → GDSP_ERR_EMPTY. */
int gdsp_fft2(const double *x, double *out, int64_t rows, int64_t cols, int inverse);

/* fft.FFT2Real / fft.IFFT2Real — fft/fft.go:104-107, :114-117. x: rows×cols
 * float64. */
int gdsp_fft2_real(const double *x, double *out, int64_t rows, int64_t cols, int inverse);

/* fft.FFTN / fft.IFFTN — fft/fft.go:157-192 (computeFFTN): the N-D DFT of a
 * row-major dsputils.Matrix (dsputils/matrix.go:21-57) with dims[0..ndims),
 * each >= 1 ("invalid dimensions" otherwise, GDSP_ERR_INVALID). x, out:
 * prod(dims) complex128. */
int gdsp_fftn(const double *x, double *out, const int64_t *dims, int ndims, int inverse);

/* fft.EnsureRadix2Factors — fft/radix2.go:35-37: pre-build (and cache) the
 * device plan for length n on the current device. Works for any n >= 2. */
int gdsp_ensure_plan(int64_t n);

/* fft.SetWorkerPoolSize — fft/fft.go:95-101. The GPU path has no worker
 * pool; the value is recorded (n < 0 → 0) and reported by
 * gdsp_worker_pool_size for API parity. */
void gdsp_set_worker_pool_size(int n);
int gdsp_worker_pool_size(void);

/* ---- spectral package ------------------------------------------------------ */

/* spectral.Segment — spectral/spectral.go:22-33: number of segments of length
 * `size` with `noverlap` overlap in a signal of length lx. Writes *count. */
int gdsp_segment_count(int64_t lx, int64_t size, int64_t noverlap, int64_t *count);

/* spectral.Pwelch — spectral/pwelch.go:74-145.
 * x: n float64 samples. nfft/pad/noverlap as PwelchOptions (0 = defaults:
 * nfft 256, pad nfft). Go's PwelchOptions.Window is a Go func, so the shim
 * passes its tables: win_seg = wf(max(pad, nfft)) — the window the reference
 * applies to each zero-padded segment (pwelch.go:108-109, window.go:25-29) —
 * and win_nfft = wf(nfft) for the normalisation (pwelch.go:124). NULL for
 * either selects window.Hann (the default, pwelch.go:89-91).
 * pxx, freqs: caller buffers of pad/2+1 float64; *lp_out receives the count
 * (0 for empty x, as the reference returns empty slices). */
int gdsp_pwelch(const double *x, int64_t n, double fs, int64_t nfft, int64_t pad,
                int64_t noverlap, const double *win_seg, const double *win_nfft,
                int scale_off, double *pxx, double *freqs, int64_t *lp_out);

/* Additive batched spectral.Pwelch (no reference equivalent): `channels`
 * signals of n float64 each, channel c at x + c*ldx (ldx >= n), one set of
 * options for all. Row c of pxx (channels × lp, lp = pad/2+1) is what
 * gdsp_pwelch defines for x + c*ldx: the same defaults, NULL windows = Hann, a
 * channel shorter than nfft zero-padded to nfft. freqs: lp float64, once.
 * n == 0 → *lp_out = 0, GDSP_OK; channels == 0 → GDSP_OK, only freqs and
 * *lp_out written. channels < 0, n < 0, ldx < n with channels > 1, or a needed
 * NULL pointer → GDSP_ERR_INVALID; a zero stride → GDSP_ERR_DIVIDE_BY_ZERO as
 * from gdsp_segment_count; all answered before any device call. Runs on the
 * current device (a batch is not split over the device set). F = max(pad,
 * nfft) a power of 2 from 64 to 2048 runs one fused kernel over all channels;
 * every other length loops over the channels inside the library, which is
 * one call but no faster than calling gdsp_pwelch per channel. */
int gdsp_pwelch_batch(const double *x, int64_t channels, int64_t n, int64_t ldx, double fs,
                      int64_t nfft, int64_t pad, int64_t noverlap, const double *win_seg,
                      const double *win_nfft, int scale_off, double *pxx, double *freqs,
                      int64_t *lp_out);
/* 1: a gdsp_pwelch_batch / gdsp_pwelch_batch_accumulate_device call of this
 * shape (0 = the defaults, as gdsp_pwelch) runs the batched kernel under the
 * current flags; 0: the loop over the channels (F < 64, F = 4096 and up,
 * non-powers of 2, strides above 2^22, GDSP_ALGO_NO_FUSED_PWELCH_BATCH). Host
 * arithmetic only (no GPU needed). */
int gdsp_pwelch_batch_fused(int64_t channels, int64_t n, int64_t nfft, int64_t pad,
                            int64_t noverlap);

/* Additive batched cross spectra (no reference equivalent; MATLAB cpsd /
 * mscohere, scipy.signal.csd / coherence): `channels` signals x (channel c at
 * x + c*ldx) each against y — y_rows == 1: one y (n float64) for all,
 * y_rows == channels: channel c at y + c*ldy. Options, defaults, the
 * zero-padding of a signal shorter than nfft, the segments, F = max(pad,
 * nfft), the windows (NULL = Hann), norm, freqs and lp = pad/2+1 are
 * gdsp_pwelch's. With X_s, Y_s the spectra gdsp_pwelch forms of segment s of
 * x and y, Sxx[j] = sum_s |X_s[j]|^2, Syy[j] = sum_s |Y_s[j]|^2, Sxy[j] =
 * sum_s conj(X_s[j]) Y_s[j] (MATLAB's and scipy's sign), and for j < lp
 *   P..[j] = c_j S..[j] / nsegs / norm, c_j = 2 for 0 < j < lp-1, else 1
 *   coh[j] = |Sxy[j]|^2 / (Sxx[j] Syy[j])
 * so pxx of (x, x) is gdsp_pwelch's. The coherence is the plain IEEE
 * quotient: a bin without power (and every bin when there is no segment)
 * gives NaN. Without segments every P is 0.
 * Accuracy: one transform carries a segment of x and the same segment of y
 * (z = w x_s + i a w y_s), so its roundoff is relative to the larger of the two.
 * a is a power of 2 chosen per segment from the binary exponents of
 * max |w x_s| and max |w y_s| and taken out of that segment's products again,
 * exactly: it evens out a difference in level between the two signals,
 * segment by segment, and depends on nothing but that segment. What is left is
 * a difference in level within one segment's spectra: a bin where one signal is
 * far below the other signal's largest bin carries roundoff relative to the
 * latter. a spans 2^-1022 ... 2^1022, every difference in level that two
 * normal doubles can have, so the balance itself gives up neither signal: the
 * products it forms have the size of one of the two signals' own spectra, and
 * a result leaves the normal range only where that signal's own sums do.
 * a = 1 where a segment's maximum is zero, subnormal or not finite (a
 * subnormal signal beside a normal one: its P, Pxy and the coherence are the
 * other's roundoff, not meaningful). A segment of one signal that is
 * all zeros contributes exact zeros to that signal's S and to Sxy (a dead
 * channel: P = Pxy = 0, the coherence 0 / 0), not the other signal's roundoff.
 * pxy: channels × lp complex128; pxx, pyy, coh: channels × lp float64, each
 * may be NULL (skipped); freqs: lp float64.
 * Before any device call: a NULL lp_out, x, y, pxy or freqs that is needed,
 * channels < 0, n < 0, nfft < 0, pad < 0, ldx < n with channels > 1 or ldy < n
 * with y_rows > 1 → GDSP_ERR_INVALID; y_rows neither 1 nor channels →
 * GDSP_ERR_UNEQUAL; a zero stride → GDSP_ERR_DIVIDE_BY_ZERO. n == 0 →
 * *lp_out = 0, GDSP_OK; channels == 0 → only freqs and *lp_out written.
 * F a power of 2 from 64 to 2048 runs one fused kernel over all channels
 * (gdsp_cpsd_batch_fused); every other length the materialised form. Runs on
 * the current device. */
int gdsp_cpsd_batch(const double *x, int64_t ldx, const double *y, int64_t ldy, int64_t y_rows,
                    int64_t channels, int64_t n, double fs, int64_t nfft, int64_t pad,
                    int64_t noverlap, const double *win_seg, const double *win_nfft,
                    int scale_off, double *pxy, double *pxx, double *pyy, double *coh,
                    double *freqs, int64_t *lp_out);
/* 1: a gdsp_cpsd_batch / gdsp_cpsd_batch_accumulate_device call of this shape
 * (0 = the defaults) runs the fused kernel under the current flags; 0: the
 * materialised form (F < 64, F = 4096 and up, non-powers of 2, strides above
 * 2^22, GDSP_ALGO_NO_FUSED_CPSD). Host arithmetic only (no GPU needed): no
 * plan is looked at. None needs to be: the library builds a power of 2 up to
 * 2^14 as the one-kernel plan the fused kernel takes its twiddles from under
 * every other flag. */
int gdsp_cpsd_batch_fused(int64_t channels, int64_t n, int64_t nfft, int64_t pad,
                          int64_t noverlap);

/* Additive per-segment spectra (no reference equivalent; MATLAB stft /
 * spectrogram, scipy.signal.stft / spectrogram): the quantity gdsp_pwelch
 * sums away. Options, defaults (nfft 0 = 256, pad 0 = nfft), the zero-padding
 * of a signal shorter than nfft, the segments (stride = nfft - noverlap),
 * F = max(pad, nfft), the window win_seg of F entries (NULL = Hann) and
 * lp = pad/2+1 are gdsp_pwelch's; with pad < nfft a row is the first lp bins
 * of the F-point transform, as there. With X_s the transform gdsp_pwelch
 * forms of segment s (windowed, zero-padded to F; spectral/pwelch.go:104-111):
 *   STFT         out[c][s][j] = X_s[j], complex128, unscaled
 *   spectrogram  out[c][s][j] = c_j |X_s[j]|^2 / norm, float64, c_j = 2 for
 *                0 < j < lp-1, else 1; norm = sum win_nfft^2 (times fs unless
 *                scale_off), in gdsp_pwelch_finalize's order (the square sum,
 *                the doubling, the division), so the mean of the rows over s
 *                is gdsp_pwelch's pxx
 * for channel c at x + c*ldx, s < nsegs = gdsp_segment_count(max(n, nfft),
 * nfft, noverlap), j < lp: out is channels × nsegs × lp, dense. freqs[j] =
 * j*fs/pad (lp float64), times[s] = (s*stride + nfft/2)/fs (nsegs float64:
 * the segment's centre, scipy.signal.spectrogram's convention).
 * The imaginary parts of bins 0 and F/2 are exact zeros.
 * Accuracy: the fused kernel packs two segments into one transform (z = w x_s
 * + i a w x_(s+1)), whose roundoff is relative to the larger of the two. a is
 * a power of 2 from the binary exponents of the two segments' maxima, taken
 * out of segment s+1's row again, exactly (the balance of gdsp_cpsd_batch,
 * its range and its exceptions): a quiet segment beside a loud one keeps its
 * digits in its own row. A segment of all zeros gives a row of exact zeros. A
 * NaN or an infinity makes non-finite the rows of the segments that contain
 * it and changes no other row by a bit: a group of pairs that holds one runs
 * its even and its odd segments in transforms of their own. Inputs times 2^k
 * give STFT rows times 2^k and spectrogram rows times 2^2k bit for bit.
 * Before any device call: a NULL nsegs_out or lp_out, or a needed NULL x, out,
 * freqs or times, channels < 0, n < 0, nfft < 0, pad < 0, ldx < n with
 * channels > 1 → GDSP_ERR_INVALID; a zero stride → GDSP_ERR_DIVIDE_BY_ZERO
 * as from gdsp_segment_count. n == 0 → *nsegs_out = *lp_out = 0, GDSP_OK;
 * channels == 0 → only freqs, times and the counts are written. The device
 * output is held to 2^25 elements (512 MiB of complex128): longer results
 * run as ranges of segments that begin at even indices, so no bit of a row
 * depends on where a range was cut. F a power of 2 from 64 to 2048 runs one
 * fused kernel over all channels (gdsp_stft_batch_fused); every other length
 * the materialised form. Runs on the current device. */
int gdsp_stft_batch(const double *x, int64_t channels, int64_t n, int64_t ldx, int64_t nfft,
                    int64_t pad, int64_t noverlap, const double *win_seg, double *out,
                    int64_t *nsegs_out, int64_t *lp_out);
int gdsp_spectrogram_batch(const double *x, int64_t channels, int64_t n, int64_t ldx, double fs,
                           int64_t nfft, int64_t pad, int64_t noverlap, const double *win_seg,
                           const double *win_nfft, int scale_off, double *out, double *freqs,
                           double *times, int64_t *nsegs_out, int64_t *lp_out);
/* 1: a call of gdsp_stft_batch, gdsp_spectrogram_batch or their device
 * entries of this shape (0 = the defaults) runs the fused kernel under the
 * current flags; 0: the materialised form (F < 64, F = 4096 and up,
 * non-powers of 2, strides above 2^22, GDSP_ALGO_NO_FUSED_STFT). Host
 * arithmetic only (no GPU needed), as gdsp_cpsd_batch_fused. */
int gdsp_stft_batch_fused(int64_t channels, int64_t n, int64_t nfft, int64_t pad,
                          int64_t noverlap);

/* The inverse of gdsp_stft_batch by weighted overlap-add (no reference
 * equivalent; MATLAB istft, scipy.signal.istft: the least-squares inverse of
 * Griffin and Lim). Options, defaults, F = max(pad, nfft), stride = nfft -
 * noverlap, lp = pad/2+1 and the window w = win_seg[0 .. nfft) (the first nfft
 * entries of the window of F, NULL = Hann) are gdsp_stft_batch's; pad >= nfft
 * after the defaults is required (a row with pad < nfft is a truncated
 * spectrum and has no inverse). X is channels x nsegs x lp complex128, dense.
 * For channel c with rows X_s:
 *   y_s    = the first nfft samples of the F-point inverse real transform of
 *            X_s (Hermitian completion of the lp bins, 1/F included; the
 *            imaginary parts of bins 0 and, F even, F/2 are not read)
 *   num[i] = sum_s w[i - s*stride] y_s[i - s*stride]   over the segments that
 *   D[i]   = sum_s w[i - s*stride]^2                   cover i, ascending s
 *   out[c*ldo + i] = num[i] / D[i] where D[i] > 0, exactly 0 where D[i] == 0
 * for i < n_full = (nsegs-1)*stride + nfft. D == 0 is an exact test, not a
 * threshold: on rows from gdsp_stft_batch the result is the signal wherever
 * D > 0, for any window and overlap (no COLA condition). n == 0 means n_full;
 * *n_out = the samples written per row.
 * Accuracy: the fused kernel packs rows (2p, 2p+1), by absolute index, into
 * one inverse transform, balanced by a power of 2 from the binary exponents
 * of the two rows' maxima and taken out again exactly (gdsp_stft_batch): a
 * quiet row beside a loud one keeps its digits, a row of zeros contributes
 * exact zeros, and a pair that holds a NaN or an infinity runs its two rows in
 * transforms of their own, so a row's samples depend on its pair alone.
 * Before any device call: a NULL n_out or a needed NULL X or out, negative
 * counts, nfft < 0, pad < nfft after the defaults, n > n_full, ldo < n with
 * channels > 1 -> GDSP_ERR_INVALID; a zero stride with nsegs > 1 ->
 * GDSP_ERR_DIVIDE_BY_ZERO. channels == 0 or nsegs == 0: nothing is written
 * (*n_out = 0 for nsegs == 0). The device copy of X is held to 2^25 complex
 * elements: longer inputs run as output ranges that begin at multiples of
 * 2*stride, each with the rows that reach into it, so no bit depends on the
 * cut. F a power of 2 from 64 to 2048 with 0 <= noverlap and nfft <= 4*stride
 * runs one fused kernel (gdsp_istft_batch_fused); every other shape the
 * materialised form. Runs on the current device. */
int gdsp_istft_batch(const void *X, int64_t channels, int64_t nsegs, int64_t nfft, int64_t pad,
                     int64_t noverlap, const double *win_seg, int64_t n, double *out, int64_t ldo,
                     int64_t *n_out);
/* 1: a call of gdsp_istft_batch or its device entry of this shape (0 = the
 * defaults) runs the fused kernel under the current flags; 0: the materialised
 * form (F < 64, F = 4096 and up, non-powers of 2, pad < nfft, more than 4
 * segments over a sample, a negative noverlap, GDSP_ALGO_NO_FUSED_ISTFT). Host
 * arithmetic only (no GPU needed). */
int gdsp_istft_batch_fused(int64_t channels, int64_t nsegs, int64_t nfft, int64_t pad,
                           int64_t noverlap);

/* window.Hann — window/window.go:62-76, as a host table generator used by the
 * shim for the default window (L float64 written to out). */
int gdsp_window_hann(int64_t L, double *out);

/* ---- wav package (the wav -> Pwelch feeder) -------------------------------- */

/* wav.(*Wav).ReadFloats — wav/wav.go:135-161 — on the GPU: converts `count`
 * little-endian samples of a WAV data chunk (what ReadSamples reads,
 * wav.go:110-131) with the reference's float32 formulas. audio_format 1 with
 * bits_per_sample 8 or 16 (PCM) or 3 (IEEE float32); anything else →
 * GDSP_ERR_UNSUPPORTED ("wav: unknown bits per sample" / "unknown audio
 * format" in the reference). out_f64 = 0 writes float32 (the reference's
 * []float32), 1 writes float64 (the float32 values widened: a Pwelch input).
 * Host-pointer form: in/out on the host, synchronous. */
int gdsp_wav_read_floats(const void *in, int64_t count, int audio_format, int bits_per_sample,
                         void *out, int out_f64);

/* ---- multi-device (one node's GPUs inside one call) ------------------------- */
/* The reference keeps its parallelism inside the call (radix2FFT's goroutine
 * pool, fft/radix2.go:89-151; Pwelch's one accumulation loop,
 * spectral/pwelch.go:107-122). These keep that across GPUs: a batched FFT
 * splits its rows into contiguous shards, one per device, with no
 * collective; Pwelch splits its segments (each device reads its samples plus
 * the nfft - stride halo) and combines the per-device accumulators with one
 * in-process RCCL reduce (sum, float64) before the host finalises Pxx. Each
 * multi-device call runs whole (accumulate, reduce, copy back) before the
 * next one from any host thread starts. */

/* Library-wide device set. When it has been configured (here, or by
 * GDSP_DEVICES="0,1,2,3" / "all" at first use) with more than one entry,
 * gdsp_fft_batch, gdsp_fft_real_batch and gdsp_pwelch split calls whose input
 * is at least GDSP_MULTI_MIN_BYTES (64 MiB by default) and has at least 2
 * rows / segments over it. Unconfigured (the default, or ndev = 0 here) the
 * set is the calling thread's current device, so no call leaves it. A device
 * may be listed more than once: its shards run side by side on separate
 * streams (a Pwelch over such a set, or without a loadable librccl, sums the
 * per-device accumulators on the host instead of by RCCL). Devices must be
 * visible. */
int gdsp_set_devices(const int *devices, int ndev);
/* The current device set: writes up to cap ids, returns the set's size (0
 * without a GPU). */
int gdsp_get_devices(int *devices, int cap);
/* Multi-device calls since process start (diagnostics and tests): batched
 * FFT calls and Pwelch calls split over a device set, and how the Pwelch
 * accumulators were combined (RCCL reduce / host sum). Any pointer may be
 * NULL. */
int gdsp_multi_stats(int64_t *batch_calls, int64_t *pwelch_calls, int64_t *rccl_reduces,
                     int64_t *host_reduces);
/* How calls were cut into pieces since process start (diagnostics and tests;
 * host-side counters, no kernel takes part). later_chunks: second and later
 * iterations of the host loops that cut one call into several launches (the
 * materialised Pwelch's pair chunks and Cpsd's channel and segment runs, the
 * channels-per-launch loops of the fused batched Pwelch and Cpsd, the channel
 * loop of the batched Pwelch where it has no fused kernel, the segment ranges
 * of gdsp_stft_batch / gdsp_spectrogram_batch and the channel and segment runs
 * of their materialised form, the output ranges of gdsp_istft_batch and the
 * channel and segment runs of its materialised form, the composed FIR's
 * transform chunks, the output ranges of gdsp_upfirdn_batch, the row ranges
 * of gdsp_hilbert_batch and the row chunks of its composed form, the time
 * chunks of gdsp_sosfilt_batch and of both passes of gdsp_sosfiltfilt_batch,
 * the row ranges of gdsp_czt_batch and the row chunks of its composed form,
 * the row ranges of gdsp_dct_batch and the row chunks of its composed form,
 * and the 65535-row pieces of gdsp_fft_axis_device / gdsp_fftn_device and of the
 * multi-pass, four-step and chirp-z executors).
 * multi_unit_launches: launches of a Pwelch, batched-Pwelch, Cpsd, STFT or ISTFT kernel
 * whose persistent workers each take at least two pairs (or pair groups). A
 * test reads both before and after a call to prove that the call reached the
 * path it was shaped for. Any pointer may be NULL. */
int gdsp_loop_stats(int64_t *later_chunks, int64_t *multi_unit_launches);

/* fft.FFT / fft.IFFT over `batch` rows of n complex128 (as gdsp_fft_batch),
 * always split over `devices` (NULL or ndev = 0: the library's device set);
 * at most `batch` devices take part. Host pointers, synchronous. */
int gdsp_fft_batch_multi(const double *x, double *out, int64_t n, int64_t batch, int inverse,
                         const int *devices, int ndev);

/* spectral.Pwelch (as gdsp_pwelch), always split over `devices` (NULL or
 * ndev = 0: the library's device set) with the RCCL reduce of the per-bin
 * accumulators — also for a single device (host sum for a set that repeats
 * a device). Thread-safe: the accumulators are owned by the call. */
int gdsp_pwelch_multi(const double *x, int64_t n, double fs, int64_t nfft, int64_t pad,
                      int64_t noverlap, const double *win_seg, const double *win_nfft,
                      int scale_off, double *pxx, double *freqs, int64_t *lp_out,
                      const int *devices, int ndev);

/* Shard i of ndev, as the calls above split the work: rows [*lo, *hi) of a
 * batch; and for Pwelch, segments [*seg_lo, *seg_hi) of nsegs and the
 * samples [*x_lo, *x_hi) they read (empty when the shard has no segment).
 * Host arithmetic only (no GPU needed). */
int gdsp_batch_shard(int64_t batch, int ndev, int i, int64_t *lo, int64_t *hi);
int gdsp_pwelch_shard(int64_t nsegs, int64_t nfft, int64_t noverlap, int ndev, int i,
                      int64_t *seg_lo, int64_t *seg_hi, int64_t *x_lo, int64_t *x_hi);

/* ---- device-pointer API (stream-ordered; multi-GPU building blocks) ---------- */

typedef struct gdsp_plan gdsp_plan;

/* Create / fetch the cached plan for transform length n on the current
 * device. Plans are owned by the library cache; destroy is a no-op for cached
 * plans and exists for API symmetry. */
int gdsp_plan_create(int64_t n, gdsp_plan **plan);
int gdsp_plan_destroy(gdsp_plan *plan);
/* The same transform as fft.FFT for non-power-of-2 n, always computed with
 * Bluestein's chirp-z (fft/bluestein.go:68-94) — the reference's algorithm —
 * even where the default plan uses the mixed-radix kernel. n >= 2. Cached
 * separately from gdsp_plan_create's plans. */
int gdsp_plan_create_chirpz(int64_t n, gdsp_plan **plan);
/* Which algorithm a plan runs: 0 trivial (n<=1), 1 one-kernel LDS Stockham,
 * 2 multi-pass global Stockham (large power of 2), 3 fused Bluestein,
 * 4 composed Bluestein (M > 16384), 5 one-kernel mixed radix (non-power-of-2
 * n <= 4096 whose prime factors are all <= 13), 6 mixed four-step (such n
 * above 8192 = n1*n2 with one-kernel factors: transposes + row kernels),
 * 7 Rader (a prime 17 <= n <= 8193 whose n - 1 has a list of radices <= 25
 * within 640 threads per transform: the DFT as
 * a cyclic convolution of length n - 1, two FFTs of n - 1 points in one
 * runtime-compiled kernel; GDSP_ALGO_NO_RADER keeps such primes on kind 3),
 * 8 prime-factor Rader (a composite n <= 8192 = n1 * n2, n2 > 31 its largest
 * prime factor with a kind-7 plan, gcd(n1, n2) = 1, n1 with an in-register
 * DFT: the Good-Thomas map, DFT_n1 per column and n1 Rader transforms of n2
 * points, one runtime-compiled kernel; GDSP_ALGO_NO_RADER keeps kind 3). */
int gdsp_plan_kind(const gdsp_plan *plan);
/* Geometry of a plan (any pointer may be NULL): its length n; the chirp-z
 * convolution length m (kinds 3 and 4; the reference's NextPowerOf2(2n-1),
 * bluestein.go:70, or a smooth m >= 2n-1 that the composed chirp-z may
 * choose; kind 7: Rader's cyclic convolution length n - 1; kind 8: n2 - 1);
 * the four-step split n = n1*n2 (kinds 2 and 6) or the prime-factor split
 * (kind 8: cofactor n1, prime n2); and whether a
 * runtime-compiled specialisation backs it (1) or not (0). 0 where n/a. */
int gdsp_plan_info(const gdsp_plan *plan, int64_t *n, int64_t *m, int64_t *n1, int64_t *n2,
                   int *runtime_compiled);
/* The radix list of a plan's mixed-radix passes: kind 5 its transform's,
 * kind 7 the cyclic convolution's (n - 1), kind 8 the prime factor's
 * convolution (n2 - 1), and a kind-3 plan on the smooth-L chirp-z kernel
 * the list of its convolution length (the m of gdsp_plan_info). Writes
 * min(count, cap) radices and returns the count; 0 for the other plans. */
int gdsp_plan_radices(const gdsp_plan *plan, int *rad, int cap);
/* Output parts of a kind-3 plan: 1 for the one-convolution chirp-z of
 * bluestein.go:68-94; P > 1 when n in (8192, 14563] (NextPowerOf2(2n-1) =
 * 32768, beyond one kernel) runs as P fused convolutions of M = 16384, each
 * giving ceil(n/P) of the outputs (GDSP_ALGO_NO_CHIRPZ_PARTS: the composed
 * chirp-z instead). */
int gdsp_plan_parts(const gdsp_plan *plan);

/* Batched C2C on device buffers: d_in/d_out hold batch*n complex128 (may
 * alias only if equal). inverse != 0 → IFFT semantics (1/n scaling). */
int gdsp_fft_batch_device(const gdsp_plan *plan, const void *d_in, void *d_out,
                          int64_t batch, int inverse, void *stream);

/* fft.FFTReal / fft.IFFTReal — fft/fft.go:25-32 — over `batch` device rows:
 * d_in holds batch*n float64 (read as they are: no ToComplex copy), d_out
 * batch*n complex128 and must not overlap d_in. inverse != 0 → IFFTReal
 * semantics (an empty plan is then GDSP_ERR_EMPTY, like IFFT). */
int gdsp_fft_real_batch_device(const gdsp_plan *plan, const double *d_in, void *d_out,
                               int64_t batch, int inverse, void *stream);

/* gdsp_convolve_batch on device buffers, rows of plan's length n: d_x and
 * d_out hold batch*n complex128 (d_out may alias d_x), d_y y_rows*n (y_rows 1
 * or batch). d_work: scratch of y_rows*n complex128 for the spectrum of y,
 * distinct from d_out (may be NULL: the library allocates); with d_work given
 * the call neither allocates nor synchronises where the plan's transform
 * does not. Power-of-2 n from 256 to 16384 run one fused kernel per call after
 * the spectrum of y (load, FFT, times FFT(y)/n, second FFT, store: one read
 * and one write of the rows); every other length FFT, row multiply, IFFT.
 * Status codes as gdsp_convolve_batch, n == 0 included; a NULL plan →
 * GDSP_ERR_INVALID. */
int gdsp_convolve_batch_device(const gdsp_plan *plan, const void *d_x, const void *d_y,
                               int64_t y_rows, void *d_out, int64_t batch,
                               void *d_work, void *stream);
/* 1: the fused kernel serves this plan under the current flags; 0: composed */
int gdsp_convolve_fused(const gdsp_plan *plan);

/* gdsp_fir_batch on device buffers (no reference equivalent), stream-ordered:
 * d_x rows of n float64 at stride ldx, d_h h_rows*m float64, d_out rows of
 * the output length at stride ldo. The address ranges of d_x and d_out must
 * not overlap (a block reads a halo that another workgroup writes):
 * GDSP_ERR_INVALID. d_work: scratch (may be NULL: the library's workspace
 * pool) of 16*F*h_rows bytes for the taps' spectra, and in the composed form
 * 16*F*min(T, max(1, 2^24 / F)) more, T = channels * ceil(ceil(output length /
 * (F - m + 1)) / 2) transforms. Status codes as gdsp_fir_batch, decided
 * before any device call. */
int gdsp_fir_batch_device(const void *d_x, int64_t ldx, const void *d_h, int64_t h_rows,
                          int64_t m, int64_t channels, int64_t n, int full, int64_t block,
                          void *d_out, int64_t ldo, void *d_work, void *stream);

/* gdsp_upfirdn_batch on device buffers (no reference equivalent),
 * stream-ordered: d_x rows of n float64 at stride ldx, d_h m float64, d_out
 * rows of out_end - out_begin float64 at stride ldo (output out_begin of row
 * c at d_out + c*ldo). The address ranges of d_x and d_out must not overlap
 * (a tile reads a halo that another workgroup's outputs would overwrite):
 * GDSP_ERR_INVALID. d_work: scratch of up * ceil(m / up) doubles for the
 * phase-major taps (may be NULL: the library's workspace pool); with d_work
 * given the call neither allocates nor synchronises. Status codes as
 * gdsp_upfirdn_batch, decided before any device call. */
int gdsp_upfirdn_batch_device(const void *d_x, int64_t ldx, const void *d_h, int64_t m,
                              int64_t up, int64_t down, int64_t channels, int64_t n,
                              int64_t out_begin, int64_t out_end, void *d_out, int64_t ldo,
                              void *d_work, void *stream);

/* gdsp_hilbert_batch on device buffers (no reference equivalent),
 * stream-ordered: d_x rows of n float64 at stride ldx (doubles), d_out rows of
 * N output elements at stride ldo (output elements: complex128 for
 * GDSP_HILBERT_ANALYTIC, float64 otherwise). The address ranges of d_x and
 * d_out must not overlap (the kinds that store the input read it again while
 * other workgroups store): GDSP_ERR_INVALID, decided after gdsp_hilbert_batch's
 * own checks. d_work (may be NULL: the library's workspace pool): nothing
 * where gdsp_hilbert_fused(N) (the fused call then neither allocates nor
 * synchronises); otherwise R * N * 24 bytes, R = min(rows, max(1, 2^24 div
 * N)): R rows of N complex128, then R rows of N float64, 16-byte aligned. */
/* gdsp_sosfilt_batch and gdsp_sosfiltfilt_batch on device buffers (no
 * reference equivalent), stream-ordered; sos is a host pointer (the tables are
 * host arithmetic and reach the device as kernel arguments), d_zi and d_zf
 * device pointers or NULL. d_out may be exactly d_x (same pointer and row
 * stride) in gdsp_sosfilt_batch_device: pass 3 reads a tile before it stores
 * it; any other overlap, and every overlap in gdsp_sosfiltfilt_batch_device ->
 * GDSP_ERR_INVALID, decided after the host entry's checks. d_work (NULL: the
 * library's workspace): gdsp_sosfilt_work_doubles or
 * gdsp_sosfiltfilt_work_doubles float64 (the latter holds the forward pass's
 * result, n + 2 padlen doubles per row); with it a call neither allocates nor
 * synchronises. No row is cut: a call is bit-equal to the host entry's. */
int gdsp_sosfilt_batch_device(const void *d_x, int64_t ldx, const double *sos, int64_t S,
                              const void *d_zi, int64_t channels, int64_t n, void *d_out,
                              int64_t ldo, void *d_zf, void *d_work, void *stream);
int gdsp_sosfiltfilt_batch_device(const void *d_x, int64_t ldx, const double *sos, int64_t S,
                                  int64_t padlen, int64_t channels, int64_t n, void *d_out,
                                  int64_t ldo, void *d_work, void *stream);

int gdsp_hilbert_batch_device(const void *d_x, int64_t ldx, int64_t rows, int64_t n,
                              int64_t nfft, int kind, void *d_out, int64_t ldo,
                              void *d_work, void *stream);

/* gdsp_dct_batch on device buffers (no reference equivalent), stream-ordered:
 * d_x rows of n float64 at stride ldx, d_out rows of N float64 at stride ldo.
 * d_out may be exactly d_x (the same pointer, ldo == ldx, N <= n): a workgroup,
 * or the gather of a chunk, has read a whole row before any of it is stored.
 * Every other overlap of the address ranges -> GDSP_ERR_INVALID, decided after
 * gdsp_dct_batch's own checks. d_work (may be NULL: the library's workspace
 * pool): gdsp_dct_work_doubles(rows, N) float64, 16-byte aligned. With d_work
 * given, or where gdsp_dct_fused(N), a call neither allocates nor synchronises
 * once the plan and the w_k table of N exist on the device (the first call for
 * an N builds them). */
int gdsp_dct_batch_device(const void *d_x, int64_t ldx, int64_t rows, int64_t n, int64_t nfft,
                          int type, int norm, void *d_out, int64_t ldo, void *d_work,
                          void *stream);

/* The chirp-z transform's plan (gdsp_czt_batch's parameters, no reference
 * equivalent): the device tables A, FFT_F(v) / F (computed from the float64 v
 * by the engine's own transform) and P on the caller's current device, and the
 * plan cache's F-point transform. In this order: a NULL plan pointer, a
 * negative size, a_abs <= 0, a parameter that is not finite or step_div < 1 ->
 * GDSP_ERR_INVALID; n == 0 or m == 0 -> GDSP_ERR_EMPTY; n + m - 1 > 2^20 ->
 * GDSP_ERR_UNSUPPORTED; a_abs^-(n-1) outside the normal double range ->
 * GDSP_ERR_INVALID; then the device. A plan may be used by any number of
 * calls and streams of its device; gdsp_czt_plan_destroy waits for the device
 * and frees the tables (NULL: nothing). gdsp_czt_plan_info: n, m, F and
 * whether a call made now runs the fused kernel (any pointer may be NULL). */
typedef struct gdsp_czt_plan gdsp_czt_plan;
int gdsp_czt_plan_create(int64_t n, int64_t m, double a_abs, double a_turns, double step_turns,
                         int64_t step_div, gdsp_czt_plan **plan);
int gdsp_czt_plan_destroy(gdsp_czt_plan *plan);
int gdsp_czt_plan_info(const gdsp_czt_plan *plan, int64_t *n, int64_t *m, int64_t *F,
                       int *fused);
/* Bytes of d_work for `rows` rows under the current flags: 0 in the fused
 * form, else min(rows, max(1, 2^24 div F)) * F * 16. Host arithmetic. */
int64_t gdsp_czt_work_bytes(const gdsp_czt_plan *plan, int64_t rows);
/* gdsp_czt_batch on device buffers, stream-ordered: d_x rows of n float64
 * (is_real = 1) or complex128 (0) at stride ldx elements, d_out rows of m
 * complex128 at stride ldo. In this order: a NULL plan, a negative rows,
 * is_real outside 0..1, with rows > 1 ldx < n or ldo < m -> GDSP_ERR_INVALID;
 * rows == 0 -> GDSP_OK; a NULL d_x or d_out -> GDSP_ERR_INVALID; overlapping
 * address ranges of d_x and d_out, or a d_work of fewer than
 * gdsp_czt_work_bytes(plan, rows) bytes (work_bytes) -> GDSP_ERR_INVALID.
 * d_work may be NULL (the library's workspace pool); the fused form takes
 * none, and with d_work given a call neither allocates nor synchronises. */
int gdsp_czt_batch_device(const gdsp_czt_plan *plan, const void *d_x, int64_t ldx, int is_real,
                          int64_t rows, void *d_out, int64_t ldo, void *d_work,
                          int64_t work_bytes, void *stream);

/* FFT2/IFFT2 on a device rows×cols complex128 matrix. d_work: scratch of
 * rows*cols complex128 (may be NULL: the library allocates stream-ordered). */
int gdsp_fft2_device(const void *d_in, void *d_out, int64_t rows, int64_t cols,
                     int inverse, void *d_work, void *stream);

/* FFTN/IFFTN on a device array (dims on the host). */
int gdsp_fftn_device(const void *d_in, void *d_out, const int64_t *dims, int ndims, int inverse,
                     void *stream);

/* One axis of FFTN: the 1-D FFT/IFFT along dimension `axis` of a device
 * row-major array (the per-dimension loop of computeFFTN, fft/fft.go:172-185;
 * axis 0 of a rows x cols matrix is computeFFT2's column pass, :138-147).
 * The building block of the multi-GPU FFT2 (row FFTs, all-to-all, column
 * FFTs on a column block). */
int gdsp_fft_axis_device(const void *d_in, void *d_out, const int64_t *dims, int ndims,
                         int axis, int inverse, void *stream);

/* Pwelch partial accumulation over segments [seg_begin, seg_end) of a device
 * signal d_x (n float64, sample 0 = sample 0 of segment 0). Adds into
 * d_acc[0..flen) (flen = max(pad, nfft)) the per-bin sums S_k of |Z_k|² over
 * the packed segment pairs; gdsp_pwelch_finalize turns the summed
 * accumulators (over every shard / rank) into Pxx. d_win_seg: flen float64
 * window table on the device. d_acc must be zeroed by the caller before the
 * first call. Every segment of the range must lie inside the n samples:
 * (seg_end - 1) * (nfft - noverlap) + nfft > n → GDSP_ERR_INVALID for any
 * non-empty range, [0, 1) of a signal shorter than nfft included (the kernels
 * read whole segments: pad such a signal to nfft first, as gdsp_pwelch does);
 * nothing is read or written then. An empty range is GDSP_OK and touches
 * nothing. */
int gdsp_pwelch_accumulate_device(const double *d_x, int64_t n, int64_t nfft, int64_t pad,
                                  int64_t noverlap, int64_t seg_begin, int64_t seg_end,
                                  const double *d_win_seg, double *d_acc, void *stream);

/* Host finalisation (spectral/pwelch.go:113-142): from the summed
 * accumulators acc[0..flen) over all nsegs segments produce
 * pxx[j] = c_j * (acc[j] + acc[(flen-j)%flen]) / 2 / nsegs / norm and
 * freqs[j] = j*fs/pad for j < pad/2+1. */
int gdsp_pwelch_finalize(const double *acc, int64_t flen, int64_t nsegs, int64_t nfft,
                         int64_t pad, const double *win_nfft, double fs, int scale_off,
                         double *pxx, double *freqs);

/* gdsp_pwelch_accumulate_device over the channels of a planar device batch:
 * channel c is n float64 at d_x + c*ldx (ldx >= n, any value: odd ones too),
 * and its sums are added into d_acc + c*flen (channels × flen, zeroed by the
 * caller before the first call). The same segments [seg_begin, seg_end) of
 * every channel; geometry checks as gdsp_pwelch_accumulate_device, plus
 * channels < 0, n < 0 or ldx < n with channels > 1 → GDSP_ERR_INVALID.
 * Lengths and fallback as gdsp_pwelch_batch (gdsp_pwelch_batch_fused). */
int gdsp_pwelch_batch_accumulate_device(const double *d_x, int64_t channels, int64_t n,
                                        int64_t ldx, int64_t nfft, int64_t pad, int64_t noverlap,
                                        int64_t seg_begin, int64_t seg_end,
                                        const double *d_win_seg, double *d_acc, void *stream);

/* gdsp_pwelch_finalize on the device, per channel: d_acc channels × flen
 * summed accumulators → d_pxx channels × (pad/2+1), the host function's
 * operations in its order (bit-identical results). win_nfft: host table of
 * nfft (NULL = Hann); freqs: host buffer of pad/2+1 (may be NULL). Stream-
 * ordered; the PSDs never leave the device. */
int gdsp_pwelch_batch_finalize_device(const double *d_acc, int64_t channels, int64_t flen,
                                      int64_t nsegs, int64_t nfft, int64_t pad,
                                      const double *win_nfft, double fs, int scale_off,
                                      double *d_pxx, double *freqs, void *stream);

/* The cross-spectral sums of gdsp_cpsd_batch on device buffers: adds the
 * sums over segments [seg_begin, seg_end) of every channel into d_acc,
 * channels × 4 × hb float64 (hb = max(pad, nfft)/2 + 1; planes Sxx, Syy,
 * Re Sxy, Im Sxy), zeroed by the caller before the first call. These are the
 * true sums of the range (no pairing term is left in them, unlike the Pwelch
 * accumulators), so ranges add in any split, and no segment's arithmetic
 * depends on where a range begins (the balance of gdsp_cpsd_batch is per
 * segment). d_x channel c at d_x + c*ldx,
 * d_y at d_y + (y_rows == 1 ? 0 : c)*ldy; d_win_seg: the window of max(pad,
 * nfft) on the device. nfft <= 0, pad <= 0, a negative or reversed range,
 * channels < 0, n < 0, ldx < n with channels > 1, ldy < n with y_rows > 1, a
 * needed NULL pointer, or seg_end past the signal → GDSP_ERR_INVALID; y_rows
 * neither 1 nor channels → GDSP_ERR_UNEQUAL; nfft == noverlap with seg_end > 1
 * → GDSP_ERR_DIVIDE_BY_ZERO; all before any device call. */
int gdsp_cpsd_batch_accumulate_device(const double *d_x, int64_t ldx, const double *d_y,
                                      int64_t ldy, int64_t y_rows, int64_t channels, int64_t n,
                                      int64_t nfft, int64_t pad, int64_t noverlap,
                                      int64_t seg_begin, int64_t seg_end,
                                      const double *d_win_seg, double *d_acc, void *stream);

/* Finalisation of d_acc (channels × 4 × (flen/2+1)) on the device into any of
 * d_pxy (channels × lp complex128), d_pxx, d_pyy, d_coh (channels × lp
 * float64), lp = pad/2+1; a NULL output is skipped. Every P by
 * gdsp_pwelch_finalize's operations in its order. win_nfft: host table of
 * nfft (NULL = Hann); freqs: host buffer of lp (may be NULL). */
int gdsp_cpsd_batch_finalize_device(const double *d_acc, int64_t channels, int64_t flen,
                                    int64_t nsegs, int64_t nfft, int64_t pad,
                                    const double *win_nfft, double fs, int scale_off,
                                    void *d_pxy, double *d_pxx, double *d_pyy, double *d_coh,
                                    double *freqs, void *stream);

/* gdsp_stft_batch on device buffers: the rows of segments [seg_begin,
 * seg_end) of every channel (channel c: n float64 at d_x + c*ldx) into d_out,
 * complex128; row (c, s) at element c*ld_chan + (s - seg_begin)*ld_seg, its
 * lp = pad/2+1 bins contiguous. The strides are the caller's, in elements of
 * the output type: ld_seg >= lp and, with channels > 1, ld_chan >= (seg_end -
 * seg_begin)*ld_seg; nothing between the rows is written. d_win_seg: the
 * window of max(pad, nfft) on the device. A range that begins at an odd
 * segment pairs the segments differently in the fused kernel, so its rows
 * agree with the whole call's to roundoff, not bit for bit; a range that
 * begins at an even one gives the same bits. nfft <= 0, pad <= 0, a negative
 * or reversed range, channels < 0, n < 0, ldx < n with channels > 1, ld_seg <
 * lp, ld_chan too small, a needed NULL pointer, or seg_end past the signal →
 * GDSP_ERR_INVALID; nfft == noverlap with seg_end > 1 →
 * GDSP_ERR_DIVIDE_BY_ZERO; all before any device call. channels == 0 or an
 * empty range: nothing is written, GDSP_OK. */
int gdsp_stft_batch_device(const double *d_x, int64_t ldx, int64_t channels, int64_t n,
                           int64_t nfft, int64_t pad, int64_t noverlap, int64_t seg_begin,
                           int64_t seg_end, const double *d_win_seg, void *d_out, int64_t ld_seg,
                           int64_t ld_chan, void *stream);
/* The same for gdsp_spectrogram_batch: float64 rows c_j |X_s[j]|^2 / norm;
 * norm as gdsp_spectrogram_batch forms it (1: the raw c_j |X|^2), the
 * divisor as it is given. */
int gdsp_spectrogram_batch_device(const double *d_x, int64_t ldx, int64_t channels, int64_t n,
                                  int64_t nfft, int64_t pad, int64_t noverlap, int64_t seg_begin,
                                  int64_t seg_end, const double *d_win_seg, double norm,
                                  double *d_out, int64_t ld_seg, int64_t ld_chan, void *stream);

/* gdsp_istft_batch on device buffers: samples [out_begin, out_end) of every
 * channel, out_end <= n_full, into d_out[c*ldo + (i - out_begin)]. d_X holds
 * rows seg_row0 ... seg_row0 + seg_rows - 1 of every channel: row (c, s) at
 * element c*ld_chan + (s - seg_row0)*ld_seg, its lp complex128 contiguous. The
 * rows of every segment that covers a sample of the range must be present,
 * and for the shapes gdsp_istft_batch_fused serves the partner of each such
 * row in its pair (2p, 2p+1) too, where nsegs has one: the fused kernel
 * transforms a pair together and a row's bits depend on its partner. Other
 * rows are not read. Any range then gives the bits of the whole call; a range
 * that no segment covers (a negative noverlap leaves gaps) is zeros. A
 * needed NULL pointer, negative counts, nfft <= 0, pad < nfft, ld_seg < lp,
 * ld_chan < seg_rows*ld_seg or ldo < out_end - out_begin with channels > 1, a
 * reversed range, out_end > n_full, seg_row0 + seg_rows > nsegs or a missing
 * row -> GDSP_ERR_INVALID; a zero stride with nsegs > 1 ->
 * GDSP_ERR_DIVIDE_BY_ZERO; all before any device call. channels == 0, nsegs
 * == 0 or an empty range: nothing is written, GDSP_OK. */
int gdsp_istft_batch_device(const void *d_X, int64_t ld_seg, int64_t ld_chan, int64_t channels,
                            int64_t nsegs, int64_t seg_row0, int64_t seg_rows, int64_t nfft,
                            int64_t pad, int64_t noverlap, const double *d_win_seg,
                            int64_t out_begin, int64_t out_end, double *d_out, int64_t ldo,
                            void *stream);

/* gdsp_wav_read_floats_device for a multi-channel data chunk, into planar
 * float64 rows: d_out[c*ld_out + i] = the widened float32 of sample c of
 * frame i (d_in[i*channels + c]), i < frames, c < channels <= 65535, ld_out
 * >= frames. Format errors as gdsp_wav_read_floats_device. */
int gdsp_wav_read_floats_planar_device(const void *d_in, int64_t frames, int64_t channels,
                                       int audio_format, int bits_per_sample, double *d_out,
                                       int64_t ld_out, void *stream);

/* gdsp_wav_read_floats on device buffers (d_in: the raw data-chunk bytes at
 * any alignment; d_out: count float32 or float64), stream-ordered: decode a
 * WAV stream straight into the HBM-resident Pwelch input. */
int gdsp_wav_read_floats_device(const void *d_in, int64_t count, int audio_format,
                                int bits_per_sample, void *d_out, int out_f64, void *stream);

/* Device synthetic input: d_out[i] = uniform[-1,1) from splitmix64(seed,
 * offset + i), i < count (float64). Identical to the host generator the tests
 * use; lets the bench generate inputs in HBM without a PCIe copy. */
int gdsp_fill_uniform_device(double *d_out, int64_t count, uint64_t seed, uint64_t offset,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GDSP_FFT_H */
