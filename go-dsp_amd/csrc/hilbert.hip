// hilbert.hip — the analytic signal of real rows (scipy.signal.hilbert(x, N)):
// row r cut or zero-padded to N samples, h_r = IFFT_N(m FFT_N(x_r)) with
// m[f] = -i for 0 < f < N/2, +i for N/2 < f < N and 0 at f = 0 and f = N/2,
// stored as x_r + i h_r (ANALYTIC), h_r (QUADRATURE) or sqrt(fma(x, x, h h))
// (ENVELOPE). No reference equivalent.
//
//   hilbert_lds_kernel    N = 256 ... 16384 a power of 2: a row as z = x + 0 i,
//                         FFT_N, the multiplier as a swap of re and im on the
//                         last pass (HilbertEpi: no table, no multiply), second
//                         FFT_N as the inverse, the outputs stored, in one
//                         workgroup — the samples read once (at 16384 once more
//                         from L2 for the real part and the envelope) and each
//                         output written once
//   hilbert_gather_kernel, the composed form's ends (every other N, and
//   hilbert_mask_kernel,   GDSP_ALGO_NO_FUSED_HILBERT): padded real rows for
//   hilbert_store_kernel   the plan's real-row transform, the multiplier in
//                         place, and after the plan's inverse the three kinds
//
// One row per transform, in both forms. m maps real rows to real rows, so two
// rows a, b could ride one transform as a + i b and come back as Ha + i Hb; an
// earlier form of this kernel did, at about half the arithmetic. But a packed
// row's roundoff depends on its partner (the twiddle products mix re and im),
// so a NaN in one row, which forces the partner to be computed alone, moved the
// partner's bits by 5-12 u. What the entry promises instead: a row's outputs
// depend on that row alone, bit for bit — whatever its neighbours hold, however
// a job is cut into calls. A row of exact zeros gives exact zeros, a quiet row
// keeps its own relative accuracy beside a loud one, and a NaN or an infinity
// makes every output of its own row non-finite and changes no bit elsewhere,
// all without a balance, a vote or a rerun.
#include <type_traits>

#include "conv_core.hpp"
#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

// Where the kinds that store the input (ANALYTIC's real part, ENVELOPE) keep
// the loaded samples: in registers through both transforms up to 8192, read
// again at the store (an L2 hit) at 16384, where 512 threads have 256 registers
// each. -DGDSP_HILBERT_KEEP=0 or 1 forces one form for every
// size (the comparison builds).
#ifdef GDSP_HILBERT_KEEP
__host__ __device__ constexpr bool hilbert_keep(int) { return GDSP_HILBERT_KEEP != 0; }
#else
__host__ __device__ constexpr bool hilbert_keep(int log2n) { return log2n <= 13; }
#endif

template <int KIND>
using HilbertOut = typename std::conditional<KIND == 0, cd, double>::type;

// Epilogue of the first FFT's last pass (fft_regs EPI): v = conj(m u). Register
// k of thread t holds bin t + k T, so k < E/2 is a positive frequency
// (-i u = u.y - i u.x, conjugated (u.y, u.x)) and k >= E/2 a negative one
// (conj(i u) = (-u.y, -u.x)), decided at compile time; bins 0 and N/2 are
// registers 0 and E/2 of thread 0. The conjugate turns the second forward FFT
// into the inverse (conv_core.hpp, YhatEpi).
struct HilbertEpi {
  bool t0;  // thread 0 of the transform
  static constexpr bool on = true;
  __device__ static constexpr bool want(int) { return true; }
  __device__ cd load(int) const { return {0.0, 0.0}; }
  template <int E>
  __device__ void apply(cd (&v)[E], int k, cd u, cd) const {
    double re = k < E / 2 ? u.y : -u.y, im = k < E / 2 ? u.x : -u.x;
    if (k == 0 || k == E / 2) {
      re = t0 ? 0.0 : re;  // per component: a select of the struct goes through scratch
      im = t0 ? 0.0 : im;
    }
    v[k] = {re, im};
  }
};

// sqrt(x^2 + h^2) as both forms compute it
__device__ __forceinline__ double hilbert_env(double x, double h) { return sqrt(fma(x, x, h * h)); }

// One workgroup holds TPW rows in registers (thread t of a row owns elements
// t + k T), as convolve_lds_kernel does. nn = min(n, N): the samples read of a
// row.
template <int LOG2N, int LOG2E, int KIND>
__global__ __launch_bounds__((Geo<LOG2N, LOG2E>::WG)) void hilbert_lds_kernel(
    const double *__restrict__ x, int64_t ldx, int64_t rows, int nn,
    HilbertOut<KIND> *__restrict__ out, int64_t ldo, const cd *__restrict__ tw, double scale) {
  using G = Geo<LOG2N, LOG2E>;
  constexpr int E = G::E, T = G::T;
  constexpr bool KEEP = hilbert_keep(LOG2N) && KIND != 1;
  static_assert(T >= 16, "rows of fewer than 16 threads need LDS staging to stay coalesced");
  __shared__ double lds[G::LDS_DOUBLES];
  const int lt = threadIdx.x;
  const int slot = G::TPW == 1 ? 0 : lt / T, t = lt & (T - 1);
  const int64_t g = xcd_remap(blockIdx.x, gridDim.x) * G::TPW + slot;
  // Only the last workgroup can hold slots past the rows (TPW > 1): they run
  // the last row again (clamped) and store nothing, so the whole workgroup
  // reaches every barrier.
  const bool valid = G::TPW == 1 || g < rows;
  const int64_t gl = valid ? g : rows - 1;
  const double *const xr = x + gl * ldx;
  HilbertOut<KIND> *const dst = out + gl * ldo;
  double *const lre = lds + slot * G::STRIDE;
  cd v[E];
  double kept[KEEP ? E : 1];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int i = t + k * T;
    // read once where nothing reads it again; else left for the L2
    if constexpr (KIND == 1 || KEEP) v[k].x = i < nn ? ld_nt(&xr[i]) : 0.0;
    else v[k].x = i < nn ? xr[i] : 0.0;
    v[k].y = 0.0;
    if constexpr (KEEP) kept[k] = v[k].x;
  }
  const HilbertEpi he{t == 0};
  fft_regs<LOG2N, true, 1, LOG2E, 0, 0, const cd *, 1, 0, HilbertEpi, conv_prew(LOG2N)>(
      v, t, tw, lre, lre, true, he);
  fft_regs<LOG2N, true, 1, LOG2E, 0, 0, const cd *, 1, 0, NoEpi, conv_prew(LOG2N)>(
      v, t, tw, lre, lre, false);
  // v = conj(N (h + i 0)): the real parts are h, the imaginary parts roundoff
  if (!valid) return;
  const int to = opaque_int(t);
  // in runs of CH elements, fenced: the samples read again for all E at once
  // would sit beside the transform's registers
  constexpr int CH = E > 16 ? 4 : 8;
#pragma unroll
  for (int k0 = 0; k0 < E; k0 += CH) {
    double xs[CH];
    if constexpr (KEEP) {
#pragma unroll
      for (int k = 0; k < CH; ++k) xs[k] = kept[k0 + k];
    } else if constexpr (KIND != 1) {
#pragma unroll
      for (int k = 0; k < CH; ++k)
        xs[k] = to + (k0 + k) * T < nn ? ld_nt(&xr[to + (k0 + k) * T]) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int i = to + (k0 + k) * T;
      const double h = v[k0 + k].x * scale;
      if constexpr (KIND == 0) st_nt(&dst[i], cd{xs[k], h});
      else if constexpr (KIND == 1) __builtin_nontemporal_store(h, &dst[i]);
      else __builtin_nontemporal_store(hilbert_env(xs[k], h), &dst[i]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int LOG2N, int KIND>
static hipError_t launch_hil_t(const double *x, int64_t ldx, int64_t rows, int64_t nn, void *out,
                               int64_t ldo, const cd *tw, hipStream_t s) {
  constexpr int LOG2E = conv_log2e(LOG2N);
  using G = Geo<LOG2N, LOG2E>;
  const int64_t nblk = (rows + G::TPW - 1) / G::TPW;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((hilbert_lds_kernel<LOG2N, LOG2E, KIND>), dim3((unsigned)nblk), dim3(G::WG),
                     0, s, x, ldx, rows, (int)nn, (HilbertOut<KIND> *)out, ldo, tw,
                     1.0 / (double)G::N);
  return hipGetLastError();
}

bool hilbert_lds_applies(int64_t N) {
  return N >= ((int64_t)1 << kConvMinLog2) && N <= ((int64_t)1 << kMaxLdsLog2) &&
         (N & (N - 1)) == 0;
}

hipError_t launch_hilbert_lds(int log2n, int kind, const double *x, int64_t ldx, int64_t rows,
                              int64_t n, void *out, int64_t ldo, const cd *tw, hipStream_t s) {
  const int64_t N = (int64_t)1 << log2n, nn = n < N ? n : N;
  if (rows <= 0 || n <= 0 || kind < 0 || kind > 2 || !x || !out || !tw ||
      (rows > 1 && (ldx < nn || ldo < N)))
    return hipErrorInvalidValue;
  static_assert(kConvMinLog2 == 8 && kMaxLdsLog2 == 14, "the cases below");
#define GDSP_HIL_CASE(L)                                                               \
  case L:                                                                              \
    return kind == 0   ? launch_hil_t<L, 0>(x, ldx, rows, nn, out, ldo, tw, s)         \
           : kind == 1 ? launch_hil_t<L, 1>(x, ldx, rows, nn, out, ldo, tw, s)         \
                       : launch_hil_t<L, 2>(x, ldx, rows, nn, out, ldo, tw, s)
  switch (log2n) {
    GDSP_HIL_CASE(8);
    GDSP_HIL_CASE(9);
    GDSP_HIL_CASE(10);
    GDSP_HIL_CASE(11);
    GDSP_HIL_CASE(12);
    GDSP_HIL_CASE(13);
    GDSP_HIL_CASE(14);
    default: return hipErrorInvalidValue;
  }
#undef GDSP_HIL_CASE
}

// ---- the composed form --------------------------------------------------------
// buf[r N + i] = x[(r0 + r) ldx + i] for i < nn, else 0
__global__ __launch_bounds__(256) void hilbert_gather_kernel(const double *__restrict__ x,
                                                             int64_t ldx, int64_t r0, int64_t nn,
                                                             int64_t N, double *__restrict__ buf,
                                                             int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / N, i = e - r * N;
  buf[e] = i < nn ? x[(r0 + r) * ldx + i] : 0.0;
}

// spec[r N + f] times m[f], in place: a swap with a sign, or an exact zero
__global__ __launch_bounds__(256) void hilbert_mask_kernel(cd *spec, int64_t N, int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t f = e % N;
  const cd u = spec[e];
  cd v = {0.0, 0.0};
  if (f != 0 && 2 * f != N) v = 2 * f < N ? cd{u.y, -u.x} : cd{-u.y, u.x};
  spec[e] = v;
}

// row r0 + r of out from the real part of the inverse transform (spec) and the
// row's own samples; spec == nullptr: h = 0 (N = 1)
template <int KIND>
__global__ __launch_bounds__(256) void hilbert_store_kernel(
    const double *__restrict__ x, int64_t ldx, int64_t r0, int64_t nn, int64_t N,
    const cd *__restrict__ spec, HilbertOut<KIND> *__restrict__ out, int64_t ldo, int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / N, i = e - r * N;
  const double h = spec ? spec[e].x : 0.0;
  HilbertOut<KIND> *const o = out + (r0 + r) * ldo + i;
  if constexpr (KIND == 1) {
    *o = h;
  } else {
    const double xr = i < nn ? x[(r0 + r) * ldx + i] : 0.0;
    if constexpr (KIND == 0) *o = cd{xr, h};
    else *o = hilbert_env(xr, h);
  }
}

static bool hilbert_grid(int64_t cnt, int64_t N, int64_t *count, unsigned *nblk) {
  if (cnt <= 0 || N <= 0 || cnt > INT64_MAX / N) return false;
  *count = cnt * N;
  const int64_t b = (*count + 255) / 256;
  if (b > 0x7fffffff) return false;
  *nblk = (unsigned)b;
  return true;
}

hipError_t launch_hilbert_gather(const double *x, int64_t ldx, int64_t r0, int64_t cnt, int64_t n,
                                 int64_t N, double *buf, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!x || !buf || n <= 0 || !hilbert_grid(cnt, N, &count, &nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hilbert_gather_kernel, dim3(nblk), dim3(256), 0, s, x, ldx, r0,
                     n < N ? n : N, N, buf, count);
  return hipGetLastError();
}

hipError_t launch_hilbert_mask(cd *spec, int64_t cnt, int64_t N, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!spec || !hilbert_grid(cnt, N, &count, &nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hilbert_mask_kernel, dim3(nblk), dim3(256), 0, s, spec, N, count);
  return hipGetLastError();
}

hipError_t launch_hilbert_store(int kind, const double *x, int64_t ldx, int64_t r0, int64_t cnt,
                                int64_t n, int64_t N, const cd *spec, void *out, int64_t ldo,
                                hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!x || !out || n <= 0 || kind < 0 || kind > 2 || !hilbert_grid(cnt, N, &count, &nblk))
    return hipErrorInvalidValue;
  const int64_t nn = n < N ? n : N;
  if (kind == 0)
    hipLaunchKernelGGL(hilbert_store_kernel<0>, dim3(nblk), dim3(256), 0, s, x, ldx, r0, nn, N,
                       spec, (cd *)out, ldo, count);
  else if (kind == 1)
    hipLaunchKernelGGL(hilbert_store_kernel<1>, dim3(nblk), dim3(256), 0, s, x, ldx, r0, nn, N,
                       spec, (double *)out, ldo, count);
  else
    hipLaunchKernelGGL(hilbert_store_kernel<2>, dim3(nblk), dim3(256), 0, s, x, ldx, r0, nn, N,
                       spec, (double *)out, ldo, count);
  return hipGetLastError();
}

}  // namespace gdsp
