// dct.hip — the cosine transforms of real rows (scipy.fft.dct / idct, types II
// and III): row r cut or zero-padded to N samples,
//   II   y[k] = 2 sum_{j<N} x[j] cos(pi k (2j+1) / (2N))
//   III  y[j] = x[0] + 2 sum_{1<=k<N} x[k] cos(pi k (2j+1) / (2N))
// times the norm's factors. No reference equivalent. One N-point FFT per row
// (Makhoul): with h = ceil(N/2), v[j] = x[2j] (j < h), v[N-1-j] = x[2j+1] and
// w_k = exp(-i pi k / (2N)),
//   II   V = FFT_N(v), y[k] = 2 Re(w_k V[k]); V[N-k] = conj V[k], so the same
//        product gives y[N-k] = -2 Im(w_k V[k])
//   III  conj W[k] = (x[k] + i x[N-k]) w_k (W[0] = x[0]), v = Re FFT_N(conj W)
//        (the unnormalised inverse of the Hermitian W by the conjugate trick of
//        conv_core.hpp), y[2j] = v[j], y[2j+1] = v[N-1-j]
//
//   dct_lds_kernel     N = 256 ... 16384 a power of 2: a row as z = v + 0 i (II)
//                      or conj W (III), one FFT_N in registers, w_k as the last
//                      pass's epilogue (II) or at the load (III), the scale, the
//                      store, in one workgroup — every sample read from HBM once
//                      and every output written once: the even/odd permutation
//                      is a stride-2 access whose line's other half is the same
//                      row's (an L2 hit), as measured
//   dct2_gather_kernel, dct2_store_kernel,   the composed form's ends (every
//   dct3_pre_kernel, dct3_store_kernel,      other N up to 2^20, and
//   dct_n1_kernel                            GDSP_ALGO_NO_FUSED_DCT) around the
//                                            plan's transform
//
// One row per transform, in both forms, as in hilbert.hip: two real rows could
// ride one transform, but a packed row's roundoff depends on its partner. A
// row's outputs depend on that row alone, bit for bit; a row of zeros gives
// zeros; a NaN or Inf makes its own row non-finite and changes nothing else.
#include <cmath>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "conv_core.hpp"
#include "fft_device.hpp"
#include "launch.hpp"
#include "plan.hpp"

namespace gdsp {

// sample index of v[i], and its inverse
__host__ __device__ __forceinline__ int64_t dct_src(int64_t i, int64_t N) {
  return i < (N + 1) / 2 ? 2 * i : 2 * (N - 1 - i) + 1;
}
__host__ __device__ __forceinline__ int64_t dct_pos(int64_t i, int64_t N) {
  return (i & 1) ? N - 1 - (i >> 1) : i >> 1;
}

// Whether type II applies w_k as the last pass's epilogue: up to 8192. At 16384
// 512 threads have 256 registers each and the epilogue's prefetched factors
// spill (156 bytes of scratch a lane); there w_k is applied after the
// transform, at the store, as the chirp-z kernel applies its postmultiplier.
__host__ __device__ constexpr bool dct_epi(int log2n) { return log2n <= 13; }

// Epilogue of type II's last pass (fft_regs EPI): register k of thread t holds
// bin b = t + k T; v[k] = w_b V[b] for the bins up to N/2 (registers below
// E/2, and register E/2 for thread 0's bin N/2), the factor loaded ahead of
// the butterfly's arithmetic. The registers above are not computed.
template <int T, int EH>
struct DctEpi {
  const cd *w;  // the w_k table + t
  static constexpr bool on = true;
  __device__ static constexpr bool want(int k) { return k <= EH; }
  __device__ cd load(int k) const { return w[k * T]; }
  template <int E>
  __device__ void apply(cd (&v)[E], int k, cd u, cd f) const { v[k] = cmul(u, f); }
};

// One workgroup holds TPW rows in registers (thread t of a row owns elements
// t + k T), as hilbert_lds_kernel does. nn = min(n, N): the samples read of a
// row. wk: w_k, N entries. II stores Re(w_k V[k]) scale (k = 0: scale0); III
// takes x[0] a0 and stores v scale.
// The even/odd permutation (II's load, III's store) is a stride-2 access whose
// line's other half the same row takes (an L2 hit), and III's x[N-k] a second
// read of the row: faster at every size than whole-line accesses through the
// row's LDS, by up to 2.1x for type II.
// out may be x itself (exactly in place), so x is not __restrict__: every load
// of a row stands before the transform's first barrier, every store after its
// last, and no row reaches into another's.
template <int LOG2N, int LOG2E, int TYPE>
__global__ __launch_bounds__((Geo<LOG2N, LOG2E>::WG)) void dct_lds_kernel(
    const double *x, int64_t ldx, int64_t rows, int nn, double *out, int64_t ldo,
    const cd *__restrict__ tw, const cd *__restrict__ wk, double a0, double scale,
    double scale0) {
  using G = Geo<LOG2N, LOG2E>;
  constexpr int E = G::E, T = G::T, N = G::N;
  static_assert(T >= 16, "rows of fewer than 16 threads need LDS staging to stay coalesced");
  static_assert(G::NPASS > 1, "the barriers of the exchanges order in-place loads and stores");
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
  double *const dst = out + gl * ldo;
  double *const lre = lds + slot * G::STRIDE;
  cd v[E];
  if constexpr (TYPE == 2) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int j = (int)dct_src(t + k * T, N);
      v[k].x = j < nn ? xr[j] : 0.0;  // the line's other half: an L2 hit
      v[k].y = 0.0;
    }
    if constexpr (dct_epi(LOG2N)) {
      const DctEpi<T, E / 2> de{wk + t};
      fft_regs<LOG2N, true, 0, LOG2E, 0, 0, const cd *, 1, 0, DctEpi<T, E / 2>,
               conv_prew(LOG2N)>(v, t, tw, lre, lre, true, de);
    } else {
      fft_regs<LOG2N, true, 0, LOG2E, 0, 0, const cd *, 1, 0, NoEpi, conv_prew(LOG2N)>(
          v, t, tw, lre, lre, true);
    }
    if (!valid) return;
    const int to = dct_epi(LOG2N) ? t : opaque_int(t);
    // bins b < N/2 give y[b] and y[N-b]: two runs of whole lines (without the
    // epilogue: w_k here, in fenced runs of 4, so the factors of all E/2 do
    // not sit beside the transform's registers)
#pragma unroll
    for (int k0 = 0; k0 < E / 2; k0 += 4) {
      cd p[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        p[k] = dct_epi(LOG2N) ? v[k0 + k] : cmul(v[k0 + k], wk[to + (k0 + k) * T]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = to + (k0 + k) * T;
        const double s = k0 + k == 0 && t == 0 ? scale0 : scale;
        __builtin_nontemporal_store(p[k].x * s, &dst[b]);
        if (k0 + k > 0 || t > 0) __builtin_nontemporal_store(-p[k].y * scale, &dst[N - b]);
      }
      if constexpr (!dct_epi(LOG2N)) __builtin_amdgcn_sched_barrier(0);
    }
    if (t == 0) {
      const cd p = dct_epi(LOG2N) ? v[E / 2] : cmul(v[E / 2], wk[N / 2]);
      __builtin_nontemporal_store(p.x * scale, &dst[N / 2]);
    }
  } else {
    // E = 32: in fenced runs of 8 behind a laundered index, or the addresses
    // and factors of all 32 are alive at once beside the transform's registers
    int tl = t;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      if constexpr (E > 16) {
        if (k % 8 == 0) tl = opaque_int(t);
      }
      const int i = tl + k * T, m = (N - i) & (N - 1);
      double a = i < nn ? xr[i] : 0.0;
      double b = m < nn ? xr[m] : 0.0;  // the second read of the row: an L2 hit
      if (k == 0) {  // W[0] = a0 x[0]
        a = t == 0 ? a * a0 : a;
        b = t == 0 ? 0.0 : b;
      }
      v[k] = cmul(cd{a, b}, wk[i]);
      if constexpr (E > 16) {
        if (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);
      }
    }
    fft_regs<LOG2N, true, 1, LOG2E, 0, 0, const cd *, 1, 0, NoEpi, conv_prew(LOG2N)>(
        v, t, tw, lre, lre, true);
    // the real parts are v[j], j = t + k T; the imaginary parts roundoff
    if (!valid) return;
    // (the index laundered, as hilbert_lds_kernel's store has it: no store
    // address is computed before the transform)
    const int to = opaque_int(t);
#pragma unroll
    for (int k = 0; k < E; ++k) dst[dct_src(to + k * T, N)] = v[k].x * scale;
  }
}

template <int LOG2N, int TYPE>
static hipError_t launch_dct_t(const double *x, int64_t ldx, int64_t rows, int64_t nn,
                               double *out, int64_t ldo, const cd *tw, const cd *wk, double a0,
                               double scale, double scale0, hipStream_t s) {
  constexpr int LOG2E = conv_log2e(LOG2N);
  using G = Geo<LOG2N, LOG2E>;
  const int64_t nblk = (rows + G::TPW - 1) / G::TPW;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((dct_lds_kernel<LOG2N, LOG2E, TYPE>), dim3((unsigned)nblk), dim3(G::WG), 0,
                     s, x, ldx, rows, (int)nn, out, ldo, tw, wk, a0, scale, scale0);
  return hipGetLastError();
}

bool dct_lds_applies(int64_t N) {
  return N >= ((int64_t)1 << kConvMinLog2) && N <= ((int64_t)1 << kMaxLdsLog2) &&
         (N & (N - 1)) == 0;
}

hipError_t launch_dct_lds(int log2n, int type, const double *x, int64_t ldx, int64_t rows,
                          int64_t n, double *out, int64_t ldo, const cd *tw, const cd *wk,
                          double a0, double scale, double scale0, hipStream_t s) {
  const int64_t N = (int64_t)1 << log2n, nn = n < N ? n : N;
  if (rows <= 0 || n <= 0 || (type != 2 && type != 3) || !x || !out || !tw || !wk ||
      (rows > 1 && (ldx < nn || ldo < N)))
    return hipErrorInvalidValue;
  static_assert(kConvMinLog2 == 8 && kMaxLdsLog2 == 14, "the cases below");
#define GDSP_DCT_CASE(L)                                                                   \
  case L:                                                                                  \
    return type == 2                                                                       \
               ? launch_dct_t<L, 2>(x, ldx, rows, nn, out, ldo, tw, wk, a0, scale, scale0, s) \
               : launch_dct_t<L, 3>(x, ldx, rows, nn, out, ldo, tw, wk, a0, scale, scale0, s)
  switch (log2n) {
    GDSP_DCT_CASE(8);
    GDSP_DCT_CASE(9);
    GDSP_DCT_CASE(10);
    GDSP_DCT_CASE(11);
    GDSP_DCT_CASE(12);
    GDSP_DCT_CASE(13);
    GDSP_DCT_CASE(14);
    default: return hipErrorInvalidValue;
  }
#undef GDSP_DCT_CASE
}

// ---- the composed form --------------------------------------------------------
// buf[r N + i] = v[i] of row r0 + r (the padded row's sample dct_src(i))
__global__ __launch_bounds__(256) void dct2_gather_kernel(const double *__restrict__ x,
                                                          int64_t ldx, int64_t r0, int64_t nn,
                                                          int64_t N, double *__restrict__ buf,
                                                          int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / N, i = e - r * N, j = dct_src(i, N);
  buf[e] = j < nn ? x[(r0 + r) * ldx + j] : 0.0;
}

// y[k] = Re(w_k V[k]) scale (k = 0: scale0) from the full spectra
__global__ __launch_bounds__(256) void dct2_store_kernel(const cd *__restrict__ spec,
                                                         const cd *__restrict__ wk, int64_t N,
                                                         int64_t r0, double *__restrict__ out,
                                                         int64_t ldo, double scale, double scale0,
                                                         int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / N, k = e - r * N;
  out[(r0 + r) * ldo + k] = cmul(spec[e], wk[k]).x * (k == 0 ? scale0 : scale);
}

// spec[r N + k] = conj W[k] = (x[k] + i x[N-k]) w_k of row r0 + r, x[0] times a0
__global__ __launch_bounds__(256) void dct3_pre_kernel(const double *__restrict__ x, int64_t ldx,
                                                       int64_t r0, int64_t nn, int64_t N,
                                                       const cd *__restrict__ wk, double a0,
                                                       cd *__restrict__ spec, int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / N, k = e - r * N, m = N - k;
  const double *const xr = x + (r0 + r) * ldx;
  double a = k < nn ? xr[k] : 0.0;
  const double b = k > 0 && m < nn ? xr[m] : 0.0;
  if (k == 0) a *= a0;
  spec[e] = cmul(cd{a, b}, wk[k]);
}

// y[i] = Re spec[dct_pos(i)] scale
__global__ __launch_bounds__(256) void dct3_store_kernel(const cd *__restrict__ spec, int64_t N,
                                                         int64_t r0, double *__restrict__ out,
                                                         int64_t ldo, double scale,
                                                         int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / N, i = e - r * N;
  out[(r0 + r) * ldo + i] = spec[r * N + dct_pos(i, N)].x * scale;
}

// N = 1: y[0] = x[0] c (out may be x itself: neither is __restrict__)
__global__ __launch_bounds__(256) void dct_n1_kernel(const double *x, int64_t ldx, double *out,
                                                     int64_t ldo, int64_t rows, double c) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < rows) out[r * ldo] = x[r * ldx] * c;
}

static bool dct_grid(int64_t cnt, int64_t N, int64_t *count, unsigned *nblk) {
  if (cnt <= 0 || N <= 0 || cnt > INT64_MAX / N) return false;
  *count = cnt * N;
  const int64_t b = (*count + 255) / 256;
  if (b > 0x7fffffff) return false;
  *nblk = (unsigned)b;
  return true;
}

hipError_t launch_dct2_gather(const double *x, int64_t ldx, int64_t r0, int64_t cnt, int64_t n,
                              int64_t N, double *buf, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!x || !buf || n <= 0 || !dct_grid(cnt, N, &count, &nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dct2_gather_kernel, dim3(nblk), dim3(256), 0, s, x, ldx, r0, n < N ? n : N,
                     N, buf, count);
  return hipGetLastError();
}

hipError_t launch_dct2_store(const cd *spec, const cd *wk, int64_t N, int64_t r0, int64_t cnt,
                             double *out, int64_t ldo, double scale, double scale0,
                             hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!spec || !wk || !out || !dct_grid(cnt, N, &count, &nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dct2_store_kernel, dim3(nblk), dim3(256), 0, s, spec, wk, N, r0, out, ldo,
                     scale, scale0, count);
  return hipGetLastError();
}

hipError_t launch_dct3_pre(const double *x, int64_t ldx, int64_t r0, int64_t cnt, int64_t n,
                           int64_t N, const cd *wk, double a0, cd *spec, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!x || !wk || !spec || n <= 0 || !dct_grid(cnt, N, &count, &nblk))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dct3_pre_kernel, dim3(nblk), dim3(256), 0, s, x, ldx, r0, n < N ? n : N, N,
                     wk, a0, spec, count);
  return hipGetLastError();
}

hipError_t launch_dct3_store(const cd *spec, int64_t N, int64_t r0, int64_t cnt, double *out,
                             int64_t ldo, double scale, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!spec || !out || !dct_grid(cnt, N, &count, &nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dct3_store_kernel, dim3(nblk), dim3(256), 0, s, spec, N, r0, out, ldo, scale,
                     count);
  return hipGetLastError();
}

hipError_t launch_dct_n1(const double *x, int64_t ldx, double *out, int64_t ldo, int64_t rows,
                         double c, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!x || !out || !dct_grid(rows, 1, &count, &nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dct_n1_kernel, dim3(nblk), dim3(256), 0, s, x, ldx, out, ldo, rows, c);
  return hipGetLastError();
}

}  // namespace gdsp

// ---- the host part --------------------------------------------------------------
using gdsp::cd;
using namespace gdsp_api;

namespace {

constexpr long double kPiL = 3.141592653589793238462643383279502884L;
// samples of one chunk of the composed form and of one range of the host entry
constexpr int64_t DCT_CHUNK_ELEMS = (int64_t)1 << 24;
constexpr int64_t kDctMaxN = (int64_t)1 << 20;

// w_k = exp(-i pi k / (2N)), k < N, in long double, rounded once. Past N/2 the
// cosine is taken as the sine of the complement pi (N - k) / (2N), an exact
// ratio too: every angle evaluated is at most pi/4, so the small component
// keeps its relative accuracy.
void dct_twiddles(int64_t N, cd *w) {
  for (int64_t k = 0; k < N; ++k) {
    const bool low = 2 * k <= N;
    const long double a = kPiL * (long double)(low ? k : N - k) / (long double)(2 * N);
    const long double c = cosl(a), s = sinl(a);
    w[k] = low ? cd{(double)c, -(double)s} : cd{(double)s, -(double)c};
  }
}

// the device tables, one per (device, N), built on first use and kept
std::mutex g_dct_mu;
std::map<std::pair<int, int64_t>, DevPtr<cd>> g_dct_tab;

int dct_table(int64_t N, const cd **out) {
  int dev = 0;
  STCHK(current_device(&dev));
  std::lock_guard<std::mutex> lk(g_dct_mu);
  auto it = g_dct_tab.find({dev, N});
  if (it == g_dct_tab.end()) {
    std::vector<cd> h((size_t)N);
    dct_twiddles(N, h.data());
    DevPtr<cd> t;
    STCHK(device_table(dev, h, t));
    it = g_dct_tab.emplace(std::make_pair(dev, N), std::move(t)).first;
  }
  *out = it->second.get();
  return GDSP_OK;
}

bool dct_fused_now(int64_t N) {
  return N > 0 && gdsp::dct_lds_applies(N) && !(gdsp::algo_flags() & GDSP_ALGO_NO_FUSED_DCT);
}

int64_t dct_chunk_rows(int64_t N, int64_t rows) {
  int64_t r = DCT_CHUNK_ELEMS / N;
  if (r < 1) r = 1;
  return r < rows ? r : rows;
}

// The factors of a (type, norm): type II stores Re(w_k V[k]) scale (k = 0:
// scale0), type III takes x[0] a0 and stores v scale; long double, rounded once.
// one: y[0] / x[0] at N = 1 (ortho's type III sqrt(2) sqrt(1/2) is 1 there, not
// the product of two rounded factors).
struct DctNorm {
  double a0, scale, scale0, one;
};
DctNorm dct_norm(int type, int norm, int64_t N) {
  const long double n2 = 2.0L * (long double)N;
  const long double f = norm == GDSP_DCT_BACKWARD ? 1.0L
                        : norm == GDSP_DCT_FORWARD ? 1.0L / n2
                                                   : sqrtl(1.0L / n2);
  if (type == 3) {
    const long double a0 = norm == GDSP_DCT_ORTHO ? sqrtl(2.0L) : 1.0L;
    return {(double)a0, (double)f, (double)f, (double)(a0 * f)};
  }
  const long double f0 = norm == GDSP_DCT_ORTHO ? sqrtl(1.0L / (2.0L * n2)) : f;
  return {1.0, (double)(2.0L * f), (double)(2.0L * f0), (double)(2.0L * f0)};
}

// Argument checks shared by the host and device entries, in the order of the
// header's table; *done: nothing to do; *N: the transform length. No device
// call is made.
int dct_check(const void *x, int64_t ldx, int64_t rows, int64_t n, int64_t nfft, int type,
              int norm, const void *out, int64_t ldo, int64_t *N, bool *done) {
  *done = false;
  if (rows < 0 || n < 0 || nfft < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (type != 2 && type != 3) return fail(GDSP_ERR_INVALID, "type must be 2 or 3");
  if (norm < GDSP_DCT_BACKWARD || norm > GDSP_DCT_FORWARD)
    return fail(GDSP_ERR_INVALID, "norm must be 0, 1 or 2");
  *N = nfft == 0 ? n : nfft;
  if (rows > 1 && (ldx < (n < *N ? n : *N) || ldo < *N))
    return fail(GDSP_ERR_INVALID, "row stride below the row length");
  if (rows == 0) {
    *done = true;
    return GDSP_OK;
  }
  if (n == 0 || *N == 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  if (!x || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  if (*N > kDctMaxN) return fail(GDSP_ERR_UNSUPPORTED, "transform length above 2^20");
  return GDSP_OK;
}

// work (NULL: the workspace pool): nothing in the fused form and at N = 1;
// composed, dct_chunk_rows(N, rows) rows of N complex128, then as many of N
// float64 (type II's permuted rows)
int dct_rows(const double *d_x, int64_t ldx, int64_t rows, int64_t n, int64_t N, int type,
             int norm, double *d_out, int64_t ldo, void *work, hipStream_t s) {
  const DctNorm f = dct_norm(type, norm, N);
  if (N == 1) {  // no transform: II 2 x[0], III x[0], times the norm's factors
    HIPCHK(gdsp::launch_dct_n1(d_x, ldx, d_out, ldo, rows, f.one, s));
    return GDSP_OK;
  }
  gdsp_plan *p = nullptr;
  STCHK(get_plan(N, &p));
  const cd *wk = nullptr;
  STCHK(dct_table(N, &wk));
  // a power of 2 up to 2^14 is KIND_LDS under every flag set; the kind is
  // checked because the kernel reads that plan's twiddle table
  if (dct_fused_now(N) && p->kind == KIND_LDS) {
    HIPCHK(gdsp::launch_dct_lds(p->log2n, type, d_x, ldx, rows, n, d_out, ldo, p->tw, wk, f.a0,
                                f.scale, f.scale0, s));
    return GDSP_OK;
  }
  const int64_t cr = dct_chunk_rows(N, rows);
  DevBuf w;
  if (!work) {
    STCHK(w.alloc((size_t)cr * (size_t)N * (sizeof(cd) + sizeof(double)), s, SLOT_DCT));
    work = w.p;
  }
  cd *spec = (cd *)work;
  double *buf = (double *)(spec + cr * N);
  for (int64_t r0 = 0; r0 < rows; r0 += cr) {
    later_chunk(r0);
    const int64_t cnt = rows - r0 < cr ? rows - r0 : cr;
    if (type == 2) {
      HIPCHK(gdsp::launch_dct2_gather(d_x, ldx, r0, cnt, n, N, buf, s));
      STCHK(exec_plan(p, buf, spec, cnt, false, gdsp::LOAD_REAL, s));
      HIPCHK(gdsp::launch_dct2_store(spec, wk, N, r0, cnt, d_out, ldo, f.scale, f.scale0, s));
    } else {
      // the inverse of W as the forward transform of conj W, without a 1/N
      HIPCHK(gdsp::launch_dct3_pre(d_x, ldx, r0, cnt, n, N, wk, f.a0, spec, s));
      STCHK(exec_plan(p, spec, spec, cnt, false, gdsp::LOAD_COMPLEX, s));
      HIPCHK(gdsp::launch_dct3_store(spec, N, r0, cnt, d_out, ldo, f.scale, s));
    }
  }
  return GDSP_OK;
}

}  // namespace

int gdsp_dct_fused(int64_t nfft) { return dct_fused_now(nfft) ? 1 : 0; }

int64_t gdsp_dct_work_doubles(int64_t rows, int64_t nfft) {
  if (rows <= 0 || nfft <= 1 || nfft > kDctMaxN || dct_fused_now(nfft)) return 0;
  return dct_chunk_rows(nfft, rows) * nfft * 3;
}

int gdsp_dct_twiddles(int64_t nfft, double *re_im) {
  if (nfft < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (nfft == 0) return fail(GDSP_ERR_EMPTY, "empty table");
  if (!re_im) return fail(GDSP_ERR_INVALID, "NULL pointer");
  if (nfft > kDctMaxN) return fail(GDSP_ERR_UNSUPPORTED, "transform length above 2^20");
  dct_twiddles(nfft, (cd *)re_im);
  return GDSP_OK;
}

int gdsp_dct_batch_device(const void *d_x, int64_t ldx, int64_t rows, int64_t n, int64_t nfft,
                          int type, int norm, void *d_out, int64_t ldo, void *d_work,
                          void *stream) {
  int64_t N = 0;
  bool done = false;
  STCHK(dct_check(d_x, ldx, rows, n, nfft, type, norm, d_out, ldo, &N, &done));
  if (done) return GDSP_OK;
  const int64_t nn = n < N ? n : N;
  // exactly in place is served: a workgroup, or the gather of a chunk, has read
  // a whole row before any of it is stored, and no row reaches into another
  const bool in_place = d_out == d_x && N <= n && (rows == 1 || ldo == ldx);
  if (rows == 1) ldx = nn, ldo = N;
  const uintptr_t xa = (uintptr_t)d_x, oa = (uintptr_t)d_out;
  const uintptr_t xe = xa + ((uintptr_t)(rows - 1) * (uintptr_t)ldx + (uintptr_t)nn) * 8;
  const uintptr_t oe = oa + ((uintptr_t)(rows - 1) * (uintptr_t)ldo + (uintptr_t)N) * 8;
  if (!in_place && xa < oe && oa < xe)
    return fail(GDSP_ERR_INVALID, "d_out overlaps d_x and is not exactly in place");
  return dct_rows((const double *)d_x, ldx, rows, n, N, type, norm, (double *)d_out, ldo, d_work,
                  (hipStream_t)stream);
}

int gdsp_dct_batch(const double *x, int64_t ldx, int64_t rows, int64_t n, int64_t nfft, int type,
                   int norm, double *out, int64_t ldo) {
  int64_t N = 0;
  bool done = false;
  STCHK(dct_check(x, ldx, rows, n, nfft, type, norm, out, ldo, &N, &done));
  if (done) return GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const int64_t nn = n < N ? n : N;  // the samples a row gives
  if (rows == 1) ldx = nn, ldo = N;
  int64_t rng = DCT_CHUNK_ELEMS / N;
  if (rng < 1) rng = 1;
  DevBuf dx, dout;
  for (int64_t r0 = 0; r0 < rows; r0 += rng) {
    later_chunk(r0);
    const int64_t cnt = rows - r0 < rng ? rows - r0 : rng;
    STCHK(dx.alloc((size_t)cnt * (size_t)nn * sizeof(double), s, SLOT_IN));
    STCHK(dout.alloc((size_t)cnt * (size_t)N * sizeof(double), s, SLOT_DCT_OUT));
    double *px = (double *)dx.p, *po = (double *)dout.p;
    STCHK(run_queued(s, [&]() -> int {
      STCHK(stage_rows(px, x + r0 * ldx, cnt, nn, ldx, nn, s));
      return dct_rows(px, nn, cnt, nn, N, type, norm, po, N, nullptr, s);
    }));
    // returns after the stream drained: the next range may reuse the buffers
    STCHK(unstage_rows(out + r0 * ldo, po, cnt, N, ldo, s));
  }
  return GDSP_OK;
}
