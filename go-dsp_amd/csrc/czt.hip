// czt.hip — the chirp-z transform of rows on an arc of a circle
// (scipy.signal.czt with |w| = 1, scipy.signal.zoom_fft): for z_k = a_abs
// exp(2 pi i (a_turns + k step)), step = step_turns / step_div turns, k < m,
//   X[k] = sum_{j<n} x[j] z_k^-j.
// No reference equivalent. With c(j) = exp(-pi i step j^2), jk = (j^2 + k^2 -
// (k - j)^2) / 2 makes it a convolution (Bluestein) on F >= n + m - 1 points:
//   A[j] = a_abs^-j exp(-2 pi i j a_turns) c(j)              (premultiplier)
//   v[d mod F] = conj(c(d)), -(n-1) <= d <= m-1; Vhat = FFT_F(v) / F
//   X[k] = c(k) IFFT_F(FFT_F(x A, zero-padded) FFT_F(v))[k]  (P[k] = c(k))
//
//   czt_lds_kernel   F = 256 ... 16384: a row times A as it is loaded, FFT_F,
//                    times Vhat on the last pass (YhatEpi), the second FFT_F as
//                    the inverse with the postmultiplier on its last pass
//                    (CztPostEpi), the first m outputs stored, in one workgroup:
//                    n samples read and m outputs written once per row
//   czt_pre_kernel,  the composed form's ends (F = 2^15 ... 2^20, and
//   czt_mul_kernel,  GDSP_ALGO_NO_FUSED_CZT): rows times A padded to F, after
//   czt_post_kernel  the plan's FFT_F the conjugated product with Vhat, and
//                    after the plan's second FFT_F the postmultiply and store
//
// The chirp-z kernels of the FFT planner (fft_kernels.hip bluestein_kernel,
// chirpz6k.hpp) are this with a = 1, step = 1 / n and m = n. Spirals (|w| != 1)
// are not offered: Bluestein's split of |w|^(jk) into |w|^(+-j^2/2) loses the
// result to the convolution's roundoff (include/gdsp_fft.h).
//
// One row per transform, in both forms, as in hilbert.hip: a row's outputs
// depend on that row alone, bit for bit. Two real rows are not packed into one
// transform. The 1/F of the inverse is in Vhat, a power of 2: rows times 2^k
// give outputs times 2^k.
//
// The host part: the tables (every angle reduced exactly in integers before
// any floating-point trigonometry), the plan object and the C entries.
#include <cmath>
#include <memory>
#include <vector>

#include "conv_core.hpp"
#include "fft_device.hpp"
#include "launch.hpp"
#include "plan.hpp"

namespace gdsp {

// Epilogue of the second FFT's last pass: the transform's conjugate (the
// inverse, conv_core.hpp) times the postmultiplier, loaded ahead of the
// butterfly's arithmetic. p: the table (F entries, zero past m) + t.
template <int T>
struct CztPostEpi {
  const cd *p;
  static constexpr bool on = true;
  __device__ static constexpr bool want(int) { return true; }
  __device__ cd load(int k) const { return p[k * T]; }
  template <int E>
  __device__ void apply(cd (&v)[E], int k, cd u, cd f) const { v[k] = cmul(conjg(u), f); }
};

// Whether the postmultiplier rides the second FFT's last pass (CztPostEpi) or
// follows it at the store: at 16384 a thread's 32 elements leave no registers
// for the epilogue's factors (136 spilled with it, 32 without).
__host__ __device__ constexpr bool czt_post_epi(int log2n) { return log2n <= 13; }

// One workgroup holds TPW rows in registers (thread t of a row owns elements
// t + k T), as convolve_lds_kernel does. A, vhat and P have F entries (A zero
// past n, P zero past m) and are shared by every row: read through L2.
template <int LOG2N, int LOG2E, bool REAL>
__global__ __launch_bounds__((Geo<LOG2N, LOG2E>::WG)) void czt_lds_kernel(
    const void *__restrict__ x, int64_t ldx, int64_t rows, int n, int m, cd *__restrict__ out,
    int64_t ldo, const cd *__restrict__ tw, const cd *__restrict__ A,
    const cd *__restrict__ vhat, const cd *__restrict__ P) {
  using G = Geo<LOG2N, LOG2E>;
  constexpr int E = G::E, T = G::T;
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
  double *const lre = lds + slot * G::STRIDE;
  cd v[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int i = t + k * T;
    const cd a = A[i];
    if constexpr (REAL) {
      const double xs = i < n ? ld_nt(reinterpret_cast<const double *>(x) + gl * ldx + i) : 0.0;
      v[k] = i < n ? cd{xs * a.x, xs * a.y} : cd{0.0, 0.0};
    } else {
      const cd xs = i < n ? ld_nt(reinterpret_cast<const cd *>(x) + gl * ldx + i) : cd{0.0, 0.0};
      v[k] = i < n ? cmul(xs, a) : cd{0.0, 0.0};
    }
  }
  const YhatEpi<T> ye{vhat + t};
  fft_regs<LOG2N, true, 1, LOG2E, 0, 0, const cd *, 1, 0, YhatEpi<T>, conv_prew(LOG2N)>(
      v, t, tw, lre, lre, true, ye);
  cd *const dst = out + g * ldo;
  if constexpr (czt_post_epi(LOG2N)) {
    const CztPostEpi<T> pe{P + t};
    fft_regs<LOG2N, true, 1, LOG2E, 0, 0, const cd *, 1, 0, CztPostEpi<T>, conv_prew(LOG2N)>(
        v, t, tw, lre, lre, false, pe);
    if (!valid) return;
    const int to = opaque_int(t);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int i = to + k * T;
      if (i < m) st_nt(&dst[i], v[k]);
    }
  } else {
    fft_regs<LOG2N, true, 1, LOG2E, 0, 0, const cd *, 1, 0, NoEpi, conv_prew(LOG2N)>(
        v, t, tw, lre, lre, false);
    if (!valid) return;
    const int to = opaque_int(t);
    // in fenced runs of 4, as the Hilbert kernel reads its samples again
#pragma unroll
    for (int k0 = 0; k0 < E; k0 += 4) {
      cd p[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = P[to + (k0 + k) * T];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = to + (k0 + k) * T;
        if (i < m) st_nt(&dst[i], cmul(conjg(v[k0 + k]), p[k]));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int LOG2N, bool REAL>
static hipError_t launch_czt_t(const void *x, int64_t ldx, int64_t rows, int64_t n, int64_t m,
                               cd *out, int64_t ldo, const cd *tw, const cd *A, const cd *vhat,
                               const cd *P, hipStream_t s) {
  constexpr int LOG2E = conv_log2e(LOG2N);
  using G = Geo<LOG2N, LOG2E>;
  const int64_t nblk = (rows + G::TPW - 1) / G::TPW;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((czt_lds_kernel<LOG2N, LOG2E, REAL>), dim3((unsigned)nblk), dim3(G::WG), 0,
                     s, x, ldx, rows, (int)n, (int)m, out, ldo, tw, A, vhat, P);
  return hipGetLastError();
}

bool czt_lds_applies(int64_t F) {
  return F >= ((int64_t)1 << kConvMinLog2) && F <= ((int64_t)1 << kMaxLdsLog2) &&
         (F & (F - 1)) == 0;
}

hipError_t launch_czt_lds(int log2f, bool real, const void *x, int64_t ldx, int64_t rows,
                          int64_t n, int64_t m, cd *out, int64_t ldo, const cd *tw, const cd *A,
                          const cd *vhat, const cd *P, hipStream_t s) {
  const int64_t F = (int64_t)1 << log2f;
  if (rows <= 0 || n <= 0 || m <= 0 || n + m - 1 > F || !x || !out || !tw || !A || !vhat || !P ||
      (rows > 1 && (ldx < n || ldo < m)))
    return hipErrorInvalidValue;
  static_assert(kConvMinLog2 == 8 && kMaxLdsLog2 == 14, "the cases below");
#define GDSP_CZT_CASE(L)                                                                      \
  case L:                                                                                     \
    return real ? launch_czt_t<L, true>(x, ldx, rows, n, m, out, ldo, tw, A, vhat, P, s)      \
                : launch_czt_t<L, false>(x, ldx, rows, n, m, out, ldo, tw, A, vhat, P, s)
  switch (log2f) {
    GDSP_CZT_CASE(8);
    GDSP_CZT_CASE(9);
    GDSP_CZT_CASE(10);
    GDSP_CZT_CASE(11);
    GDSP_CZT_CASE(12);
    GDSP_CZT_CASE(13);
    GDSP_CZT_CASE(14);
    default: return hipErrorInvalidValue;
  }
#undef GDSP_CZT_CASE
}

// ---- the composed form --------------------------------------------------------
// buf[r F + i] = x[(r0 + r) ldx + i] A[i] for i < n, else 0
template <bool REAL>
__global__ __launch_bounds__(256) void czt_pre_kernel(const void *__restrict__ x, int64_t ldx,
                                                      int64_t r0, int64_t n, int64_t F,
                                                      const cd *__restrict__ A,
                                                      cd *__restrict__ buf, int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / F, i = e - r * F;
  cd o = {0.0, 0.0};
  if (i < n) {
    const cd a = A[i];
    if constexpr (REAL) {
      const double xs = reinterpret_cast<const double *>(x)[(r0 + r) * ldx + i];
      o = {xs * a.x, xs * a.y};
    } else {
      o = cmul(reinterpret_cast<const cd *>(x)[(r0 + r) * ldx + i], a);
    }
  }
  buf[e] = o;
}

// spec[r F + f] = conj(spec[r F + f] vhat[f]), in place: the next forward
// transform is then the inverse's conjugate
__global__ __launch_bounds__(256) void czt_mul_kernel(cd *spec, const cd *__restrict__ vhat,
                                                      int64_t F, int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  spec[e] = conjg(cmul(spec[e], vhat[e % F]));
}

// out[(r0 + r) ldo + i] = conj(spec[r F + i]) P[i], i < m (count = cnt m)
__global__ __launch_bounds__(256) void czt_post_kernel(const cd *__restrict__ spec, int64_t F,
                                                       int64_t r0, int64_t m,
                                                       const cd *__restrict__ P,
                                                       cd *__restrict__ out, int64_t ldo,
                                                       int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / m, i = e - r * m;
  out[(r0 + r) * ldo + i] = cmul(conjg(spec[r * F + i]), P[i]);
}

static bool czt_grid(int64_t cnt, int64_t len, int64_t *count, unsigned *nblk) {
  if (cnt <= 0 || len <= 0 || cnt > INT64_MAX / len) return false;
  *count = cnt * len;
  const int64_t b = (*count + 255) / 256;
  if (b > 0x7fffffff) return false;
  *nblk = (unsigned)b;
  return true;
}

hipError_t launch_czt_pre(bool real, const void *x, int64_t ldx, int64_t r0, int64_t cnt,
                          int64_t n, int64_t F, const cd *A, cd *buf, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!x || !A || !buf || n <= 0 || n > F || !czt_grid(cnt, F, &count, &nblk))
    return hipErrorInvalidValue;
  if (real)
    hipLaunchKernelGGL(czt_pre_kernel<true>, dim3(nblk), dim3(256), 0, s, x, ldx, r0, n, F, A,
                       buf, count);
  else
    hipLaunchKernelGGL(czt_pre_kernel<false>, dim3(nblk), dim3(256), 0, s, x, ldx, r0, n, F, A,
                       buf, count);
  return hipGetLastError();
}

hipError_t launch_czt_mul(cd *spec, const cd *vhat, int64_t cnt, int64_t F, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!spec || !vhat || !czt_grid(cnt, F, &count, &nblk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(czt_mul_kernel, dim3(nblk), dim3(256), 0, s, spec, vhat, F, count);
  return hipGetLastError();
}

hipError_t launch_czt_post(const cd *spec, int64_t F, int64_t r0, int64_t cnt, int64_t m,
                           const cd *P, cd *out, int64_t ldo, hipStream_t s) {
  int64_t count = 0;
  unsigned nblk = 0;
  if (!spec || !P || !out || m > F || !czt_grid(cnt, m, &count, &nblk))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(czt_post_kernel, dim3(nblk), dim3(256), 0, s, spec, F, r0, m, P, out, ldo,
                     count);
  return hipGetLastError();
}

}  // namespace gdsp

// ---- the host part --------------------------------------------------------------
using gdsp::cd;
using namespace gdsp_api;

namespace {

typedef unsigned __int128 u128;

constexpr long double kTwoPi = 6.283185307179586476925286766559005768L;
// rows of F complex128 in one chunk of the composed form and one range of the
// host entry
constexpr int64_t CZT_CHUNK_ELEMS = (int64_t)1 << 24;
constexpr int64_t kCztMaxF = (int64_t)1 << 20;

long double to_ld(u128 v) {
  return (long double)(uint64_t)(v >> 64) * 18446744073709551616.0L + (long double)(uint64_t)v;
}

int bit_length(u128 v) {
  int b = 0;
  while (v) {
    v >>= 1;
    ++b;
  }
  return b;
}

// mult x / div turns modulo 1, in [-1/2, 1/2], for a finite double x = sig 2^e
// taken exactly, an integer mult < 2^40 and an integer div in [1, 2^64]: the
// product mult sig and the modulus div 2^-e are integers, reduced in 128 bits;
// only the remainder's quotient is rounded (to long double). Where the modulus
// does not fit 127 bits it exceeds every product: the angle is below one turn
// and is left as it is.
struct Turns {
  bool zero = false, direct = false;
  int sign = 1;
  u128 sig = 0, den = 1;
  long double xl = 0.0L;
  Turns(double x, u128 div) {
    if (x == 0.0) {
      zero = true;
      return;
    }
    sign = x < 0 ? -1 : 1;
    int ex = 0;
    const uint64_t s = (uint64_t)ldexp(frexp(fabs(x), &ex), 53);
    const int e = ex - 53;
    if (e >= 0) {  // an integer: sig 2^e mod div first
      u128 p = (u128)1 % div;
      for (int q = 0; q < e; ++q) p = (p * 2) % div;
      sig = ((u128)s % div) * p % div;  // factors below 2^64
      den = div;
    } else if (bit_length(div) - e <= 127) {
      sig = s;
      den = div << -e;
    } else {
      direct = true;
      xl = (long double)fabs(x) / to_ld(div);
    }
  }
  long double at(uint64_t mult) const {
    if (zero || mult == 0) return 0.0L;
    if (direct) return sign * ((long double)mult * xl);
    const u128 r = ((u128)mult * sig) % den;  // mult < 2^40, sig < 2^64
    const u128 c = den - r;
    const long double f = r <= c ? to_ld(r) / to_ld(den) : -(to_ld(c) / to_ld(den));
    return sign * f;
  }
};

bool czt_params_ok(double a_abs, double a_turns, double step_turns, int64_t step_div) {
  return std::isfinite(a_abs) && a_abs > 0.0 && std::isfinite(a_turns) &&
         std::isfinite(step_turns) && step_div >= 1;
}

int64_t czt_length(int64_t n, int64_t m) {
  if (n < 1 || m < 1 || n > kCztMaxF || m > kCztMaxF || n + m - 1 > kCztMaxF) return 0;
  int64_t F = 256;
  while (F < n + m - 1) F <<= 1;
  return F;
}

bool czt_fused_now(int64_t F) {
  return F > 0 && gdsp::czt_lds_applies(F) && !(gdsp::algo_flags() & GDSP_ALGO_NO_FUSED_CZT);
}

// A (n), v (F) and P (m), or GDSP_ERR_INVALID; no message is recorded here
int czt_tables(int64_t n, int64_t m, int64_t F, double a_abs, double a_turns, double step_turns,
               int64_t step_div, cd *A, cd *v, cd *P) {
  if (n < 1 || m < 1 || F < n + m - 1 || F > kCztMaxF || !A || !v || !P ||
      !czt_params_ok(a_abs, a_turns, step_turns, step_div))
    return GDSP_ERR_INVALID;
  const Turns chirp(step_turns, (u128)2 * (u128)(uint64_t)step_div), start(a_turns, 1);
  const int64_t top = n > m ? n : m;
  // c(j) = exp(-2 pi i fc), fc = j^2 step / 2 turns reduced; long double,
  // rounded once where a table takes it
  std::vector<long double> fc((size_t)top);
  for (int64_t j = 0; j < top; ++j) fc[(size_t)j] = chirp.at((uint64_t)j * (uint64_t)j);
  const long double la = (long double)a_abs;
  for (int64_t j = 0; j < n; ++j) {
    const long double mag = a_abs == 1.0 ? 1.0L : powl(la, -(long double)j);
    const long double ang = kTwoPi * (fc[(size_t)j] + start.at((uint64_t)j));
    if (!std::isnormal((double)mag)) return GDSP_ERR_INVALID;
    A[j] = {(double)(mag * cosl(ang)), (double)(-mag * sinl(ang))};
  }
  for (int64_t i = 0; i < F; ++i) v[i] = {0.0, 0.0};
  for (int64_t d = -(n - 1); d < m; ++d) {
    const long double ang = kTwoPi * fc[(size_t)(d < 0 ? -d : d)];
    v[d < 0 ? F + d : d] = {(double)cosl(ang), (double)sinl(ang)};
  }
  for (int64_t k = 0; k < m; ++k) {
    const long double ang = kTwoPi * fc[(size_t)k];
    P[k] = {(double)cosl(ang), (double)(-sinl(ang))};
  }
  return GDSP_OK;
}

// The checks of a plan's parameters that answer before any device call, in
// the header's order; *F: the convolution length.
int czt_shape_check(int64_t n, int64_t m, double a_abs, double a_turns, double step_turns,
                    int64_t step_div, int64_t *F) {
  if (n < 0 || m < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (!czt_params_ok(a_abs, a_turns, step_turns, step_div))
    return fail(GDSP_ERR_INVALID, "a_abs <= 0, a non-finite parameter or step_div < 1");
  if (n == 0 || m == 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  *F = czt_length(n, m);
  if (*F == 0) return fail(GDSP_ERR_UNSUPPORTED, "n + m - 1 above 2^20");
  return GDSP_OK;
}

}  // namespace

struct gdsp_czt_plan {
  int device = 0;
  int64_t n = 0, m = 0, F = 0;
  int log2f = 0;
  const gdsp_plan *fft = nullptr;  // the plan cache's F-point transform: tw, the composed form
  DevPtr<cd> A, vhat, P;           // F entries each; A zero past n, P zero past m
};

namespace {

int czt_plan_build(int64_t n, int64_t m, double a_abs, double a_turns, double step_turns,
                   int64_t step_div, std::unique_ptr<gdsp_czt_plan> &out) {
  int64_t F = 0;
  STCHK(czt_shape_check(n, m, a_abs, a_turns, step_turns, step_div, &F));
  std::vector<cd> A((size_t)F, cd{0.0, 0.0}), v((size_t)F), P((size_t)F, cd{0.0, 0.0});
  if (czt_tables(n, m, F, a_abs, a_turns, step_turns, step_div, A.data(), v.data(), P.data()) !=
      GDSP_OK)
    return fail(GDSP_ERR_INVALID, "a_abs^-(n-1) outside the normal double range");
  std::unique_ptr<gdsp_czt_plan> p(new gdsp_czt_plan());
  STCHK(current_device(&p->device));
  p->n = n;
  p->m = m;
  p->F = F;
  p->log2f = ilog2(F);
  gdsp_plan *fp = nullptr;
  STCHK(get_plan(F, &fp));  // the plan mutex is held in here only
  p->fft = fp;
  STCHK(device_table(p->device, A, p->A));
  STCHK(device_table(p->device, P, p->P));
  // FFT_F(v) on the device with the engine itself, with the inverse's 1/F
  STCHK(plan_spectrum_table(p->device, fp, v, F, 1, 1.0 / (double)F, p->vhat));
  out = std::move(p);
  return GDSP_OK;
}

int64_t czt_chunk_rows(int64_t F, int64_t rows) {
  int64_t r = CZT_CHUNK_ELEMS / F;
  if (r < 1) r = 1;
  return r < rows ? r : rows;
}

// work (NULL: the workspace pool): nothing in the fused form; composed,
// czt_chunk_rows(F, rows) rows of F complex128
int czt_rows(const gdsp_czt_plan *p, const void *d_x, int64_t ldx, bool real, int64_t rows,
             cd *d_out, int64_t ldo, void *work, hipStream_t s) {
  // a power of 2 up to 2^14 is KIND_LDS under every flag set; the kind is
  // checked because the kernel reads that plan's twiddle table
  if (czt_fused_now(p->F) && p->fft->kind == KIND_LDS) {
    HIPCHK(gdsp::launch_czt_lds(p->log2f, real, d_x, ldx, rows, p->n, p->m, d_out, ldo,
                                p->fft->tw, p->A.get(), p->vhat.get(), p->P.get(), s));
    return GDSP_OK;
  }
  const int64_t cr = czt_chunk_rows(p->F, rows);
  DevBuf w;
  if (!work) {
    STCHK(w.alloc((size_t)cr * (size_t)p->F * sizeof(cd), s, SLOT_CZT));
    work = w.p;
  }
  cd *buf = (cd *)work;
  for (int64_t r0 = 0; r0 < rows; r0 += cr) {
    later_chunk(r0);
    const int64_t cnt = rows - r0 < cr ? rows - r0 : cr;
    HIPCHK(gdsp::launch_czt_pre(real, d_x, ldx, r0, cnt, p->n, p->F, p->A.get(), buf, s));
    STCHK(exec_plan(p->fft, buf, buf, cnt, false, gdsp::LOAD_COMPLEX, s));
    HIPCHK(gdsp::launch_czt_mul(buf, p->vhat.get(), cnt, p->F, s));
    STCHK(exec_plan(p->fft, buf, buf, cnt, false, gdsp::LOAD_COMPLEX, s));
    HIPCHK(gdsp::launch_czt_post(buf, p->F, r0, cnt, p->m, p->P.get(), d_out, ldo, s));
  }
  return GDSP_OK;
}

// Argument checks shared by the host and device entries, in the order of the
// header's table; *done: nothing to do. No device call is made.
int czt_check(const void *x, int64_t ldx, int is_real, int64_t rows, int64_t n, int64_t m,
              bool params_ok, const void *out, int64_t ldo, bool *done) {
  *done = false;
  if (rows < 0 || n < 0 || m < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (is_real != 0 && is_real != 1) return fail(GDSP_ERR_INVALID, "is_real must be 0 or 1");
  if (rows > 1 && (ldx < n || ldo < m))
    return fail(GDSP_ERR_INVALID, "row stride below the row length");
  if (!params_ok)
    return fail(GDSP_ERR_INVALID, "a_abs <= 0, a non-finite parameter or step_div < 1");
  if (rows == 0) {
    *done = true;
    return GDSP_OK;
  }
  if (n == 0 || m == 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  if (!x || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  return GDSP_OK;
}

}  // namespace

int gdsp_czt_tables(int64_t n, int64_t m, int64_t F, double a_abs, double a_turns,
                    double step_turns, int64_t step_div, double *A, double *v, double *P) {
  if (czt_tables(n, m, F, a_abs, a_turns, step_turns, step_div, (cd *)A, (cd *)v, (cd *)P) !=
      GDSP_OK)
    return fail(GDSP_ERR_INVALID, "czt tables: a size, a parameter or a_abs^-(n-1) out of range");
  return GDSP_OK;
}

int64_t gdsp_czt_length(int64_t n, int64_t m, int *fused) {
  const int64_t F = czt_length(n, m);
  if (fused) *fused = czt_fused_now(F) ? 1 : 0;
  return F;
}

int gdsp_czt_fused(int64_t n, int64_t m) { return czt_fused_now(czt_length(n, m)) ? 1 : 0; }

int gdsp_czt_plan_create(int64_t n, int64_t m, double a_abs, double a_turns, double step_turns,
                         int64_t step_div, gdsp_czt_plan **plan) {
  if (!plan) return fail(GDSP_ERR_INVALID, "NULL plan pointer");
  *plan = nullptr;
  std::unique_ptr<gdsp_czt_plan> p;
  STCHK(czt_plan_build(n, m, a_abs, a_turns, step_turns, step_div, p));
  *plan = p.release();
  return GDSP_OK;
}

int gdsp_czt_plan_destroy(gdsp_czt_plan *plan) {
  delete plan;  // hipFree waits for the device: nothing queued reads a freed table
  return GDSP_OK;
}

int gdsp_czt_plan_info(const gdsp_czt_plan *plan, int64_t *n, int64_t *m, int64_t *F,
                       int *fused) {
  if (!plan) return fail(GDSP_ERR_INVALID, "NULL plan");
  if (n) *n = plan->n;
  if (m) *m = plan->m;
  if (F) *F = plan->F;
  if (fused) *fused = czt_fused_now(plan->F) ? 1 : 0;
  return GDSP_OK;
}

int64_t gdsp_czt_work_bytes(const gdsp_czt_plan *plan, int64_t rows) {
  if (!plan || rows <= 0 || czt_fused_now(plan->F)) return 0;
  return czt_chunk_rows(plan->F, rows) * plan->F * (int64_t)sizeof(cd);
}

int gdsp_czt_batch_device(const gdsp_czt_plan *plan, const void *d_x, int64_t ldx, int is_real,
                          int64_t rows, void *d_out, int64_t ldo, void *d_work,
                          int64_t work_bytes, void *stream) {
  if (!plan) return fail(GDSP_ERR_INVALID, "NULL plan");
  bool done = false;
  STCHK(czt_check(d_x, ldx, is_real, rows, plan->n, plan->m, true, d_out, ldo, &done));
  if (done) return GDSP_OK;
  if (rows == 1) ldx = plan->n, ldo = plan->m;
  // other workgroups store while a row is still to be read
  const uintptr_t esz = is_real ? sizeof(double) : sizeof(cd);
  const uintptr_t xa = (uintptr_t)d_x, oa = (uintptr_t)d_out;
  const uintptr_t xe = xa + ((uintptr_t)(rows - 1) * (uintptr_t)ldx + (uintptr_t)plan->n) * esz;
  const uintptr_t oe =
      oa + ((uintptr_t)(rows - 1) * (uintptr_t)ldo + (uintptr_t)plan->m) * sizeof(cd);
  if (xa < oe && oa < xe) return fail(GDSP_ERR_INVALID, "d_out overlaps d_x");
  if (d_work && work_bytes < gdsp_czt_work_bytes(plan, rows))
    return fail(GDSP_ERR_INVALID, "work buffer below gdsp_czt_work_bytes");
  int dev = 0;
  STCHK(current_device(&dev));
  if (dev != plan->device) return fail(GDSP_ERR_INVALID, "the plan belongs to another device");
  return czt_rows(plan, d_x, ldx, is_real != 0, rows, (cd *)d_out, ldo, d_work,
                  (hipStream_t)stream);
}

int gdsp_czt_batch(const void *x, int64_t ldx, int is_real, int64_t rows, int64_t n, int64_t m,
                   double a_abs, double a_turns, double step_turns, int64_t step_div, double *out,
                   int64_t ldo) {
  bool done = false;
  STCHK(czt_check(x, ldx, is_real, rows, n, m,
                  czt_params_ok(a_abs, a_turns, step_turns, step_div), out, ldo, &done));
  if (done) return GDSP_OK;
  std::unique_ptr<gdsp_czt_plan> p;
  STCHK(czt_plan_build(n, m, a_abs, a_turns, step_turns, step_div, p));
  hipStream_t s = thread_stream(p->device);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const int64_t xd = is_real ? 1 : 2;  // doubles per input element
  if (rows == 1) ldx = n, ldo = m;
  int64_t rng = CZT_CHUNK_ELEMS / p->F;
  if (rng < 1) rng = 1;
  const double *hx = (const double *)x;
  DevBuf dx, dout;
  for (int64_t r0 = 0; r0 < rows; r0 += rng) {
    later_chunk(r0);
    const int64_t cnt = rows - r0 < rng ? rows - r0 : rng;
    STCHK(dx.alloc((size_t)cnt * (size_t)(n * xd) * sizeof(double), s, SLOT_IN));
    STCHK(dout.alloc((size_t)cnt * (size_t)m * sizeof(cd), s, SLOT_CZT_OUT));
    double *px = (double *)dx.p;
    cd *po = (cd *)dout.p;
    STCHK(run_queued(s, [&]() -> int {
      STCHK(stage_rows(px, hx + r0 * ldx * xd, cnt, n * xd, ldx * xd, n * xd, s));
      return czt_rows(p.get(), px, n, is_real != 0, cnt, po, m, nullptr, s);
    }));
    // returns after the stream drained: the next range may reuse the buffers
    STCHK(unstage_rows(out + r0 * ldo * 2, (const double *)po, cnt, m * 2, ldo * 2, s));
  }
  return GDSP_OK;
}
