// plan.hip — the FFT planner: which algorithm a length takes (build_plan and
// its split finders), the device tables of a plan, the plan-time races, and
// the plan cache. The executors it calls back into are in gdsp_api.hip.
#include "plan.hpp"

#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <tuple>

using gdsp::cd;
using namespace gdsp_api;

namespace {

// recursive: building a Bluestein plan runs FFT_M(b), whose four-step path
// fetches sub-plans from this cache on the same thread
std::recursive_mutex g_plan_mu;
// keyed by (device, n, algorithm flags the plan was built under)
std::map<std::tuple<int, int64_t, unsigned>, gdsp_plan *> g_plans;
std::map<std::tuple<int, int64_t, unsigned>, gdsp_plan *> g_chirpz_plans;  // forced Bluestein

// The algorithm flags a plan is built under: read once by the outermost
// get_plan_locked of a thread (the cache key) and used by every decision of
// that build and of the sub-plans it fetches, so a concurrent
// gdsp_set_algorithm cannot leave a plan built under mixed flags in the
// cache (plans are built under g_plan_mu; the snapshot is per thread).
thread_local int t_build_depth = 0;
thread_local unsigned t_build_flags = 0;
unsigned plan_flags() { return gdsp::algo_flags(); }

int get_plan_locked(int dev, int64_t n, gdsp_plan **out, bool chirpz = false);

// count elements of h as a complete device table (plans are shared by every
// stream and thread). The stream is drained on a failure too: no queued copy
// may still write the table when it is freed.
template <class T>
int upload(int dev, const T *h, size_t count, DevPtr<T> &out) {
  T *d = nullptr;
  HIPCHK(hipMalloc((void **)&d, count * sizeof(T)));
  DevPtr<T> t(d);
  hipStream_t s = thread_stream(dev);
  const int st = copy_h2d(d, h, count * sizeof(T), s);
  const hipError_t e = hipStreamSynchronize(s);
  STCHK(st);
  if (e != hipSuccess) return fail(GDSP_ERR_HIP, hipGetErrorString(e));
  out = std::move(t);
  return GDSP_OK;
}

// p->tw = T_n[k] = exp(-2 pi i k/n), evaluated in long double and rounded once.
int upload_twiddles(int dev, int64_t n, gdsp_plan *p) {
  std::vector<cd> h((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    long double a = -2.0L * 3.141592653589793238462643383279502884L * (long double)k /
                    (long double)n;
    h[(size_t)k].x = (double)cosl(a);
    h[(size_t)k].y = (double)sinl(a);
  }
  DevPtr<cd> tw;
  STCHK(upload(dev, h.data(), h.size(), tw));
  p->tw = p->own(std::move(tw));
  return GDSP_OK;
}

// Radices of the mixed-radix kernel for n (fft_mixed.hip), or false when n is
// a power of 2, too long, or has a prime factor above 13 (-> Bluestein).
bool mixed_radices(int64_t n, std::vector<int> &rad, bool specs = true) {
  rad.clear();
  if (n < 2 || n > gdsp::kMixedSpecMax || is_pow2(n)) return false;
  if (n > gdsp::kMixedMax) {  // beyond the runtime-radix kernel: specialisations only
    int fr[16], fnp = 0;
    if (!specs || !gdsp::mixed_fixed_radices((int)n, fr, &fnp)) return false;
    rad.assign(fr, fr + fnp);
    return true;
  }
  int64_t m = n;
  int a = 0;
  while (m % 2 == 0) {
    m /= 2;
    ++a;
  }
  std::vector<int> odd;
  for (int q : {13, 11, 7, 5, 3})
    while (m % q == 0) {
      m /= q;
      odd.push_back(q);
    }
  if (m != 1) return false;
  int fr[16], fnp = 0;
  if (specs && gdsp::mixed_fixed_radices((int)n, fr, &fnp)) {
    rad.assign(fr, fr + fnp);
    return true;
  }
  while (a >= 4) {
    rad.push_back(16);
    a -= 4;
  }
  if (a) rad.push_back(1 << a);
  rad.insert(rad.end(), odd.begin(), odd.end());
  return rad.size() <= 12;
}

// Descriptor + per-pass twiddle bases W_{Ns*R}^k (k < Ns; the kernels
// raise them to the powers r = 1..R-1 in registers) of one radix list.
// geometry: check the thread count of the mixed-radix kernels' geometry (the
// fused chirp-z kernels, which only take the twiddle bases, have their own)
int make_mixed_desc(int dev, int64_t n, const std::vector<int> &rad, gdsp::MixedDesc &d,
                    DevPtr<cd> &tw, bool geometry = true) {
  d.n = (int)n;
  d.npass = (int)rad.size();
  d.codes = 0;
  int need = 1;
  for (size_t q = 0; q < rad.size(); ++q) {
    d.codes |= (uint64_t)rad[q] << (5 * q);
    const int jmax = rad[q] > 16 ? 1 : 16 / rad[q], nb = (int)n / rad[q];
    need = std::max(need, (nb + jmax - 1) / jmax);
  }
  int t1 = 1;
  while (t1 < need) t1 <<= 1;
  if (t1 > 64) t1 = (need + 63) / 64 * 64;
  // (the runtime-radix kernels check t1 <= 512 themselves; a compiled or
  // runtime-compiled specialisation may use up to 1024 threads per transform)
  if (geometry && t1 > 1024) return fail(GDSP_ERR_UNSUPPORTED, "mixed-radix geometry");
  d.t1 = t1;
  d.tpw = std::max(1, std::min(256 / t1, gdsp::kMixedMax / (int)n));
  std::vector<cd> h;
  int64_t ns = rad[0];
  for (size_t q = 1; q < rad.size(); ++q) {
    const int R = rad[q];
    for (int64_t k = 0; k < ns; ++k) {
      const long double ang = -2.0L * 3.141592653589793238462643383279502884L * (long double)k /
                              (long double)(ns * R);
      h.push_back({(double)cosl(ang), (double)sinl(ang)});
    }
    ns *= R;
  }
  if (h.empty()) h.push_back({1.0, 0.0});
  return upload(dev, h.data(), h.size(), tw);
}

int build_mixed(int dev, int64_t n, const std::vector<int> &rad, gdsp_plan *p) {
  p->kind = KIND_MIXED;
  DevPtr<cd> tw;
  STCHK(make_mixed_desc(dev, n, rad, p->md, tw));
  p->tw = p->own(std::move(tw));
  {
    int pr[16], pnp = 0;
    if (gdsp::pwelch_fixed_radices((int)n, pr, &pnp)) {
      STCHK(make_mixed_desc(dev, n, std::vector<int>(pr, pr + pnp), p->md_pw, tw));
      p->tw_pw = p->own(std::move(tw));
    }
  }
  // the runtime-radix kernels (fused Pwelch) take the generic list: radices
  // <= 16, no composites (a compiled specialisation's list may hold them)
  std::vector<int> gen;
  if (!mixed_radices(n, gen, false)) {
    p->md_gen = gdsp::MixedDesc{};  // no runtime-radix list (n > kMixedMax)
    return GDSP_OK;
  }
  if (gen == rad) {
    p->md_gen = p->md;
    p->tw_gen = p->tw;
    return GDSP_OK;
  }
  STCHK(make_mixed_desc(dev, n, gen, p->md_gen, tw));
  p->tw_gen = p->own(std::move(tw));
  return GDSP_OK;
}

// Output parts of the split chirp-z for n (see gdsp_plan::parts): the fewest
// P <= 8 with n + ceil(n/P) - 1 <= 16384 where NextPowerOf2(2n-1) exceeds
// one kernel, else 0 (composed chirp-z). P = 8 (n <= 14563) measured 10.8
// against 11.5 ms for the composed chirp-z per 2^27 samples, P = 2 4x faster.
int chirpz_parts(int64_t n) {
  const bool off = (plan_flags() & GDSP_ALGO_NO_CHIRPZ_PARTS) != 0;
  const int64_t mk = (int64_t)1 << gdsp::kMaxLdsLog2;
  if (off || next_pow2_ref(2 * n - 1) <= mk) return 0;
  for (int parts = 2; parts <= 8; ++parts)
    if (n + (n + parts - 1) / parts - 1 <= mk) return parts;
  return 0;
}

// Lengths one kernel transforms per row: powers of 2 up to the LDS limit,
// the mixed-radix set, and every other m <= 8192 through the fused chirp-z
// kernel (M = NextPowerOf2(2m - 1) <= 16384), so a length with a large prime
// factor but a smooth cofactor (8191 * 64) still gets a three-pass four-step
// instead of the composed chirp-z over 2n-point rows.
bool one_kernel_len(int64_t m) {
  if (m < 2) return false;
  if (chirpz_parts(m)) {
    // only a prime builds as the output-split chirp-z plan: a composite in
    // (8192, 14563] has a four-step split, which build_plan takes first
    bool prime = true;
    for (int64_t d = 2; d * d <= m && prime; ++d) prime = m % d != 0;
    if (prime) return true;
  }
  if (is_pow2(m)) return ilog2(m) <= gdsp::kMaxLdsLog2;
  std::vector<int> rad;
  if (mixed_radices(m, rad)) return true;
  int jr[5], jnp = 0;  // a runtime-compiled specialisation
  if (gdsp::jit_enabled() && gdsp::jit_radices((int)m, jr, &jnp)) return true;
  return next_pow2_ref(2 * m - 1) <= ((int64_t)1 << gdsp::kMaxLdsLog2);
}

// n = n1 * n2 with both factors one-kernel lengths, n1 <= n2 as balanced as
// possible (fewest, shortest transposes); false if none exists.
bool mixed4_split(int64_t n, int64_t &n1, int64_t &n2) {
  for (int64_t d = (int64_t)sqrtl((long double)n); d >= 2; --d) {
    if (n % d == 0 && one_kernel_len(d) && one_kernel_len(n / d)) {
      n1 = d;
      n2 = n / d;
      return true;
    }
  }
  return false;
}

// n = R * C with R a power of 2 in [16, 512] (column tiles) and C a
// one-kernel length; the largest such R (shortest rows) wins.
bool pow2col_split(int64_t n, int64_t &r, int64_t &c) {
  for (int64_t R = (int64_t)1 << gdsp::kColMaxLog2; R >= ((int64_t)1 << gdsp::kColMinLog2);
       R >>= 1) {
    if (n % R == 0 && one_kernel_len(n / R)) {
      r = R;
      c = n / R;
      return true;
    }
  }
  return false;
}

// n = L * C with L a single radix (<= 25, largest first) and C a one-kernel
// length.
bool radixcol_split(int64_t n, int64_t &l, int64_t &c) {
  for (int L : {25, 20, 16, 15, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2}) {
    if (gdsp::colradix_supported(L) && n % L == 0 && one_kernel_len(n / L)) {
      l = L;
      c = n / L;
      return true;
    }
  }
  return false;
}

// the runtime-compiled column pass for the column length L of n = L * (n / L)
bool mixcol_try(int dev, int64_t n, int64_t L, gdsp_plan *p) {
  if (!gdsp::jit_enabled() || n % L || L < 26 || L > 1016 || is_pow2(L) || !one_kernel_len(L))
    return false;
  gdsp_plan *p1 = nullptr;
  if (get_plan_locked(dev, L, &p1) != GDSP_OK || p1->kind != KIND_MIXED) return false;
  int rad[16], np = p1->md.npass;
  if (np < 2 || np > 16) return false;
  for (int q = 0; q < np; ++q) rad[q] = (int)((p1->md.codes >> (5 * q)) & 31);
  gdsp::JitCol *col = gdsp::jit_col_build(dev, rad, np);
  if (!col) return false;
  p->mixcol = col;
  p->n1 = L;
  p->n2 = n / L;
  p->p1 = p1;
  return true;
}

// n = L * C with L in [26, 1016] a smooth non-power-of-2 length (the
// column pass, colfixed_kernel compiled for L's radix list) and C a
// one-kernel length; the smallest such L (widest column tiles) whose column
// kernel builds wins.
bool mixcol_build(int dev, int64_t n, gdsp_plan *p) {
  if (!gdsp::jit_enabled()) return false;
  for (int64_t L = 26; L <= 1016; ++L) {
    if (n % L || is_pow2(L) || !one_kernel_len(n / L) || !one_kernel_len(L)) continue;
    if (mixcol_try(dev, n, L, p)) return true;
  }
  return false;
}

// n = L * 2^k, 2^k in [16, 1024], with a column pass for L (one radix <= 25:
// colradix_kernel; 26 <= L <= 1016 smooth: the runtime-compiled
// colfixed_kernel): two HBM passes, the columns and then the rows of 2^k
// with the transpose in their store (rowfft_t_kernel), instead of three.
// Rows of 256 first (256-B output segments), then shorter ones (longer
// segments, longer columns), then 512 and 1024.
bool pow2rows_build(int dev, int64_t n, gdsp_plan *p) {
  for (int k : {8, 7, 6, 5, 4, 9, 10}) {
    const int64_t C = (int64_t)1 << k;
    if (n % C) continue;
    const int64_t L = n / C;
    if (L < 2 || is_pow2(L)) continue;
    if (L <= 25 && gdsp::colradix_supported((int)L)) {
      p->radixcol = true;
      p->n1 = L;
      p->n2 = C;
    } else if (!mixcol_try(dev, n, L, p)) {
      continue;
    }
    p->rowst = true;
    return true;
  }
  return false;
}

// n = L * C with C <= 1024 a smooth one-kernel length (not a power of 2; its
// rows by the runtime-compiled rowt_fixed_kernel, the transpose in their
// store) and a column pass for L (a power of 2 in [16, 512], one radix <= 25
// or a runtime-compiled column length in [26, 1016]): two HBM passes where
// pow2rows_build finds no power-of-2 row length (10^6 = 1000 x 1000, 44100).
// Rows of 1000 (10 x 10 x 10) first where the columns are >= 64 points long,
// then the split closest to C = sqrt(n): per 2^27 samples (profiles/r04/
// mixed4_rows_ab.txt) 10^6, 600000, 200000, 100000, 50000 took 1.6-2.0 ms
// on rows of 1000 but up to 3.1 on the balanced split, while 44100 took
// 1.93-2.03 ms at C = 225 / 210 and 2.42 at 630 (2.34 in three passes), and
// 30000 1.78 at C = 150 and 2.50 at 1000.
bool mixrows_build(int dev, int64_t n, gdsp_plan *p) {
  if (!gdsp::jit_enabled()) return false;
  std::vector<int64_t> cands;
  for (int64_t C = 16; C <= 1024; ++C)
    if (n % C == 0 && !is_pow2(C)) cands.push_back(C);
  const long double r = sqrtl((long double)n);
  // the rows-of-1000 preference holds only where its columns are >= 64
  // points; every other candidate (short columns included: the single-radix
  // colradix_kernel takes L <= 25) is ordered by its distance from sqrt(n)
  auto pref = [n](int64_t c) { return c == 1000 && n / c >= 64; };
  std::stable_sort(cands.begin(), cands.end(), [r, pref](int64_t a, int64_t b) {
    if (pref(a) != pref(b)) return pref(a);
    return fabsl((long double)a - r) < fabsl((long double)b - r);
  });
  for (const int64_t C : cands) {
    if (!one_kernel_len(C)) continue;
    const int64_t L = n / C;
    const bool p2col = is_pow2(L) && L >= 16 && L <= 512;
    const bool rcol = !is_pow2(L) && L <= 25 && gdsp::colradix_supported((int)L);
    const bool mcol = !is_pow2(L) && L >= 26 && L <= 1016 && one_kernel_len(L);
    if (!p2col && !rcol && !mcol) continue;
    gdsp_plan *pc = nullptr;
    if (get_plan_locked(dev, C, &pc) != GDSP_OK || pc->kind != KIND_MIXED) continue;
    int rad[16], np = pc->md.npass;
    if (np < 1 || np > 16) continue;
    for (int q = 0; q < np; ++q) rad[q] = (int)((pc->md.codes >> (5 * q)) & 31);
    // the column pass's parts (p1, mixcol) into a local, given to p once the
    // rows' kernel is built too: a candidate that fails leaves p untouched
    gdsp_plan col;
    if (p2col) {
      if (get_plan_locked(dev, L, &col.p1) != GDSP_OK) continue;
    } else if (!rcol && !mixcol_try(dev, n, L, &col)) {
      continue;
    }
    gdsp::JitRowT *rt = gdsp::jit_rowt_build(dev, rad, np);
    if (!rt) continue;  // (a built column kernel stays cached in the JIT module list)
    p->pow2col = p2col;
    p->radixcol = rcol;
    p->mixcol = col.mixcol;
    p->p1 = col.p1;
    p->n1 = L;
    p->n2 = C;
    p->rowt = rt;
    p->rowst = true;
    return true;
  }
  return false;
}

bool is_prime64(int64_t n) {
  if (n < 2) return false;
  for (int64_t d = 2; d * d <= n; ++d)
    if (n % d == 0) return false;
  return true;
}

int64_t pow_mod(int64_t b, int64_t e, int64_t m) {
  int64_t r = 1 % m;
  b %= m;
  for (; e > 0; e >>= 1) {
    if (e & 1) r = r * b % m;
    b = b * b % m;
  }
  return r;
}

// smallest primitive root of the prime p
int64_t primitive_root(int64_t p) {
  std::vector<int64_t> f;
  int64_t m = p - 1;
  for (int64_t d = 2; d * d <= m; ++d)
    if (m % d == 0) {
      f.push_back(d);
      while (m % d == 0) m /= d;
    }
  if (m > 1) f.push_back(m);
  for (int64_t g = 2; g < p; ++g) {
    bool ok = true;
    for (int64_t q : f) ok = ok && pow_mod(g, (p - 1) / q, p) != 1;
    if (ok) return g;
  }
  return 0;
}

// Radix list of Rader's convolution length N = P - 1: the compiled
// specialisation's list where there is one, else the runtime-compiled
// choice (jit_radices); a power of 2 as radix-16 passes with the remainder
// last (FPass runs any radix dft_any has).
bool rader_radices(int64_t N, std::vector<int> &rad) {
  rad.clear();
  if (N < 2 || N > gdsp::kMixedSpecMax) return false;
  // (N = 3000: the specialisation's 25 15 8, 1.66 ms per 65 536 x 3001;
  // 8 15 25, 20 15 10, 10 10 3 10, 12 10 25 and 15 10 20 took 2.2-3.8 ms,
  // profiles/r05/rader_radix_ab.txt; the fused Pwelch's own four-pass lists
  // are slower here too: 3001 on 15 5 5 8 1.41-1.42 against 1.30-1.31 ms per
  // 2^27 samples, 4001 on 10 10 10 4 1.63 against 1.40-1.41,
  // scripts/archive/gpu_r05_raderpw.sh)
  if (is_pow2(N)) {
    int a = ilog2(N);
    while (a >= 4) {
      rad.push_back(16);
      a -= 4;
    }
    if (a) rad.push_back(1 << a);
    return true;
  }
  int fr[16], fnp = 0;
  if (gdsp::mixed_fixed_radices((int)N, fr, &fnp) || gdsp::jit_radices((int)N, fr, &fnp)) {
    rad.assign(fr, fr + fnp);
    return true;
  }
  return false;
}

// The spectrum of a convolution kernel as a device table: FFT_len of each of
// the `count` rows of the host vector b, times scale (the convolution's
// inverse FFT's 1/len), computed on the device by the engine itself (the
// plan `fft` for len). The stream is drained before this returns, so the
// table is complete and, on a failure, nothing queued reads what is freed.
int spectrum_table(int dev, const gdsp_plan *fft, const std::vector<cd> &b, int64_t len,
                   int64_t count, double scale, DevPtr<cd> &out) {
  hipStream_t s = thread_stream(dev);
  const size_t nb = (size_t)len * (size_t)count;
  DevPtr<cd> db, bh;
  STCHK(upload(dev, b.data(), nb, db));
  cd *d = nullptr;
  HIPCHK(hipMalloc((void **)&d, nb * sizeof(cd)));
  bh.reset(d);
  int st = exec_plan(fft, db.get(), d, count, false, gdsp::LOAD_COMPLEX, s);
  hipError_t e = st == GDSP_OK ? gdsp::launch_scale(d, (int64_t)nb, scale, s) : hipSuccess;
  const hipError_t es = hipStreamSynchronize(s);
  if (e == hipSuccess) e = es;
  STCHK(st);
  if (e != hipSuccess) return fail(GDSP_ERR_HIP, hipGetErrorString(e));
  out = std::move(bh);
  return GDSP_OK;
}

// Rader's algorithm (rader_fixed_kernel, mixed_fixed.hpp) for a prime n >= 17
// whose n - 1 has a radix list: the DFT as a cyclic convolution of length
// n - 1 (two FFTs of n - 1 points in one kernel) instead of bluestein.go:68-94's
// chirp-z (FFTs of NextPowerOf2(2n - 1), or of a smaller smooth M, chirpz6k.hip).
// *built = false (and p untouched) where it does not apply or the kernel
// does not compile: the plan then takes the chirp-z below.
int rader_try(int dev, int64_t n, gdsp_plan *p, bool *built) {
  *built = false;
  if ((plan_flags() & GDSP_ALGO_NO_RADER) || !gdsp::jit_enabled() || n < 17 ||
      n > gdsp::kMixedSpecMax + 1 || !is_prime64(n))
    return GDSP_OK;
  const int64_t N = n - 1;
  std::vector<int> rad;
  if (!rader_radices(N, rad)) return GDSP_OK;
  // a radix-29 or -31 pass (dft_odd's long constant tables) costs more than
  // the chirp-z it would replace: 2729 (2728 = 8 11 31) 1.82 against 1.74 ms
  // per 2^27 samples (profiles/r05/rader_sweep.jsonl)
  for (int r : rad)
    if (r > 25) return GDSP_OK;
  // nor does a list needing more than 640 threads per transform (the largest
  // pass count over the butterflies a thread takes, as FixedGeo): 8191 (8190
  // = 15 13 7 6, 683 threads) 2.10-2.12 against 2.03-2.04 ms per 2^27
  // samples, 8009 (8008 = 13 11 7 8, 728 threads) ties (2.03-2.06 against
  // 2.08-2.17); 6007 (6006 = 13 11 7 6, 546 threads) gains 7 %
  {
    int t1 = 1;
    for (int r : rad) {
      const int64_t nb = N / r, jm = r > 16 ? 1 : 16 / r, need = (nb + jm - 1) / jm;
      if (need > t1) t1 = (int)need;
    }
    if (t1 > 640) return GDSP_OK;
  }
  gdsp::JitRader *j = gdsp::jit_rader_build(dev, rad.data(), (int)rad.size());
  if (!j) return GDSP_OK;
  gdsp_plan *pn = nullptr;  // FFT_N for bhat
  STCHK(get_plan_locked(dev, N, &pn));
  const int64_t g = primitive_root(n);
  if (!g) return fail(GDSP_ERR_INVALID, "no primitive root");
  std::vector<int> gp((size_t)N), gi((size_t)N);
  int64_t x = 1;
  for (int64_t q = 0; q < N; ++q) {
    gp[(size_t)q] = (int)x;
    x = x * g % n;
  }
  for (int64_t r = 0; r < N; ++r) gi[(size_t)r] = gp[(size_t)((N - r) % N)];
  // b[q] = W_n^ginv[q], the exponent reduced exactly, in long double
  std::vector<cd> b((size_t)N);
  for (int64_t q = 0; q < N; ++q) {
    const long double a =
        -2.0L * 3.141592653589793238462643383279502884L * (long double)gi[(size_t)q] / (long double)n;
    b[(size_t)q] = {(double)cosl(a), (double)sinl(a)};
  }
  // The tables are built into locals and given to p only when every step
  // succeeded; a failure frees them and leaves p untouched.
  gdsp::MixedDesc d{};
  DevPtr<cd> tw, bh;
  DevPtr<int> dgp, dgi;
  STCHK(make_mixed_desc(dev, N, rad, d, tw));
  STCHK(upload(dev, gp.data(), (size_t)N, dgp));
  STCHK(upload(dev, gi.data(), (size_t)N, dgi));
  // FFT_N(b) on the device with the engine itself, with the inverse's 1/N
  STCHK(spectrum_table(dev, pn, b, N, 1, 1.0 / (double)N, bh));
  p->kind = KIND_RADER;
  p->rader = j;
  p->tw = p->own(std::move(tw));
  p->md = d;
  p->m = N;
  p->gpow = p->own(std::move(dgp));
  p->ginv = p->own(std::move(dgi));
  p->bhat = p->own(std::move(bh));
  *built = true;
  return GDSP_OK;
}

// Plan-time race of two ways to run a batched transform of n, where the cost
// model cannot rank them (the prime-factor Rader kernel against the chirp-z
// plan it would replace; the smooth-L chirp-z against the power-of-2 one):
// ~2^23 samples of synthetic rows, each candidate launched three times,
// alternating, on the building thread's stream; true (a wins): a's fastest
// launch < margin x b's. Plans are built once per (device, n, flags), so this
// costs a few milliseconds once. GDSP_ALGO_NO_RACE skips the race: a wins
// (the model's candidate).
// A race never fails a plan. A candidate whose runner returns an error loses
// to the other; where the machinery around them fails (the scratch, the
// events, the fill, the elapsed time) a wins, as without a race. Either way
// the thread's last HIP error is cleared, so that no later check picks it up.
// The stream is drained before this returns: the loser's tables may be freed.
using Runner = std::function<int(const cd *in, cd *out, int64_t batch, hipStream_t s)>;
bool race(int dev, int64_t n, const Runner &a, const Runner &b, double margin) {
  if (plan_flags() & GDSP_ALGO_NO_RACE) return true;
  hipStream_t s = thread_stream(dev);
  const int64_t batch = std::max<int64_t>(1, ((int64_t)1 << 23) / n);
  const size_t bytes = (size_t)batch * (size_t)n * sizeof(cd);
  cd *in = nullptr, *out = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool ok = hipMalloc((void **)&in, bytes) == hipSuccess;
  DevPtr<cd> in_owner(in);
  ok = ok && hipMalloc((void **)&out, bytes) == hipSuccess;
  DevPtr<cd> out_owner(out);
  ok = ok && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess &&
       gdsp::launch_fill_uniform(reinterpret_cast<double *>(in), 2 * batch * n, 0x5EED, 0, s) ==
           hipSuccess;
  float best[2] = {1e30f, 1e30f};
  const Runner *run[2] = {&a, &b};
  int failed = -1;  // the candidate whose runner returned an error
  for (int c = 0; c < 2 && ok && failed < 0; ++c)  // warm-up
    if ((*run[c])(in, out, batch, s) != GDSP_OK) failed = c;
  for (int it = 0; it < 3; ++it)
    for (int c = 0; c < 2 && ok && failed < 0; ++c) {
      float ms = 0.0f;
      ok = hipEventRecord(e0, s) == hipSuccess;
      if (ok && (*run[c])(in, out, batch, s) != GDSP_OK) failed = c;
      ok = ok && failed < 0 && hipEventRecord(e1, s) == hipSuccess &&
           hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
      if (ok) best[c] = std::min(best[c], ms);
    }
  (void)hipStreamSynchronize(s);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (failed >= 0 || !ok) {
    (void)hipGetLastError();
    return failed != 0;
  }
  return best[0] < margin * best[1];
}

// skip: the kinds a plan built as a race's alternative leaves out
enum { SKIP_RADER = 1, SKIP_PFA = 2 };
int build_plan(int dev, int64_t n, gdsp_plan *p, bool chirpz = false, int skip = 0);

// The candidate `mine` for n against the plan n gets without the kinds in
// skip, timed (race): the candidate stays where it is 3 % faster (near a tie
// the alternative, the reference's algorithm, is kept), where there is no
// alternative to race, and under GDSP_ALGO_NO_RACE: nullptr. Otherwise the
// alternative plan, tables and all, for the caller to move into its own.
std::unique_ptr<gdsp_plan> race_alternative(int dev, int64_t n, int skip, const Runner &mine) {
  if (plan_flags() & GDSP_ALGO_NO_RACE) return nullptr;
  auto alt = std::make_unique<gdsp_plan>();
  if (build_plan(dev, n, alt.get(), false, skip) != GDSP_OK) {
    (void)hipStreamSynchronize(thread_stream(dev));  // nothing queued reads its tables
    return nullptr;
  }
  Runner other = [&](const cd *in, cd *out, int64_t batch, hipStream_t s) -> int {
    return exec_plan(alt.get(), in, out, batch, false, gdsp::LOAD_COMPLEX, s);
  };
  if (race(dev, n, mine, other, 0.97)) return nullptr;
  return alt;
}

// Rader's plan for a prime n (kind 7, built by rader_try) against the chirp-z
// plan n gets without it, timed (race): kept where it is 3 % faster,
// otherwise p becomes that plan. Round 5 measured Rader 1.1-2.2x faster on a
// sample of primes (profiles/r05/rader_sweep.jsonl); the race covers the
// lists it did not sample (a radix-17/19/23 pass in n - 1's list: the
// round-6 kind-8 calibration lost on those, profiles/r06/pfa_calib.jsonl).
void rader_race(int dev, int64_t n, gdsp_plan *p) {
  Runner rader = [&](const cd *in, cd *out, int64_t batch, hipStream_t s) -> int {
    return exec_plan(p, in, out, batch, false, gdsp::LOAD_COMPLEX, s);
  };
  if (auto alt = race_alternative(dev, n, SKIP_RADER | SKIP_PFA, rader)) *p = std::move(*alt);
}

// A composite n <= 8192 whose largest prime factor P > 31 has a Rader plan
// and whose cofactor M = n / P (gcd(M, P) = 1) has an in-register DFT:
// rader_pfa_kernel (mixed_fixed.hpp), Good-Thomas over M x P with the M
// DFT_P as Rader convolutions of length P - 1, one kernel, on the prime P's
// plan tables — where it beats the plan n gets without it (the race; the
// prime-factor kernel loses where the Rader list has a radix-17/19/23 pass
// or the cofactor is large: 38 of 150 sampled lengths at 0.59-0.99 x the
// chirp-z time, profiles/r06/pfa_calib.jsonl, and no cost model separated
// them). *built: p is complete (kind 8, or the alternative plan where that
// won); false (p untouched): not applicable, build_plan goes on as before.
int pfa_rader_try(int dev, int64_t n, gdsp_plan *p, bool *built) {
  *built = false;
  if ((plan_flags() & GDSP_ALGO_NO_RADER) || !gdsp::jit_enabled() || n > gdsp::kMixedSpecMax ||
      is_prime64(n))
    return GDSP_OK;
  int64_t P = 1, m = n;
  for (int64_t d = 2; d * d <= m; ++d)
    while (m % d == 0) {
      P = d;
      m /= d;
    }
  if (m > 1) P = m;  // the largest prime factor
  const int64_t M = n / P;
  if (P <= 31 || M % P == 0 || !gdsp::pfa_cofactor_supported((int)M)) return GDSP_OK;
  gdsp_plan *pp = nullptr;
  STCHK(get_plan_locked(dev, P, &pp));
  if (pp->kind != KIND_RADER) return GDSP_OK;
  int rad[16];
  const int np = pp->md.npass;
  if (np < 1 || np > 16) return GDSP_OK;
  for (int q = 0; q < np; ++q) rad[q] = (int)((pp->md.codes >> (5 * q)) & 31);
  gdsp::JitRader *j = gdsp::jit_rader_pfa_build(dev, (int)M, rad, np);
  if (!j) return GDSP_OK;
  const double scale = 1.0 / (double)n;
  Runner pfa = [&](const cd *in, cd *out, int64_t batch, hipStream_t s) -> int {
    HIPCHK(gdsp::jit_launch_rader(j, false, gdsp::LOAD_COMPLEX, in, out, batch, pp->tw,
                                  pp->bhat, pp->gpow, pp->ginv, scale, s));
    return GDSP_OK;
  };
  *built = true;
  if (auto alt = race_alternative(dev, n, SKIP_PFA, pfa)) {
    *p = std::move(*alt);
    return GDSP_OK;
  }
  p->kind = KIND_RADER_PFA;
  p->rader = j;
  p->p2 = pp;
  p->n1 = M;
  p->n2 = P;
  p->m = P - 1;
  return GDSP_OK;
}

// The fused chirp-z on a smooth convolution length L >= 2n - 1
// (bluestein_fixed_kernel), tried on a complete fused chirp-z plan p on M
// (a power of 2, or the M = 16 RB 16 kernel): L where the lane-cost
// model puts it below 0.85 of M's kernel (blufix_length: n just above a
// power of 2 — 4097 <= n <= 6144 on L <= 12288 instead of 16384, ...),
// built with its own tables (b on L, bhat = FFT_L(b) / L by the engine), and
// kept where it wins the race against p as it is (3 % margin). The same
// linear convolution, hence the same DFT. GDSP_ALGO_CHIRPZ_POW2 keeps the
// power of 2; the forced chirp-z plan keeps its M.
int blufix_try(int dev, int64_t n, gdsp_plan *p, const std::vector<cd> &w) {
  if (p->kind != KIND_BLUESTEIN || p->parts != 1 || (plan_flags() & GDSP_ALGO_CHIRPZ_POW2) ||
      !gdsp::jit_enabled())
    return GDSP_OK;
  std::vector<int> now;
  if (p->c6k) {
    int rad6[4];
    now.assign(rad6, rad6 + gdsp::chirpz6k_radices(p->m, rad6));
  } else {
    int a = p->log2m;
    for (; a >= 4; a -= 4) now.push_back(16);
    if (a) now.push_back(1 << a);
  }
  int rad[4], np = 0;
  const int L = gdsp::blufix_length(n, p->m, now.data(), (int)now.size(), rad, &np);
  if (!L) return GDSP_OK;
  gdsp::JitBlu *j = gdsp::jit_blu_build(dev, n, rad, np);
  if (!j) return GDSP_OK;
  gdsp_plan *lp = nullptr;  // FFT_L for bhat
  STCHK(get_plan_locked(dev, L, &lp));
  gdsp::MixedDesc d{};
  DevPtr<cd> tw, bh;
  STCHK(make_mixed_desc(dev, L, std::vector<int>(rad, rad + np), d, tw));
  std::vector<cd> b((size_t)L, cd{0.0, 0.0});
  for (int64_t i = 0; i < n; ++i) {  // bluestein.go:78-85 on L
    b[(size_t)i] = w[(size_t)i];
    if (i != 0) b[(size_t)(L - i)] = w[(size_t)i];
  }
  STCHK(spectrum_table(dev, lp, b, L, 1, 1.0 / (double)L, bh));
  const double scale = 1.0 / (double)n;
  Runner smooth = [&](const cd *in, cd *out, int64_t batch, hipStream_t q) -> int {
    HIPCHK(gdsp::jit_launch_blu(j, false, gdsp::LOAD_COMPLEX, in, out, batch, tw.get(), p->chirp,
                                bh.get(), scale, q));
    return GDSP_OK;
  };
  Runner now_plan = [&](const cd *in, cd *out, int64_t batch, hipStream_t q) -> int {
    return exec_plan(p, in, out, batch, false, gdsp::LOAD_COMPLEX, q);
  };
  if (!race(dev, n, smooth, now_plan, 0.97)) return GDSP_OK;
  p->blufix = j;
  p->tw_blu = p->own(std::move(tw));
  p->bhat_blu = p->own(std::move(bh));
  p->m_blu = L;
  p->md_blu = d;
  return GDSP_OK;
}

// skip (SKIP_RADER, SKIP_PFA): without those kinds, for the alternative a
// race times them against (race_alternative)
int build_plan(int dev, int64_t n, gdsp_plan *p, bool chirpz, int skip) {
  p->device = dev;
  p->n = n;
  if (n <= 1) {
    p->kind = KIND_TRIVIAL;
    return GDSP_OK;
  }
  if (is_pow2(n) && !chirpz) {
    p->log2n = ilog2(n);
    p->kind = p->log2n <= gdsp::kMaxLdsLog2 ? KIND_LDS : KIND_GLOBAL;
    return upload_twiddles(dev, n, p);
  }
  std::vector<int> rad;
  int fr[16], fnp = 0;
  if (!chirpz && n <= gdsp::kMixedSpecMax && !gdsp::mixed_fixed_radices((int)n, fr, &fnp) &&
      gdsp::jit_enabled()) {
    // smooth length without a compiled specialisation: compile one (hipRTC);
    // if that fails it takes the runtime-radix kernel or Bluestein below
    int jr[5], jnp = 0;
    if (gdsp::jit_radices((int)n, jr, &jnp)) {
      if (gdsp::JitSpec *j = gdsp::jit_spec_build(dev, jr, jnp, (int)n)) {
        p->jit = j;
        return build_mixed(dev, n, std::vector<int>(jr, jr + jnp), p);
      }
    }
  }
  if (!chirpz && mixed_radices(n, rad)) return build_mixed(dev, n, rad, p);
  if (!chirpz && next_pow2_ref(2 * n - 1) > ((int64_t)1 << gdsp::kMaxLdsLog2) &&
      (pow2rows_build(dev, n, p) || mixrows_build(dev, n, p))) {
    p->kind = KIND_MIXED4;
    STCHK(get_plan_locked(dev, p->n2, &p->p2));
    return upload_twiddles(dev, n, p);
  }
  if (!chirpz && next_pow2_ref(2 * n - 1) > ((int64_t)1 << gdsp::kMaxLdsLog2) &&
      pow2col_split(n, p->n1, p->n2)) {
    // n = 2^a * C with 2^a in [16, 512] and C a one-kernel length: the
    // power-of-2 four-step structure (column tiles, rows of C, transpose)
    p->kind = KIND_MIXED4;
    p->pow2col = true;
    STCHK(get_plan_locked(dev, p->n1, &p->p1));
    STCHK(get_plan_locked(dev, p->n2, &p->p2));
    return upload_twiddles(dev, n, p);
  }
  if (!chirpz && next_pow2_ref(2 * n - 1) > ((int64_t)1 << gdsp::kMaxLdsLog2) &&
      radixcol_split(n, p->n1, p->n2)) {
    p->kind = KIND_MIXED4;
    p->radixcol = true;
    STCHK(get_plan_locked(dev, p->n2, &p->p2));
    return upload_twiddles(dev, n, p);
  }
  if (!chirpz && next_pow2_ref(2 * n - 1) > ((int64_t)1 << gdsp::kMaxLdsLog2) &&
      mixcol_build(dev, n, p)) {
    // the same three-launch structure with a runtime-compiled column pass
    p->kind = KIND_MIXED4;
    STCHK(get_plan_locked(dev, p->n2, &p->p2));
    return upload_twiddles(dev, n, p);
  }
  if (!chirpz && next_pow2_ref(2 * n - 1) > ((int64_t)1 << gdsp::kMaxLdsLog2) &&
      mixed4_split(n, p->n1, p->n2)) {
    // smooth n beyond one kernel, where Bluestein would be the composed
    // multi-pass chain: four-step over one-kernel factors (5 passes; 3-3.5x
    // faster than composed chirp-z at 10^4..10^6, while the fused chirp-z
    // kernel still wins for n <= 8192: 3.5 vs 6.3 ms at n = 5000)
    p->kind = KIND_MIXED4;
    STCHK(get_plan_locked(dev, p->n1, &p->p1));
    STCHK(get_plan_locked(dev, p->n2, &p->p2));
    return upload_twiddles(dev, n, p);
  }
  if (!chirpz) {
    bool built = false;
    if (!(skip & SKIP_RADER)) {
      STCHK(rader_try(dev, n, p, &built));
      if (built) {
        rader_race(dev, n, p);
        return GDSP_OK;
      }
    }
    if (!(skip & SKIP_PFA)) {
      STCHK(pfa_rader_try(dev, n, p, &built));
      if (built) return GDSP_OK;
    }
  }
  // Bluestein factors, bluestein.go:32-61: w_k = (cos, sin)(Pi/n * k*k),
  // k = 0 exactly 1 (the angle reduced mod 2 Pi exactly, below).
  p->m = next_pow2_ref(2 * n - 1);
  p->log2m = ilog2(p->m);
  p->kind = p->log2m <= gdsp::kMaxLdsLog2 ? KIND_BLUESTEIN : KIND_BLUESTEIN_COMPOSED;
  if (p->kind == KIND_BLUESTEIN_COMPOSED && !chirpz && !p->mplan) {
    // Output-split chirp-z: X[k0 + k] for k < kpart needs a circular
    // convolution of length >= n + kpart - 1 only (bluestein.go:70 sizes it for
    // all n outputs, 2n - 1), so P parts of kpart = ceil(n/P) run on the
    // one-kernel M = 16384 wherever n + kpart - 1 <= 16384 with P <= 8
    // (n <= 14563); the composed chirp-z over 32768 moves ~8 HBM passes of M
    // per transform. GDSP_ALGO_NO_CHIRPZ_PARTS keeps the composed path.
    if (const int parts = chirpz_parts(n)) {
      p->m = (int64_t)1 << gdsp::kMaxLdsLog2;
      p->log2m = gdsp::kMaxLdsLog2;
      p->kind = KIND_BLUESTEIN;
      p->parts = parts;
      p->kpart = (n + parts - 1) / parts;
    }
  }
  p->unfused = (plan_flags() & GDSP_ALGO_CHIRPZ_UNFUSED) != 0;
  if (p->kind == KIND_BLUESTEIN_COMPOSED && !chirpz &&
      !(plan_flags() & GDSP_ALGO_CHIRPZ_POW2)) {
    // The composed chirp-z is HBM-bound, so its cost follows M: take the
    // smallest M >= 2n - 1 with a three-pass split (power-of-2 or
    // single-radix columns, one-kernel rows) instead of bluestein.go:70's
    // power of 2; the convolution, hence the DFT, is the same. Only where it
    // measured faster: M <= 0.55 of a power of 2 <= 2^16 (8209: 19.5 vs 22.1
    // ms, 16411: 19.4 vs 21.3; 10007, 65537, 100003 were slower), and only
    // where the power of 2 has no two-pass FFT (exec_fourstep2, 2^15..2^20):
    // against it the smooth M lost (16411 15.6 vs 9.9 ms per 2^27 samples
    // with the premultiply folded in; profiles/r04/fourstep2_ab.txt).
    // The forced chirp-z plan keeps the reference's M for the composed
    // chirp-z (the fused one at 1025..1536 / 2049..3072 takes M = 3072 / 6144
    // below).
    for (int64_t m = 2 * n - 1;
         p->m <= 65536 && !fourstep2_applies(ilog2(p->m)) && m <= (p->m * 11) / 20; ++m) {
      int64_t r = 0, c = 0;
      if (pow2col_split(m, r, c) || radixcol_split(m, r, c)) {
        gdsp_plan *mp = nullptr;
        if (get_plan_locked(dev, m, &mp) == GDSP_OK && mp->kind == KIND_MIXED4 &&
            (mp->pow2col || mp->radixcol)) {
          p->m = m;
          p->log2m = 0;
          p->mplan = mp;
        }
        break;
      }
    }
  }
  bool c6k_ok = !(plan_flags() & GDSP_ALGO_CHIRPZ_POW2);
  if (p->kind == KIND_BLUESTEIN && p->parts == 1 && gdsp::chirpz6k_m(n) && c6k_ok) {
    // 129 <= n <= 3200: bluestein.go:70 pads the convolution to
    // NextPowerOf2(2n - 1); the smallest M = 16 * RB * 16 >= 2n - 1 of the
    // kept RB gives the same linear convolution (and DFT) on up to 44 %
    // fewer points (chirpz6k.hip). GDSP_ALGO_CHIRPZ_POW2 keeps the power of 2.
    p->m = gdsp::chirpz6k_m(n);
    p->log2m = 0;
    p->c6k = true;
    gdsp::MixedDesc d6{};
    int rad6[4];
    const int np6 = gdsp::chirpz6k_radices(p->m, rad6);
    DevPtr<cd> tw6k;
    STCHK(make_mixed_desc(dev, p->m, std::vector<int>(rad6, rad6 + np6), d6, tw6k, false));
    p->tw6k = p->own(std::move(tw6k));
  }
  if (!p->mplan) STCHK(get_plan_locked(dev, p->m, &p->mplan));
  std::vector<cd> w((size_t)n), chirp((size_t)n),
      b((size_t)p->m * (size_t)p->parts, cd{0.0, 0.0});
  for (int64_t k = 0; k < n; ++k) {
    double sn = 0.0, cs = 1.0;
    if (k != 0) {
      // k*k mod 2n in integers, then the angle in long double: each factor
      // within half an ulp of exp(i Pi k*k / n). bluestein.go:53 leaves the
      // angle at Pi/n * k*k, whose rounding error grows with k*k (3e2 u at
      // n = 100, 2e4 u at 3000, 6e4 u at 16411 in the transform); the engine
      // keeps the exact DFT (tests/test_accuracy_gpu.py)
      const long double ang = 3.141592653589793238462643383279502884L *
                              (long double)((k * k) % (2 * n)) / (long double)n;
      sn = (double)sinl(ang);
      cs = (double)cosl(ang);
    }
    w[(size_t)k] = {cs, sn};
    chirp[(size_t)k] = {cs, -sn};
  }
  if (p->parts == 1) {
    for (int64_t i = 0; i < n; ++i) {  // bluestein.go:78-85
      b[(size_t)i] = w[(size_t)i];
      if (i != 0) b[(size_t)(p->m - i)] = w[(size_t)i];
    }
  } else {
    // part q: c[j mod M] = w_(k0 + j), j in [-(n-1), kpart-1], k0 = q kpart
    // (w_(-i) = w_i; indices k0 + j >= n feed no wanted output)
    for (int q = 0; q < p->parts; ++q) {
      cd *c = b.data() + (size_t)q * (size_t)p->m;
      const int64_t k0 = q * p->kpart;
      for (int64_t j = -(n - 1); j < p->kpart; ++j) {
        const int64_t i = k0 + j < 0 ? -(k0 + j) : k0 + j;
        if (i < n) c[(size_t)(j < 0 ? p->m + j : j)] = w[(size_t)i];
      }
    }
  }
  DevPtr<cd> dchirp, bhat;
  STCHK(upload(dev, chirp.data(), (size_t)n, dchirp));
  p->chirp = p->own(std::move(dchirp));
  // FFT_M(b) on the device with the engine itself, then fold the IFFT's 1/M
  STCHK(spectrum_table(dev, p->mplan, b, p->m, p->parts, 1.0 / (double)p->m, bhat));
  p->bhat = p->own(std::move(bhat));
  if (!chirpz) STCHK(blufix_try(dev, n, p, w));
  return GDSP_OK;
}

int get_plan_locked(int dev, int64_t n, gdsp_plan **out, bool chirpz) {
  auto &cache = chirpz ? g_chirpz_plans : g_plans;
  auto key = std::make_tuple(dev, n, plan_flags());
  auto it = cache.find(key);
  if (it != cache.end()) {
    *out = it->second;
    return GDSP_OK;
  }
  gdsp_plan *p = new gdsp_plan();
  struct Depth {  // leaves the snapshot on every exit, exceptions included
    explicit Depth(unsigned f) {
      if (t_build_depth++ == 0) t_build_flags = f;
    }
    ~Depth() { --t_build_depth; }
  };
  int st;
  {
    Depth d(std::get<2>(key));
    st = build_plan(dev, n, p, chirpz);
  }
  if (st != GDSP_OK) {
    // a plan that failed to build frees what it allocated, once nothing
    // queued on the building thread's stream reads it any more
    (void)hipStreamSynchronize(thread_stream(dev));
    delete p;
    return st;
  }
  cache[key] = p;
  *out = p;
  return GDSP_OK;
}

}  // namespace

namespace gdsp_api {

int get_plan(int64_t n, gdsp_plan **out, bool chirpz) {
  int dev = 0;
  STCHK(current_device(&dev));
  std::lock_guard<std::recursive_mutex> lk(g_plan_mu);
  return get_plan_locked(dev, n, out, chirpz);
}

int device_table(int dev, const std::vector<cd> &h, DevPtr<cd> &out) {
  return upload(dev, h.data(), h.size(), out);
}

int plan_spectrum_table(int dev, const gdsp_plan *fft, const std::vector<cd> &b, int64_t len,
                        int64_t count, double scale, DevPtr<cd> &out) {
  return spectrum_table(dev, fft, b, len, count, scale, out);
}

bool build_flags(unsigned *flags) {
  *flags = t_build_flags;
  return t_build_depth > 0;
}

}  // namespace gdsp_api
