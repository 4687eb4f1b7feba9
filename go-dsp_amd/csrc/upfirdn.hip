// upfirdn.hip — polyphase resampling of real rows (scipy.signal.upfirdn: zero-
// stuff by up, filter with m taps, keep every down-th sample; no reference
// equivalent): with p = (j down) mod up, i0 = (j down) div up, T = ceil(m / up),
//   out[c, j] = sum_{t < T} h[p + t up] x[c, i0 - t],
// taps at index >= m and samples outside the row counting as 0.
//
//   upfirdn_taps_kernel   the taps in phase-major order, hp[p T + t] = h[p + t up]
//                         (0 past m), once per call
//   upfirdn_poly_kernel   the fused form: a workgroup owns tiles of J = Q E
//                         consecutive outputs of one channel; the samples a
//                         tile reads come from HBM once into LDS, the phase
//                         table once per workgroup; every output is stored once
//   upfirdn_plain_kernel  one thread per output, taps and samples from global
//                         memory: every shape the fused form does not serve
//
// Both forms sum an output in ascending t with one fused multiply-add per
// term from +0.0, terms of zero weight and samples outside the row included:
// an output's bits do not depend on the form, tile, range or launch.
#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

namespace {

constexpr int kUfThreads = 256;
// table plus tile: 64 KiB, so that two workgroups share a CU
constexpr int kUfLdsDoubles = 8192;
// a thread's slots are Q <= kUfMaxQ apart
constexpr int kUfMaxQ = 2048;
// loads of a tile's samples a thread keeps in flight
constexpr int kUfLoads = 6;

__device__ __forceinline__ int uf_clampi(int64_t v, int lim) {
  return v < 0 ? 0 : (v > lim ? lim : (int)v);
}

// PAD: one padding double every 32 (a row of the 64 banks): lanes that read
// the tile at a stride of 2, 4, 8, 16 or 32 doubles (up = 1, lane l reads
// sample l down) fall on 32 distinct banks per ds_read_b64 group of 32 lanes.
// Without it (down <= up: lanes at most a sample apart) the index is linear
// in t and the unrolled reads share one address register.
template <bool PAD>
__device__ __forceinline__ int uf_padx(int i) {
  return PAD ? i + (i >> 5) : i;
}

// Samples off + ib + u 256, u < U, of a row into the tile: U loads in flight
// together, each index clamped into the window [lo, hi) (not empty) of samples
// the row holds, so that no load hangs on a branch; outside it the tile gets 0
template <int U, bool PAD>
__device__ __forceinline__ void uf_load(double *lx, const double *xrow, int64_t off, int ib, int lo,
                                        int hi) {
  double v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = ib + u * kUfThreads;
    v[u] = ld_nt(&xrow[off + (i < lo ? lo : (i >= hi ? hi - 1 : i))]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = ib + u * kUfThreads;
    lx[uf_padx<PAD>(i)] = (i >= lo && i < hi) ? v[u] : 0.0;
  }
}

}  // namespace

// hp[p T + t] = h[p + t up] for p + t up < m, else 0; count = up T
__global__ void upfirdn_taps_kernel(const double *__restrict__ h, int64_t m, int64_t up, int64_t T,
                                    double *hp, int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t p = e / T, t = e - p * T, k = p + t * up;
  hp[e] = k < m ? h[k] : 0.0;
}

// Workgroup blk of the launch (after xcd_remap: neighbouring workgroups of a
// row, which share a halo of T - 1 samples, run on one XCD and find it in
// that XCD's L2) serves channel c0 + blk / wpr and the K tiles from (blk %
// wpr) K of that row. Tile b holds outputs jt0 + [0, cnt), jt0 = out_begin +
// b J: thread lt takes the slots q = lt, lt + 256, ... < Q and of each the E
// outputs jt0 + q + k Q. Q is a multiple of the phase period up / gcd(up,
// down), so the E outputs share the phase p — each tap is read once and used
// E times — and lie QD = Q down / up samples apart. LDS: the table, row p at
// p Tp (Tp odd where up > 1: lanes on different phases at one t on different
// banks), then the tile's samples xs + [0, span), xs = (jt0 down) div up - (T -
// 1), at uf_padx. The rows hold samples [x_lo, x_hi) of the signal. The taps
// loop is unrolled by 8: a thread's LDS reads are in flight together (two
// workgroups of four waves per CU leave their latency nothing else to hide
// behind), the multiply-adds of an output stay in ascending t.
template <int E, bool PAD>
__global__ __launch_bounds__(kUfThreads) void upfirdn_poly_kernel(
    const double *x, int64_t ldx, int64_t x_lo, int64_t x_hi, const double *__restrict__ hp, int up,
    int down, int T, int Tp, int Q, int QD, int span, int64_t tpr, int64_t wpr, int K, int64_t c0,
    int64_t out_begin, int64_t out_end, double *out, int64_t ldo) {
  extern __shared__ double uf_lds[];
  double *lh = uf_lds, *lx = uf_lds + up * Tp;
  const int lt = threadIdx.x;
  const int64_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t cr = blk / wpr, w = blk - cr * wpr, c = c0 + cr;
  const int J = Q * E;
  if (Tp == T) {
    for (int e = lt; e < up * T; e += kUfThreads) lh[e] = hp[e];
  } else {
    for (int e = lt; e < up * T; e += kUfThreads) {
      const int p = e / T;
      lh[p * Tp + (e - p * T)] = hp[e];
    }
  }
  const double *xrow = x + c * ldx;
  double *orow = out + c * ldo;
  const int64_t b0 = w * K, b1 = b0 + K < tpr ? b0 + K : tpr;
  for (int64_t b = b0; b < b1; ++b) {
    // the tile's 64-bit geometry once per thread; the guards compare ints
    const int64_t jt0 = out_begin + b * J;
    const int cnt = uf_clampi(out_end - jt0, J);
    const int64_t a0 = jt0 * down, d0 = a0 / up;
    const int r0 = (int)(a0 - d0 * up);
    const int64_t xs = d0 - (T - 1);
    const int lo = uf_clampi(x_lo - xs, span), hi = uf_clampi(x_hi - xs, span);
    const int64_t off = xs - x_lo;  // sample xs + i of the signal is xrow[off + i]
    if (b > b0) __syncthreads();    // the previous tile's reads
    if (hi > lo) {
      // whole batches of kUfLoads loads, then pairs, then one: no thread loads
      // more than a pair past its share of a short tile
      int ib = lt;
      for (; ib + (kUfLoads - 1) * kUfThreads < span; ib += kUfLoads * kUfThreads)
        uf_load<kUfLoads, PAD>(lx, xrow, off, ib, lo, hi);
      for (; ib + kUfThreads < span; ib += 2 * kUfThreads)
        uf_load<2, PAD>(lx, xrow, off, ib, lo, hi);
      if (ib < span) uf_load<1, PAD>(lx, xrow, off, ib, lo, hi);
    } else {
      for (int i = lt; i < span; i += kUfThreads) lx[uf_padx<PAD>(i)] = 0.0;
    }
    __syncthreads();
    for (int q = lt; q < Q; q += kUfThreads) {
      const unsigned a = (unsigned)r0 + (unsigned)q * (unsigned)down;
      const unsigned i0 = a / (unsigned)up;
      const int p = (int)(a - i0 * (unsigned)up);
      const int base = (int)i0 + T - 1;  // sample i0 of slot q's first output
      const double *hrow = lh + p * Tp;
      double acc[E];
#pragma unroll
      for (int k = 0; k < E; ++k) acc[k] = 0.0;
#pragma unroll 8
      for (int t = 0; t < T; ++t) {
        const double hv = hrow[t];
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] = fma(hv, lx[uf_padx<PAD>(base + k * QD - t)], acc[k]);
      }
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int jr = q + k * Q;
        if (jr < cnt) __builtin_nontemporal_store(acc[k], &orow[(jt0 - out_begin) + jr]);
      }
    }
  }
}

// One thread per output: block b of the launch serves channel c0 + b / bpr and
// outputs out_begin + (b % bpr) 256 + [0, 256) of it. UP1 (up == 1): every
// lane reads the same tap, through the scalar cache. t in [t_lo, t_hi) reads a
// sample of the row; where that is every t (all but the ends of a row) the loop
// carries no guard. The terms and their order are the fused form's.
template <bool UP1>
__global__ __launch_bounds__(kUfThreads) void upfirdn_plain_kernel(
    const double *__restrict__ x, int64_t ldx, int64_t x_lo, int64_t x_hi,
    const double *__restrict__ hp, int64_t up, int64_t down, int T, int64_t bpr, int64_t c0,
    int64_t out_begin, int64_t out_end, double *__restrict__ out, int64_t ldo) {
  const int64_t cr = (int64_t)blockIdx.x / bpr, b = (int64_t)blockIdx.x - cr * bpr, c = c0 + cr;
  const int64_t j = out_begin + b * kUfThreads + threadIdx.x;
  if (j >= out_end) return;
  const int64_t a = j * down, i0 = UP1 ? a : a / up, p = UP1 ? 0 : a - i0 * up;
  const double *xrow = x + c * ldx, *hrow = hp + p * T;
  const int t_lo = uf_clampi(i0 - x_hi + 1, T), t_hi = uf_clampi(i0 - x_lo + 1, T);
  const double *xp = xrow + (i0 - x_lo);  // sample i0: read only at t in [t_lo, t_hi)
  double acc = 0.0;
  if (t_lo == 0 && t_hi == T) {
#pragma unroll 8
    for (int t = 0; t < T; ++t) acc = fma(hrow[t], xp[-(int64_t)t], acc);
  } else {
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
      const bool ok = t >= t_lo && t < t_hi;
      const double v = *(ok ? xp - t : xrow);  // xrow[0] exists: x_hi > x_lo
      acc = fma(hrow[t], ok ? v : 0.0, acc);
    }
  }
  out[c * ldo + (j - out_begin)] = acc;
}

static int64_t uf_gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t r = a % b;
    a = b;
    b = r;
  }
  return a;
}

UpfirdnGeo upfirdn_geometry(int64_t m, int64_t up, int64_t down) {
  UpfirdnGeo g = {};
  if (m <= 0 || up < 1 || down < 1 || up > 65536 || down > 65536 || m > ((int64_t)1 << 24))
    return g;
  const int64_t T = (m + up - 1) / up, Tp = up == 1 ? T : (T | 1), table = up * Tp;
  if (table > kUfLdsDoubles) return g;
  const int64_t P = up / uf_gcd(up, down);  // outputs P apart share a phase
  if (P > kUfMaxQ) return g;
  // Q: the first multiple of P from 256 on that leaves at most 5 % of the
  // threads' slot rounds idle, else the one that leaves the least
  int64_t Q = 0;
  double best = 0;
  for (int64_t k = (kUfThreads + P - 1) / P; k * P <= kUfMaxQ; ++k) {
    const int64_t q = k * P, rounds = (q + kUfThreads - 1) / kUfThreads;
    const double eff = (double)q / (double)(rounds * kUfThreads);
    if (eff > best) {
      best = eff;
      Q = q;
    }
    if (eff >= 0.95) break;
  }
  if (Q == 0) return g;
  // lanes more than a sample apart wrap over the banks within a read: padded
  // (at 2/3 the wrapped lanes land on the banks the stride leaves out)
  const bool pad = down > up;
  for (int E = 4; E >= 1; E >>= 1) {
    const int64_t J = Q * E, span = ((J - 1) * down + up - 1) / up + T;
    const int64_t lds = table + span + (pad ? span >> 5 : 0) + 1;
    if (lds > kUfLdsDoubles) continue;
    g.fits = true;
    g.T = (int)T;
    g.Tp = (int)Tp;
    g.Q = (int)Q;
    g.E = E;
    g.pad = pad;
    g.QD = (int)(Q / P * (down / uf_gcd(up, down)));
    g.span = (int)span;
    g.lds_doubles = (int)lds;
    return g;
  }
  return g;
}

hipError_t launch_upfirdn_taps(const double *h, int64_t m, int64_t up, double *hp, hipStream_t s) {
  if (m <= 0 || up < 1 || !h || !hp) return hipErrorInvalidValue;
  const int64_t T = (m + up - 1) / up, count = up * T, nblk = (count + 255) / 256;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(upfirdn_taps_kernel, dim3((unsigned)nblk), dim3(256), 0, s, h, m, up, T, hp,
                     count);
  return hipGetLastError();
}

hipError_t launch_upfirdn_poly(const UpfirdnGeo &g, const double *x, int64_t ldx, int64_t x_lo,
                               int64_t x_hi, const double *hp, int64_t up, int64_t down,
                               int64_t channels, int64_t out_begin, int64_t out_end, double *out,
                               int64_t ldo, hipStream_t s) {
  if (!g.fits || channels <= 0 || out_end <= out_begin || out_begin < 0 || !x || !hp || !out)
    return hipErrorInvalidValue;
  const int64_t J = (int64_t)g.Q * g.E, tpr = (out_end - out_begin + J - 1) / J;
  // tiles per workgroup: the table is read once per workgroup; enough
  // workgroups stay to fill the device several times over
  int64_t K = channels * tpr / 4096;
  K = K < 1 ? 1 : (K > 8 ? 8 : K);
  if (K > tpr) K = tpr;
  const int64_t wpr = (tpr + K - 1) / K, cpl = 0x7fffffff / wpr;  // channels per launch
  if (cpl < 1) return hipErrorInvalidValue;
  const size_t lds = (size_t)g.lds_doubles * sizeof(double);
  for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
    const int64_t cc = channels - c0 < cpl ? channels - c0 : cpl;
    const dim3 grid((unsigned)(cc * wpr)), blockd(kUfThreads);
#define GDSP_UF_LAUNCH(EE)                                                                      \
  if (g.pad)                                                                                    \
    hipLaunchKernelGGL((upfirdn_poly_kernel<EE, true>), grid, blockd, lds, s, x, ldx, x_lo,     \
                       x_hi, hp, (int)up, (int)down, g.T, g.Tp, g.Q, g.QD, g.span, tpr, wpr,    \
                       (int)K, c0, out_begin, out_end, out, ldo);                               \
  else                                                                                          \
    hipLaunchKernelGGL((upfirdn_poly_kernel<EE, false>), grid, blockd, lds, s, x, ldx, x_lo,    \
                       x_hi, hp, (int)up, (int)down, g.T, g.Tp, g.Q, g.QD, g.span, tpr, wpr,    \
                       (int)K, c0, out_begin, out_end, out, ldo)
    switch (g.E) {
      case 4: GDSP_UF_LAUNCH(4); break;
      case 2: GDSP_UF_LAUNCH(2); break;
      case 1: GDSP_UF_LAUNCH(1); break;
      default: return hipErrorInvalidValue;
    }
#undef GDSP_UF_LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_upfirdn_plain(const double *x, int64_t ldx, int64_t x_lo, int64_t x_hi,
                                const double *hp, int64_t m, int64_t up, int64_t down,
                                int64_t channels, int64_t out_begin, int64_t out_end, double *out,
                                int64_t ldo, hipStream_t s) {
  if (m <= 0 || up < 1 || down < 1 || channels <= 0 || out_end <= out_begin || out_begin < 0 ||
      x_hi <= x_lo || m > ((int64_t)1 << 24) || !x || !hp || !out)
    return hipErrorInvalidValue;
  const int T = (int)((m + up - 1) / up);
  const int64_t bpr = (out_end - out_begin + kUfThreads - 1) / kUfThreads, cpl = 0x7fffffff / bpr;
  if (cpl < 1) return hipErrorInvalidValue;
  for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
    const int64_t cc = channels - c0 < cpl ? channels - c0 : cpl;
    const dim3 grid((unsigned)(cc * bpr)), blockd(kUfThreads);
    if (up == 1)
      hipLaunchKernelGGL(upfirdn_plain_kernel<true>, grid, blockd, 0, s, x, ldx, x_lo, x_hi, hp, up,
                         down, T, bpr, c0, out_begin, out_end, out, ldo);
    else
      hipLaunchKernelGGL(upfirdn_plain_kernel<false>, grid, blockd, 0, s, x, ldx, x_lo, x_hi, hp,
                         up, down, T, bpr, c0, out_begin, out_end, out, ldo);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace gdsp
