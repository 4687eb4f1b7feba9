// fir.hip — FIR filtering of long real rows by overlap-save: out[c, i] =
// sum_{k < m} h[k] x[c, i - k], x zero outside [0, n), one h for all rows or
// one per row (no reference equivalent).
//
//   fir_ols_kernel      F = 256 ... 16384, m <= F / 2: two overlapping real
//                       blocks of a row as a + i b, FFT_F, times FFT_F(h),
//                       inverse FFT_F, the valid parts of Re and Im stored, in
//                       one workgroup — the samples read about once and
//                       written once as float64, nothing in between in HBM
//   fir_taps_kernel     the zero-padded taps as complex rows of F (their
//                       spectrum comes from the plan's batched FFT)
//   fir_gather_kernel,  the composed form's ends: the packed blocks as complex
//   fir_scatter_kernel  rows of F; the valid parts of the inverse transform
//
// Block b of a row (L = F - m + 1) reads x[b L - (m - 1) + i], i in [0, F),
// and owns out[b L + j], j in [0, L): positions m - 1 + j of its circular
// convolution with the taps. The taps are real, so FFT_F(a + i b) times their
// spectrum transforms back to (a * h) + i (b * h): transform p of a row
// carries blocks 2p and 2p + 1 with no separation step.
#include "conv_core.hpp"
#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

// Where transform g of the job (channel c = g / tpr, pair p = g % tpr) reads
// and writes, as 32-bit windows on the F positions of its two blocks: all
// 64-bit arithmetic is done once per thread, the per-element guards compare
// ints.
struct FirSlot {
  const double *src;  // x row + first sample of block 2p (may lie before the row)
  double *dst;        // out row + first output of block 2p
  int lo[2], hi[2];   // loads of block 2p + j: lo <= i < hi (else 0)
  int cnt[2];         // outputs of block 2p + j: positions m - 1 + [0, cnt)
};

// 8-byte nontemporal store through a bounds-checked descriptor (fft_device.hpp
// buf_st_nt): offsets past the descriptor's bytes are dropped by the hardware
__device__ __forceinline__ void buf_st1_nt(rsrc_t r, uint32_t off, double v) {
  decltype(__builtin_amdgcn_raw_buffer_load_b64(r, 0, 0, 0)) q;
  __builtin_memcpy(&q, &v, sizeof(double));
  __builtin_amdgcn_raw_buffer_store_b64(q, r, off, 0, 2);
}

__device__ __forceinline__ int clampi(int64_t v, int lim) {
  return v < 0 ? 0 : (v > lim ? lim : (int)v);
}

__device__ __forceinline__ FirSlot fir_slot(const double *x, int64_t ldx, double *out, int64_t ldo,
                                            int64_t g, int64_t tpr, int64_t n, int64_t out_len,
                                            int m, int F, bool valid) {
  const int L = F - m + 1;
  const int64_t c = g / tpr, p = g - c * tpr;
  const int64_t o0 = 2 * p * (int64_t)L;  // first output of block 2p
  const int64_t s0 = o0 - (m - 1);        // its first sample
  FirSlot s;
  s.src = x + c * ldx + s0;
  s.dst = out + c * ldo + o0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t sj = s0 + (int64_t)j * L, oj = o0 + (int64_t)j * L;
    s.lo[j] = clampi(-sj, F);
    s.hi[j] = clampi(n - sj, F);
    // a block past the end of the row (or of the job) stores nothing
    s.cnt[j] = valid ? clampi(out_len - oj, L) : 0;
  }
  return s;
}

// One workgroup holds TPW transforms in registers (thread t of a transform
// owns elements t + k T), as convolve_lds_kernel does; total = channels * tpr
// transforms, tpr = ceil(blocks / 2) per row. hspec: FFT_F of the zero-padded
// taps, row c at hspec + c hstride (0: one for all). A block that is partial,
// or missing (an odd block count, a slot past the job), only narrows the
// windows of single loads and stores: every thread reaches every barrier.
template <int LOG2N, bool SPLIT, int LOG2E>
__global__ __launch_bounds__((Geo<LOG2N, LOG2E>::WG)) void fir_ols_kernel(
    const double *x, int64_t ldx, double *out, int64_t ldo, int64_t total, int64_t tpr, int64_t n,
    int64_t out_len, int m, const cd *__restrict__ tw, const cd *__restrict__ hspec,
    int64_t hstride, double scale) {
  using G = Geo<LOG2N, LOG2E>;
  static_assert(G::T >= 16, "rows of fewer than 16 threads need LDS staging to stay coalesced");
  __shared__ double lds[(SPLIT ? 1 : 2) * G::LDS_DOUBLES];
  const int lt = threadIdx.x;
  // a transform of whole waves: its slot, and all that follows from it, is
  // wave-uniform (the stores' descriptors below must be)
  const int slot = G::T >= 64 ? __builtin_amdgcn_readfirstlane(lt / G::T) : lt / G::T;
  const int t = lt & (G::T - 1);
  // neighbouring transforms of a row go to one XCD: the halo a block shares
  // with the next is re-read from that XCD's L2
  const int64_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t g = blk * G::TPW + slot;
  // Only the last workgroup can hold slots past the job (TPW > 1): they run a
  // valid transform (clamped) and store nothing.
  const bool valid = G::TPW == 1 || g < total;
  const int64_t gl = G::TPW == 1 ? g : (g < total ? g : total - 1);
  double *lre = lds + slot * G::STRIDE;
  double *lim = SPLIT ? lre : lds + G::LDS_DOUBLES + slot * G::STRIDE;
  const FirSlot fs = fir_slot(x, ldx, out, ldo, gl, tpr, n, out_len, m, G::N, valid);
  const int L = G::N - m + 1;
  cd v[G::E];
#pragma unroll
  for (int k = 0; k < G::E; ++k) {
    const int i = t + k * G::T;
    v[k].x = (i >= fs.lo[0] && i < fs.hi[0]) ? ld_nt(&fs.src[i]) : 0.0;
  }
#pragma unroll
  for (int k = 0; k < G::E; ++k) {
    const int i = t + k * G::T;
    v[k].y = (i >= fs.lo[1] && i < fs.hi[1]) ? ld_nt(&fs.src[(int64_t)L + i]) : 0.0;
  }
  const YhatEpi<G::T> ye{hspec + (gl / tpr) * hstride + t};
  fft_regs<LOG2N, SPLIT, 1, LOG2E, 0, 0, const cd *, 1, 0, YhatEpi<G::T>, conv_prew(LOG2N)>(
      v, t, tw, lre, lim, true, ye);
  fft_regs<LOG2N, SPLIT, 1, LOG2E, 0, 0, const cd *, 1, 0, NoEpi, conv_prew(LOG2N)>(
      v, t, tw, lre, lim, false);
  // v = conj(F (a * h + i b * h)): block 2p is Re, block 2p + 1 is -Im
  const int j0 = opaque_int(t) - (m - 1);  // the block's output index of element t
  if constexpr (G::T >= 64) {
    // outputs [0, cnt) of each block through a descriptor of just that range:
    // positions before m - 1 (a negative index, a huge unsigned offset) and
    // past cnt are dropped by the bounds check, with no branch per element
    const rsrc_t r0 = make_rsrc(fs.dst, (int64_t)fs.cnt[0] * 8);
    const rsrc_t r1 = make_rsrc(fs.dst + L, (int64_t)fs.cnt[1] * 8);
    const uint32_t off = (uint32_t)j0 * 8u;
#pragma unroll
    for (int k = 0; k < G::E; ++k) buf_st1_nt(r0, off + (uint32_t)(k * G::T) * 8u, v[k].x * scale);
#pragma unroll
    for (int k = 0; k < G::E; ++k) buf_st1_nt(r1, off + (uint32_t)(k * G::T) * 8u, -v[k].y * scale);
  } else {
    // several transforms per wave: no wave-uniform range, so a guard per element
#pragma unroll
    for (int k = 0; k < G::E; ++k) {
      const int j = j0 + k * G::T;
      if ((unsigned)j < (unsigned)fs.cnt[0]) __builtin_nontemporal_store(v[k].x * scale, &fs.dst[j]);
    }
#pragma unroll
    for (int k = 0; k < G::E; ++k) {
      const int j = j0 + k * G::T;
      if ((unsigned)j < (unsigned)fs.cnt[1])
        __builtin_nontemporal_store(-v[k].y * scale, &fs.dst[(int64_t)L + j]);
    }
  }
}

template <int LOG2N>
static hipError_t launch_fir_t(const double *x, int64_t ldx, double *out, int64_t ldo,
                               int64_t total, int64_t tpr, int64_t n, int64_t out_len, int m,
                               const cd *tw, const cd *hspec, int64_t hstride, hipStream_t s) {
  constexpr int LOG2E = conv_log2e(LOG2N);
  using G = Geo<LOG2N, LOG2E>;
  const int64_t nblk = (total + G::TPW - 1) / G::TPW;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((fir_ols_kernel<LOG2N, true, LOG2E>), dim3((unsigned)nblk), dim3(G::WG), 0, s,
                     x, ldx, out, ldo, total, tpr, n, out_len, m, tw, hspec, hstride,
                     1.0 / (double)G::N);
  return hipGetLastError();
}

int64_t fir_ols_workgroups(int log2f, int64_t total) {
  const int e = conv_log2e(log2f);
  const int64_t t = (int64_t)1 << (log2f - e);
  const int64_t tpw = t >= 256 ? 1 : 256 / t;
  return (total + tpw - 1) / tpw;
}

hipError_t launch_fir_ols(int log2f, const double *x, int64_t ldx, double *out, int64_t ldo,
                          int64_t channels, int64_t n, int64_t out_len, int64_t m, const cd *tw,
                          const cd *hspec, int64_t hstride, hipStream_t s) {
  const int64_t F = (int64_t)1 << log2f;
  if (channels <= 0 || n <= 0 || m <= 0 || 2 * m > F || out_len <= 0 || !x || !out || !tw ||
      !hspec || (hstride != 0 && hstride != F))
    return hipErrorInvalidValue;
  const int64_t L = F - m + 1, nb = (out_len + L - 1) / L, tpr = (nb + 1) / 2;
  const int64_t total = channels * tpr;
  static_assert(kConvMinLog2 == 8 && kMaxLdsLog2 == 14, "the cases below");
#define GDSP_FIR_CASE(K)                                                                       \
  case K:                                                                                      \
    return launch_fir_t<K>(x, ldx, out, ldo, total, tpr, n, out_len, (int)m, tw, hspec, hstride, s)
  switch (log2f) {
    GDSP_FIR_CASE(8);
    GDSP_FIR_CASE(9);
    GDSP_FIR_CASE(10);
    GDSP_FIR_CASE(11);
    GDSP_FIR_CASE(12);
    GDSP_FIR_CASE(13);
    GDSP_FIR_CASE(14);
    default: return hipErrorInvalidValue;
  }
#undef GDSP_FIR_CASE
}

// out[r F + i] = h[r m + i] for i < m, else 0
__global__ void fir_taps_kernel(const double *__restrict__ h, int64_t m, int64_t F, cd *out,
                                int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / F, i = e - r * F;
  out[e] = cd{i < m ? h[r * m + i] : 0.0, 0.0};
}

hipError_t launch_fir_taps(const double *h, int64_t h_rows, int64_t m, int64_t F, cd *out,
                           hipStream_t s) {
  if (h_rows <= 0 || m <= 0 || m > F || !h || !out) return hipErrorInvalidValue;
  const int64_t count = h_rows * F, nblk = (count + 255) / 256;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fir_taps_kernel, dim3((unsigned)nblk), dim3(256), 0, s, h, m, F, out, count);
  return hipGetLastError();
}

// Transforms [g0, g0 + cnt) of the job as rows of F: row r element i =
// (sample i of block 2p, sample i of block 2p + 1), the fused kernel's packing
__global__ void fir_gather_kernel(const double *__restrict__ x, int64_t ldx, int64_t g0,
                                  int64_t tpr, int64_t n, int64_t m, int64_t F, cd *buf,
                                  int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / F, i = e - r * F, g = g0 + r;
  const int64_t c = g / tpr, p = g - c * tpr, L = F - m + 1;
  const int64_t i0 = 2 * p * L - (m - 1) + i, i1 = i0 + L;
  const double *row = x + c * ldx;
  buf[e] = cd{i0 >= 0 && i0 < n ? row[i0] : 0.0, i1 >= 0 && i1 < n ? row[i1] : 0.0};
}

__global__ void fir_scatter_kernel(const cd *__restrict__ buf, int64_t g0, int64_t tpr,
                                   int64_t out_len, int64_t m, int64_t F, double *out, int64_t ldo,
                                   int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e / F, i = e - r * F, g = g0 + r;
  if (i < m - 1) return;
  const int64_t c = g / tpr, p = g - c * tpr, L = F - m + 1;
  const int64_t o0 = 2 * p * L + i - (m - 1), o1 = o0 + L;
  const cd v = buf[e];
  double *row = out + c * ldo;
  if (o0 < out_len) row[o0] = v.x;
  if (o1 < out_len) row[o1] = v.y;
}

hipError_t launch_fir_gather(const double *x, int64_t ldx, int64_t g0, int64_t cnt, int64_t tpr,
                             int64_t n, int64_t m, int64_t F, cd *buf, hipStream_t s) {
  if (cnt <= 0 || tpr <= 0 || m <= 0 || m > F || !x || !buf) return hipErrorInvalidValue;
  const int64_t count = cnt * F, nblk = (count + 255) / 256;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fir_gather_kernel, dim3((unsigned)nblk), dim3(256), 0, s, x, ldx, g0, tpr, n,
                     m, F, buf, count);
  return hipGetLastError();
}

hipError_t launch_fir_scatter(const cd *buf, int64_t g0, int64_t cnt, int64_t tpr, int64_t out_len,
                              int64_t m, int64_t F, double *out, int64_t ldo, hipStream_t s) {
  if (cnt <= 0 || tpr <= 0 || m <= 0 || m > F || !out || !buf) return hipErrorInvalidValue;
  const int64_t count = cnt * F, nblk = (count + 255) / 256;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fir_scatter_kernel, dim3((unsigned)nblk), dim3(256), 0, s, buf, g0, tpr,
                     out_len, m, F, out, ldo, count);
  return hipGetLastError();
}

}  // namespace gdsp
