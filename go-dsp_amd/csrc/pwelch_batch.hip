// pwelch_batch.hip — the fused Pwelch accumulation (spectral/pwelch.go:104-122)
// over the channels of a planar batch: channel c is n float64 from x + c ldx
// (any ldx >= n: every load is one double). The lengths of pwelch_wave.hip,
// F = max(Pad, NFFT) a power of 2 from 64 to 2048, and that kernel's
// arithmetic and synchronisation: packed segment pairs z = w x_s + i w x_(s+1),
// S = 64 / T transforms side by side in a wave exchanging through wave-private
// LDS (two-wave workgroups at F = 2048), |Z_k|^2 summed in registers, the HALF
// (Noverlap = NFFT / 2), PAD (NFFT < F) and plain variants. See
// pwelch_wave.hip for the reasoning behind each of those; what is new here is
// the channel dimension.
//
// A worker (a wave, or the two waves of a workgroup at F = 2048) owns a
// contiguous range of pair groups of one channel: worker index = channel *
// wpc + i, i < wpc workers per channel. The launch sizes wpc from the whole
// job (pwelch_batch_geometry), so many short channels get one worker each and
// a few long ones share the machine as a single signal would. Partials are
// [channel][wpc * S rows][F]; reduce_batch_l1 / reduce_batch_l2 add each
// channel's rows into acc + c F in a fixed order.
#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

constexpr int kPwbWaves = 4;  // waves per workgroup

template <int LOG2F>
struct PwbGeo {
  using G = Geo<LOG2F>;
  static constexpr int T = G::T;
  static constexpr bool WAVE = T <= 64;
  static constexpr int S = WAVE ? 64 / T : 1;       // transforms (pairs) per worker
  static constexpr int WPB = WAVE ? kPwbWaves : 1;  // workers per workgroup
  static constexpr int BLOCK = WAVE ? 64 * kPwbWaves : T;
  static constexpr int TWN = G::N / G::radix(G::NPASS - 1);
  // waves per SIMD the registers are held to, as PwwGeo::wpe
  static constexpr int wpe(bool half) { return WAVE && half ? 3 : 1; }
};

template <int LOG2F, bool HALF, bool PAD>
__global__ __launch_bounds__((PwbGeo<LOG2F>::BLOCK))
__attribute__((amdgpu_waves_per_eu(PwbGeo<LOG2F>::wpe(HALF)))) void pwelch_batch_kernel(
    const double *__restrict__ x, int64_t ldx, int64_t channels, int64_t wpc, int64_t nfft,
    int64_t stride, int64_t seg_begin, int64_t seg_end, int64_t groups_per_worker,
    const double *__restrict__ win, const cd *__restrict__ tw, double *__restrict__ partial) {
  using G = Geo<LOG2F>;
  using W = PwbGeo<LOG2F>;
  constexpr int E = G::E, T = G::T, F = G::N, H = E / 2;
  static_assert(E == 16 && (T <= 64 ? 64 % T == 0 : T == 128), "one transform per wave or two waves");
  static_assert(!(HALF && PAD), "half overlap implies Pad = NFFT");
  constexpr int S = W::S;
  constexpr int XS = G::STRIDE;  // exchange doubles per transform
  // LDS: the exchange regions, the window, and the twiddle bases
  __shared__ double lds[W::WPB * S * XS + F + 2 * W::TWN];
  const int lt = (int)threadIdx.x;
  const int w = W::WAVE ? lt >> 6 : 0, lane = W::WAVE ? lt & 63 : lt;
  const int s = lane / T, t = lane % T;
  double *const lre = lds + (w * S + s) * XS;
  double *const wl = lds + W::WPB * S * XS;
  cd *const twl = reinterpret_cast<cd *>(wl + F);
  for (int i = lt; i < F; i += W::BLOCK) wl[i] = win[i];
  for (int i = lt; i < W::TWN; i += W::BLOCK) twl[i] = tw[i];
  __syncthreads();
  // the worker, its channel and its group range: uniform over its waves. The
  // last workgroup's workers past channels * wpc have nothing to do (the
  // kernel's only workgroup barrier at WPB > 1 is the one above).
  const int64_t worker = (int64_t)blockIdx.x * W::WPB + __builtin_amdgcn_readfirstlane(w);
  const int64_t chan = worker / wpc;
  if (chan >= channels) return;
  x += chan * ldx;
  const int64_t npairs = (seg_end - seg_begin + 1) / 2;
  const int64_t ngroups = (npairs + S - 1) / S;
  const int64_t g0 = (worker - chan * wpc) * groups_per_worker;
  const int64_t gend = g0 + groups_per_worker < ngroups ? g0 + groups_per_worker : ngroups;
  // [g0, gm): full groups (each of the S pairs exists and has its partner),
  // run without masks; [gm, gend): at most the channel's last group, masked
  const int64_t gfull = (seg_end - seg_begin) / 2 / S;
  const int64_t gm = PAD ? g0 : (gend < gfull ? gend : (g0 > gfull ? g0 : gfull));
  double acc[E];
#pragma unroll
  for (int k = 0; k < E; ++k) acc[k] = 0.0;
  constexpr int NB = HALF ? H : E;  // second-segment samples loaded (HALF: its new half)
  auto run = [&](const double (&a)[E], const double (&b)[NB], bool ina_all, bool inb_all,
                 bool active, bool has1) {
    const int tt = opaque_int(t);
    cd v[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int i = t + k * T;
      const double wk = wl[tt + k * T];
      double ak = a[k], bk = HALF ? (k < H ? a[k + H] : b[k - H]) : b[k];
      if (!ina_all) ak = active && (!PAD || i < nfft) ? ak : 0.0;
      if (!inb_all) bk = has1 && (!PAD || i < nfft) ? bk : 0.0;
      v[k] = {ak * wk, bk * wk};
    }
    fft_regs<LOG2F, true, 2, 4, 0, 0, const cd *, 1, 0, NoEpi, 0, 16, W::WAVE>(v, tt, twl, lre,
                                                                              lre, false);
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = fma(v[k].y, v[k].y, fma(v[k].x, v[k].x, acc[k]));
  };
  // Full groups: 2 S consecutive segments from one wave-uniform base, every
  // load a buffer load from a scalar descriptor, the lane's loop-invariant
  // offset and a compile-time one.
  const uint32_t loff = (uint32_t)((2 * s * stride + t) * 8);
  auto load_full = [&](int64_t g, double (&a)[E], double (&b)[NB]) {
    const rsrc_t r = make_rsrc(x + (seg_begin + 2 * g * S) * stride, 0x7fffffff);
    const int sb = (int)(stride * 8);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      constexpr int kMaxImm = 4095;
      const int c = k * T * 8;
      a[k] = buf_ld1s(r, loff + (c <= kMaxImm ? c : 0), c <= kMaxImm ? 0 : c);
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      constexpr int kMaxImm = 4095;
      const int c = (HALF ? k + H : k) * T * 8;
      b[k] = buf_ld1s(r, loff + (c <= kMaxImm ? c : 0), sb + (c <= kMaxImm ? 0 : c));
    }
  };
  if constexpr (!PAD) {
    for (int64_t g = g0; g < gm; ++g) {
      double a[E], b[NB];
      load_full(g, a, b);
      run(a, b, true, true, true, true);
    }
  }
  // The masked groups: unconditional loads from clamped addresses inside the
  // channel (a slot past the pairs reads the last pair, a missing partner
  // reads segment s0 again, elements past nfft read element nfft - 1), the
  // mask applied where the samples are used.
  for (int64_t g = gm; g < gend; ++g) {
    const int64_t p = g * S + s;
    const bool active = p < npairs;
    const int64_t s0 = seg_begin + 2 * (active ? p : npairs - 1);
    const bool has1 = active && s0 + 1 < seg_end;
    const double *xa = opaque_ptr(x) + s0 * stride;
    const double *xb = has1 ? xa + stride : xa;
    double a[E], b[NB];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int i = t + k * T;
      a[k] = xa[!PAD || i < nfft ? i : nfft - 1];
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int i = t + (HALF ? k + H : k) * T;
      b[k] = xb[!PAD || i < nfft ? i : nfft - 1];
    }
    run(a, b, false, false, active, has1);
  }
  // every slot writes its row (zeros for a slot with no pairs): the reduce
  // sums all wpc * S rows of the channel
  double *dst = partial + (worker * S + s) * (int64_t)F;
#pragma unroll
  for (int k = 0; k < E; ++k) dst[t + k * T] = acc[k];
}

// Deterministic reduction of the channels' partial rows, the order of
// reduce_partials_l1 / l2 per channel: level 1 sums fixed chunks of 64 rows
// per bin, level 2 sums `nrows` rows (the chunk sums, or the partial rows
// themselves where a channel has at most one chunk) in order and adds into
// acc + c F. One thread per (channel, [chunk,] bin), flattened in the grid's
// x: F is a multiple of 64, so a wave stays in one row.
constexpr int kPwbChunk = 64;
__global__ __launch_bounds__(256) void reduce_batch_l1(const double *__restrict__ partial,
                                                       int64_t channels, int64_t rows,
                                                       int64_t nchunks, int F,
                                                       double *__restrict__ chunk_sums) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= channels * nchunks * F) return;
  const int k = (int)(i % F);
  const int64_t cc = i / F, c = cc / nchunks, ch = cc % nchunks;
  const int64_t r0 = ch * kPwbChunk;
  const int64_t r1 = r0 + kPwbChunk < rows ? r0 + kPwbChunk : rows;
  const double *p = partial + (c * rows + r0) * F + k;
  double s = 0.0;
  if (r1 - r0 == kPwbChunk) {
    double v[kPwbChunk];
#pragma unroll
    for (int j = 0; j < kPwbChunk; ++j) v[j] = p[(int64_t)j * F];
#pragma unroll
    for (int j = 0; j < kPwbChunk; ++j) s += v[j];
  } else {
    for (int64_t r = r0; r < r1; ++r, p += F) s += *p;
  }
  chunk_sums[i] = s;
}

__global__ __launch_bounds__(256) void reduce_batch_l2(const double *__restrict__ rows_in,
                                                       int64_t channels, int64_t nrows, int F,
                                                       double *__restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= channels * F) return;
  const int k = (int)(i % F);
  const int64_t c = i / F;
  const double *p = rows_in + c * nrows * F + k;
  double s = 0.0;
  int64_t r = 0;
  for (; r + 8 <= nrows; r += 8) {  // eight loads in flight, summed in order
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[(r + j) * F];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; r < nrows; ++r) s += p[r * F];
  acc[i] += s;
}

// gdsp_pwelch_finalize's arithmetic (spectral/pwelch.go:113-142) per channel:
// the same operations in the same order (a sum, a product by 0.5, a
// division, a doubling, a division: nothing an FMA could absorb), so the
// result equals the host's bit for bit.
__global__ __launch_bounds__(256) void pwelch_finalize_kernel(const double *__restrict__ acc,
                                                              int64_t channels, int64_t flen,
                                                              int64_t lp, int64_t nsegs,
                                                              double norm,
                                                              double *__restrict__ pxx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= channels * lp) return;
  const int64_t c = i / lp, j = i % lp;
  const double *a = acc + c * flen;
  double d = 0.0;
  if (nsegs > 0) {
    d = 0.5 * (a[j] + a[(flen - j) % flen]) / (double)nsegs;
    if (j > 0 && j < lp - 1) d *= 2;
  }
  pxx[i] = d / norm;
}

template <int LOG2F, bool HALF, bool PAD>
static hipError_t launch_pwb_t(const double *x, int64_t ldx, int64_t channels, int64_t wpc,
                               int64_t nfft, int64_t stride, int64_t seg_begin, int64_t seg_end,
                               int64_t gpw, const double *win, const cd *tw, double *partial,
                               hipStream_t s) {
  constexpr int WPB = PwbGeo<LOG2F>::WPB;
  const int64_t nblk = (channels * wpc + WPB - 1) / WPB;
  if (nblk < 1 || nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((pwelch_batch_kernel<LOG2F, HALF, PAD>), dim3((unsigned)nblk),
                     dim3(PwbGeo<LOG2F>::BLOCK), 0, s, x, ldx, channels, wpc, nfft, stride,
                     seg_begin, seg_end, gpw, win, tw, partial);
  return hipGetLastError();
}

bool pwelch_batch_applies(int log2f) { return log2f >= 6 && log2f <= 11; }

// Workers per channel, pair groups per worker and partial rows per channel.
// The workers of the whole job are what pwelch_wave_geometry gives a single
// signal (two or three waves per SIMD: its comments), shared by the channels
// and capped by a channel's groups; at least one per channel.
void pwelch_batch_geometry(int log2f, bool half, int64_t channels, int64_t nsegs, int64_t *wpc,
                           int64_t *gpw, int64_t *rows) {
  const int T = (1 << log2f) / 16;
  const bool wave = T <= 64;
  const int S = wave ? 64 / T : 1;
  const int64_t npairs = (nsegs + 1) / 2;
  int64_t ngroups = (npairs + S - 1) / S;
  if (ngroups < 1) ngroups = 1;
  const int64_t target = !wave ? 1024 : half && log2f >= 7 ? 3072 : 2048;
  int64_t want = channels > 0 ? target / channels : target;
  if (want < 1) want = 1;
  if (want > ngroups) want = ngroups;
  const int64_t g = (ngroups + want - 1) / want;
  *gpw = g;
  *wpc = (ngroups + g - 1) / g;
  *rows = *wpc * S;
}

hipError_t launch_pwelch_batch(int log2f, bool half, const double *x, int64_t ldx,
                               int64_t channels, int64_t wpc, int64_t nfft, int64_t stride,
                               int64_t seg_begin, int64_t seg_end, int64_t gpw, const double *win,
                               const cd *tw, double *partial, hipStream_t s) {
  if (channels < 1 || wpc < 1 || gpw < 1) return hipErrorInvalidValue;
  switch (log2f) {
#define GDSP_PWB(L)                                                                              \
  case L:                                                                                        \
    return half ? launch_pwb_t<L, true, false>(x, ldx, channels, wpc, nfft, stride, seg_begin,  \
                                               seg_end, gpw, win, tw, partial, s)               \
           : nfft < (1 << L)                                                                     \
               ? launch_pwb_t<L, false, true>(x, ldx, channels, wpc, nfft, stride, seg_begin,   \
                                              seg_end, gpw, win, tw, partial, s)                \
               : launch_pwb_t<L, false, false>(x, ldx, channels, wpc, nfft, stride, seg_begin,  \
                                               seg_end, gpw, win, tw, partial, s);
    GDSP_PWB(6) GDSP_PWB(7) GDSP_PWB(8) GDSP_PWB(9) GDSP_PWB(10) GDSP_PWB(11)
#undef GDSP_PWB
    default: return hipErrorInvalidValue;
  }
}

int64_t reduce_batch_scratch_doubles(int64_t channels, int64_t rows, int64_t F) {
  const int64_t nchunks = (rows + kPwbChunk - 1) / kPwbChunk;
  return nchunks > 1 ? channels * nchunks * F : 0;
}

hipError_t launch_reduce_batch(const double *partial, int64_t channels, int64_t rows, int64_t F,
                               double *acc, double *scratch, hipStream_t s) {
  const int64_t nchunks = (rows + kPwbChunk - 1) / kPwbChunk;
  const int64_t n1 = channels * nchunks * F, n2 = channels * F;
  if (channels < 1 || rows < 1 || (n1 + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
  if (nchunks > 1) {
    hipLaunchKernelGGL(reduce_batch_l1, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s,
                       partial, channels, rows, nchunks, (int)F, scratch);
    hipLaunchKernelGGL(reduce_batch_l2, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s,
                       scratch, channels, nchunks, (int)F, acc);
  } else {
    hipLaunchKernelGGL(reduce_batch_l2, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s,
                       partial, channels, rows, (int)F, acc);
  }
  return hipGetLastError();
}

hipError_t launch_pwelch_finalize(const double *acc, int64_t channels, int64_t flen, int64_t lp,
                                  int64_t nsegs, double norm, double *pxx, hipStream_t s) {
  const int64_t n = channels * lp;
  if (n < 1 || (n + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pwelch_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     acc, channels, flen, lp, nsegs, norm, pxx);
  return hipGetLastError();
}

}  // namespace gdsp
