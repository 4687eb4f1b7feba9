// stft_batch.hip — the per-segment spectra of a planar batch: for every
// channel c and segment s the first lp bins of X_s, the F-point transform of
// segment s windowed and zero-padded as spectral.Pwelch forms it
// (spectral/pwelch.go:104-111), stored as a row of the caller's
// [channel][segment][lp] layout: complex128 X_s[j] (the STFT), or float64
// c_j |X_s[j]|^2 / norm (POWER: the spectrogram). A sibling of
// pwelch_batch.hip for the same lengths (F = max(Pad, NFFT) a power of 2 from
// 64 to 2048) with its worker / channel geometry, its packed segment pairs
// z = w x_s + i a w x_(s+1), its buffer loads of full groups and its masked
// tail of clamped in-channel loads; and of cpsd_batch.hip, whose mirror
// exchange separates the two real spectra of one transform inside the
// transform's own exchange region:
//   2 X_s[j] = Z_j + conj Z_(F-j),  2 a X_(s+1)[j] = (Z_j - conj Z_(F-j)) / i.
// Nothing is summed: there are no partials and no reduce. The epilogue stores
// bins t + k T, k < 8, of both segments (consecutive lanes, consecutive bins:
// 16-byte stores, 8-byte in power mode) and lane 0 bin F / 2, masked to
// j < lp, each row from a 64-bit base.
//
// What a sum forgives and a row does not:
//
// Balance. The transform's roundoff is relative to the louder of its two
// segments, so a quiet segment beside a loud one (a fade-in, a channel switched
// on late) would lose that many digits in its own row. Every pair has cpsd's
// power of 2, a = 2^(e_s - e_(s+1)) from the binary exponents of max |w x_s|
// and max |w x_(s+1)|, clamped to +-1022, 1 where a maximum is zero, subnormal
// or not finite; segment s + 1 is packed times a and its row multiplied by
// 1 / a, both exact. The exponents are reduced as integers (the high words of
// |v|), so a NaN counts as 2047 like an infinity: fmax would drop it.
//
// Zeros. A segment whose every sample is an exact zero gives a row of exact
// zeros, not its partner's roundoff: its row is multiplied by 0 (cpsd's ox /
// ia).
//
// Containment. The separation would carry a NaN or an infinity of one segment
// into its partner's row. A group in which any pair holds a non-finite maximum
// (a wave-uniform vote on the exponents the balance computed; workgroup-uniform
// at F = 2048) stores nothing from the packed transform and runs twice more:
// the even segments alone (the partner masked to zero, only row s stored),
// then the odd ones alone. Rare, so its cost does not matter; every other
// group's rows keep their bits.
//
// Every other length, strides above 2^22 and GDSP_ALGO_NO_FUSED_STFT run the
// materialised form below: gathered real rows w x_s, the plan's batched
// transform of real rows (one segment per transform: no balance needed, zeros
// and containment for free), and a kernel that writes the first lp bins or
// their scaled powers.
#include <type_traits>

#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

constexpr int kStbWaves = 4;  // waves per workgroup

// the balance's range in binary orders (cpsd_batch.hip, kCpsdMaxDe)
constexpr int kStftMaxDe = 1022;
__device__ constexpr int stft_clamp_de(int d) {
  return d < -kStftMaxDe ? -kStftMaxDe : (d > kStftMaxDe ? kStftMaxDe : d);
}

// a lane's 64-bit offset the compiler may not trace (opaque_int's purpose)
__device__ __forceinline__ int64_t opaque_i64(int64_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <int LOG2F>
struct StbGeo {
  using G = Geo<LOG2F>;
  static constexpr int T = G::T;
  static constexpr bool WAVE = T <= 64;
  static constexpr int S = WAVE ? 64 / T : 1;       // transforms (pairs) per worker
  static constexpr int WPB = WAVE ? kStbWaves : 1;  // workers per workgroup
  static constexpr int BLOCK = WAVE ? 64 * kStbWaves : T;
  static constexpr int TWN = G::N / G::radix(G::NPASS - 1);
};

template <int LOG2F, bool PAD, bool POWER>
__global__ __launch_bounds__((StbGeo<LOG2F>::BLOCK))
__attribute__((amdgpu_waves_per_eu(2))) void stft_batch_kernel(
    const double *__restrict__ x, int64_t ldx, int64_t channels, int64_t wpc, int64_t nfft,
    int64_t stride, int64_t seg_begin, int64_t seg_end, int64_t groups_per_worker,
    const double *__restrict__ win, const cd *__restrict__ tw,
    typename std::conditional<POWER, double, cd>::type *__restrict__ out, int lp, int64_t ld_seg,
    int64_t ld_chan, double norm) {
  using G = Geo<LOG2F>;
  using W = StbGeo<LOG2F>;
  using OutT = typename std::conditional<POWER, double, cd>::type;
  constexpr int E = G::E, T = G::T, F = G::N, H = E / 2;
  static_assert(E == 16 && (T <= 64 ? 64 % T == 0 : T == 128), "one transform per wave or two waves");
  constexpr int S = W::S;
  constexpr int XS = G::STRIDE;  // exchange doubles per transform
  static_assert(XS >= F, "the mirror exchange uses F slots of the region");
  // LDS: the exchange regions, the window, the twiddle bases, and (two-wave
  // workers) each wave's exponent pair for the balance
  __shared__ double lds[W::WPB * S * XS + F + 2 * W::TWN + (W::WAVE ? 0 : 2)];
  const int lt = (int)threadIdx.x;
  const int w = W::WAVE ? lt >> 6 : 0, lane = W::WAVE ? lt & 63 : lt;
  const int s = lane / T, t = lane % T;
  double *const lre = lds + (w * S + s) * XS;
  double *const wl = lds + W::WPB * S * XS;
  cd *const twl = reinterpret_cast<cd *>(wl + F);
  for (int i = lt; i < F; i += W::BLOCK) wl[i] = win[i];
  for (int i = lt; i < W::TWN; i += W::BLOCK) twl[i] = tw[i];
  __syncthreads();
  // the worker, its channel and its group range: uniform over its waves
  // (pwelch_batch.hip; the barrier above is the only one all workers share)
  const int64_t worker = (int64_t)blockIdx.x * W::WPB + __builtin_amdgcn_readfirstlane(w);
  const int64_t chan = worker / wpc;
  if (chan >= channels) return;
  x += chan * ldx;
  out += chan * ld_chan;
  const int nf = (int)nfft;  // <= F
  const int64_t nseg = seg_end - seg_begin;
  const int64_t npairs = (nseg + 1) / 2;
  const int64_t ngroups = (npairs + S - 1) / S;
  const int64_t g0 = (worker - chan * wpc) * groups_per_worker;
  const int64_t gend = g0 + groups_per_worker < ngroups ? g0 + groups_per_worker : ngroups;
  // [g0, gm): full groups (each of the S pairs exists and has its partner),
  // run without masks; [gm, gend): at most the channel's last group, masked
  const int64_t gfull = nseg / 2 / S;
  const int64_t gm = PAD ? g0 : (gend < gfull ? gend : (g0 > gfull ? g0 : gfull));
  // One packed transform of group g and its two rows per slot. mode 0: both
  // segments; 1: the even segment alone, 2: the odd one alone (a group that
  // holds a non-finite sample). Returns the mode to run the group in next
  // (0: done), the same value in every lane of the worker.
  auto run = [&](const double (&a)[E], const double (&b)[E], bool all, bool active, bool has1,
                 int64_t g, int mode) -> int {
    const int tt = opaque_int(t);
    const bool ka = mode != 2, kb = mode != 1;
    cd v[E];
    int mhx = 0, mhy = 0, lox = 0, loy = 0;  // max of the high words of |v|, or of the low ones
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int i = t + k * T;
      const double wk = wl[tt + k * T];
      double ak = a[k], bk = b[k];
      if (!all) {
        ak = active && (!PAD || i < nf) ? ak : 0.0;
        bk = has1 && (!PAD || i < nf) ? bk : 0.0;
      }
      ak = ka ? ak : 0.0;
      bk = kb ? bk : 0.0;
      v[k] = {ak * wk, bk * wk};
      mhx = max(mhx, __double2hiint(v[k].x) & 0x7fffffff);
      mhy = max(mhy, __double2hiint(v[k].y) & 0x7fffffff);
      lox |= __double2loint(v[k].x);
      loy |= __double2loint(v[k].y);
    }
    // biased exponents of max |w x_s| and max |w x_(s+1)| over the transform
    // (-1: every sample an exact zero, 0: subnormal, 2047: not finite)
    int ex = (mhx | lox) == 0 ? -1 : mhx >> 20;
    int ey = (mhy | loy) == 0 ? -1 : mhy >> 20;
#pragma unroll
    for (int m = 1; m < (W::WAVE ? T : 64); m <<= 1) {
      ex = max(ex, __shfl_xor(ex, m));
      ey = max(ey, __shfl_xor(ey, m));
    }
    if constexpr (!W::WAVE) {
      // the worker's two waves: one pair each, behind the barrier
      int *const xe = reinterpret_cast<int *>(lds + W::WPB * S * XS + F + 2 * W::TWN);
      if ((lt & 63) == 0) {
        xe[2 * (lt >> 6)] = ex;
        xe[2 * (lt >> 6) + 1] = ey;
      }
      __syncthreads();
      ex = max(xe[0], xe[2]);
      ey = max(xe[1], xe[3]);
    }
    if (mode == 0) {
      // containment: any pair of the group with a non-finite segment
      const bool bad = __any(ex == 2047 || ey == 2047) != 0;
      if (bad) {
        if constexpr (!W::WAVE) __syncthreads();  // the exponent pairs are written again
        return 1;
      }
    }
    const bool bal = ex > 0 && ey > 0 && ex < 2047 && ey < 2047;
    const int de = !bal ? 0 : stft_clamp_de(ex - ey);
    const double al = __hiloint2double((1023 + de) << 20, 0);
    // an all-zero segment: exact zeros for its row, not the partner's roundoff
    const double ia = ey < 0 ? 0.0 : __hiloint2double((1023 - de) << 20, 0);
    const double ox = ex < 0 ? 0.0 : 1.0;
#pragma unroll
    for (int k = 0; k < E; ++k) v[k].y *= al;
    fft_regs<LOG2F, true, 2, 4, 0, 0, const cd *, 1, 0, NoEpi, 0, 16, W::WAVE>(v, tt, twl, lre,
                                                                              lre, false);
    // the mirror exchange (cpsd_batch.hip): upper-half bins into slots bin -
    // F/2 (real) and bin (imaginary), after every lane of the transform has
    // read its last pass's exchange
    xsync<W::WAVE>();
#pragma unroll
    for (int k = H; k < E; ++k) {
      lre[tt + (k - H) * T] = v[k].x;
      lre[F / 2 + tt + (k - H) * T] = v[k].y;
    }
    xsync<W::WAVE>();
    // the rows of this slot's pair: segments 2 p and 2 p + 1 of the range
    const int64_t p = g * S + s;
    const bool st0 = active && ka, st1 = has1 && kb;
    OutT *const r0 = out + 2 * p * ld_seg;
    OutT *const r1 = r0 + ld_seg;
    auto store = [&](int j, bool inner, double px, double qx, double cy, double dy) {
      // X_s = (px + i qx) / 2, X_(s+1) = (cy + i dy) / (2 a)
      const double xr = 0.5 * px * ox, xi = 0.5 * qx * ox;
      const double yr = 0.5 * cy * ia, yi = 0.5 * dy * ia;
      if (j >= lp) return;
      if constexpr (POWER) {
        // gdsp_pwelch_finalize's order: the square sum, the doubling, the division
        double u = fma(xi, xi, xr * xr), z = fma(yi, yi, yr * yr);
        if (inner && j < lp - 1) {
          u *= 2;
          z *= 2;
        }
        if (st0) __builtin_nontemporal_store(u / norm, r0 + j);
        if (st1) __builtin_nontemporal_store(z / norm, r1 + j);
      } else {
        if (st0) st_nt(r0 + j, cd{xr, xi});
        if (st1) st_nt(r1 + j, cd{yr, yi});
      }
    };
    // the mirrors first (one run of LDS reads), then bin by bin: the fence
    // keeps the scheduler from forming every row value and address before the
    // first store, which costs more registers than the transform itself
    cd mir[H];
#pragma unroll
    for (int k = 0; k < H; ++k) {
      mir[k] = v[k];  // bin 0 mirrors itself
      if (k > 0) {
        mir[k] = {lre[F / 2 - tt - k * T], lre[F - tt - k * T]};
      } else {
        const int o = tt == 0 ? 0 : F / 2 - tt;
        const double rx = lre[o], ry = lre[F / 2 + o];
        mir[k].x = tt == 0 ? mir[k].x : rx;  // per component: a select of the struct goes through scratch
        mir[k].y = tt == 0 ? mir[k].y : ry;
      }
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const cd m = mir[k];
      store(t + k * T, k > 0 || t > 0, v[k].x + m.x, v[k].y - m.y, v[k].y + m.y, m.x - v[k].x);
      __builtin_amdgcn_sched_barrier(0);
    }
    // bin F / 2 (lane 0's register 8) mirrors itself: imaginary parts exactly 0
    if (t == 0) store(F / 2, true, v[H].x + v[H].x, 0.0, v[H].y + v[H].y, 0.0);
    return mode == 1 ? 2 : 0;
  };
  // Full groups: 2 S consecutive segments from one wave-uniform base, every
  // load a buffer load from a scalar descriptor, the lane's loop-invariant
  // offset and a compile-time one (pwelch_batch.hip).
  const uint32_t loff = (uint32_t)((2 * s * stride + t) * 8);
  if constexpr (!PAD) {
    for (int64_t g = g0; g < gm; ++g) {
      int mode = 0;
      do {
        const rsrc_t r = make_rsrc(x + (seg_begin + 2 * g * S) * stride, 0x7fffffff);
        const int sb = (int)(stride * 8);
        double a[E], b[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
          constexpr int kMaxImm = 4095;
          const int c = k * T * 8;
          a[k] = buf_ld1s(r, loff + (c <= kMaxImm ? c : 0), c <= kMaxImm ? 0 : c);
          b[k] = buf_ld1s(r, loff + (c <= kMaxImm ? c : 0), sb + (c <= kMaxImm ? 0 : c));
        }
        mode = run(a, b, true, true, true, g, mode);
      } while (mode != 0);
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
    const int64_t oa = s0 * stride, ob = has1 ? oa + stride : oa;
    int mode = 0;
    do {
      // opaque per run: hoisted out of this loop, the 32 element addresses
      // would stay live through the transform
      const double *xa = x + opaque_i64(oa);
      const double *xb = x + opaque_i64(ob);
      double a[E], b[E];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int i = t + k * T;
        const int ii = !PAD || i < nf ? i : nf - 1;
        a[k] = xa[ii];
        b[k] = xb[ii];
      }
      mode = run(a, b, false, active, has1, g, mode);
    } while (mode != 0);
  }
}

// ---- the materialised form ---------------------------------------------------
// Row r = c * ns + j of buf: w x of segment seg0 + j of channel c as flen
// float64, zero past nfft.
__global__ __launch_bounds__(256) void stft_gather_kernel(
    const double *__restrict__ x, int64_t ldx, int64_t channels, int64_t ns, int64_t nfft,
    int64_t flen, int64_t stride, int64_t seg0, const double *__restrict__ win,
    double *__restrict__ buf) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= channels * ns * flen) return;
  const int64_t r = tid / flen, i = tid - r * flen;
  const int64_t c = r / ns, j = r - c * ns;
  buf[tid] = i < nfft ? x[c * ldx + (seg0 + j) * stride + i] * win[i] : 0.0;
}

// The first lp bins of transformed row r = c * ns + j into row (c, row0 + j)
// of the caller's layout: as they are (bins 0 and flen / 2 of a real row's
// transform are real: their imaginary parts are stored as exact zeros, as the
// fused kernel's), or their powers scaled in the fused kernel's order.
template <bool POWER>
__global__ __launch_bounds__(256) void stft_rows_kernel(
    const cd *__restrict__ buf, int64_t channels, int64_t ns, int64_t flen, int64_t lp, double norm,
    typename std::conditional<POWER, double, cd>::type *__restrict__ out, int64_t row0,
    int64_t ld_seg, int64_t ld_chan) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= channels * ns * lp) return;
  const int64_t r = tid / lp, j = tid - r * lp;
  const int64_t c = r / ns, sj = r - c * ns;
  cd z = buf[r * flen + j];
  if (j == 0 || 2 * j == flen) z.y = 0.0;
  const int64_t o = c * ld_chan + (row0 + sj) * ld_seg + j;
  if constexpr (POWER) {
    double u = fma(z.y, z.y, z.x * z.x);
    if (j > 0 && j < lp - 1) u *= 2;
    out[o] = u / norm;
  } else {
    out[o] = z;
  }
}

template <int LOG2F, bool PAD, bool POWER>
static hipError_t launch_stb_t(const double *x, int64_t ldx, int64_t channels, int64_t wpc,
                               int64_t nfft, int64_t stride, int64_t seg_begin, int64_t seg_end,
                               int64_t gpw, const double *win, const cd *tw, void *out, int64_t lp,
                               int64_t ld_seg, int64_t ld_chan, double norm, hipStream_t s) {
  using OutT = typename std::conditional<POWER, double, cd>::type;
  constexpr int WPB = StbGeo<LOG2F>::WPB;
  const int64_t nblk = (channels * wpc + WPB - 1) / WPB;
  if (nblk < 1 || nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((stft_batch_kernel<LOG2F, PAD, POWER>), dim3((unsigned)nblk),
                     dim3(StbGeo<LOG2F>::BLOCK), 0, s, x, ldx, channels, wpc, nfft, stride,
                     seg_begin, seg_end, gpw, win, tw, (OutT *)out, (int)lp, ld_seg, ld_chan, norm);
  return hipGetLastError();
}

bool stft_batch_applies(int log2f) { return log2f >= 6 && log2f <= 11; }

// Workers per channel and pair groups per worker: pwelch_batch_geometry's rule
// (the workers of the whole job shared by the channels, capped by a channel's
// groups, at least one per channel), without partial rows.
void stft_batch_geometry(int log2f, int64_t channels, int64_t nsegs, int64_t *wpc, int64_t *gpw) {
  const int T = (1 << log2f) / 16;
  const bool wave = T <= 64;
  const int S = wave ? 64 / T : 1;
  const int64_t npairs = (nsegs + 1) / 2;
  int64_t ngroups = (npairs + S - 1) / S;
  if (ngroups < 1) ngroups = 1;
  const int64_t target = wave ? 2048 : 1024;
  int64_t want = channels > 0 ? target / channels : target;
  if (want < 1) want = 1;
  if (want > ngroups) want = ngroups;
  const int64_t g = (ngroups + want - 1) / want;
  *gpw = g;
  *wpc = (ngroups + g - 1) / g;
}

hipError_t launch_stft_batch(int log2f, bool power, const double *x, int64_t ldx, int64_t channels,
                             int64_t wpc, int64_t nfft, int64_t stride, int64_t seg_begin,
                             int64_t seg_end, int64_t gpw, const double *win, const cd *tw,
                             void *out, int64_t lp, int64_t ld_seg, int64_t ld_chan, double norm,
                             hipStream_t s) {
  if (channels < 1 || wpc < 1 || gpw < 1 || seg_end <= seg_begin || lp < 1 ||
      lp > ((int64_t)1 << log2f) / 2 + 1 || ld_seg < lp)
    return hipErrorInvalidValue;
  switch (log2f) {
#define GDSP_STB_P(L, PAD)                                                                       \
  (power ? launch_stb_t<L, PAD, true>(x, ldx, channels, wpc, nfft, stride, seg_begin, seg_end,  \
                                      gpw, win, tw, out, lp, ld_seg, ld_chan, norm, s)          \
         : launch_stb_t<L, PAD, false>(x, ldx, channels, wpc, nfft, stride, seg_begin, seg_end, \
                                       gpw, win, tw, out, lp, ld_seg, ld_chan, norm, s))
#define GDSP_STB(L) \
  case L: return nfft < (1 << L) ? GDSP_STB_P(L, true) : GDSP_STB_P(L, false);
    GDSP_STB(6) GDSP_STB(7) GDSP_STB(8) GDSP_STB(9) GDSP_STB(10) GDSP_STB(11)
#undef GDSP_STB
#undef GDSP_STB_P
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_stft_gather(const double *x, int64_t ldx, int64_t channels, int64_t ns,
                              int64_t nfft, int64_t flen, int64_t stride, int64_t seg0,
                              const double *win, double *buf, hipStream_t s) {
  const int64_t n = channels * ns * flen;
  if (n < 1 || (n + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stft_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx,
                     channels, ns, nfft, flen, stride, seg0, win, buf);
  return hipGetLastError();
}

hipError_t launch_stft_rows(const cd *buf, int64_t channels, int64_t ns, int64_t flen, int64_t lp,
                            bool power, double norm, void *out, int64_t row0, int64_t ld_seg,
                            int64_t ld_chan, hipStream_t s) {
  const int64_t n = channels * ns * lp;
  if (n < 1 || (n + 255) / 256 > 0x7fffffff || lp > flen || ld_seg < lp)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (power)
    hipLaunchKernelGGL(stft_rows_kernel<true>, grid, dim3(256), 0, s, buf, channels, ns, flen, lp,
                       norm, (double *)out, row0, ld_seg, ld_chan);
  else
    hipLaunchKernelGGL(stft_rows_kernel<false>, grid, dim3(256), 0, s, buf, channels, ns, flen, lp,
                       norm, (cd *)out, row0, ld_seg, ld_chan);
  return hipGetLastError();
}

}  // namespace gdsp
