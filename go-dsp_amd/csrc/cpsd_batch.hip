// cpsd_batch.hip — the fused cross-spectral accumulation over the channels of
// a planar batch: for every channel c the sums over its segments s of
//   Sxx[j] = |X_s[j]|^2, Syy[j] = |Y_s[j]|^2, Sxy[j] = conj(X_s[j]) Y_s[j]
// for the bins j <= F / 2, where X_s and Y_s are the spectra spectral.Pwelch
// forms of segment s of x and of y (spectral/pwelch.go:104-112). A sibling of
// pwelch_batch.hip for the same lengths (F = max(Pad, NFFT) a power of 2 from
// 64 to 2048), with its worker / channel geometry, its wave-private exchanges
// and its masked tail of clamped in-channel loads.
//
// One transform carries both signals: z = w x_s + i w y_s, so
//   X_j = (Z_j + conj Z_(F-j)) / 2,  Y_j = (Z_j - conj Z_(F-j)) / (2 i).
// A worker's slot is therefore one segment of both signals (not a pair of
// segments), a group is S segments, and nothing but true per-segment sums
// reaches the accumulators.
//
// The mirror. After fft_regs the thread holds bins t + k T, k < 16. The
// mirror F - j of bin j = t + k T, 0 < j < F / 2 (k < 8), is bin (T - t) % T +
// k' T of the same transform with k' = 15 - k (t > 0) or 16 - k (t = 0): an
// upper-half bin of another lane. The upper halves (registers 8..15) go
// through the transform's own exchange region, free after the last pass:
// real parts at slots [0, F/2), imaginary parts at [F/2, F), slot = bin -
// F/2, and bin j reads slot F/2 - j. Bins 0 and F/2 are their own mirrors
// and use the thread's registers, so their Im Sxy is an exact zero.
//
// Balance. The transform's roundoff is relative to |Z|, the larger of the two
// spectra, so a y segment far below its x segment (or the reverse) would lose
// that many digits. Every transform therefore has a power of 2 of its own,
// alpha = 2^(e_x - e_y) from the binary exponents of max |w x_s| and
// max |w y_s| of the very segment it packs (a reduction over the transform's
// lanes of values already in registers), packs alpha w y_s, and multiplies the
// two Y terms of every bin by 1 / alpha before they enter the sums. All these
// products are by powers of 2, exact, so alpha decides how evenly the roundoff
// falls on the two signals of that segment and nothing else; no segment's
// scale depends on another segment or on where a range begins.
//
// A segment of one signal whose every sample is an exact zero contributes exact
// zeros: its X (or Y) terms, which would otherwise be the transform's roundoff
// of the other signal, are multiplied by 0 instead of 1 (or 1 / alpha). A dead
// channel therefore has Pyy = Pxy = 0 and a coherence of 0 / 0.
//
// Partials are [channel][wpc * S rows][4][hb], hb = F / 2 + 1, planes Sxx,
// Syy, Re Sxy, Im Sxy; reduce_batch_l1 / l2 (pwelch_batch.hip) add each
// channel's rows into acc + c 4 hb in their fixed order with F := 4 hb.
//
// Every other length runs the materialised form below: a balance per row,
// gathered rows w x_s + i alpha w y_s, the plan's batched transform, and cpsd_partials_kernel
// over each row and its mirror.
#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

constexpr int kCpbWaves = 4;  // waves per workgroup

// The balance's range in binary orders: alpha = 2^de and 1 / alpha must be
// normal doubles, nothing else. Every product the balance forms (alpha w y
// at x's level going in, the Y terms times 1 / alpha at y's level coming out)
// has the size of one of the two signals' own spectra, so it leaves the normal
// range only where that signal's own sums do.
constexpr int kCpsdMaxDe = 1022;
__host__ __device__ constexpr int cpsd_clamp_de(int d) {
  return d < -kCpsdMaxDe ? -kCpsdMaxDe : (d > kCpsdMaxDe ? kCpsdMaxDe : d);
}

template <int LOG2F>
struct CpbGeo {
  using G = Geo<LOG2F>;
  static constexpr int T = G::T;
  static constexpr bool WAVE = T <= 64;
  static constexpr int S = WAVE ? 64 / T : 1;       // transforms (segments) per worker
  static constexpr int WPB = WAVE ? kCpbWaves : 1;  // workers per workgroup
  static constexpr int BLOCK = WAVE ? 64 * kCpbWaves : T;
  static constexpr int TWN = G::N / G::radix(G::NPASS - 1);
};

template <int LOG2F, bool PAD>
__global__ __launch_bounds__((CpbGeo<LOG2F>::BLOCK))
__attribute__((amdgpu_waves_per_eu(2))) void cpsd_batch_kernel(
    const double *__restrict__ x, int64_t ldx, const double *__restrict__ y, int64_t ldy,
    int64_t channels, int64_t wpc, int64_t nfft, int64_t stride, int64_t seg_begin,
    int64_t seg_end, int64_t groups_per_worker, const double *__restrict__ win,
    const cd *__restrict__ tw, double *__restrict__ partial) {
  using G = Geo<LOG2F>;
  using W = CpbGeo<LOG2F>;
  constexpr int E = G::E, T = G::T, F = G::N, H = E / 2, HB = F / 2 + 1;
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
  // the worker, its channel and its group range: uniform over its waves. At
  // WPB > 1 the barrier above is the kernel's only workgroup barrier (the
  // waves are independent workers with trip counts of their own); at WPB = 1
  // the two waves of the worker leave or stay together and run the same trips.
  const int64_t worker = (int64_t)blockIdx.x * W::WPB + __builtin_amdgcn_readfirstlane(w);
  const int64_t chan = worker / wpc;
  if (chan >= channels) return;
  x += chan * ldx;
  y += chan * ldy;  // ldy = 0: one y for every channel
  const int nf = (int)nfft;  // <= F
  const int64_t nseg = seg_end - seg_begin;
  const int64_t ngroups = (nseg + S - 1) / S;
  const int64_t g0 = (worker - chan * wpc) * groups_per_worker;
  const int64_t gend = g0 + groups_per_worker < ngroups ? g0 + groups_per_worker : ngroups;
  // [g0, gm): full groups (each of the S segments exists), run without masks;
  // [gm, gend): at most the channel's last group, masked
  const int64_t gfull = nseg / S;
  const int64_t gm = PAD ? g0 : (gend < gfull ? gend : (g0 > gfull ? g0 : gfull));
  // sums of (2 X, 2 Y) products: bins t + k T, k < 8, and bin F / 2 (lane 0's
  // register 8; the other lanes' copies are never stored)
  double sxx[H + 1], syy[H + 1], sre[H + 1], sim[H + 1];
#pragma unroll
  for (int k = 0; k <= H; ++k) sxx[k] = syy[k] = sre[k] = sim[k] = 0.0;
  auto run = [&](const double (&a)[E], const double (&b)[E], bool all, bool active) {
    const int tt = opaque_int(t);
    cd v[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int i = t + k * T;
      const double wk = wl[tt + k * T];
      double ak = a[k], bk = b[k];
      if (!all) {
        const bool in = active && (!PAD || i < nf);
        ak = in ? ak : 0.0;
        bk = in ? bk : 0.0;
      }
      v[k] = {ak * wk, bk * wk};
    }
    // the segment's balance: biased exponents of max |w x| and max |w y| over
    // the transform (-1: every sample an exact zero, 0: subnormal, 2047: not
    // finite; then alpha = 1), their difference held to +-kCpsdMaxDe
    double mx = 0.0, my = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      mx = fmax(mx, fabs(v[k].x));
      my = fmax(my, fabs(v[k].y));
    }
    int ex = mx == 0.0 ? -1 : __double2hiint(mx) >> 20;
    int ey = my == 0.0 ? -1 : __double2hiint(my) >> 20;
#pragma unroll
    for (int m = 1; m < (W::WAVE ? T : 64); m <<= 1) {
      ex = max(ex, __shfl_xor(ex, m));
      ey = max(ey, __shfl_xor(ey, m));
    }
    if constexpr (!W::WAVE) {
      // the worker's two waves: one pair each, behind the barrier. The next
      // transform writes its pair only after this one's exchanges' barriers.
      int *const xe = reinterpret_cast<int *>(lds + W::WPB * S * XS + F + 2 * W::TWN);
      if ((lt & 63) == 0) {
        xe[2 * (lt >> 6)] = ex;
        xe[2 * (lt >> 6) + 1] = ey;
      }
      __syncthreads();
      ex = max(xe[0], xe[2]);
      ey = max(xe[1], xe[3]);
    }
    const bool bal = ex > 0 && ey > 0 && ex < 2047 && ey < 2047;
    const int de = !bal ? 0 : cpsd_clamp_de(ex - ey);
    const double al = __hiloint2double((1023 + de) << 20, 0);
    // an all-zero segment: exact zeros for its terms, not the other signal's roundoff
    const double ia = ey < 0 ? 0.0 : __hiloint2double((1023 - de) << 20, 0);
    const double ox = ex < 0 ? 0.0 : 1.0;
#pragma unroll
    for (int k = 0; k < E; ++k) v[k].y *= al;
    fft_regs<LOG2F, true, 2, 4, 0, 0, const cd *, 1, 0, NoEpi, 0, 16, W::WAVE>(v, tt, twl, lre,
                                                                              lre, false);
    // the mirror exchange: upper-half bins into slots bin - F/2 (real) and
    // bin (imaginary), after every lane of the transform has read its last
    // pass's exchange
    xsync<W::WAVE>();
#pragma unroll
    for (int k = H; k < E; ++k) {
      lre[tt + (k - H) * T] = v[k].x;
      lre[F / 2 + tt + (k - H) * T] = v[k].y;
    }
    xsync<W::WAVE>();
#pragma unroll
    for (int k = 0; k <= H; ++k) {
      cd m = v[k];  // bins 0 and F / 2 mirror themselves
      if (k > 0 && k < H) {
        m = {lre[F / 2 - tt - k * T], lre[F - tt - k * T]};
      } else if (k == 0) {
        const int o = tt == 0 ? 0 : F / 2 - tt;
        const double rx = lre[o], ry = lre[F / 2 + o];
        m.x = tt == 0 ? m.x : rx;  // per component: a select of the struct goes through scratch
        m.y = tt == 0 ? m.y : ry;
      }
      const double p = (v[k].x + m.x) * ox, q = (v[k].y - m.y) * ox;  // 2 X
      const double c = (v[k].y + m.y) * ia, d = (m.x - v[k].x) * ia;  // 2 Y
      sxx[k] = fma(q, q, fma(p, p, sxx[k]));
      syy[k] = fma(d, d, fma(c, c, syy[k]));
      sre[k] = fma(q, d, fma(p, c, sre[k]));
      sim[k] += p * d - q * c;
    }
  };
  // Full groups: S consecutive segments of x and of y from one wave-uniform
  // base each, every load a buffer load from a scalar descriptor, the lane's
  // loop-invariant offset and a compile-time one.
  const uint32_t loff = (uint32_t)((s * stride + t) * 8);
  auto load_full = [&](int64_t g, double (&a)[E], double (&b)[E]) {
    const int64_t o = (seg_begin + g * S) * stride;
    const rsrc_t rx = make_rsrc(x + o, 0x7fffffff);
    const rsrc_t ry = make_rsrc(y + o, 0x7fffffff);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      constexpr int kMaxImm = 4095;
      const int c = k * T * 8;
      a[k] = buf_ld1s(rx, loff + (c <= kMaxImm ? c : 0), c <= kMaxImm ? 0 : c);
      b[k] = buf_ld1s(ry, loff + (c <= kMaxImm ? c : 0), c <= kMaxImm ? 0 : c);
    }
  };
  if constexpr (!PAD) {
    for (int64_t g = g0; g < gm; ++g) {
      double a[E], b[E];
      load_full(g, a, b);
      run(a, b, true, true);
    }
  }
  // The masked groups: unconditional loads from clamped addresses inside the
  // channel (a slot past the segments reads the last segment, elements past
  // nfft read element nfft - 1), the mask applied where the samples are used.
  for (int64_t g = gm; g < gend; ++g) {
    const int64_t p = g * S + s;
    const bool active = p < nseg;
    const int64_t o = (seg_begin + (active ? p : nseg - 1)) * stride;
    const double *xa = opaque_ptr(x) + o;
    const double *ya = opaque_ptr(y) + o;
    double a[E], b[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int i = t + k * T;
      const int ii = !PAD || i < nf ? i : nf - 1;  // 32-bit: a scalar base and a lane offset
      a[k] = xa[ii];
      b[k] = ya[ii];
    }
    run(a, b, false, active);
  }
  // every slot writes its row (zeros for a slot with no segments): the reduce
  // sums all wpc * S rows of the channel. The factor 1/4 of (2 X)(2 Y) is exact.
  double *dst = partial + (worker * S + s) * (int64_t)(4 * HB);
#pragma unroll
  for (int k = 0; k < H; ++k) {
    dst[t + k * T] = 0.25 * sxx[k];
    dst[HB + t + k * T] = 0.25 * syy[k];
    dst[2 * HB + t + k * T] = 0.25 * sre[k];
    dst[3 * HB + t + k * T] = 0.25 * sim[k];
  }
  if (t == 0) {
    dst[F / 2] = 0.25 * sxx[H];
    dst[HB + F / 2] = 0.25 * syy[H];
    dst[2 * HB + F / 2] = 0.25 * sre[H];
    dst[3 * HB + F / 2] = 0.25 * sim[H];
  }
}

// ---- the materialised form ---------------------------------------------------
// The balance of row r = c * ns + j (a block per row): alpha[r] = 2^(e_x - e_y),
// e the binary exponents of max |w x| and max |w y| over segment seg0 + j of
// channel c; 1 where either maximum is zero, subnormal or not finite. The
// difference is held to +-kCpsdMaxDe.
// A segment of all zeros is marked for cpsd_partials_kernel: alpha = 0 where
// y's is (its Y terms are exact zeros), -alpha where only x's is (its X terms).
__global__ __launch_bounds__(256) void cpsd_balance_kernel(
    const double *__restrict__ x, int64_t ldx, const double *__restrict__ y, int64_t ldy,
    int64_t ns, int64_t nfft, int64_t stride, int64_t seg0, const double *__restrict__ win,
    double *__restrict__ alpha) {
  __shared__ double mx[256], my[256];
  const int64_t r = blockIdx.x, c = r / ns, j = r - c * ns;
  const int64_t off = (seg0 + j) * stride;
  const int t = (int)threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int64_t i = t; i < nfft; i += 256) {
    a = fmax(a, fabs(x[c * ldx + off + i] * win[i]));
    b = fmax(b, fabs(y[c * ldy + off + i] * win[i]));
  }
  mx[t] = a;
  my[t] = b;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      mx[t] = fmax(mx[t], mx[t + h]);
      my[t] = fmax(my[t], my[t + h]);
    }
    __syncthreads();
  }
  if (t == 0) {
    const int ex = __double2hiint(mx[0]) >> 20, ey = __double2hiint(my[0]) >> 20;
    const bool bal = ex > 0 && ey > 0 && ex < 2047 && ey < 2047;
    const int de = !bal ? 0 : cpsd_clamp_de(ex - ey);
    const double al = __hiloint2double((1023 + de) << 20, 0);
    alpha[r] = my[0] == 0.0 ? 0.0 : (mx[0] == 0.0 ? -al : al);
  }
}

// Row r = c * ns + j of buf: w x + i |alpha[r]| w y of segment seg0 + j of
// channel c, zero past nfft.
__global__ __launch_bounds__(256) void cpsd_gather_kernel(
    const double *__restrict__ x, int64_t ldx, const double *__restrict__ y, int64_t ldy,
    int64_t channels, int64_t ns, int64_t nfft, int64_t flen, int64_t stride, int64_t seg0,
    const double *__restrict__ win, const double *__restrict__ alpha, cd *__restrict__ buf) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= channels * ns * flen) return;
  const int64_t r = tid / flen, i = tid - r * flen;
  const int64_t c = r / ns, j = r - c * ns;
  cd v = {0.0, 0.0};
  if (i < nfft) {
    const int64_t o = (seg0 + j) * stride + i;
    v = {x[c * ldx + o] * win[i], y[c * ldy + o] * win[i] * fabs(alpha[r])};
  }
  buf[tid] = v;
}

// partial[c][q][4][hb]: the four sums over rows [q rpp, (q + 1) rpp) of channel
// c's ns transformed rows, each bin with its mirror (F - k) % F, each row's
// balance taken out of its Y terms before they are summed.
__global__ __launch_bounds__(256) void cpsd_partials_kernel(const cd *__restrict__ buf,
                                                            int64_t channels, int64_t ns,
                                                            int64_t flen, int64_t rpp,
                                                            int64_t parts,
                                                            const double *__restrict__ alpha,
                                                            double *__restrict__ partial) {
  const int64_t hb = flen / 2 + 1;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= channels * parts * hb) return;
  const int64_t k = tid % hb, cq = tid / hb, c = cq / parts, q = cq - c * parts;
  const int64_t km = (flen - k) % flen;
  const int64_t r0 = q * rpp, r1 = r0 + rpp < ns ? r0 + rpp : ns;
  double sxx = 0.0, syy = 0.0, sre = 0.0, sim = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const cd *row = buf + (c * ns + r) * flen;
    const cd z = row[k], m = row[km];
    const double al = alpha[c * ns + r];
    const double ia = al == 0.0 ? 0.0 : 1.0 / fabs(al);  // exact: a power of 2
    const double ox = al < 0.0 ? 0.0 : 1.0;
    const double p = (z.x + m.x) * ox, e = (z.y - m.y) * ox;  // 2 X
    const double g = (z.y + m.y) * ia, d = (m.x - z.x) * ia;  // 2 Y
    sxx += p * p + e * e;
    syy += g * g + d * d;
    sre += p * g + e * d;
    sim += p * d - e * g;
  }
  double *dst = partial + cq * 4 * hb + k;
  dst[0] = 0.25 * sxx;
  dst[hb] = 0.25 * syy;
  dst[2 * hb] = 0.25 * sre;
  dst[3 * hb] = 0.25 * sim;
}

// Finalisation per channel and bin j < lp from acc[channel][4][hb]: every P
// by gdsp_pwelch_finalize's operations in its order (the sum, / nsegs, x 2
// between the ends, / norm); the coherence as the plain quotient of the sums
// (0 / 0 = NaN where a bin holds no power). A null output is skipped.
__global__ __launch_bounds__(256) void cpsd_finalize_kernel(
    const double *__restrict__ acc, int64_t channels, int64_t hb, int64_t lp, int64_t nsegs,
    double norm, cd *__restrict__ pxy, double *__restrict__ pxx, double *__restrict__ pyy,
    double *__restrict__ coh) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= channels * lp) return;
  const int64_t c = i / lp, j = i % lp;
  const double *a = acc + c * 4 * hb + j;
  const double sxx = a[0], syy = a[hb], sre = a[2 * hb], sim = a[3 * hb];
  auto scale = [&](double v) {
    double d = 0.0;
    if (nsegs > 0) {
      d = v / (double)nsegs;
      if (j > 0 && j < lp - 1) d *= 2;
    }
    return d / norm;
  };
  if (pxy) pxy[i] = {scale(sre), scale(sim)};
  if (pxx) pxx[i] = scale(sxx);
  if (pyy) pyy[i] = scale(syy);
  if (coh) coh[i] = (sre * sre + sim * sim) / (sxx * syy);
}

template <int LOG2F, bool PAD>
static hipError_t launch_cpb_t(const double *x, int64_t ldx, const double *y, int64_t ldy,
                               int64_t channels, int64_t wpc, int64_t nfft, int64_t stride,
                               int64_t seg_begin, int64_t seg_end, int64_t gpw, const double *win,
                               const cd *tw, double *partial, hipStream_t s) {
  constexpr int WPB = CpbGeo<LOG2F>::WPB;
  const int64_t nblk = (channels * wpc + WPB - 1) / WPB;
  if (nblk < 1 || nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((cpsd_batch_kernel<LOG2F, PAD>), dim3((unsigned)nblk),
                     dim3(CpbGeo<LOG2F>::BLOCK), 0, s, x, ldx, y, ldy, channels, wpc, nfft, stride,
                     seg_begin, seg_end, gpw, win, tw, partial);
  return hipGetLastError();
}

bool cpsd_batch_applies(int log2f) { return log2f >= 6 && log2f <= 11; }

// Workers per channel, segment groups per worker and partial rows per channel:
// pwelch_batch_geometry's rule over groups of S segments (two waves per SIMD).
void cpsd_batch_geometry(int log2f, int64_t channels, int64_t nsegs, int64_t *wpc, int64_t *gpw,
                         int64_t *rows) {
  const int T = (1 << log2f) / 16;
  const bool wave = T <= 64;
  const int S = wave ? 64 / T : 1;
  int64_t ngroups = (nsegs + S - 1) / S;
  if (ngroups < 1) ngroups = 1;
  const int64_t target = wave ? 2048 : 1024;
  int64_t want = channels > 0 ? target / channels : target;
  if (want < 1) want = 1;
  if (want > ngroups) want = ngroups;
  const int64_t g = (ngroups + want - 1) / want;
  *gpw = g;
  *wpc = (ngroups + g - 1) / g;
  *rows = *wpc * S;
}

hipError_t launch_cpsd_batch(int log2f, const double *x, int64_t ldx, const double *y, int64_t ldy,
                             int64_t channels, int64_t wpc, int64_t nfft, int64_t stride,
                             int64_t seg_begin, int64_t seg_end, int64_t gpw, const double *win,
                             const cd *tw, double *partial, hipStream_t s) {
  if (channels < 1 || wpc < 1 || gpw < 1 || seg_end <= seg_begin) return hipErrorInvalidValue;
  switch (log2f) {
#define GDSP_CPB(L)                                                                             \
  case L:                                                                                       \
    return nfft < (1 << L)                                                                      \
               ? launch_cpb_t<L, true>(x, ldx, y, ldy, channels, wpc, nfft, stride, seg_begin, \
                                       seg_end, gpw, win, tw, partial, s)                      \
               : launch_cpb_t<L, false>(x, ldx, y, ldy, channels, wpc, nfft, stride, seg_begin, \
                                        seg_end, gpw, win, tw, partial, s);
    GDSP_CPB(6) GDSP_CPB(7) GDSP_CPB(8) GDSP_CPB(9) GDSP_CPB(10) GDSP_CPB(11)
#undef GDSP_CPB
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_cpsd_balance(const double *x, int64_t ldx, const double *y, int64_t ldy,
                               int64_t channels, int64_t ns, int64_t nfft, int64_t stride,
                               int64_t seg0, const double *win, double *alpha, hipStream_t s) {
  const int64_t rows = channels * ns;
  if (rows < 1 || rows > 0x7fffffff || nfft < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cpsd_balance_kernel, dim3((unsigned)rows), dim3(256), 0, s, x, ldx, y, ldy, ns,
                     nfft, stride, seg0, win, alpha);
  return hipGetLastError();
}

hipError_t launch_cpsd_gather(const double *x, int64_t ldx, const double *y, int64_t ldy,
                              int64_t channels, int64_t ns, int64_t nfft, int64_t flen,
                              int64_t stride, int64_t seg0, const double *win,
                              const double *alpha, cd *buf, hipStream_t s) {
  const int64_t n = channels * ns * flen;
  if (n < 1 || (n + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cpsd_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx,
                     y, ldy, channels, ns, nfft, flen, stride, seg0, win, alpha, buf);
  return hipGetLastError();
}

hipError_t launch_cpsd_partials(const cd *buf, int64_t channels, int64_t ns, int64_t flen,
                                int64_t rpp, const double *alpha, double *partial,
                                hipStream_t s) {
  const int64_t parts = (ns + rpp - 1) / rpp;
  const int64_t n = channels * parts * (flen / 2 + 1);
  if (n < 1 || (n + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cpsd_partials_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, buf,
                     channels, ns, flen, rpp, parts, alpha, partial);
  return hipGetLastError();
}

hipError_t launch_cpsd_finalize(const double *acc, int64_t channels, int64_t hb, int64_t lp,
                                int64_t nsegs, double norm, cd *pxy, double *pxx, double *pyy,
                                double *coh, hipStream_t s) {
  const int64_t n = channels * lp;
  if (n < 1 || (n + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cpsd_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, acc,
                     channels, hb, lp, nsegs, norm, pxy, pxx, pyy, coh);
  return hipGetLastError();
}

}  // namespace gdsp
