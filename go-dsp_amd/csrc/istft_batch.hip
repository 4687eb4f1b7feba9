// istft_batch.hip — the overlap-add inverse of stft_batch.hip's rows: for every
// channel the signal
//   out[i] = num[i] / D[i],  num[i] = sum_s w[i - s stride] y_s[i - s stride],
//                            D[i]   = sum_s w[i - s stride]^2
// over the segments s that cover sample i, in ascending s, exactly 0 where
// D[i] == 0; y_s the first NFFT samples of the F-point inverse real transform
// of row X_s (lp = F / 2 + 1 bins, Hermitian completion, 1 / F included). The
// least-squares inverse of Griffin and Lim (scipy.signal.istft, MATLAB istft).
//
// The fused kernel serves F = Pad a power of 2 from 64 to 2048 with 0 <
// stride <= NFFT <= 4 stride (at most 4 segments over a sample). It shares
// stft_batch.hip's workers (a wave of S = 64 / T transforms, or two waves of
// one at F = 2048) and its packed pairs, by absolute index: rows (2 p, 2 p + 1)
// go through one inverse complex transform,
//   Z[j] = X_a[j] + i a X_b[j],  Z[F - j] = conj X_a[j] + i a conj X_b[j],
// whose result is z = y_a + i a y_b: no separation step. The transform is the
// forward fft_regs on conj Z (fir.hip, convolve.hip): y_a = Re U / F, a y_b =
// -Im U / F for U = FFT(conj Z).
//
// Loads. Every lane reads bins t + k T, k < 8, of both rows (16-byte loads,
// consecutive lanes consecutive bins) and bin F / 2: each half-spectrum
// element comes from HBM once. The upper half of conj Z is the mirror
// X_a[j] - i a X_b[j]; its two parts go through the transform's own exchange
// region (F slots, written by bin, read reversed: no bank conflict either
// way), not through a second read that would have to hit L2 behind 2 S rows
// of other traffic.
//
// Per row, as stft_batch.hip: the balance a = 2^(e_a - e_b) from the binary
// exponents of the rows' largest used parts (the imaginary parts of bins 0
// and F / 2 are dropped when loaded and count nowhere), taken out of y_b
// again exactly; a row of exact zeros is multiplied by 0, so it adds exact
// zeros, not its partner's roundoff; and containment: a pair that holds a NaN
// or an infinity writes nothing from the packed transform, and the worker
// runs the group twice more, the even rows alone, then the odd ones, from
// which only such pairs take their rows. So the samples of a row depend on
// its pair alone, not on the group it shares a wave with, and not on how a
// call was cut into ranges or workers.
//
// Overlap-add, output-stationary, no atomics. A group is 2 S consecutive
// segments, aligned by absolute index; group g owns samples [g, g + 1) 2 S
// stride. The worker writes the 2 S rows w y_s into LDS, then every lane sums
// its samples of the group's blocks of `stride` over the at most 4 rows that
// cover them in ascending s, starting from the carry: the partial sums of the
// NFFT - stride samples beyond the previous group, kept in LDS from group to
// group. Each finished sample is divided by its D (num / D, as the
// materialised form) and stored once, nontemporal. A worker owns a run of
// whole groups; for its first one it recomputes the halo: the earlier groups
// that still reach into its range (3 segments at most: one group, two where a
// group is a single pair), storing nothing from them. A sample's sum starts
// at +0 in the first group that covers it, in the halo as in the normal flow,
// so the bits do not depend on where a worker begins.
//
// D is periodic with stride away from the two ends: launch_istft_dtable
// builds the 9 blocks of `stride` values a call can meet (blocks 0 ... 3 of
// the signal, the periodic middle, blocks nsegs ... nsegs + 3) once, in
// ascending s; the kernel reads D, it does not form it.
//
// Every other shape and GDSP_ALGO_NO_FUSED_ISTFT run the materialised form at
// the end of this file: rows completed to dense complex rows of F, the plan's
// batched inverse transform, and a kernel with one thread per output sample
// that sums num and D in ascending s and divides (num / D).
#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

constexpr int kIstWaves = 2;  // wave workers per workgroup (the LDS budget)

// the balance's range in binary orders (stft_batch.hip, kStftMaxDe)
constexpr int kIstMaxDe = 1022;
__device__ constexpr int ist_clamp_de(int d) {
  return d < -kIstMaxDe ? -kIstMaxDe : (d > kIstMaxDe ? kIstMaxDe : d);
}

// groups a worker takes at least, where a channel has that many: the halo (one
// group; two at F >= 1024 above half overlap) stays a fifth (a third) of the
// worker's transforms at worst, in jobs too small to fill the device
constexpr int64_t kIstMinGroups = 4;

template <int LOG2F>
struct IstGeo {
  using G = Geo<LOG2F>;
  static constexpr int T = G::T, F = G::N;
  static constexpr bool WAVE = T <= 64;
  static constexpr int S = WAVE ? 64 / T : 1;       // transforms (pairs) per worker
  static constexpr int WPB = WAVE ? kIstWaves : 1;  // workers per workgroup
  static constexpr int NT = WAVE ? 64 : T;          // threads per worker
  static constexpr int BLOCK = WPB * NT;
  static constexpr int TWN = G::N / G::radix(G::NPASS - 1);
  static constexpr int XS = G::STRIDE;    // exchange doubles per transform
  static constexpr int ROWS = 2 * S * F;  // the group's rows w y_s
  static constexpr int CARRY = 3 * F / 4;  // NFFT - stride <= 3 NFFT / 4
  static constexpr int PER = S * XS + ROWS + CARRY;  // doubles per worker
  // the window is kept in LDS by the wave workers; the two-wave worker reads
  // it through L1 / L2 and keeps two workgroups per CU instead
  static constexpr int WIN = WAVE ? F : 0;
  static constexpr int LDS = WPB * PER + WIN + 2 * TWN + (WAVE ? 0 : 2);
};

template <int LOG2F, bool PAD>
__global__ __launch_bounds__((IstGeo<LOG2F>::BLOCK)) void istft_batch_kernel(
    const cd *__restrict__ X, int64_t ld_seg, int64_t ld_chan, int64_t channels, int64_t nsegs,
    int64_t row_lo, int64_t row_hi, int nf, int stride, int64_t g_begin, int64_t g_end,
    int64_t wpc, int64_t gpw, int halo, const double *__restrict__ win,
    const double *__restrict__ dtab, const cd *__restrict__ tw, int64_t out_begin,
    int64_t out_end, double *__restrict__ out, int64_t ldo) {
  using G = Geo<LOG2F>;
  using W = IstGeo<LOG2F>;
  constexpr int E = G::E, T = G::T, F = G::N, H = E / 2;
  static_assert(E == 16 && (T <= 64 ? 64 % T == 0 : T == 128), "one transform per wave or two waves");
  constexpr int S = W::S, XS = W::XS, NT = W::NT;
  static_assert(XS > F, "the mirror exchange uses F + 1 slots of the region");
  __shared__ double lds[W::LDS];
  const int lt = (int)threadIdx.x;
  const int w = W::WAVE ? lt >> 6 : 0, lane = W::WAVE ? lt & 63 : lt;
  const int s = lane / T, t = lane % T;
  double *const wk = lds + w * W::PER;
  double *const lre = wk + s * XS;
  double *const rows = wk + S * XS;
  double *const carry = rows + W::ROWS;
  double *const wl = lds + W::WPB * W::PER;
  cd *const twl = reinterpret_cast<cd *>(wl + W::WIN);
  if constexpr (W::WAVE)
    for (int i = lt; i < F; i += W::BLOCK) wl[i] = win[i];
  for (int i = lt; i < W::TWN; i += W::BLOCK) twl[i] = tw[i];
  for (int i = lane; i < W::CARRY; i += NT) carry[i] = 0.0;
  __syncthreads();
  // the worker, its channel and its groups: uniform over its waves (the
  // barrier above is the only one all workers of a workgroup share)
  const int64_t worker = (int64_t)blockIdx.x * W::WPB + __builtin_amdgcn_readfirstlane(w);
  const int64_t chan = worker / wpc;
  if (chan >= channels) return;
  X += chan * ld_chan;
  out += chan * ldo;
  const int64_t gs = g_begin + (worker - chan * wpc) * gpw;
  const int64_t ge = gs + gpw < g_end ? gs + gpw : g_end;
  if (gs >= ge) return;
  const int64_t gh = gs - halo > 0 ? gs - halo : 0;
  const int C = nf - stride;        // samples beyond a group that its rows reach
  const int owned = 2 * S * stride;  // samples a group owns
  const int L = owned + C;
  const int kc = (C + stride - 1) / stride;  // blocks of the carry, <= 3
  const double inv_f = 1.0 / (double)F;
  auto present = [&](int64_t sa) { return sa >= row_lo && sa < row_hi; };

  // One packed inverse transform per slot and its two rows w y into LDS. mode
  // 0: both rows; 1: the even row alone, 2: the odd one alone. Returns the
  // mode to run the group in next (0: done), uniform over the worker.
  auto run = [&](const cd *xa, const cd *xb, bool act0, bool act1, int mode) -> int {
    const int tt = opaque_int(t);
    const bool ka = mode != 2, kb = mode != 1;
    cd v[E];
    double ph[H], qh[H];
    int mhx = 0, mhy = 0, lox = 0, loy = 0;  // max of the high words of |.|, or of the low ones
    auto note = [](double u, int &mh, int &lo) {
      mh = max(mh, __double2hiint(u) & 0x7fffffff);
      lo |= __double2loint(u);
    };
    // bin F / 2: its real parts only
    double ahx = ld_nt(&xa[F / 2].x), bhx = ld_nt(&xb[F / 2].x);
    ahx = act0 ? ahx : 0.0;
    bhx = act1 ? bhx : 0.0;
    note(ahx, mhx, lox);
    note(bhx, mhy, loy);
    cd a[H], b[H];
#pragma unroll
    for (int k = 0; k < H; ++k) {
      a[k] = ld_nt(xa + tt + k * T);
      b[k] = ld_nt(xb + tt + k * T);
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {
      a[k].x = act0 ? a[k].x : 0.0;
      a[k].y = act0 ? a[k].y : 0.0;
      b[k].x = act1 ? b[k].x : 0.0;
      b[k].y = act1 ? b[k].y : 0.0;
      if (k == 0) {  // bin 0's imaginary part is not read into anything
        a[k].y = t == 0 ? 0.0 : a[k].y;
        b[k].y = t == 0 ? 0.0 : b[k].y;
      }
      note(a[k].x, mhx, lox);
      note(a[k].y, mhx, lox);
      note(b[k].x, mhy, loy);
      note(b[k].y, mhy, loy);
    }
    // biased exponents of the rows' largest used parts (-1: a row of exact
    // zeros, 0: subnormal, 2047: not finite), as loaded, whatever the mode
    int ex = (mhx | lox) == 0 ? -1 : mhx >> 20;
    int ey = (mhy | loy) == 0 ? -1 : mhy >> 20;
#pragma unroll
    for (int m = 1; m < (W::WAVE ? T : 64); m <<= 1) {
      ex = max(ex, __shfl_xor(ex, m));
      ey = max(ey, __shfl_xor(ey, m));
    }
    if constexpr (!W::WAVE) {
      // the worker's two waves: one pair each, behind the barrier
      int *const xe = reinterpret_cast<int *>(lds + W::PER + 2 * W::TWN);
      if ((lt & 63) == 0) {
        xe[2 * (lt >> 6)] = ex;
        xe[2 * (lt >> 6) + 1] = ey;
      }
      __syncthreads();
      ex = max(xe[0], xe[2]);
      ey = max(xe[1], xe[3]);
    }
    // containment: this pair's rows come from the packed transform, or from
    // the two transforms of one row each
    const bool dirty = ex == 2047 || ey == 2047;
    const bool wa = mode == 0 ? !dirty : (dirty && mode == 1);
    const bool wb = mode == 0 ? !dirty : (dirty && mode == 2);
    const int ea = ka ? ex : -1, eb = kb ? ey : -1;
    const bool bal = ea > 0 && eb > 0 && ea < 2047 && eb < 2047;
    const int de = !bal ? 0 : ist_clamp_de(ea - eb);
    const double al = __hiloint2double((1023 + de) << 20, 0);
    // y_a = Re U ox / F, y_b = -Im U / (a F); a row of zeros: exact zeros
    const double sa = ea < 0 ? 0.0 : inv_f;
    const double sb = eb < 0 ? 0.0 : -(__hiloint2double((1023 - de) << 20, 0) * inv_f);
    ahx = ka ? ahx : 0.0;
    bhx = kb ? bhx * al : 0.0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const double ax = ka ? a[k].x : 0.0, ay = ka ? a[k].y : 0.0;
      const double bx = kb ? b[k].x * al : 0.0, by = kb ? b[k].y * al : 0.0;
      v[k] = {ax - by, -ay - bx};  // conj Z[j] = conj X_a - i a conj X_b
      ph[k] = ax + by;             // conj Z[F - j] = X_a - i a X_b
      qh[k] = ay - bx;
    }
    // the mirror exchange: bin j's two parts into slots j and F / 2 + j, after
    // every lane of the transform has read the last exchange of the one before
    xsync<W::WAVE>();
#pragma unroll
    for (int k = 0; k < H; ++k) {
      lre[tt + k * T] = ph[k];
      lre[F / 2 + tt + k * T] = qh[k];
    }
    xsync<W::WAVE>();
#pragma unroll
    for (int k = H; k < E; ++k) {
      const int m = F - tt - k * T;  // 1 ... F / 2
      v[k] = {lre[m], lre[F / 2 + m]};
    }
    // bin F / 2 (lane 0's register 8) mirrors itself
    v[H].x = t == 0 ? ahx : v[H].x;
    v[H].y = t == 0 ? -bhx : v[H].y;
    fft_regs<LOG2F, true, 2, 4, 0, 0, const cd *, 1, 0, NoEpi, 0, 16, W::WAVE>(v, tt, twl, lre,
                                                                              lre, false);
    double *const ra = rows + 2 * s * F;
    double *const rb = ra + F;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int i = t + k * T;
      if (PAD && i >= nf) continue;  // samples NFFT ... F - 1 are discarded
      double wv;
      if constexpr (W::WAVE) wv = wl[tt + k * T];
      else wv = win[tt + k * T];
      if (wa) ra[tt + k * T] = wv * (v[k].x * sa);
      if (wb) rb[tt + k * T] = wv * (v[k].y * sb);
    }
    if (mode == 0) return __any(dirty) != 0 ? 1 : 0;
    return mode == 1 ? 2 : 0;
  };

  for (int64_t g = gh; g < ge; ++g) {
    const int64_t sg = 2 * S * g;  // the group's first segment
    if (sg < nsegs) {
      // clamped in-buffer loads (a slot past the channel's rows, a missing
      // partner, a row the caller did not pass), the mask applied where used
      const int64_t s0 = sg + 2 * s;
      const bool act0 = present(s0), act1 = present(s0 + 1);
      const int64_t c0 = s0 < row_lo ? row_lo : (s0 >= row_hi ? row_hi - 1 : s0);
      const int64_t c1 = s0 + 1 < row_lo ? row_lo : (s0 + 1 >= row_hi ? row_hi - 1 : s0 + 1);
      const cd *const xa = X + (c0 - row_lo) * ld_seg;
      const cd *const xb = X + (c1 - row_lo) * ld_seg;
      int mode = 0;
      do {
        mode = run(xa, xb, act0, act1, mode);
      } while (mode != 0);
    }
    xsync<W::WAVE>();
    // sample u of the group's span: the carry, then rows q - 3 ... q of block q
    auto sum = [&](int q, int r) -> double {
      const int u = q * stride + r;
      double acc = u < C ? carry[u] : 0.0;
#pragma unroll
      for (int m = 3; m >= 0; --m) {
        const int row = q - m, idx = r + m * stride;
        if (row >= 0 && row < 2 * S && idx < nf && sg + row < nsegs && present(sg + row))
          acc = __dadd_rn(acc, rows[row * F + idx]);
      }
      return acc;
    };
    const bool store = g >= gs;
    const int64_t ibase = g * (int64_t)owned;
    for (int q = 0; q < 2 * S; ++q) {
      // the block's row of the D table (launch_istft_dtable)
      const int64_t b = sg + q;
      const int64_t past = b - nsegs > 3 ? 3 : b - nsegs;
      const int tb = b < 4 ? (int)b : (b < nsegs ? 4 : 5 + (int)past);
      for (int r = lane; r < stride; r += NT) {
        const double acc = sum(q, r);
        const int64_t i = ibase + q * stride + r;
        if (store && i >= out_begin && i < out_end) {
          const double d = dtab[(int64_t)tb * stride + r];
          __builtin_nontemporal_store(d > 0.0 ? acc / d : 0.0, out + (i - out_begin));
        }
      }
    }
    xsync<W::WAVE>();
    // the carry of the next group, block by block: a block reads slots that a
    // later one writes
    for (int q = 2 * S; q < 2 * S + kc; ++q) {
      for (int r = lane; r < stride; r += NT) {
        const int u = q * stride + r;
        if (u < L) carry[u - owned] = sum(q, r);
      }
      xsync<W::WAVE>();
    }
  }
}

// D of the 9 blocks of `stride` samples a call can meet: table block tb < 4 is
// block tb of the signal, 4 any block b with 4 <= b < nsegs (every one of them
// has all its segments), 5 + k block nsegs + k; D[r] = sum of w[r + m stride]^2
// over the segments b - m that exist, in ascending s (descending m).
__global__ __launch_bounds__(256) void istft_dtable_kernel(const double *__restrict__ win,
                                                            int64_t nfft, int64_t stride,
                                                            int64_t nsegs,
                                                            double *__restrict__ dtab) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= 9 * stride) return;
  const int64_t tb = tid / stride, r = tid - tb * stride;
  const int64_t b = tb < 5 ? tb : nsegs + tb - 5;
  double d = 0.0;
  for (int m = 3; m >= 0; --m) {
    const int64_t sa = b - m, idx = r + m * stride;
    if (sa < 0 || sa >= nsegs || idx >= nfft) continue;
    const double wv = win[idx];
    d = __dadd_rn(d, __dmul_rn(wv, wv));
  }
  dtab[tid] = d;
}

// ---- the materialised form ---------------------------------------------------
// Row r = c * ns + j of buf: the F = flen points of the Hermitian completion of
// row (c, seg0 + j), the imaginary parts of bins 0 and (flen even) flen / 2
// dropped.
__global__ __launch_bounds__(256) void istft_complete_kernel(
    const cd *__restrict__ X, int64_t ld_seg, int64_t ld_chan, int64_t row_lo, int64_t nc,
    int64_t seg0, int64_t ns, int64_t flen, cd *__restrict__ buf) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= nc * ns * flen) return;
  const int64_t r = tid / flen, k = tid - r * flen;
  const int64_t c = r / ns, j = r - c * ns;
  const bool up = k > flen / 2;
  cd z = X[c * ld_chan + (seg0 + j - row_lo) * ld_seg + (up ? flen - k : k)];
  if (up) z.y = -z.y;
  if (k == 0 || 2 * k == flen) z.y = 0.0;
  buf[tid] = z;
}

// One thread per sample i0 <= i < i1 of nc channels: num and D over the
// segments that cover i in ascending s from the inverse transforms in buf
// (rows of segments [seg0, seg0 + ns)), then num / D.
__global__ __launch_bounds__(256) void istft_ola_kernel(
    const cd *__restrict__ buf, int64_t nc, int64_t seg0, int64_t ns, int64_t nsegs, int64_t flen,
    int64_t nfft, int64_t stride, const double *__restrict__ win, int64_t i0, int64_t i1,
    double *__restrict__ out, int64_t ldo) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t len = i1 - i0;
  if (tid >= nc * len) return;
  const int64_t c = tid / len, i = i0 + (tid - c * len);
  int64_t shi = i / stride, slo = i >= nfft ? (i - nfft) / stride + 1 : 0;
  if (shi > nsegs - 1) shi = nsegs - 1;
  double num = 0.0, d = 0.0;
  for (int64_t sa = slo; sa <= shi; ++sa) {
    const int64_t idx = i - sa * stride;
    const double wv = win[idx];
    num = __dadd_rn(num, __dmul_rn(wv, buf[(c * ns + (sa - seg0)) * flen + idx].x));
    d = __dadd_rn(d, __dmul_rn(wv, wv));
  }
  out[c * ldo + (i - i0)] = d > 0.0 ? num / d : 0.0;
}

template <int LOG2F, bool PAD>
static hipError_t launch_ist_t(const cd *X, int64_t ld_seg, int64_t ld_chan, int64_t channels,
                               int64_t nsegs, int64_t row_lo, int64_t row_hi, int64_t nfft,
                               int64_t stride, int64_t g_begin, int64_t g_end, int64_t wpc,
                               int64_t gpw, int halo, const double *win, const double *dtab,
                               const cd *tw, int64_t out_begin, int64_t out_end, double *out,
                               int64_t ldo, hipStream_t s) {
  constexpr int WPB = IstGeo<LOG2F>::WPB;
  const int64_t nblk = (channels * wpc + WPB - 1) / WPB;
  if (nblk < 1 || nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((istft_batch_kernel<LOG2F, PAD>), dim3((unsigned)nblk),
                     dim3(IstGeo<LOG2F>::BLOCK), 0, s, X, ld_seg, ld_chan, channels, nsegs, row_lo,
                     row_hi, (int)nfft, (int)stride, g_begin, g_end, wpc, gpw, halo, win, dtab, tw,
                     out_begin, out_end, out, ldo);
  return hipGetLastError();
}

bool istft_batch_applies(int log2f) { return log2f >= 6 && log2f <= 11; }

int istft_group_segments(int log2f) {
  const int T = (1 << log2f) / 16;
  return T <= 64 ? 2 * (64 / T) : 2;
}

// Workers per channel and groups per worker: stft_batch_geometry's rule (the
// workers of the whole job shared by the channels, at least one per channel),
// with kIstMinGroups groups per worker where workers have a halo to recompute.
void istft_batch_geometry(int log2f, int64_t channels, int64_t ngroups, int halo_groups,
                          int64_t *wpc, int64_t *gpw) {
  const bool wave = (1 << log2f) / 16 <= 64;
  if (ngroups < 1) ngroups = 1;
  const int64_t target = wave ? 2048 : 1024;
  int64_t want = channels > 0 ? target / channels : target;
  if (want < 1) want = 1;
  if (want > ngroups) want = ngroups;
  int64_t g = (ngroups + want - 1) / want;
  if (halo_groups > 0 && g < kIstMinGroups) g = kIstMinGroups;
  if (g > ngroups) g = ngroups;
  *gpw = g;
  *wpc = (ngroups + g - 1) / g;
}

int64_t istft_dtable_doubles(int64_t stride) { return 9 * stride; }

hipError_t launch_istft_dtable(const double *win, int64_t nfft, int64_t stride, int64_t nsegs,
                               double *dtab, hipStream_t s) {
  if (stride < 1 || nfft < stride || nfft > 4 * stride || nsegs < 1) return hipErrorInvalidValue;
  const int64_t n = 9 * stride;
  hipLaunchKernelGGL(istft_dtable_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, win,
                     nfft, stride, nsegs, dtab);
  return hipGetLastError();
}

hipError_t launch_istft_batch(int log2f, const cd *X, int64_t ld_seg, int64_t ld_chan,
                              int64_t channels, int64_t nsegs, int64_t row_lo, int64_t row_hi,
                              int64_t nfft, int64_t stride, int64_t g_begin, int64_t g_end,
                              int64_t wpc, int64_t gpw, const double *win, const double *dtab,
                              const cd *tw, int64_t out_begin, int64_t out_end, double *out,
                              int64_t ldo, hipStream_t s) {
  const int64_t F = (int64_t)1 << log2f;
  if (channels < 1 || wpc < 1 || gpw < 1 || g_end <= g_begin || g_begin < 0 || nsegs < 1 ||
      row_lo < 0 || row_hi <= row_lo || row_hi > nsegs || stride < 1 || nfft < stride ||
      nfft > 4 * stride || nfft > F || ld_seg < F / 2 + 1 || out_begin < 0 ||
      out_end <= out_begin || out_end > (nsegs - 1) * stride + nfft)
    return hipErrorInvalidValue;
  // the earlier groups whose rows reach into a worker's first one
  const int gseg = istft_group_segments(log2f);
  const int kc = (int)((nfft - stride + stride - 1) / stride);
  const int halo = (kc + gseg - 1) / gseg;
  switch (log2f) {
#define GDSP_IST_P(L, PAD)                                                                        \
  launch_ist_t<L, PAD>(X, ld_seg, ld_chan, channels, nsegs, row_lo, row_hi, nfft, stride, g_begin, \
                       g_end, wpc, gpw, halo, win, dtab, tw, out_begin, out_end, out, ldo, s)
#define GDSP_IST(L) \
  case L: return nfft < (1 << L) ? GDSP_IST_P(L, true) : GDSP_IST_P(L, false);
    GDSP_IST(6) GDSP_IST(7) GDSP_IST(8) GDSP_IST(9) GDSP_IST(10) GDSP_IST(11)
#undef GDSP_IST
#undef GDSP_IST_P
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_istft_complete(const cd *X, int64_t ld_seg, int64_t ld_chan, int64_t row_lo,
                                 int64_t nc, int64_t seg0, int64_t ns, int64_t flen, cd *buf,
                                 hipStream_t s) {
  const int64_t n = nc * ns * flen;
  if (n < 1 || (n + 255) / 256 > 0x7fffffff || seg0 < row_lo || ld_seg < flen / 2 + 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(istft_complete_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X,
                     ld_seg, ld_chan, row_lo, nc, seg0, ns, flen, buf);
  return hipGetLastError();
}

hipError_t launch_istft_ola(const cd *buf, int64_t nc, int64_t seg0, int64_t ns, int64_t nsegs,
                            int64_t flen, int64_t nfft, int64_t stride, const double *win,
                            int64_t i0, int64_t i1, double *out, int64_t ldo, hipStream_t s) {
  const int64_t n = nc * (i1 - i0);
  if (n < 1 || (n + 255) / 256 > 0x7fffffff || stride < 1 || nfft < 1 || nfft > flen || i0 < 0 ||
      i1 > (nsegs - 1) * stride + nfft)
    return hipErrorInvalidValue;
  // the rows the range needs are those the caller transformed
  const int64_t slo = i0 >= nfft ? (i0 - nfft) / stride + 1 : 0;
  int64_t shi = (i1 - 1) / stride;
  if (shi > nsegs - 1) shi = nsegs - 1;
  if (slo < seg0 || shi >= seg0 + ns) return hipErrorInvalidValue;
  hipLaunchKernelGGL(istft_ola_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, buf, nc,
                     seg0, ns, nsegs, flen, nfft, stride, win, i0, i1, out, ldo);
  return hipGetLastError();
}

}  // namespace gdsp
