// launch.hpp — host launchers of the gfx950 kernels (fft_kernels.hip), used by
// the C ABI layer (gdsp_api.hip; the Welch family's in welch.hip). Internal to
// libgdspfft.
#pragma once
#ifndef __HIPCC_RTC__  // the device-side parts are also compiled by hipRTC (mixed_jit.cpp)
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif

namespace gdsp {

struct cd;

enum { LOAD_COMPLEX = 0, LOAD_REAL = 1 };

// largest power-of-2 length handled by the one-kernel LDS transform / the
// fused Bluestein kernel (M) / the fused Pwelch kernel
constexpr int kMaxLdsLog2 = 14;

// Mixed-radix one-kernel transform (fft_mixed.hip): n = prod of the radices
// in `codes` (5 bits per pass, radices 2,3,4,5,7,8,11,13,16 in the runtime-radix
// kernels, also 6,9,10,12,15,20,25 in the compiled specialisations), n <= kMixedMax
// (kMixedSpecMax for a specialisation).
struct MixedDesc {
  uint64_t codes;
  int n, npass, t1, tpw;
};
constexpr int kMixedMax = 4096;
// compiled specialisations (fft_specs*.hip) reach this far (re/im exchange)
constexpr int kMixedSpecMax = 8192;

#ifndef __HIPCC_RTC__

// ---- configuration (gdsp_api.hip) ------------------------------------------
// Deployment knobs: the only process environment the library reads.
enum Knob {
  KNOB_DEVICES,          // GDSP_DEVICES: initial multi-device set ("0,1,2" / "all")
  KNOB_MULTI_MIN_BYTES,  // GDSP_MULTI_MIN_BYTES: split threshold of host calls
  KNOB_JIT,              // GDSP_JIT=0: no runtime-compiled specialisations
  KNOB_JIT_INCLUDE,      // GDSP_JIT_INCLUDE: header directory for hipRTC
  KNOB_JIT_CACHE,        // GDSP_JIT_CACHE: code-object cache directory
  KNOB_JIT_VERBOSE,      // GDSP_JIT_VERBOSE: log runtime compilations
  KNOB_XDG_CACHE_HOME,   // default cache location
  KNOB_HOME,
};
const char *knob(Knob k);
// Algorithm selection flags (gdsp_set_algorithm, include/gdsp_fft.h) in
// force when a plan is built.
unsigned algo_flags();

hipError_t launch_fft_lds(int log2n, bool inv, int load, bool split, const void *in, cd *out,
                          int64_t batch, const cd *tw, double scale, hipStream_t s);
// the N = 4096 case of launch_fft_lds (fft_lds12.hip)
hipError_t launch_fft_lds12(bool inv, int load, bool split, const void *in, cd *out, int64_t batch,
                            const cd *tw, double scale, hipStream_t s);
// fused Pwelch over a mixed-radix segment length d.n = max(pad, nfft) with
// d.npass >= 2 (fft_mixed.hip); same partial layout as launch_pwelch
hipError_t launch_pwelch_mixed(const MixedDesc &d, const double *x, int64_t nfft, int64_t stride,
                               int64_t seg_begin, int64_t seg_end, int64_t ppw, int64_t nworkers,
                               const double *win, const cd *tw, double *partial, hipStream_t s);
// fused Pwelch with wave-resident transforms (pwelch_wave.hip), 64 <= F <= 1024:
// the launch geometry (groups of pairs per wave, workgroups, partial rows)
bool pwelch_wave_applies(int log2f);
void pwelch_wave_geometry(int log2f, bool half, int64_t nsegs, int64_t *gpw, int64_t *nblk,
                          int64_t *nrows);
hipError_t launch_pwelch_wave(int log2f, bool half, const double *x, int64_t nfft, int64_t stride,
                              int64_t seg_begin, int64_t seg_end, int64_t gpw, int64_t nblk,
                              const double *win, const cd *tw, double *partial, hipStream_t s);
// the same kernel family over the channels of a planar batch (pwelch_batch.hip),
// channel c at x + c ldx: workers per channel (wpc), pair groups per worker
// and partial rows per channel for the whole job; the launch over `channels`
// channels into partial[channel][rows][F]; the fixed-order reduce of every
// channel's rows into acc + c F (scratch: reduce_batch_scratch_doubles); and
// gdsp_pwelch_finalize's arithmetic per channel into pxx[channel][lp]
bool pwelch_batch_applies(int log2f);
void pwelch_batch_geometry(int log2f, bool half, int64_t channels, int64_t nsegs, int64_t *wpc,
                           int64_t *gpw, int64_t *rows);
hipError_t launch_pwelch_batch(int log2f, bool half, const double *x, int64_t ldx,
                               int64_t channels, int64_t wpc, int64_t nfft, int64_t stride,
                               int64_t seg_begin, int64_t seg_end, int64_t gpw, const double *win,
                               const cd *tw, double *partial, hipStream_t s);
int64_t reduce_batch_scratch_doubles(int64_t channels, int64_t rows, int64_t F);
hipError_t launch_reduce_batch(const double *partial, int64_t channels, int64_t rows, int64_t F,
                               double *acc, double *scratch, hipStream_t s);
hipError_t launch_pwelch_finalize(const double *acc, int64_t channels, int64_t flen, int64_t lp,
                                  int64_t nsegs, double norm, double *pxx, hipStream_t s);
// the cross-spectral sums of two planar batches (cpsd_batch.hip): x channel c
// at x + c ldx, y channel c at y + c ldy (ldy = 0: one y for all), one segment
// of both per transform. The fused kernel for the lengths of the batched
// Pwelch, into partial[channel][rows][4][hb] (hb = F / 2 + 1; planes Sxx, Syy,
// Re Sxy, Im Sxy; reduced by launch_reduce_batch with F := 4 hb); the
// materialised form for every other length (rows w x_s + i w y_s of segments
// [seg0, seg0 + ns) of every channel, then, after the plan's transform, the
// sums of each row and its mirror over parts of rpp rows); and the finaliser
// of acc[channel][4][hb] into any of pxy, pxx, pyy, coh [channel][lp].
// Every segment's y is packed times a power of 2 that is taken out of its
// products again (cpsd_batch.hip, Balance): inside the fused kernel; in the
// materialised form alpha[row] from launch_cpsd_balance, rows as the gather's
bool cpsd_batch_applies(int log2f);
void cpsd_batch_geometry(int log2f, int64_t channels, int64_t nsegs, int64_t *wpc, int64_t *gpw,
                         int64_t *rows);
hipError_t launch_cpsd_batch(int log2f, const double *x, int64_t ldx, const double *y, int64_t ldy,
                             int64_t channels, int64_t wpc, int64_t nfft, int64_t stride,
                             int64_t seg_begin, int64_t seg_end, int64_t gpw, const double *win,
                             const cd *tw, double *partial, hipStream_t s);
hipError_t launch_cpsd_balance(const double *x, int64_t ldx, const double *y, int64_t ldy,
                               int64_t channels, int64_t ns, int64_t nfft, int64_t stride,
                               int64_t seg0, const double *win, double *alpha, hipStream_t s);
hipError_t launch_cpsd_gather(const double *x, int64_t ldx, const double *y, int64_t ldy,
                              int64_t channels, int64_t ns, int64_t nfft, int64_t flen,
                              int64_t stride, int64_t seg0, const double *win,
                              const double *alpha, cd *buf, hipStream_t s);
hipError_t launch_cpsd_partials(const cd *buf, int64_t channels, int64_t ns, int64_t flen,
                                int64_t rpp, const double *alpha, double *partial,
                                hipStream_t s);
hipError_t launch_cpsd_finalize(const double *acc, int64_t channels, int64_t hb, int64_t lp,
                                int64_t nsegs, double norm, cd *pxy, double *pxx, double *pyy,
                                double *coh, hipStream_t s);
// the per-segment spectra of a planar batch (stft_batch.hip): row (c, s -
// seg_begin) of out, at element c ld_chan + (s - seg_begin) ld_seg, is the
// first lp bins of the F-point transform of segment s of channel c, windowed
// and zero-padded: complex128 (power = false), or float64 c_j |X|^2 / norm.
// The fused kernel for the lengths of the batched Pwelch (packed segment
// pairs, balanced by a power of 2 per pair, its geometry without partials:
// workers per channel and pair groups per worker); the materialised form for
// every other length: rows w x_s of segments [seg0, seg0 + ns) of every
// channel as float64 rows of flen, then, after the plan's transform of real
// rows, launch_stft_rows into the caller's layout at segment row `row0`.
bool stft_batch_applies(int log2f);
void stft_batch_geometry(int log2f, int64_t channels, int64_t nsegs, int64_t *wpc, int64_t *gpw);
hipError_t launch_stft_batch(int log2f, bool power, const double *x, int64_t ldx, int64_t channels,
                             int64_t wpc, int64_t nfft, int64_t stride, int64_t seg_begin,
                             int64_t seg_end, int64_t gpw, const double *win, const cd *tw,
                             void *out, int64_t lp, int64_t ld_seg, int64_t ld_chan, double norm,
                             hipStream_t s);
hipError_t launch_stft_gather(const double *x, int64_t ldx, int64_t channels, int64_t ns,
                              int64_t nfft, int64_t flen, int64_t stride, int64_t seg0,
                              const double *win, double *buf, hipStream_t s);
hipError_t launch_stft_rows(const cd *buf, int64_t channels, int64_t ns, int64_t flen, int64_t lp,
                            bool power, double norm, void *out, int64_t row0, int64_t ld_seg,
                            int64_t ld_chan, hipStream_t s);
// the overlap-add inverse of those rows (istft_batch.hip): out[c ldo + i -
// out_begin] = num[i] / D[i] (exactly 0 where D[i] == 0) for out_begin <= i <
// out_end, num and D summed over the segments that cover i in ascending s. X
// holds rows [row_lo, row_hi) of every channel, row (c, s) at c ld_chan + (s -
// row_lo) ld_seg; rows outside are neither read nor used. The fused kernel
// (F = 2^log2f from 64 to 2048 = pad, 0 < stride <= nfft <= 4 stride): groups
// of istft_group_segments(log2f) segments aligned by absolute index, group g
// owning samples [g, g + 1) * that * stride; groups [g_begin, g_end) over wpc
// workers per channel of gpw groups each (istft_batch_geometry), every worker
// recomputing its halo; dtab from launch_istft_dtable (istft_dtable_doubles
// (stride) doubles). The materialised form: launch_istft_complete writes the
// dense Hermitian rows of segments [seg0, seg0 + ns) of nc channels (buf row
// c ns + j), and after the plan's inverse transform launch_istft_ola sums
// samples [i0, i1) with one thread each from those rows.
bool istft_batch_applies(int log2f);
int istft_group_segments(int log2f);
void istft_batch_geometry(int log2f, int64_t channels, int64_t ngroups, int halo_groups,
                          int64_t *wpc, int64_t *gpw);
int64_t istft_dtable_doubles(int64_t stride);
hipError_t launch_istft_dtable(const double *win, int64_t nfft, int64_t stride, int64_t nsegs,
                               double *dtab, hipStream_t s);
hipError_t launch_istft_batch(int log2f, const cd *X, int64_t ld_seg, int64_t ld_chan,
                              int64_t channels, int64_t nsegs, int64_t row_lo, int64_t row_hi,
                              int64_t nfft, int64_t stride, int64_t g_begin, int64_t g_end,
                              int64_t wpc, int64_t gpw, const double *win, const double *dtab,
                              const cd *tw, int64_t out_begin, int64_t out_end, double *out,
                              int64_t ldo, hipStream_t s);
hipError_t launch_istft_complete(const cd *X, int64_t ld_seg, int64_t ld_chan, int64_t row_lo,
                                 int64_t nc, int64_t seg0, int64_t ns, int64_t flen, cd *buf,
                                 hipStream_t s);
hipError_t launch_istft_ola(const cd *buf, int64_t nc, int64_t seg0, int64_t ns, int64_t nsegs,
                            int64_t flen, int64_t nfft, int64_t stride, const double *win,
                            int64_t i0, int64_t i1, double *out, int64_t ldo, hipStream_t s);
// fused Pwelch on a compiled specialisation (d = the plan's specialisation
// descriptor, d.n = max(pad, nfft)); workers per block, 0 if d is none or
// its kernel cannot stage a pair of span = stride + nfft samples
int pwelch_fixed_workers_per_block(const MixedDesc &d, int64_t span);
hipError_t launch_pwelch_fixed(const MixedDesc &d, const double *x, int64_t nfft, int64_t stride,
                               int64_t seg_begin, int64_t seg_end, int64_t ppw, int64_t nworkers,
                               const double *win, const cd *tw, double *partial, hipStream_t s);
// runtime-compiled specialisations (mixed_jit.hip, hipRTC): a radix list for
// a smooth n <= kMixedSpecMax without a compiled one, and its kernels
struct JitSpec;
bool jit_enabled();
bool jit_radices(int n, int *rad, int *npass);
JitSpec *jit_spec_build(int dev, const int *rad, int np, int n);  // nullptr: not built
// colfixed_kernel (mixed_fixed.hpp) for the column length prod(rad)
struct JitCol;
JitCol *jit_col_build(int dev, const int *rad, int np);  // nullptr: not built
// rowt_fixed_kernel (mixed_fixed.hpp) for the row length prod(rad): rows of
// a two-pass mixed four-step with the transpose in their store
struct JitRowT;
JitRowT *jit_rowt_build(int dev, const int *rad, int np);  // nullptr: not built
hipError_t jit_launch_rowt(const JitRowT *j, bool conj_scale_out, const cd *in, cd *out,
                           int64_t rows, int64_t L, const cd *tw, double scale, hipStream_t s);
hipError_t jit_launch_col(const JitCol *j, bool conj_in, const cd *in, cd *out, int64_t C,
                          int64_t n, int64_t batch, const cd *tw, const cd *twn, hipStream_t s);
hipError_t jit_launch_fft(const JitSpec *j, bool inv, int load, const void *in, cd *out,
                          int64_t batch, const cd *tw, double scale, hipStream_t s);
int jit_pw_tpw(const JitSpec *j, int64_t span);  // as pwelch_fixed_workers_per_block
// rader_fixed_kernel (mixed_fixed.hpp): a prime P = prod(rad) + 1 by Rader's
// algorithm on the inlined mixed-radix chain of its N = P - 1
struct JitRader;
JitRader *jit_rader_build(int dev, const int *rad, int np);  // nullptr: not built
hipError_t jit_launch_rader(const JitRader *j, bool inv, int load, const void *in, cd *out,
                            int64_t batch, const cd *tw, const cd *bhat, const int *gpow,
                            const int *ginv, double scale, hipStream_t s);
// rader_pfa_kernel (mixed_fixed.hpp): n = m * P (gcd 1), P = prod(rad) + 1
// prime, by the prime-factor map and m Rader sub-transforms in one kernel;
// launched by jit_launch_rader with the prime P's tables. nullptr: m has no
// in-register DFT, the geometry does not fit, or the kernel did not build.
bool pfa_cofactor_supported(int m);
// bluestein_fixed_kernel (mixed_fixed.hpp): the fused chirp-z on a smooth
// convolution length L = prod(rad) >= 2n - 1. blufix_length: L (and its list)
// where the lane-cost model puts it below 0.85 of the current fused kernel
// on m_now with list rad_now, else 0.
int blufix_length(int64_t n, int64_t m_now, const int *rad_now, int np_now, int *rad, int *np);
struct JitBlu;
JitBlu *jit_blu_build(int dev, int64_t n, const int *rad, int np);  // nullptr: not built
hipError_t jit_launch_blu(const JitBlu *j, bool inv, int load, const void *in, cd *out,
                          int64_t batch, const cd *tw, const cd *chirp, const cd *bhat,
                          double scale, hipStream_t s);
JitRader *jit_rader_pfa_build(int dev, int m, const int *rad, int np);
hipError_t jit_launch_pwelch(const JitSpec *j, const double *x, int64_t nfft, int64_t stride,
                             int64_t seg_begin, int64_t seg_end, int64_t ppw, int64_t nworkers,
                             const double *win, const cd *tw, double *partial, hipStream_t s);
// radix list of a compiled specialisation for n (false: use the generic list)
bool mixed_fixed_radices(int n, int *rad, int *npass);
// the fused Pwelch's own list for n where it differs from the FFT's (fft_mixed.hip)
bool pwelch_fixed_radices(int n, int *rad, int *npass);
hipError_t launch_fft_mixed(const MixedDesc &d, bool inv, int load, const void *in, cd *out,
                            int64_t batch, const cd *tw, double scale, hipStream_t s);
hipError_t launch_bluestein(int log2m, bool inv, const cd *in, cd *out, int64_t n,
                            int64_t batch, const cd *twm, const cd *chirp, const cd *bhat,
                            double scale, hipStream_t s);
// fused chirp-z on M = 16 * RB * 16 (chirpz6k.hip): the smallest such M >=
// 2n - 1 of the kept pass-B radices RB, n >= 129, where it is not above the
// power of 2 (chirpz6k_m; 0 otherwise). tw = W_{16 RB}^k (k < 16) then W_M^k (k < M/16), bhat = FFT_M(b)/M; load LOAD_REAL: float64
// rows (forward only)
int chirpz6k_m(int64_t n);
// the pass radices of the fused chirp-z on m: {16, RB, 16} or {16, R1, R2, 16}
// (chirpz4_kernel); returns their count (0: not a chirpz6k length)
int chirpz6k_radices(int64_t m, int *rad);
hipError_t launch_chirpz6k(int64_t m, bool inv, int load, const void *in, cd *out, int64_t n,
                           int64_t batch, const cd *tw, const cd *chirp, const cd *bhat,
                           double scale, hipStream_t s);
// output-split chirp-z on M = 2^log2m (13 or 14): parts * kpart >= n outputs,
// n + kpart - 1 <= M, bhat = parts tables of M, twm = T_M
hipError_t launch_bluestein_parts(int log2m, bool inv, const cd *in, cd *out, int64_t n,
                                  int64_t batch, int parts, int64_t kpart, const cd *twm,
                                  const cd *chirp, const cd *bhat, double scale, hipStream_t s);
hipError_t launch_global_pass(int radix, bool conj_in, int load, bool conj_scale_out,
                              const void *in, cd *out, const cd *tw, int log2n, int log2ns,
                              int64_t batch, double scale, hipStream_t s);
int pwelch_workers_per_block(int log2f);
hipError_t launch_pwelch(int log2f, const double *x, int64_t nfft, int64_t stride,
                         int64_t seg_begin, int64_t seg_end, int64_t ppw, int64_t nworkers,
                         const double *win, const cd *tw, double *partial, hipStream_t s);
// Noverlap = NFFT/2, Pad = NFFT, 5 <= log2f <= 14 (E even and T | F/2)
hipError_t launch_pwelch_half(int log2f, const double *x, int64_t seg_begin, int64_t seg_end,
                              int64_t ppw, int64_t nworkers, const double *win, const cd *tw,
                              double *partial, hipStream_t s);
// the row kernel (pwelch_row.hip) behind launch_pwelch_half(12, ...)
// any other overlap at F = 4096, Pad = NFFT (pwelch_rowg_kernel)
hipError_t launch_pwelch_rowg4096(const double *x, int64_t stride, int64_t seg_begin,
                                  int64_t seg_end, int64_t ppw, int64_t nworkers,
                                  const double *win, const cd *tw, double *partial,
                                  hipStream_t s);
hipError_t launch_pwelch_row4096(const double *x, int64_t seg_begin, int64_t seg_end, int64_t ppw,
                                 int64_t nworkers, const double *win, const cd *tw,
                                 double *partial, hipStream_t s);
hipError_t launch_reduce_partials(const double *partial, int64_t nworkers, int64_t F, double *acc,
                                  double *scratch, hipStream_t s);
int64_t reduce_scratch_doubles(int64_t nworkers, int64_t F);
// materialised Pwelch: packed segment pairs (nrows rows of flen), then
// per-bin partial power sums over parts of rpp rows (<= 65535 parts)
hipError_t launch_segments_to_complex(const double *x, int64_t nfft, int64_t flen, int64_t stride,
                                      int64_t seg0, int64_t seg_end, int64_t nrows,
                                      const double *win, cd *buf, hipStream_t s);
hipError_t launch_power_partials(const cd *buf, int64_t nrows, int64_t flen, int64_t rpp,
                                 double *partial, hipStream_t s);
// Column pass of the mixed four-step for a single-radix column length L
// (fft_mixed.hip): DFT_L down each of the C columns of batch L x C matrices
// (matrix stride n = L*C), times W_n^(col*k), in place allowed
bool colradix_supported(int L);
hipError_t launch_colradix(int L, bool conj_in, const cd *in, cd *out, int64_t C, int64_t n,
                           int64_t batch, const cd *tw, hipStream_t s);
// FFT2 column pass on row-segment tiles; 4 <= log2l <= 9 (see fft_kernels.hip)
constexpr int kColMinLog2 = 4, kColMaxLog2 = 9;
// twiddle: 0 none, 1 W_R^(group*j), 2 W_R^(col*j); table index mod 2^log2r, or mod
// twn when twn > 0 (a non-power-of-2 N)
// the composed chirp-z's first column pass (DFT_R, R = 2^log2l, 7 ... 10, of
// the R x C view, times W_M^(col j)) on a = x * chirp zero-padded to M = R C,
// the premultiply folded into its loads: x rows of n, out rows of M
hipError_t launch_colfft_chirp(int log2l, bool conj_in, const cd *x, cd *out, int64_t C,
                               int64_t n, const cd *chirp, const cd *twl, const cd *twr,
                               int64_t batch, hipStream_t s);
// row DFT_C (C = 2^log2c, 4 ... 10) of `rows` rows (batch * R, any R) with
// the four-step transpose fused into the store: out[b N + k2 R + k1] =
// DFT_C(in row b R + k1)[k2] (fft_kernels.hip). mode 0 as is, 1 conj and
// scale (inverse), 2 conj(X tab) (the composed chirp-z's b-hat step), 3
// conj(X) tab for k < n into rows of n (its output step; inv: conj and scale)
hipError_t launch_rowfft_t(int log2c, int mode, const cd *in, cd *out, int64_t rows, int64_t R,
                           const cd *tw, double scale, hipStream_t s, const cd *tab = nullptr,
                           int64_t n = 0, bool inv = false);
hipError_t launch_colfft(int log2l, bool conj_in, int twiddle, bool conj_scale_out, const cd *in,
                         cd *out, int64_t C, int64_t ngroups, int64_t in_step, int64_t in_stride,
                         int64_t out_step, int64_t out_stride, const cd *twl, const cd *twr,
                         int log2r, double scale, int64_t batch, int64_t mat_stride,
                         hipStream_t s, int64_t twn = 0);
// batch <= 65535 matrices of rows x cols, consecutive; optional conj+scale
// out, and twiddle tw[r*c] (source row r, column c; needs r*c < twn)
hipError_t launch_transpose(const cd *in, cd *out, int64_t rows, int64_t cols, hipStream_t s,
                            int64_t batch = 1, bool conj_scale = false, double scale = 1.0,
                            const cd *tw = nullptr, int64_t twn = 0, bool tw_conj = false);
// the final transpose of a composed chirp-z FFT_M with the next chirp-z step
// folded in (fft_kernels.hip transpose_blu_kernel): mode 1 conj(v * bhat),
// mode 2 the result rows of n
hipError_t launch_transpose_blu(const cd *in, cd *out, int64_t rows, int64_t cols, int64_t batch,
                                int mode, int64_t n, const cd *tab, bool inv, double scale,
                                hipStream_t s);
hipError_t launch_real_to_complex(const double *in, cd *out, int64_t count, hipStream_t s);
hipError_t launch_chirp_premul(const cd *in, cd *a, int64_t n, int64_t m, int64_t batch,
                               const cd *chirp, bool conj_in, hipStream_t s);
hipError_t launch_bhat_mul_conj(cd *a, int64_t m, int64_t batch, const cd *bhat, hipStream_t s);
hipError_t launch_chirp_postmul(const cd *a, cd *out, int64_t n, int64_t m, int64_t batch,
                                const cd *chirp, bool inv, double scale, hipStream_t s);
hipError_t launch_pointwise_mul(const cd *a, const cd *b, cd *out, int64_t count, hipStream_t s);
hipError_t launch_scale(cd *a, int64_t count, double sc, hipStream_t s);
// fused circular convolution of power-of-2 rows (convolve.hip): out row g =
// IFFT_n(FFT_n(x row g) * FFT_n(y)) in one kernel, 2^kConvMinLog2 <= n <=
// 2^kMaxLdsLog2. yspec = FFT_n(y) (the kernel applies the inverse's 1/n as it
// stores); yspec_stride 0: one spectrum for every row, n: row g takes
// yspec + g n. out may alias x, not yspec.
constexpr int kConvMinLog2 = 8;
hipError_t launch_convolve_lds(int log2n, const cd *x, cd *out, int64_t batch, const cd *tw,
                               const cd *yspec, int64_t yspec_stride, hipStream_t s);
// out[g n + k] = a[g n + k] * b[g b_stride + k] (b_stride 0 or n); out may alias a
hipError_t launch_pointwise_mul_rows(const cd *a, const cd *b, int64_t b_stride, cd *out,
                                     int64_t n, int64_t batch, hipStream_t s);
// Overlap-save FIR filter of real rows (fir.hip): out[c ldo + i] = sum_{k<m}
// h[k] x[c ldx + i - k] for i < out_len (n, or n + m - 1), x zero outside
// [0, n). Blocks of L = F - m + 1 outputs, two per transform, tpr =
// ceil(ceil(out_len / L) / 2) transforms per row. hspec = FFT_F of the
// zero-padded taps (launch_fir_taps, then the plan's transform), hstride 0
// (one for all rows) or F. The fused kernel: F = 2^log2f, 2^kConvMinLog2 ...
// 2^kMaxLdsLog2, m <= F / 2, in fir_ols_workgroups(log2f, channels * tpr)
// workgroups; out must not overlap x. The composed form's ends for any F >=
// m: transforms [g0, g0 + cnt) of the job gathered as complex rows of F, and
// the valid parts of their inverse transforms scattered.
int64_t fir_ols_workgroups(int log2f, int64_t total);
hipError_t launch_fir_ols(int log2f, const double *x, int64_t ldx, double *out, int64_t ldo,
                          int64_t channels, int64_t n, int64_t out_len, int64_t m, const cd *tw,
                          const cd *hspec, int64_t hstride, hipStream_t s);
hipError_t launch_fir_taps(const double *h, int64_t h_rows, int64_t m, int64_t F, cd *out,
                           hipStream_t s);
hipError_t launch_fir_gather(const double *x, int64_t ldx, int64_t g0, int64_t cnt, int64_t tpr,
                             int64_t n, int64_t m, int64_t F, cd *buf, hipStream_t s);
hipError_t launch_fir_scatter(const cd *buf, int64_t g0, int64_t cnt, int64_t tpr, int64_t out_len,
                              int64_t m, int64_t F, double *out, int64_t ldo, hipStream_t s);
// Polyphase resampling of real rows (upfirdn.hip): out[c ldo + j - out_begin] =
// sum_{t<T} hp[p T + t] x[c ldx + i0 - t - x_lo], p = (j down) mod up, i0 =
// (j down) div up, T = ceil(m / up), for j in [out_begin, out_end); the rows
// hold samples [x_lo, x_hi) of the signal (the rest counts as 0). hp: the
// phase-major taps launch_upfirdn_taps writes (up T doubles). The fused form
// runs on the geometry upfirdn_geometry admits (fits == false: none); both
// launchers cut a grid past 2^31 - 1 workgroups into runs of channels.
struct UpfirdnGeo {
  bool fits;     // the fused kernel serves the shape
  int T, Tp;     // taps per phase; the row length of the table in LDS
  int Q, E;      // a thread's slots are Q apart (a multiple of the phase period); outputs each
  bool pad;      // the tile in LDS with one padding double every 32
  int QD;        // Q down / up: the samples between a slot's outputs
  int span;      // samples of a tile: ((Q E - 1) down + up - 1) div up + T
  int lds_doubles;
};
UpfirdnGeo upfirdn_geometry(int64_t m, int64_t up, int64_t down);
hipError_t launch_upfirdn_taps(const double *h, int64_t m, int64_t up, double *hp, hipStream_t s);
hipError_t launch_upfirdn_poly(const UpfirdnGeo &g, const double *x, int64_t ldx, int64_t x_lo,
                               int64_t x_hi, const double *hp, int64_t up, int64_t down,
                               int64_t channels, int64_t out_begin, int64_t out_end, double *out,
                               int64_t ldo, hipStream_t s);
hipError_t launch_upfirdn_plain(const double *x, int64_t ldx, int64_t x_lo, int64_t x_hi,
                                const double *hp, int64_t m, int64_t up, int64_t down,
                                int64_t channels, int64_t out_begin, int64_t out_end, double *out,
                                int64_t ldo, hipStream_t s);
// The analytic signal of real rows (hilbert.hip): row r of x (n samples, ldx
// apart) cut or zero-padded to N, h = IFFT_N(m FFT_N(x)) with the Hilbert
// multiplier m, stored N elements per row, ldo output elements apart: kind 0
// complex128 x + i h, 1 float64 h, 2 float64 sqrt(fma(x, x, h h)). The fused
// kernel: N = 2^log2n where hilbert_lds_applies(N), one row per transform, tw
// the KIND_LDS plan's table; out must not overlap x. The composed form's
// kernels for any N, rows [r0, r0 + cnt): padded real rows of N into buf, the
// multiplier on cnt spectra in place, and the store from the inverse
// transform's real parts (spec; NULL: h = 0).
bool hilbert_lds_applies(int64_t N);
hipError_t launch_hilbert_lds(int log2n, int kind, const double *x, int64_t ldx, int64_t rows,
                              int64_t n, void *out, int64_t ldo, const cd *tw, hipStream_t s);
hipError_t launch_hilbert_gather(const double *x, int64_t ldx, int64_t r0, int64_t cnt, int64_t n,
                                 int64_t N, double *buf, hipStream_t s);
hipError_t launch_hilbert_mask(cd *spec, int64_t cnt, int64_t N, hipStream_t s);
hipError_t launch_hilbert_store(int kind, const double *x, int64_t ldx, int64_t r0, int64_t cnt,
                                int64_t n, int64_t N, const cd *spec, void *out, int64_t ldo,
                                hipStream_t s);
// The cosine transforms of real rows (dct.hip): row r of x (n samples, ldx
// apart) cut or zero-padded to N, type 2 or 3, N float64 per row, ldo apart.
// wk: w_k = exp(-i pi k / (2N)), N entries. Type 2 stores Re(w_k V[k]) scale
// (k = 0: scale0); type 3 takes x[0] a0 and stores v scale. The fused kernel:
// N = 2^log2n where dct_lds_applies(N), one row per transform, tw the KIND_LDS
// plan's table; out may be exactly x (same stride, N <= n), nothing else of
// it. The composed form's kernels for any N, rows [r0, r0 + cnt): type 2's
// permuted padded rows into buf and its store from the full spectra; type 3's
// rows of conj W into spec and its store from the transform's real parts;
// N = 1: out[r ldo] = x[r ldx] c.
bool dct_lds_applies(int64_t N);
hipError_t launch_dct_lds(int log2n, int type, const double *x, int64_t ldx, int64_t rows,
                          int64_t n, double *out, int64_t ldo, const cd *tw, const cd *wk,
                          double a0, double scale, double scale0, hipStream_t s);
hipError_t launch_dct2_gather(const double *x, int64_t ldx, int64_t r0, int64_t cnt, int64_t n,
                              int64_t N, double *buf, hipStream_t s);
hipError_t launch_dct2_store(const cd *spec, const cd *wk, int64_t N, int64_t r0, int64_t cnt,
                             double *out, int64_t ldo, double scale, double scale0,
                             hipStream_t s);
hipError_t launch_dct3_pre(const double *x, int64_t ldx, int64_t r0, int64_t cnt, int64_t n,
                           int64_t N, const cd *wk, double a0, cd *spec, hipStream_t s);
hipError_t launch_dct3_store(const cd *spec, int64_t N, int64_t r0, int64_t cnt, double *out,
                             int64_t ldo, double scale, hipStream_t s);
hipError_t launch_dct_n1(const double *x, int64_t ldx, double *out, int64_t ldo, int64_t rows,
                         double c, hipStream_t s);
// Recursive filtering of real rows by S second-order sections (sosfilt.hip).
// A launch filters the virtual row of io.n samples of every channel from the
// states zi (channels x S x 2; NULL: zeros) and leaves the states after the
// last sample in zf (NULL: not wanted). The virtual row (SosIo) is the row
// itself, its odd extension by `pad` samples at both ends, or a row read from
// its last sample backwards, of which only the last nout results are stored,
// reversed back (sosfiltfilt's second pass).
enum { SOS_IO_PLAIN = 0, SOS_IO_ODD_EXT = 1, SOS_IO_REVERSED = 2 };
struct SosIo {
  const double *src;  // rows of nx doubles, lds apart
  int64_t lds;
  double *dst;        // rows ldd apart: n results (nout where reversed)
  int64_t ldd;
  int64_t n;          // samples filtered: nx, nx + 2 pad, or <= nx where reversed
  int64_t nx, pad, nout;
  int mode;
};
constexpr int kSosThreads = 256, kSosE = 16, kSosTile = kSosThreads * kSosE;
constexpr int kSosMaxFused = 8, kSosMaxSections = 64;
// the time-parallel form's tables, built by the host (gdsp_api.hip): per
// section a block of kSosSecDoubles — b0 b1 b2 a1 a2 at 0, the zero-input
// response c[i][j] (output i of a thread for unit state j) at 8, M^(2^k), k <
// 7, row-major 2 x 2 at 8 + 2 E, M = A^E the state map over a thread's samples
// — then Phi = A^tile of the whole cascade, 2 S x 2 S row-major, at
// kSosPhiOffset. The plain form takes b0 b1 b2 a1 a2 per section, 5 S doubles.
constexpr int kSosSecDoubles = 72, kSosPhiOffset = kSosMaxFused * kSosSecDoubles;
constexpr int kSosTableDoubles = kSosPhiOffset + 4 * kSosMaxFused * kSosMaxFused;
constexpr int kSosTablePart = 448;
struct SosTablePart {
  int offset, count;
  double v[kSosTablePart];
};
hipError_t launch_sos_tables(const double *host, int64_t count, double *tab, hipStream_t s);
// scratch: channels (2 T + 1) 2 S doubles, T = ceil(n / tile) (pass 1's end
// states and pass 2's entry states); not read where a row is one tile
hipError_t launch_sos_tiles(const SosIo &io, const double *tab, int S, int64_t channels,
                            const double *zi, double *zf, double *scratch, hipStream_t s);
hipError_t launch_sos_plain(const SosIo &io, const double *coef, int S, int64_t channels,
                            const double *zi, double *zf, hipStream_t s);
hipError_t launch_sos_ffzi(const SosIo &io, int64_t at, const double *zi, int S, int64_t channels,
                           double *zi_rows, hipStream_t s);
// The chirp-z transform of rows (czt.hip): row r of x (n float64 when `real`,
// else complex128, ldx elements apart) times A, convolved on F = 2^log2f >= n
// + m - 1 points with the chirp whose spectrum over F is vhat, times P; m
// complex128 per row, ldo apart. A, vhat and P have F entries (A zero past n,
// P zero past m). The fused kernel where czt_lds_applies(F), tw the KIND_LDS
// plan's table; out must not overlap x. The composed form's kernels, rows [r0,
// r0 + cnt): rows times A padded to F into buf, conj(spec vhat) in place, and
// conj(spec) P stored.
bool czt_lds_applies(int64_t F);
hipError_t launch_czt_lds(int log2f, bool real, const void *x, int64_t ldx, int64_t rows,
                          int64_t n, int64_t m, cd *out, int64_t ldo, const cd *tw, const cd *A,
                          const cd *vhat, const cd *P, hipStream_t s);
hipError_t launch_czt_pre(bool real, const void *x, int64_t ldx, int64_t r0, int64_t cnt,
                          int64_t n, int64_t F, const cd *A, cd *buf, hipStream_t s);
hipError_t launch_czt_mul(cd *spec, const cd *vhat, int64_t cnt, int64_t F, hipStream_t s);
hipError_t launch_czt_post(const cd *spec, int64_t F, int64_t r0, int64_t cnt, int64_t m,
                           const cd *P, cd *out, int64_t ldo, hipStream_t s);
// wav.ReadFloats conversion (wav.hip): audio_format 1 (bits 8 / 16) or 3
hipError_t launch_wav_decode(const void *in, int64_t count, int audio_format, int bits,
                             void *out, bool f64, hipStream_t s);
// interleaved frames into planar float64 rows: out[c ld + i] = sample c of frame i
hipError_t launch_wav_decode_planar(const void *in, int64_t frames, int channels,
                                    int audio_format, int bits, double *out, int64_t ld,
                                    hipStream_t s);
hipError_t launch_fill_uniform(double *out, int64_t count, uint64_t seed, uint64_t offset,
                               hipStream_t s);

#endif  // __HIPCC_RTC__

}  // namespace gdsp
