// welch.hip — the Welch family of the C ABI (include/gdsp_fft.h): Pwelch, the
// batched Pwelch over the channels of a planar batch, the batched cross
// spectra (Cpsd, coherence), the per-segment spectra (STFT, spectrogram) and
// their overlap-add inverse (ISTFT); with them spectral.Segment's count and
// the Hann table. Host arithmetic only: the kernels are in pwelch_*.hip,
// cpsd_batch.hip, stft_batch.hip, istft_batch.hip and the transform files,
// behind launch.hpp.
#include <math.h>

#include <string>
#include <vector>

#include "fft_device.hpp"
#include "gdsp_fft.h"
#include "launch.hpp"
#include "api_internal.hpp"
#include "plan.hpp"

using gdsp::cd;
using namespace gdsp_api;

void gdsp_api::hann_table(int64_t L, double *r) {  // window/window.go:62-76
  if (L <= 0) return;
  if (L == 1) {
    r[0] = 1;
    return;
  }
  const int64_t N = L - 1;
  const double coef = 2 * M_PI / (double)N;
  for (int64_t i = 0; i <= N; ++i) r[i] = 0.5 * (1 - cos(coef * (double)i));
}

int gdsp_api::segment_count(int64_t lx, int64_t size, int64_t noverlap, int64_t *count) {
  const int64_t stride = size - noverlap;  // spectral/spectral.go:22-33
  if (lx == size) {
    *count = 1;
  } else if (lx > size) {
    if (stride == 0) return fail(GDSP_ERR_DIVIDE_BY_ZERO, "integer divide by zero");
    *count = (lx - size) / stride + 1;
    if (*count < 0) return fail(GDSP_ERR_INVALID, "makeslice: len out of range");
  } else {
    *count = 0;
  }
  return GDSP_OK;
}

const double *gdsp_api::hann_or(const double *w, int64_t L, std::vector<double> &store) {
  if (w) return w;
  store.resize((size_t)L);
  hann_table(L, store.data());
  return store.data();
}

bool gdsp_api::welch_defaults(int64_t *nfft, int64_t *pad) {
  if (*nfft == 0) *nfft = 256;
  if (*pad == 0) *pad = *nfft;
  return *nfft >= 0 && *pad >= 0;
}

int gdsp_api::welch_shape(int64_t n, int64_t nfft, int64_t pad, int64_t noverlap, WelchShape *w) {
  w->lx = n < nfft ? nfft : n;
  w->flen = pad > nfft ? pad : nfft;
  w->lp = pad / 2 + 1;
  return segment_count(w->lx, nfft, noverlap, &w->nsegs);
}

namespace {

// The fused kernels address a pair's (or a wave's group of pairs') samples
// with 32-bit offsets from one base; a very negative Noverlap (spectral.go:
// 22-43 allows it) spreads the segments beyond that, so strides above 2^22
// samples take the materialised paths, which index in 64 bits.
constexpr int64_t kWelchMaxFusedStride = (int64_t)1 << 22;

// the window's norm (spectral/pwelch.go:124-132; no window: Hann) and the
// frequencies of the Pad / 2 + 1 bins (:138-142)
double welch_norm(const double *win_nfft, int64_t nfft, double fs, int scale_off) {
  std::vector<double> hw;
  win_nfft = hann_or(win_nfft, nfft, hw);
  double norm = 0;
  for (int64_t i = 0; i < nfft; ++i) norm += win_nfft[i] * win_nfft[i];
  if (!scale_off) norm *= fs;
  return norm;
}

void welch_freqs(int64_t pad, double fs, double *freqs) {
  const double coef = fs / (double)pad;
  for (int64_t j = 0; j < pad / 2 + 1; ++j) freqs[j] = (double)j * coef;
}

// The partial sums of an accumulate call and the scratch of their reduction
// into the accumulators in the fixed order: `rows` rows of F doubles
// (launch_reduce_partials), or that per channel (launch_reduce_batch).
struct Partials {
  DevBuf part, red;
  double *p() const { return (double *)part.p; }
  int alloc(int64_t rows, int64_t F, hipStream_t s) {
    STCHK(part.alloc((size_t)rows * (size_t)F * sizeof(double), s, SLOT_PW_PART));
    return red.alloc((size_t)gdsp::reduce_scratch_doubles(rows, F) * sizeof(double), s,
                     SLOT_PW_RED);
  }
  int reduce(int64_t rows, int64_t F, double *d_acc, hipStream_t s) {
    HIPCHK(gdsp::launch_reduce_partials(p(), rows, F, d_acc, (double *)red.p, s));
    return GDSP_OK;
  }
  int alloc_batch(int64_t channels, int64_t rows, int64_t F, hipStream_t s) {
    STCHK(part.alloc((size_t)channels * (size_t)rows * (size_t)F * sizeof(double), s,
                     SLOT_PW_PART));
    return red.alloc(
        (size_t)gdsp::reduce_batch_scratch_doubles(channels, rows, F) * sizeof(double), s,
        SLOT_PW_RED);
  }
  int reduce_batch(int64_t channels, int64_t rows, int64_t F, double *d_acc, hipStream_t s) {
    HIPCHK(gdsp::launch_reduce_batch(p(), channels, rows, F, d_acc, (double *)red.p, s));
    return GDSP_OK;
  }
};

// npairs packed segment pairs over at most `target` persistent workers, each a
// contiguous range of ppw pairs
void pair_workers(int64_t npairs, int64_t target, int64_t *ppw, int64_t *nworkers) {
  if (target > npairs) target = npairs;
  *ppw = (npairs + target - 1) / target;
  *nworkers = (npairs + *ppw - 1) / *ppw;
}

// channels per launch of a batched kernel: the partials (per_channel doubles
// each) within the materialised path's 512 MiB
int64_t channels_per_launch(int64_t per_channel, int64_t channels) {
  const int64_t cpl = ((int64_t)1 << 26) / per_channel;
  return cpl < 1 ? 1 : (cpl > channels ? channels : cpl);
}

// Whether a batched kernel (its lengths: applies) serves transforms of flen
// over this stride, unless the flag `off` is set. The flags are
// gdsp_set_algorithm's: algo_flags() differs from them only inside a plan
// build, and a build (the race included) runs exec_plan, never a Welch entry.
bool batch_fused(int64_t flen, int64_t stride, bool (*applies)(int), unsigned off) {
  return flen > 0 && is_pow2(flen) && applies(ilog2(flen)) && stride <= kWelchMaxFusedStride &&
         !(gdsp::algo_flags() & off);
}

// The batched kernel (pwelch_batch.hip) serves the lengths of the wave
// kernels; every other length and stride, and any shape under
// GDSP_ALGO_NO_FUSED_PWELCH_BATCH, loops over the channels with
// gdsp_pwelch_accumulate_device.
bool pwelch_batch_fused(int64_t flen, int64_t stride) {
  return batch_fused(flen, stride, gdsp::pwelch_batch_applies, GDSP_ALGO_NO_FUSED_PWELCH_BATCH);
}

// The fused kernel (cpsd_batch.hip) serves the lengths of the batched Pwelch;
// every other length and stride, and any shape under GDSP_ALGO_NO_FUSED_CPSD,
// runs the materialised form.
bool cpsd_batch_fused(int64_t flen, int64_t stride) {
  return batch_fused(flen, stride, gdsp::cpsd_batch_applies, GDSP_ALGO_NO_FUSED_CPSD);
}

// The fused per-segment kernel (stft_batch.hip) serves the same lengths and
// strides; every other one, and any shape under GDSP_ALGO_NO_FUSED_STFT, runs
// the materialised form.
bool stft_batch_fused(int64_t flen, int64_t stride) {
  return batch_fused(flen, stride, gdsp::stft_batch_applies, GDSP_ALGO_NO_FUSED_STFT);
}

// gdsp_pwelch_batch_fused / gdsp_cpsd_batch_fused / gdsp_stft_batch_fused: the
// predicate on a call's options
int fused_answer(bool (*fused)(int64_t, int64_t), int64_t channels, int64_t n, int64_t nfft,
                 int64_t pad, int64_t noverlap) {
  if (channels < 0 || n < 0 || !welch_defaults(&nfft, &pad)) return 0;
  return fused(pad > nfft ? pad : nfft, nfft - noverlap) ? 1 : 0;
}

// ---- per-segment spectra: STFT (complex rows) and spectrogram (power rows) ----

// elements of a host call's device output, and complex elements of a
// materialised chunk's rows: 512 MiB of complex128, as the other entries
constexpr int64_t kStftChunkElems = (int64_t)1 << 25;

// gdsp_stft_batch_device / gdsp_spectrogram_batch_device
int stft_device(bool power, const double *d_x, int64_t ldx, int64_t channels, int64_t n,
                int64_t nfft, int64_t pad, int64_t noverlap, int64_t seg_begin, int64_t seg_end,
                const double *d_win_seg, double norm, void *d_out, int64_t ld_seg, int64_t ld_chan,
                void *stream) {
  if (nfft <= 0 || pad <= 0 || seg_begin < 0 || seg_end < seg_begin)
    return fail(GDSP_ERR_INVALID, "bad STFT geometry");
  if (channels < 0 || n < 0 || (channels > 1 && ldx < n))
    return fail(GDSP_ERR_INVALID, "bad batch geometry");
  const int64_t lp = pad / 2 + 1, nseg = seg_end - seg_begin;
  if (ld_seg < lp || (channels > 1 && nseg > 0 && ld_chan / nseg < ld_seg))
    return fail(GDSP_ERR_INVALID, "output strides below the rows");
  const int64_t stride = nfft - noverlap;
  // Segment divides by the stride only where there is more than one segment
  if (stride == 0 && seg_end > 1) return fail(GDSP_ERR_DIVIDE_BY_ZERO, "integer divide by zero");
  if (channels == 0 || nseg == 0) return GDSP_OK;
  if (!d_x || !d_win_seg || !d_out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  // a negative stride (Noverlap > NFFT) leaves at most segment 0 (Segment)
  if ((seg_end - 1) * stride + nfft > n || (stride < 0 && seg_end > 1))
    return fail(GDSP_ERR_INVALID, "segments exceed the signal");
  const int64_t flen = pad > nfft ? pad : nfft;
  const size_t esize = power ? sizeof(double) : sizeof(cd);
  hipStream_t s = (hipStream_t)stream;
  gdsp_plan *p = nullptr;
  STCHK(get_plan(flen, &p));
  // the plan's kind is checked because the kernel reads that plan's twiddle
  // table (gdsp_cpsd_batch_accumulate_device)
  if (stft_batch_fused(flen, stride) && p->kind == KIND_LDS) {
    int64_t wpc = 0, gpw = 0;
    gdsp::stft_batch_geometry(p->log2n, channels, nseg, &wpc, &gpw);
    multi_unit(gpw);
    HIPCHK(gdsp::launch_stft_batch(p->log2n, power, d_x, ldx, channels, wpc, nfft, stride,
                                   seg_begin, seg_end, gpw, d_win_seg, p->tw, d_out, lp, ld_seg,
                                   ld_chan, norm, s));
    return GDSP_OK;
  }
  // materialised form: chunks of at most 512 MiB of complex rows (and their
  // real rows), whole channels where a channel's segments fit, else one
  // channel's segments in runs; one real segment per transform
  int64_t maxrows = kStftChunkElems / flen;
  if (maxrows < 1) maxrows = 1;
  const int64_t ns_max = nseg < maxrows ? nseg : maxrows;  // segments per run
  int64_t cpl = maxrows / ns_max;                           // channels per launch
  if (cpl > channels) cpl = channels;
  DevBuf rows, buf;
  STCHK(rows.alloc((size_t)cpl * (size_t)ns_max * (size_t)flen * sizeof(double), s, SLOT_ST_ROWS));
  STCHK(buf.alloc((size_t)cpl * (size_t)ns_max * (size_t)flen * sizeof(cd), s, SLOT_PW_BUF));
  for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
    const int64_t nc = channels - c0 < cpl ? channels - c0 : cpl;
    later_chunk(c0);
    void *const oc = (char *)d_out + (size_t)c0 * (size_t)ld_chan * esize;
    for (int64_t j0 = 0; j0 < nseg; j0 += ns_max) {
      const int64_t ns = nseg - j0 < ns_max ? nseg - j0 : ns_max;
      later_chunk(j0);
      HIPCHK(gdsp::launch_stft_gather(d_x + c0 * ldx, ldx, nc, ns, nfft, flen, stride,
                                      seg_begin + j0, d_win_seg, (double *)rows.p, s));
      STCHK(exec_plan(p, rows.p, (cd *)buf.p, nc * ns, false, gdsp::LOAD_REAL, s));
      HIPCHK(gdsp::launch_stft_rows((const cd *)buf.p, nc, ns, flen, lp, power, norm, oc, j0,
                                    ld_seg, ld_chan, s));
    }
  }
  return GDSP_OK;
}

// gdsp_stft_batch / gdsp_spectrogram_batch: out is channels x nsegs x lp,
// dense. The device output holds at most kStftChunkElems elements: segment
// ranges that begin at even indices (the pairs of the fused kernel, and with
// them every bit of a row, do not depend on where the cut falls), each copied
// back before the next is computed.
int stft_host(bool power, const double *x, int64_t channels, int64_t n, int64_t ldx, double fs,
              int64_t nfft, int64_t pad, int64_t noverlap, const double *win_seg,
              const double *win_nfft, int scale_off, double *out, double *freqs, double *times,
              int64_t *nsegs_out, int64_t *lp_out) {
  if (!nsegs_out || !lp_out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  *nsegs_out = *lp_out = 0;
  if (channels < 0 || n < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (n == 0) return GDSP_OK;
  if (!welch_defaults(&nfft, &pad)) return fail(GDSP_ERR_INVALID, "negative NFFT/Pad");
  if (channels > 1 && ldx < n) return fail(GDSP_ERR_INVALID, "ldx below the channel length");
  WelchShape w;
  STCHK(welch_shape(n, nfft, pad, noverlap, &w));
  if ((power && (!freqs || (w.nsegs > 0 && !times))) ||
      (channels > 0 && w.nsegs > 0 && (!x || !out)))
    return fail(GDSP_ERR_INVALID, "NULL pointer");
  const int64_t stride = nfft - noverlap;
  if (power) {
    welch_freqs(pad, fs, freqs);
    // the segment's centre (scipy.signal.spectrogram, matplotlib specgram)
    for (int64_t i = 0; i < w.nsegs; ++i)
      times[i] = ((double)(i * stride) + 0.5 * (double)nfft) / fs;
  }
  *nsegs_out = w.nsegs;
  *lp_out = w.lp;
  if (channels == 0 || w.nsegs == 0) return GDSP_OK;
  const double norm = power ? welch_norm(win_nfft, nfft, fs, scale_off) : 1.0;
  std::vector<double> hseg;
  win_seg = hann_or(win_seg, w.flen, hseg);
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const int64_t dpe = power ? 1 : 2;  // doubles per output element
  int64_t per = (kStftChunkElems / (channels * w.lp)) & ~(int64_t)1;  // segments per range: even
  if (per < 2) per = 2;
  if (per > w.nsegs) per = w.nsegs;
  DevBuf dx, dw, dout;
  STCHK(dx.alloc((size_t)channels * (size_t)w.lx * sizeof(double), s, SLOT_IN));
  STCHK(dw.alloc((size_t)w.flen * sizeof(double), s, SLOT_AUX));
  STCHK(dout.alloc((size_t)channels * (size_t)per * (size_t)w.lp * (size_t)dpe * sizeof(double), s,
                   SLOT_ST_OUT));
  for (int64_t s0 = 0; s0 < w.nsegs; s0 += per) {
    const int64_t ns = w.nsegs - s0 < per ? w.nsegs - s0 : per;
    later_chunk(s0);
    STCHK(run_queued(s, [&]() -> int {
      if (s0 == 0) {
        STCHK(stage_rows((double *)dx.p, x, channels, n, ldx, w.lx, s));
        STCHK(copy_h2d(dw.p, win_seg, (size_t)w.flen * sizeof(double), s));
      }
      return stft_device(power, (const double *)dx.p, w.lx, channels, w.lx, nfft, pad, noverlap, s0,
                         s0 + ns, (const double *)dw.p, norm, dout.p, w.lp, ns * w.lp, s);
    }));
    // channel c's rows [s0, s0 + ns): dense on the device, nsegs rows apart on the host
    STCHK(unstage_rows(out + s0 * w.lp * dpe, (const double *)dout.p, channels, ns * w.lp * dpe,
                       w.nsegs * w.lp * dpe, s));
  }
  return GDSP_OK;
}

// ---- the overlap-add inverse of the STFT rows ----------------------------------

// complex elements of a host call's device copy of X, and of a materialised
// chunk's dense rows: 512 MiB of complex128, a constant of this entry
constexpr int64_t kIstftChunkElems = (int64_t)1 << 25;

// The fused kernel (istft_batch.hip) serves F = Pad of the batched kernels'
// lengths with 0 < stride <= NFFT <= 4 stride: at most 4 segments over a
// sample, no gaps between segments (a negative Noverlap would make the D table
// as long as the gaps).
bool istft_batch_fused(int64_t nfft, int64_t pad, int64_t stride) {
  return pad >= nfft && stride >= 1 && stride <= nfft && nfft <= 4 * stride &&
         batch_fused(pad, stride, gdsp::istft_batch_applies, GDSP_ALGO_NO_FUSED_ISTFT);
}

// the first and the last segment that cover a sample of [i0, i1)
void istft_cover(int64_t i0, int64_t i1, int64_t nsegs, int64_t nfft, int64_t stride,
                 int64_t *slo, int64_t *shi) {
  *slo = i0 >= nfft ? (i0 - nfft) / stride + 1 : 0;
  *shi = (i1 - 1) / stride;
  if (*shi > nsegs - 1) *shi = nsegs - 1;
}

// gdsp_istft_batch_device
int istft_device(const void *d_X, int64_t ld_seg, int64_t ld_chan, int64_t channels,
                 int64_t nsegs, int64_t seg_row0, int64_t seg_rows, int64_t nfft, int64_t pad,
                 int64_t noverlap, const double *d_win_seg, int64_t out_begin, int64_t out_end,
                 double *d_out, int64_t ldo, void *stream) {
  if (nfft <= 0 || pad < nfft) return fail(GDSP_ERR_INVALID, "bad ISTFT geometry: Pad below NFFT");
  if (channels < 0 || nsegs < 0 || seg_row0 < 0 || seg_rows < 0 || seg_rows > nsegs ||
      seg_row0 > nsegs - seg_rows)
    return fail(GDSP_ERR_INVALID, "bad batch geometry");
  if (out_begin < 0 || out_end < out_begin) return fail(GDSP_ERR_INVALID, "bad sample range");
  const int64_t lp = pad / 2 + 1, len = out_end - out_begin;
  if (ld_seg < lp || (channels > 1 && seg_rows > 0 && ld_chan / seg_rows < ld_seg))
    return fail(GDSP_ERR_INVALID, "input strides below the rows");
  if (channels > 1 && ldo < len) return fail(GDSP_ERR_INVALID, "ldo below the range");
  int64_t stride = nfft - noverlap;
  if (stride == 0 && nsegs > 1) return fail(GDSP_ERR_DIVIDE_BY_ZERO, "integer divide by zero");
  if (stride < 0 && nsegs > 1) return fail(GDSP_ERR_INVALID, "a negative stride");
  if (nsegs == 0) {
    if (len > 0) return fail(GDSP_ERR_INVALID, "sample range past the signal");
    return GDSP_OK;
  }
  const bool fused = istft_batch_fused(nfft, pad, stride);
  if (nsegs == 1 && stride < 1) stride = nfft;  // one segment: the stride places nothing
  if (stride > (INT64_MAX - nfft) / nsegs) return fail(GDSP_ERR_INVALID, "signal length overflows");
  const int64_t n_full = (nsegs - 1) * stride + nfft;
  if (out_end > n_full) return fail(GDSP_ERR_INVALID, "sample range past the signal");
  if (channels == 0 || len == 0) return GDSP_OK;
  if (!d_X || !d_win_seg || !d_out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  int64_t slo = 0, shi = 0;
  istft_cover(out_begin, out_end, nsegs, nfft, stride, &slo, &shi);
  // a range inside a gap between segments (a negative Noverlap) needs no row
  const bool covered = slo <= shi;
  if (covered && fused) {
    // the fused kernel transforms rows (2p, 2p + 1) together: a row's bits
    // depend on its partner, so the range's rows are needed as whole pairs
    slo &= ~(int64_t)1;
    if (shi + 1 < nsegs) shi |= 1;
  }
  if (covered && (slo < seg_row0 || shi >= seg_row0 + seg_rows))
    return fail(GDSP_ERR_INVALID, fused ? "rows of the range are missing (whole pairs are needed)"
                                        : "rows of the range are missing");
  hipStream_t s = (hipStream_t)stream;
  gdsp_plan *p = nullptr;
  STCHK(get_plan(pad, &p));
  if (fused && p->kind == KIND_LDS) {
    const int64_t owned = gdsp::istft_group_segments(p->log2n) * stride;
    const int64_t g_begin = out_begin / owned, g_end = (out_end - 1) / owned + 1;
    const int halo = (int)((nfft - stride + owned - 1) / owned);
    int64_t wpc = 0, gpw = 0;
    gdsp::istft_batch_geometry(p->log2n, channels, g_end - g_begin, halo, &wpc, &gpw);
    DevBuf dtab;
    STCHK(dtab.alloc((size_t)gdsp::istft_dtable_doubles(stride) * sizeof(double), s, SLOT_IS_D));
    HIPCHK(gdsp::launch_istft_dtable(d_win_seg, nfft, stride, nsegs, (double *)dtab.p, s));
    multi_unit(gpw);
    HIPCHK(gdsp::launch_istft_batch(p->log2n, (const cd *)d_X, ld_seg, ld_chan, channels, nsegs,
                                    seg_row0, seg_row0 + seg_rows, nfft, stride, g_begin, g_end,
                                    wpc, gpw, d_win_seg, (const double *)dtab.p, p->tw, out_begin,
                                    out_end, d_out, ldo, s));
    return GDSP_OK;
  }
  // materialised form: chunks of at most 512 MiB of dense complex rows, whole
  // channels where the rows of a channel's range fit, else one channel's range
  // in runs of samples, each with the rows that reach into it (its halo)
  int64_t maxrows = kIstftChunkElems / pad;
  const int64_t reach = (nfft + stride - 1) / stride;  // segments over a sample
  if (maxrows < reach + 1) maxrows = reach + 1;
  const int64_t need = covered ? shi - slo + 1 : 1;
  int64_t cpl = 1, run = len;  // channels per launch, samples per run
  if (need <= maxrows) {
    cpl = maxrows / need < channels ? maxrows / need : channels;
  } else {
    run = (maxrows - reach) * stride;
  }
  const int64_t ns_max = need <= maxrows ? need : maxrows;
  DevBuf buf;
  STCHK(buf.alloc((size_t)cpl * (size_t)ns_max * (size_t)pad * sizeof(cd), s, SLOT_PW_BUF));
  const cd *const X = (const cd *)d_X;
  for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
    const int64_t nc = channels - c0 < cpl ? channels - c0 : cpl;
    later_chunk(c0);
    for (int64_t i0 = out_begin; i0 < out_end; i0 += run) {
      const int64_t i1 = out_end - i0 < run ? out_end : i0 + run;
      later_chunk(i0 - out_begin);
      int64_t a = 0, b = 0;
      istft_cover(i0, i1, nsegs, nfft, stride, &a, &b);
      const int64_t ns = b - a + 1;
      double *const o = d_out + c0 * ldo + (i0 - out_begin);
      if (ns < 1) {  // a run inside a gap between segments: D == 0, exact zeros
        HIPCHK(hipMemset2DAsync(o, (size_t)ldo * sizeof(double), 0,
                                (size_t)(i1 - i0) * sizeof(double), (size_t)nc, s));
        continue;
      }
      HIPCHK(gdsp::launch_istft_complete(X + c0 * ld_chan, ld_seg, ld_chan, seg_row0, nc, a, ns,
                                         pad, (cd *)buf.p, s));
      STCHK(exec_plan(p, buf.p, (cd *)buf.p, nc * ns, true, gdsp::LOAD_COMPLEX, s));
      HIPCHK(gdsp::launch_istft_ola((const cd *)buf.p, nc, a, ns, nsegs, pad, nfft, stride,
                                    d_win_seg, i0, i1, o, ldo, s));
    }
  }
  return GDSP_OK;
}

// gdsp_istft_batch: X is channels x nsegs x lp, dense. The device copy of X
// holds at most kIstftChunkElems elements: output ranges that begin at
// multiples of 2 stride (whole pairs of the fused kernel), each uploaded with
// the pairs that reach into it, each range copied back before the next.
int istft_host(const void *X, int64_t channels, int64_t nsegs, int64_t nfft, int64_t pad,
               int64_t noverlap, const double *win_seg, int64_t n, double *out, int64_t ldo,
               int64_t *n_out) {
  if (!n_out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  *n_out = 0;
  if (channels < 0 || nsegs < 0 || n < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (!welch_defaults(&nfft, &pad)) return fail(GDSP_ERR_INVALID, "negative NFFT/Pad");
  if (nfft == 0 || pad < nfft) return fail(GDSP_ERR_INVALID, "Pad below NFFT has no inverse");
  int64_t stride = nfft - noverlap;
  if (stride == 0 && nsegs > 1) return fail(GDSP_ERR_DIVIDE_BY_ZERO, "integer divide by zero");
  if (stride < 0 && nsegs > 1) return fail(GDSP_ERR_INVALID, "a negative stride");
  if (nsegs == 0) return n > 0 ? fail(GDSP_ERR_INVALID, "n past the signal") : GDSP_OK;
  if (nsegs == 1 && stride < 1) stride = nfft;
  if (stride > (INT64_MAX - nfft) / nsegs) return fail(GDSP_ERR_INVALID, "signal length overflows");
  const int64_t n_full = (nsegs - 1) * stride + nfft;
  if (n > n_full) return fail(GDSP_ERR_INVALID, "n past the signal");
  if (n == 0) n = n_full;
  if (channels > 1 && ldo < n) return fail(GDSP_ERR_INVALID, "ldo below the row length");
  if (channels > 0 && (!X || !out)) return fail(GDSP_ERR_INVALID, "NULL pointer");
  *n_out = n;
  if (channels == 0) return GDSP_OK;
  const int64_t lp = pad / 2 + 1;
  std::vector<double> hseg;
  win_seg = hann_or(win_seg, pad, hseg);
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  // rows per range: the range's own pairs and the two pairs before them
  const int64_t reach = (nfft + stride - 1) / stride;
  const int64_t halo = (reach + 1) & ~(int64_t)1;
  const int64_t fit = kIstftChunkElems / (channels * lp);
  int64_t per = nsegs, rows_max = nsegs;  // new rows per range, rows on the device
  if (fit < nsegs) {
    per = (fit - halo - 2) & ~(int64_t)1;
    if (per < 2) per = 2;
    rows_max = per + halo + 2 < nsegs ? per + halo + 2 : nsegs;
  }
  const int64_t span = per >= nsegs ? n : per * stride;  // samples per range
  DevBuf dx, dw, dout;
  STCHK(dx.alloc((size_t)channels * (size_t)rows_max * (size_t)lp * sizeof(cd), s, SLOT_IN));
  STCHK(dw.alloc((size_t)pad * sizeof(double), s, SLOT_AUX));
  STCHK(dout.alloc((size_t)channels * (size_t)(span < n ? span : n) * sizeof(double), s,
                   SLOT_ST_OUT));
  const cd *const hx = (const cd *)X;
  for (int64_t i0 = 0; i0 < n; i0 += span) {
    const int64_t i1 = n - i0 < span ? n : i0 + span;
    later_chunk(i0);
    int64_t a = 0, b = 0;
    istft_cover(i0, i1, nsegs, nfft, stride, &a, &b);
    if (b < a) b = a;  // a range inside a gap: no row is needed, one is passed
    a &= ~(int64_t)1;  // whole pairs
    if (b + 1 < nsegs && !(b & 1)) ++b;
    const int64_t nr = b - a + 1;
    if (nr > rows_max) return fail(GDSP_ERR_INVALID, "internal: ISTFT range rows");
    STCHK(run_queued(s, [&]() -> int {
      if (i0 == 0) STCHK(copy_h2d(dw.p, win_seg, (size_t)pad * sizeof(double), s));
      for (int64_t c = 0; c < channels; ++c)
        STCHK(copy_h2d((cd *)dx.p + c * nr * lp, hx + (c * nsegs + a) * lp,
                       (size_t)nr * (size_t)lp * sizeof(cd), s));
      return istft_device(dx.p, lp, nr * lp, channels, nsegs, a, nr, nfft, pad, noverlap,
                          (const double *)dw.p, i0, i1, (double *)dout.p, i1 - i0, s);
    }));
    STCHK(unstage_rows(out + i0, (const double *)dout.p, channels, i1 - i0, ldo, s));
  }
  return GDSP_OK;
}

}  // namespace

extern "C" {

int gdsp_segment_count(int64_t lx, int64_t size, int64_t noverlap, int64_t *count) {
  if (!count) return fail(GDSP_ERR_INVALID, "NULL pointer");
  return segment_count(lx, size, noverlap, count);
}

int gdsp_window_hann(int64_t L, double *out) {
  if (L < 0) return fail(GDSP_ERR_INVALID, "negative size");
  hann_table(L, out);
  return GDSP_OK;
}

int gdsp_pwelch_accumulate_device(const double *d_x, int64_t n, int64_t nfft, int64_t pad,
                                  int64_t noverlap, int64_t seg_begin, int64_t seg_end,
                                  const double *d_win_seg, double *d_acc, void *stream) {
  if (nfft <= 0 || pad <= 0 || seg_begin < 0 || seg_end < seg_begin)
    return fail(GDSP_ERR_INVALID, "bad Pwelch geometry");
  if (seg_end == seg_begin) return GDSP_OK;
  const int64_t stride = nfft - noverlap;
  if ((seg_end - 1) * stride + nfft > n)
    return fail(GDSP_ERR_INVALID, "segments exceed the signal");
  const int64_t flen = pad > nfft ? pad : nfft;
  hipStream_t s = (hipStream_t)stream;  // NULL = the null stream
  gdsp_plan *p = nullptr;
  STCHK(get_plan(flen, &p));
  const int64_t nseg = seg_end - seg_begin;
  const bool fused = stride <= kWelchMaxFusedStride;
  Partials pt;
  if (fused && p->kind == KIND_LDS && gdsp::pwelch_wave_applies(p->log2n)) {
    // 64 <= F <= 1024: wave-resident transforms, no workgroup barriers
    // (pwelch_wave.hip), every wave a persistent worker over pair groups;
    // F = 2048: two-wave workgroups
    const bool half = 2 * noverlap == nfft && flen == nfft;
    int64_t gpw = 0, nblk = 0, nrows = 0;
    gdsp::pwelch_wave_geometry(p->log2n, half, nseg, &gpw, &nblk, &nrows);
    multi_unit(gpw);
    STCHK(pt.alloc(nrows, flen, s));
    HIPCHK(gdsp::launch_pwelch_wave(p->log2n, half, d_x, nfft, stride, seg_begin, seg_end, gpw,
                                    nblk, d_win_seg, p->tw, pt.p(), s));
    return pt.reduce(nrows, flen, d_acc, s);
  }
  // The other fused kernels: packed segment pairs, persistent workers over
  // contiguous pair ranges (the 50 % overlap of consecutive pairs is re-read
  // from L2), at most 2048 workers per workgroup slot: 512 / 1024 / 4096
  // measured 2.86 / 2.81 / 2.77 against 2.76 ms for 2048 (BASELINE configs[4])
  constexpr int64_t wmul = 2048;
  const int64_t npairs = (nseg + 1) / 2;
  int64_t ppw = 0, nworkers = 0;
  auto workers = [&](int64_t target) -> int {
    pair_workers(npairs, target, &ppw, &nworkers);
    multi_unit(ppw);
    return pt.alloc(nworkers, flen, s);
  };
  if (fused && p->kind == KIND_LDS && p->log2n >= 4) {
    STCHK(workers(wmul * (int64_t)gdsp::pwelch_workers_per_block(p->log2n)));
    if (2 * noverlap == nfft && flen == nfft && p->log2n >= 5) {
      // half overlap: each sample loaded once, window in LDS
      HIPCHK(gdsp::launch_pwelch_half(p->log2n, d_x, seg_begin, seg_end, ppw, nworkers, d_win_seg,
                                      p->tw, pt.p(), s));
    } else if (p->log2n == 12 && flen == nfft) {
      // any other overlap at 4096: the row kernel's structure without the carry
      HIPCHK(gdsp::launch_pwelch_rowg4096(d_x, stride, seg_begin, seg_end, ppw, nworkers,
                                          d_win_seg, p->tw, pt.p(), s));
    } else {
      HIPCHK(gdsp::launch_pwelch(p->log2n, d_x, nfft, stride, seg_begin, seg_end, ppw, nworkers,
                                 d_win_seg, p->tw, pt.p(), s));
    }
    return pt.reduce(nworkers, flen, d_acc, s);
  }
  // the fused Pwelch on a compiled or runtime-compiled specialisation, on the
  // Pwelch's own list where it has one (md_pw); 0 workers per block where its
  // kernel cannot stage a pair this far apart (negative Noverlap)
  const bool own = p->md_pw.n > 0 && !p->jit;
  const gdsp::MixedDesc &pmd = own ? p->md_pw : p->md;
  const int wpb_fixed =
      !fused || p->kind != KIND_MIXED ? 0
      : p->jit                        ? gdsp::jit_pw_tpw(p->jit, stride + nfft)
                                      : gdsp::pwelch_fixed_workers_per_block(pmd, stride + nfft);
  if (wpb_fixed > 0 && !(gdsp::algo_flags() & GDSP_ALGO_GENERIC_MIXED)) {
    // fused path on a compiled specialisation (e.g. NFFT 1000, 3000)
    STCHK(workers(wmul * (int64_t)wpb_fixed));
    if (p->jit)
      HIPCHK(gdsp::jit_launch_pwelch(p->jit, d_x, nfft, stride, seg_begin, seg_end, ppw, nworkers,
                                     d_win_seg, p->tw, pt.p(), s));
    else
      HIPCHK(gdsp::launch_pwelch_fixed(pmd, d_x, nfft, stride, seg_begin, seg_end, ppw, nworkers,
                                       d_win_seg, own ? p->tw_pw : p->tw, pt.p(), s));
    return pt.reduce(nworkers, flen, d_acc, s);
  }
  if (fused && p->kind == KIND_MIXED && p->md_gen.npass >= 2) {
    // fused mixed-radix path (smooth NFFT / Pad up to 4096)
    STCHK(workers(wmul));
    HIPCHK(gdsp::launch_pwelch_mixed(p->md_gen, d_x, nfft, stride, seg_begin, seg_end, ppw,
                                     nworkers, d_win_seg, p->tw_gen, pt.p(), s));
    return pt.reduce(nworkers, flen, d_acc, s);
  }
  // materialised path (lengths without a fused kernel): packed segment pairs
  // as complex rows, the batched FFT of the plan, per-bin partial power sums,
  // deterministic reduction into acc
  int64_t rows = ((int64_t)1 << 25) / flen;  // 512 MiB of rows per chunk
  constexpr int64_t kRpp = 64;
  if (rows < 1) rows = 1;
  if (rows > 65535 * kRpp) rows = 65535 * kRpp;  // partial-sum grid limit
  if (rows > npairs) rows = npairs;
  DevBuf buf;
  STCHK(buf.alloc((size_t)rows * (size_t)flen * sizeof(cd), s, SLOT_PW_BUF));
  STCHK(pt.alloc((rows + kRpp - 1) / kRpp, flen, s));
  for (int64_t r0 = 0; r0 < npairs; r0 += rows) {
    later_chunk(r0);
    const int64_t nr = (npairs - r0) < rows ? (npairs - r0) : rows;
    HIPCHK(gdsp::launch_segments_to_complex(d_x, nfft, flen, stride, seg_begin + 2 * r0, seg_end,
                                            nr, d_win_seg, (cd *)buf.p, s));
    STCHK(exec_plan(p, buf.p, (cd *)buf.p, nr, false, gdsp::LOAD_COMPLEX, s));
    HIPCHK(gdsp::launch_power_partials((const cd *)buf.p, nr, flen, kRpp, pt.p(), s));
    STCHK(pt.reduce((nr + kRpp - 1) / kRpp, flen, d_acc, s));
  }
  return GDSP_OK;
}

int gdsp_pwelch_finalize(const double *acc, int64_t flen, int64_t nsegs, int64_t nfft,
                         int64_t pad, const double *win_nfft, double fs, int scale_off,
                         double *pxx, double *freqs) {
  // spectral/pwelch.go:113-142
  if (flen <= 0 || nfft <= 0 || pad <= 0 || !pxx || !freqs)
    return fail(GDSP_ERR_INVALID, "bad argument");
  const int64_t lp = pad / 2 + 1;
  const double norm = welch_norm(win_nfft, nfft, fs, scale_off);
  for (int64_t j = 0; j < lp; ++j) {
    double d = 0.0;
    if (nsegs > 0) {
      d = 0.5 * (acc[j] + acc[(flen - j) % flen]) / (double)nsegs;
      if (j > 0 && j < lp - 1) d *= 2;
    }
    pxx[j] = d / norm;
  }
  welch_freqs(pad, fs, freqs);
  return GDSP_OK;
}

int gdsp_pwelch(const double *x, int64_t n, double fs, int64_t nfft, int64_t pad,
                int64_t noverlap, const double *win_seg, const double *win_nfft, int scale_off,
                double *pxx, double *freqs, int64_t *lp_out) {
  // spectral/pwelch.go:74-145
  if (!lp_out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  *lp_out = 0;
  if (n < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (n == 0) return GDSP_OK;
  if (!welch_defaults(&nfft, &pad)) return fail(GDSP_ERR_INVALID, "negative NFFT/Pad");
  WelchShape w;
  STCHK(welch_shape(n, nfft, pad, noverlap, &w));
  std::vector<double> hseg;
  win_seg = hann_or(win_seg, w.flen, hseg);
  if (w.nsegs >= 2 && multi_wanted((size_t)n * sizeof(double), w.nsegs))
    return pwelch_multi(x, n, fs, nfft, pad, noverlap, win_seg, win_nfft, scale_off, pxx, freqs,
                        lp_out, nullptr, 0);
  std::vector<double> acc((size_t)w.flen, 0.0);
  if (w.nsegs > 0) {
    int dev = 0;
    STCHK(current_device(&dev));
    hipStream_t s = thread_stream(dev);
    if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
    const size_t fbytes = (size_t)w.flen * sizeof(double);
    DevBuf dx, dw, dacc;
    STCHK(dx.alloc((size_t)w.lx * sizeof(double), s, SLOT_IN));
    STCHK(dw.alloc(fbytes, s, SLOT_AUX));
    STCHK(dacc.alloc(fbytes, s, SLOT_AUX2));
    STCHK(run_queued(s, [&]() -> int {
      STCHK(stage_rows((double *)dx.p, x, 1, n, n, w.lx, s));
      STCHK(copy_h2d(dw.p, win_seg, fbytes, s));
      HIPCHK(hipMemsetAsync(dacc.p, 0, fbytes, s));
      return gdsp_pwelch_accumulate_device((const double *)dx.p, w.lx, nfft, pad, noverlap, 0,
                                           w.nsegs, (const double *)dw.p, (double *)dacc.p, s);
    }));
    STCHK(copy_d2h(acc.data(), dacc.p, fbytes, s));
  }
  STCHK(gdsp_pwelch_finalize(acc.data(), w.flen, w.nsegs, nfft, pad, win_nfft, fs, scale_off, pxx,
                             freqs));
  *lp_out = w.lp;
  return GDSP_OK;
}

// ---- batched Pwelch: the channels of a planar batch in one call ---------------

int gdsp_pwelch_batch_fused(int64_t channels, int64_t n, int64_t nfft, int64_t pad,
                            int64_t noverlap) {
  return fused_answer(pwelch_batch_fused, channels, n, nfft, pad, noverlap);
}

int gdsp_pwelch_batch_accumulate_device(const double *d_x, int64_t channels, int64_t n,
                                        int64_t ldx, int64_t nfft, int64_t pad, int64_t noverlap,
                                        int64_t seg_begin, int64_t seg_end,
                                        const double *d_win_seg, double *d_acc, void *stream) {
  if (nfft <= 0 || pad <= 0 || seg_begin < 0 || seg_end < seg_begin)
    return fail(GDSP_ERR_INVALID, "bad Pwelch geometry");
  if (channels < 0 || n < 0 || (channels > 1 && ldx < n))
    return fail(GDSP_ERR_INVALID, "bad batch geometry");
  if (channels == 0 || seg_end == seg_begin) return GDSP_OK;
  if (!d_x || !d_win_seg || !d_acc) return fail(GDSP_ERR_INVALID, "NULL pointer");
  const int64_t stride = nfft - noverlap;
  if ((seg_end - 1) * stride + nfft > n)
    return fail(GDSP_ERR_INVALID, "segments exceed the signal");
  const int64_t flen = pad > nfft ? pad : nfft;
  hipStream_t s = (hipStream_t)stream;
  gdsp_plan *p = nullptr;
  if (pwelch_batch_fused(flen, stride)) STCHK(get_plan(flen, &p));
  if (!p || p->kind != KIND_LDS) {
    for (int64_t c = 0; c < channels; ++c) {
      later_chunk(c);
      STCHK(gdsp_pwelch_accumulate_device(d_x + c * ldx, n, nfft, pad, noverlap, seg_begin,
                                          seg_end, d_win_seg, d_acc + c * flen, stream));
    }
    return GDSP_OK;
  }
  const bool half = 2 * noverlap == nfft && flen == nfft;
  int64_t wpc = 0, gpw = 0, rows = 0;
  gdsp::pwelch_batch_geometry(p->log2n, half, channels, seg_end - seg_begin, &wpc, &gpw, &rows);
  const int64_t cpl = channels_per_launch(rows * flen, channels);
  Partials pt;
  STCHK(pt.alloc_batch(cpl, rows, flen, s));
  for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
    const int64_t nc = channels - c0 < cpl ? channels - c0 : cpl;
    later_chunk(c0);
    multi_unit(gpw);
    HIPCHK(gdsp::launch_pwelch_batch(p->log2n, half, d_x + c0 * ldx, ldx, nc, wpc, nfft, stride,
                                     seg_begin, seg_end, gpw, d_win_seg, p->tw, pt.p(), s));
    STCHK(pt.reduce_batch(nc, rows, flen, d_acc + c0 * flen, s));
  }
  return GDSP_OK;
}

int gdsp_pwelch_batch_finalize_device(const double *d_acc, int64_t channels, int64_t flen,
                                      int64_t nsegs, int64_t nfft, int64_t pad,
                                      const double *win_nfft, double fs, int scale_off,
                                      double *d_pxx, double *freqs, void *stream) {
  if (channels < 0 || flen <= 0 || nfft <= 0 || pad <= 0 || nsegs < 0)
    return fail(GDSP_ERR_INVALID, "bad argument");
  if (channels > 0 && (!d_acc || !d_pxx)) return fail(GDSP_ERR_INVALID, "NULL pointer");
  const int64_t lp = pad / 2 + 1;
  if (lp > flen) return fail(GDSP_ERR_INVALID, "accumulators shorter than Pad / 2 + 1");
  const double norm = welch_norm(win_nfft, nfft, fs, scale_off);
  if (freqs) welch_freqs(pad, fs, freqs);
  if (channels == 0) return GDSP_OK;
  HIPCHK(gdsp::launch_pwelch_finalize(d_acc, channels, flen, lp, nsegs, norm, d_pxx,
                                      (hipStream_t)stream));
  return GDSP_OK;
}

int gdsp_pwelch_batch(const double *x, int64_t channels, int64_t n, int64_t ldx, double fs,
                      int64_t nfft, int64_t pad, int64_t noverlap, const double *win_seg,
                      const double *win_nfft, int scale_off, double *pxx, double *freqs,
                      int64_t *lp_out) {
  if (!lp_out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  *lp_out = 0;
  if (channels < 0 || n < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (n == 0) return GDSP_OK;
  if (!welch_defaults(&nfft, &pad)) return fail(GDSP_ERR_INVALID, "negative NFFT/Pad");
  if (channels > 1 && ldx < n) return fail(GDSP_ERR_INVALID, "ldx below the channel length");
  WelchShape w;
  STCHK(welch_shape(n, nfft, pad, noverlap, &w));
  if (!freqs || (channels > 0 && (!x || !pxx))) return fail(GDSP_ERR_INVALID, "NULL pointer");
  if (channels == 0) {
    welch_freqs(pad, fs, freqs);
    *lp_out = w.lp;
    return GDSP_OK;
  }
  std::vector<double> hseg, hnfft;
  win_seg = hann_or(win_seg, w.flen, hseg);
  win_nfft = hann_or(win_nfft, nfft, hnfft);  // once for every channel's finalisation
  std::vector<double> acc((size_t)channels * (size_t)w.flen, 0.0);
  if (w.nsegs > 0) {
    int dev = 0;
    STCHK(current_device(&dev));
    hipStream_t s = thread_stream(dev);
    if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
    const size_t abytes = acc.size() * sizeof(double);
    DevBuf dx, dw, dacc;
    STCHK(dx.alloc((size_t)channels * (size_t)w.lx * sizeof(double), s, SLOT_IN));
    STCHK(dw.alloc((size_t)w.flen * sizeof(double), s, SLOT_AUX));
    STCHK(dacc.alloc(abytes, s, SLOT_AUX2));
    STCHK(run_queued(s, [&]() -> int {
      STCHK(stage_rows((double *)dx.p, x, channels, n, ldx, w.lx, s));
      STCHK(copy_h2d(dw.p, win_seg, (size_t)w.flen * sizeof(double), s));
      HIPCHK(hipMemsetAsync(dacc.p, 0, abytes, s));
      return gdsp_pwelch_batch_accumulate_device((const double *)dx.p, channels, w.lx, w.lx, nfft,
                                                 pad, noverlap, 0, w.nsegs, (const double *)dw.p,
                                                 (double *)dacc.p, s);
    }));
    STCHK(copy_d2h(acc.data(), dacc.p, abytes, s));
  }
  for (int64_t c = 0; c < channels; ++c)
    STCHK(gdsp_pwelch_finalize(acc.data() + c * w.flen, w.flen, w.nsegs, nfft, pad, win_nfft, fs,
                               scale_off, pxx + c * w.lp, freqs));
  *lp_out = w.lp;
  return GDSP_OK;
}

// ---- batched cross spectra: Cpsd and coherence of x channels against y --------

int gdsp_cpsd_batch_fused(int64_t channels, int64_t n, int64_t nfft, int64_t pad,
                          int64_t noverlap) {
  return fused_answer(cpsd_batch_fused, channels, n, nfft, pad, noverlap);
}

int gdsp_cpsd_batch_accumulate_device(const double *d_x, int64_t ldx, const double *d_y,
                                      int64_t ldy, int64_t y_rows, int64_t channels, int64_t n,
                                      int64_t nfft, int64_t pad, int64_t noverlap,
                                      int64_t seg_begin, int64_t seg_end,
                                      const double *d_win_seg, double *d_acc, void *stream) {
  if (nfft <= 0 || pad <= 0 || seg_begin < 0 || seg_end < seg_begin)
    return fail(GDSP_ERR_INVALID, "bad Cpsd geometry");
  if (channels < 0 || n < 0 || y_rows < 0 || (channels > 1 && ldx < n) || (y_rows > 1 && ldy < n))
    return fail(GDSP_ERR_INVALID, "bad batch geometry");
  if (y_rows != 1 && y_rows != channels)
    return fail(GDSP_ERR_UNEQUAL, "y is neither one row nor a row per channel");
  const int64_t stride = nfft - noverlap;
  // Segment divides by the stride only where there is more than one segment
  if (stride == 0 && seg_end > 1) return fail(GDSP_ERR_DIVIDE_BY_ZERO, "integer divide by zero");
  if (channels == 0 || seg_end == seg_begin) return GDSP_OK;
  if (!d_x || !d_y || !d_win_seg || !d_acc) return fail(GDSP_ERR_INVALID, "NULL pointer");
  // a negative stride (Noverlap > NFFT) leaves at most segment 0 (Segment)
  if ((seg_end - 1) * stride + nfft > n || (stride < 0 && seg_end > 1))
    return fail(GDSP_ERR_INVALID, "segments exceed the signal");
  const int64_t flen = pad > nfft ? pad : nfft;
  const int64_t hb = flen / 2 + 1, nseg = seg_end - seg_begin;
  const int64_t ldyk = y_rows == 1 ? 0 : ldy;  // the kernels' y row stride
  hipStream_t s = (hipStream_t)stream;
  gdsp_plan *p = nullptr;
  STCHK(get_plan(flen, &p));
  Partials pt;
  // get_plan builds a power of 2 up to 2^14 as KIND_LDS under every flag set
  // (build_plan, plan.hip), so gdsp_cpsd_batch_fused's answer holds here; the
  // kind is checked because the kernel reads that plan's twiddle table
  if (cpsd_batch_fused(flen, stride) && p->kind == KIND_LDS) {
    int64_t wpc = 0, gpw = 0, rows = 0;
    gdsp::cpsd_batch_geometry(p->log2n, channels, nseg, &wpc, &gpw, &rows);
    const int64_t cpl = channels_per_launch(rows * 4 * hb, channels);
    STCHK(pt.alloc_batch(cpl, rows, 4 * hb, s));
    for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
      const int64_t nc = channels - c0 < cpl ? channels - c0 : cpl;
      later_chunk(c0);
      multi_unit(gpw);
      HIPCHK(gdsp::launch_cpsd_batch(p->log2n, d_x + c0 * ldx, ldx, d_y + c0 * ldyk, ldyk, nc, wpc,
                                     nfft, stride, seg_begin, seg_end, gpw, d_win_seg, p->tw,
                                     pt.p(), s));
      STCHK(pt.reduce_batch(nc, rows, 4 * hb, d_acc + c0 * 4 * hb, s));
    }
    return GDSP_OK;
  }
  // materialised form: chunks of at most 512 MiB of complex rows, whole
  // channels where a channel's segments fit, else one channel's segments in
  // runs; parts of kRpp rows, reduced in the fixed order
  constexpr int64_t kRpp = 64;
  int64_t maxrows = ((int64_t)1 << 25) / flen;
  if (maxrows < 1) maxrows = 1;
  const int64_t ns_max = nseg < maxrows ? nseg : maxrows;  // segments per run
  int64_t cpl = maxrows / ns_max;                           // channels per launch
  if (cpl > channels) cpl = channels;
  DevBuf buf, bal;
  STCHK(buf.alloc((size_t)cpl * (size_t)ns_max * (size_t)flen * sizeof(cd), s, SLOT_PW_BUF));
  STCHK(bal.alloc((size_t)cpl * (size_t)ns_max * sizeof(double), s, SLOT_CP_BAL));
  double *alpha = (double *)bal.p;  // a power of 2 per row (cpsd_batch.hip, Balance)
  STCHK(pt.alloc_batch(cpl, (ns_max + kRpp - 1) / kRpp, 4 * hb, s));
  for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
    const int64_t nc = channels - c0 < cpl ? channels - c0 : cpl;
    later_chunk(c0);
    for (int64_t j0 = 0; j0 < nseg; j0 += ns_max) {
      const int64_t ns = nseg - j0 < ns_max ? nseg - j0 : ns_max;
      later_chunk(j0);
      HIPCHK(gdsp::launch_cpsd_balance(d_x + c0 * ldx, ldx, d_y + c0 * ldyk, ldyk, nc, ns, nfft,
                                       stride, seg_begin + j0, d_win_seg, alpha, s));
      HIPCHK(gdsp::launch_cpsd_gather(d_x + c0 * ldx, ldx, d_y + c0 * ldyk, ldyk, nc, ns, nfft,
                                      flen, stride, seg_begin + j0, d_win_seg, alpha,
                                      (cd *)buf.p, s));
      STCHK(exec_plan(p, buf.p, (cd *)buf.p, nc * ns, false, gdsp::LOAD_COMPLEX, s));
      HIPCHK(gdsp::launch_cpsd_partials((const cd *)buf.p, nc, ns, flen, kRpp, alpha, pt.p(), s));
      STCHK(pt.reduce_batch(nc, (ns + kRpp - 1) / kRpp, 4 * hb, d_acc + c0 * 4 * hb, s));
    }
  }
  return GDSP_OK;
}

int gdsp_cpsd_batch_finalize_device(const double *d_acc, int64_t channels, int64_t flen,
                                    int64_t nsegs, int64_t nfft, int64_t pad,
                                    const double *win_nfft, double fs, int scale_off,
                                    void *d_pxy, double *d_pxx, double *d_pyy, double *d_coh,
                                    double *freqs, void *stream) {
  if (channels < 0 || flen <= 0 || nfft <= 0 || pad <= 0 || nsegs < 0)
    return fail(GDSP_ERR_INVALID, "bad argument");
  if (channels > 0 && !d_acc) return fail(GDSP_ERR_INVALID, "NULL pointer");
  const int64_t lp = pad / 2 + 1, hb = flen / 2 + 1;
  if (lp > hb) return fail(GDSP_ERR_INVALID, "accumulators shorter than Pad / 2 + 1");
  const double norm = welch_norm(win_nfft, nfft, fs, scale_off);
  if (freqs) welch_freqs(pad, fs, freqs);
  if (channels == 0 || (!d_pxy && !d_pxx && !d_pyy && !d_coh)) return GDSP_OK;
  HIPCHK(gdsp::launch_cpsd_finalize(d_acc, channels, hb, lp, nsegs, norm, (cd *)d_pxy, d_pxx,
                                    d_pyy, d_coh, (hipStream_t)stream));
  return GDSP_OK;
}

int gdsp_cpsd_batch(const double *x, int64_t ldx, const double *y, int64_t ldy, int64_t y_rows,
                    int64_t channels, int64_t n, double fs, int64_t nfft, int64_t pad,
                    int64_t noverlap, const double *win_seg, const double *win_nfft,
                    int scale_off, double *pxy, double *pxx, double *pyy, double *coh,
                    double *freqs, int64_t *lp_out) {
  if (!lp_out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  *lp_out = 0;
  if (channels < 0 || n < 0 || y_rows < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (n == 0) return GDSP_OK;
  if (y_rows != 1 && y_rows != channels)
    return fail(GDSP_ERR_UNEQUAL, "y is neither one row nor a row per channel");
  if (!welch_defaults(&nfft, &pad)) return fail(GDSP_ERR_INVALID, "negative NFFT/Pad");
  if ((channels > 1 && ldx < n) || (y_rows > 1 && ldy < n))
    return fail(GDSP_ERR_INVALID, "row stride below the channel length");
  WelchShape w;
  STCHK(welch_shape(n, nfft, pad, noverlap, &w));
  if (!freqs || (channels > 0 && (!x || !y || !pxy))) return fail(GDSP_ERR_INVALID, "NULL pointer");
  const int64_t lx = w.lx, lp = w.lp, hb = w.flen / 2 + 1;
  if (channels == 0) {
    welch_freqs(pad, fs, freqs);
    *lp_out = lp;
    return GDSP_OK;
  }
  std::vector<double> hseg;
  win_seg = hann_or(win_seg, w.flen, hseg);
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const size_t rowb = (size_t)lx * sizeof(double);
  const size_t abytes = (size_t)channels * (size_t)(4 * hb) * sizeof(double);
  const size_t cl = (size_t)channels * (size_t)lp;
  // outputs in one buffer: pxy (2 cl doubles), then pxx, pyy, coh where asked
  double *const outs[3] = {pxx, pyy, coh};
  size_t ndbl = 2 * cl;
  for (double *o : outs) ndbl += o ? cl : 0;
  DevBuf dx, dy, dw, dacc, dout;
  STCHK(dx.alloc((size_t)channels * rowb, s, SLOT_IN));
  STCHK(dy.alloc((size_t)y_rows * rowb, s, SLOT_CP_Y));
  STCHK(dw.alloc((size_t)w.flen * sizeof(double), s, SLOT_AUX));
  STCHK(dacc.alloc(abytes, s, SLOT_AUX2));
  STCHK(dout.alloc(ndbl * sizeof(double), s, SLOT_CP_OUT));
  double *px = (double *)dx.p, *py = (double *)dy.p, *po = (double *)dout.p;
  double *dev_out[3] = {nullptr, nullptr, nullptr};
  size_t off = 2 * cl;
  for (int i = 0; i < 3; ++i)
    if (outs[i]) {
      dev_out[i] = po + off;
      off += cl;
    }
  STCHK(run_queued(s, [&]() -> int {
    STCHK(stage_rows(px, x, channels, n, ldx, lx, s));
    STCHK(stage_rows(py, y, y_rows, n, ldy, lx, s));
    STCHK(copy_h2d(dw.p, win_seg, (size_t)w.flen * sizeof(double), s));
    HIPCHK(hipMemsetAsync(dacc.p, 0, abytes, s));
    STCHK(gdsp_cpsd_batch_accumulate_device(px, lx, py, lx, y_rows, channels, lx, nfft, pad,
                                            noverlap, 0, w.nsegs, (const double *)dw.p,
                                            (double *)dacc.p, s));
    return gdsp_cpsd_batch_finalize_device((const double *)dacc.p, channels, w.flen, w.nsegs, nfft,
                                           pad, win_nfft, fs, scale_off, po, dev_out[0],
                                           dev_out[1], dev_out[2], freqs, s);
  }));
  STCHK(copy_d2h(pxy, po, 2 * cl * sizeof(double), s));
  for (int i = 0; i < 3; ++i)
    if (outs[i]) STCHK(copy_d2h(outs[i], dev_out[i], cl * sizeof(double), s));
  *lp_out = lp;
  return GDSP_OK;
}

// ---- per-segment spectra: STFT and spectrogram --------------------------------

int gdsp_stft_batch_fused(int64_t channels, int64_t n, int64_t nfft, int64_t pad,
                          int64_t noverlap) {
  return fused_answer(stft_batch_fused, channels, n, nfft, pad, noverlap);
}

int gdsp_stft_batch_device(const double *d_x, int64_t ldx, int64_t channels, int64_t n,
                           int64_t nfft, int64_t pad, int64_t noverlap, int64_t seg_begin,
                           int64_t seg_end, const double *d_win_seg, void *d_out, int64_t ld_seg,
                           int64_t ld_chan, void *stream) {
  return stft_device(false, d_x, ldx, channels, n, nfft, pad, noverlap, seg_begin, seg_end,
                     d_win_seg, 1.0, d_out, ld_seg, ld_chan, stream);
}

int gdsp_spectrogram_batch_device(const double *d_x, int64_t ldx, int64_t channels, int64_t n,
                                  int64_t nfft, int64_t pad, int64_t noverlap, int64_t seg_begin,
                                  int64_t seg_end, const double *d_win_seg, double norm,
                                  double *d_out, int64_t ld_seg, int64_t ld_chan, void *stream) {
  return stft_device(true, d_x, ldx, channels, n, nfft, pad, noverlap, seg_begin, seg_end,
                     d_win_seg, norm, d_out, ld_seg, ld_chan, stream);
}

int gdsp_stft_batch(const double *x, int64_t channels, int64_t n, int64_t ldx, int64_t nfft,
                    int64_t pad, int64_t noverlap, const double *win_seg, double *out,
                    int64_t *nsegs_out, int64_t *lp_out) {
  return stft_host(false, x, channels, n, ldx, 1.0, nfft, pad, noverlap, win_seg, nullptr, 1, out,
                   nullptr, nullptr, nsegs_out, lp_out);
}

int gdsp_spectrogram_batch(const double *x, int64_t channels, int64_t n, int64_t ldx, double fs,
                           int64_t nfft, int64_t pad, int64_t noverlap, const double *win_seg,
                           const double *win_nfft, int scale_off, double *out, double *freqs,
                           double *times, int64_t *nsegs_out, int64_t *lp_out) {
  return stft_host(true, x, channels, n, ldx, fs, nfft, pad, noverlap, win_seg, win_nfft,
                   scale_off, out, freqs, times, nsegs_out, lp_out);
}

// ---- the overlap-add inverse of the STFT rows ----------------------------------

int gdsp_istft_batch_fused(int64_t channels, int64_t nsegs, int64_t nfft, int64_t pad,
                           int64_t noverlap) {
  if (channels < 0 || nsegs < 0 || !welch_defaults(&nfft, &pad)) return 0;
  return istft_batch_fused(nfft, pad, nfft - noverlap) ? 1 : 0;
}

int gdsp_istft_batch_device(const void *d_X, int64_t ld_seg, int64_t ld_chan, int64_t channels,
                            int64_t nsegs, int64_t seg_row0, int64_t seg_rows, int64_t nfft,
                            int64_t pad, int64_t noverlap, const double *d_win_seg,
                            int64_t out_begin, int64_t out_end, double *d_out, int64_t ldo,
                            void *stream) {
  return istft_device(d_X, ld_seg, ld_chan, channels, nsegs, seg_row0, seg_rows, nfft, pad,
                      noverlap, d_win_seg, out_begin, out_end, d_out, ldo, stream);
}

int gdsp_istft_batch(const void *X, int64_t channels, int64_t nsegs, int64_t nfft, int64_t pad,
                     int64_t noverlap, const double *win_seg, int64_t n, double *out, int64_t ldo,
                     int64_t *n_out) {
  return istft_host(X, channels, nsegs, nfft, pad, noverlap, win_seg, n, out, ldo, n_out);
}

}  // extern "C"
