// api_internal.hpp — the host vocabulary the translation units of the C ABI
// share: gdsp_api.hip (streams, staging, workspaces, executors, the FFT,
// Convolve, FIR, resampling, Hilbert and recursive-filter entries), czt.hip (the chirp-z
// transform's tables, plan object and entries), dct.hip (the cosine transforms' table and
// entries), welch.hip (the Welch family: Pwelch, batched
// Pwelch, Cpsd, STFT, ISTFT), plan.hip (the planner) and multi.hip (the multi-device
// layer). Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "gdsp_fft.h"

namespace gdsp_api {

// ---- streams, staging and workspaces (gdsp_api.hip) --------------------------
// Record msg as the calling thread's gdsp_last_error and return st.
int fail(int st, const std::string &msg);
// The current device, or GDSP_ERR_NO_DEVICE.
int current_device(int *dev);
// One non-blocking stream per (thread, device) for the host-pointer API.
hipStream_t thread_stream(int dev);
// Host <-> device through the calling thread's pinned staging (current
// device), queued on s; copy_d2h returns after s drained.
int copy_h2d(void *dst, const void *src, size_t bytes, hipStream_t s);
int copy_d2h(void *dst, const void *src, size_t bytes, hipStream_t s);

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return gdsp_api::fail(GDSP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define STCHK(expr)               \
  do {                            \
    int s_ = (expr);              \
    if (s_ != GDSP_OK) return s_; \
  } while (0)

// Grow-only device scratch of the current device per (stream, use-site slot),
// ordered by the stream itself (the workspace map, gdsp_api.hip).
enum Slot {
  SLOT_IN = 0, SLOT_OUT, SLOT_AUX, SLOT_AUX2, SLOT_GLOBAL, SLOT_GLOBAL_IN, SLOT_REAL,
  SLOT_BLU, SLOT_FFT2, SLOT_PW_PART, SLOT_PW_RED, SLOT_PW_BUF, SLOT_FS0, SLOT_FS1, SLOT_FS2,
  SLOT_FS3, SLOT_FFTN, SLOT_MX0, SLOT_MX1, SLOT_PARTS, SLOT_CONV, SLOT_CP_Y, SLOT_CP_OUT, SLOT_CP_BAL,
  SLOT_FIR, SLOT_FIR_H, SLOT_FIR_OUT, SLOT_ST_ROWS, SLOT_ST_OUT, SLOT_IS_D,
  SLOT_UF, SLOT_UF_H, SLOT_UF_OUT, SLOT_HB, SLOT_HB_OUT,
  SLOT_SOS, SLOT_SOS_Z, SLOT_CZT, SLOT_CZT_OUT, SLOT_DCT, SLOT_DCT_OUT,
  SLOT_COUNT
};

struct DevBuf {
  void *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  int alloc(size_t bytes, hipStream_t st, Slot slot);
};

// `rows` host rows of n doubles, ld apart, as device rows of lx >= n doubles,
// zero-padded where lx > n (dsputils.ZeroPadF): one copy when dense, else one
// per row. And dense device rows of n back into host rows ld apart.
int stage_rows(double *d, const double *h, int64_t rows, int64_t n, int64_t ld, int64_t lx,
               hipStream_t s);
int unstage_rows(double *h, const double *d, int64_t rows, int64_t n, int64_t ld, hipStream_t s);

// queue() puts a host call's copies and kernels on s. Where it fails, s is
// drained before its status returns: queued copies still read the staging halves.
template <class F>
int run_queued(hipStream_t s, F &&queue) {
  const int st = queue();
  if (st != GDSP_OK) (void)hipStreamSynchronize(s);
  return st;
}

// Counters of gdsp_loop_stats. A host chunk loop calls later_chunk(i0) in
// every iteration: the second and later ones (i0 > 0) count. multi_unit(u)
// stands before a launch of a Pwelch, batched-Pwelch, Cpsd, STFT or ISTFT kernel
// whose workers take u pairs or groups each: u >= 2 counts.
void later_chunk(int64_t i0);
void multi_unit(int64_t units);

// Host-pointer batched transform on the calling thread's current device.
int host_batch(const void *x, size_t in_elem_bytes, double *out, int64_t n, int64_t batch,
               bool inv, int load);

inline bool is_pow2(int64_t x) { return (x & (x - 1)) == 0; }

inline int ilog2(int64_t x) {
  int r = 0;
  while (x > 1) {
    x >>= 1;
    ++r;
  }
  return r;
}

// dsputils.NextPowerOf2 (dsputils/dsputils.go:39-45): float Log2/Ceil/Pow.
inline int64_t next_pow2_ref(int64_t x) {
  if (is_pow2(x)) return x;
  return (int64_t)pow(2.0, ceil(log2((double)x)));
}

// ---- the Welch family's host arithmetic (welch.hip) --------------------------
// window.Hann table (window/window.go:62-76) and spectral.Segment count
// (spectral/spectral.go:22-33).
void hann_table(int64_t L, double *out);
int segment_count(int64_t lx, int64_t size, int64_t noverlap, int64_t *count);
// w, or the Hann table of L built into store where no window is given.
const double *hann_or(const double *w, int64_t L, std::vector<double> &store);
// The defaults of spectral/pwelch.go:79-95 (NFFT 0 -> 256, Pad 0 -> NFFT);
// false: a negative NFFT or Pad.
bool welch_defaults(int64_t *nfft, int64_t *pad);
// The shape of a call after the defaults: the row length after
// dsputils.ZeroPadF(x, nfft), Segment's count of it, the transform length and
// Pad / 2 + 1. An entry's own checks stand between the two steps.
struct WelchShape {
  int64_t lx, nsegs, flen, lp;
};
int welch_shape(int64_t n, int64_t nfft, int64_t pad, int64_t noverlap, WelchShape *w);

// ---- the multi-device layer (multi.hip) --------------------------------------
// Whether a host-pointer call of `bytes` input over `units` independent units
// (rows or segments) is split over the library's device set; then the split
// itself.
bool multi_wanted(size_t bytes, int64_t units);
int fft_batch_multi(const void *x, size_t in_elem_bytes, double *out, int64_t n, int64_t batch,
                    bool inv, int load, const int *devices, int ndev);
int pwelch_multi(const double *x, int64_t n, double fs, int64_t nfft, int64_t pad,
                 int64_t noverlap, const double *win_seg, const double *win_nfft, int scale_off,
                 double *pxx, double *freqs, int64_t *lp_out, const int *devices, int ndev);

}  // namespace gdsp_api
