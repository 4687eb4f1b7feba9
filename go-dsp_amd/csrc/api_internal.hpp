// api_internal.hpp — what the multi-device layer (multi.hip) and the planner
// (plan.hip) use of the single-device host path in gdsp_api.hip. Not part of
// the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "gdsp_fft.h"

namespace gdsp_api {

// ---- shared by gdsp_api.hip and plan.hip ------------------------------------
// Record msg as the calling thread's gdsp_last_error and return st.
int fail(int st, const std::string &msg);
// The current device, or GDSP_ERR_NO_DEVICE.
int current_device(int *dev);
// One non-blocking stream per (thread, device) for the host-pointer API.
hipStream_t thread_stream(int dev);
// Host -> device through the calling thread's pinned staging, queued on s.
int copy_h2d(void *dst, const void *src, size_t bytes, hipStream_t s);

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

// ---- for the multi-device layer ---------------------------------------------

// Scratch slots the multi-device layer reuses (the Workspace slots of
// gdsp_api.hip, keyed by (device, stream)).
enum ScratchSlot { SCRATCH_SIGNAL = 0, SCRATCH_WINDOW = 1, SCRATCH_ACC = 2 };

// Record msg as the calling thread's gdsp_last_error and return st.
int set_error(int st, const std::string &msg);
// The calling thread's non-blocking stream on device dev (created once).
hipStream_t stream_for(int dev);
// Grow-only device scratch of the current device, ordered by stream s.
int scratch(size_t bytes, hipStream_t s, ScratchSlot slot, void **p);
// Host <-> device through the calling thread's pinned staging (current device).
int h2d(void *dst, const void *src, size_t bytes, hipStream_t s);
int d2h(void *dst, const void *src, size_t bytes, hipStream_t s);  // returns after s drained
// Host-pointer batched transform on the calling thread's current device.
int batch_on_current_device(const void *x, size_t in_elem_bytes, double *out, int64_t n,
                            int64_t batch, bool inv, int load);
// window.Hann table and spectral.Segment count (gdsp_api.hip).
void hann(int64_t L, double *out);
int segments(int64_t lx, int64_t size, int64_t noverlap, int64_t *count);

// Multi-device layer (multi.hip). Whether a host-pointer call of `bytes`
// input over `units` independent units (rows or segments) is split over the
// library's device set; then the split itself.
bool multi_wanted(size_t bytes, int64_t units);
int fft_batch_multi(const void *x, size_t in_elem_bytes, double *out, int64_t n, int64_t batch,
                    bool inv, int load, const int *devices, int ndev);
int pwelch_multi(const double *x, int64_t n, double fs, int64_t nfft, int64_t pad,
                 int64_t noverlap, const double *win_seg, const double *win_nfft, int scale_off,
                 double *pxx, double *freqs, int64_t *lp_out, const int *devices, int ndev);

}  // namespace gdsp_api
