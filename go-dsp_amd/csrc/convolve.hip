// convolve.hip — batched circular convolution (fft.Convolve per row,
// fft/fft.go:55-69: IFFT(FFT(x) * FFT(y))) of rows of one length against one
// y or one y per row.
//
//   convolve_lds_kernel       power-of-2 n, 256 ... 16384: load, FFT_n, times
//                             FFT_n(y) / n, second FFT_n, store, in one
//                             workgroup — one HBM read and one HBM write per
//                             row where FFT, multiply, IFFT make three of each
//   pointwise_mul_rows_kernel the multiply of that composed chain (every other
//                             length), second operand broadcast or per row
//
// The fused kernel is the chirp-z kernel (fft_kernels.hip bluestein_kernel)
// without its chirps: no premultiply, no zero padding, every output kept.
#include "conv_core.hpp"  // YhatEpi, conv_prew, conv_log2e: shared with fir.hip
#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

// One workgroup holds TPW whole rows in registers (thread t of a row owns
// elements t + k T). A row is complete in registers before its first store,
// so out may alias x; yspec (FFT_n(y), one row or one per row) is read between
// the two FFTs and must not. The inverse's 1/n (scale) goes on the outputs as
// they are stored: a power of 2, so the results are those of a table of
// FFT_n(y) / n bit for bit, without the pass over the table that scaling it
// would cost a call with one y per row.
template <int LOG2N, bool SPLIT, int LOG2E>
__global__ __launch_bounds__((Geo<LOG2N, LOG2E>::WG)) void convolve_lds_kernel(
    const cd *x, cd *out, int64_t batch, const cd *__restrict__ tw, const cd *__restrict__ yspec,
    int64_t yspec_stride, double scale) {
  using G = Geo<LOG2N, LOG2E>;
  static_assert(G::T >= 16, "rows of fewer than 16 threads need LDS staging to stay coalesced");
  __shared__ double lds[(SPLIT ? 1 : 2) * G::LDS_DOUBLES];
  const int lt = threadIdx.x;
  const int slot = lt / G::T;
  const int t = lt & (G::T - 1);
  const int64_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t g = blk * G::TPW + slot;
  // Only the last workgroup can hold slots past the batch (TPW > 1): they
  // load a valid row (clamped) and skip the store, so the whole workgroup
  // reaches every barrier.
  const bool valid = G::TPW == 1 || g < batch;
  const int64_t gl = G::TPW == 1 ? g : (g < batch ? g : batch - 1);
  double *lre = lds + slot * G::STRIDE;
  double *lim = SPLIT ? lre : lds + G::LDS_DOUBLES + slot * G::STRIDE;
  const cd *src = x + gl * G::N;
  cd v[G::E];
#pragma unroll
  for (int k = 0; k < G::E; ++k) v[k] = ld_nt(&src[t + k * G::T]);
  const YhatEpi<G::T> ye{yspec + gl * yspec_stride + t};
  fft_regs<LOG2N, SPLIT, 1, LOG2E, 0, 0, const cd *, 1, 0, YhatEpi<G::T>, conv_prew(LOG2N)>(
      v, t, tw, lre, lim, true, ye);
  fft_regs<LOG2N, SPLIT, 1, LOG2E, 0, 0, const cd *, 1, 0, NoEpi, conv_prew(LOG2N)>(
      v, t, tw, lre, lim, false);
  if (valid) {
    cd *dst = out + g * G::N;
    const int to = opaque_int(t);
#pragma unroll
    for (int k = 0; k < G::E; ++k)
      st_nt(&dst[to + k * G::T], cd{v[k].x * scale, -v[k].y * scale});
  }
}

template <int LOG2N>
static hipError_t launch_conv_t(const cd *x, cd *out, int64_t batch, const cd *tw,
                                const cd *yspec, int64_t yspec_stride, hipStream_t s) {
  constexpr int LOG2E = conv_log2e(LOG2N);
  using G = Geo<LOG2N, LOG2E>;
  const int64_t nblk = (batch + G::TPW - 1) / G::TPW;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((convolve_lds_kernel<LOG2N, true, LOG2E>), dim3((unsigned)nblk),
                     dim3(G::WG), 0, s, x, out, batch, tw, yspec, yspec_stride,
                     1.0 / (double)G::N);
  return hipGetLastError();
}

hipError_t launch_convolve_lds(int log2n, const cd *x, cd *out, int64_t batch, const cd *tw,
                               const cd *yspec, int64_t yspec_stride, hipStream_t s) {
  if (batch <= 0 || !x || !out || !tw || !yspec ||
      (yspec_stride != 0 && yspec_stride != ((int64_t)1 << log2n)))
    return hipErrorInvalidValue;
  static_assert(kConvMinLog2 == 8 && kMaxLdsLog2 == 14, "the cases below");
  switch (log2n) {
    case 8: return launch_conv_t<8>(x, out, batch, tw, yspec, yspec_stride, s);
    case 9: return launch_conv_t<9>(x, out, batch, tw, yspec, yspec_stride, s);
    case 10: return launch_conv_t<10>(x, out, batch, tw, yspec, yspec_stride, s);
    case 11: return launch_conv_t<11>(x, out, batch, tw, yspec, yspec_stride, s);
    case 12: return launch_conv_t<12>(x, out, batch, tw, yspec, yspec_stride, s);
    case 13: return launch_conv_t<13>(x, out, batch, tw, yspec, yspec_stride, s);
    case 14: return launch_conv_t<14>(x, out, batch, tw, yspec, yspec_stride, s);
    default: return hipErrorInvalidValue;
  }
}

// out[g n + k] = a[g n + k] * b[g b_stride + k]: the composed chain's multiply
__global__ void pointwise_mul_rows_kernel(const cd *a, const cd *__restrict__ b, int64_t b_stride,
                                          cd *out, int64_t n, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t g = i / n;
  out[i] = cmul(a[i], b[g * b_stride + (i - g * n)]);
}

hipError_t launch_pointwise_mul_rows(const cd *a, const cd *b, int64_t b_stride, cd *out,
                                     int64_t n, int64_t batch, hipStream_t s) {
  if (n <= 0 || batch <= 0 || (b_stride != 0 && b_stride != n)) return hipErrorInvalidValue;
  const int64_t count = n * batch, nblk = (count + 255) / 256;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pointwise_mul_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, s, a, b,
                     b_stride, out, n, count);
  return hipGetLastError();
}

}  // namespace gdsp
