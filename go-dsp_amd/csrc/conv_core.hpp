// conv_core.hpp — what the kernels that run FFT_n, times a spectrum, inverse
// FFT_n inside one workgroup share: the circular convolution (convolve.hip)
// and the overlap-save FIR filter (fir.hip).
#pragma once
#include "fft_device.hpp"

namespace gdsp {

// Epilogue of the first FFT's last pass (fft_regs EPI): v = conj(X * yhat),
// the factor loaded ahead of its butterfly's arithmetic. The conjugate turns
// the second forward FFT into the inverse: IFFT(Z) = conj(FFT(conj(Z))) / n.
template <int T>
struct YhatEpi {
  const cd *m;  // the row's FFT(y) + t
  static constexpr bool on = true;
  __device__ static constexpr bool want(int) { return true; }
  __device__ cd load(int k) const { return m[k * T]; }
  template <int E>
  __device__ void apply(cd (&v)[E], int k, cd u, cd f) const { v[k] = conjg(cmul(u, f)); }
};

// Twiddle-base prefetch (fft_regs PREW) as the chirp-z kernel settled it per
// size: on, except at 2^10 where it cost that kernel a wave per SIMD
__host__ __device__ constexpr int conv_prew(int log2n) { return log2n == 10 ? 0 : 1; }
// Elements per thread as the chirp-z kernel's two-FFT body measured them: 32
// (three passes, two exchanges) at 8192 and 16384, 16 below
__host__ __device__ constexpr int conv_log2e(int log2n) { return log2n >= 13 ? 5 : 4; }

}  // namespace gdsp
