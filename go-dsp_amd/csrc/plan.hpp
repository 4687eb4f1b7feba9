// plan.hpp — the FFT planner (plan.hip): what a plan holds, the plan cache's
// entry point, and what the planner uses of the executors in gdsp_api.hip.
#pragma once
#include <memory>
#include <utility>
#include <vector>

#include "api_internal.hpp"
#include "fft_device.hpp"
#include "launch.hpp"

// A device allocation with one owner: hipFree on destruction, move-only.
struct HipFree {
  void operator()(void *p) const { (void)hipFree(p); }
};
template <class T>
using DevPtr = std::unique_ptr<T, HipFree>;

enum PlanKind { KIND_TRIVIAL = 0, KIND_LDS = 1, KIND_GLOBAL = 2, KIND_BLUESTEIN = 3,
                KIND_BLUESTEIN_COMPOSED = 4, KIND_MIXED = 5, KIND_MIXED4 = 6, KIND_RADER = 7,
                KIND_RADER_PFA = 8 };

struct gdsp_plan {
  using cd = gdsp::cd;
  gdsp_plan() = default;
  gdsp_plan(gdsp_plan &&) = default;  // move-only: the tables have one owner
  gdsp_plan &operator=(gdsp_plan &&) = default;
  // The device tables the plan owns, freed with it; the executors read them
  // through the plain pointers below. Sub-plans (p1, p2, mplan: the plan
  // cache's) and runtime-compiled kernels (the JIT module list's) are not
  // owned. A cached plan is never deleted: nothing is freed at process exit.
  std::vector<DevPtr<void>> owned;
  template <class T>
  T *own(DevPtr<T> t) {
    T *r = t.get();
    owned.emplace_back(std::move(t));
    return r;
  }
  int device = 0;
  int64_t n = 0;
  int kind = KIND_TRIVIAL;
  int log2n = 0;
  cd *tw = nullptr;  // power of 2: T_n[k] = exp(-2 pi i k/n), n entries;
                     // mixed radix: the per-pass butterfly-major table
  gdsp::MixedDesc md{};
  gdsp::MixedDesc md_gen{};  // generic radix list (runtime-radix kernels)
  cd *tw_gen = nullptr;      // (tw itself where the lists are the same)
  // the fused Pwelch's own compiled list where it differs from md's
  // (pwelch_fixed_radices; md_pw.n = 0: none)
  gdsp::MixedDesc md_pw{};
  cd *tw_pw = nullptr;
  gdsp::JitSpec *jit = nullptr;  // runtime-compiled specialisation of md (mixed_jit.hip)
  // mixed four-step (KIND_MIXED4): n = n1 * n2, one-kernel sub-plans, tw = T_n;
  // pow2col: n1 is a power of 2 in [16, 512], so the column DFT runs on
  // row-segment tiles; radixcol: n1 <= 25 is one radix, a column per thread
  // (either way 3 HBM passes instead of 5)
  int64_t n1 = 0, n2 = 0;
  bool pow2col = false, radixcol = false;
  // rowst: n2 a power of 2 in [16, 1024] and n1 a radixcol / mixcol column:
  // two passes, the rows' store carrying the transpose (rowfft_t_kernel)
  bool rowst = false;
  gdsp::JitRowT *rowt = nullptr;  // rowst with n2 smooth, not a power of 2: the rows' kernel
  // mixcol: n1 in [26, 1016] smooth, its column pass runtime-compiled
  gdsp::JitCol *mixcol = nullptr;
  gdsp_plan *p1 = nullptr, *p2 = nullptr;
  // Bluestein (fft/bluestein.go): M = NextPowerOf2(2n-1), chirp = conj(w),
  // bhat = FFT_M(b)/M
  int64_t m = 0;
  int log2m = 0;
  gdsp_plan *mplan = nullptr;
  cd *chirp = nullptr;
  cd *bhat = nullptr;
  // output-split chirp-z (bluestein_kernel PARTS): n in (8192, 16384] whose
  // NextPowerOf2(2n-1) = 32768 exceeds one kernel runs as `parts` fused
  // convolutions of M = 16384, each giving kpart outputs; bhat holds parts * M
  int parts = 1;
  // fused chirp-z on M = 16 RB 16 (chirpz6k.hip: the smallest such M >= 2n - 1,
  // 129 <= n <= 3200, where bluestein.go:70 pads to NextPowerOf2(2n - 1));
  // tw6k: its pass twiddle bases
  bool c6k = false;
  cd *tw6k = nullptr;
  // composed chirp-z without its fused transposes (GDSP_ALGO_CHIRPZ_UNFUSED)
  bool unfused = false;
  int64_t kpart = 0;
  // Rader (KIND_RADER, a prime n whose n - 1 has a radix list): the kernel,
  // m = n - 1 (the cyclic convolution's length), tw its per-pass twiddle
  // bases, bhat = FFT_m(b)/m, gpow[q] = g^q mod n, ginv[r] = g^-r mod n
  gdsp::JitRader *rader = nullptr;
  int *gpow = nullptr, *ginv = nullptr;
  // fused chirp-z on a smooth convolution length (KIND_BLUESTEIN, m = L):
  // bluestein_fixed_kernel for n, tw_blu its per-pass twiddle bases
  gdsp::JitBlu *blufix = nullptr;
  cd *tw_blu = nullptr, *bhat_blu = nullptr;
  int64_t m_blu = 0;
  gdsp::MixedDesc md_blu{};
  // prime-factor Rader (KIND_RADER_PFA, n = n1 * n2, n2 a prime with a Rader
  // plan p2 whose tables the kernel reads, gcd(n1, n2) = 1): rader is
  // rader_pfa_kernel for the cofactor n1, m = n2 - 1
};

namespace gdsp_api {

// The cached plan for n on the current device under the algorithm flags in
// force (built on first use); chirpz: the forced Bluestein plan.
int get_plan(int64_t n, gdsp_plan **out, bool chirpz = false);
// The flags snapshot of the plan being built on this thread (gdsp::algo_flags
// returns it during the build); false outside a build.
bool build_flags(unsigned *flags);

// What the planner's tables are made with, for a plan object kept outside the
// cache (czt.hip): h as a complete device table; and FFT_len of each of the
// `count` rows of b times scale, computed on the device by the engine itself
// through the plan `fft` for len (the calling thread's stream is drained
// before either returns). Neither takes the plan mutex itself.
int device_table(int dev, const std::vector<gdsp::cd> &h, DevPtr<gdsp::cd> &out);
int plan_spectrum_table(int dev, const gdsp_plan *fft, const std::vector<gdsp::cd> &b,
                        int64_t len, int64_t count, double scale, DevPtr<gdsp::cd> &out);

// The executors (gdsp_api.hip) as the planner uses them: a plan's table of
// FFT_M(b) is computed by the engine itself, and a race times whole plans.
int exec_plan(const gdsp_plan *p, const void *in, gdsp::cd *out, int64_t batch, bool inv,
              int load, hipStream_t s);
// the power of 2 2^ln has the two-pass four-step (exec_fourstep2)
inline bool fourstep2_applies(int ln) { return ln >= 15 && ln <= 20; }

}  // namespace gdsp_api
