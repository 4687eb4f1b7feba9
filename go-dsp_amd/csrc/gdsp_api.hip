// gdsp_api.hip — the C ABI of libgdspfft (include/gdsp_fft.h): per-thread
// streams, staging and workspaces, the executors of a plan (plan.hip builds
// it), host-pointer entry points (what cgo binds) and device-pointer entry
// points (what the multi-GPU drivers call). The Welch family's entries
// (Pwelch, batched Pwelch, Cpsd) are in welch.hip; api_internal.hpp is what
// the two share.
//
// Every transform runs on the GPU. There is no CPU compute path: without a
// HIP device the entry points return GDSP_ERR_NO_DEVICE.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "fft_device.hpp"
#include "gdsp_fft.h"
#include "launch.hpp"
#include "api_internal.hpp"
#include "plan.hpp"

using gdsp::cd;
using namespace gdsp_api;

#define GDSP_VERSION "gdspfft 0.3.0 (gfx950)"

namespace {
thread_local std::string g_last_error;
int g_worker_pool_size = 0;  // fft.SetWorkerPoolSize mirror (no GPU meaning)
// loop counters for tests and diagnostics (gdsp_loop_stats)
std::atomic<int64_t> g_later_chunks{0}, g_multi_unit_launches{0};
}  // namespace

void gdsp_api::later_chunk(int64_t i0) {
  if (i0 > 0) g_later_chunks.fetch_add(1, std::memory_order_relaxed);
}

void gdsp_api::multi_unit(int64_t units) {
  if (units >= 2) g_multi_unit_launches.fetch_add(1, std::memory_order_relaxed);
}

int gdsp_api::fail(int st, const std::string &msg) {
  g_last_error = msg;
  return st;
}

int gdsp_api::current_device(int *dev) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(GDSP_ERR_NO_DEVICE, "no HIP device visible");
  if (hipGetDevice(dev) != hipSuccess) return fail(GDSP_ERR_NO_DEVICE, "hipGetDevice failed");
  return GDSP_OK;
}

// One non-blocking stream per (thread, device) for the host-pointer API.
hipStream_t gdsp_api::thread_stream(int dev) {
  thread_local std::map<int, hipStream_t> streams;
  auto it = streams.find(dev);
  if (it != streams.end()) return it->second;
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
  streams[dev] = s;
  return s;
}

namespace {

// The one-kernel transform exchanges real and imaginary halves in turn
// (half the LDS, so more workgroups per CU than with two buffers).
bool lds_split_default() { return true; }

std::atomic<unsigned> g_algo{GDSP_ALGO_DEFAULT};
constexpr unsigned kAlgoAll = GDSP_ALGO_GENERIC_MIXED | GDSP_ALGO_NO_CHIRPZ_PARTS |
                              GDSP_ALGO_CHIRPZ_POW2 | GDSP_ALGO_CHIRPZ_UNFUSED |
                              GDSP_ALGO_NO_RADER | GDSP_ALGO_NO_RACE |
                              GDSP_ALGO_NO_FUSED_CONVOLVE | GDSP_ALGO_NO_FUSED_PWELCH_BATCH |
                              GDSP_ALGO_NO_FUSED_CPSD | GDSP_ALGO_NO_FUSED_FIR |
                              GDSP_ALGO_NO_FUSED_STFT | GDSP_ALGO_NO_FUSED_ISTFT |
                              GDSP_ALGO_NO_FUSED_UPFIRDN | GDSP_ALGO_NO_FUSED_HILBERT |
                              GDSP_ALGO_NO_FUSED_SOSFILT | GDSP_ALGO_NO_FUSED_CZT |
                              GDSP_ALGO_NO_FUSED_DCT;

// Scratch device memory: a grow-only buffer per (device, stream, use-site
// slot), allocated with hipMalloc. Reuse is ordered by the stream itself: a
// slot is only ever used by work queued on its stream, so a later call can
// overwrite it only after the earlier kernels on that stream ran. Growing a
// slot synchronises its stream before freeing the old buffer.
// (Stream-ordered hipMallocAsync/hipFreeAsync lost kernel output
// intermittently under the ROCm 7.2 runtime here — tests/cpp reproduced it —
// so the library does not use it.) Device-API callers must not drive one
// stream from two host threads at once.
struct Workspace {
  void *buf[SLOT_COUNT] = {};
  size_t cap[SLOT_COUNT] = {};
};

std::mutex g_ws_mu;
std::map<std::pair<int, hipStream_t>, Workspace> g_ws;

}  // namespace

int gdsp_api::DevBuf::alloc(size_t bytes, hipStream_t st, Slot slot) {
  if (bytes == 0) bytes = 16;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(GDSP_ERR_NO_DEVICE, "hipGetDevice failed");
  std::lock_guard<std::mutex> lk(g_ws_mu);
  Workspace &w = g_ws[std::make_pair(dev, st)];
  if (w.cap[slot] < bytes) {
    if (w.buf[slot]) {
      HIPCHK(hipStreamSynchronize(st));  // queued users of the old buffer
      HIPCHK(hipFree(w.buf[slot]));
      w.buf[slot] = nullptr;
      w.cap[slot] = 0;
    }
    const size_t want = bytes + bytes / 4;  // headroom against regrowth
    hipError_t e = hipMalloc(&w.buf[slot], want);
    if (e != hipSuccess) {
      w.buf[slot] = nullptr;
      return fail(GDSP_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    w.cap[slot] = want;
  }
  p = w.buf[slot];
  return GDSP_OK;
}

namespace {

// Host <-> device copies through library-owned pinned staging buffers (two
// halves, double-buffered). The caller's memory is only touched by memcpy on
// the host, so pageable (Go / numpy) buffers never reach the HIP runtime and
// no pointer is retained after the call returns (cgo rule).
struct Staging {
  char *buf = nullptr;
  size_t half = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool pending[2] = {false, false};  // a queued copy may still read / write the half
  ~Staging() {
    if (buf) (void)hipHostFree(buf);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// 8 MiB halves: a 16 MiB vector (BenchmarkFFT's 2^20) already pipelines its
// host memcpy with the DMA of the previous half
constexpr size_t kStagingHalf = (size_t)8 << 20;

// memcpy between the caller's pageable memory and the pinned staging, split
// over a few host threads for large chunks (one thread copies ~10-20 GB/s,
// well below what PCIe moves)
void host_copy(void *dst, const void *src, size_t n) {
  constexpr size_t kPar = (size_t)2 << 20;
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned k = n < kPar ? 1 : std::min<unsigned>(4, hw ? hw : 1);
  if (k <= 1) {
    memcpy(dst, src, n);
    return;
  }
  const size_t part = (n / k + 63) & ~(size_t)63;
  std::thread th[3];
  size_t rest = n;  // this thread also copies [rest, n) if a thread could not start
  unsigned used = 0;
  for (unsigned i = 1; i < k && i * part < n; ++i) {
    const size_t off = i * part, c = std::min(part, n - off);
    try {
      th[used] = std::thread([=] { memcpy((char *)dst + off, (const char *)src + off, c); });
      ++used;
    } catch (...) {  // nothing may throw past the C ABI
      rest = off;
      break;
    }
  }
  memcpy(dst, src, std::min(part, n));
  if (rest < n) memcpy((char *)dst + rest, (const char *)src + rest, n - rest);
  for (unsigned i = 0; i < used; ++i) th[i].join();
}

int staging_get(Staging **out) {
  thread_local std::map<int, Staging> per_dev;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(GDSP_ERR_NO_DEVICE, "hipGetDevice failed");
  Staging &st = per_dev[dev];
  if (!st.buf) {
    HIPCHK(hipHostMalloc((void **)&st.buf, 2 * kStagingHalf, hipHostMallocDefault));
    st.half = kStagingHalf;
    for (auto &e : st.ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  *out = &st;
  return GDSP_OK;
}

}  // namespace

// Host -> device through the staging halves. A half is refilled only after
// the copy that last used it has completed (its event); the copies themselves
// stay queued, and the stream orders them before the kernels and the
// device -> host copies that follow on the same stream.
int gdsp_api::copy_h2d(void *dst, const void *src, size_t bytes, hipStream_t s) {
  Staging *st = nullptr;
  STCHK(staging_get(&st));
  int h = 0;
  for (size_t off = 0; off < bytes; off += st->half, h ^= 1) {
    const size_t c = bytes - off < st->half ? bytes - off : st->half;
    char *stg = st->buf + (size_t)h * st->half;
    if (st->pending[h]) {
      HIPCHK(hipEventSynchronize(st->ev[h]));
      st->pending[h] = false;
    }
    host_copy(stg, (const char *)src + off, c);
    HIPCHK(hipMemcpyAsync((char *)dst + off, stg, c, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(st->ev[h], s));
    st->pending[h] = true;
  }
  return GDSP_OK;
}

// Device -> host, double-buffered; returns once every chunk has landed in
// dst, so everything queued on s before it has completed too.
int gdsp_api::copy_d2h(void *dst, const void *src, size_t bytes, hipStream_t s) {
  Staging *st = nullptr;
  STCHK(staging_get(&st));
  const size_t nchunk = (bytes + st->half - 1) / st->half;
  auto issue = [&](size_t i) -> int {
    const size_t off = i * st->half;
    const size_t c = bytes - off < st->half ? bytes - off : st->half;
    HIPCHK(hipMemcpyAsync(st->buf + (i & 1) * st->half, (const char *)src + off, c,
                          hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(st->ev[i & 1], s));
    st->pending[i & 1] = true;
    return GDSP_OK;
  };
  if (nchunk) STCHK(issue(0));
  for (size_t i = 0; i < nchunk; ++i) {
    if (i + 1 < nchunk) STCHK(issue(i + 1));
    HIPCHK(hipEventSynchronize(st->ev[i & 1]));
    st->pending[i & 1] = false;
    const size_t off = i * st->half;
    const size_t c = bytes - off < st->half ? bytes - off : st->half;
    host_copy((char *)dst + off, st->buf + (i & 1) * st->half, c);
  }
  return GDSP_OK;
}

int gdsp_api::stage_rows(double *d, const double *h, int64_t rows, int64_t n, int64_t ld,
                         int64_t lx, hipStream_t s) {
  if (lx > n) HIPCHK(hipMemsetAsync(d, 0, (size_t)rows * (size_t)lx * sizeof(double), s));
  if (lx == n && (ld == n || rows == 1))
    return copy_h2d(d, h, (size_t)rows * (size_t)n * sizeof(double), s);
  for (int64_t c = 0; c < rows; ++c)
    STCHK(copy_h2d(d + c * lx, h + c * ld, (size_t)n * sizeof(double), s));
  return GDSP_OK;
}

int gdsp_api::unstage_rows(double *h, const double *d, int64_t rows, int64_t n, int64_t ld,
                           hipStream_t s) {
  if (ld == n || rows == 1) return copy_d2h(h, d, (size_t)rows * (size_t)n * sizeof(double), s);
  for (int64_t c = 0; c < rows; ++c)
    STCHK(copy_d2h(h + c * ld, d + c * n, (size_t)n * sizeof(double), s));
  return GDSP_OK;
}

namespace {

// Mapped pinned host memory per (thread, device) for small host calls
// (input at 0, output at kZeroCopyOut): the kernels access it over the
// fabric, which for a few hundred KiB costs less than two copy launches.
constexpr size_t kZeroCopyOut = (size_t)512 << 10;
constexpr size_t kZeroCopyMax = (size_t)512 << 10;  // in + out bytes of one call
struct ZeroCopy {
  char *host = nullptr;
  void *dev = nullptr;
  ~ZeroCopy() {
    if (host) (void)hipHostFree(host);
  }
};

int zero_copy_get(ZeroCopy **out) {
  thread_local std::map<int, ZeroCopy> per_dev;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(GDSP_ERR_NO_DEVICE, "hipGetDevice failed");
  ZeroCopy &z = per_dev[dev];
  if (!z.host) {
    HIPCHK(hipHostMalloc((void **)&z.host, 2 * kZeroCopyOut, hipHostMallocMapped));
    hipError_t e = hipHostGetDevicePointer(&z.dev, z.host, 0);
    if (e != hipSuccess) {
      (void)hipHostFree(z.host);
      z.host = nullptr;
      return fail(GDSP_ERR_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
    }
  }
  *out = &z;
  return GDSP_OK;
}

// Large power of 2: radix-16 Stockham passes through HBM, last pass into out.
int exec_global(const gdsp_plan *p, const void *in, cd *out, int64_t batch, bool inv, int load,
                hipStream_t s) {
  std::vector<int> radix;
  int rem = p->log2n;
  while (rem >= 4) {
    radix.push_back(16);
    rem -= 4;
  }
  if (rem) radix.push_back(1 << rem);
  const int np = (int)radix.size();
  const size_t bytes = (size_t)batch * (size_t)p->n * sizeof(cd);
  DevBuf scratch, inbuf;
  STCHK(scratch.alloc(bytes, s, SLOT_GLOBAL));
  const void *src = in;
  if (in == (const void *)out && ((np - 1) % 2 == 0)) {
    STCHK(inbuf.alloc(bytes, s, SLOT_GLOBAL_IN));
    HIPCHK(hipMemcpyAsync(inbuf.p, in, bytes, hipMemcpyDeviceToDevice, s));
    src = inbuf.p;
  }
  int log2ns = 0;
  for (int q = 0; q < np; ++q) {
    cd *dst = ((np - 1 - q) % 2 == 0) ? out : (cd *)scratch.p;
    HIPCHK(gdsp::launch_global_pass(radix[q], inv && q == 0, q == 0 ? load : gdsp::LOAD_COMPLEX,
                                    inv && q == np - 1, src, dst, p->tw, p->log2n, log2ns, batch,
                                    1.0 / (double)p->n, s));
    src = dst;
    log2ns += ilog2(radix[q]);
  }
  return GDSP_OK;
}

// Large power of 2, N = R*C (x as R rows x C columns, n = C*n1 + n2):
//   A  column DFT_R over n1 for every n2, times W_N^(n2*k1)  (tile kernel, into work)
//   B  row DFT_C over n2 for every k1, contiguous rows        (LDS kernel / recursion)
//   C  X[k1 + R*k2] = Y[k1][k2]: transpose R x C -> C x R      (into out)
// Three HBM round trips for N <= 2^22 (vs one per radix-16 pass), any batch.
int exec_plan_depth(const gdsp_plan *p, const void *in, cd *out, int64_t batch, bool inv,
                    int load, hipStream_t s, int depth);

void fourstep_split(int ln, int *lr, int *lc);

// 2^15 <= N <= 2^20: two HBM round trips instead of three. N = R*C with
// rows of C = 256 (512 at 2^18, 1024 from 2^19): the column pass as below,
// then the rows DFT_C with the transpose fused into their store
// (rowfft_t_kernel: a workgroup's TPW = 256 / (C / 16) rows leave as 64-256-B
// segments of X). Per 2^27 samples (profiles/r04/fourstep2_ab.txt): 2^15
// 2.10 -> 1.46 ms, 2^16 2.17 -> 1.55, 2^17 2.16 -> 1.57, 2^18 2.11 -> 1.60,
// 2^19 2.16 -> 1.88, 2^20 2.21 -> 1.90; BenchmarkFFT's one 2^20 transform
// 0.039 -> 0.031 ms. (fourstep2_applies: plan.hpp, the planner asks it too.)
int fourstep2_lc(int ln) { return ln >= 19 ? 10 : (ln >= 18 ? 9 : 8); }

int exec_fourstep2(const gdsp_plan *p, const void *in, cd *out, int64_t batch, bool inv, int load,
                   hipStream_t s, int depth) {
  const int ln = p->log2n;
  const int lc = fourstep2_lc(ln), lr = ln - lc;
  gdsp_plan *pr = nullptr, *pcol = nullptr;
  STCHK(get_plan((int64_t)1 << lr, &pr));
  STCHK(get_plan((int64_t)1 << lc, &pcol));
  const int64_t N = p->n, R = (int64_t)1 << lr, C = (int64_t)1 << lc;
  DevBuf work;
  // (its own slot per recursion depth: as the rows of a longer four-step it
  // runs while the caller's work buffer, SLOT_FS0 + depth - 1, holds them)
  STCHK(work.alloc((size_t)batch * (size_t)N * sizeof(cd), s, (Slot)(SLOT_FS0 + depth)));
  cd *w = (cd *)work.p;
  const cd *src = (const cd *)in;
  if (load == gdsp::LOAD_REAL) {
    HIPCHK(gdsp::launch_real_to_complex((const double *)in, w, batch * N, s));
    src = w;
  }
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    later_chunk(b0);
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    HIPCHK(gdsp::launch_colfft(lr, inv, 2, false, src + b0 * N, w + b0 * N, C, 1, 0, 1, 0, 1,
                               pr->tw, p->tw, ln, 1.0, nb, N, s));
  }
  HIPCHK(gdsp::launch_rowfft_t(lc, inv ? 1 : 0, w, out, batch * R, R, pcol->tw, 1.0 / (double)N,
                               s));
  return GDSP_OK;
}

int exec_fourstep(const gdsp_plan *p, const void *in, cd *out, int64_t batch, bool inv, int load,
                  hipStream_t s, int depth) {
  const int ln = p->log2n;
  if (depth >= 4) return fail(GDSP_ERR_UNSUPPORTED, "transform too long");
  if (fourstep2_applies(ln)) return exec_fourstep2(p, in, out, batch, inv, load, s, depth);
  int lr, lc;
  fourstep_split(ln, &lr, &lc);
  // Few transforms: rows of 8192 leave the row pass at <= 256 workgroups, and
  // rows of 4096 (twice the rows, the column DFT twice as long) measured
  // 5-20 % faster per call at batch * 2^(ln-13) <= 256 (2^17..2^21 at batch 1:
  // 2^20 0.0275 -> 0.026 ms, 2^18 0.022 -> 0.0177; scripts/archive/dev/fs_split_ab.py,
  // profiles/r02/fs_split.jsonl); larger batches keep 8192.
  if (lc == 13 && lr + 1 <= gdsp::kColMaxLog2 && (batch << lr) <= 256) {
    lc = 12;
    lr += 1;
  }
  if (depth >= 4) return fail(GDSP_ERR_UNSUPPORTED, "transform too long");
  gdsp_plan *pr = nullptr, *pcol = nullptr;
  STCHK(get_plan((int64_t)1 << lr, &pr));
  STCHK(get_plan((int64_t)1 << lc, &pcol));
  const int64_t N = p->n, R = (int64_t)1 << lr, C = (int64_t)1 << lc;
  DevBuf work;
  STCHK(work.alloc((size_t)batch * (size_t)N * sizeof(cd), s, (Slot)(SLOT_FS0 + depth)));
  cd *w = (cd *)work.p;
  const cd *src = (const cd *)in;
  if (load == gdsp::LOAD_REAL) {
    HIPCHK(gdsp::launch_real_to_complex((const double *)in, w, batch * N, s));
    src = w;
  }
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    later_chunk(b0);
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    HIPCHK(gdsp::launch_colfft(lr, inv, 2, false, src + b0 * N, w + b0 * N, C, 1, 0, 1, 0, 1,
                               pr->tw, p->tw, ln, 1.0, nb, N, s));
  }
  STCHK(exec_plan_depth(pcol, w, w, batch * R, false, gdsp::LOAD_COMPLEX, s, depth + 1));
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    later_chunk(b0);
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    HIPCHK(gdsp::launch_transpose(w + b0 * N, out + b0 * N, R, C, s, nb, inv,
                                  1.0 / (double)N));
  }
  return GDSP_OK;
}

// Smooth non-power-of-2 n = N1*N2 beyond one kernel (x as N1 rows x N2
// columns, n = N2*n1 + n2, k = k1 + N1*k2), every step a one-kernel pass:
//   a  transpose x -> B (N2 x N1)                          (w1)
//   b  DFT_N1 along B's rows                               (in place)
//   c  transpose -> Y (N1 x N2), times W_N^(n2*k1)         (w2)
//   d  DFT_N2 along Y's rows                               (in place)
//   e  transpose -> X (N2 x N1), X[k1 + N1*k2] = Z[k1][k2] (out)
// Inverse: inverse sub-transforms (1/N1 * 1/N2 = 1/N) and conj(W).
// The reference runs these lengths through Bluestein (fft/bluestein.go).
// Column pass (conj in for an inverse) and rows of a three-pass mixed
// four-step plan, src -> w; the R x C -> C x R transpose is left to the caller.
int mixed4_col_rows(const gdsp_plan *p, const cd *src, cd *w, int64_t batch, bool inv,
                    hipStream_t s) {
  const int64_t N = p->n, N1 = p->n1, N2 = p->n2;
  const int lr = p->pow2col ? ilog2(N1) : 0;
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    later_chunk(b0);
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    if (p->mixcol)
      HIPCHK(gdsp::jit_launch_col(p->mixcol, inv, src + b0 * N, w + b0 * N, N2, N, nb, p->p1->tw,
                                  p->tw, s));
    else if (p->radixcol)
      HIPCHK(gdsp::launch_colradix((int)N1, inv, src + b0 * N, w + b0 * N, N2, N, nb, p->tw, s));
    else
      HIPCHK(gdsp::launch_colfft(lr, inv, 2, false, src + b0 * N, w + b0 * N, N2, 1, 0, 1, 0, 1,
                                 p->p1->tw, p->tw, 0, 1.0, nb, N, s, N));
  }
  return exec_plan(p->p2, w, w, batch * N1, false, gdsp::LOAD_COMPLEX, s);
}

int exec_mixed4(const gdsp_plan *p, const void *in, cd *out, int64_t batch, bool inv, int load,
                hipStream_t s) {
  const int64_t N = p->n, N1 = p->n1, N2 = p->n2;
  if (p->rowst) {
    // columns DFT_N1 times W_N^(col*k1) (conj in for an inverse), then rows
    // DFT_N2 (a power of 2) whose store carries the transpose (and conj +
    // 1/N for an inverse)
    DevBuf work;
    STCHK(work.alloc((size_t)batch * (size_t)N * sizeof(cd), s, SLOT_MX0));
    cd *w = (cd *)work.p;
    const cd *src = (const cd *)in;
    if (load == gdsp::LOAD_REAL) {
      HIPCHK(gdsp::launch_real_to_complex((const double *)in, w, batch * N, s));
      src = w;
    }
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
      later_chunk(b0);
      const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
      if (p->mixcol)
        HIPCHK(gdsp::jit_launch_col(p->mixcol, inv, src + b0 * N, w + b0 * N, N2, N, nb, p->p1->tw,
                                    p->tw, s));
      else if (p->radixcol)
        HIPCHK(gdsp::launch_colradix((int)N1, inv, src + b0 * N, w + b0 * N, N2, N, nb, p->tw, s));
      else
        HIPCHK(gdsp::launch_colfft(ilog2(N1), inv, 2, false, src + b0 * N, w + b0 * N, N2, 1, 0, 1,
                                   0, 1, p->p1->tw, p->tw, 0, 1.0, nb, N, s, N));
    }
    if (p->rowt)
      HIPCHK(gdsp::jit_launch_rowt(p->rowt, inv, w, out, batch * N1, N1, p->p2->tw,
                                   1.0 / (double)N, s));
    else
      HIPCHK(gdsp::launch_rowfft_t(ilog2(N2), inv ? 1 : 0, w, out, batch * N1, N1, p->p2->tw,
                                   1.0 / (double)N, s));
    return GDSP_OK;
  }
  if (p->pow2col || p->radixcol || p->mixcol) {
    // as exec_fourstep with R = N1 (power of 2) and C = N2 (any one-kernel
    // length): column DFT_R on row-segment tiles times W_N^(col*k1) (table
    // index mod N), rows DFT_C, conj/scale-fused transpose R x C -> C x R
    DevBuf work;
    STCHK(work.alloc((size_t)batch * (size_t)N * sizeof(cd), s, SLOT_MX0));
    cd *w = (cd *)work.p;
    const cd *src = (const cd *)in;
    if (load == gdsp::LOAD_REAL) {
      HIPCHK(gdsp::launch_real_to_complex((const double *)in, w, batch * N, s));
      src = w;
    }
    STCHK(mixed4_col_rows(p, src, w, batch, inv, s));
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
      later_chunk(b0);
      const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
      HIPCHK(gdsp::launch_transpose(w + b0 * N, out + b0 * N, N1, N2, s, nb, inv,
                                    1.0 / (double)N));
    }
    return GDSP_OK;
  }
  const size_t bytes = (size_t)batch * (size_t)N * sizeof(cd);
  DevBuf b1, b2;
  STCHK(b1.alloc(bytes, s, SLOT_MX0));
  STCHK(b2.alloc(bytes, s, SLOT_MX1));
  cd *w1 = (cd *)b1.p, *w2 = (cd *)b2.p;
  const cd *src = (const cd *)in;
  if (load == gdsp::LOAD_REAL) {
    HIPCHK(gdsp::launch_real_to_complex((const double *)in, w2, batch * N, s));
    src = w2;
  }
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    later_chunk(b0);
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    HIPCHK(gdsp::launch_transpose(src + b0 * N, w1 + b0 * N, N1, N2, s, nb));
  }
  STCHK(exec_plan(p->p1, w1, w1, batch * N2, inv, gdsp::LOAD_COMPLEX, s));
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    later_chunk(b0);
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    HIPCHK(gdsp::launch_transpose(w1 + b0 * N, w2 + b0 * N, N2, N1, s, nb, false, 1.0, p->tw, N,
                                  inv));
  }
  STCHK(exec_plan(p->p2, w2, w2, batch * N1, inv, gdsp::LOAD_COMPLEX, s));
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    later_chunk(b0);
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    HIPCHK(gdsp::launch_transpose(w2 + b0 * N, out + b0 * N, N1, N2, s, nb));
  }
  return GDSP_OK;
}

// log2 of the column and row lengths exec_fourstep uses for a 2^ln FFT
void fourstep_split(int ln, int *lr, int *lc) {
  if (ln - 13 >= gdsp::kColMinLog2 && ln - 13 <= gdsp::kColMaxLog2) {
    *lc = 13;
    *lr = ln - 13;
  } else if (ln - 13 < gdsp::kColMinLog2) {
    *lr = gdsp::kColMinLog2;
    *lc = ln - *lr;
  } else {
    *lr = gdsp::kColMaxLog2;
    *lc = ln - *lr;  // rows longer than 8192 recurse
  }
}

int exec_bluestein_composed(const gdsp_plan *p, const cd *in, cd *out, int64_t batch, bool inv,
                            hipStream_t s) {
  DevBuf a;
  STCHK(a.alloc((size_t)batch * (size_t)p->m * sizeof(cd), s, SLOT_BLU));
  cd *da = (cd *)a.p;
  const bool two_pass =
      !p->unfused && p->mplan->kind == KIND_GLOBAL && fourstep2_applies(p->log2m);
  // (the two-pass form folds the premultiply into its first column pass)
  if (!two_pass) HIPCHK(gdsp::launch_chirp_premul(in, da, p->n, p->m, batch, p->chirp, inv, s));
  const gdsp_plan *mp = p->mplan;
  if (!p->unfused && mp->kind == KIND_MIXED4 && (mp->pow2col || mp->radixcol || mp->mixcol)) {
    // smooth M (a three-pass mixed four-step): the same two fused transposes
    const int64_t M = p->m;
    DevBuf work;
    STCHK(work.alloc((size_t)batch * (size_t)M * sizeof(cd), s, SLOT_MX0));
    cd *w = (cd *)work.p;
    for (int pass = 1; pass <= 2; ++pass) {
      STCHK(mixed4_col_rows(mp, da, w, batch, false, s));
      for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
        later_chunk(b0);
        const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
        if (pass == 1)
          HIPCHK(gdsp::launch_transpose_blu(w + b0 * M, da + b0 * M, mp->n1, mp->n2, nb, 1, p->n,
                                            p->bhat, false, 1.0, s));
        else
          HIPCHK(gdsp::launch_transpose_blu(w + b0 * M, out + b0 * p->n, mp->n1, mp->n2, nb, 2,
                                            p->n, p->chirp, inv, 1.0 / (double)p->n, s));
      }
    }
    return GDSP_OK;
  }
  if (two_pass) {
    // 2^15 <= M <= 2^20: both FFT_M as the two-pass four-step, the
    // premultiply in the first column pass's loads (colfft_chirp_kernel: x
    // read once, the zero padding never), the b-hat and output steps in the
    // rows' transposed store (rowfft_t_kernel modes 2 and 3): 2 + 2 passes
    // over M instead of 1 + 3 + 3
    const int lc2 = fourstep2_lc(p->log2m), lr2 = p->log2m - lc2;
    const int64_t M = p->m, R = (int64_t)1 << lr2, C = (int64_t)1 << lc2;
    gdsp_plan *pr = nullptr, *pcol = nullptr;
    STCHK(get_plan(R, &pr));
    STCHK(get_plan(C, &pcol));
    DevBuf work;
    STCHK(work.alloc((size_t)batch * (size_t)M * sizeof(cd), s, SLOT_FS0));
    cd *w = (cd *)work.p;
    for (int pass = 1; pass <= 2; ++pass) {
      for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
        later_chunk(b0);
        const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
        if (pass == 1)
          HIPCHK(gdsp::launch_colfft_chirp(lr2, inv, in + b0 * p->n, w + b0 * M, C, p->n, p->chirp,
                                           pr->tw, p->mplan->tw, nb, s));
        else
          HIPCHK(gdsp::launch_colfft(lr2, false, 2, false, da + b0 * M, w + b0 * M, C, 1, 0, 1, 0,
                                     1, pr->tw, p->mplan->tw, p->log2m, 1.0, nb, M, s));
      }
      if (pass == 1)
        HIPCHK(gdsp::launch_rowfft_t(lc2, 2, w, da, batch * R, R, pcol->tw, 1.0, s, p->bhat,
                                     p->n, false));
      else
        HIPCHK(gdsp::launch_rowfft_t(lc2, 3, w, out, batch * R, R, pcol->tw,
                                     1.0 / (double)p->n, s, p->chirp, p->n, inv));
    }
    return GDSP_OK;
  }
  int lr = 0, lc = 0;
  fourstep_split(p->log2m, &lr, &lc);
  if (!p->unfused && lc <= 13 && p->mplan->kind == KIND_GLOBAL) {
    // both FFT_M as exec_fourstep's column tiles + rows, each final
    // transpose carrying the chirp-z step after it: conj(A * bhat) into da,
    // then conj(r) * chirp into out (two passes over M fewer)
    const int64_t M = p->m, R = (int64_t)1 << lr, C = (int64_t)1 << lc;
    gdsp_plan *pr = nullptr, *pcol = nullptr;
    STCHK(get_plan(R, &pr));
    STCHK(get_plan(C, &pcol));
    DevBuf work;
    STCHK(work.alloc((size_t)batch * (size_t)M * sizeof(cd), s, SLOT_FS0));
    cd *w = (cd *)work.p;
    for (int pass = 1; pass <= 2; ++pass) {
      for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
        later_chunk(b0);
        const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
        HIPCHK(gdsp::launch_colfft(lr, false, 2, false, da + b0 * M, w + b0 * M, C, 1, 0, 1, 0, 1,
                                   pr->tw, p->mplan->tw, p->log2m, 1.0, nb, M, s));
      }
      STCHK(exec_plan_depth(pcol, w, w, batch * R, false, gdsp::LOAD_COMPLEX, s, 1));
      for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
        later_chunk(b0);
        const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
        if (pass == 1)
          HIPCHK(gdsp::launch_transpose_blu(w + b0 * M, da + b0 * M, R, C, nb, 1, p->n, p->bhat,
                                            false, 1.0, s));
        else
          HIPCHK(gdsp::launch_transpose_blu(w + b0 * M, out + b0 * p->n, R, C, nb, 2, p->n,
                                            p->chirp, inv, 1.0 / (double)p->n, s));
      }
    }
    return GDSP_OK;
  }
  STCHK(exec_plan(p->mplan, da, da, batch, false, gdsp::LOAD_COMPLEX, s));
  HIPCHK(gdsp::launch_bhat_mul_conj(da, p->m, batch, p->bhat, s));
  STCHK(exec_plan(p->mplan, da, da, batch, false, gdsp::LOAD_COMPLEX, s));
  HIPCHK(gdsp::launch_chirp_postmul(da, out, p->n, p->m, batch, p->chirp, inv,
                                    1.0 / (double)p->n, s));
  return GDSP_OK;
}

// Batched transform of `batch` rows of n on device buffers. load = LOAD_REAL
// reads float64 rows (fft.FFTReal); in == out is allowed.
}  // namespace
int gdsp_api::exec_plan(const gdsp_plan *p, const void *in, cd *out, int64_t batch, bool inv,
                        int load, hipStream_t s) {
  return exec_plan_depth(p, in, out, batch, inv, load, s, 0);
}
namespace {

int exec_plan_depth(const gdsp_plan *p, const void *in, cd *out, int64_t batch, bool inv,
                    int load, hipStream_t s, int depth) {
  if (batch <= 0) return GDSP_OK;
  const double scale = 1.0 / (double)(p->n > 0 ? p->n : 1);
  switch (p->kind) {
    case KIND_TRIVIAL: {
      if (p->n == 0) return GDSP_OK;
      if (load == gdsp::LOAD_REAL) {
        HIPCHK(gdsp::launch_real_to_complex((const double *)in, out, batch, s));
      } else if (in != (const void *)out) {
        HIPCHK(hipMemcpyAsync(out, in, (size_t)batch * sizeof(cd), hipMemcpyDeviceToDevice, s));
      }
      return GDSP_OK;
    }
    case KIND_MIXED:
      if (p->jit)
        HIPCHK(gdsp::jit_launch_fft(p->jit, inv, load, in, out, batch, p->tw, scale, s));
      else
        HIPCHK(gdsp::launch_fft_mixed(p->md, inv, load, in, out, batch, p->tw, scale, s));
      return GDSP_OK;
    case KIND_MIXED4:
      return exec_mixed4(p, in, out, batch, inv, load, s);
    case KIND_RADER:
      HIPCHK(gdsp::jit_launch_rader(p->rader, inv, load, in, out, batch, p->tw, p->bhat, p->gpow,
                                    p->ginv, scale, s));
      return GDSP_OK;
    case KIND_RADER_PFA: {
      const gdsp_plan *q = p->p2;  // the prime factor's Rader tables
      HIPCHK(gdsp::jit_launch_rader(p->rader, inv, load, in, out, batch, q->tw, q->bhat, q->gpow,
                                    q->ginv, scale, s));
      return GDSP_OK;
    }
    case KIND_LDS:
      HIPCHK(gdsp::launch_fft_lds(p->log2n, inv, load, lds_split_default(), in, out, batch, p->tw,
                                  scale, s));
      return GDSP_OK;
    case KIND_GLOBAL:
      if (p->log2n <= 13 + 3 * gdsp::kColMaxLog2)
        return exec_fourstep(p, in, out, batch, inv, load, s, depth);
      return exec_global(p, in, out, batch, inv, load, s);
    case KIND_BLUESTEIN:
    case KIND_BLUESTEIN_COMPOSED: {
      if (p->kind == KIND_BLUESTEIN && p->blufix) {
        HIPCHK(gdsp::jit_launch_blu(p->blufix, inv, load, in, out, batch, p->tw_blu, p->chirp,
                                    p->bhat_blu, scale, s));
        return GDSP_OK;
      }
      if (p->kind == KIND_BLUESTEIN && p->c6k) {
        // real input read by the kernel itself (no complex copy first)
        HIPCHK(gdsp::launch_chirpz6k(p->m, inv, load, in, out, p->n, batch, p->tw6k, p->chirp,
                                     p->bhat, scale, s));
        return GDSP_OK;
      }
      const cd *src = (const cd *)in;
      DevBuf tmp;
      if (load == gdsp::LOAD_REAL) {
        STCHK(tmp.alloc((size_t)batch * (size_t)p->n * sizeof(cd), s, SLOT_REAL));
        HIPCHK(gdsp::launch_real_to_complex((const double *)in, (cd *)tmp.p, batch * p->n, s));
        src = (const cd *)tmp.p;
      }
      if (p->kind == KIND_BLUESTEIN && p->parts > 1) {
        // the parts of a row run in different workgroups, so a part may
        // write the row before another has read it: in place (the four-step
        // rows, or a caller's in == out) goes through a copy of the input
        DevBuf cp;
        if ((const void *)src == (const void *)out) {
          const size_t bytes = (size_t)batch * (size_t)p->n * sizeof(cd);
          STCHK(cp.alloc(bytes, s, SLOT_PARTS));
          HIPCHK(hipMemcpyAsync(cp.p, src, bytes, hipMemcpyDeviceToDevice, s));
          src = (const cd *)cp.p;
        }
        HIPCHK(gdsp::launch_bluestein_parts(p->log2m, inv, src, out, p->n, batch, p->parts,
                                            p->kpart, p->mplan->tw, p->chirp, p->bhat, scale,
                                            s));
        return GDSP_OK;
      }
      if (p->kind == KIND_BLUESTEIN) {
        HIPCHK(gdsp::launch_bluestein(p->log2m, inv, src, out, p->n, batch, p->mplan->tw, p->chirp,
                                      p->bhat, scale, s));
        return GDSP_OK;
      }
      return exec_bluestein_composed(p, src, out, batch, inv, s);
    }
  }
  return fail(GDSP_ERR_INVALID, "bad plan kind");
}

}  // namespace

// Host-pointer batched transform: H2D, exec, D2H, synchronise.
int gdsp_api::host_batch(const void *x, size_t in_elem_bytes, double *out, int64_t n,
                         int64_t batch, bool inv, int load) {
  if (n < 0 || batch < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (batch == 0) return GDSP_OK;
  if (n == 0) {
    if (inv) return fail(GDSP_ERR_EMPTY, "IFFT of an empty slice (index out of range)");
    return GDSP_OK;
  }
  if (!x || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  gdsp_plan *p = nullptr;
  STCHK(get_plan(n, &p));
  hipStream_t s = thread_stream(p->device);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const size_t in_bytes = (size_t)batch * (size_t)n * in_elem_bytes;
  const size_t out_bytes = (size_t)batch * (size_t)n * sizeof(cd);
  if (in_bytes + out_bytes <= kZeroCopyMax) {
    // small calls: the kernels read and write mapped pinned host memory
    // directly — one launch and one synchronisation instead of two copies
    ZeroCopy *zc = nullptr;
    STCHK(zero_copy_get(&zc));
    memcpy(zc->host, x, in_bytes);
    char *dbase = (char *)zc->dev;
    const int st = exec_plan(p, dbase, (cd *)(dbase + kZeroCopyOut), batch, inv, load, s);
    // drain even on failure: kernels already queued may still touch the
    // mapped buffer the next call on this thread refills
    const hipError_t se = hipStreamSynchronize(s);
    if (st != GDSP_OK) return st;
    if (se != hipSuccess)
      return fail(GDSP_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    memcpy(out, zc->host + kZeroCopyOut, out_bytes);
    return GDSP_OK;
  }
  DevBuf din, dout;
  STCHK(din.alloc(in_bytes, s, SLOT_IN));
  STCHK(dout.alloc(out_bytes, s, SLOT_OUT));
  STCHK(run_queued(s, [&]() -> int {
    STCHK(copy_h2d(din.p, x, in_bytes, s));
    return exec_plan(p, din.p, (cd *)dout.p, batch, inv, load, s);
  }));
  STCHK(copy_d2h(out, dout.p, out_bytes, s));  // returns after the stream drained
  return GDSP_OK;
}

// Configuration (launch.hpp): the deployment knobs, the development build's
// experiment switches and the algorithm flags.
namespace gdsp {
const char *knob(Knob k) {
  static const char *const names[] = {"GDSP_DEVICES",   "GDSP_MULTI_MIN_BYTES", "GDSP_JIT",
                                      "GDSP_JIT_INCLUDE", "GDSP_JIT_CACHE",     "GDSP_JIT_VERBOSE",
                                      "XDG_CACHE_HOME",  "HOME"};
  return (int)k >= 0 && (int)k < (int)(sizeof names / sizeof names[0]) ? getenv(names[k]) : nullptr;
}
// Inside a plan build (build_flags, plan.hip) every reader — mixed_fixed_radices,
// pwelch_fixed_radices, jit_enabled, ... — sees the flags snapshot the plan is
// cached under (plan_flags), so a concurrent gdsp_set_algorithm cannot give
// one plan parts chosen under different flags.
unsigned algo_flags() {
  unsigned f = 0;
  return gdsp_api::build_flags(&f) ? f : g_algo.load(std::memory_order_relaxed);
}
}  // namespace gdsp

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

const char *gdsp_status_string(int st) {
  switch (st) {
    case GDSP_OK: return "ok";
    case GDSP_ERR_INVALID: return "invalid argument";
    case GDSP_ERR_UNEQUAL: return "arrays not of equal size";
    case GDSP_ERR_EMPTY: return "empty input array";
    case GDSP_ERR_RAGGED: return "ragged input array";
    case GDSP_ERR_DIVIDE_BY_ZERO: return "integer divide by zero";
    case GDSP_ERR_NO_DEVICE: return "no HIP device";
    case GDSP_ERR_HIP: return "HIP runtime error";
    case GDSP_ERR_NOMEM: return "out of memory";
    case GDSP_ERR_UNSUPPORTED: return "unsupported size";
  }
  return "unknown status";
}

const char *gdsp_last_error(void) { return g_last_error.c_str(); }
const char *gdsp_version(void) { return GDSP_VERSION; }

int gdsp_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int gdsp_set_algorithm(unsigned flags) {
  if (flags & ~kAlgoAll) return fail(GDSP_ERR_INVALID, "unknown algorithm flag");
  g_algo.store(flags);
  return GDSP_OK;
}

unsigned gdsp_get_algorithm(void) { return g_algo.load(); }

int gdsp_loop_stats(int64_t *later_chunks, int64_t *multi_unit_launches) {
  if (later_chunks) *later_chunks = g_later_chunks.load(std::memory_order_relaxed);
  if (multi_unit_launches)
    *multi_unit_launches = g_multi_unit_launches.load(std::memory_order_relaxed);
  return GDSP_OK;
}

int gdsp_fft(const double *x, double *out, int64_t n) {
  return host_batch(x, sizeof(cd), out, n, 1, false, gdsp::LOAD_COMPLEX);
}

int gdsp_ifft(const double *x, double *out, int64_t n) {
  return host_batch(x, sizeof(cd), out, n, 1, true, gdsp::LOAD_COMPLEX);
}

int gdsp_fft_real(const double *x, double *out, int64_t n) {
  return host_batch(x, sizeof(double), out, n, 1, false, gdsp::LOAD_REAL);
}

int gdsp_ifft_real(const double *x, double *out, int64_t n) {
  if (n < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (n == 0) return fail(GDSP_ERR_EMPTY, "IFFT of an empty slice (index out of range)");
  std::vector<double> c((size_t)(2 * n), 0.0);  // dsputils.ToComplex
  for (int64_t i = 0; i < n; ++i) c[(size_t)(2 * i)] = x[i];
  return host_batch(c.data(), sizeof(cd), out, n, 1, true, gdsp::LOAD_COMPLEX);
}

// Large batches are split over the library's device set (gdsp_set_devices;
// multi.hip): parallelism stays inside the call, as in radix2.go:89-151.
int gdsp_fft_batch(const double *x, double *out, int64_t n, int64_t batch, int inverse) {
  if (n > 0 && gdsp_api::multi_wanted((size_t)n * (size_t)batch * sizeof(cd), batch))
    return gdsp_api::fft_batch_multi(x, sizeof(cd), out, n, batch, inverse != 0,
                                     gdsp::LOAD_COMPLEX, nullptr, 0);
  return host_batch(x, sizeof(cd), out, n, batch, inverse != 0, gdsp::LOAD_COMPLEX);
}

int gdsp_fft_real_batch(const double *x, double *out, int64_t n, int64_t batch) {
  if (n > 0 && gdsp_api::multi_wanted((size_t)n * (size_t)batch * sizeof(double), batch))
    return gdsp_api::fft_batch_multi(x, sizeof(double), out, n, batch, false, gdsp::LOAD_REAL,
                                     nullptr, 0);
  return host_batch(x, sizeof(double), out, n, batch, false, gdsp::LOAD_REAL);
}

int gdsp_convolve(const double *x, const double *y, double *out, int64_t n) {
  // fft.Convolve, fft/fft.go:55-69: IFFT(FFT(x) * FFT(y))
  if (n < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (n == 0) return fail(GDSP_ERR_EMPTY, "IFFT of an empty slice (index out of range)");
  if (!x || !y || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  gdsp_plan *p = nullptr;
  STCHK(get_plan(n, &p));
  hipStream_t s = thread_stream(p->device);
  const size_t bytes = (size_t)n * sizeof(cd);
  DevBuf d;
  STCHK(d.alloc(3 * bytes, s, SLOT_IN));
  cd *dx = (cd *)d.p, *dy = dx + n, *dz = dy + n;
  STCHK(copy_h2d(dx, x, bytes, s));
  STCHK(copy_h2d(dy, y, bytes, s));
  STCHK(exec_plan(p, dx, dx, 2, false, gdsp::LOAD_COMPLEX, s));  // both rows at once
  HIPCHK(gdsp::launch_pointwise_mul(dx, dy, dz, n, s));
  STCHK(exec_plan(p, dz, dz, 1, true, gdsp::LOAD_COMPLEX, s));
  STCHK(copy_d2h(out, dz, bytes, s));
  return GDSP_OK;
}

// Batched fft.Convolve. The fused kernel (convolve.hip) serves the one-kernel
// powers of 2 from 2^kConvMinLog2 up; every other plan runs FFT, row
// multiply, IFFT.
static bool convolve_fused(const gdsp_plan *p) {
  return p->kind == KIND_LDS && p->log2n >= gdsp::kConvMinLog2 &&
         p->log2n <= gdsp::kMaxLdsLog2 && !(g_algo.load() & GDSP_ALGO_NO_FUSED_CONVOLVE);
}

// Argument checks shared by the host and device entries; *done: nothing to do
static int convolve_check(int64_t n, int64_t batch, int64_t y_rows, const void *x, const void *y,
                          const void *out, bool *done) {
  *done = false;
  if (n < 0 || batch < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (y_rows != 1 && y_rows != batch)
    return fail(GDSP_ERR_INVALID, "y_rows must be 1 or the batch");
  if (batch == 0) {
    *done = true;
    return GDSP_OK;
  }
  if (n == 0) return fail(GDSP_ERR_EMPTY, "IFFT of an empty slice (index out of range)");
  if (!x || !y || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  return GDSP_OK;
}

// work: y_rows * n, the spectrum of y
static int convolve_rows(const gdsp_plan *p, const cd *x, const cd *y, int64_t y_rows, cd *out,
                         int64_t batch, cd *work, hipStream_t s) {
  const int64_t n = p->n, ystride = y_rows == 1 ? 0 : n;
  STCHK(exec_plan(p, y, work, y_rows, false, gdsp::LOAD_COMPLEX, s));
  if (convolve_fused(p)) {
    HIPCHK(gdsp::launch_convolve_lds(p->log2n, x, out, batch, p->tw, work, ystride, s));
    return GDSP_OK;
  }
  STCHK(exec_plan(p, x, out, batch, false, gdsp::LOAD_COMPLEX, s));
  HIPCHK(gdsp::launch_pointwise_mul_rows(out, work, ystride, out, n, batch, s));
  return exec_plan(p, out, out, batch, true, gdsp::LOAD_COMPLEX, s);
}

int gdsp_convolve_fused(const gdsp_plan *plan) { return plan && convolve_fused(plan) ? 1 : 0; }

int gdsp_convolve_batch_device(const gdsp_plan *plan, const void *d_x, const void *d_y,
                               int64_t y_rows, void *d_out, int64_t batch, void *d_work,
                               void *stream) {
  if (!plan) return fail(GDSP_ERR_INVALID, "NULL plan");
  bool done = false;
  STCHK(convolve_check(plan->n, batch, y_rows, d_x, d_y, d_out, &done));
  if (done) return GDSP_OK;
  hipStream_t s = (hipStream_t)stream;
  DevBuf w;
  cd *work = (cd *)d_work;
  if (!work) {
    STCHK(w.alloc((size_t)y_rows * (size_t)plan->n * sizeof(cd), s, SLOT_CONV));
    work = (cd *)w.p;
  }
  return convolve_rows(plan, (const cd *)d_x, (const cd *)d_y, y_rows, (cd *)d_out, batch, work, s);
}

int gdsp_convolve_batch(const double *x, const double *y, double *out, int64_t n, int64_t batch,
                        int64_t y_rows) {
  bool done = false;
  STCHK(convolve_check(n, batch, y_rows, x, y, out, &done));
  if (done) return GDSP_OK;
  gdsp_plan *p = nullptr;
  STCHK(get_plan(n, &p));
  hipStream_t s = thread_stream(p->device);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const size_t xb = (size_t)batch * (size_t)n * sizeof(cd);
  const size_t yb = (size_t)y_rows * (size_t)n * sizeof(cd);
  DevBuf dx, dy;
  STCHK(dx.alloc(xb, s, SLOT_IN));
  STCHK(dy.alloc(2 * yb, s, SLOT_AUX));  // y, then its spectrum
  cd *py = (cd *)dy.p;
  STCHK(run_queued(s, [&]() -> int {
    STCHK(copy_h2d(dx.p, x, xb, s));
    STCHK(copy_h2d(py, y, yb, s));
    return convolve_rows(p, (const cd *)dx.p, py, y_rows, (cd *)dx.p, batch, py + y_rows * n, s);
  }));
  STCHK(copy_d2h(out, dx.p, xb, s));  // returns after the stream drained
  return GDSP_OK;
}

// ---- FIR filtering of real rows by overlap-save (fir.hip) --------------------
// The block length is host arithmetic on a committed table: per-F cost of the
// fused kernel, ms per 2^27 points through its transform pair (time x L / F
// per 2^27 samples), the median over the lines of that F in this kernel's own
// sweep (scripts/bench_fir.py, the cost_table of profiles/fir_batch.json;
// DESIGN.md §3). Nothing is timed when a call is made.
static constexpr int kFirMinLog2 = gdsp::kConvMinLog2, kFirMaxLog2 = gdsp::kMaxLdsLog2;
static constexpr int kFirComposedMaxLog2 = 20;
static const double kFirCost[kFirMaxLog2 - kFirMinLog2 + 1] = {0.5123, 0.4192, 0.4006, 0.4420,
                                                                0.4340, 0.4775, 0.6127};

// The block length of a call (0: the call fails) and whether F and m alone
// admit the fused kernel
static int64_t fir_block_for(int64_t m, int64_t block, bool *fused_range) {
  *fused_range = false;
  if (m <= 0 || block < 0) return 0;
  int64_t F = 0;
  if (block != 0) {
    if (!gdsp_api::is_pow2(block) || block < ((int64_t)1 << kFirMinLog2) ||
        block > ((int64_t)1 << kFirComposedMaxLog2) || block < 2 * m)
      return 0;
    F = block;
  } else if (m <= ((int64_t)1 << (kFirMaxLog2 - 1))) {
    double best = 0;
    for (int k = kFirMinLog2; k <= kFirMaxLog2; ++k) {
      const int64_t f = (int64_t)1 << k;
      if (f < 2 * m) continue;
      const double c = kFirCost[k - kFirMinLog2] * (double)f / (double)(f - m + 1);
      if (F == 0 || c < best) {
        F = f;
        best = c;
      }
    }
  } else {
    // beyond the fused kernel: the smallest power of 2 that is at least 4
    // times the halo of m - 1 samples (8193 taps run on 32768)
    F = (int64_t)1 << kFirComposedMaxLog2;
    if (4 * (m - 1) > F) return 0;
    while (F / 2 >= 4 * (m - 1)) F /= 2;
  }
  *fused_range = F <= ((int64_t)1 << kFirMaxLog2) && 2 * m <= F;
  return F;
}

// transforms per row and in all: two blocks of L = F - m + 1 outputs each
static void fir_geometry(int64_t F, int64_t m, int64_t channels, int64_t out_len, int64_t *tpr,
                         int64_t *total) {
  const int64_t L = F - m + 1, nb = (out_len + L - 1) / L;
  *tpr = (nb + 1) / 2;
  *total = channels * *tpr;
}

static bool fir_fused(int64_t F, bool fused_range, int64_t total) {
  return fused_range && !(g_algo.load() & GDSP_ALGO_NO_FUSED_FIR) &&
         gdsp::fir_ols_workgroups(gdsp_api::ilog2(F), total) <= 0x7fffffff;
}

// rows of the composed form's chunk: at most 256 MiB of complex rows
static int64_t fir_chunk_rows(int64_t F, int64_t total) {
  int64_t r = ((int64_t)1 << 24) / F;
  if (r < 1) r = 1;
  return r < total ? r : total;
}

// Argument checks shared by the host and device entries, in the order of the
// header's table; *done: nothing to do. No device call is made.
static int fir_check(const void *x, int64_t ldx, const void *h, int64_t h_rows, int64_t m,
                     int64_t channels, int64_t n, int full, int64_t block, const void *out,
                     int64_t ldo, int64_t *F, bool *fused_range, bool *done) {
  *done = false;
  *F = 0;
  if (m < 0 || n < 0 || channels < 0 || h_rows < 0 || block < 0)
    return fail(GDSP_ERR_INVALID, "negative size");
  if (full != 0 && full != 1) return fail(GDSP_ERR_INVALID, "full must be 0 or 1");
  if (h_rows != 1 && h_rows != channels)
    return fail(GDSP_ERR_INVALID, "h_rows must be 1 or the channels");
  if (block != 0 && (!gdsp_api::is_pow2(block) || block < ((int64_t)1 << kFirMinLog2) ||
                     block > ((int64_t)1 << kFirComposedMaxLog2) || block < 2 * m))
    return fail(GDSP_ERR_INVALID, "block must be a power of 2 in [256, 2^20] and at least 2 m");
  if (n > INT64_MAX / 4 || m > INT64_MAX / 4) return fail(GDSP_ERR_INVALID, "size overflow");
  const int64_t out_len = full ? n + m - 1 : n;
  if (channels > 1 && (ldx < n || ldo < out_len))
    return fail(GDSP_ERR_INVALID, "row stride below the row length");
  if (channels == 0) {
    *done = true;
    return GDSP_OK;
  }
  if (n == 0 || m == 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  *F = fir_block_for(m, block, fused_range);
  if (*F == 0) return fail(GDSP_ERR_UNSUPPORTED, "taps beyond the composed form's block lengths");
  if (!x || !h || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  return GDSP_OK;
}

// d_work: h_rows F complex128 (the taps' spectra), then in the composed form
// fir_chunk_rows(F, total) rows of F more
static int fir_rows(const double *d_x, int64_t ldx, const double *d_h, int64_t h_rows, int64_t m,
                    int64_t channels, int64_t n, int64_t out_len, int64_t F, bool fused_range,
                    double *d_out, int64_t ldo, cd *work, hipStream_t s) {
  gdsp_plan *p = nullptr;
  STCHK(get_plan(F, &p));
  int64_t tpr = 0, total = 0;
  fir_geometry(F, m, channels, out_len, &tpr, &total);
  const int64_t hstride = h_rows == 1 ? 0 : F;
  HIPCHK(gdsp::launch_fir_taps(d_h, h_rows, m, F, work, s));
  STCHK(exec_plan(p, work, work, h_rows, false, gdsp::LOAD_COMPLEX, s));
  // get_plan builds a power of 2 up to 2^14 as KIND_LDS under every flag set
  // (build_plan, plan.hip); the kind is checked because the kernel reads that
  // plan's twiddle table
  if (fir_fused(F, fused_range, total) && p->kind == KIND_LDS) {
    HIPCHK(gdsp::launch_fir_ols(p->log2n, d_x, ldx, d_out, ldo, channels, n, out_len, m, p->tw,
                                work, hstride, s));
    return GDSP_OK;
  }
  cd *buf = work + h_rows * F;
  const int64_t rows = fir_chunk_rows(F, total);
  for (int64_t g0 = 0; g0 < total; g0 += rows) {
    later_chunk(g0);
    const int64_t cnt = total - g0 < rows ? total - g0 : rows;
    HIPCHK(gdsp::launch_fir_gather(d_x, ldx, g0, cnt, tpr, n, m, F, buf, s));
    STCHK(exec_plan(p, buf, buf, cnt, false, gdsp::LOAD_COMPLEX, s));
    if (h_rows == 1) {
      HIPCHK(gdsp::launch_pointwise_mul_rows(buf, work, 0, buf, F, cnt, s));
    } else {
      // one multiply per channel's run of rows in the chunk
      for (int64_t g = g0; g < g0 + cnt;) {
        const int64_t c = g / tpr, end = (c + 1) * tpr < g0 + cnt ? (c + 1) * tpr : g0 + cnt;
        cd *run = buf + (g - g0) * F;
        HIPCHK(gdsp::launch_pointwise_mul_rows(run, work + c * F, 0, run, F, end - g, s));
        g = end;
      }
    }
    STCHK(exec_plan(p, buf, buf, cnt, true, gdsp::LOAD_COMPLEX, s));
    HIPCHK(gdsp::launch_fir_scatter(buf, g0, cnt, tpr, out_len, m, F, d_out, ldo, s));
  }
  return GDSP_OK;
}

static size_t fir_work_bytes(int64_t F, int64_t m, int64_t h_rows, int64_t channels,
                             int64_t out_len, bool fused_range) {
  int64_t tpr = 0, total = 0;
  fir_geometry(F, m, channels, out_len, &tpr, &total);
  const int64_t rows = h_rows + (fir_fused(F, fused_range, total) ? 0 : fir_chunk_rows(F, total));
  return (size_t)rows * (size_t)F * sizeof(cd);
}

int64_t gdsp_fir_block(int64_t m, int64_t block, int *fused) {
  bool fr = false;
  const int64_t F = fir_block_for(m, block, &fr);
  if (fused) *fused = F != 0 && fr && !(g_algo.load() & GDSP_ALGO_NO_FUSED_FIR) ? 1 : 0;
  return F;
}

int gdsp_fir_batch_device(const void *d_x, int64_t ldx, const void *d_h, int64_t h_rows,
                          int64_t m, int64_t channels, int64_t n, int full, int64_t block,
                          void *d_out, int64_t ldo, void *d_work, void *stream) {
  int64_t F = 0;
  bool fr = false, done = false;
  STCHK(fir_check(d_x, ldx, d_h, h_rows, m, channels, n, full, block, d_out, ldo, &F, &fr, &done));
  if (done) return GDSP_OK;
  const int64_t out_len = full ? n + m - 1 : n;
  // a block's halo is another workgroup's output range: no overlap at all
  const uintptr_t xa = (uintptr_t)d_x, oa = (uintptr_t)d_out;
  const uintptr_t xe = xa + ((uintptr_t)(channels - 1) * (uintptr_t)ldx + (uintptr_t)n) * 8;
  const uintptr_t oe = oa + ((uintptr_t)(channels - 1) * (uintptr_t)ldo + (uintptr_t)out_len) * 8;
  if (xa < oe && oa < xe) return fail(GDSP_ERR_INVALID, "d_out overlaps d_x");
  hipStream_t s = (hipStream_t)stream;
  DevBuf w;
  cd *work = (cd *)d_work;
  if (!work) {
    STCHK(w.alloc(fir_work_bytes(F, m, h_rows, channels, out_len, fr), s, SLOT_FIR));
    work = (cd *)w.p;
  }
  return fir_rows((const double *)d_x, channels > 1 ? ldx : n, (const double *)d_h, h_rows, m,
                  channels, n, out_len, F, fr, (double *)d_out, channels > 1 ? ldo : out_len, work,
                  s);
}

int gdsp_fir_batch(const double *x, int64_t ldx, const double *h, int64_t h_rows, int64_t m,
                   int64_t channels, int64_t n, int full, int64_t block, double *out,
                   int64_t ldo) {
  int64_t F = 0;
  bool fr = false, done = false;
  STCHK(fir_check(x, ldx, h, h_rows, m, channels, n, full, block, out, ldo, &F, &fr, &done));
  if (done) return GDSP_OK;
  const int64_t out_len = full ? n + m - 1 : n;
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  DevBuf dx, dh, dout, dw;
  STCHK(dx.alloc((size_t)channels * (size_t)n * sizeof(double), s, SLOT_IN));
  STCHK(dh.alloc((size_t)h_rows * (size_t)m * sizeof(double), s, SLOT_FIR_H));
  STCHK(dout.alloc((size_t)channels * (size_t)out_len * sizeof(double), s, SLOT_FIR_OUT));
  STCHK(dw.alloc(fir_work_bytes(F, m, h_rows, channels, out_len, fr), s, SLOT_FIR));
  double *px = (double *)dx.p, *po = (double *)dout.p;
  STCHK(run_queued(s, [&]() -> int {
    STCHK(stage_rows(px, x, channels, n, ldx, n, s));
    STCHK(copy_h2d(dh.p, h, (size_t)h_rows * (size_t)m * sizeof(double), s));
    return fir_rows(px, n, (const double *)dh.p, h_rows, m, channels, n, out_len, F, fr, po,
                    out_len, (cd *)dw.p, s);
  }));
  // every sample left the caller's memory before the first result lands in
  // it, so out may alias x
  return unstage_rows(out, po, channels, out_len, ldo, s);
}

// ---- polyphase resampling of real rows (upfirdn.hip) --------------------------
static constexpr int64_t kUpfirdnMaxRate = 65536, kUpfirdnMaxTaps = (int64_t)1 << 24;
// outputs of one chunk of the host entry (all rows together)
static constexpr int64_t UPFIRDN_CHUNK_ELEMS = (int64_t)1 << 25;

// (n - 1) up + m, or -1 where int64 does not hold it (n, m, up >= 1)
static int64_t upfirdn_full_len(int64_t n, int64_t m, int64_t up) {
  int64_t v = 0;
  if (__builtin_mul_overflow(n - 1, up, &v) || __builtin_add_overflow(v, m, &v)) return -1;
  return v;
}

static bool upfirdn_supported(int64_t n, int64_t m, int64_t up, int64_t down) {
  return up <= kUpfirdnMaxRate && down <= kUpfirdnMaxRate && m <= kUpfirdnMaxTaps &&
         upfirdn_full_len(n, m, up) >= 0;
}

int64_t gdsp_upfirdn_length(int64_t n, int64_t m, int64_t up, int64_t down) {
  if (n < 0 || m < 0 || up < 1 || down < 1) return -1;
  if (n == 0 || m == 0) return 0;
  if (!upfirdn_supported(n, m, up, down)) return -1;
  return (upfirdn_full_len(n, m, up) - 1) / down + 1;
}

int gdsp_upfirdn_fused(int64_t m, int64_t up, int64_t down) {
  return !(g_algo.load() & GDSP_ALGO_NO_FUSED_UPFIRDN) && gdsp::upfirdn_geometry(m, up, down).fits;
}

// Argument checks shared by the host and device entries, in the order of the
// header's table, up to the NULL pointers; *done: nothing to do; *out_end: the
// range's end with -1 resolved. No device call is made.
static int upfirdn_check(const void *x, int64_t ldx, const void *h, int64_t m, int64_t up,
                         int64_t down, int64_t channels, int64_t n, int64_t out_begin,
                         int64_t *out_end, const void *out, int64_t ldo, bool *done) {
  *done = false;
  if (m < 0 || n < 0 || channels < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (up < 1 || down < 1) return fail(GDSP_ERR_INVALID, "up and down must be at least 1");
  // L, saturated where int64 does not hold (n - 1) up + m (refused below)
  int64_t L = 0;
  if (n > 0 && m > 0) {
    const int64_t full = upfirdn_full_len(n, m, up);
    L = full < 0 ? INT64_MAX : (full - 1) / down + 1;
  }
  if (*out_end == -1) *out_end = L;
  if (out_begin < 0 || out_begin > *out_end || *out_end > L)
    return fail(GDSP_ERR_INVALID, "output range not within [0, L]");
  if (channels > 1 && (ldx < n || ldo < *out_end - out_begin))
    return fail(GDSP_ERR_INVALID, "row stride below the row length");
  if (channels == 0) {
    *done = true;
    return GDSP_OK;
  }
  if (n == 0 || m == 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  if (!upfirdn_supported(n, m, up, down))
    return fail(GDSP_ERR_UNSUPPORTED, "up or down above 65536, more than 2^24 taps, or a length "
                                      "beyond int64");
  if (!x || !h || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  return GDSP_OK;
}

// Outputs [out_begin, out_end) of every row; the rows at d_x hold samples
// [x_lo, x_hi) of the signal. work: up ceil(m / up) doubles.
static int upfirdn_rows(const double *d_x, int64_t ldx, int64_t x_lo, int64_t x_hi,
                        const double *d_h, int64_t m, int64_t up, int64_t down, int64_t channels,
                        int64_t out_begin, int64_t out_end, double *d_out, int64_t ldo,
                        double *work, hipStream_t s) {
  HIPCHK(gdsp::launch_upfirdn_taps(d_h, m, up, work, s));
  const gdsp::UpfirdnGeo g = gdsp::upfirdn_geometry(m, up, down);
  if (g.fits && !(g_algo.load() & GDSP_ALGO_NO_FUSED_UPFIRDN)) {
    HIPCHK(gdsp::launch_upfirdn_poly(g, d_x, ldx, x_lo, x_hi, work, up, down, channels, out_begin,
                                     out_end, d_out, ldo, s));
  } else {
    HIPCHK(gdsp::launch_upfirdn_plain(d_x, ldx, x_lo, x_hi, work, m, up, down, channels,
                                      out_begin, out_end, d_out, ldo, s));
  }
  return GDSP_OK;
}

static size_t upfirdn_work_bytes(int64_t m, int64_t up) {
  return (size_t)(up * ((m + up - 1) / up)) * sizeof(double);
}

int gdsp_upfirdn_batch_device(const void *d_x, int64_t ldx, const void *d_h, int64_t m,
                              int64_t up, int64_t down, int64_t channels, int64_t n,
                              int64_t out_begin, int64_t out_end, void *d_out, int64_t ldo,
                              void *d_work, void *stream) {
  bool done = false;
  STCHK(upfirdn_check(d_x, ldx, d_h, m, up, down, channels, n, out_begin, &out_end, d_out, ldo,
                      &done));
  if (done) return GDSP_OK;
  const int64_t cnt = out_end - out_begin;
  // a tile's halo is read while another workgroup stores: no overlap at all
  const uintptr_t xa = (uintptr_t)d_x, oa = (uintptr_t)d_out;
  const uintptr_t xe = xa + ((uintptr_t)(channels - 1) * (uintptr_t)ldx + (uintptr_t)n) * 8;
  const uintptr_t oe = oa + ((uintptr_t)(channels - 1) * (uintptr_t)ldo + (uintptr_t)cnt) * 8;
  if (xa < oe && oa < xe) return fail(GDSP_ERR_INVALID, "d_out overlaps d_x");
  if (cnt == 0) return GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = (hipStream_t)stream;
  DevBuf w;
  double *work = (double *)d_work;
  if (!work) {
    STCHK(w.alloc(upfirdn_work_bytes(m, up), s, SLOT_UF));
    work = (double *)w.p;
  }
  return upfirdn_rows((const double *)d_x, channels > 1 ? ldx : n, 0, n, (const double *)d_h, m,
                      up, down, channels, out_begin, out_end, (double *)d_out,
                      channels > 1 ? ldo : cnt, work, s);
}

int gdsp_upfirdn_batch(const double *x, int64_t ldx, const double *h, int64_t m, int64_t up,
                       int64_t down, int64_t channels, int64_t n, int64_t out_begin,
                       int64_t out_end, double *out, int64_t ldo) {
  bool done = false;
  STCHK(upfirdn_check(x, ldx, h, m, up, down, channels, n, out_begin, &out_end, out, ldo, &done));
  if (done || out_end == out_begin) return GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const int64_t T = (m + up - 1) / up;
  int64_t rng = UPFIRDN_CHUNK_ELEMS / channels;  // outputs of a row per chunk
  if (rng < 1) rng = 1;
  if (channels == 1) ldx = n, ldo = out_end - out_begin;
  DevBuf dx, dh, dout, dw;
  STCHK(dh.alloc((size_t)m * sizeof(double), s, SLOT_UF_H));
  STCHK(dw.alloc(upfirdn_work_bytes(m, up), s, SLOT_UF));
  for (int64_t jb = out_begin; jb < out_end; jb += rng) {
    later_chunk(jb - out_begin);
    const int64_t je = out_end - jb < rng ? out_end : jb + rng, cnt = je - jb;
    // the samples the chunk reads: [i0(jb) - (T - 1), i0(je - 1)] within the row
    int64_t ib = jb * down / up - (T - 1), ie = (je - 1) * down / up + 1;
    if (ib < 0) ib = 0;
    if (ie > n) ie = n;
    const int64_t len = ie - ib;
    STCHK(dx.alloc((size_t)channels * (size_t)len * sizeof(double), s, SLOT_IN));
    STCHK(dout.alloc((size_t)channels * (size_t)cnt * sizeof(double), s, SLOT_UF_OUT));
    double *px = (double *)dx.p, *po = (double *)dout.p;
    STCHK(run_queued(s, [&]() -> int {
      STCHK(stage_rows(px, x + ib, channels, len, ldx, len, s));
      if (jb == out_begin) STCHK(copy_h2d(dh.p, h, (size_t)m * sizeof(double), s));
      return upfirdn_rows(px, len, ib, ie, (const double *)dh.p, m, up, down, channels, jb, je, po,
                          cnt, (double *)dw.p, s);
    }));
    // returns after the stream drained: the next chunk may reuse the buffers
    STCHK(unstage_rows(out + (jb - out_begin), po, channels, cnt, ldo, s));
  }
  return GDSP_OK;
}

// ---- the analytic signal of real rows (hilbert.hip) ---------------------------
// samples of one chunk of the host entry and of the composed form (all rows
// together)
static constexpr int64_t HILBERT_CHUNK_ELEMS = (int64_t)1 << 24;

static bool hilbert_fused(int64_t N) {
  return gdsp::hilbert_lds_applies(N) && !(g_algo.load() & GDSP_ALGO_NO_FUSED_HILBERT);
}

int gdsp_hilbert_fused(int64_t nfft) { return nfft > 0 && hilbert_fused(nfft) ? 1 : 0; }

// rows of the composed form's chunk
static int64_t hilbert_chunk_rows(int64_t N, int64_t rows) {
  int64_t r = HILBERT_CHUNK_ELEMS / N;
  if (r < 1) r = 1;
  return r < rows ? r : rows;
}

// Argument checks shared by the host and device entries, in the order of the
// header's table, up to the NULL pointers; *done: nothing to do; *N: the
// transform length. No device call is made.
static int hilbert_check(const void *x, int64_t ldx, int64_t rows, int64_t n, int64_t nfft,
                         int kind, const void *out, int64_t ldo, int64_t *N, bool *done) {
  *done = false;
  if (rows < 0 || n < 0 || nfft < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (kind < GDSP_HILBERT_ANALYTIC || kind > GDSP_HILBERT_ENVELOPE)
    return fail(GDSP_ERR_INVALID, "kind must be 0, 1 or 2");
  *N = nfft == 0 ? n : nfft;
  if (rows > 1 && (ldx < n || ldo < *N))
    return fail(GDSP_ERR_INVALID, "row stride below the row length");
  if (rows == 0) {
    *done = true;
    return GDSP_OK;
  }
  if (n == 0 || *N == 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  if (!x || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  return GDSP_OK;
}

// work (NULL: the workspace pool): nothing in the fused form; composed,
// hilbert_chunk_rows(N, rows) rows of N complex128, then as many of N float64
static int hilbert_rows(const double *d_x, int64_t ldx, int64_t rows, int64_t n, int64_t N,
                        int kind, void *d_out, int64_t ldo, void *work, hipStream_t s) {
  gdsp_plan *p = nullptr;
  STCHK(get_plan(N, &p));
  // a power of 2 up to 2^14 is KIND_LDS under every flag set (fir_rows); the
  // kind is checked because the kernel reads that plan's twiddle table
  if (hilbert_fused(N) && p->kind == KIND_LDS) {
    HIPCHK(gdsp::launch_hilbert_lds(p->log2n, kind, d_x, ldx, rows, n, d_out, ldo, p->tw, s));
    return GDSP_OK;
  }
  const int64_t cr = hilbert_chunk_rows(N, rows);
  DevBuf w;
  if (!work) {
    STCHK(w.alloc((size_t)cr * (size_t)N * (sizeof(cd) + sizeof(double)), s, SLOT_HB));
    work = w.p;
  }
  cd *spec = (cd *)work;
  double *buf = (double *)(spec + cr * N);
  for (int64_t r0 = 0; r0 < rows; r0 += cr) {
    later_chunk(r0);
    const int64_t cnt = rows - r0 < cr ? rows - r0 : cr;
    if (N == 1) {  // h = 0
      HIPCHK(gdsp::launch_hilbert_store(kind, d_x, ldx, r0, cnt, n, N, nullptr, d_out, ldo, s));
      continue;
    }
    HIPCHK(gdsp::launch_hilbert_gather(d_x, ldx, r0, cnt, n, N, buf, s));
    STCHK(exec_plan(p, buf, spec, cnt, false, gdsp::LOAD_REAL, s));
    HIPCHK(gdsp::launch_hilbert_mask(spec, cnt, N, s));
    STCHK(exec_plan(p, spec, spec, cnt, true, gdsp::LOAD_COMPLEX, s));
    HIPCHK(gdsp::launch_hilbert_store(kind, d_x, ldx, r0, cnt, n, N, spec, d_out, ldo, s));
  }
  return GDSP_OK;
}

int gdsp_hilbert_batch_device(const void *d_x, int64_t ldx, int64_t rows, int64_t n,
                              int64_t nfft, int kind, void *d_out, int64_t ldo, void *d_work,
                              void *stream) {
  int64_t N = 0;
  bool done = false;
  STCHK(hilbert_check(d_x, ldx, rows, n, nfft, kind, d_out, ldo, &N, &done));
  if (done) return GDSP_OK;
  if (rows == 1) ldx = n, ldo = N;
  // the kinds that store the input read it again while other workgroups store
  const uintptr_t esz = kind == GDSP_HILBERT_ANALYTIC ? sizeof(cd) : sizeof(double);
  const uintptr_t xa = (uintptr_t)d_x, oa = (uintptr_t)d_out;
  const uintptr_t xe = xa + ((uintptr_t)(rows - 1) * (uintptr_t)ldx + (uintptr_t)n) * 8;
  const uintptr_t oe = oa + ((uintptr_t)(rows - 1) * (uintptr_t)ldo + (uintptr_t)N) * esz;
  if (xa < oe && oa < xe) return fail(GDSP_ERR_INVALID, "d_out overlaps d_x");
  return hilbert_rows((const double *)d_x, ldx, rows, n, N, kind, d_out, ldo, d_work,
                      (hipStream_t)stream);
}

int gdsp_hilbert_batch(const double *x, int64_t ldx, int64_t rows, int64_t n, int64_t nfft,
                       int kind, double *out, int64_t ldo) {
  int64_t N = 0;
  bool done = false;
  STCHK(hilbert_check(x, ldx, rows, n, nfft, kind, out, ldo, &N, &done));
  if (done) return GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const int64_t nn = n < N ? n : N;                         // the samples a row gives
  const int64_t od = kind == GDSP_HILBERT_ANALYTIC ? 2 : 1;  // doubles per output element
  if (rows == 1) ldx = n, ldo = N;
  // row ranges that start at even rows
  int64_t rng = (HILBERT_CHUNK_ELEMS / N) & ~(int64_t)1;
  if (rng < 2) rng = 2;
  DevBuf dx, dout;
  for (int64_t r0 = 0; r0 < rows; r0 += rng) {
    later_chunk(r0);
    const int64_t cnt = rows - r0 < rng ? rows - r0 : rng;
    STCHK(dx.alloc((size_t)cnt * (size_t)nn * sizeof(double), s, SLOT_IN));
    STCHK(dout.alloc((size_t)cnt * (size_t)N * (size_t)od * sizeof(double), s, SLOT_HB_OUT));
    double *px = (double *)dx.p, *po = (double *)dout.p;
    STCHK(run_queued(s, [&]() -> int {
      STCHK(stage_rows(px, x + r0 * ldx, cnt, nn, ldx, nn, s));
      return hilbert_rows(px, nn, cnt, nn, N, kind, po, N, nullptr, s);
    }));
    // returns after the stream drained: the next chunk may reuse the buffers
    STCHK(unstage_rows(out + r0 * ldo * od, po, cnt, N * od, ldo * od, s));
  }
  return GDSP_OK;
}

// ---- recursive filtering of real rows (sosfilt.hip) ---------------------------
// samples of one chunk of the host entries (all rows together)
static constexpr int64_t SOSFILT_CHUNK_ELEMS = (int64_t)1 << 25;

static bool sos_coeffs_ok(const double *sos, int64_t S) {
  for (int64_t i = 0; i < 6 * S; ++i)
    if (!std::isfinite(sos[i])) return false;
  for (int64_t s = 0; s < S; ++s)
    if (sos[6 * s + 3] != 1.0) return false;
  return true;
}

int gdsp_sosfilt_fused(const double *sos, int64_t S) {
  if (!sos || S < 1 || S > gdsp::kSosMaxFused || (g_algo.load() & GDSP_ALGO_NO_FUSED_SOSFILT))
    return 0;
  if (!sos_coeffs_ok(sos, S)) return 0;
  for (int64_t s = 0; s < S; ++s) {
    const double a1 = sos[6 * s + 4], a2 = sos[6 * s + 5];
    if (!(fabs(a2) < 1.0 && fabs(a1) < 1.0 + a2)) return 0;
  }
  return 1;
}

int64_t gdsp_sosfilt_granule(int64_t S) {
  return S >= 1 && S <= gdsp::kSosMaxSections ? gdsp::kSosTile : 0;
}

int gdsp_sosfilt_zi(const double *sos, int64_t S, double *zi) {
  if (S < 0) return fail(GDSP_ERR_INVALID, "negative size");
  if (S == 0) return GDSP_OK;
  if (!sos || !zi) return fail(GDSP_ERR_INVALID, "NULL pointer");
  if (!sos_coeffs_ok(sos, S)) return fail(GDSP_ERR_INVALID, "a0 must be 1, coefficients finite");
  long double scale = 1.0L;
  for (int64_t s = 0; s < S; ++s) {
    const long double b0 = sos[6 * s], b1 = sos[6 * s + 1], b2 = sos[6 * s + 2],
                      a1 = sos[6 * s + 4], a2 = sos[6 * s + 5];
    const long double den = 1.0L + a1 + a2;
    if (den == 0.0L) return fail(GDSP_ERR_INVALID, "a section with a pole at z = 1");
    const long double gain = (b0 + b1 + b2) / den;  // the step response settles at it
    const long double z1 = b2 - a2 * gain, z0 = b1 - a1 * gain + z1;
    zi[2 * s] = (double)(scale * z0);
    zi[2 * s + 1] = (double)(scale * z1);
    scale *= gain;
  }
  return GDSP_OK;
}

int64_t gdsp_sosfiltfilt_padlen(const double *sos, int64_t S) {
  if (!sos || S < 1 || S > gdsp::kSosMaxSections) return -1;
  int64_t zb = 0, za = 0;
  for (int64_t s = 0; s < S; ++s) {
    zb += sos[6 * s + 2] == 0.0;
    za += sos[6 * s + 5] == 0.0;
  }
  return 3 * (2 * S + 1 - (zb < za ? zb : za));
}

// doubles of device scratch a launch over rows of n samples takes: the tables,
// then per row the end and entry states of its tiles
static int64_t sos_work_doubles(int64_t S, int64_t channels, int64_t n) {
  const int64_t T = (n + gdsp::kSosTile - 1) / gdsp::kSosTile;
  return gdsp::kSosTableDoubles + channels * (2 * T + 1) * 2 * S;
}

int64_t gdsp_sosfilt_work_doubles(int64_t S, int64_t channels, int64_t n) {
  if (S < 1 || S > gdsp::kSosMaxSections || channels < 0 || n < 0) return -1;
  return sos_work_doubles(S, channels, n);
}

int64_t gdsp_sosfiltfilt_work_doubles(int64_t S, int64_t channels, int64_t n, int64_t padlen) {
  if (S < 1 || S > gdsp::kSosMaxSections || channels < 0 || n < 0 || padlen < 0) return -1;
  const int64_t L = n + 2 * padlen;
  return sos_work_doubles(S, channels, L) + 2 * S + channels * 2 * S + channels * L;
}

namespace {

typedef long double ld_t;

// c = a b, square matrices of order m
void sos_matmul(const ld_t *a, const ld_t *b, ld_t *c, int m) {
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      ld_t acc = 0;
      for (int k = 0; k < m; ++k) acc += a[i * m + k] * b[k * m + j];
      c[i * m + j] = acc;
    }
}

// The time-parallel form's tables (launch.hpp), in long double, rounded once.
void sos_build_tables(const double *sos, int S, double *t) {
  using namespace gdsp;
  for (int i = 0; i < kSosTableDoubles; ++i) t[i] = 0.0;
  for (int s = 0; s < S; ++s) {
    double *ts = t + s * kSosSecDoubles;
    const double *q = sos + 6 * s;
    ts[0] = q[0], ts[1] = q[1], ts[2] = q[2], ts[3] = q[4], ts[4] = q[5];
    // zero input: y = z0; z0' = -a1 z0 + z1; z1' = -a2 z0
    const ld_t A[4] = {-(ld_t)q[4], 1, -(ld_t)q[5], 0};
    ld_t P[4] = {1, 0, 0, 1}, N[4];
    for (int i = 0; i < kSosE; ++i) {  // P = A^i: its first row is output i
      ts[8 + 2 * i] = (double)P[0], ts[8 + 2 * i + 1] = (double)P[1];
      sos_matmul(A, P, N, 2);
      for (int e = 0; e < 4; ++e) P[e] = N[e];
    }
    for (int k = 0; k < 7; ++k) {  // P = M^(2^k)
      for (int e = 0; e < 4; ++e) ts[8 + 2 * kSosE + 4 * k + e] = (double)P[e];
      sos_matmul(P, P, N, 2);
      for (int e = 0; e < 4; ++e) P[e] = N[e];
    }
  }
  // one step of the whole cascade on zero input, column by column
  const int m = 2 * S;
  std::vector<ld_t> A((size_t)m * m, 0), B((size_t)m * m);
  for (int j = 0; j < m; ++j) {
    ld_t y = 0;  // the cascade's input
    for (int s = 0; s < S; ++s) {
      const double *q = sos + 6 * s;
      const ld_t z0 = j == 2 * s, z1 = j == 2 * s + 1, xin = y;
      y = (ld_t)q[0] * xin + z0;
      A[(2 * s) * m + j] = (ld_t)q[1] * xin - (ld_t)q[4] * y + z1;
      A[(2 * s + 1) * m + j] = (ld_t)q[2] * xin - (ld_t)q[5] * y;
    }
  }
  for (int64_t len = 1; len < kSosTile; len *= 2) {
    sos_matmul(A.data(), A.data(), B.data(), m);
    A.swap(B);
  }
  for (int i = 0; i < m * m; ++i) t[kSosPhiOffset + i] = (double)A[i];
}

// The tables of the last filter a thread used: building them is host work of
// a twelve-fold squaring of a 2 S x 2 S matrix.
const double *sos_tables_cached(const double *sos, int S) {
  thread_local int cs = 0;
  thread_local double key[6 * gdsp::kSosMaxFused], tab[gdsp::kSosTableDoubles];
  if (cs != S || memcmp(key, sos, (size_t)S * 6 * sizeof(double)) != 0) {
    sos_build_tables(sos, S, tab);
    memcpy(key, sos, (size_t)S * 6 * sizeof(double));
    cs = S;
  }
  return tab;
}

// The filter's tables into work (once per call), then launches over them.
int sos_upload(const double *sos, int S, bool fused, double *work, hipStream_t s) {
  if (fused) {
    HIPCHK(gdsp::launch_sos_tables(sos_tables_cached(sos, S), gdsp::kSosTableDoubles, work, s));
  } else {
    double coef[5 * gdsp::kSosMaxSections];
    for (int i = 0; i < S; ++i) {
      const double *q = sos + 6 * i;
      double *c = coef + 5 * i;
      c[0] = q[0], c[1] = q[1], c[2] = q[2], c[3] = q[4], c[4] = q[5];
    }
    HIPCHK(gdsp::launch_sos_tables(coef, 5 * S, work, s));
  }
  return GDSP_OK;
}

int sos_run(const gdsp::SosIo &io, int S, bool fused, int64_t channels, const double *d_zi,
            double *d_zf, double *work, hipStream_t s) {
  if (fused) {
    HIPCHK(gdsp::launch_sos_tiles(io, work, S, channels, d_zi, d_zf,
                                  work + gdsp::kSosTableDoubles, s));
  } else {
    HIPCHK(gdsp::launch_sos_plain(io, work, S, channels, d_zi, d_zf, s));
  }
  return GDSP_OK;
}

gdsp::SosIo sos_io_plain(const double *src, int64_t lds, double *dst, int64_t ldd, int64_t n) {
  gdsp::SosIo io = {};
  io.src = src, io.lds = lds, io.dst = dst, io.ldd = ldd, io.n = n, io.nx = n;
  io.mode = gdsp::SOS_IO_PLAIN;
  return io;
}

// Argument checks shared by the host and device entries, in the order of the
// header's table; *done: nothing to do. padlen: -2 for sosfilt; else
// sosfiltfilt's (-1: the default), resolved into *pl. No device call is made.
int sos_check(const void *x, int64_t ldx, const double *sos, int64_t S, int64_t padlen,
              int64_t channels, int64_t n, const void *out, int64_t ldo, int64_t *pl,
              bool *done) {
  *done = false;
  if (S < 0 || channels < 0 || n < 0 || padlen < -2)
    return fail(GDSP_ERR_INVALID, "negative size");
  if (channels > 1 && (ldx < n || ldo < n))
    return fail(GDSP_ERR_INVALID, "row stride below the row length");
  if (channels == 0) {
    *done = true;
    return GDSP_OK;
  }
  if (n == 0 || S == 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  if (S > gdsp::kSosMaxSections) return fail(GDSP_ERR_UNSUPPORTED, "more than 64 sections");
  if (!x || !sos || !out) return fail(GDSP_ERR_INVALID, "NULL pointer");
  if (!sos_coeffs_ok(sos, S))
    return fail(GDSP_ERR_INVALID, "a0 must be 1 and every coefficient finite");
  if (padlen != -2) {
    *pl = padlen == -1 ? gdsp_sosfiltfilt_padlen(sos, S) : padlen;
    if (n <= *pl) return fail(GDSP_ERR_INVALID, "the rows must be longer than padlen");
    if (*pl > ((int64_t)1 << 40) || n > INT64_MAX - 2 * *pl)
      return fail(GDSP_ERR_INVALID, "padlen out of range");
  }
  return GDSP_OK;
}

bool sos_overlap(const void *a, int64_t lda, const void *b, int64_t ldb, int64_t rows, int64_t n) {
  const uintptr_t xa = (uintptr_t)a, oa = (uintptr_t)b;
  const uintptr_t xe = xa + ((uintptr_t)(rows - 1) * (uintptr_t)lda + (uintptr_t)n) * 8;
  const uintptr_t oe = oa + ((uintptr_t)(rows - 1) * (uintptr_t)ldb + (uintptr_t)n) * 8;
  return xa < oe && oa < xe;
}

// samples of a row per chunk of the host entries: a multiple of the granule
int64_t sos_chunk_len(int64_t S, int64_t channels) {
  const int64_t G = gdsp_sosfilt_granule(S);
  int64_t rng = SOSFILT_CHUNK_ELEMS / channels / G * G;
  return rng < G ? G : rng;
}

}  // namespace

int gdsp_sosfilt_batch_device(const void *d_x, int64_t ldx, const double *sos, int64_t S,
                              const void *d_zi, int64_t channels, int64_t n, void *d_out,
                              int64_t ldo, void *d_zf, void *d_work, void *stream) {
  bool done = false;
  int64_t pl = 0;
  STCHK(sos_check(d_x, ldx, sos, S, -2, channels, n, d_out, ldo, &pl, &done));
  if (done) return GDSP_OK;
  if (channels == 1) ldx = ldo = n;
  // pass 3 reads a tile before it stores it, and tiles do not share samples:
  // out may be x itself, and nothing else that overlaps it
  if (!(d_x == d_out && ldx == ldo) && sos_overlap(d_x, ldx, d_out, ldo, channels, n))
    return fail(GDSP_ERR_INVALID, "d_out overlaps d_x without being d_x");
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = (hipStream_t)stream;
  DevBuf w;
  double *work = (double *)d_work;
  if (!work) {
    STCHK(w.alloc((size_t)sos_work_doubles(S, channels, n) * sizeof(double), s, SLOT_SOS));
    work = (double *)w.p;
  }
  const bool fused = gdsp_sosfilt_fused(sos, S) != 0;
  STCHK(sos_upload(sos, (int)S, fused, work, s));
  return sos_run(sos_io_plain((const double *)d_x, ldx, (double *)d_out, ldo, n), (int)S, fused,
                 channels, (const double *)d_zi, (double *)d_zf, work, s);
}

// Host rows through the device in chunks of time, in place on the staged
// chunk, the state carried in two device buffers that swap. make(v0, len, dst):
// the chunk's samples as dense host rows, or NULL where the caller's rows
// x + v0 serve; take(v0, len, src): dense device rows back to the caller.
typedef std::function<int(int64_t, int64_t, double *)> SosStage;
typedef std::function<int(int64_t, int64_t, const double *)> SosTake;
static int sos_host_chunks(const double *sos, int64_t S, int64_t channels, int64_t n,
                           const double *zi_host, double *zf_host, const SosStage &stage,
                           const SosTake &take, hipStream_t s) {
  const int64_t rng = sos_chunk_len(S, channels);
  const int64_t first = n < rng ? n : rng;
  const size_t zbytes = (size_t)channels * 2 * (size_t)S * sizeof(double);
  DevBuf dx, dz, dw;
  STCHK(dx.alloc((size_t)channels * (size_t)first * sizeof(double), s, SLOT_IN));
  STCHK(dz.alloc(2 * zbytes, s, SLOT_SOS_Z));
  STCHK(dw.alloc((size_t)sos_work_doubles(S, channels, first) * sizeof(double), s, SLOT_SOS));
  double *px = (double *)dx.p, *za = (double *)dz.p, *zb = za + channels * 2 * S;
  const bool fused = gdsp_sosfilt_fused(sos, S) != 0;
  for (int64_t v0 = 0; v0 < n; v0 += rng) {
    later_chunk(v0);
    const int64_t len = n - v0 < rng ? n - v0 : rng;
    const bool lastc = v0 + len == n;
    STCHK(run_queued(s, [&]() -> int {
      STCHK(stage(v0, len, px));
      if (v0 == 0) {
        STCHK(sos_upload(sos, (int)S, fused, (double *)dw.p, s));
        if (zi_host) STCHK(copy_h2d(za, zi_host, zbytes, s));
      }
      return sos_run(sos_io_plain(px, len, px, len, len), (int)S, fused, channels,
                     (v0 == 0 && !zi_host) ? nullptr : za, (lastc && !zf_host) ? nullptr : zb,
                     (double *)dw.p, s);
    }));
    // returns after the stream drained: the next chunk may reuse the buffers
    STCHK(take(v0, len, px));
    std::swap(za, zb);
  }
  if (zf_host) STCHK(copy_d2h(zf_host, za, zbytes, s));
  return GDSP_OK;
}

int gdsp_sosfilt_batch(const double *x, int64_t ldx, const double *sos, int64_t S,
                       const double *zi, int64_t channels, int64_t n, double *out, int64_t ldo,
                       double *zf) {
  bool done = false;
  int64_t pl = 0;
  STCHK(sos_check(x, ldx, sos, S, -2, channels, n, out, ldo, &pl, &done));
  if (done) return GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  if (channels == 1) ldx = ldo = n;
  return sos_host_chunks(
      sos, S, channels, n, zi, zf,
      [&](int64_t v0, int64_t len, double *px) -> int {
        return stage_rows(px, x + v0, channels, len, ldx, len, s);
      },
      [&](int64_t v0, int64_t len, const double *px) -> int {
        return unstage_rows(out + v0, px, channels, len, ldo, s);
      },
      s);
}

int gdsp_sosfiltfilt_batch_device(const void *d_x, int64_t ldx, const double *sos, int64_t S,
                                  int64_t padlen, int64_t channels, int64_t n, void *d_out,
                                  int64_t ldo, void *d_work, void *stream) {
  bool done = false;
  int64_t pl = 0;
  if (padlen < -1) return fail(GDSP_ERR_INVALID, "negative size");
  STCHK(sos_check(d_x, ldx, sos, S, padlen, channels, n, d_out, ldo, &pl, &done));
  if (done) return GDSP_OK;
  if (channels == 1) ldx = ldo = n;
  if (sos_overlap(d_x, ldx, d_out, ldo, channels, n))
    return fail(GDSP_ERR_INVALID, "d_out overlaps d_x");
  double zi[2 * gdsp::kSosMaxSections];
  STCHK(gdsp_sosfilt_zi(sos, S, zi));
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = (hipStream_t)stream;
  DevBuf w;
  double *work = (double *)d_work;
  if (!work) {
    STCHK(w.alloc((size_t)gdsp_sosfiltfilt_work_doubles(S, channels, n, pl) * sizeof(double), s,
                  SLOT_SOS));
    work = (double *)w.p;
  }
  const int64_t L = n + 2 * pl;
  double *d_zi = work + sos_work_doubles(S, channels, L), *zrows = d_zi + 2 * S,
         *mid = zrows + channels * 2 * S;
  const bool fused = gdsp_sosfilt_fused(sos, S) != 0;
  STCHK(sos_upload(sos, (int)S, fused, work, s));
  HIPCHK(gdsp::launch_sos_tables(zi, 2 * S, d_zi, s));
  // forward over the odd extension, which the loader forms
  gdsp::SosIo fw = {};
  fw.src = (const double *)d_x, fw.lds = ldx, fw.dst = mid, fw.ldd = L, fw.n = L, fw.nx = n;
  fw.pad = pl, fw.mode = gdsp::SOS_IO_ODD_EXT;
  HIPCHK(gdsp::launch_sos_ffzi(fw, 0, d_zi, (int)S, channels, zrows, s));
  STCHK(sos_run(fw, (int)S, fused, channels, zrows, nullptr, work, s));
  // backward over that, as far as the first sample kept
  gdsp::SosIo bw = {};
  bw.src = mid, bw.lds = L, bw.dst = (double *)d_out, bw.ldd = ldo, bw.n = L - pl, bw.nx = L;
  bw.nout = n, bw.mode = gdsp::SOS_IO_REVERSED;
  HIPCHK(gdsp::launch_sos_ffzi(bw, 0, d_zi, (int)S, channels, zrows, s));
  return sos_run(bw, (int)S, fused, channels, zrows, nullptr, work, s);
}

int gdsp_sosfiltfilt_batch(const double *x, int64_t ldx, const double *sos, int64_t S,
                           int64_t padlen, int64_t channels, int64_t n, double *out,
                           int64_t ldo) {
  bool done = false;
  int64_t pl = 0;
  if (padlen < -1) return fail(GDSP_ERR_INVALID, "negative size");
  STCHK(sos_check(x, ldx, sos, S, padlen, channels, n, out, ldo, &pl, &done));
  if (done) return GDSP_OK;
  double zi[2 * gdsp::kSosMaxSections];
  STCHK(gdsp_sosfilt_zi(sos, S, zi));
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  if (channels == 1) ldx = ldo = n;
  const int64_t L = n + 2 * pl, Lb = L - pl, S2 = 2 * S;
  const int64_t rng = sos_chunk_len(S, channels);
  // the intermediate of both passes stays in host memory
  std::vector<double> mid((size_t)channels * (size_t)L), zrows((size_t)channels * (size_t)S2);
  std::vector<double> buf((size_t)channels * (size_t)(L < rng ? L : rng));
  // sample v of row c's odd extension, as the device entry's loader forms it
  auto ext = [&](int64_t c, int64_t v) -> double {
    const double *r = x + c * ldx;
    const int64_t u = v - pl;
    if (u < 0) return 2.0 * r[0] - r[-u];
    if (u >= n) return 2.0 * r[n - 1] - r[2 * (n - 1) - u];
    return r[u];
  };
  for (int64_t c = 0; c < channels; ++c)
    for (int64_t j = 0; j < S2; ++j) zrows[c * S2 + j] = zi[j] * ext(c, 0);
  STCHK(sos_host_chunks(
      sos, S, channels, L, zrows.data(), nullptr,
      [&](int64_t v0, int64_t len, double *px) -> int {
        for (int64_t c = 0; c < channels; ++c)
          for (int64_t i = 0; i < len; ++i) buf[c * len + i] = ext(c, v0 + i);
        return stage_rows(px, buf.data(), channels, len, len, len, s);
      },
      [&](int64_t v0, int64_t len, const double *px) -> int {
        return unstage_rows(mid.data() + v0, px, channels, len, L, s);
      },
      s));
  for (int64_t c = 0; c < channels; ++c)
    for (int64_t j = 0; j < S2; ++j) zrows[c * S2 + j] = zi[j] * mid[c * L + L - 1];
  return sos_host_chunks(
      sos, S, channels, Lb, zrows.data(), nullptr,
      [&](int64_t v0, int64_t len, double *px) -> int {
        for (int64_t c = 0; c < channels; ++c)
          for (int64_t i = 0; i < len; ++i) buf[c * len + i] = mid[c * L + L - 1 - (v0 + i)];
        return stage_rows(px, buf.data(), channels, len, len, len, s);
      },
      [&](int64_t v0, int64_t len, const double *px) -> int {
        STCHK(unstage_rows(buf.data(), px, channels, len, len, s));
        for (int64_t c = 0; c < channels; ++c)
          for (int64_t i = 0; i < len; ++i) {
            const int64_t j = Lb - 1 - (v0 + i);
            if (j < n) out[c * ldo + j] = buf[c * len + i];
          }
        return GDSP_OK;
      },
      s);
}

int gdsp_fft2_device(const void *d_in, void *d_out, int64_t rows, int64_t cols, int inverse,
                     void *d_work, void *stream) {
  // fft/fft.go:123-154: column pass (length rows, batch cols), then row pass
  if (rows <= 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  if (cols < 0) return fail(GDSP_ERR_INVALID, "negative size");
  // computeFFT2's row pass calls IFFT on each empty row, which panics
  // (fft/fft.go:40, :149-151); FFT of an empty row returns it unchanged
  if (cols == 0)
    return inverse ? fail(GDSP_ERR_EMPTY, "IFFT of an empty slice (index out of range)") : GDSP_OK;
  hipStream_t s = (hipStream_t)stream;  // NULL = the null stream (HIP convention)
  int dev = 0;
  STCHK(current_device(&dev));
  gdsp_plan *pr = nullptr, *pc = nullptr;
  STCHK(get_plan(rows, &pr));
  STCHK(get_plan(cols, &pc));
  DevBuf w;
  cd *work = (cd *)d_work;
  if (!work) {
    STCHK(w.alloc((size_t)rows * (size_t)cols * sizeof(cd), s, SLOT_FFT2));
    work = (cd *)w.p;
  }
  const bool inv = inverse != 0;
  const int lr = ilog2(rows);
  if (is_pow2(rows) && lr >= gdsp::kColMinLog2 && lr <= 2 * gdsp::kColMaxLog2) {
    // row pass (contiguous rows, any length) -> work; column pass on
    // row-segment tiles: one kernel for rows <= 512, otherwise the four-step
    // split rows = R1*R2 (A in place on work, B from work into out)
    STCHK(exec_plan(pc, d_in, work, rows, inv, gdsp::LOAD_COMPLEX, s));
    const double sc = 1.0 / (double)rows;
    if (lr <= gdsp::kColMaxLog2) {
      HIPCHK(gdsp::launch_colfft(lr, inv, 0, inv, work, (cd *)d_out, cols, 1, 0, 1, 0, 1,
                                 pr->tw, nullptr, lr, sc, 1, 0, s));
    } else {
      const int l1 = lr / 2, l2 = lr - l1;  // R1 <= R2
      gdsp_plan *p1 = nullptr, *p2 = nullptr;
      STCHK(get_plan((int64_t)1 << l1, &p1));
      STCHK(get_plan((int64_t)1 << l2, &p2));
      const int64_t R1 = (int64_t)1 << l1, R2 = (int64_t)1 << l2;
      HIPCHK(gdsp::launch_colfft(l1, inv, 1, false, work, work, cols, R2, 1, R2, 1, R2, p1->tw,
                                 pr->tw, lr, 1.0, 1, 0, s));
      HIPCHK(gdsp::launch_colfft(l2, false, 0, inv, work, (cd *)d_out, cols, R1, R2, 1, 1, R1,
                                 p2->tw, nullptr, lr, sc, 1, 0, s));
    }
    return GDSP_OK;
  }
  HIPCHK(gdsp::launch_transpose((const cd *)d_in, work, rows, cols, s));
  STCHK(exec_plan(pr, work, work, cols, inv, gdsp::LOAD_COMPLEX, s));
  HIPCHK(gdsp::launch_transpose(work, (cd *)d_out, cols, rows, s));
  STCHK(exec_plan(pc, d_out, (cd *)d_out, rows, inv, gdsp::LOAD_COMPLEX, s));
  return GDSP_OK;
}

// One axis of computeFFTN (fft/fft.go:172-185): the 1-D transform of the
// `outer` x `inner` lines of length L, read from src (cur itself, or the
// caller's input for the first axis), result in cur; other is scratch.
static int fft_axis(const cd *src, cd *cur, cd *other, int64_t L, int64_t inner, int64_t outer,
                    bool inv, hipStream_t s) {
  gdsp_plan *pl = nullptr;
  STCHK(get_plan(L, &pl));
  if (inner == 1) {
    STCHK(exec_plan(pl, src, cur, outer, inv, gdsp::LOAD_COMPLEX, s));
    return GDSP_OK;
  }
  const int lL = ilog2(L);
  const double sc = 1.0 / (double)L;
  if (is_pow2(L) && lL >= gdsp::kColMinLog2 && lL <= 2 * gdsp::kColMaxLog2) {
    const int l1 = lL <= gdsp::kColMaxLog2 ? lL : lL / 2, l2 = lL - l1;
    gdsp_plan *p1 = nullptr, *p2 = nullptr;
    STCHK(get_plan((int64_t)1 << l1, &p1));
    if (l2) STCHK(get_plan((int64_t)1 << l2, &p2));
    const int64_t R1 = (int64_t)1 << l1, R2 = (int64_t)1 << l2;
    for (int64_t o0 = 0; o0 < outer; o0 += 65535) {
      later_chunk(o0);
      const int64_t nb = outer - o0 < 65535 ? outer - o0 : 65535;
      const cd *s0 = src + o0 * L * inner;
      cd *c0 = cur + o0 * L * inner, *t0 = other + o0 * L * inner;
      if (!l2) {
        HIPCHK(gdsp::launch_colfft(lL, inv, 0, inv, s0, c0, inner, 1, 0, 1, 0, 1, pl->tw,
                                   nullptr, lL, sc, nb, L * inner, s));
      } else {
        // A: src -> other, B: other -> cur (the result lands in cur, and
        // the caller's input is never written)
        HIPCHK(gdsp::launch_colfft(l1, inv, 1, false, s0, t0, inner, R2, 1, R2, 1, R2, p1->tw,
                                   pl->tw, lL, 1.0, nb, L * inner, s));
        HIPCHK(gdsp::launch_colfft(l2, false, 0, inv, t0, c0, inner, R1, R2, 1, 1, R1, p2->tw,
                                   nullptr, lL, sc, nb, L * inner, s));
      }
    }
    return GDSP_OK;
  }
  for (int64_t o0 = 0; o0 < outer; o0 += 65535) {
    later_chunk(o0);
    const int64_t nb = outer - o0 < 65535 ? outer - o0 : 65535;
    HIPCHK(gdsp::launch_transpose(src + o0 * L * inner, other + o0 * L * inner, L, inner, s, nb));
  }
  STCHK(exec_plan(pl, other, other, outer * inner, inv, gdsp::LOAD_COMPLEX, s));
  for (int64_t o0 = 0; o0 < outer; o0 += 65535) {
    later_chunk(o0);
    const int64_t nb = outer - o0 < 65535 ? outer - o0 : 65535;
    HIPCHK(gdsp::launch_transpose(other + o0 * L * inner, cur + o0 * L * inner, inner, L, s, nb));
  }
  return GDSP_OK;
}

// fft.FFTN / IFFTN (fft/fft.go:157-192): the 1-D transform along every line
// of dimension 0, then 1, ... of a row-major array. Per axis (length L,
// `inner` elements after it, `outer` before): contiguous lines (inner = 1) go
// to the batched row kernels; strided power-of-2 lines to the column-tile
// kernels batched over `outer` (one pass for L <= 512, the four-step split
// above); anything else through a batched transpose, the row kernels and a
// transpose back. axis >= 0 transforms that axis only.
static int fftn_device(const cd *in, cd *out, const int64_t *dims, int ndims, bool inv,
                       hipStream_t s, int axis = -1) {
  if (ndims < 1 || !dims) return fail(GDSP_ERR_INVALID, "no dimensions");
  if (axis >= ndims) return fail(GDSP_ERR_INVALID, "axis out of range");
  int64_t total = 1;
  for (int i = 0; i < ndims; ++i) {
    if (dims[i] < 1) return fail(GDSP_ERR_INVALID, "invalid dimensions");  // matrix.go:43
    total *= dims[i];
  }
  DevBuf work;
  STCHK(work.alloc((size_t)total * sizeof(cd), s, SLOT_FFTN));
  cd *cur = out, *other = (cd *)work.p;
  const cd *src = in;  // the first transformed axis reads the input directly
  int64_t inner = total;
  for (int d = 0; d < ndims; ++d) {
    const int64_t L = dims[d];
    inner /= L;
    const int64_t outer = total / (L * inner);
    if ((axis >= 0 && d != axis) || L == 1) continue;
    STCHK(fft_axis(src, cur, other, L, inner, outer, inv, s));
    src = cur;
  }
  if (src != out)
    HIPCHK(hipMemcpyAsync(out, src, (size_t)total * sizeof(cd), hipMemcpyDeviceToDevice, s));
  return GDSP_OK;
}

static int fft2_host(const double *x, bool real_in, double *out, int64_t rows, int64_t cols,
                     int inverse) {
  if (rows <= 0) return fail(GDSP_ERR_EMPTY, "empty input array");
  if (cols < 0) return fail(GDSP_ERR_INVALID, "negative size");
  // computeFFT2's row pass calls IFFT on each empty row, which panics
  // (fft/fft.go:40, :149-151); FFT of an empty row returns it unchanged
  if (cols == 0)
    return inverse ? fail(GDSP_ERR_EMPTY, "IFFT of an empty slice (index out of range)") : GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  const size_t cnt = (size_t)rows * (size_t)cols;
  DevBuf din, dout;
  STCHK(din.alloc(cnt * sizeof(cd), s, SLOT_IN));
  STCHK(dout.alloc(cnt * sizeof(cd), s, SLOT_OUT));
  if (real_in) {
    DevBuf dr;
    STCHK(dr.alloc(cnt * sizeof(double), s, SLOT_AUX));
    STCHK(copy_h2d(dr.p, x, cnt * sizeof(double), s));
    HIPCHK(gdsp::launch_real_to_complex((const double *)dr.p, (cd *)din.p, (int64_t)cnt, s));
  } else {
    STCHK(copy_h2d(din.p, x, cnt * sizeof(cd), s));
  }
  STCHK(gdsp_fft2_device(din.p, dout.p, rows, cols, inverse, nullptr, (void *)s));
  STCHK(copy_d2h(out, dout.p, cnt * sizeof(cd), s));
  return GDSP_OK;
}

int gdsp_fft2(const double *x, double *out, int64_t rows, int64_t cols, int inverse) {
  return fft2_host(x, false, out, rows, cols, inverse);
}

int gdsp_fft2_real(const double *x, double *out, int64_t rows, int64_t cols, int inverse) {
  return fft2_host(x, true, out, rows, cols, inverse);
}

int gdsp_fft_axis_device(const void *d_in, void *d_out, const int64_t *dims, int ndims,
                         int axis, int inverse, void *stream) {
  if (axis < 0) return fail(GDSP_ERR_INVALID, "axis out of range");
  int dev = 0;
  STCHK(current_device(&dev));
  return fftn_device((const cd *)d_in, (cd *)d_out, dims, ndims, inverse != 0,
                     (hipStream_t)stream, axis);
}

int gdsp_fftn_device(const void *d_in, void *d_out, const int64_t *dims, int ndims, int inverse,
                     void *stream) {
  int dev = 0;
  STCHK(current_device(&dev));
  return fftn_device((const cd *)d_in, (cd *)d_out, dims, ndims, inverse != 0,
                     (hipStream_t)stream);
}

int gdsp_fftn(const double *x, double *out, const int64_t *dims, int ndims, int inverse) {
  if (ndims < 1 || !dims || !x || !out) return fail(GDSP_ERR_INVALID, "bad argument");
  int64_t total = 1;
  for (int i = 0; i < ndims; ++i) {
    if (dims[i] < 1) return fail(GDSP_ERR_INVALID, "invalid dimensions");
    total *= dims[i];
  }
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  const size_t bytes = (size_t)total * sizeof(cd);
  DevBuf din, dout;
  STCHK(din.alloc(bytes, s, SLOT_IN));
  STCHK(dout.alloc(bytes, s, SLOT_OUT));
  STCHK(copy_h2d(din.p, x, bytes, s));
  STCHK(fftn_device((const cd *)din.p, (cd *)dout.p, dims, ndims, inverse != 0, s));
  STCHK(copy_d2h(out, dout.p, bytes, s));
  return GDSP_OK;
}

int gdsp_ensure_plan(int64_t n) {
  if (n < 0) return fail(GDSP_ERR_INVALID, "negative size");
  gdsp_plan *p = nullptr;
  return get_plan(n, &p);
}

void gdsp_set_worker_pool_size(int n) { g_worker_pool_size = n < 0 ? 0 : n; }
int gdsp_worker_pool_size(void) { return g_worker_pool_size; }

int gdsp_plan_create(int64_t n, gdsp_plan **plan) {
  if (n < 0 || !plan) return fail(GDSP_ERR_INVALID, "bad argument");
  return get_plan(n, plan);
}

int gdsp_plan_create_chirpz(int64_t n, gdsp_plan **plan) {
  if (n < 2 || !plan) return fail(GDSP_ERR_INVALID, "bad argument");
  return get_plan(n, plan, true);
}

int gdsp_plan_destroy(gdsp_plan *) { return GDSP_OK; }

int gdsp_plan_kind(const gdsp_plan *plan) { return plan ? plan->kind : -1; }
int gdsp_plan_parts(const gdsp_plan *plan) { return plan ? plan->parts : 0; }

int gdsp_plan_radices(const gdsp_plan *plan, int *rad, int cap) {
  if (!plan || cap < 0 || (cap > 0 && !rad)) return fail(GDSP_ERR_INVALID, "bad argument");
  const gdsp::MixedDesc *d = nullptr;
  if (plan->kind == KIND_MIXED || plan->kind == KIND_RADER) d = &plan->md;
  else if (plan->blufix) d = &plan->md_blu;
  else if (plan->kind == KIND_RADER_PFA && plan->p2) d = &plan->p2->md;
  if (!d) return 0;
  for (int q = 0; q < d->npass && q < cap; ++q) rad[q] = (int)((d->codes >> (5 * q)) & 31);
  return d->npass;
}

int gdsp_plan_info(const gdsp_plan *plan, int64_t *n, int64_t *m, int64_t *n1, int64_t *n2,
                   int *runtime_compiled) {
  if (!plan) return fail(GDSP_ERR_INVALID, "NULL plan");
  if (n) *n = plan->n;
  if (m) *m = plan->blufix ? plan->m_blu : plan->m;
  if (n1) *n1 = plan->n1;
  if (n2) *n2 = plan->n2;
  if (runtime_compiled)
    *runtime_compiled = (plan->jit || plan->mixcol || plan->rader || plan->blufix) ? 1 : 0;
  return GDSP_OK;
}

int gdsp_fft_batch_device(const gdsp_plan *plan, const void *d_in, void *d_out, int64_t batch,
                          int inverse, void *stream) {
  if (!plan || batch < 0) return fail(GDSP_ERR_INVALID, "bad argument");
  if (plan->n == 0 && inverse) return fail(GDSP_ERR_EMPTY, "IFFT of an empty slice");
  return exec_plan(plan, d_in, (cd *)d_out, batch, inverse != 0, gdsp::LOAD_COMPLEX,
                   (hipStream_t)stream);
}

int gdsp_fft_real_batch_device(const gdsp_plan *plan, const double *d_in, void *d_out,
                               int64_t batch, int inverse, void *stream) {
  if (!plan || batch < 0) return fail(GDSP_ERR_INVALID, "bad argument");
  if (plan->n == 0 && inverse) return fail(GDSP_ERR_EMPTY, "IFFT of an empty slice");
  const size_t in_bytes = (size_t)batch * (size_t)plan->n * sizeof(double);
  const char *i0 = (const char *)d_in, *o0 = (const char *)d_out;
  if (batch > 0 && plan->n > 0 && i0 < o0 + 2 * in_bytes && o0 < i0 + in_bytes)
    return fail(GDSP_ERR_INVALID, "real input overlaps the complex output");
  hipStream_t s = (hipStream_t)stream;
  if (inverse && batch > 0 && plan->n > 0) {
    // IFFTReal (fft.go:30-32 = IFFT(ToComplex(x))): the kernels read real rows
    // in the forward direction only, so widen into d_out and transform there
    HIPCHK(gdsp::launch_real_to_complex(d_in, (cd *)d_out, batch * plan->n, s));
    return exec_plan(plan, d_out, (cd *)d_out, batch, true, gdsp::LOAD_COMPLEX, s);
  }
  return exec_plan(plan, d_in, (cd *)d_out, batch, inverse != 0, gdsp::LOAD_REAL, s);
}

static bool wav_format_ok(int audio_format, int bits) {
  return (audio_format == 1 && (bits == 8 || bits == 16)) || audio_format == 3;
}

static int64_t wav_sample_bytes(int audio_format, int bits) {
  return audio_format == 3 ? 4 : bits / 8;
}

int gdsp_wav_read_floats_device(const void *d_in, int64_t count, int audio_format,
                                int bits_per_sample, void *d_out, int out_f64, void *stream) {
  if (count < 0 || (count && (!d_in || !d_out))) return fail(GDSP_ERR_INVALID, "bad argument");
  if (!wav_format_ok(audio_format, bits_per_sample))
    return fail(GDSP_ERR_UNSUPPORTED, audio_format == 1 ? "wav: unknown bits per sample"
                                                        : "wav: unknown audio format");
  if (count == 0) return GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  HIPCHK(gdsp::launch_wav_decode(d_in, count, audio_format, bits_per_sample, d_out, out_f64 != 0,
                                 (hipStream_t)stream));
  return GDSP_OK;
}

int gdsp_wav_read_floats_planar_device(const void *d_in, int64_t frames, int64_t channels,
                                       int audio_format, int bits_per_sample, double *d_out,
                                       int64_t ld_out, void *stream) {
  if (frames < 0 || channels < 0 || channels > 65535 || (channels > 1 && ld_out < frames) ||
      (frames && channels && (!d_in || !d_out)))
    return fail(GDSP_ERR_INVALID, "bad argument");
  if (!wav_format_ok(audio_format, bits_per_sample))
    return fail(GDSP_ERR_UNSUPPORTED, audio_format == 1 ? "wav: unknown bits per sample"
                                                        : "wav: unknown audio format");
  if (frames == 0 || channels == 0) return GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  HIPCHK(gdsp::launch_wav_decode_planar(d_in, frames, (int)channels, audio_format,
                                        bits_per_sample, d_out, ld_out, (hipStream_t)stream));
  return GDSP_OK;
}

int gdsp_wav_read_floats(const void *in, int64_t count, int audio_format, int bits_per_sample,
                         void *out, int out_f64) {
  if (count < 0 || (count && (!in || !out))) return fail(GDSP_ERR_INVALID, "bad argument");
  if (!wav_format_ok(audio_format, bits_per_sample))
    return fail(GDSP_ERR_UNSUPPORTED, audio_format == 1 ? "wav: unknown bits per sample"
                                                        : "wav: unknown audio format");
  if (count == 0) return GDSP_OK;
  int dev = 0;
  STCHK(current_device(&dev));
  hipStream_t s = thread_stream(dev);
  if (!s) return fail(GDSP_ERR_HIP, "stream creation failed");
  const size_t in_bytes = (size_t)count * (size_t)wav_sample_bytes(audio_format, bits_per_sample);
  const size_t out_bytes = (size_t)count * (out_f64 ? 8 : 4);
  DevBuf din, dout;
  STCHK(din.alloc(in_bytes, s, SLOT_IN));
  STCHK(dout.alloc(out_bytes, s, SLOT_OUT));
  STCHK(copy_h2d(din.p, in, in_bytes, s));
  HIPCHK(gdsp::launch_wav_decode(din.p, count, audio_format, bits_per_sample, dout.p,
                                 out_f64 != 0, s));
  STCHK(copy_d2h(out, dout.p, out_bytes, s));  // returns after the stream drained
  return GDSP_OK;
}

int gdsp_fill_uniform_device(double *d_out, int64_t count, uint64_t seed, uint64_t offset,
                             void *stream) {
  if (count < 0 || (!d_out && count)) return fail(GDSP_ERR_INVALID, "bad argument");
  int dev = 0;
  STCHK(current_device(&dev));
  HIPCHK(gdsp::launch_fill_uniform(d_out, count, seed, offset, (hipStream_t)stream));
  return GDSP_OK;
}

}  // extern "C"
