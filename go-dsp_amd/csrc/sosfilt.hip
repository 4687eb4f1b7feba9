// sosfilt.hip — recursive (IIR) filtering of real rows by second-order
// sections (scipy.signal.sosfilt; no reference equivalent). Every section is
// the transposed direct form II
//   y = b0 x + z0;   z0 = b1 x - a1 y + z1;   z1 = b2 x - a2 y
// (sos_step below, the one place the recurrence is written), the sections in
// cascade order, one set of coefficients for all rows.
//
//   sos_tables_kernel  the host's tables (long double, rounded) into device
//                      memory, once per call
//   sos_tile_kernel    the time-parallel form, S <= 8 stable sections: a
//                      workgroup owns one tile of 256 x 16 samples of one row.
//                      PASS 1 runs it from zero state and keeps only the end
//                      state; PASS 3 runs it from the true entry state and
//                      stores every sample once
//   sos_scan_kernel    pass 2: st[k + 1] = Phi st[k] + g[k] along each row,
//                      one wave per row, sequential over the tiles
//   sos_plain_kernel   one thread per row, sequential, from global memory:
//                      any S <= 64 and any coefficients
//   sos_ffzi_kernel    sosfiltfilt's initial states zi[s] * (first sample)
//
// A tile: the samples go through LDS (coalesced HBM accesses on both sides;
// thread t owns samples t E .. t E + E - 1, at a stride of E + 1 doubles so
// that the lanes' reads fall on distinct banks). Per section the thread runs
// its E samples from zero state in registers; the end states are scanned
// (Kogge-Stone over the lanes of a wave on shuffles with M^(2^k), M = A^E;
// the four waves' ends through LDS, sequentially with M^64); the state that
// enters the thread is the scan's value of the lane before it plus M^lane
// applied to the state entering the wave; each sample then gets the zero-input
// response of that state, two multiply-adds from the E x 2 table. The corrected
// samples are the next section's input. Nothing waits on another workgroup and
// nothing is atomic; the arithmetic of a sample depends on its position from
// the row's start and on nothing else.
#include "fft_device.hpp"
#include "launch.hpp"

namespace gdsp {

namespace {

constexpr int kT = kSosThreads, kE = kSosE, kTile = kSosTile;
static_assert(kT * kE == kTile && kT == 256 && kE == 16, "tile geometry");
constexpr int kLevels = 7;  // M^(2^k), k = 0..5 inside a wave, 6 between waves

// table offsets within a section's block (SosTables in launch.hpp)
constexpr int kCoef = 0, kZir = 8, kPow = 8 + 2 * kE;
static_assert(kPow + 4 * kLevels <= kSosSecDoubles, "section block");

__device__ __forceinline__ int sos_padx(int i) { return i + (i >> 4); }

// one step of a section: returns y, advances (z0, z1)
__device__ __forceinline__ double sos_step(double b0, double b1, double b2, double a1, double a2,
                                           double x, double &z0, double &z1) {
  const double y = fma(b0, x, z0);
  z0 = fma(b1, x, fma(-a1, y, z1));
  z1 = fma(b2, x, -a2 * y);
  return y;
}

// sample v of the virtual row (SosIo in launch.hpp)
__device__ __forceinline__ double sos_load(const SosIo &io, const double *row, int64_t v) {
  if (io.mode == SOS_IO_PLAIN) return ld_nt(&row[v]);
  if (io.mode == SOS_IO_REVERSED) return ld_nt(&row[io.nx - 1 - v]);
  const int64_t u = v - io.pad;  // the odd extension about both ends
  if (u < 0) return fma(2.0, row[0], -row[-u]);
  if (u >= io.nx) return fma(2.0, row[io.nx - 1], -row[2 * (io.nx - 1) - u]);
  return ld_nt(&row[u]);
}

// where sample v of the result goes, or -1: not stored
__device__ __forceinline__ int64_t sos_store_index(const SosIo &io, int64_t v) {
  if (io.mode != SOS_IO_REVERSED) return v;
  const int64_t i = io.n - 1 - v;  // the middle nout samples, reversed back
  return i < io.nout ? i : -1;
}

}  // namespace

__global__ void sos_tables_kernel(SosTablePart part, double *tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < part.count) tab[part.offset + i] = part.v[i];
}

// Workgroup blk serves channel c0 + blk / tpr and tile blk % tpr of it.
// PASS 1: from zero state; the end state (2 S doubles) to g[(c np1 + k) 2 S].
// PASS 3: from states[(c (np1 + 1) + k) 2 S] (states == NULL: the call has one
// tile per row, from zi or zeros); every sample stored once; the thread that
// holds the row's last sample writes zf when the row does not end on a tile
// (then pass 2 has the value).
template <int PASS>
__global__ __launch_bounds__(kSosThreads) void sos_tile_kernel(
    SosIo io, const double *__restrict__ tab, int S, int64_t tpr, int64_t c0, int64_t np1,
    const double *states, double *g, const double *zi, double *zf) {
  __shared__ double lx[kTile + kTile / 16];
  __shared__ double lw[kSosMaxFused][4][2];
  const int lt = threadIdx.x, lane = lt & 63, wv = lt >> 6;
  const int64_t blk = blockIdx.x;
  const int64_t cr = blk / tpr, k = blk - cr * tpr, c = c0 + cr;
  const int64_t v0 = k * kTile;
  const int cnt = io.n - v0 < kTile ? (int)(io.n - v0) : kTile;
  const double *row = io.src + c * io.lds;

  {
    double v[kE];
#pragma unroll
    for (int u = 0; u < kE; ++u) {
      const int i = lt + u * kT;
      v[u] = i < cnt ? sos_load(io, row, v0 + i) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kE; ++u) lx[sos_padx(lt + u * kT)] = v[u];
  }
  __syncthreads();
  double x[kE];
#pragma unroll
  for (int i = 0; i < kE; ++i) x[i] = lx[sos_padx(lt * kE + i)];

  const int S2 = 2 * S;
  const int r = cnt - lt * kE;  // samples of the row from this thread's first on (any sign)
  const bool tail = v0 + cnt == io.n;  // the row's last tile
  for (int s = 0; s < S; ++s) {
    const double *ts = tab + s * kSosSecDoubles;
    const double b0 = ts[kCoef], b1 = ts[kCoef + 1], b2 = ts[kCoef + 2], a1 = ts[kCoef + 3],
                 a2 = ts[kCoef + 4];
    double y[kE], f0 = 0.0, f1 = 0.0;
#pragma unroll
    for (int i = 0; i < kE; ++i) y[i] = sos_step(b0, b1, b2, a1, a2, x[i], f0, f1);
    // inclusive scan of the end states over the wave
#pragma unroll
    for (int l = 0; l < 6; ++l) {
      const double *m = ts + kPow + 4 * l;
      const double p0 = __shfl_up(f0, 1 << l), p1 = __shfl_up(f1, 1 << l);
      const double n0 = fma(m[0], p0, fma(m[1], p1, f0)), n1 = fma(m[2], p0, fma(m[3], p1, f1));
      if (lane >= (1 << l)) f0 = n0, f1 = n1;
    }
    if (lane == 63) lw[s][wv][0] = f0, lw[s][wv][1] = f1;
    // the state entering the tile
    double e0 = 0.0, e1 = 0.0;
    if (PASS == 3) {
      if (states) {
        const double *st = states + (c * (np1 + 1) + k) * S2 + 2 * s;
        e0 = st[0], e1 = st[1];
      } else if (zi) {
        e0 = zi[c * S2 + 2 * s], e1 = zi[c * S2 + 2 * s + 1];
      }
    }
    __syncthreads();
    // the state entering this wave; in pass 1 also the one leaving the tile
    const double *m6 = ts + kPow + 4 * 6;
    for (int w = 0; w < wv; ++w) {
      const double w0 = lw[s][w][0], w1 = lw[s][w][1];
      const double n0 = fma(m6[0], e0, fma(m6[1], e1, w0)), n1 = fma(m6[2], e0, fma(m6[3], e1, w1));
      e0 = n0, e1 = n1;
    }
    if (PASS == 1 && lt == kT - 1) {  // of the last wave: its own end is f
      double *gs = g + (c * np1 + k) * S2 + 2 * s;
      gs[0] = fma(m6[0], e0, fma(m6[1], e1, f0));
      gs[1] = fma(m6[2], e0, fma(m6[3], e1, f1));
    }
    // M^lane on it, plus the scan's value of the lane before
    double q0 = e0, q1 = e1;
#pragma unroll
    for (int l = 0; l < 6; ++l) {
      const double *m = ts + kPow + 4 * l;
      const double n0 = fma(m[0], q0, m[1] * q1), n1 = fma(m[2], q0, m[3] * q1);
      if ((lane >> l) & 1) q0 = n0, q1 = n1;
    }
    const double u0 = __shfl_up(f0, 1), u1 = __shfl_up(f1, 1);
    const double in0 = lane ? u0 + q0 : q0, in1 = lane ? u1 + q1 : q1;
    if (PASS == 3 && zf && tail && r > 0 && r <= kE) {
      // the row ends in this thread: its state after r samples
      double z0 = in0, z1 = in1;
#pragma unroll
      for (int i = 0; i < kE; ++i)
        if (i < r) (void)sos_step(b0, b1, b2, a1, a2, x[i], z0, z1);
      zf[c * S2 + 2 * s] = z0, zf[c * S2 + 2 * s + 1] = z1;
    }
#pragma unroll
    for (int i = 0; i < kE; ++i)
      x[i] = fma(ts[kZir + 2 * i], in0, fma(ts[kZir + 2 * i + 1], in1, y[i]));
  }
  if (PASS == 1) return;
#pragma unroll
  for (int i = 0; i < kE; ++i) lx[sos_padx(lt * kE + i)] = x[i];
  __syncthreads();
  double *orow = io.dst + c * io.ldd;
#pragma unroll
  for (int u = 0; u < kE; ++u) {
    const int i = lt + u * kT;
    if (i < cnt) {
      const int64_t j = sos_store_index(io, v0 + i);
      if (j >= 0) __builtin_nontemporal_store(lx[sos_padx(i)], &orow[j]);
    }
  }
}

// the value of v in lane `lane` (a constant), through a scalar register
__device__ __forceinline__ double sos_bcast(double v, int lane) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, lane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), lane);
  return __builtin_bit_cast(double, (unsigned long long)lo | ((unsigned long long)hi << 32));
}

// One wave per row; lane j < 2 S holds component j of the state and row j of
// Phi (block lower triangular: a section's state depends on the sections up
// to it, so only i <= j | 1 is summed, term i into chain i mod 4 in ascending
// i, st = (c0 + c1) + (c2 + c3) with g in c0). The arithmetic of a step does
// not depend on k: a row may be cut at any tile. The chain of steps is what
// bounds a long row, so nothing else may wait in it: the end states g of 64
// tiles at a time come through LDS, loaded by the whole wave while the block
// before is stepped through (a load from global memory inside a step cost the
// step an L2 round trip), and the state goes from lane to lane through scalar
// registers, all 2 S reads ahead of the multiply-adds (as shuffles through
// LDS, waited for pair by pair, a step of 8 sections took 0.45 us).
template <int S>
__global__ __launch_bounds__(64) void sos_scan_kernel(const double *__restrict__ tab,
                                                      int64_t np1, const double *__restrict__ g,
                                                      const double *zi, double *states,
                                                      double *zf) {
  constexpr int kBlk = 64, S2 = 2 * S;
  __shared__ double lg[kBlk * S2];
  const int j = threadIdx.x;
  const int64_t c = blockIdx.x;
  const bool on = j < S2;
  const int top = j | 1;
  double ph[S2];
#pragma unroll
  for (int i = 0; i < S2; ++i) ph[i] = on ? tab[kSosPhiOffset + j * S2 + i] : 0.0;
  double st = (on && zi) ? zi[c * S2 + j] : 0.0;
  const double *gr = g + c * np1 * S2;
  double *sr = states + c * (np1 + 1) * S2;
  if (on) sr[j] = st;
  const int64_t total = np1 * S2;  // doubles of g of this row
  double r[S2];
#pragma unroll
  for (int u = 0; u < S2; ++u) {
    const int64_t e = (int64_t)u * 64 + j;
    r[u] = e < total ? gr[e] : 0.0;
  }
  for (int64_t k0 = 0; k0 < np1; k0 += kBlk) {
    __syncthreads();  // the steps of the block before have read lg
#pragma unroll
    for (int u = 0; u < S2; ++u) lg[u * 64 + j] = r[u];
    __syncthreads();
    // the next block's loads stay in flight over this block's steps
#pragma unroll
    for (int u = 0; u < S2; ++u) {
      const int64_t e = (k0 + kBlk) * S2 + (int64_t)u * 64 + j;
      r[u] = e < total ? gr[e] : 0.0;
    }
    const int cnt = np1 - k0 < kBlk ? (int)(np1 - k0) : kBlk;
    double gn = on ? lg[j] : 0.0;
    for (int kk = 0; kk < cnt; ++kk) {
      double acc[4] = {gn, 0.0, 0.0, 0.0};
      if (on && kk + 1 < cnt) gn = lg[(kk + 1) * S2 + j];
      double t[S2];
#pragma unroll
      for (int i = 0; i < S2; ++i) t[i] = sos_bcast(st, i);
#pragma unroll
      for (int i = 0; i < S2; ++i) {
        const double n = fma(ph[i], t[i], acc[i & 3]);
        acc[i & 3] = i <= top ? n : acc[i & 3];
      }
      st = (acc[0] + acc[1]) + (acc[2] + acc[3]);
      if (on) sr[(k0 + kk + 1) * S2 + j] = st;
    }
  }
  if (on && zf) zf[c * S2 + j] = st;
}

// Thread c: row c, section by section. Section 0 reads the virtual row; the
// sections between work in place (on dst, or on src where the row is read
// reversed); the last one stores through the output map.
__global__ __launch_bounds__(64) void sos_plain_kernel(SosIo io, const double *__restrict__ tab,
                                                       int S, int64_t channels, const double *zi,
                                                       double *zf) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= channels) return;
  const double *row = io.src + c * io.lds;
  double *orow = io.dst + c * io.ldd;
  const bool rev = io.mode == SOS_IO_REVERSED;
  double *buf = rev ? const_cast<double *>(row) : orow;
  for (int s = 0; s < S; ++s) {
    const double *ts = tab + 5 * s;
    const double b0 = ts[0], b1 = ts[1], b2 = ts[2], a1 = ts[3], a2 = ts[4];
    double z0 = zi ? zi[(c * S + s) * 2] : 0.0, z1 = zi ? zi[(c * S + s) * 2 + 1] : 0.0;
    const bool last = s == S - 1;
    for (int64_t v = 0; v < io.n; ++v) {
      const int64_t bi = rev ? io.nx - 1 - v : v;
      const double xin = s == 0 ? sos_load(io, row, v) : buf[bi];
      const double y = sos_step(b0, b1, b2, a1, a2, xin, z0, z1);
      if (last) {
        const int64_t jo = sos_store_index(io, v);
        if (jo >= 0) orow[jo] = y;
      } else {
        buf[bi] = y;
      }
    }
    if (zf) zf[(c * S + s) * 2] = z0, zf[(c * S + s) * 2 + 1] = z1;
  }
}

// zi_rows[c][s][j] = zi[s][j] * (sample `at` of the virtual row of channel c)
__global__ void sos_ffzi_kernel(SosIo io, int64_t at, const double *__restrict__ zi, int S,
                                int64_t channels, double *zi_rows) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= channels * 2 * S) return;
  const int64_t c = e / (2 * S), j = e - c * 2 * S;
  zi_rows[e] = zi[j] * sos_load(io, io.src + c * io.lds, at);
}

hipError_t launch_sos_tables(const double *host, int64_t count, double *tab, hipStream_t s) {
  if (!host || !tab || count <= 0) return hipErrorInvalidValue;
  for (int64_t o = 0; o < count; o += kSosTablePart) {
    SosTablePart part;
    part.offset = (int)o;
    part.count = (int)(count - o < kSosTablePart ? count - o : kSosTablePart);
    for (int i = 0; i < part.count; ++i) part.v[i] = host[o + i];
    hipLaunchKernelGGL(sos_tables_kernel, dim3((part.count + 255) / 256), dim3(256), 0, s, part,
                       tab);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

static bool sos_io_ok(const SosIo &io) {
  if (!io.src || !io.dst || io.n <= 0 || io.nx <= 0) return false;
  if (io.mode == SOS_IO_PLAIN) return io.nx == io.n;
  if (io.mode == SOS_IO_ODD_EXT) return io.pad >= 0 && io.pad < io.nx && io.n == io.nx + 2 * io.pad;
  if (io.mode == SOS_IO_REVERSED) return io.n <= io.nx && io.nout >= 0 && io.nout <= io.n;
  return false;
}

hipError_t launch_sos_tiles(const SosIo &io, const double *tab, int S, int64_t channels,
                            const double *zi, double *zf, double *scratch, hipStream_t s) {
  if (!sos_io_ok(io) || !tab || S < 1 || S > kSosMaxFused || channels <= 0)
    return hipErrorInvalidValue;
  const int64_t nt = (io.n + kTile - 1) / kTile, full = io.n / kTile;
  const bool ends_on_tile = full * kTile == io.n;
  const bool scan = nt > 1 || (ends_on_tile && zf);
  // tiles whose end state pass 2 needs
  const int64_t np1 = !scan ? 0 : (ends_on_tile && !zf ? full - 1 : full);
  if (scan && !scratch) return hipErrorInvalidValue;
  double *g = scratch, *states = scratch ? scratch + channels * np1 * 2 * S : nullptr;
  const dim3 blockd(kSosThreads);
  if (np1 > 0) {
    const int64_t cpl = 0x7fffffff / np1;
    if (cpl < 1) return hipErrorInvalidValue;
    for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
      const int64_t cc = channels - c0 < cpl ? channels - c0 : cpl;
      hipLaunchKernelGGL(sos_tile_kernel<1>, dim3((unsigned)(cc * np1)), blockd, 0, s, io, tab, S,
                         np1, c0, np1, (const double *)nullptr, g, (const double *)nullptr,
                         (double *)nullptr);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  if (scan) {
    if (channels > 0x7fffffff) return hipErrorInvalidValue;
    double *zfs = ends_on_tile ? zf : nullptr;
    const dim3 grid((unsigned)channels), wave(64);
#define GDSP_SOS_SCAN(SS)                                                                        \
  case SS:                                                                                       \
    hipLaunchKernelGGL(sos_scan_kernel<SS>, grid, wave, 0, s, tab, np1, (const double *)g, zi,   \
                       states, zfs);                                                             \
    break
    switch (S) {
      GDSP_SOS_SCAN(1);
      GDSP_SOS_SCAN(2);
      GDSP_SOS_SCAN(3);
      GDSP_SOS_SCAN(4);
      GDSP_SOS_SCAN(5);
      GDSP_SOS_SCAN(6);
      GDSP_SOS_SCAN(7);
      GDSP_SOS_SCAN(8);
    }
#undef GDSP_SOS_SCAN
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const int64_t cpl = 0x7fffffff / nt;
  if (cpl < 1) return hipErrorInvalidValue;
  for (int64_t c0 = 0; c0 < channels; c0 += cpl) {
    const int64_t cc = channels - c0 < cpl ? channels - c0 : cpl;
    hipLaunchKernelGGL(sos_tile_kernel<3>, dim3((unsigned)(cc * nt)), blockd, 0, s, io, tab, S, nt,
                       c0, np1, scan ? (const double *)states : (const double *)nullptr,
                       (double *)nullptr, zi, ends_on_tile && scan ? (double *)nullptr : zf);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_sos_plain(const SosIo &io, const double *coef, int S, int64_t channels,
                            const double *zi, double *zf, hipStream_t s) {
  if (!sos_io_ok(io) || !coef || S < 1 || S > kSosMaxSections || channels <= 0)
    return hipErrorInvalidValue;
  const int64_t nblk = (channels + 63) / 64;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sos_plain_kernel, dim3((unsigned)nblk), dim3(64), 0, s, io, coef, S, channels,
                     zi, zf);
  return hipGetLastError();
}

hipError_t launch_sos_ffzi(const SosIo &io, int64_t at, const double *zi, int S, int64_t channels,
                           double *zi_rows, hipStream_t s) {
  if (!sos_io_ok(io) || at < 0 || at >= io.n || !zi || !zi_rows || S < 1 || channels <= 0)
    return hipErrorInvalidValue;
  const int64_t cnt = channels * 2 * S, nblk = (cnt + 255) / 256;
  if (nblk > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sos_ffzi_kernel, dim3((unsigned)nblk), dim3(256), 0, s, io, at, zi, S,
                     channels, zi_rows);
  return hipGetLastError();
}

}  // namespace gdsp
