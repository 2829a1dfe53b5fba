// rt_lights_gpu.hip — a distant light's mesh grid, built on the device
// (rt_lights_gpu.h). The passes, per light:
//
//   k_light_faces   one thread per face: the back-face cull, the projected
//                   vertices and the grown box (NaN: never listed); the boxes'
//                   bounds and the kept count reduced per wave, then by
//                   atomics (min / max / integer sums: any order gives the
//                   host's bits). One read-back; the host forms the header
//                   (rt_bins_geom.h light_grid_header).
//   k_light_pairs   count: a block's 256 faces cover anything from one cell
//                   to the whole grid each, so the block deals its (face,
//                   cell) pairs over all its threads by an area prefix and a
//                   binary search; a pair that passes light_face_in_cell adds
//                   one to its cell. rocPRIM scans the counts into `off`; the
//                   64-bit total is read back (it sizes the entries, and a
//                   list past int32 means no grid, as on the host).
//   k_light_lrec    one thread per face: the light's shadow-test records.
//   k_light_pairs   fill: the same pairs again take a slot of their cell (an
//                   atomic cursor) and store (leaf index, coverage, cell).
//   k_light_order   one thread per entry: its rank among its cell's entries
//                   under the host's order — coverage descending, ties by
//                   leaf index ascending, a strict total order, so the result
//                   does not depend on the order the atomics filled the cell
//                   in — and writes the entry and its record at that rank.
//                   The kBinPad padding entries repeat the entry the host
//                   emitted last — the last non-empty cell's highest leaf
//                   index, whatever its rank — and k_light_pad writes those
//                   of a grid without entries.
//   k_light_sat_*   the occupancy prefix sums: a scan along every row, then
//                   an accumulation down every column (integers: exact).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <cmath>
#include <cstring>
#include <limits>

#include "rt_bins.h"
#include "rt_bins_geom.h"
#include "rt_hip.h"
#include "rt_lights_gpu.h"

namespace rtmi {
namespace {

constexpr int kBlock = 256;
enum : int { RED_UMIN = 0, RED_UMAX = 1, RED_VMIN = 2, RED_VMAX = 3, RED_KEPT = 4, RED_TOTAL = 5, RED_SCALE = 6, RED_WORDS = 8 };

// doubles as unsigned keys of the same order (atomicMin / atomicMax)
__host__ __device__ inline unsigned long long key_of(double x) {
  unsigned long long u;
  memcpy(&u, &x, sizeof u);
  return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__host__ __device__ inline double double_of(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? k & 0x7fffffffffffffffull : ~k;
  double x;
  memcpy(&x, &u, sizeof x);
  return x;
}

__device__ inline double wave_min(double x) {
  for (int d = 32; d > 0; d >>= 1) x = bg::dmin(x, __shfl_xor(x, d));
  return x;
}
__device__ inline double wave_max(double x) {
  for (int d = 32; d > 0; d >>= 1) x = bg::dmax(x, __shfl_xor(x, d));
  return x;
}
__device__ inline long long wave_sum(long long x) {
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

__global__ __launch_bounds__(kBlock) void k_light_scale(const DevBinTri* tris, long long n, unsigned long long* red) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  double s = 1.0;
  if (i < n) s = bg::light_face_scale(s, tris[i].v);
  s = wave_max(s);
  if ((threadIdx.x & 63) == 0) atomicMax(&red[RED_SCALE], key_of(s));
}

__global__ __launch_bounds__(kBlock) void k_light_faces(const DevBinTri* tris, long long n, bg::LightBasis lb,
                                                        double delta, double* proj, double* box,
                                                        unsigned long long* red) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
  long long kept = 0;
  if (i < n) {
    double q[6], b[4];
    if (bg::light_face_box(lb, tris[i].v, delta, q, b)) {
      for (int k = 0; k < 6; ++k) proj[6 * i + k] = q[k];
      // a NaN bound is skipped, as by the host's std::min / std::max
      umin = bg::dmin(umin, b[0]);
      umax = bg::dmax(umax, b[1]);
      vmin = bg::dmin(vmin, b[2]);
      vmax = bg::dmax(vmax, b[3]);
      kept = 1;
    } else {
      b[0] = b[1] = b[2] = b[3] = NAN;
    }
    for (int k = 0; k < 4; ++k) box[4 * i + k] = b[k];
  }
  umin = wave_min(umin);
  umax = wave_max(umax);
  vmin = wave_min(vmin);
  vmax = wave_max(vmax);
  kept = wave_sum(kept);
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&red[RED_UMIN], key_of(umin));
    atomicMax(&red[RED_UMAX], key_of(umax));
    atomicMin(&red[RED_VMIN], key_of(vmin));
    atomicMax(&red[RED_VMAX], key_of(vmax));
    if (kept) atomicAdd(&red[RED_KEPT], (unsigned long long)kept);
  }
}

// FILL = false: cnt[cell] += 1 per listed pair, red[RED_TOTAL] += the block's
// pairs. FILL = true: the pair takes slot off[cell] + cnt[cell]++ (cnt zeroed
// again by the caller) of tmp_i / tmp_cov / tmp_cell, `total` slots in all.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_light_pairs(long long n, LightGrid g, double delta, const double* proj,
                                                        const double* box, int32_t* cnt, const int32_t* off,
                                                        long long total, int32_t* tmp_i, double* tmp_cov,
                                                        int32_t* tmp_cell, unsigned long long* red) {
  __shared__ long long pre[kBlock + 1];
  __shared__ int c0s[kBlock], r0s[kBlock], ws[kBlock];
  const int t = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * kBlock, i = base + t;
  long long area = 0;
  int c0 = 0, r0 = 0, w = 1;
  if (i < n && !isnan(box[4 * i])) {
    int rc[4];
    bg::light_cell_range(g, &box[4 * i], rc);
    if (rc[0] <= rc[1] && rc[2] <= rc[3]) {
      c0 = rc[0];
      r0 = rc[2];
      w = rc[1] - rc[0] + 1;
      area = (long long)w * (long long)(rc[3] - rc[2] + 1);
    }
  }
  c0s[t] = c0;
  r0s[t] = r0;
  ws[t] = w;
  if (t == 0) pre[0] = 0;
  pre[t + 1] = area;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {  // inclusive scan of pre[1 ..]
    const long long add = t + 1 > d ? pre[t + 1 - d] : 0;
    __syncthreads();
    pre[t + 1] += add;
    __syncthreads();
  }
  const long long pairs = pre[kBlock];
  const long long ncell = (long long)g.gu * g.gv;
  long long mine = 0;
  for (long long p = t; p < pairs; p += kBlock) {
    int lo = 0, hi = kBlock - 1;  // the last face f with pre[f] <= p
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pre[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int f = lo;
    const long long local = p - pre[f];
    const int c = c0s[f] + (int)(local % ws[f]), r = r0s[f] + (int)(local / ws[f]);
    const double* q = &proj[6 * (base + f)];
    if (!bg::light_face_in_cell(g, q, delta, c, r)) continue;
    const long long cell = (long long)r * g.gu + c;
    if (cell < 0 || cell >= ncell) continue;  // (the range is clamped to the grid)
    if (!FILL) {
      atomicAdd(&cnt[cell], 1);
      ++mine;
    } else {
      const long long slot = (long long)off[cell] + atomicAdd(&cnt[cell], 1);
      if (slot < 0 || slot >= total) continue;  // (count and fill list the same pairs)
      tmp_i[slot] = (int32_t)(base + f);
      tmp_cov[slot] = bg::light_cell_cover(g, q, c, r);
      tmp_cell[slot] = (int32_t)cell;
    }
  }
  if (!FILL) {
    mine = wave_sum(mine);
    if ((t & 63) == 0 && mine) atomicAdd(&red[RED_TOTAL], (unsigned long long)mine);
  }
}

__device__ inline LTri record_of(const LTri* lrec, int32_t rec, long long nnodes, long long ntri) {
  const long long slot = (long long)rec / (long long)sizeof(TriFast) - nnodes;
  return slot >= 0 && slot < ntri ? lrec[slot] : bg::culled_ltri();
}

__global__ __launch_bounds__(kBlock) void k_light_lrec(const DevBinTri* tris, long long n, double d0, double d1,
                                                       double d2, long long nnodes, long long ntri, LTri* lrec) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const long long slot = (long long)tris[i].rec / (long long)sizeof(TriFast) - nnodes;
  if (slot < 0 || slot >= ntri) return;
  const double d[3] = {d0, d1, d2};
  bg::make_ltri(tris[i].v, d, tris[i].face, &lrec[slot]);
}

__global__ __launch_bounds__(kBlock) void k_light_order(long long total, const int32_t* tmp_i, const double* tmp_cov,
                                                        const int32_t* tmp_cell, const int32_t* off,
                                                        const DevBinTri* tris, long long n, long long ncell,
                                                        const LTri* lrec, long long nnodes, long long ntri,
                                                        int32_t* ent, LTri* grec) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= total) return;
  const int32_t cell = tmp_cell[e], i = tmp_i[e];
  if (cell < 0 || cell >= ncell || i < 0 || i >= n) return;  // (every slot was filled with a pair of the grid)
  const int32_t b = off[cell], en = off[cell + 1];
  if (b < 0 || en > total) return;
  const double cov = tmp_cov[e];
  int32_t rank = 0;
  bool last = true;  // the cell's highest leaf index: the entry the host emitted last
  for (int32_t j = b; j < en; ++j) {
    const double cj = tmp_cov[j];
    const int32_t ij = tmp_i[j];
    rank += (cj > cov || (cj == cov && ij < i)) ? 1 : 0;
    last = last && ij <= i;
  }
  const long long pos = (long long)b + rank;
  if (pos >= en) return;  // (ranks stay inside the cell)
  const int32_t rec = tris[i].rec;
  const LTri lt = record_of(lrec, rec, nnodes, ntri);
  ent[pos] = rec;
  grec[pos] = lt;
  // the host pads before it orders the cells (rt_bins.cpp fill_bins): the
  // padding repeats the last entry EMITTED, the last cell's highest leaf index
  if (en == total && last)
    for (int k = 0; k < kBinPad; ++k) {
      ent[total + k] = rec;
      grec[total + k] = lt;
    }
}

__global__ void k_light_pad(long long total, int32_t fallback, long long nnodes, long long ntri, const LTri* lrec,
                            int32_t* ent, LTri* grec) {
  if ((int)threadIdx.x >= kBinPad || total > 0) return;  // (k_light_order pads a grid with entries)
  const int32_t rec = fallback;
  ent[total + threadIdx.x] = rec;
  grec[total + threadIdx.x] = record_of(lrec, rec, nnodes, ntri);
}

__global__ __launch_bounds__(kBlock) void k_light_sat_rows(const int32_t* off, int gu, int gv, int32_t* sat) {
  const int v = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (v >= gv) return;
  int32_t row = 0;
  for (int u = 0; u < gu; ++u) {
    const long long c = (long long)v * gu + u;
    row += off[c + 1] > off[c] ? 1 : 0;
    sat[(long long)(v + 1) * (gu + 1) + u + 1] = row;
  }
}
__global__ __launch_bounds__(kBlock) void k_light_sat_cols(int gu, int gv, int32_t* sat) {
  const int u = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (u >= gu) return;
  int32_t acc = 0;
  for (int v = 0; v < gv; ++v) {
    const long long k = (long long)(v + 1) * (gu + 1) + u + 1;
    acc += sat[k];
    sat[k] = acc;
  }
}

__global__ __launch_bounds__(kBlock) void k_light_culled(LTri* p, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) p[i] = bg::culled_ltri();
}

unsigned grid_of(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

#define LG_TRY(expr)                     \
  do {                                   \
    const hipError_t e_ = (expr);        \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)
// a DevBuf allocation: these entry points answer with hipError_t values
#define LG_ALLOC(buf, count)                                          \
  do {                                                                \
    if ((buf).alloc(count) != RT_OK) return (int)hipErrorOutOfMemory; \
  } while (0)

// per-pass times of a timed build: events between the passes
struct PassClock {
  bool on;
  hipStream_t st;
  hipEvent_t ev[7] = {};
  int n = 0;
  PassClock(bool timed, hipStream_t s) : on(timed), st(s) {}
  void mark() {
    if (!on || n >= 7) return;
    if (hipEventCreate(&ev[n]) != hipSuccess) {
      on = false;
      return;
    }
    (void)hipEventRecord(ev[n++], st);
  }
  void read(float* ms) {
    for (int k = 0; k + 1 < n; ++k) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
  }
  ~PassClock() {
    for (int k = 0; k < n; ++k) (void)hipEventDestroy(ev[k]);
  }
};

}  // namespace
}  // namespace rtmi

extern "C" int rtmi_lights_scale(const rtmi::DevBinTri* tris, int64_t n, double* scale, void* stream) {
  using namespace rtmi;
  hipStream_t st = (hipStream_t)stream;
  *scale = 1.0;
  if (n <= 0) return 0;
  DevBuf<unsigned long long> red;
  LG_ALLOC(red, RED_WORDS);
  unsigned long long h[RED_WORDS] = {};
  h[RED_SCALE] = key_of(1.0);
  LG_TRY(hipMemcpyAsync(red.p, h, sizeof h, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_light_scale, dim3(grid_of(n)), dim3(kBlock), 0, st, tris, (long long)n, red.p);
  LG_TRY(hipGetLastError());
  LG_TRY(hipMemcpyAsync(h, red.p, sizeof h, hipMemcpyDeviceToHost, st));
  LG_TRY(hipStreamSynchronize(st));
  *scale = double_of(h[RED_SCALE]);
  return 0;
}

extern "C" int rtmi_lights_fill_culled(rtmi::LTri* p, int64_t n, void* stream) {
  using namespace rtmi;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_light_culled, dim3(grid_of(n)), dim3(kBlock), 0, (hipStream_t)stream, p, (long long)n);
  LG_TRY(hipGetLastError());
  return (int)hipStreamSynchronize((hipStream_t)stream);
}

extern "C" void rtmi_lights_free(rtmi::LightGridDev* g) {
  if (g->off) (void)hipFree(g->off);
  if (g->ent) (void)hipFree(g->ent);
  if (g->grec) (void)hipFree(g->grec);
  if (g->sat) (void)hipFree(g->sat);
  g->off = g->ent = g->sat = nullptr;
  g->grec = nullptr;
}

extern "C" int rtmi_light_grid_build(const rtmi::LightGridJob* job, rtmi::LightGridDev* out, int timed,
                                     void* stream) {
  using namespace rtmi;
  hipStream_t st = (hipStream_t)stream;
  std::memset(out, 0, sizeof *out);
  const long long n = job->n;
  bg::LightBasis lb;
  if (n <= 0 || !bg::light_basis(job->w2o, job->dir, &lb)) return 0;
  const double delta = 1e-5 * job->scale;
  PassClock clock(timed != 0, st);
  // 1. faces
  DevBuf<double> proj, box;
  DevBuf<unsigned long long> red;
  LG_ALLOC(proj, (size_t)n * 6);
  LG_ALLOC(box, (size_t)n * 4);
  LG_ALLOC(red, RED_WORDS);
  unsigned long long h[RED_WORDS] = {};
  h[RED_UMIN] = h[RED_VMIN] = key_of(INFINITY);
  h[RED_UMAX] = h[RED_VMAX] = key_of(-INFINITY);
  LG_TRY(hipMemcpyAsync(red.p, h, sizeof h, hipMemcpyHostToDevice, st));
  clock.mark();
  hipLaunchKernelGGL(k_light_faces, dim3(grid_of(n)), dim3(kBlock), 0, st, job->tris, n, lb, delta, proj.p, box.p,
                     red.p);
  LG_TRY(hipGetLastError());
  LG_TRY(hipMemcpyAsync(h, red.p, sizeof h, hipMemcpyDeviceToHost, st));
  LG_TRY(hipStreamSynchronize(st));
  const long long kept = (long long)h[RED_KEPT];
  LightGrid g{};
  bg::light_grid_header(lb, job->scale, kept, double_of(h[RED_UMIN]), double_of(h[RED_UMAX]), double_of(h[RED_VMIN]),
                        double_of(h[RED_VMAX]), job->density, &g);
  const long long ncell = (long long)g.gu * g.gv;
  // 2. count
  clock.mark();
  DevBuf<int32_t> cnt, off;
  LG_ALLOC(cnt, (size_t)ncell + 1);
  LG_ALLOC(off, (size_t)ncell + 1);
  LG_TRY(hipMemsetAsync(cnt.p, 0, ((size_t)ncell + 1) * sizeof(int32_t), st));
  long long total = 0;
  if (kept > 0) {
    hipLaunchKernelGGL(k_light_pairs<false>, dim3(grid_of(n)), dim3(kBlock), 0, st, n, g, delta, proj.p, box.p, cnt.p,
                       (const int32_t*)nullptr, 0LL, (int32_t*)nullptr, (double*)nullptr, (int32_t*)nullptr, red.p);
    LG_TRY(hipGetLastError());
    LG_TRY(hipMemcpyAsync(h, red.p, sizeof h, hipMemcpyDeviceToHost, st));
    LG_TRY(hipStreamSynchronize(st));
    total = (long long)h[RED_TOTAL];
    if (total + kBinPad > (long long)std::numeric_limits<int32_t>::max()) return 0;  // "too many bin entries"
  }
  // 3. offsets
  clock.mark();
  {
    size_t bytes = 0;
    LG_TRY(rocprim::exclusive_scan(nullptr, bytes, cnt.p, off.p, 0, (size_t)ncell + 1, rocprim::plus<int32_t>(), st));
    DevBuf<unsigned char> tmp;
    LG_ALLOC(tmp, bytes);
    LG_TRY(rocprim::exclusive_scan(tmp.p, bytes, cnt.p, off.p, 0, (size_t)ncell + 1, rocprim::plus<int32_t>(), st));
    LG_TRY(hipStreamSynchronize(st));  // tmp goes
  }
  // 4. this light's records
  clock.mark();
  hipLaunchKernelGGL(k_light_lrec, dim3(grid_of(n)), dim3(kBlock), 0, st, job->tris, n, lb.rd[0], lb.rd[1], lb.rd[2],
                     (long long)job->nnodes, (long long)job->ntri, job->lrec);
  LG_TRY(hipGetLastError());
  // 5. fill, order, pad
  clock.mark();
  const size_t nent = (size_t)total + kBinPad;
  DevBuf<int32_t> ent, tmp_i, tmp_cell, sat;
  DevBuf<double> tmp_cov;
  DevBuf<LTri> grec;
  LG_ALLOC(ent, nent);
  LG_ALLOC(grec, nent);
  if (total > 0) {
    LG_ALLOC(tmp_i, (size_t)total);
    LG_ALLOC(tmp_cell, (size_t)total);
    LG_ALLOC(tmp_cov, (size_t)total);
    LG_TRY(hipMemsetAsync(cnt.p, 0, ((size_t)ncell + 1) * sizeof(int32_t), st));
    LG_TRY(hipMemsetAsync(tmp_i.p, 0, (size_t)total * sizeof(int32_t), st));
    LG_TRY(hipMemsetAsync(tmp_cell.p, 0xff, (size_t)total * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_light_pairs<true>, dim3(grid_of(n)), dim3(kBlock), 0, st, n, g, delta, proj.p, box.p, cnt.p,
                       off.p, total, tmp_i.p, tmp_cov.p, tmp_cell.p, red.p);
    LG_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_light_order, dim3(grid_of(total)), dim3(kBlock), 0, st, total, tmp_i.p, tmp_cov.p, tmp_cell.p,
                       off.p, job->tris, n, ncell, job->lrec, (long long)job->nnodes, (long long)job->ntri, ent.p, grec.p);
    LG_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_light_pad, dim3(1), dim3(64), 0, st, total, kept > 0 ? 0 : job->rec0, (long long)job->nnodes,
                     (long long)job->ntri, job->lrec, ent.p, grec.p);
  LG_TRY(hipGetLastError());
  // 6. occupancy prefix sums
  clock.mark();
  const size_t nsat = (size_t)(g.gu + 1) * (size_t)(g.gv + 1);
  LG_ALLOC(sat, nsat);
  LG_TRY(hipMemsetAsync(sat.p, 0, nsat * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_light_sat_rows, dim3(grid_of(g.gv)), dim3(kBlock), 0, st, off.p, g.gu, g.gv, sat.p);
  LG_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_light_sat_cols, dim3(grid_of(g.gu)), dim3(kBlock), 0, st, g.gu, g.gv, sat.p);
  LG_TRY(hipGetLastError());
  clock.mark();
  LG_TRY(hipStreamSynchronize(st));
  clock.read(out->ms);
  out->built = 1;
  out->g = g;
  out->off = off.take();
  out->ent = ent.take();
  out->grec = grec.take();
  out->sat = sat.take();
  out->noff = ncell + 1;
  out->nent = (int64_t)nent;
  out->nsat = (int64_t)nsat;
  return 0;
}
