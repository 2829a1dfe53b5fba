// rt_objgrid_gpu.hip — the object light grids' cell masks, built on the
// device (rt_objgrid_gpu.h). One launch covers every light: blockIdx.y is the
// grid, a block's 256 threads take 256 consecutive cells of it (row-major, as
// the masks lie), and each thread writes its cell's 64-bit mask with one
// coalesced store.
//
// The object loop is the same for every lane of a block: the records are read
// at addresses that do not depend on the lane (scalar loads), an object whose
// rectangle misses all of the block's rows is skipped with one compare before
// its hull is touched, and a lane inside the rectangle runs the host's
// hull_meets_box on the host's cell bounds — the same expressions in the same
// order, compiled without contraction, so every mask equals the host's.
#include <hip/hip_runtime.h>

#include "rt_bins_geom.h"
#include "rt_objgrid_gpu.h"

namespace rtmi {
namespace {

constexpr int kBlock = 256;

// rt_bins.cpp hull_meets_box on the record's precomputed extent and edges
__device__ inline bool hull_meets_cell(const ObjGridRec& r, double u0, double v0, double u1, double v1) {
  if (r.pu1 < u0 || r.pu0 > u1 || r.pv1 < v0 || r.pv0 > v1) return false;
  for (int i = 0; i < r.nh; ++i) {
    const double nx = r.edge[i][0], ny = r.edge[i][1], lim = r.edge[i][2];
    const double m = bg::dmin(bg::dmin(nx * u0 + ny * v0, nx * u1 + ny * v0), bg::dmin(nx * u0 + ny * v1, nx * u1 + ny * v1));
    if (m > lim) return false;
  }
  return true;
}

__global__ __launch_bounds__(kBlock) void k_object_grids(const ObjGridLight* __restrict__ lights,
                                                         const ObjGridRec* __restrict__ recs,
                                                         unsigned long long off_grid,
                                                         unsigned long long* __restrict__ masks) {
  const ObjGridLight& L = lights[blockIdx.y];
  const int gu = L.gu, ncell = L.gu * L.gv;
  const int first = (int)blockIdx.x * kBlock;
  if (first >= ncell) return;  // (the launch is sized by the largest grid)
  const int last = min(first + kBlock, ncell) - 1;
  const int row_lo = first / gu, row_hi = last / gu;
  const int cell = first + (int)threadIdx.x;
  const bool live = cell < ncell;
  const int rr = cell / gu, cc = cell - rr * gu;
  const double hc = L.hc, delta = L.delta;
  const double cu0 = L.u0 + cc * hc - delta, cv0 = L.v0 + rr * hc - delta;
  const double cu1 = cu0 + hc + 2 * delta, cv1 = cv0 + hc + 2 * delta;
  unsigned long long mask = off_grid;
  const ObjGridRec* rec = recs + L.rec_base;
  for (int k = 0; k < L.nrec; ++k) {
    const ObjGridRec& r = rec[k];
    if (r.r1 < row_lo || r.r0 > row_hi) continue;  // no lane's row: uniform
    if (live && rr >= r.r0 && rr <= r.r1 && cc >= r.c0 && cc <= r.c1 &&
        (r.nh < 3 || hull_meets_cell(r, cu0, cv0, cu1, cv1)))
      mask |= 1ull << r.obj;
  }
  if (live) masks[(size_t)L.mask_base + (size_t)cell] = mask;
}

}  // namespace
}  // namespace rtmi

extern "C" int rtmi_object_grids_build(const rtmi::ObjGridLight* lights, int32_t nl, int32_t max_cells,
                                       const rtmi::ObjGridRec* recs, unsigned long long off_grid,
                                       unsigned long long* masks, void* stream) {
  using namespace rtmi;
  if (nl <= 0 || max_cells <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  // blockIdx.y holds at most 65535 grids per launch
  for (int32_t l0 = 0; l0 < nl; l0 += 65535) {
    const dim3 grid((unsigned)((max_cells + kBlock - 1) / kBlock), (unsigned)(nl - l0 < 65535 ? nl - l0 : 65535));
    hipLaunchKernelGGL(k_object_grids, grid, dim3(kBlock), 0, st, lights + l0, recs, off_grid, masks);
    if (hipError_t e = hipGetLastError()) return (int)e;
  }
  return (int)hipStreamSynchronize(st);
}
