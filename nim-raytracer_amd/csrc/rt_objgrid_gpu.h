// rt_objgrid_gpu.h — device builder of the object light grids (rt_bins.h:
// scenes of 4..64 objects, per distant light a grid of 64-bit object masks).
// The host forms, per light, the header and one record per bounded object
// (rt_bins.cpp plan_object_light_grid: its cell rectangle and the edges of its
// projected hull); the device tests every cell against the records and writes
// the cell's mask — what build_object_light_grid's cell loop writes on the
// host, byte for byte (both compiled without contraction).
#pragma once
#include <stdint.h>

namespace rtmi {

// One bounded object of one light's grid.
struct ObjGridRec {
  int32_t c0, c1, r0, r1;  // its cell rectangle, inclusive (empty when c0 > c1 or r0 > r1)
  int32_t nh;              // hull vertices (< 3: every cell of the rectangle takes the object)
  int32_t obj;             // its bit in the masks
  double pu0, pu1, pv0, pv1;  // the hull's extent along e1 / e2
  double edge[8][3];       // per hull edge: outward normal (nx, ny) and nx * a.u + ny * a.v
};
static_assert(sizeof(ObjGridRec) == 248, "ObjGridRec is uploaded as it is");

// One light's grid as the launch reads it.
struct ObjGridLight {
  double u0, v0, hc, delta;  // (double)g.u0, (double)g.v0, 1 / (double)g.inv_h, the boxes' growth
  int32_t gu, gv;
  int32_t mask_base;         // the grid's first mask (LightGrid.off_base)
  int32_t rec_base, nrec;    // its records in the record array
  int32_t pad;
};

}  // namespace rtmi

// Writes mask_base .. mask_base + gu * gv of `masks` for each of the `nl`
// grids: off_grid, with bit rec.obj set for every record whose rectangle holds
// the cell and whose hull meets the cell grown by delta. lights / recs / masks
// are device arrays. Returns a hipError_t (0: fine); waits for its work.
extern "C" int rtmi_object_grids_build(const rtmi::ObjGridLight* lights, int32_t nl, int32_t max_cells,
                                       const rtmi::ObjGridRec* recs, unsigned long long off_grid,
                                       unsigned long long* masks, void* stream);
