// rt_lights_gpu.h — device builder of the distant lights' mesh grids
// (rt_scene_set_lights). One call builds one light's grid from the scene's
// resident faces (rt_frame.h DevBinTri, leaf order) into device buffers of
// its own: what rt_bins.cpp build_light_grid + grid_occupancy and rt_scene_lights.cpp's
// record loops (make_ltri, the cell-order gather) produce on the host, byte
// for byte — both sides call rt_bins_geom.h's functions, compiled without
// contraction.
#pragma once
#include <stdint.h>

#include "rt_common.h"
#include "rt_frame.h"

namespace rtmi {

struct LightGridJob {
  const DevBinTri* tris;   // device, n faces
  int64_t n;
  int32_t rec0;            // tris[0].rec (the empty grid's padding entries)
  double w2o[16];          // the mesh object's world_to_object
  double dir[3];           // the light's travel direction (world)
  double scale;            // rtmi_lights_scale
  double density;          // rt_bins.h light_grid_density
  int64_t nnodes, ntri;    // a face's record slot: rec / sizeof(TriFast) - nnodes, in [0, ntri)
  LTri* lrec;              // device, this light's ntri slots (pre-filled with the culled record)
};

// Device buffers of one built grid; the caller owns them (rtmi_lights_free).
struct LightGridDev {
  int32_t built;           // 0: no grid for this light (degenerate direction, too many entries)
  LightGrid g;             // off_base / ent_base left 0
  int32_t* off;            // gu * gv + 1
  int32_t* ent;            // nent: the cells' entries, then kBinPad padding entries
  LTri* grec;              // nent: lrec in entry order
  int32_t* sat;            // (gu + 1) * (gv + 1) occupancy prefix sums
  int64_t noff, nent, nsat;
  float ms[6];             // per pass (faces, count, scan, records, fill + order, prefix sums); timed only
};

}  // namespace rtmi

// hipError_t values (0: fine). All three wait for their work before returning.
extern "C" int rtmi_lights_scale(const rtmi::DevBinTri* tris, int64_t n, double* scale, void* stream);
extern "C" int rtmi_lights_fill_culled(rtmi::LTri* p, int64_t n, void* stream);
extern "C" int rtmi_light_grid_build(const rtmi::LightGridJob* job, rtmi::LightGridDev* out, int timed, void* stream);
extern "C" void rtmi_lights_free(rtmi::LightGridDev* g);
