// rt_aov64.h — the float64 feature-buffer kernels (rt_kernels_aov64.hip,
// rt_render_aovs_f64*): their second kernel argument and launch interface.
#pragma once
#include <cstdint>

#include "rt_common.h"

namespace rtmi {

// The outputs of a float64 feature-buffer call (all pointers device memory):
// the kernels' second argument, after the RenderParams<double> (which keeps
// its layout). The six channels are rt_aov_buffers64's (width * height
// elements, x 3 for normal and albedo; nullptr: not wanted).
struct Aov64Params {
  double* alpha;
  double* depth;
  int32_t* object;
  int32_t* face;
  double* normal;
  double* albedo;
  const double* obj_albedo;  // nobj * 3: rt_object_desc.albedo as given (rt_scene::albedo64)
};

}  // namespace rtmi

extern "C" {
// px: 0 one lane per pixel (k_aov64_lane), 1 one pixel per wave (k_aov64_px)
int rtmi_launch_aov_f64(const rtmi::RenderParams<double>* p, const rtmi::Aov64Params* q, int px, int blocks,
                        void* stream);
// resident blocks per CU of k_aov64_px (its grid: one wave per resident slot)
int rtmi_aov64_blocks_per_cu();
// pixels per wave batch of k_aov64_px (the grid covers nbatch = pixels / P)
int rtmi_aov64_batch();
}
