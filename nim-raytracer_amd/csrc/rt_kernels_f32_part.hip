// rt_kernels_f32_part.hip — the float32 render kernel specialised for scene
// feature subsets (rt_fast.h F_* bits). Compiled 16 times (Makefile,
// -DRTMI_PART=0..15), each object instantiating 8 of the 128 subsets of
// {sphere, box, mesh, general transform, point light, reflection,
// stochastic sampling}; the plane is always included. The host launches the exact subset a scene uses
// (rtmi.cpp scene_features), so e.g. the mesh + plane scenes of C3-C5 run
// without the sphere / box / rotation / point-light / reflection code paths
// (fewer branches, fewer SALU, 66 instead of 72+ VGPRs).
#include "rt_fast.h"
#include "rt_fast_aov.h"
#include "rt_fast_query.h"
#include "rt_fast_shade.h"

#ifndef RTMI_PART
#error "compile with -DRTMI_PART=<0..15>"
#endif

namespace {

using rtmi::FastParams;
namespace f = rtmi::fast;

constexpr unsigned subset_mask(unsigned i) {
  return f::F_PLANE | ((i & 1u) ? f::F_SPHERE : 0u) | ((i & 2u) ? f::F_BOX : 0u) | ((i & 4u) ? f::F_MESH : 0u) |
         ((i & 8u) ? f::F_XF_GENERAL : 0u) | ((i & 16u) ? f::F_POINT : 0u) | ((i & 32u) ? f::F_REFLECT : 0u) |
         ((i & 64u) ? f::F_STOCHASTIC : 0u);
}

// the lean-pixel and batched general-pixel kernels exist for the subsets
// whose scenes can have lean pixels: a mesh, no reflection, no point light
// (rt_render.cpp: the two-class launch)
constexpr bool has_lean(unsigned i) { return (i & 4u) && !(i & 32u) && !(i & 16u); }
// the reflection-compacting kernel exists for the reflective subsets
constexpr bool has_wave(unsigned i) { return (i & 32u) != 0u; }
// the float32 radiance-query kernel reads its rays from memory: it exists for
// the subsets without stochastic sampling
constexpr bool has_shade(unsigned i) { return (i & 64u) == 0u; }
// the float32 ray-query kernel depends on the geometry bits alone: it exists
// for the 16 subsets of {sphere, box, mesh, general transform} (parts 0 and 1)
constexpr bool has_trace(unsigned i) { return i < 16u; }
// the feature-buffer kernel traces camera rays and shades nothing: it exists
// for the same 16 subsets with and without stochastic sampling (parts 0, 1, 8, 9)
constexpr bool has_aov(unsigned i) { return (i & 48u) == 0u; }

// The host address of kernel (family, subset I), null where the family has
// none for the subset. Taking an address instantiates the kernel.
template <unsigned I>
const void* kernel_of(int family) {
  constexpr unsigned F = subset_mask(I);
  switch (family) {
    case rtmi::K32_FAST:
      return (const void*)f::k_render_fast<false, F>;
    case rtmi::K32_LEAN:
      if constexpr (has_lean(I)) return (const void*)f::k_render_lean<F>;
      break;
    case rtmi::K32_GEN:
      if constexpr (has_lean(I)) return (const void*)f::k_render_gen<F>;
      break;
    case rtmi::K32_WAVE:
      if constexpr (has_wave(I)) return (const void*)f::k_render_wave<F>;
      break;
    case rtmi::K32_SHADE:
      if constexpr (has_shade(I)) return (const void*)f::k_shade_rays_f32<F>;
      break;
    case rtmi::K32_TRACE:
      if constexpr (has_trace(I)) return (const void*)f::k_trace_rays_f32<F>;
      break;
    case rtmi::K32_AOV:
      if constexpr (has_aov(I)) return (const void*)f::k_render_aov<F>;
      break;
  }
  return nullptr;
}

constexpr unsigned B = RTMI_PART * 8u;

}  // namespace

#define RTMI_CAT2(a, b) a##b
#define RTMI_CAT(a, b) RTMI_CAT2(a, b)

// kernel (family, subset index i) of this part's 8 subsets; i >> 3 selects the part
extern "C" const void* RTMI_CAT(rtmi_f32_kernel_part, RTMI_PART)(int family, unsigned i) {
  static const void* (*const kOf[8])(int) = {kernel_of<B + 0>, kernel_of<B + 1>, kernel_of<B + 2>, kernel_of<B + 3>,
                                             kernel_of<B + 4>, kernel_of<B + 5>, kernel_of<B + 6>, kernel_of<B + 7>};
  return kOf[i & 7u](family);
}
