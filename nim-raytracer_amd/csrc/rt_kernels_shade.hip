// rt_kernels_shade.hip — radiance queries (include/rtmi.h rt_shade_rays*):
// shade(ray, trace(ray, scene.objects, +inf)) (renderer.nim:47-127) for
// caller-supplied rays, in the float64 arithmetic of the parity render. Built
// with -ffp-contract=off like rt_kernels_f64.hip and rt_kernels_query.hip, so
// every operation rounds as the reference's (and the oracle's) does.
#include "rt_device.h"
#include "rt_query.h"
#include "rt_query_rays.h"

namespace rtmi {

// ---- k_shade_rays -----------------------------------------------------------
// One ray per lane, 64 consecutive slots of the (sorted) batch per wave and
// step, grid-stride over the waves of a grid sized by the device, as
// k_trace_rays; ray i is read by query_ray's rules and shaded by
// shade_path<double, false, false, LEVELS> — the path of k_render<double>.
//
// Nothing of the scene's own camera is read. With LISTS = false, trace()
// compiles neither obj_ray's cache reads (cached_o / cached_d are
// `LISTS && ...`) nor mesh_lists (pixel slots, light grids, sh64 records):
// every mesh search is traverse(), and shade_path's one other cache read
// (the plane normal) is `LISTS && cache`. The defaults pinfo = kPixCount,
// pix = -1, cache = nullptr make cam_skip and sh_skip false, so no pixel
// record rules a mesh out. The RenderParams carry the objects, lights,
// meshes, BVH, bg, bias and max_depth only (rt_queries.cpp fill_query).
//
// shade_path and trace are wave-coherent — ballots, readlane, the traversal
// stack's entry i in lane i — so EVERY lane of a wave reaches every call:
// slots past n and degenerate rays go in with active = false (holding a
// harmless finite ray), and no lane leaves the loop early (its bounds are
// wave-uniform). An inactive lane adds nothing to the Stats (popcounts of
// ballots over `active`) and its colour is never used.
//
// LEVELS = 1: no reflection ray can follow the first hit (no reflective
// material, or max_depth < 1); kMaxShadeLevels otherwise, with shade_path's
// per-level colour state. No occupancy is asked for: left to itself the
// compiler takes 138 VGPRs (3 waves per SIMD) for the first and 222 (2 waves,
// where k_render_px64 pins its reflective form) for the second, neither with
// scratch; asked for 4 waves both spill (DESIGN.md "Radiance queries").
template <int LEVELS>
__global__ __launch_bounds__(256) void k_shade_rays(const RenderParams<double> params_by_value, const QueryParams q,
                                                    const ShadeOut so) {
  using R = double;
  (void)params_by_value;  // read through rparams()
  const RT_CONST RenderParams<R>& p = rparams<R>();
  const int lane = (int)__lane_id();
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + wib;
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const long long nsteps = (q.n + 63) >> 6;
  WaveStats ws;
#pragma unroll
  for (int k = 0; k < kStatSlots; ++k) ws.v[k] = 0u;
  unsigned long long tot = 0ull;

  for (long long b = wave; b < nsteps; b += nwaves) {
    const long long slot = (b << 6) + lane;
    const bool in = slot < q.n;
    const long long i = in ? (q.order ? (long long)q.order[slot] : slot) : 0;
    V3<R> o{R(0), R(0), R(0)}, d{R(0), R(0), R(1)};
    R tn = pinf<R>();
    bool ok = false;
    if (in) ok = query_ray(p, q, i, o, d, tn);
    if (!ok) {  // a masked lane computes along with the wave: give it finite operands
      o = V3<R>{R(0), R(0), R(0)};
      d = V3<R>{R(0), R(0), R(1)};
    }
    ws.v[STAT_PRIMARY] += popc32(ballot(ok));
    V3<R> c = shade_path<R, false, false, LEVELS>(rparams<R>(), o, d, ok, ws);
    if (!ok) c = V3<R>{R(0), R(0), R(0)};  // a degenerate ray's colour
    if (in) {
      if (so.rgb) {
        R* out = so.rgb + 3 * i;
        out[0] = c.x; out[1] = c.y; out[2] = c.z;
      }
      if (so.rgb32) {
        float* out = so.rgb32 + 3 * i;
        out[0] = (float)c.x; out[1] = (float)c.y; out[2] = (float)c.z;
      }
    }
    flush_stats(ws, tot, lane);
  }
  if (lane < kStatSlots) q.partials[wave * kStatSlots + lane] = tot;
}

// calcPixel's sum (renderer.nim:147-159) over each run of `group` ray
// colours: from vec3(0), the colours added in index order — one thread per
// output walks its run, never a tree, so the sum rounds as the reference's —
// then one multiplication by inv_len = 1.0 / group.
__global__ __launch_bounds__(256) void k_shade_reduce(const double* ray_rgb, long long ngroups, int group,
                                                      double inv_len, double* rgb, float* rgb32) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ngroups) return;
  const double* c = ray_rgb + 3 * k * group;
  double x = 0.0, y = 0.0, z = 0.0;
  for (int j = 0; j < group; ++j) {
    x = x + c[3 * j];
    y = y + c[3 * j + 1];
    z = z + c[3 * j + 2];
  }
  x = x * inv_len;
  y = y * inv_len;
  z = z * inv_len;
  if (rgb) {
    rgb[3 * k] = x; rgb[3 * k + 1] = y; rgb[3 * k + 2] = z;
  }
  if (rgb32) {
    rgb32[3 * k] = (float)x; rgb32[3 * k + 1] = (float)y; rgb32[3 * k + 2] = (float)z;
  }
}

template __global__ void k_shade_rays<1>(const RenderParams<double>, const QueryParams, const ShadeOut);
template __global__ void k_shade_rays<kMaxShadeLevels>(const RenderParams<double>, const QueryParams, const ShadeOut);

}  // namespace rtmi

extern "C" int rtmi_shade_blocks_per_cu(int reflective) {
  int n = 0;
  const void* k = reflective ? (const void*)rtmi::k_shade_rays<rtmi::kMaxShadeLevels> : (const void*)rtmi::k_shade_rays<1>;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 256, 0) != hipSuccess) return 0;
  return n;
}

extern "C" int rtmi_launch_shade(const rtmi::RenderParams<double>* p, const rtmi::QueryParams* q,
                                 const rtmi::ShadeOut* so, int reflective, int blocks, void* stream) {
  if (reflective)
    hipLaunchKernelGGL((rtmi::k_shade_rays<rtmi::kMaxShadeLevels>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p,
                       *q, *so);
  else
    hipLaunchKernelGGL((rtmi::k_shade_rays<1>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, *q, *so);
  return (int)hipGetLastError();
}

extern "C" int rtmi_launch_shade_reduce(const double* ray_rgb, long long ngroups, int group, double inv_len, double* rgb,
                                        float* rgb32, void* stream) {
  const unsigned blocks = (unsigned)((ngroups + 255) / 256);
  hipLaunchKernelGGL(rtmi::k_shade_reduce, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ray_rgb, ngroups, group,
                     inv_len, rgb, rgb32);
  return (int)hipGetLastError();
}
