// rt_fast_shade.h — float32 radiance queries (include/rtmi.h
// rt_shade_rays_f32*): the float32 render's colour along caller-supplied
// rays. On top of rt_fast_trace.h: shade_path with rays read from memory
// instead of formed from the scene's camera.
#pragma once
#include "rt_fast.h"

namespace rtmi {
namespace fast {

// Occupancy of k_shade_rays_f32: the family defaults of k_render_fast, lowered
// per subset to the highest occupancy without spills (rt_occupancy.h
// kOcc_shade, tools/occupancy_table.py).
template <unsigned F>
constexpr unsigned shade_waves() {
#ifdef RTMI_WAVES_PER_EU
  return RTMI_WAVES_PER_EU;
#else
  return occ_table<F>(kOcc_shade, ((F & F_MESH) && !(F & (F_POINT | F_REFLECT))) ? RTMI_MESH_WAVES
                                                                                  : RTMI_ANALYTIC_WAVES);
#endif
}

// ---- k_shade_rays_f32 -------------------------------------------------------
// One ray per lane, 64 consecutive slots of the (sorted) batch per wave and
// step, grid-stride over the waves of a grid sized by residency, as
// k_shade_rays: every wave owns one row of p->partials. Ray i is shaded by
// shade_path<false, F> — k_render_fast's one-sample path — with pix = -1 and
// pinfo = kPixCount: no pixel list, object mask or pixel record is reachable
// (trace reads p->obj_pix and p->pix_slots behind pix >= 0, mesh_search reads
// p->pix_cnt behind a pixel list; pinfo >> 24 == 0 takes no shadow skip and
// (pinfo & kPixCount) != 0 rules no mesh out). The FastParams carry the scene
// words only (rt_render.cpp fast_scene_words), bias, max_depth and partials.
//
// shade_path is wave-coherent, so EVERY lane reaches it at every step: slots
// past n and degenerate rays (a non-finite component, an all-zero direction)
// go in with active = false holding a finite dummy ray, and no lane leaves
// the loop early (its bounds are wave-uniform). An inactive lane adds nothing
// to the Stats (popcounts of ballots over `active`).
//
// The rays are read with per-lane vector loads (cp() / at() are for
// wave-uniform addresses). The 32-bit wave counters are flushed every step:
// a step adds at most 64 x levels x (1 + lights) x objects to any of them.
template <unsigned F>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(shade_waves<F>()))) void
k_shade_rays_f32(const FastParams params_by_value, const Shade32Params q) {
  (void)params_by_value;  // read through params() (kernarg segment)
  KP p = params();
  __shared__ float lds[4][lds_slots<F>()][64];          // 4 waves per 256-thread block
  __shared__ unsigned long long lds_tot[4][kStatSlots];  // per-wave 64-bit Stats totals
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  LdsF* ls = (LdsF*)&lds[wib][0][__lane_id()];
  Stats32 ws;
  RT_STATS_BEGIN(lds_tot, wib, __lane_id(), ws);
  const long long wave = (long long)blockIdx.x * 4 + wib;
  const long long nwaves = (long long)gridDim.x * 4;
  const long long nsteps = (q.n + 63) >> 6;
  for (long long b = wave; b < nsteps; b += nwaves) {
    p = params();
    const int lane = lane_id_fresh();
    const long long slot = (b << 6) + lane;
    const bool in = slot < q.n;
    const long long i = in ? (q.order ? (long long)q.order[slot] : slot) : 0;
    F3 o = f3(0.0f, 0.0f, 0.0f), d = f3(0.0f, 0.0f, 1.0f);
    if (in) {
      const float* po = q.orig + 3 * i;
      const float* pd = q.dir + 3 * i;
      o = f3(po[0], po[1], po[2]);
      d = f3(pd[0], pd[1], pd[2]);
    }
    const bool finite = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) &&
                        __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z);
    const bool zero = d.x == 0.0f && d.y == 0.0f && d.z == 0.0f;
    const bool ok = in && finite && !zero;
    if (!ok) {  // a masked lane computes along with the wave: give it finite operands
      o = f3(0.0f, 0.0f, 0.0f);
      d = f3(0.0f, 0.0f, 1.0f);
    }
    ws.v[STAT_PRIMARY] += pc(bal(ok));
    Acc acc;
    acc.v = f3(0.0f, 0.0f, 0.0f);
    shade_path<false, F>(p, o, d, ok, -1, kPixCount, ls, acc, ws);
    if (in) {
      float* out = q.rgb + 3 * i;
      out[0] = ok ? acc.v.x : 0.0f;  // a degenerate ray's colour: +0
      out[1] = ok ? acc.v.y : 0.0f;
      out[2] = ok ? acc.v.z : 0.0f;
    }
    flush_stats(ws, lds_tot[wib], lane_id_fresh());
  }
  stats_end(params(), ws, lds_tot, wib);
}

}  // namespace fast
}  // namespace rtmi
