// rt_fast_query.h — float32 ray queries and picks (include/rtmi.h
// rt_trace_rays_f32* / rt_pick_pixels_f32*): what the float32 render's trace
// answers for caller-supplied rays, and for the rays the RT_FP32 render forms
// at caller-supplied image positions. On top of rt_fast_trace.h, beside
// rt_fast_shade.h: trace with rays read from memory, the hit written out
// instead of shaded.
#pragma once
#include "rt_fast.h"

namespace rtmi {
namespace fast {

// Occupancy of k_trace_rays_f32: the family defaults of k_render_fast, lowered
// per subset to the highest occupancy without spills (rt_occupancy.h
// kOcc_trace, tools/occupancy_table.py).
template <unsigned F>
constexpr unsigned trace_waves() {
#ifdef RTMI_WAVES_PER_EU
  return RTMI_WAVES_PER_EU;
#else
  return occ_table<F>(kOcc_trace, (F & F_MESH) ? RTMI_MESH_WAVES : RTMI_ANALYTIC_WAVES);
#endif
}

// ---- k_trace_rays_f32 -------------------------------------------------------
// One ray per lane, 64 consecutive slots of the (sorted) batch per wave and
// step, grid-stride over the waves of a grid sized by residency, as
// k_shade_rays_f32: every wave owns one row of p->partials. Ray i is traced by
// trace<false, F> with pix = -1 and light = -1: no pixel list, object mask or
// light grid is reachable, a mesh's faces are searched through the BVH on
// their TriFast records. RT_QUERY_ANY_HIT calls it as a shadow ray does
// (shadow = true: the exact early exit of scenes with one mesh). F holds
// geometry bits only — trace reads no other. The FastParams carry the scene
// words (rt_render.cpp fast_scene_words), partials, and for picks the camera
// constants of fast_camera: a pick's ray is the render's own, from the camera
// origin p->cam[0..2] along camera_ray_dir(p, x, y).
//
// trace is wave-coherent, so EVERY lane reaches it at every step: slots past
// n and degenerate rays (a non-finite component, an all-zero direction, a NaN
// t_near) go in with active = false holding a finite dummy ray, and no lane
// leaves the loop early (its bounds are wave-uniform). An inactive lane adds
// nothing to the Stats (popcounts of ballots over `active`).
//
// Any-hit, normals and picks are wave-uniform run-time branches. The rays are
// read with per-lane vector loads (cp() / at() are for wave-uniform
// addresses), a hit is written as one 16-byte vector store. The 32-bit wave
// counters are flushed every step: a step adds at most 64 x objects to one.
template <unsigned F>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(trace_waves<F>()))) void
k_trace_rays_f32(const FastParams params_by_value, const Trace32Params q) {
  (void)params_by_value;  // read through params() (kernarg segment)
  KP p = params();
  __shared__ unsigned long long lds_tot[4][kStatSlots];  // per-wave 64-bit Stats totals
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  Stats32 ws;
  RT_STATS_BEGIN(lds_tot, wib, __lane_id(), ws);
  const long long wave = (long long)blockIdx.x * 4 + wib;
  const long long nwaves = (long long)gridDim.x * 4;
  const long long nsteps = (q.n + 63) >> 6;
  const bool shadow = q.any_hit != 0;
  for (long long b = wave; b < nsteps; b += nwaves) {
    p = params();
    const int lane = lane_id_fresh();
    const long long slot = (b << 6) + lane;
    const bool in = slot < q.n;
    const long long i = in ? (q.order ? (long long)q.order[slot] : slot) : 0;
    F3 o = f3(0.0f, 0.0f, 0.0f), d = f3(0.0f, 0.0f, 1.0f);
    float tn_given = finf();
    if (q.xy) {  // a pick: the RT_FP32 render's camera ray at the float image position
      float px = 0.0f, py = 0.0f;
      if (in) {
        px = q.xy[2 * i];
        py = q.xy[2 * i + 1];
      }
      o = f3(p->cam[0], p->cam[1], p->cam[2]);
      d = camera_ray_dir(p, px, py);  // a non-finite position leaves a non-finite direction
    } else if (in) {
      const float* po = q.orig + 3 * i;
      const float* pd = q.dir + 3 * i;
      o = f3(po[0], po[1], po[2]);
      d = f3(pd[0], pd[1], pd[2]);
      if (q.tnear) tn_given = q.tnear[i];
    }
    const bool finite = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) &&
                        __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z);
    const bool zero = d.x == 0.0f && d.y == 0.0f && d.z == 0.0f;
    const bool ok = in && finite && !zero && !(tn_given != tn_given);
    if (!ok) {  // a masked lane computes along with the wave: give it finite operands
      o = f3(0.0f, 0.0f, 0.0f);
      d = f3(0.0f, 0.0f, 1.0f);
    }
    const float tn = ok ? tn_given : finf();
    ws.v[STAT_PRIMARY] += pc(bal(ok));
    const Hit h = trace<false, F>(p, o, d, tn, ok, shadow, -1, -1, ws);
    const bool lit = ok && h.obj >= 0;
    if (q.normals) {
      // shade_level's N (rt_fast_trace.h), gathered per distinct object hit by
      // the wave so the object records are read with scalar loads
      const F3 hw = f3(__builtin_fmaf(d.x, h.t, o.x), __builtin_fmaf(d.y, h.t, o.y), __builtin_fmaf(d.z, h.t, o.z));
      F3 N = f3(0.0f, 0.0f, 0.0f);
      unsigned long long pending = bal(lit);
      while (pending) {
        const int lead = (int)__builtin_ctzll(pending);
        const int oi = __builtin_amdgcn_readlane(h.obj, lead);
        // `mine` compares against an opaque copy, as in shade_level: the
        // object's uniform records stay on scalar loads
        int oi_cmp = oi;
        asm volatile("" : "+s"(oi_cmp));
        const bool mine = lit && h.obj == oi_cmp;
        pending &= ~bal(mine);
        const FObj ob = at(p->objs, oi);
        const RT_CONST FObjX& ox = at(p->objx, oi);
        const int nbase = ox.normal_base;
        if (mine) {
          F3 n;
          if ((F & F_MESH) && ob.type == GEOM_MESH) {
            const float* fn = p->normals + 3 * (size_t)(nbase + h.tri);
            n = f3(fn[0], fn[1], fn[2]);
          } else {
            F3 ho, unused;
            to_object<F>(p, ob, oi, hw, f3(0.0f, 0.0f, 0.0f), ho, unused);
            n = analytic_normal<F>(ob, ho);
          }
          if ((F & F_XF_GENERAL) && ob.xf == XF_GENERAL) {  // object_to_world * n, not re-normalised
            const float* m = ox.o2w;
            N = f3(__builtin_fmaf(m[0], n.x, __builtin_fmaf(m[3], n.y, m[6] * n.z)),
                   __builtin_fmaf(m[1], n.x, __builtin_fmaf(m[4], n.y, m[7] * n.z)),
                   __builtin_fmaf(m[2], n.x, __builtin_fmaf(m[5], n.y, m[8] * n.z)));
          } else {
            N = n;
          }
        }
      }
      if (in) {
        float* out = q.normals + 3 * i;
        out[0] = N.x;
        out[1] = N.y;
        out[2] = N.z;
      }
    }
    if (in) {
      // any-hit: only hit / no hit is the answer (t and the face are whatever
      // the early exit stopped at): t echoes t_near
      Hit32 r;
      r.t = (lit && !shadow) ? h.t : tn_given;
      r.obj = lit ? h.obj : -1;
      r.face = (lit && !shadow) ? h.tri : -1;
      r.reserved = 0;
      q.hits[i] = r;
    }
    flush_stats(ws, lds_tot[wib], lane_id_fresh());
  }
  stats_end(params(), ws, lds_tot, wib);
}

}  // namespace fast
}  // namespace rtmi
