// rt_fast_aov.h — per-pixel feature buffers of an RT_FP32 frame (include/rtmi.h
// rt_render_aovs*): coverage, depth, object / face id, normal and albedo over
// the frame's own samples. On top of rt_fast.h, beside rt_fast_query.h:
// k_render_fast's work queue, pixel groups and sample tables, the camera rays
// traced and nothing shaded, the hits reduced per pixel instead of colours.
#pragma once
#include "rt_fast.h"

namespace rtmi {
namespace fast {

// Occupancy of k_render_aov: at least 5 waves per SIMD (<= 96 VGPRs) for every
// subset. The mesh subsets carry the traversal's registers next to the nine
// per-lane accumulators and spilled up to 85 VGPRs at the render family's 7;
// at 5 none spills (profiles/aov/kernel_resources.txt), so there is no table.
template <unsigned F>
constexpr unsigned aov_waves() {
#ifdef RTMI_WAVES_PER_EU
  return RTMI_WAVES_PER_EU;
#else
  return RTMI_ANALYTIC_WAVES;
#endif
}

// ---- reductions over a pixel's L lanes --------------------------------------
// Lane i of the pixel exchanges with lane i ^ 1, i ^ 2 (quad_perm), 7 - i
// (row_half_mirror), 15 - i (row_mirror), i ^ 16 (a bpermute) — each a
// symmetric exchange inside the aligned group of L lanes, so after the steps
// below L every lane of the pixel holds the reduction of all L (a row_ror, as
// finish_item's sums use, would reach into the neighbouring pixel at L = 8).
// One pixel per wave (L = 64): the four rows' results through readlane. The
// order of the operations is fixed by L alone, so a float sum does not depend
// on flags, lists or the data.
template <int CTRL>
__device__ __forceinline__ int dpp_get(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_get(float v) {
  return __int_as_float(dpp_get<CTRL>(__float_as_int(v)));
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_get(unsigned long long v) {
  const unsigned lo = (unsigned)dpp_get<CTRL>((int)(unsigned)v);
  const unsigned hi = (unsigned)dpp_get<CTRL>((int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ int lane_get(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float lane_get(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ unsigned long long lane_get(unsigned long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ int xor16_get(int v) { return __shfl_xor(v, 16); }
__device__ __forceinline__ float xor16_get(float v) { return __shfl_xor(v, 16); }
__device__ __forceinline__ unsigned long long xor16_get(unsigned long long v) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, 16);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), 16);
  return ((unsigned long long)hi << 32) | lo;
}
template <class T, class Op>
__device__ __forceinline__ T pixel_reduce(T v, int L, Op op) {
  if (L >= 2) v = op(v, dpp_get<0xB1>(v));    // quad_perm 1,0,3,2
  if (L >= 4) v = op(v, dpp_get<0x4E>(v));    // quad_perm 2,3,0,1
  if (L >= 8) v = op(v, dpp_get<0x141>(v));   // row_half_mirror
  if (L >= 16) v = op(v, dpp_get<0x140>(v));  // row_mirror
  if (L == 32) v = op(v, xor16_get(v));
  if (L == 64) v = op(op(lane_get(v, 0), lane_get(v, 16)), op(lane_get(v, 32), lane_get(v, 48)));
  return v;
}
struct OpAddI {
  __device__ __forceinline__ int operator()(int a, int b) const { return a + b; }
};
struct OpAddF {
  __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};
struct OpMinU64 {
  __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const {
    return b < a ? b : a;
  }
};
__device__ __forceinline__ F3 pixel_sum3(F3 v, int L) {
  return f3(pixel_reduce(v.x, L, OpAddF{}), pixel_reduce(v.y, L, OpAddF{}), pixel_reduce(v.z, L, OpAddF{}));
}

// A value the compiler may not fuse into the add that follows (mul_nc's
// reason): the sums add the N and albedo a pick returns, rounded as returned.
__device__ __forceinline__ F3 opaque3(F3 v) {
  asm("" : "+v"(v.x), "+v"(v.y), "+v"(v.z));
  return v;
}

// ---- k_render_aov -----------------------------------------------------------
// k_render_fast's skeleton: the grid is the resident waves, each pulls pixel
// groups from the sharded work queue; a group is 64 / L pixels of L lanes,
// lane `sub` of a pixel takes samples sub, sub + L, ... (iters of them) at
// the positions camera_pos forms for the render. Every sample's camera ray
// goes through trace<false, F> as the render's does: with the pixel's face
// list and object mask when this call built them (pix >= 0), the BVH
// otherwise — the same hit either way, which is what rt_pick_pixels_f32
// answers at that position. A one-pixel wave whose record says the list is
// empty skips the mesh (pinfo, as k_render_fast).
//
// Per lane: the hit count, the smallest key (bits of t) << 32 | sample index
// with its object and face, and the float32 sums of N and of the hit object's
// albedo, each from +0 in sample order. N is k_trace_rays_f32's gather, per
// distinct object hit by the wave, so the object records and the albedo are
// scalar loads. Per pixel: pixel_reduce over its lanes; lane sub == 0 stores
// the sums, the lane that holds the winning key stores the ids.
//
// F holds the geometry bits and F_STOCHASTIC — nothing here reads a light or
// a material's reflection. Rows and channels the caller did not ask for are
// never written (q's null pointers; wave-uniform branches).
template <unsigned F>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(aov_waves<F>()))) void
k_render_aov(const FastParams params_by_value, const Aov32Params q) {
  (void)params_by_value;  // read through params() (kernarg segment)
  KP p = params();
  extern __shared__ float sample_lds[];                  // (multi-)jittered tables, sized by the host
  __shared__ unsigned long long lds_tot[4][kStatSlots];  // per-wave 64-bit Stats totals
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  Stats32 ws;
  RT_STATS_BEGIN(lds_tot, wib, __lane_id(), ws);
  const int shard = (int)(blockIdx.x % (unsigned int)p->shards);
  unsigned int* head = p->queue + shard * kQueueStride;
  int qj = 0;
  if (__lane_id() == 0) qj = (int)atomicAdd(head, 1u);
  qj = __builtin_amdgcn_readfirstlane(qj);
  int qj_next = 0;  // the reservation one item ahead (lane 0 holds it)
  if (__lane_id() == 0) qj_next = (int)atomicAdd(head, 1u);
  int g = fast_item(qj, p->shards, shard);
  int nflush = 0;
  const int ngroups = p->ngroups;
  const bool want_n = q.normal != nullptr, want_a = q.albedo != nullptr;
  while (g < ngroups) {
    p = params();
    const int L = p->lanes_per_px;
    const int iters = p->iters;
    const GroupPix gp = group_pixel(p, g, lane_id_fresh());
    LdsF* tb = sample_table<F>(p, gp, sample_lds, wib, L);
    const int pix = gp.valid ? gp.y * p->width + gp.x : -1;
    unsigned pinfo = kPixCount;  // the pixel's record of a one-pixel wave, as k_render_fast reads it
    if ((F & F_MESH) && p->pix_info) {
      const unsigned long long vm = bal(gp.valid);
      if (vm != 0ull) pinfo = at(p->pix_info, __builtin_amdgcn_readlane(pix, (int)__builtin_ctzll(vm)));
    }
    const bool no_mesh = (pinfo & kPixCount) == 0u;
    int nhit = 0, bobj = -1, bface = -1;
    unsigned long long best = ~0ull;
    F3 nsum = f3(0.0f, 0.0f, 0.0f), asum = f3(0.0f, 0.0f, 0.0f);
    for (int it = 0; it < iters; ++it) {
      p = params();
      const int s = it * L + gp.sub;  // this lane's sample index
      const bool sv = gp.valid & (s < p->spp);
      const F3 d = camera_dir<F>(p, gp, s < p->spp ? s : 0, tb);
      const F3 o = f3(p->cam[0], p->cam[1], p->cam[2]);
      ws.v[STAT_PRIMARY] += pc(bal(sv));
      const Hit h = trace<false, F>(p, o, d, finf(), sv, false, sv ? pix : -1, -1, ws, no_mesh);
      const bool lit = sv && h.obj >= 0;
      nhit += lit ? 1 : 0;
      // (+ 0: a hit at -0 keys as +0, below every positive t)
      const unsigned long long key = lit ? tkey(h.t + 0.0f, (unsigned)s) : ~0ull;
      if (key < best) {
        best = key;
        bobj = h.obj;
        bface = h.tri;
      }
      if (want_n || want_a) {
        // shade_level's N and the object's albedo, gathered per distinct
        // object hit by the wave (k_trace_rays_f32's loop)
        const F3 hw = f3(__builtin_fmaf(d.x, h.t, o.x), __builtin_fmaf(d.y, h.t, o.y), __builtin_fmaf(d.z, h.t, o.z));
        F3 N = f3(0.0f, 0.0f, 0.0f), A = f3(0.0f, 0.0f, 0.0f);
        unsigned long long pending = bal(lit);
        while (pending) {
          const int lead = (int)__builtin_ctzll(pending);
          const int oi = __builtin_amdgcn_readlane(h.obj, lead);
          int oi_cmp = oi;  // (an opaque copy: the object's records stay on scalar loads)
          asm volatile("" : "+s"(oi_cmp));
          const bool mine = lit && h.obj == oi_cmp;
          pending &= ~bal(mine);
          const FObj ob = at(p->objs, oi);
          const RT_CONST FObjX& ox = at(p->objx, oi);
          const int nbase = ox.normal_base;
          const RT_CONST float* al = cp(q.obj_albedo) + 3 * oi;
          const float a0 = al[0], a1 = al[1], a2 = al[2];
          if (mine) {
            A = f3(a0, a1, a2);
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
        N = opaque3(N);
        nsum = f3(nsum.x + N.x, nsum.y + N.y, nsum.z + N.z);
        asum = f3(asum.x + A.x, asum.y + A.y, asum.z + A.z);
      }
    }
    p = params();
    const int lane = lane_id_fresh();
    // the pixel's totals, in every one of its lanes
    const int hits = pixel_reduce(nhit, L, OpAddI{});
    const unsigned long long kmin = pixel_reduce(best, L, OpMinU64{});
    if (want_n) nsum = pixel_sum3(nsum, L);
    if (want_a) asum = pixel_sum3(asum, L);
    if (gp.valid) {
      const size_t at_px = (size_t)gp.out_row * (size_t)p->width + (size_t)gp.x;
      const bool none = kmin == ~0ull;
      if (gp.sub == 0) {
        const float il = p->inv_len;
        if (q.alpha) q.alpha[at_px] = (float)hits * il;
        if (q.depth) q.depth[at_px] = none ? finf() : __uint_as_float((unsigned)(kmin >> 32));
        if (want_n) {
          float* o3 = q.normal + 3 * at_px;
          o3[0] = nsum.x * il, o3[1] = nsum.y * il, o3[2] = nsum.z * il;
        }
        if (want_a) {
          float* o3 = q.albedo + 3 * at_px;
          o3[0] = asum.x * il, o3[1] = asum.y * il, o3[2] = asum.z * il;
        }
      }
      // the ids: the one lane whose own best key won (sample indices differ
      // from lane to lane), lane 0 of the pixel when no sample hit
      if (none ? gp.sub == 0 : best == kmin) {
        if (q.object) q.object[at_px] = none ? -1 : bobj;
        if (q.face) q.face[at_px] = none ? -1 : bface;
      }
    }
    // 32-bit wave counters -> the wave's 64-bit LDS totals, every
    // p->stat_flush items (before any counter can wrap) and at the end
    if (++nflush >= p->stat_flush) {
      flush_stats(ws, lds_tot[wib], lane);
      nflush = 0;
    }
    qj = __builtin_amdgcn_readfirstlane(qj_next);
    if (lane == 0) qj_next = (int)atomicAdd(head, 1u);
    g = fast_item(qj, p->shards, shard);
  }
  stats_end(params(), ws, lds_tot, wib);
}

}  // namespace fast
}  // namespace rtmi
