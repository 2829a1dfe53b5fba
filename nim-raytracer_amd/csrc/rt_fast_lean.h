// rt_fast_lean.h — lean_batch (rt_fast.h has the map): batches of samples
// that only visit analytic objects.
#pragma once
#include "rt_fast_batch.h"

namespace rtmi {
namespace fast {

// Lean pixels, kLeanBatch samples per lane at once. A lean pixel (one-pixel
// wave; its pixel list is empty and every light is a distant light whose
// shadow skip bit is set, no reflection: FastParams.pix_info) never touches
// the mesh, so its samples only visit the analytic objects. The per-sample
// loop pays the scalar work of every object visit (record loads, type
// dispatch, loop control, hit-count popcounts: the CU's one scalar unit,
// shared by its 32 resident waves, is the kernel's busiest pipe) once per 64
// rays; here each lane carries kLeanBatch samples through the same object
// and light loops, so that work is paid once per 64 x kLeanBatch rays. Same
// arithmetic per sample as shade_path (camera_dir, analytic_t, the
// irradiance sum), the samples' colours added to the pixel in sample order:
// frames bit-identical to the one-sample loop (tests: binned vs
// RT_FLAG_NO_BINNING, which takes no pixel records).
// trace's hit rule "t >= 0 and t < lim" (renderer.nim:58-62) for a limit lim
// in [+0, +inf] as ONE unsigned compare of the float bits: non-negative
// floats order like their bit patterns, a negative t or a NaN has bits above
// every such lim, and t + 0.0f turns -0.0 (which the rule accepts) into
// +0.0 and leaves every other value as it is. The float form is two compares
// and a scalar AND of their lane masks per ray and object (the batches'
// busiest pipe is the CU's one scalar unit). A sample that takes no part
// holds lim = +0.0, below which nothing lies.
__device__ __forceinline__ bool hit_below(float t, float lim) {
  return __float_as_uint(t + 0.0f) < __float_as_uint(lim);
}

#ifndef RTMI_LEAN_BATCH
#define RTMI_LEAN_BATCH 4
#endif
constexpr int kLeanBatch = RTMI_LEAN_BATCH;
// OB (object-binned batches, scenes without a mesh: k_render_fast): the
// camera rays visit only the objects of `cmask` (the wave's pixels' object
// masks, rt_bins.h build_object_pixel_masks) and each light's shadow rays
// only those of the light-grid cells their origins fall in — in scene order,
// exactly as trace's object bins (an object no bin lists cannot be hit, so it
// adds nothing to a closest hit or a hit count).
// An object-binned batch takes the light-grid cell masks of all its samples'
// shadow origins at once (below), not each sample's cells in turn. The
// object mask either way holds every object a shadow ray can hit, so frames
// and Stats do not change.
template <unsigned F, int S = kLeanBatch, bool OB = false>
__device__ __forceinline__ void lean_batch(KP p, const GroupPix& gp, int it0, const LdsF* tb, Acc& acc,
                                           Stats32& ws, unsigned long long cmask = ~0ull) {
  // Branch-free: per-sample predicates are lane masks in SGPRs and every
  // update is a select (v_cndmask), so the samples' code is straight-line
  // VALU (no exec-mask save / restore per sample). A masked-off term adds an
  // exact zero (fma(ci, 0, E) == E, acc + 0 == acc for the non-negative
  // sums), so values equal shade_path's branchy ones bit for bit.
  const F3 o = f3(p->cam[0], p->cam[1], p->cam[2]);
  F3 d[S];
  bool sv[S];
  batch_dirs<F, S>(p, gp, it0, tb, d, sv);
  unsigned nprim = 0u;
  // trace (renderer.nim:47-67) of the camera rays over the analytic objects
  // in scene order (the mesh is left out: none of the pixel's rays can hit
  // it). A hit is t >= 0 below the running minimum th; invalid samples start
  // at th = -1, which no t >= 0 is below (so th alone says: -1 invalid,
  // +inf sky, else a hit). Per-lane hit counts (VALU) instead of a mask
  // popcount per sample and object (SALU).
  float th[S];
  int hob[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    nprim += pc(bal(sv[k]));
    th[k] = sv[k] ? finf() : 0.0f;  // (hit_below: +0 takes no hit)
    hob[k] = -1;
  }
  ws.v[STAT_PRIMARY] += nprim;
  const int nobj = p->nobj, mesh = p->shadow_mesh;
  // the record arrays' bases pinned in SGPRs for the batch (opaque): the
  // compiler otherwise re-reads them from the kernel arguments before every
  // object / light visit, a dependent scalar load in front of the record's
  const FObj* objs = p->objs;
  const FLight* lights = p->lights;
  asm volatile("" : "+s"(objs), "+s"(lights));
  unsigned hitl = 0u;
  // the analytic objects in scene order
  // (one loop with a skip test: two index ranges around the mesh measured
  // 2 % slower, the loop body compiled twice)
  auto analytic_objects = [&](auto&& body) {
    for (int i = 0; i < nobj; ++i)
      if (i != mesh) body(i);
  };
  // OB: the objects of a mask in scene order (object bins exist for <= 64 objects)
  auto masked_objects = [&](unsigned long long m, auto&& body) {
    if constexpr (OB) {
      m &= nobj >= 64 ? ~0ull : ((1ull << nobj) - 1ull);
      while (m != 0ull) {
        const int i = (int)__builtin_ctzll(m);
        m &= m - 1ull;
        if (i != mesh) body(i);
      }
    } else {
      (void)m;
      analytic_objects(body);
    }
  };
  F3 oc[S];
#pragma unroll
  for (int k = 0; k < S; ++k) oc[k] = o;
  masked_objects(cmask, [&](const int i) {
    const FObj ob = at(objs, i);
    analytic_t_batch<F, S>(p, ob, i, oc, d, [&](int k, float t) {
      // trace's rule (t >= 0 ? t : inf) < th, as two compares (th <= inf)
      const bool c = hit_below(t, th[k]);
      th[k] = c ? t : th[k];
      hob[k] = c ? i : hob[k];
      hitl += c ? 1u : 0u;
    });
  });
  // shade (renderer.nim:71-127): normals per distinct object hit, the shadow
  // origins hitW + N * bias. A hit has t < inf (it beat the initial limit).
  unsigned long long litm[S], pend[S];
  F3 N[S], so[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    litm[k] = bal(hob[k] >= 0);  // (a hit beat th's start: +inf, or +0 for a sample that takes no part)
    pend[k] = litm[k];
    N[k] = f3(0.0f, 0.0f, 0.0f);
    so[k] = f3(__builtin_fmaf(d[k].x, th[k], o.x), __builtin_fmaf(d[k].y, th[k], o.y),
               __builtin_fmaf(d[k].z, th[k], o.z));  // the hit point until N is known
  }
  // every analytic object a plane (the mesh + plane subsets): a plane's
  // normal does not depend on the hit point, so with ONE object hit by the
  // batch's lit samples (the usual ground pixel) N and each light's N.L
  // are wave-uniform — formed once, the same values as per sample
  constexpr bool kPlanesOnly = !(F & (F_SPHERE | F_BOX));
  int nhobj = 0;
  F3 Nu = f3(0.0f, 0.0f, 0.0f), alb_u = f3(0.0f, 0.0f, 0.0f);
  for (;;) {
    const int oi = first_pending<S>(pend, hob);
    if (oi < 0) break;
    ++nhobj;
    int oi_cmp = oi;
    asm volatile("" : "+s"(oi_cmp));
    const FObj ob = at(objs, oi);
    const RT_CONST FObjX& ox = at(p->objx, oi);
    if constexpr (kPlanesOnly) {
      F3 n = f3(0.0f, 1.0f, 0.0f);  // Plane normal (geom.nim:365-366)
      if ((F & F_XF_GENERAL) && ob.xf == XF_GENERAL) {  // object_to_world * n, not re-normalised
        const float* m = ox.o2w;
        n = f3(__builtin_fmaf(m[0], n.x, __builtin_fmaf(m[3], n.y, m[6] * n.z)),
               __builtin_fmaf(m[1], n.x, __builtin_fmaf(m[4], n.y, m[7] * n.z)),
               __builtin_fmaf(m[2], n.x, __builtin_fmaf(m[5], n.y, m[8] * n.z)));
      }
      Nu = n;
      alb_u = f3(ox.albedo_pi[0], ox.albedo_pi[1], ox.albedo_pi[2]);
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const unsigned long long mine = bal(hob[k] == oi_cmp) & pend[k];
        pend[k] &= ~mine;
        const bool mi = lane_in(mine);
        N[k] = f3(mi ? n.x : N[k].x, mi ? n.y : N[k].y, mi ? n.z : N[k].z);
      }
      continue;
    }
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const unsigned long long mine = bal(hob[k] == oi_cmp) & pend[k];
      pend[k] &= ~mine;
      F3 ho, unused;
      to_object<F>(p, ob, oi, so[k], f3(0.0f, 0.0f, 0.0f), ho, unused);
      F3 n = analytic_normal<F>(ob, ho);
      if ((F & F_XF_GENERAL) && ob.xf == XF_GENERAL) {  // object_to_world * n, not re-normalised
        const float* m = ox.o2w;
        n = f3(__builtin_fmaf(m[0], n.x, __builtin_fmaf(m[3], n.y, m[6] * n.z)),
               __builtin_fmaf(m[1], n.x, __builtin_fmaf(m[4], n.y, m[7] * n.z)),
               __builtin_fmaf(m[2], n.x, __builtin_fmaf(m[5], n.y, m[8] * n.z)));
      }
      const bool mi = lane_in(mine);
      N[k] = f3(mi ? n.x : N[k].x, mi ? n.y : N[k].y, mi ? n.z : N[k].z);
    }
  }
  const bool uni = kPlanesOnly && nhobj == 1;
  const float bias = p->bias;
#pragma unroll
  for (int k = 0; k < S; ++k)
    so[k] = f3(__builtin_fmaf(N[k].x, bias, so[k].x), __builtin_fmaf(N[k].y, bias, so[k].y),
               __builtin_fmaf(N[k].z, bias, so[k].z));
  // one shadow ray per light and lit sample (distant lights only: a point
  // light has no skip bit, so its pixels are never lean)
  F3 E[S];
  unsigned long long anylit = 0ull;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    E[k] = f3(0.0f, 0.0f, 0.0f);
    anylit |= litm[k];
  }
  const int nl = anylit ? p->nlight : 0;
  unsigned nlit = 0u;
#pragma unroll
  for (int k = 0; k < S; ++k) nlit += pc(litm[k]);
  ws.v[STAT_SHADOW] += (unsigned)nl * nlit;
  auto light_loop = [&](auto uniform) {
    constexpr bool U = decltype(uniform)::value;
    for (int li = 0; li < nl; ++li) {
      const FLight L = at(lights, li);
      const F3 sd = f3(-L.v[0], -L.v[1], -L.v[2]);
      float ts[S];  // unlit samples start at 0 (take no part)
#pragma unroll
      for (int k = 0; k < S; ++k) ts[k] = lane_in(litm[k]) ? finf() : 0.0f;
      unsigned long long smask = ~0ull;  // every object
      if constexpr (OB) {
        // the light-grid cells of the lit samples' shadow origins (trace's
        // rule: off the grid -> the unbounded objects; beyond the grid's
        // float32-safe radius, or more than 4 distinct cells -> every object)
        if (p->obj_grids && cp(p->obj_grids)[li].gu > 0) {
          const RT_CONST LightGrid& G = cp(p->obj_grids)[li];
          unsigned long long m = p->obj_off_grid;
          bool every = false;
          // every lane loads its samples' cell masks (vector loads, one round
          // trip), ORed over the wave by DPP — instead of one scalar load per
          // distinct cell, each waited for in turn. No cap on the distinct
          // cells: their union is a subset of "every object" and, the masks
          // being conservative, tests every object a ray can hit.
          unsigned long long mine = 0ull;
#pragma unroll
          for (int k = 0; k < S; ++k) {
            const bool lk = lane_in(litm[k]);
            const F3 q = so[k];
            const float gu = __builtin_fmaf(q.x, G.e1[0], __builtin_fmaf(q.y, G.e1[1], q.z * G.e1[2]));
            const float gv = __builtin_fmaf(q.x, G.e2[0], __builtin_fmaf(q.y, G.e2[1], q.z * G.e2[2]));
            const float fu = (gu - G.u0) * G.inv_h, fv = (gv - G.v0) * G.inv_h;
            const bool safe = fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fabsf(q.z)) <= G.rmax;
            const bool on = fu >= 0.0f && fu < (float)G.gu && fv >= 0.0f && fv < (float)G.gv;
            if (lk && safe && on) mine |= p->obj_grid_mask[G.off_base + (int)fv * G.gu + (int)fu];
            every = every || bal(lk && !safe) != 0ull;
          }
          m |= ((unsigned long long)wave_or((unsigned)(mine >> 32)) << 32) | wave_or((unsigned)mine);
          smask = every ? smask : m;
        }
      }
      masked_objects(smask, [&](const int i) {
        const FObj ob = at(objs, i);
        if constexpr (kPlanesOnly) {
          // Plane.intersect (geom.nim:240-248) of the parallel shadow rays:
          // the direction's test and reciprocal once (a NaN multiplier for a
          // direction parallel to the plane: no t >= 0, as -inf gives none)
          F3 r0, rdu;
          to_object<F>(p, ob, i, so[0], sd, r0, rdu);
          const float mulp = fabsf(rdu.y) > 1e-6f ? rcp(rdu.y) : __builtin_nanf("");
#pragma unroll
          for (int k = 0; k < S; ++k) {
            F3 ro, rd;
            to_object<F>(p, ob, i, so[k], sd, ro, rd);
            const float t = -ro.y * mulp;
            const bool c = hit_below(t, ts[k]);
            ts[k] = c ? t : ts[k];
            hitl += c ? 1u : 0u;
          }
        } else {
          F3 sdk[S];
#pragma unroll
          for (int k = 0; k < S; ++k) sdk[k] = sd;
          analytic_t_batch<F, S>(p, ob, i, so, sdk, [&](int k, float t) {
            const bool c = hit_below(t, ts[k]);
            ts[k] = c ? t : ts[k];
            hitl += c ? 1u : 0u;
          });
        }
      });
      // unoccluded: shadeDiffuse (shader.nim:12-17)
      const float ndl_u = U ? fmaxf(dot3(Nu, sd), 0.0f) : 0.0f;
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const bool vis = lane_in(litm[k]) && !(ts[k] < finf());
        irr_add(E[k], L.ci, vis ? (U ? ndl_u : fmaxf(dot3(N[k], sd), 0.0f)) : 0.0f);
      }
    }
  };
  if (uni)
    light_loop(Bool<true>{});
  else
    light_loop(Bool<false>{});
  ws.v[STAT_HITS] += wave_sum(hitl);
  // albedo / pi per distinct object hit (one object: from the normal pass),
  // then the samples' colours in order
  if (uni) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const F3 a = mul3(alb_u, E[k]);
      const bool mi = lane_in(litm[k]);
      E[k] = f3(mi ? a.x : E[k].x, mi ? a.y : E[k].y, mi ? a.z : E[k].z);
    }
  } else {
#pragma unroll
    for (int k = 0; k < S; ++k) pend[k] = litm[k];
    for (;;) {
      const int oi = first_pending<S>(pend, hob);
      if (oi < 0) break;
      int oi_cmp = oi;
      asm volatile("" : "+s"(oi_cmp));
      const RT_CONST FObjX& ox = at(p->objx, oi);
      const F3 alb = f3(ox.albedo_pi[0], ox.albedo_pi[1], ox.albedo_pi[2]);
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const unsigned long long mine = bal(hob[k] == oi_cmp) & pend[k];
        pend[k] &= ~mine;
        const F3 a = mul3(alb, E[k]);
        const bool mi = lane_in(mine);
        E[k] = f3(mi ? a.x : E[k].x, mi ? a.y : E[k].y, mi ? a.z : E[k].z);
      }
    }
  }
  const F3 bg = f3(p->bg[0], p->bg[1], p->bg[2]);
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const bool lt = lane_in(litm[k]), sky = th[k] == finf();
    const F3 c = f3(lt ? E[k].x : (sky ? bg.x : 0.0f), lt ? E[k].y : (sky ? bg.y : 0.0f),
                    lt ? E[k].z : (sky ? bg.z : 0.0f));
    acc_add3(acc, c.x, c.y, c.z);
  }
}

}  // namespace fast
}  // namespace rtmi
