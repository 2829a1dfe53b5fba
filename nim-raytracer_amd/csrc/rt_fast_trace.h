// rt_fast_trace.h — the float32 one-sample path (rt_fast.h has the map): BVH
// traversal and list searches of one ray per lane, trace over the scene's
// objects, and the shading loop (shade_level / shade_path). The batched
// paths of rt_fast_batch.h are compared with it bit for bit.
#pragma once
#include "rt_fast_core.h"

namespace rtmi {
namespace fast {

// Leaf: the n (1..kLeafMax, wave-uniform) triangles starting at byte offset
// `first` of the tree.
__device__ __forceinline__ void leaf(KP p, int first, int n, F3 o, F3 d, unsigned long long& key,
                                     float& tc, const char* lb = nullptr) {
  if (lb) {  // a shadow ray to a light with LTri records
    const RT_CONST LTri* l = (const RT_CONST LTri*)(lb + (unsigned)first);
    ltri_test(load_ltri(l), o, key, tc);
#pragma unroll
    for (int k = 1; k < kLeafMax; ++k) {
      if (k >= n) break;
      ltri_test(load_ltri(l + k), o, key, tc);
    }
    return;
  }
  const RT_CONST TriFast* t = rec<TriFast>(p, first);
  tri_test(load_tri(t), o, d, key, tc);
#pragma unroll
  for (int k = 1; k < kLeafMax; ++k) {
    if (k >= n) break;
    tri_test(load_tri(t + k), o, d, key, tc);
  }
}

// Wave-coherent closest hit over one mesh BVH2 (64-B nodes, both child boxes
// per scalar fetch). Per lane: `tc` is the box-culling limit (the current
// best t; -1 for lanes that take no part, so `active` never enters a lane
// mask) and `key` the best (t, face) so far. Lanes step through the same node
// sequence: a child is visited when any lane's ray hits its box; both hit ->
// the nearer (majority vote) first, the other onto a 64-entry stack held one
// entry per lane in a single VGPR. Every child reference is valid (the
// builder never emits an empty child), and no iteration guard is needed: a
// traversal visits each node at most once.
// early/stop: exact early exit for shadow rays (trace()): a lane
// retires once its best t <= stop.
// Box-test form of a ray: ni = 1/d with components below 1e-20 in magnitude
// replaced by +-1e-20 (finite slabs, no 0 * inf), oi = o * ni; a slab plane
// x = c is crossed at fma(c, ni.x, -oi.x).
struct SlabRay {
  F3 ni, oi;
};
__device__ __forceinline__ SlabRay slab_ray(F3 o, F3 d) {
  const float e = 1e-20f;
  const float dx = fabsf(d.x) < e ? __builtin_copysignf(e, d.x) : d.x;
  const float dy = fabsf(d.y) < e ? __builtin_copysignf(e, d.y) : d.y;
  const float dz = fabsf(d.z) < e ? __builtin_copysignf(e, d.z) : d.z;
  SlabRay r;
  r.ni = f3(rcp(dx), rcp(dy), rcp(dz));
  r.oi = f3(o.x * r.ni.x, o.y * r.ni.y, o.z * r.ni.z);
  return r;
}

// The search state (key, tc) is the caller's (trace()): lanes with tc < 0
// take no part (never entered, retired, or done by a bin search).
template <bool COUNT>
__device__ __forceinline__ void traverse(KP p, int root, F3 o, F3 d, SlabRay sr, bool early, float stop,
                                         unsigned long long& key, float& tc, Stats32& ws,
                                         const char* lb = nullptr) {
  if (bal(tc >= 0.0f) == 0ull) return;
  RT_STAMP(t_enter);
  const F3 ni = sr.ni, oi = sr.oi;
  const int lane = (int)__lane_id();
  int stack = 0;
  int sp = 0;
  int node = root;
  // COUNT only: the lanes whose own ray hit the current node's box at its
  // parent (per-ray visits); far children's masks are
  // stacked alongside (two more VGPR stacks, diagnostic kernel only)
  unsigned long long vm = 0ull;
  int mlo = 0, mhi = 0;
  if constexpr (COUNT) vm = bal(tc >= 0.0f);
  for (;;) {
    const BvhNode nd = *rec<BvhNode>(p, node);
    if constexpr (COUNT) {
      ws.v[STAT_NODE_FETCH] += 1u;
      ws.v[STAT_LANE_NODES] += pc(vm);
    }
    const float ax0 = __builtin_fmaf(nd.lo0[0], ni.x, -oi.x), bx0 = __builtin_fmaf(nd.hi0[0], ni.x, -oi.x);
    const float ay0 = __builtin_fmaf(nd.lo0[1], ni.y, -oi.y), by0 = __builtin_fmaf(nd.hi0[1], ni.y, -oi.y);
    const float az0 = __builtin_fmaf(nd.lo0[2], ni.z, -oi.z), bz0 = __builtin_fmaf(nd.hi0[2], ni.z, -oi.z);
    const float ax1 = __builtin_fmaf(nd.lo1[0], ni.x, -oi.x), bx1 = __builtin_fmaf(nd.hi1[0], ni.x, -oi.x);
    const float ay1 = __builtin_fmaf(nd.lo1[1], ni.y, -oi.y), by1 = __builtin_fmaf(nd.hi1[1], ni.y, -oi.y);
    const float az1 = __builtin_fmaf(nd.lo1[2], ni.z, -oi.z), bz1 = __builtin_fmaf(nd.hi1[2], ni.z, -oi.z);
    const float tn0 = fmaxf(fmaxf(fminf(ax0, bx0), fminf(ay0, by0)), fmaxf(fminf(az0, bz0), 0.0f));
    const float tf0 = fminf(fminf(fmaxf(ax0, bx0), fmaxf(ay0, by0)), fminf(fmaxf(az0, bz0), tc));
    const float tn1 = fmaxf(fmaxf(fminf(ax1, bx1), fminf(ay1, by1)), fmaxf(fminf(az1, bz1), 0.0f));
    const float tf1 = fminf(fminf(fmaxf(ax1, bx1), fmaxf(ay1, by1)), fminf(fmaxf(az1, bz1), tc));
    unsigned long long m0 = bal(tn0 <= tf0 * 1.0000004f);
    unsigned long long m1 = bal(tn1 <= tf1 * 1.0000004f);
    if (nd.n0 > 0) {
      if (m0) {
        if constexpr (COUNT) {
          ws.v[STAT_TRI_FETCH] += (unsigned int)nd.n0;
          ws.v[STAT_LANE_TRIS] += pc(m0) * (unsigned int)nd.n0;
        }
        leaf(p, nd.c0, nd.n0, o, d, key, tc, lb);
        if (early) tc = tc <= stop ? -1.0f : tc;
      }
      m0 = 0ull;
    }
    if (nd.n1 > 0) {
      if (m1) {
        if constexpr (COUNT) {
          ws.v[STAT_TRI_FETCH] += (unsigned int)nd.n1;
          ws.v[STAT_LANE_TRIS] += pc(m1) * (unsigned int)nd.n1;
        }
        leaf(p, nd.c1, nd.n1, o, d, key, tc, lb);
        if (early) tc = tc <= stop ? -1.0f : tc;
      }
      m1 = 0ull;
    }
    if (m0 && m1) {
      const unsigned long long both = m0 & m1;
      const bool first0 = pc(bal(tn0 <= tn1) & both) * 2u >= pc(both);
      const int near = first0 ? nd.c0 : nd.c1;
      const int far = first0 ? nd.c1 : nd.c0;
      stack = (lane == sp) ? far : stack;
      if constexpr (COUNT) {
        const unsigned long long fm = first0 ? m1 : m0;
        mlo = (lane == sp) ? (int)(unsigned int)fm : mlo;
        mhi = (lane == sp) ? (int)(unsigned int)(fm >> 32) : mhi;
        vm = first0 ? m0 : m1;
      }
      ++sp;
      node = near;
    } else if (m0) {
      node = nd.c0;
      if constexpr (COUNT) vm = m0;
    } else if (m1) {
      node = nd.c1;
      if constexpr (COUNT) vm = m1;
    } else {
      if (sp == 0) break;
      if (early && bal(tc >= 0.0f) == 0ull) break;
      --sp;
      node = __builtin_amdgcn_readlane(stack, sp);
      if constexpr (COUNT)
        vm = (unsigned long long)(unsigned int)__builtin_amdgcn_readlane(mlo, sp) |
             ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(mhi, sp) << 32);
    }
  }
#ifdef RTMI_STAMPS
  { RT_STAMP(t_exit); RT_ACC(5, t_enter, t_exit); }
#endif
}

// The faces listed at ent[b, e) (a pixel list or a light-grid cell, rt_bins.h)
// against every lane's ray, with the traversal's key / early-exit rules.
// ent is padded, so the four-record read-ahead stays inside the array.
template <bool COUNT>
__device__ __forceinline__ void list_search(KP p, const int32_t* ent, int b, int e, F3 o, F3 d, bool early,
                                            float stop, unsigned long long& key, float& tc, Stats32& ws,
                                            const char* lb = nullptr) {
  if constexpr (COUNT) {
    ws.v[STAT_TRI_FETCH] += (unsigned int)(e - b);
    ws.v[STAT_LANE_TRIS] += pc(bal(tc >= 0.0f)) * (unsigned int)(e - b);
  }
  auto test = [&](int off) {
    if (lb) ltri_test(load_ltri((const RT_CONST LTri*)(lb + (unsigned)off)), o, key, tc);
    else tri_test(load_tri(rec<TriFast>(p, off)), o, d, key, tc);
  };
  if (early && b < e) {  // a light cell's first face alone (the one covering most of the cell)
    test(cp(ent)[b]);
    tc = tc <= stop ? -1.0f : tc;
    if (bal(tc >= 0.0f) == 0ull) return;
    ++b;
  }
  for (int k = b; k < e; k += 4) {
    const RT_CONST int32_t* q = cp(ent) + k;
    const int r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3];
    test(r0);
    if (k + 1 < e) test(r1);
    if (k + 2 < e) test(r2);
    if (k + 3 < e) test(r3);
    if (early) {
      tc = tc <= stop ? -1.0f : tc;
      if (bal(tc >= 0.0f) == 0ull) break;
    }
  }
}

// t of analytic object i in world space, -inf on a miss (Sphere / Plane /
// Box .intersect, geom.nim:215-248, 76-96).
template <unsigned F>
__device__ __forceinline__ float analytic_t(KP p, const FObj& ob, int i, F3 o, F3 d) {
  F3 ro, rd;
  to_object<F>(p, ob, i, o, d, ro, rd);
  // without spheres and boxes in the scene every analytic object is a plane
  if (!(F & (F_SPHERE | F_BOX)) || ob.type == GEOM_PLANE) return plane(ro, rd);
  if ((F & F_SPHERE) && ob.type == GEOM_SPHERE) return sphere(ob.r, ro, rd);
  if (F & F_BOX) return aabb(ob.lo, ob.hi, ro, f3(rcp(rd.x), rcp(rd.y), rcp(rd.z)));
  return -finf();
}

// analytic_t for S rays against one object: the object's transform kind
// and type are dispatched once (uniform branches) with the S rays inside
// each case — called per ray, the dispatch and the object's record loads
// were repeated for every ray (C2's batches: ~20 scalar instructions per ray
// and object on the CU's busiest pipe). Same arithmetic per ray as
// analytic_t (bit-identical t); body(k, t) consumes ray k's t at once, and a
// scheduling barrier between rays keeps their temporaries from overlapping
// (interleaved, the S rays' transforms spilled).
template <unsigned F, int S, class Body>
__device__ __forceinline__ void analytic_t_batch(KP p, const FObj& ob, int i, const F3 (&o)[S], const F3 (&d)[S],
                                                 Body&& body) {
  auto cases = [&](auto general) {
    constexpr bool G = decltype(general)::value;
    auto xform = [&](int k, F3& ro, F3& rd) {
      if constexpr (G) {
        const RT_CONST FObjX& x = at(p->objx, i);
        const float* m = x.w2o;
        ro = f3(__builtin_fmaf(m[0], o[k].x, __builtin_fmaf(m[3], o[k].y, __builtin_fmaf(m[6], o[k].z, m[9]))),
                __builtin_fmaf(m[1], o[k].x, __builtin_fmaf(m[4], o[k].y, __builtin_fmaf(m[7], o[k].z, m[10]))),
                __builtin_fmaf(m[2], o[k].x, __builtin_fmaf(m[5], o[k].y, __builtin_fmaf(m[8], o[k].z, m[11]))));
        rd = f3(__builtin_fmaf(m[0], d[k].x, __builtin_fmaf(m[3], d[k].y, m[6] * d[k].z)),
                __builtin_fmaf(m[1], d[k].x, __builtin_fmaf(m[4], d[k].y, m[7] * d[k].z)),
                __builtin_fmaf(m[2], d[k].x, __builtin_fmaf(m[5], d[k].y, m[8] * d[k].z)));
      } else {
        ro = f3(o[k].x + ob.t[0], o[k].y + ob.t[1], o[k].z + ob.t[2]);
        rd = d[k];
      }
    };
    if (!(F & (F_SPHERE | F_BOX)) || ob.type == GEOM_PLANE) {
#pragma unroll
      for (int k = 0; k < S; ++k) {
        F3 ro, rd;
        xform(k, ro, rd);
        body(k, plane(ro, rd));
        __builtin_amdgcn_sched_barrier(0);
      }
    } else if ((F & F_SPHERE) && ob.type == GEOM_SPHERE) {
#pragma unroll
      for (int k = 0; k < S; ++k) {
        F3 ro, rd;
        xform(k, ro, rd);
        body(k, sphere(ob.r, ro, rd));
        __builtin_amdgcn_sched_barrier(0);
      }
    } else if (F & F_BOX) {
#pragma unroll
      for (int k = 0; k < S; ++k) {
        F3 ro, rd;
        xform(k, ro, rd);
        body(k, aabb(ob.lo, ob.hi, ro, f3(rcp(rd.x), rcp(rd.y), rcp(rd.z))));
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int k = 0; k < S; ++k) body(k, -finf());
    }
  };
  if ((F & F_XF_GENERAL) && ob.xf == XF_GENERAL)
    cases(Bool<true>{});
  else
    cases(Bool<false>{});
}

// The cell of face grid G (rt_bins.h) that a shadow ray's origin r, in the
// mesh's frame, falls in: its index into the grids' cell offsets, -1 for
// none. safe: r is within the grid's float32-safe radius (beyond it the cell
// proves nothing: the BVH serves the ray); on: r projects onto the grid (safe
// and off the grid: no face can be hit). mesh_search and light_cell_search
// (rt_fast_batch.h) map origins to cells here. (lean_batch's object-grid
// index keeps its own copy: through this function the object-binned
// kernels came out 24 instructions longer, profiles/r10.)
__device__ __forceinline__ int light_cell(const RT_CONST LightGrid& G, F3 r, bool& safe, bool& on) {
  const float gu = __builtin_fmaf(r.x, G.e1[0], __builtin_fmaf(r.y, G.e1[1], r.z * G.e1[2]));
  const float gv = __builtin_fmaf(r.x, G.e2[0], __builtin_fmaf(r.y, G.e2[1], r.z * G.e2[2]));
  const float fu = (gu - G.u0) * G.inv_h, fv = (gv - G.v0) * G.inv_h;
  safe = fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fabsf(r.z)) <= G.rmax;
  on = fu >= 0.0f && fu < (float)G.gu && fv >= 0.0f && fv < (float)G.gv;
  return safe && on ? G.off_base + (int)fv * G.gu + (int)fu : -1;
}

// trace (renderer.nim:47-67): linear closest hit over the objects in order;
// an object counts as a hit only when it beats the running minimum.
//
// Shadow rays only need (a) whether any object is hit below tmax and (b) the
// reference's hit count, in which an object after the mesh is counted only if
// its t beats the mesh's closest t. So once a lane has found a mesh hit at
// t <= stop = min t of the analytic objects after the mesh, every later
// comparison is decided and the lane retires: exact, not an approximation.
// Applied when the scene has exactly one mesh object (p->shadow_mesh); stop =
// min t >= 0 of the analytic objects after the mesh.
// pix: the camera ray's pixel index (y * width + x; -1 for other rays),
// light: the shadow ray's light (-1 for other rays); they select the bins.
// The search of the mesh's faces for the lanes that passed the AABB gate
// (part): the shadow early exit's stop distance, the binned lists, then the
// BVH for the lanes no bin served. Returns the best (t, face) key (key0 = the
// entry key when nothing closer was found).
template <bool COUNT, unsigned F>
__device__ __forceinline__ unsigned long long mesh_search(KP p, const FObj& ob, int i, F3 o, F3 d, F3 ro, F3 rd,
                                                          SlabRay sr, bool part, float tb, bool shadow, bool early,
                                                          int bin, const int32_t* boff, const int32_t* bent,
                                                          bool nohit, int light, Stats32& ws) {
  const bool ex = early && i == p->shadow_mesh;
  const char* lb = shadow ? lrec_of(p, light) : nullptr;  // distant-light shadow rays: LTri records
  float stop = -1.0f;
  if (ex) {
    RT_STAMP(t_st0);
    stop = finf();
    for (int j = i + 1; j < p->nobj; ++j) {
      const float tj = analytic_t<F>(p, at(p->objs, j), j, o, d);
      stop = tj >= 0.0f ? fminf(stop, tj) : stop;
    }
#if RTMI_STAMPS == 2
    { RT_STAMP(t_st1); RT_ACC(7, t_st0, t_st1); }
#endif
  }
  // search state of the lanes that enter: the best (t, face) key and
  // the culling limit; a lane retires (early exit) on a FOUND hit
  // with t <= stop, so stop is clamped to the float just below the
  // initial limit (tb > 0; for tb == 0 the bit pattern wraps to NaN,
  // fminf keeps stop, and nothing is acceptable)
  float tc = part ? tb : -1.0f;
  stop = fminf(stop, __uint_as_float(__float_as_uint(tb) - 1u));
  const unsigned long long key0 = part ? tkey(tb, 0u) : 0ull;
  unsigned long long key = key0;
  // shadow rays: the light-grid cell (after the gate: the cell
  // costs more than the gate, which already sends most waves away)
  if ((F & F_MESH) && shadow && p->grids && light >= 0 && p->grids[light].gu > 0) {
    const RT_CONST LightGrid& G = cp(p->grids)[light];
    bool safe, on;
    bin = light_cell(G, ro, safe, on);
    nohit = safe && !on;
    boff = p->grid_off;
    bent = p->grid_ent + G.ent_base;
  }
  if (bent) {  // up to 4 distinct bins per wave; lanes left over take the BVH
    unsigned long long todo = bal(part && bin >= 0), ovf = 0ull;
    for (int it = 0; it < 4 && todo != 0ull; ++it) {
      const int kb = __builtin_amdgcn_readlane(bin, (int)__builtin_ctzll(todo));
      const unsigned long long mk = bal(bin == kb);
      todo &= ~mk;
      if (boff) {  // a light-grid cell
        list_search<COUNT>(p, bent, cp(boff)[kb], cp(boff)[kb + 1], ro, rd, ex, stop, key, tc, ws, lb);
      } else {     // a pixel list (rt_frame.h slots); past its slots the BVH serves the pixel
        const int n = (int)(at(p->pix_cnt, kb) & kPixCount), b = kb << p->slot_lg;
        if (n > (1 << p->slot_lg)) ovf |= mk;
        else list_search<COUNT>(p, bent, b, b + n, ro, rd, ex, stop, key, tc, ws, lb);
      }
    }
    // done: binned lanes (their bin was searched) and lanes off the grid
    tc = (lane_in(todo | ovf) || !(bin >= 0 || nohit)) ? tc : -1.0f;
  }
  traverse<COUNT>(p, ob.root, ro, rd, sr, ex, stop, key, tc, ws, lb);
  return key;
}


// src (per lane; reflected rays): the plane the ray was reflected off, -1
// for every other ray. Such a ray starts at hit + r * bias and runs along r,
// so it meets that plane at t = -bias exactly: a miss, whatever the plane's
// transform. Recomputed from the float32 hit point, whose distance to the
// plane is rounding error (up to an ulp of the camera's height, more under a
// general transform), t comes out positive where |r . n| * bias is smaller
// than that error (the ground towards the horizon); the lane takes the exact
// answer instead.
template <bool COUNT, unsigned F>
__device__ __forceinline__ Hit trace(KP p, F3 o, F3 d, float tmax, bool active, bool shadow, int pix, int light,
                                     Stats32& ws, bool no_mesh = false, int src = -1) {
  RT_STAMP(t_trace0);
  Hit h{-1, -1, tmax};
  const bool early = (F & F_MESH) && shadow && p->shadow_mesh >= 0;
  const unsigned long long actm = bal(active);
  // Object bins (scenes of 4..64 objects, rt_bins.h): the objects the wave's
  // bins list, in scene order; an object no bin lists cannot be hit (it
  // would add nothing to the closest hit or the hit count). Up to 4 distinct
  // bins per wave, otherwise every object.
  // Compiled for scenes with spheres or boxes only: mesh + plane scenes keep
  // the plain object loop (C3: the mask loop cost 27 % there).
  constexpr bool kObjBins = (F & (F_SPHERE | F_BOX)) != 0;
  const int nobj = p->nobj;
  unsigned long long omask = nobj >= 64 ? ~0ull : ((1ull << nobj) - 1ull);
  if (!kObjBins) {
  } else if (!shadow && p->obj_pix && pix >= 0) {  // camera rays: the wave's pixels
    unsigned long long todo = bal(active && pix >= 0), m = 0ull;
    for (int it = 0; it < 4 && todo != 0ull; ++it) {
      const int kp = __builtin_amdgcn_readlane(pix, (int)__builtin_ctzll(todo));
      todo &= ~bal(pix == kp);
      m |= cp(p->obj_pix)[kp];
    }
    omask = todo == 0ull ? m : omask;
  } else if (shadow && p->obj_grids && light >= 0 && p->obj_grids[light].gu > 0) {  // distant light: cells
    const RT_CONST LightGrid& G = cp(p->obj_grids)[light];
    const float gu = __builtin_fmaf(o.x, G.e1[0], __builtin_fmaf(o.y, G.e1[1], o.z * G.e1[2]));
    const float gv = __builtin_fmaf(o.x, G.e2[0], __builtin_fmaf(o.y, G.e2[1], o.z * G.e2[2]));
    const float fu = (gu - G.u0) * G.inv_h, fv = (gv - G.v0) * G.inv_h;
    const bool safe = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)) <= G.rmax;
    const bool on = fu >= 0.0f && fu < (float)G.gu && fv >= 0.0f && fv < (float)G.gv;
    const int cell = on ? (int)fv * G.gu + (int)fu : -1;
    unsigned long long m = p->obj_off_grid;
    unsigned long long todo = bal(active && safe && on);
    for (int it = 0; it < 4 && todo != 0ull; ++it) {
      const int kc = __builtin_amdgcn_readlane(cell, (int)__builtin_ctzll(todo));
      todo &= ~bal(cell == kc);
      m |= cp(p->obj_grid_mask)[G.off_base + kc];
    }
    omask = (todo == 0ull && bal(active && !safe) == 0ull) ? m : omask;
  }
  auto visit = [&](const int i) {
    // the mesh skipped outright (no record fetch, no hit-mask work)
    if ((F & F_MESH) && no_mesh && i == p->shadow_mesh) return;
    const FObj ob = at(p->objs, i);
    float t;
    int tri = -1;
    if (!(F & F_MESH) || ob.type != GEOM_MESH) {
      t = analytic_t<F>(p, ob, i, o, d);
    } else {
      RT_STAMP(t_g0);
      F3 ro, rd;
      to_object<F>(p, ob, i, o, d, ro, rd);
      // Coherent families search the faces binned for them (rt_bins.h)
      // instead of the BVH: camera rays by pixel (pix: this lane's pixel
      // index, -1 for other rays), shadow rays to a distant light by
      // light-grid cell. A lane whose bin is empty, or that is off the grid,
      // can hit no face. When the caller knows that no lane can hit the mesh
      // (no_mesh: a one-pixel wave whose pixel list is empty, or whose
      // pixel's shadow skip bit for this light is set) the mesh is skipped
      // before the AABB gate (the gate's verdict cannot matter).
      int bin = -1;                        // this lane's bin, -1: none
      const int32_t* boff = nullptr;       // light-grid cells: CSR offsets; pixel lists: slots (boff == nullptr)
      const int32_t* bent = nullptr;
      bool nohit = false;                  // off every listed face
      if ((F & F_MESH) && !shadow && p->pix_slots && pix >= 0) {
        bin = pix;
        bent = p->pix_slots;
      }
      // no_mesh (wave-uniform, the caller's pixel record): no lane can hit the mesh
      const bool skip = no_mesh;
      if (skip) {
        t = -finf();
      } else {
        // TriangleMesh.intersect (geom.nim:339-358): a ray starting inside
        // the mesh AABB misses (entry t < 0); otherwise the closest face.
        // The AABB and the root ride in the object record (no dependent
        // FMesh fetch); the gate uses the traversal's slab form of the ray
        // (built here, not hoisted to the trace's entry by the compiler:
        // camera waves over an empty pixel list never need it).
        F3 rdl = rd;
        asm volatile("" : "+v"(rdl.x), "+v"(rdl.y), "+v"(rdl.z));
        const SlabRay sr = slab_ray(ro, rdl);
        const float ax = __builtin_fmaf(ob.lo[0], sr.ni.x, -sr.oi.x), bx = __builtin_fmaf(ob.hi[0], sr.ni.x, -sr.oi.x);
        const float ay = __builtin_fmaf(ob.lo[1], sr.ni.y, -sr.oi.y), by = __builtin_fmaf(ob.hi[1], sr.ni.y, -sr.oi.y);
        const float az = __builtin_fmaf(ob.lo[2], sr.ni.z, -sr.oi.z), bz = __builtin_fmaf(ob.hi[2], sr.ni.z, -sr.oi.z);
        const float gmin = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
        const float gmax = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * 1.00000024f;
        const bool in = gmin <= gmax && gmin >= 0.0f;
        const bool part = active && in;
        float tb = h.t;
        int best = -1;
#if RTMI_STAMPS == 2
        { RT_STAMP(t_g1); RT_ACC(8, t_g0, t_g1); }
#endif
        // shadow early exit (above): stop is only computed when some lane of
        // the wave enters the mesh
        if (ob.root >= 0 && bal(part) != 0ull) {
          const unsigned long long key0 = part ? tkey(tb, 0u) : 0ull;
          const unsigned long long key = mesh_search<COUNT, F>(p, ob, i, o, d, ro, rd, sr, part, tb, shadow, early,
                                                               bin, boff, bent, nohit, light, ws);
          if (key != key0) {
            tb = __uint_as_float((unsigned int)(key >> 32));
            best = (int)(unsigned int)key;
          }
        }
        t = !in ? -finf() : (best >= 0 ? tb : finf());
        tri = best;
      }
    }
    if ((F & F_REFLECT) && i == src) t = -finf();
    const unsigned long long um = m_ge(t, 0.0f) & m_lt(t, h.t) & actm;
    ws.v[STAT_HITS] += pc(um);
    const bool upd = lane_in(um);
    if (upd) {
      h.t = t;
      h.obj = i;
      h.tri = tri;
    }
  };
  if constexpr (kObjBins) {
    for (int base = 0; base < nobj; base += 64) {
      unsigned long long om = base == 0 ? omask : (nobj - base >= 64 ? ~0ull : ((1ull << (nobj - base)) - 1ull));
      while (om != 0ull) {
        const int i = base + (int)__builtin_ctzll(om);
        om &= om - 1ull;
        visit(i);
      }
    }
  } else {
    for (int i = 0; i < nobj; ++i) visit(i);
  }
#ifdef RTMI_STAMPS
  { RT_STAMP(t_trace1); RT_ACC(6, t_trace0, t_trace1); }
#endif
  return h;
}

// normal(*) (geom.nim:361-379) for analytic geometry, object space.
template <unsigned F>
__device__ __forceinline__ F3 analytic_normal(const FObj& ob, F3 ho) {
  if ((F & F_SPHERE) && ob.type == GEOM_SPHERE) {
    const float r = rsq(dot3(ho, ho));
    return f3(ho.x * r, ho.y * r, ho.z * r);
  }
  if ((F & F_BOX) && ob.type == GEOM_BOX) {
    const float cx = (ob.lo[0] + ob.hi[0]) * 0.5f, cy = (ob.lo[1] + ob.hi[1]) * 0.5f,
                cz = (ob.lo[2] + ob.hi[2]) * 0.5f;
    const float qx = (ho.x - cx) * rcp(fabsf((ob.lo[0] - ob.hi[0]) * 0.5f));
    const float qy = (ho.y - cy) * rcp(fabsf((ob.lo[1] - ob.hi[1]) * 0.5f));
    const float qz = (ho.z - cz) * rcp(fabsf((ob.lo[2] - ob.hi[2]) * 0.5f));
    // The reference's 1.000001: an axis counts within 1e-6 of its face, so
    // only there (an edge, a corner) is the normal diagonal. A float32 hit
    // point is good to ~1e-6 of the box size and may truncate every axis to
    // 0: then the dominant axis, rather than a NaN normal. (A wider factor
    // instead, 1.0001, made the normal diagonal, and the face unlit, within
    // 1e-4 of every edge: a band a hundred times the reference's.)
    F3 n = f3(truncf(qx * 1.000001f), truncf(qy * 1.000001f), truncf(qz * 1.000001f));
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) {
      const float ax = fabsf(qx), ay = fabsf(qy), az = fabsf(qz);
      if (ax >= ay && ax >= az) n.x = qx < 0.0f ? -1.0f : 1.0f;
      else if (ay >= az) n.y = qy < 0.0f ? -1.0f : 1.0f;
      else n.z = qz < 0.0f ? -1.0f : 1.0f;
    }
    const float r = rsq(dot3(n, n));
    return f3(n.x * r, n.y * r, n.z * r);
  }
  return f3(0.0f, 1.0f, 0.0f);  // plane
}

// One shading level of renderer.nim's shade (renderer.nim:71-127 at one
// recursion depth) for the wave's `act` lanes, at forward weight w:
//  * renderer.nim:94-101: one shadow ray per light from hitW + N*bias; the
//    light's shadeDiffuse term (shader.nim:12-17) is added when it misses.
//  * renderer.nim:104-124: reflection > 0 and depth <= maxRayDepth traces
//    r = i - 2 (n.i) n from hitW + r*bias; the level's local light is
//    weighted (1 - reflection), the reflected colour reflection.
// v: the level's radiance of this lane (background x w on a miss, the
// weighted local light on a hit); reflect / refl: whether the lane reflects
// (its reflected ray parked in LDS at LDS_RO / LDS_RD) and the hit's
// Material.reflection (0 without a hit).
// pix: the sample's pixel index (y * width + x) for the camera ray's bins;
// pinfo: the wave's pixel record (FastParams.pix_info) when the wave holds
// one pixel, else kPixCount (nothing known).
// src: trace's src of this level's ray; the parked ray's is left at LDS_SRC.
template <bool COUNT, unsigned F, bool LEAN = false>
__device__ __forceinline__ void shade_level(KP& p, F3 o, F3 d, bool act, int lev, int depth, float w, int pix,
                                            unsigned pinfo, LdsF* ls, F3& v, bool& reflect, float& refl_out,
                                            Stats32& ws, int src = -1) {
  v = f3(0.0f, 0.0f, 0.0f);
  const Hit hit = trace<COUNT, F>(p, o, d, finf(), act, false, lev == 0 ? pix : -1, -1, ws,
                                  lev == 0 && (LEAN || (pinfo & kPixCount) == 0u), src);
  if (act && hit.obj < 0) v = f3(mul_nc(w, p->bg[0]), mul_nc(w, p->bg[1]), mul_nc(w, p->bg[2]));
  const bool lit = act && hit.obj >= 0;
  const F3 hw = f3(__builtin_fmaf(d.x, hit.t, o.x), __builtin_fmaf(d.y, hit.t, o.y), __builtin_fmaf(d.z, hit.t, o.z));
  F3 N = f3(0.0f, 0.0f, 0.0f);
  F3 alb = f3(0.0f, 0.0f, 0.0f);
  float refl = 0.0f;
  int plane_hit = -1;
  unsigned long long pending = bal(lit);
  while (pending) {  // one pass per distinct object hit by the wave
    const int lead = (int)__builtin_ctzll(pending);
    const int oi = __builtin_amdgcn_readlane(hit.obj, lead);
    // `mine` compares against an opaque copy: knowing hit.obj == oi inside
    // the branch, the compiler would otherwise address the object's
    // uniform records through the per-lane hit.obj (vector loads on the
    // sample's critical path instead of scalar loads)
    int oi_cmp = oi;
    asm volatile("" : "+s"(oi_cmp));
    const bool mine = lit && hit.obj == oi_cmp;
    pending &= ~bal(mine);
    const FObj ob = at(p->objs, oi);
    const RT_CONST FObjX& ox = at(p->objx, oi);
    const F3 oalb = f3(ox.albedo_pi[0], ox.albedo_pi[1], ox.albedo_pi[2]);
    const float orefl = ox.refl;
    const int nbase = ox.normal_base;
    if (mine) {
      F3 n;
      if ((F & F_MESH) && ob.type == GEOM_MESH) {
        const float* fn = p->normals + 3 * (size_t)(nbase + hit.tri);
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
      alb = oalb;
      refl = orefl;
      if ((F & F_REFLECT) && ob.type == GEOM_PLANE) plane_hit = oi;
    }
  }
  reflect = (F & F_REFLECT) && lit && refl > 0.0f && depth <= p->max_depth;
  refl_out = refl;
  const float wl = reflect ? w * (1.0f - refl) : w;
  // albedo/pi * weight waits in LDS across the light loop (the loop's
  // register peak sits inside the shadow traversal); the lights' terms
  // are summed into E first (irr_add)
  lds_put3(ls, LDS_ALB, f3(alb.x * wl, alb.y * wl, alb.z * wl));
  F3 E = f3(0.0f, 0.0f, 0.0f);
  if (F & F_REFLECT) ws.v[STAT_REFL] += pc(bal(reflect));
  if ((F & F_REFLECT) && bal(reflect)) {  // park the reflected ray (renderer.nim:109-118)
    if (reflect) {
      const float ndi = 2.0f * dot3(N, d);
      const F3 rd = f3(d.x - N.x * ndi, d.y - N.y * ndi, d.z - N.z * ndi);
      lds_put3(ls, LDS_RO, f3(__builtin_fmaf(rd.x, p->bias, hw.x), __builtin_fmaf(rd.y, p->bias, hw.y),
                              __builtin_fmaf(rd.z, p->bias, hw.z)));
      lds_put3(ls, LDS_RD, rd);
      lds_put1(ls, LDS_SRC, __int_as_float(plane_hit));
    }
  }
  const F3 so = f3(__builtin_fmaf(N.x, p->bias, hw.x), __builtin_fmaf(N.y, p->bias, hw.y),
                   __builtin_fmaf(N.z, p->bias, hw.z));
  if ((F & F_POINT) && p->has_point_light) lds_put3(ls, LDS_HW, hw);
  // no lane shaded a hit (the sky): no shadow rays at all
  const int nl = bal(lit) != 0ull ? p->nlight : 0;
  // shadow skips of the wave's pixel (camera hits only): bit li set = no
  // shadow ray to light li can meet the mesh
  const unsigned skipw = lev == 0 ? pinfo >> 24 : 0u;
  // two instances of the light loop: with every light's skip bit set the
  // shadow traces are compiled without the mesh search (C3: most waves),
  // which the register allocation and scheduling of the loop feel even
  // when the search is skipped at run time
  auto light_loop = [&](auto lean) {
    constexpr bool kLean = decltype(lean)::value;
    for (int li = 0; li < nl; ++li) {
      if (!kLean) p = params();
      const FLight L = at(p->lights, li);
      F3 sd;
      float dist, k = 1.0f;
      if ((F & F_POINT) && L.type == LIGHT_POINT) {  // light.nim:52-62
        const F3 h = lds_get3(ls, LDS_HW);
        const F3 lv = f3(h.x - L.v[0], h.y - L.v[1], h.z - L.v[2]);
        const float r2 = dot3(lv, lv);
        const float rr = rsq(r2);
        sd = f3(-lv.x * rr, -lv.y * rr, -lv.z * rr);
        k = rcp(12.566370614359172f * r2);
        dist = r2 * rr;
      } else {  // light.nim:46-50
        sd = f3(-L.v[0], -L.v[1], -L.v[2]);
        dist = finf();
      }
      ws.v[STAT_SHADOW] += pc(bal(lit));
      const Hit sh = trace<COUNT, F>(p, so, sd, dist, lit, true, -1, li, ws,
                                     kLean || (li < 8 && ((skipw >> li) & 1u) != 0u));
      if (lit && sh.obj < 0) irr_add(E, L.ci, fmaxf(dot3(N, sd), 0.0f) * k);  // shadeDiffuse (shader.nim:12-17)
    }
  };
  if (LEAN || ((F & F_MESH) && nl > 0 && nl <= 8 && skipw == (1u << nl) - 1u))
    light_loop(Bool<true>{});
  else
    light_loop(Bool<false>{});
  if (lit) v = mul3(lds_get3(ls, LDS_ALB), E);
}

// One camera sample: trace + shade (renderer.nim:71-127), reflections as a
// loop of levels with forward weights; each level's radiance is added into
// `acc` in level order.
template <bool COUNT, unsigned F, bool LEAN = false>
__device__ __forceinline__ void shade_path(KP p, F3 o, F3 d, bool active, int pix, unsigned pinfo, LdsF* ls,
                                           Acc& acc, Stats32& ws) {
  bool act = active;
  int depth = 1;
  int src = -1;
  float w = 1.0f;
  for (int lev = 0; lev < ((F & F_REFLECT) ? kMaxShadeLevels : 1); ++lev) {
    if (LEAN == 0) p = params();
    if (bal(act) == 0ull) break;
    F3 v;
    bool reflect;
    float refl;
    shade_level<COUNT, F, LEAN>(p, o, d, act, lev, depth, w, pix, pinfo, ls, v, reflect, refl, ws, src);
    if (act) acc_add3(acc, v.x, v.y, v.z);
    // every lane reloads (lanes that do not reflect go inactive): o and d
    // are then dead across the light loop instead of carried for them
    if ((F & F_REFLECT) && bal(reflect)) {
      o = lds_get3(ls, LDS_RO);
      d = lds_get3(ls, LDS_RD);
      src = reflect ? __float_as_int(lds_get1(ls, LDS_SRC)) : -1;
    }
    w = w * refl;
    ++depth;
    act = reflect;
  }
}

}  // namespace fast
}  // namespace rtmi
