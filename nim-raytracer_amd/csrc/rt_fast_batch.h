// rt_fast_batch.h — the float32 batched paths of mesh scenes (rt_fast.h has
// the map): S samples per lane through the pixel's face list and the lights'
// grid cells — camera rays, the batched list search, the one light-cell
// shadow search, and the three general-pixel batches built on them.
#pragma once
#include "rt_fast_trace.h"

namespace rtmi {
namespace fast {

// castPrimaryRay (renderer.nim:31-44) for sample s of the lane's pixel
// (calcPixel's sample table, renderer.nim:144-159): the direction (the
// origin is the camera's, p->cam[0..2]). Camera constants are folded on the
// host: ((2 x r)/w - r) f == (x - w/2) (2 r f / w), exact 0 on the centre
// column / row as the reference's own formula gives there. Every FMA is
// explicit, so all instances of the sample loop round alike. The cx terms
// are innermost: a lane whose samples share a column (akGrid, m | 64) forms
// them once per pixel (lean1q_loop) with the same roundings.
__device__ __forceinline__ F3 camera_ray_dir(KP p, float px, float py) {
  const float cx = (px - p->cam_b) * p->cam_a;
  const float cy = (p->cam_d - py) * p->cam_c;
  const float rl = rsq(__builtin_fmaf(cy, cy, __builtin_fmaf(cx, cx, 1.0f)));
  return f3(__builtin_fmaf(cy, p->cam[6], __builtin_fmaf(cx, p->cam[3], -p->cam[9])) * rl,
            __builtin_fmaf(cy, p->cam[7], __builtin_fmaf(cx, p->cam[4], -p->cam[10])) * rl,
            __builtin_fmaf(cy, p->cam[8], __builtin_fmaf(cx, p->cam[5], -p->cam[11])) * rl);
}

template <unsigned F>
__device__ __forceinline__ void camera_pos(KP p, const GroupPix& gp, int s, const LdsF* tb, float& px_out,
                                           float& py_out) {
  float px = (float)gp.x, py = (float)gp.y;
  if (p->aa_kind == 1) {  // grid() sampling.nim:5-18: sample s = (si, sj)
    int si, sj;
    if (p->log2_grid_m >= 0) {
      si = s & (p->grid_m - 1);
      sj = s >> p->log2_grid_m;
    } else {
      sj = div_small(s, p->grid_m, p->sample_step, si);
    }
    px += __builtin_fmaf((float)si, p->sample_step, p->sample_off);
    py += __builtin_fmaf((float)sj, p->sample_step, p->sample_off);
  } else if ((F & F_STOCHASTIC) && p->aa_kind == 2) {  // jitteredGrid (sampling.nim:21-33): no table needed
    double a, b;
    jittered_entry(rng_pixel_key(p->seed, gp.x, gp.y), p->grid_m, s, a, b);
    px += (float)a;
    py += (float)b;
  } else if ((F & F_STOCHASTIC) && tb) {
    const volatile LdsF* t = tb;
    px += t[s];
    py += t[p->spp + s];
  }
  px_out = px;
  py_out = py;
}
template <unsigned F>
__device__ __forceinline__ F3 camera_dir(KP p, const GroupPix& gp, int s, const LdsF* tb) {
  float px, py;
  camera_pos<F>(p, gp, s, tb, px, py);
  return camera_ray_dir(p, px, py);
}

// The object of the lowest pending lane of the lowest pending sample (-1:
// none). A branch per sample: the branch-free form (a readlane per sample,
// scalar selects) measured 5 % slower on C3.
template <int S>
__device__ __forceinline__ int first_pending(const unsigned long long (&pend)[S], const int (&hob)[S]) {
  int oi = -1;
#pragma unroll
  for (int k = S - 1; k >= 0; --k)
    if (pend[k]) oi = __builtin_amdgcn_readlane(hob[k], (int)__builtin_ctzll(pend[k]));
  return oi;
}

// Sample positions of a batch (S samples per lane: iterations it0 .. it0+S-1
// of a one-pixel wave) and their camera-ray directions; akGrid with m a
// power of two (C2-C5) as s = (s & (m-1), s >> log2 m), the sampler decided
// once for the batch.
template <unsigned F, int S>
__device__ __forceinline__ void batch_dirs(KP p, const GroupPix& gp, int it0, const LdsF* tb, F3 (&d)[S],
                                           bool (&sv)[S]) {
  float px[S], py[S];
  // validity without short-circuit branches (a per-lane && became an
  // exec-mask branch with the argument load inside, per sample)
  const int spp = p->spp;
  const int L = p->lanes_per_px;  // 64: one-pixel waves; 16: object-binned batches of 4 pixels
  if (p->aa_kind == 1 && p->log2_grid_m >= 0 && p->log2_grid_m <= p->log2_lanes) {
    // m divides L: sample s = it * L + sub keeps the lane's column
    // s & (m-1) = sub & (m-1) in every iteration — px (and the camera ray's
    // cx) once per batch, the same values as per sample
    const int mm = p->grid_m - 1, lg = p->log2_grid_m;
    const float st = p->sample_step, of = p->sample_off;
    const float pxl = (float)gp.x + __builtin_fmaf((float)(gp.sub & mm), st, of);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int s = (it0 + k) * L + gp.sub;
      sv[k] = gp.valid & (s < spp);
      px[k] = pxl;
      py[k] = (float)gp.y + __builtin_fmaf((float)(s >> lg), st, of);
    }
  } else if (p->aa_kind == 1 && p->log2_grid_m >= 0) {
    const int mm = p->grid_m - 1, lg = p->log2_grid_m;
    const float st = p->sample_step, of = p->sample_off;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int s = (it0 + k) * L + gp.sub;
      sv[k] = gp.valid & (s < spp);
      px[k] = (float)gp.x + __builtin_fmaf((float)(s & mm), st, of);
      py[k] = (float)gp.y + __builtin_fmaf((float)(s >> lg), st, of);
    }
  } else {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int s = (it0 + k) * L + gp.sub;
      sv[k] = gp.valid & (s < spp);
      camera_pos<F>(p, gp, s < spp ? s : 0, tb, px[k], py[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < S; ++k) d[k] = camera_ray_dir(p, px[k], py[k]);
}

// batch_dirs for the one-plane kernels' launches (akGrid, m | 64, every
// sample valid, one-pixel waves): camera_ray_dir of the batch's samples with
// the cx terms, which depend on the lane's column alone, formed once — the
// same roundings as per sample. (lean1q_loop forms its rays per virtual lane,
// in a layout of its own.)
template <int S>
__device__ __forceinline__ void oneplane_dirs(KP p, const GroupPix& gp, int it0, F3 (&d)[S]) {
  const int mm = p->grid_m - 1, lg = p->log2_grid_m;
  const float st = p->sample_step, of = p->sample_off;
  const float px = (float)gp.x + __builtin_fmaf((float)(gp.sub & mm), st, of);
  const float cx = (px - p->cam_b) * p->cam_a;
  const float q0 = __builtin_fmaf(cx, cx, 1.0f);
  const float ax = __builtin_fmaf(cx, p->cam[3], -p->cam[9]), ay = __builtin_fmaf(cx, p->cam[4], -p->cam[10]),
              az = __builtin_fmaf(cx, p->cam[5], -p->cam[11]);
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const int s = (it0 + k) * 64 + gp.sub;
    const float py = (float)gp.y + __builtin_fmaf((float)(s >> lg), st, of);
    const float cy = (p->cam_d - py) * p->cam_c;
    const float rl = rsq(__builtin_fmaf(cy, cy, q0));
    d[k] = f3(__builtin_fmaf(cy, p->cam[6], ax) * rl, __builtin_fmaf(cy, p->cam[7], ay) * rl,
              __builtin_fmaf(cy, p->cam[8], az) * rl);
  }
}

// tri_test for a ray that only needs the closest t (shadow rays): the best
// t's float bits replace the (t, face) key — a tie never changes t, so t,
// the culling limit tc and "found" follow tri_test's exactly. A lane that
// takes no part holds best = +0.0 (nothing is below it).
template <class TR>
__device__ __forceinline__ void tri_test_t(const TR& T, F3 o, F3 d, float& best, float& tc) {
  const float tx = o.x - T.v0[0], ty = o.y - T.v0[1], tz = o.z - T.v0[2];
  const float cx = __builtin_fmaf(ty, d.z, -tz * d.y);
  const float cy = __builtin_fmaf(tz, d.x, -tx * d.z);
  const float cz = __builtin_fmaf(tx, d.y, -ty * d.x);
  const float u = __builtin_fmaf(T.e2[0], cx, __builtin_fmaf(T.e2[1], cy, T.e2[2] * cz));
  const float v = __builtin_fmaf(T.e1n[0], cx, __builtin_fmaf(T.e1n[1], cy, T.e1n[2] * cz));
  const float det = __builtin_fmaf(T.nn[0], d.x, __builtin_fmaf(T.nn[1], d.y, T.nn[2] * d.z));
  const float tt = __builtin_fmaf(T.nn[0], tx, __builtin_fmaf(T.nn[1], ty, T.nn[2] * tz));
  const float t = tt * rcp(-det);
  const float g = fminf(fminf(fminf(u, v), det - (u + v)), det - 0.000001f);
  const float ts = g >= 0.0f ? t : -1.0f;
  const bool acc = __float_as_uint(ts) < __float_as_uint(best);
  best = acc ? ts : best;
  tc = acc ? ts : tc;
}

// tri_test_t on a face's LTri record (shadow rays to a light with records)
template <class LR>
__device__ __forceinline__ void ltri_test_t(const LR& L, F3 o, float& best, float& tc) {
  const float ts = ltri_t(L, o);
  const bool acc = __float_as_uint(ts) < __float_as_uint(best);
  best = acc ? ts : best;
  tc = acc ? ts : tc;
}

// The faces listed at ent[b, e) against the rays of the batch's samples
// whose bit is set in fl (wave-uniform), each face record fetched once for
// all of them. Camera rays (KEY): list_search's (t, face) key. Shadow rays
// (!KEY): tri_test_t and the exact early exit (a sample's lane retires once
// it holds a hit with t <= stop; the search ends when no lane the list is
// for — own[k], the lanes whose ray lies in this cell — is left: the other
// lanes test these faces only as a harmless superset, their own cell is
// searched in its turn).
// diag (RTMI_DIAG_LANES builds, else nullptr): += the lanes still searching
// at each face test of each flagged sample (lane occupancy of the search).
// Each step's four face records are staged through the wave's LDS slice
// instead of one scalar load per record (DESIGN.md "LDS staging": C3 0.912
// -> 0.895 ms, C5 79.5 -> 78.4 ms).
// Camera searches (KEY) test the TriFast records of the tree that `ent`
// names; shadow searches (!KEY) read the light's LTri records in entry
// order, lb = the cell-ordered copy aligned with `ent` (grid_rec_of: entry
// k's record at lb + 64 k) — one load per step, not the entries and then the
// records they name.
template <int S, bool KEY>
__device__ __forceinline__ int list_search_batch(KP p, const int32_t* ent, int b, int e, unsigned fl,
                                                  const F3 (&ro)[S], const F3 (&rd)[S], const float (&stop)[S],
                                                  const unsigned long long (&own)[S], unsigned long long (&key)[S],
                                                  float (&best)[S], float (&tc)[S], unsigned* diag = nullptr,
                                                  const char* lb = nullptr) {
  constexpr bool kCellRec = !KEY;
  // the record of entry k
  auto rec_at = [&](int k) -> const char* {
    return kCellRec ? lb + (size_t)(unsigned)k * sizeof(LTri) : lb + (unsigned)cp(ent)[k];
  };
  const int b_in = b;  // returns the number of faces tested (diagnostics)
  auto lanes = [&]() {
    if (diag) {
#pragma unroll
      for (int k = 0; k < S; ++k)
        if ((fl >> k) & 1u) *diag += pc(bal(tc[k] >= 0.0f));
    }
  };
  if constexpr (!KEY) {
    // a cell's first face alone: it is the one covering most of the cell
    // (rt_bins.cpp), so lanes in the umbra retire after one test
    if (b < e) {
      const LRegs T = load_ltri((const RT_CONST LTri*)rec_at(b));
      lanes();
      unsigned long long left = 0ull;
#pragma unroll
      for (int k = 0; k < S; ++k)
        if ((fl >> k) & 1u) {
          ltri_test_t(T, ro[k], best[k], tc[k]);
          tc[k] = tc[k] <= stop[k] ? -1.0f : tc[k];
          left |= bal(tc[k] >= 0.0f) & own[k];
        }
      if (left == 0ull) return 1;
      ++b;
    }
  }
  // LDS staging (DESIGN.md "LDS staging"): the 4 face records of a step
  // staged through the wave's LDS slice — lane 16 j + w loads dword w of
  // record j (one coalesced vector load for all four), then every lane reads
  // each record back as a broadcast (ds_read_b128 x 4) — instead of one
  // scalar load per record.
  __shared__ uint4 stage_lds[4][16];
  uint4* stage = stage_lds[threadIdx.x >> 6];
  for (int k0 = b; k0 < e; k0 += 4) {
    int r[4] = {0, 0, 0, 0};
    if constexpr (!kCellRec) {
      const RT_CONST int32_t* q = cp(ent) + k0;
      r[0] = q[0], r[1] = q[1], r[2] = q[2], r[3] = q[3];
    }
    {
      const int lane = (int)__lane_id(), j = lane >> 4, w = lane & 15;
      if constexpr (kCellRec) {  // the step's four records are 256 contiguous bytes
        const unsigned int* src = (const unsigned int*)rec_at(k0);
        ((unsigned int*)stage)[lane] = k0 + j < e ? src[lane] : 0u;
      } else {
        const int rj = j == 0 ? r[0] : j == 1 ? r[1] : j == 2 ? r[2] : r[3];
        const unsigned int* src = (const unsigned int*)((const char*)p->tree + (unsigned)rj);
        ((unsigned int*)stage)[lane] = k0 + j < e ? src[w] : 0u;
      }
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j > 0 && k0 + j >= e) break;
      if constexpr (KEY) {
        TriRegs T;
        {
          const uint4 a = stage[4 * j + 0], bq = stage[4 * j + 1], c = stage[4 * j + 2], d4 = stage[4 * j + 3];
          T.v0[0] = __uint_as_float(a.x), T.v0[1] = __uint_as_float(a.y), T.v0[2] = __uint_as_float(a.z);
          T.id = a.w;
          T.e2[0] = __uint_as_float(bq.x), T.e2[1] = __uint_as_float(bq.y), T.e2[2] = __uint_as_float(bq.z);
          T.e1n[0] = __uint_as_float(c.x), T.e1n[1] = __uint_as_float(c.y), T.e1n[2] = __uint_as_float(c.z);
          T.nn[0] = __uint_as_float(d4.x), T.nn[1] = __uint_as_float(d4.y), T.nn[2] = __uint_as_float(d4.z);
        }
        lanes();
#pragma unroll
        for (int k = 0; k < S; ++k)
          if ((fl >> k) & 1u) tri_test(T, ro[k], rd[k], key[k], tc[k]);
      } else {
        LRegs T;
        {
          const uint4 a = stage[4 * j + 0], bq = stage[4 * j + 1], c = stage[4 * j + 2], d4 = stage[4 * j + 3];
          T.p[0] = __uint_as_float(a.x), T.p[1] = __uint_as_float(a.y), T.p[2] = __uint_as_float(a.z);
          T.cu = __uint_as_float(a.w);
          T.q[0] = __uint_as_float(bq.x), T.q[1] = __uint_as_float(bq.y), T.q[2] = __uint_as_float(bq.z);
          T.cv = __uint_as_float(bq.w);
          T.tv[0] = __uint_as_float(c.x), T.tv[1] = __uint_as_float(c.y), T.tv[2] = __uint_as_float(c.z);
          T.ct = __uint_as_float(c.w);
          T.id = d4.x;
        }
        lanes();
#pragma unroll
        for (int k = 0; k < S; ++k)
          if ((fl >> k) & 1u) ltri_test_t(T, ro[k], best[k], tc[k]);
      }
    }
    if constexpr (!KEY) {
      unsigned long long left = 0ull;
#pragma unroll
      for (int k = 0; k < S; ++k)
        if ((fl >> k) & 1u) {
          tc[k] = tc[k] <= stop[k] ? -1.0f : tc[k];
          left |= bal(tc[k] >= 0.0f) & own[k];
        }
      if (left == 0ull) return min(e, k0 + 4) - b_in;
    }
  }
  return e - b_in;
}

// The mesh's AABB gate (TriangleMesh.intersect, geom.nim:339-341) in the
// traversal's slab form, as trace() forms it: a ray starting inside the box
// misses.
__device__ __forceinline__ bool mesh_gate(const FObj& ob, const SlabRay& sr) {
  const float ax = __builtin_fmaf(ob.lo[0], sr.ni.x, -sr.oi.x), bx = __builtin_fmaf(ob.hi[0], sr.ni.x, -sr.oi.x);
  const float ay = __builtin_fmaf(ob.lo[1], sr.ni.y, -sr.oi.y), by = __builtin_fmaf(ob.hi[1], sr.ni.y, -sr.oi.y);
  const float az = __builtin_fmaf(ob.lo[2], sr.ni.z, -sr.oi.z), bz = __builtin_fmaf(ob.hi[2], sr.ni.z, -sr.oi.z);
  const float gmin = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  const float gmax = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * 1.00000024f;
  return gmin <= gmax && gmin >= 0.0f;
}

// The light-grid shadow search of every batch (mesh_search's, S rays per
// lane): the shadow rays (ro[k], rd[k]), in the mesh's frame, of the lanes
// pm[k] towards distant light li against the faces of their light-grid
// cells (light_cell) — every distinct cell of the batch in turn, each round
// retiring at least the lane the cell was taken from — with the exact early
// exit. lim[k]: the sample's limit, the closest t so far (+inf: none);
// stop0[k]: mesh_search's stop distance (a lane retires on a found hit with
// t <= stop), clamped here to the float below the limit; best[k]: out, the
// closest face's t below the limit — a participating lane found one iff
// best[k] != lim[k] bit for bit. A float32-safe lane off the grid can hit no
// face. Returns false, nothing searched, when the BVH is needed: a light
// without a grid, or a participating lane beyond the grid's float32-safe radius.
// diag: what diagnostic builds count into (nullptr: nothing; a default build
// has no counting code). RTMI_DIAG_GEN_COUNT: LANE_NODES += rays in searched
// cells, NODE_FETCH += cells, TRI_FETCH += face tests x flagged samples.
// RTMI_DIAG_LANES: NODE_FETCH += face tests x flagged samples, LANE_NODES +=
// the lanes still searching at each.
template <int S>
__device__ __forceinline__ bool light_cell_search(KP q, int li, const F3 (&ro)[S], const F3 (&rd)[S],
                                                  const float (&lim)[S], const float (&stop0)[S],
                                                  const unsigned long long (&pm)[S], float (&best)[S],
                                                  Stats32* diag) {
  (void)diag;
  if (!q->grids || q->grids[li].gu <= 0) return false;
  const RT_CONST LightGrid& G = cp(q->grids)[li];
  int cell[S];
  float stop[S], tc[S];
  unsigned long long todo[S], unused[S], left = 0ull, unsafe = 0ull;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const bool part = lane_in(pm[k]);
    stop[k] = fminf(stop0[k], __uint_as_float(__float_as_uint(lim[k]) - 1u));
    tc[k] = part ? lim[k] : -1.0f;   // the culling limit; -1: the lane takes no part
    best[k] = part ? lim[k] : 0.0f;  // (+0: nothing is below it)
    bool safe, on;
    cell[k] = light_cell(G, ro[k], safe, on);
    todo[k] = bal(part && cell[k] >= 0);
    unsafe |= bal(part && !safe);
    left |= todo[k];
    unused[k] = 0ull;
  }
  if (unsafe != 0ull) return false;
  const int32_t* bent = q->grid_ent + G.ent_base;
  while (left != 0ull) {
    int kb = -1;
#pragma unroll
    for (int k = S - 1; k >= 0; --k)
      if (todo[k]) kb = __builtin_amdgcn_readlane(cell[k], (int)__builtin_ctzll(todo[k]));
    unsigned fl = 0u;
    unsigned long long own[S];
    left = 0ull;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      own[k] = bal(cell[k] == kb) & todo[k];
      todo[k] &= ~own[k];
      left |= todo[k];
      fl |= own[k] != 0ull ? (1u << k) : 0u;
#ifdef RTMI_DIAG_GEN_COUNT
      if (diag) diag->v[STAT_LANE_NODES] += pc(own[k]);
#endif
    }
    unsigned* lanes = nullptr;
#ifdef RTMI_DIAG_LANES
    unsigned dl = 0u;
    if (diag) lanes = &dl;
#endif
    const int nt = list_search_batch<S, false>(q, bent, cp(q->grid_off)[kb], cp(q->grid_off)[kb + 1], fl, ro, rd, stop,
                                               own, unused, best, tc, lanes, grid_rec_of(q, li, G));
    (void)nt;
#ifdef RTMI_DIAG_LANES
    if (diag) {
      diag->v[STAT_NODE_FETCH] += (unsigned)nt * (unsigned)__builtin_popcount(fl);
      diag->v[STAT_LANE_NODES] += dl;
    }
#endif
#ifdef RTMI_DIAG_GEN_COUNT
    if (diag) {
      diag->v[STAT_NODE_FETCH] += 1u;
      diag->v[STAT_TRI_FETCH] += (unsigned)nt * (unsigned)__builtin_popcount(fl);
    }
#endif
  }
  return true;
}

// General pixels, S samples per lane at once (two-class launches: the
// pixels that are not lean). Scenes of one mesh object (FastParams
// .shadow_mesh), analytic objects and distant lights only, no reflection;
// one-pixel waves with the pixel's record (pinfo) and its camera-ray list.
// The same per-sample arithmetic as shade_path / trace / mesh_search —
// camera rays search the pixel's face list, shadow rays to a light whose
// skip bit is clear search their light-grid cells with the exact early
// exit — with each face record, object record and loop step paid once per
// 64 x S rays instead of per 64. No BVH here: when a shadow ray would need
// it (a light without a grid, an origin beyond the grid's float32-safe
// radius) the batch returns false
// before adding anything and the caller renders the whole pixel with the
// one-sample loop. Stats go to `wi` (committed by the caller). Frames and
// Stats bit-identical to the one-sample loop (test_gpu_split.py against
// RT_FLAG_NO_BATCH / NO_SPLIT / NO_BINNING).
template <unsigned F, int S>
__device__ __forceinline__ bool gen_batch(KP p, const GroupPix& gp, int it0, const LdsF* tb, unsigned pinfo,
                                          LdsF* ls, Acc& acc, Stats32& wi) {
  static_assert(3 * S <= kLdsSlots, "albedo stash: 3 LDS slots per sample");
  // kernel arguments re-read through a laundered pointer at each stage
  // (params()): hoisted, the many fields this path reads stay pinned in
  // SGPRs across the whole batch and spill
  p = params();
  const F3 o = f3(p->cam[0], p->cam[1], p->cam[2]);
  F3 d[S];
  bool sv[S];
  batch_dirs<F, S>(p, gp, it0, tb, d, sv);
  unsigned nprim = 0u;
  // th: -1 invalid sample, +inf sky, else the closest hit's t (lean_batch)
  float th[S];
  int hob[S], htri[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    nprim += pc(bal(sv[k]));
    th[k] = sv[k] ? finf() : -1.0f;
    hob[k] = -1;
    htri[k] = -1;
  }
  const int nobj = p->nobj, mesh = p->shadow_mesh;
  unsigned hitl = 0u;
  // camera rays: trace (renderer.nim:47-67) over the objects in scene order
  for (int i = 0; i < nobj; ++i) {
    p = params();
    const FObj ob = at(p->objs, i);
    if (i == mesh) {
      // an empty pixel list: no camera ray of the pixel can hit the mesh
      // (trace's no_mesh: the gate's verdict cannot matter)
      if ((pinfo & kPixCount) == 0u || ob.root < 0) continue;
      F3 ro[S], rd[S];
      unsigned long long key[S], key0[S];
      float tc[S], unused[S];
      unsigned long long anyp = 0ull, nomask[S];
#pragma unroll
      for (int k = 0; k < S; ++k) {
        to_object<F>(p, ob, i, o, d[k], ro[k], rd[k]);
        const bool part = sv[k] && mesh_gate(ob, slab_ray(ro[k], rd[k]));
        tc[k] = part ? th[k] : -1.0f;
        key0[k] = part ? tkey(th[k], 0u) : 0ull;
        key[k] = key0[k];
        unused[k] = 0.0f;
        nomask[k] = 0ull;
        anyp |= bal(part);
      }
      if (anyp != 0ull) {  // the wave's one pixel: one list for every sample (gen_batch's caller
                           // sends a pixel whose list overflowed its slots to the one-sample loop)
        const int pu = __builtin_amdgcn_readfirstlane(gp.y * p->width + gp.x);
        const int b = pu << p->slot_lg;
        list_search_batch<S, true>(p, p->pix_slots, b, b + (int)(pinfo & kPixCount), (1u << S) - 1u,
                                   ro, rd, unused, nomask, key, unused, tc);
      }
#pragma unroll
      for (int k = 0; k < S; ++k) {  // found => 0 <= t < th: the hit counts (trace's update rule)
        const bool c = key[k] != key0[k];
        th[k] = c ? __uint_as_float((unsigned int)(key[k] >> 32)) : th[k];
        hob[k] = c ? i : hob[k];
        htri[k] = c ? (int)(unsigned int)key[k] : htri[k];
        hitl += c ? 1u : 0u;
      }
      continue;
    }
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const float t = analytic_t<F>(p, ob, i, o, d[k]);
      const bool c = t >= 0.0f && t < th[k];  // (t >= 0 ? t : inf) < th, th <= inf
      th[k] = c ? t : th[k];
      hob[k] = c ? i : hob[k];
      hitl += c ? 1u : 0u;
    }
  }
  // shade (renderer.nim:71-127): normals per distinct object hit (mesh:
  // the face normal by face id, renderer.nim:84-88), shadow origins
  unsigned long long litm[S], pend[S], skym[S];  // lit / sky lanes per sample
  F3 N[S], so[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    litm[k] = m_lt(th[k], finf()) & m_ge(th[k], 0.0f);
    skym[k] = bal(th[k] == finf());
    pend[k] = litm[k];
    N[k] = f3(0.0f, 0.0f, 0.0f);
    so[k] = f3(__builtin_fmaf(d[k].x, th[k], o.x), __builtin_fmaf(d[k].y, th[k], o.y),
               __builtin_fmaf(d[k].z, th[k], o.z));  // the hit point until N is known
  }
  for (;;) {
    const int oi = first_pending<S>(pend, hob);
    if (oi < 0) break;
    int oi_cmp = oi;
    asm volatile("" : "+s"(oi_cmp));
    p = params();
    const FObj ob = at(p->objs, oi);
    const RT_CONST FObjX& ox = at(p->objx, oi);
    const bool is_mesh = (F & F_MESH) && ob.type == GEOM_MESH;
    const int nbase = ox.normal_base;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const unsigned long long mine = bal(hob[k] == oi_cmp) & pend[k];
      pend[k] &= ~mine;
      const bool mi = lane_in(mine);
      F3 n;
      if (is_mesh) {
        // every lane loads (face 0 for the others): no exec-mask branch
        const float* fn = p->normals + 3 * (size_t)(nbase + (mi ? htri[k] : 0));
        n = f3(fn[0], fn[1], fn[2]);
      } else {
        F3 ho, unused;
        to_object<F>(p, ob, oi, so[k], f3(0.0f, 0.0f, 0.0f), ho, unused);
        n = analytic_normal<F>(ob, ho);
      }
      if ((F & F_XF_GENERAL) && ob.xf == XF_GENERAL) {  // object_to_world * n, not re-normalised
        const float* m = ox.o2w;
        n = f3(__builtin_fmaf(m[0], n.x, __builtin_fmaf(m[3], n.y, m[6] * n.z)),
               __builtin_fmaf(m[1], n.x, __builtin_fmaf(m[4], n.y, m[7] * n.z)),
               __builtin_fmaf(m[2], n.x, __builtin_fmaf(m[5], n.y, m[8] * n.z)));
      }
      N[k] = f3(mi ? n.x : N[k].x, mi ? n.y : N[k].y, mi ? n.z : N[k].z);
      // albedo / pi waits in LDS (slots 3k..3k+2) until the lights are summed
      if (mi) lds_put3(ls, 3 * k, f3(ox.albedo_pi[0], ox.albedo_pi[1], ox.albedo_pi[2]));
    }
  }
  const float bias = p->bias;
#pragma unroll
  for (int k = 0; k < S; ++k)
    so[k] = f3(__builtin_fmaf(N[k].x, bias, so[k].x), __builtin_fmaf(N[k].y, bias, so[k].y),
               __builtin_fmaf(N[k].z, bias, so[k].z));
  // one shadow ray per distant light and lit sample
  F3 E[S];
  unsigned long long anylit = 0ull;
  unsigned nlit = 0u;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    E[k] = f3(0.0f, 0.0f, 0.0f);
    anylit |= litm[k];
    nlit += pc(litm[k]);
  }
  const int nl = anylit ? p->nlight : 0;
  const unsigned skipw = pinfo >> 24;  // bit l: no shadow ray to light l can meet the mesh
  for (int li = 0; li < nl; ++li) {
    p = params();
    const FLight L = at(p->lights, li);
    const F3 sd = f3(-L.v[0], -L.v[1], -L.v[2]);
    float ts[S];  // unlit samples start at 0 (take no part)
#pragma unroll
    for (int k = 0; k < S; ++k) ts[k] = lane_in(litm[k]) ? finf() : 0.0f;
    for (int i = 0; i < nobj; ++i) {
      p = params();
      const FObj ob = at(p->objs, i);
      if (i == mesh) {
        if ((li < 8 && ((skipw >> li) & 1u) != 0u) || ob.root < 0) continue;
        F3 ro[S], rd[S];
        unsigned long long pm[S], anyp = 0ull;
#pragma unroll
        for (int k = 0; k < S; ++k) {
          to_object<F>(p, ob, i, so[k], sd, ro[k], rd[k]);
          pm[k] = bal(lane_in(litm[k]) && mesh_gate(ob, slab_ray(ro[k], rd[k])));
          anyp |= pm[k];
        }
        if (anyp == 0ull) continue;  // no lane enters the mesh's box
        // mesh_search: the exact early exit's stop distance (the analytic
        // objects after the mesh)
        float stop[S], best[S];
#pragma unroll
        for (int k = 0; k < S; ++k) stop[k] = finf();
        for (int j = i + 1; j < nobj; ++j) {
          const FObj oj = at(p->objs, j);
#pragma unroll
          for (int k = 0; k < S; ++k) {
            const float tj = analytic_t<F>(p, oj, j, so[k], sd);
            stop[k] = tj >= 0.0f ? fminf(stop[k], tj) : stop[k];
          }
        }
        // the light grid's cells; false: the BVH, the caller's one-sample loop
        if (!light_cell_search<S>(p, li, ro, rd, ts, stop, pm, best, &wi)) return false;
#ifdef RTMI_DIAG_GEN_COUNT
        wi.v[STAT_LANE_NODES] += 1u;  // diagnostic: searched (light, batch) visits
#endif
#pragma unroll
        for (int k = 0; k < S; ++k) {  // found => 0 <= t < ts: the hit counts
          const bool c = lane_in(pm[k]) && __float_as_uint(best[k]) != __float_as_uint(ts[k]);
          ts[k] = c ? best[k] : ts[k];
          hitl += c ? 1u : 0u;
        }
        continue;
      }
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const float t = analytic_t<F>(p, ob, i, so[k], sd);
        const bool c = t >= 0.0f && t < ts[k];
        ts[k] = c ? t : ts[k];
        hitl += c ? 1u : 0u;
      }
    }
#pragma unroll
    for (int k = 0; k < S; ++k) {  // unoccluded: shadeDiffuse (shader.nim:12-17)
      const bool vis = lane_in(litm[k]) && !(ts[k] < finf());
      irr_add(E[k], L.ci, vis ? fmaxf(dot3(N[k], sd), 0.0f) : 0.0f);
    }
  }
  // the samples' colours in order: albedo / pi x E, the background for the sky
  p = params();
  const F3 bg = f3(p->bg[0], p->bg[1], p->bg[2]);
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const bool lt = lane_in(litm[k]), sky = lane_in(skym[k]);
    const F3 a = mul3(lds_get3(ls, 3 * k), E[k]);
    const F3 c = f3(lt ? a.x : (sky ? bg.x : 0.0f), lt ? a.y : (sky ? bg.y : 0.0f),
                    lt ? a.z : (sky ? bg.z : 0.0f));
    acc_add3(acc, c.x, c.y, c.z);
  }
  wi.v[STAT_PRIMARY] += nprim;
  wi.v[STAT_SHADOW] += (unsigned)nl * nlit;
#ifdef RTMI_DIAG_GEN_COUNT
  wi.v[STAT_LANE_TRIS] += 1u;  // diagnostic: batches
#endif
  wi.v[STAT_HITS] += wave_sum(hitl);
  return true;
}

// General pixels of the one-plane scenes (lean1q_loop's: one mesh + one
// translated plane, distant lights, akGrid m | 64, every sample valid):
// gen_batch with the two objects written out in scene order instead of the
// object / dispatch loops — the plane's camera and shadow tests in
// lean1q_loop's form, its normal (0, 1, 0), the albedo a select of the
// two objects' (no LDS stash), the camera's cx terms per lane and pixel.
// The mesh searches (pixel list, light-grid cells, the early exit's stop)
// are gen_batch's, unchanged. Returns false, before adding anything, where
// gen_batch does (a shadow ray that needs the BVH). Frames and Stats
// bit-identical to gen_batch (tests/test_gpu_split.py, RT_FLAG_NO_GEN1).
// (Packing the two samples' rays of a light cell into one slot when they fit
// one wave was measured: exact but slower, C3 0.901 -> 0.918 ms, C5 78.5 ->
// 79.4 ms — the pairing and permutes cost more than the face tests they save,
// and the kernel's spills grow from 4 to 18 VGPRs; DESIGN.md "Live-ray
// compaction of the light-cell searches".)
template <int S, int NL>
__device__ __forceinline__ bool gen1_batch(KP p, const GroupPix& gp, int pu, int it0, unsigned pinfo, Acc& acc,
                                           Stats32& wi) {
  p = params();
  const int mesh = p->shadow_mesh, po = 1 - mesh;  // the scene's two objects
  const F3 o = f3(p->cam[0], p->cam[1], p->cam[2]);
  F3 d[S];
  oneplane_dirs<S>(p, gp, it0, d);
  float th[S];
  bool hm[S];  // the closest hit is the mesh's
  int htri[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    th[k] = finf();
    hm[k] = false;
    htri[k] = -1;
  }
  unsigned hitl = 0u;
  const FObj mob = at(p->objs, mesh);
  const float pty = at(p->objs, po).t[1];
  // trace (renderer.nim:47-67) of the camera rays: the two objects in order
  auto camera_plane = [&]() {
    const float nroy = -(o.y + pty);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const float t = fabsf(d[k].y) > 1e-6f ? nroy * rcp(d[k].y) : -finf();
      const bool c = t >= 0.0f && t < th[k];
      th[k] = c ? t : th[k];
      hm[k] = c ? false : hm[k];
      hitl += c ? 1u : 0u;
    }
  };
  auto camera_mesh = [&]() {
    if ((pinfo & kPixCount) == 0u || mob.root < 0) return;  // an empty pixel list: no camera ray can hit it
    F3 ro[S], rd[S];
    unsigned long long key[S], key0[S], anyp = 0ull, nomask[S];
    float tc[S], unused[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
      ro[k] = f3(o.x + mob.t[0], o.y + mob.t[1], o.z + mob.t[2]);
      rd[k] = d[k];
#ifdef RTMI_DIAG_MESH1_CEIL  // timing only (wrong images): no camera gate
      const bool part = true;
#else
      const bool part = mesh_gate(mob, slab_ray(ro[k], rd[k]));
#endif
      tc[k] = part ? th[k] : -1.0f;
      key0[k] = part ? tkey(th[k], 0u) : 0ull;
      key[k] = key0[k];
      unused[k] = 0.0f;
      nomask[k] = 0ull;
      anyp |= bal(part);
    }
    if (anyp != 0ull) {
      const KP q = params();
      const int b = pu << q->slot_lg;
#ifdef RTMI_DIAG_LANES  // diagnostic: camera face tests (x samples) and the lanes still searching
      unsigned dl = 0u;
      wi.v[STAT_TRI_FETCH] += (unsigned)(pinfo & kPixCount) * (unsigned)S;
      list_search_batch<S, true>(q, q->pix_slots, b, b + (int)(pinfo & kPixCount), (1u << S) - 1u,
                                 ro, rd, unused, nomask, key, unused, tc, &dl);
      wi.v[STAT_LANE_TRIS] += dl;
#else
      list_search_batch<S, true>(q, q->pix_slots, b, b + (int)(pinfo & kPixCount), (1u << S) - 1u,
                                 ro, rd, unused, nomask, key, unused, tc);
#endif
    }
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const bool c = key[k] != key0[k];
      th[k] = c ? __uint_as_float((unsigned int)(key[k] >> 32)) : th[k];
      hm[k] = c ? true : hm[k];
      htri[k] = c ? (int)(unsigned int)key[k] : htri[k];
      hitl += c ? 1u : 0u;
    }
  };
  if (mesh == 0) {
    camera_mesh();
    camera_plane();
  } else {
    camera_plane();
    camera_mesh();
  }
  // shade (renderer.nim:71-127): N = the face normal (renderer.nim:84-88) or
  // the plane's (0, 1, 0); the shadow origins hitW + N * bias
  p = params();
  unsigned long long litm[S], anylit = 0ull, anymesh = 0ull;
  unsigned nlit = 0u;
  F3 N[S], so[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    litm[k] = m_lt(th[k], finf()) & m_ge(th[k], 0.0f);
    anylit |= litm[k];
    nlit += pc(litm[k]);
    anymesh |= bal(hm[k]) & litm[k];
    so[k] = f3(__builtin_fmaf(d[k].x, th[k], o.x), __builtin_fmaf(d[k].y, th[k], o.y),
               __builtin_fmaf(d[k].z, th[k], o.z));
  }
  const int nbase = at(p->objx, mesh).normal_base;
  // mesh pixels (off with RT_FLAG_NO_MESH1). all: every sample of the batch
  // is lit by a hit on the mesh, so the selects below are wave-uniformly
  // decided — N the face normal, the albedo the mesh's, no background.
  const bool m1 = (p->flags & RT_DEV_FLAG_NO_MESH1) == 0;
  bool all = m1;
  {
    const unsigned long long full = bal(true);
#pragma unroll
    for (int k = 0; k < S; ++k) all = all && (bal(hm[k]) & litm[k]) == full;
  }
#ifdef RTMI_DIAG_MESH1_CEIL  // timing only (wrong images): every pixel with a list takes the straight path
  all = (pinfo & kPixCount) != 0u;
#endif
  if (all) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
#ifdef RTMI_DIAG_MESH1_CEIL
      const float* fn = p->normals + 3 * (size_t)(nbase + max(htri[k], 0));
#else
      const float* fn = p->normals + 3 * (size_t)(nbase + htri[k]);
#endif
      N[k] = f3(fn[0], fn[1], fn[2]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const bool lt = lane_in(litm[k]);
      F3 n = f3(0.0f, 1.0f, 0.0f);
      if (anymesh != 0ull) {  // every lane loads (face 0 for the others): no exec-mask branch
        const bool mi = lt && hm[k];
        const float* fn = p->normals + 3 * (size_t)(nbase + (mi ? htri[k] : 0));
        n = f3(mi ? fn[0] : n.x, mi ? fn[1] : n.y, mi ? fn[2] : n.z);
      }
      N[k] = f3(lt ? n.x : 0.0f, lt ? n.y : 0.0f, lt ? n.z : 0.0f);
    }
  }
  const float bias = p->bias;
#pragma unroll
  for (int k = 0; k < S; ++k)
    so[k] = f3(__builtin_fmaf(N[k].x, bias, so[k].x), __builtin_fmaf(N[k].y, bias, so[k].y),
               __builtin_fmaf(N[k].z, bias, so[k].z));
  // gate: the sample slots whose shadow rays evaluate the mesh gate. A slot
  // whose lit lanes' origins all lie strictly inside the call's inset box
  // (in the mesh's frame, as shadow_mesh forms them) does not: the gate is
  // false there for every light (rt_bins_geom.h lemma 1).
  unsigned gate = (1u << S) - 1u;
  if (m1) {
    const float lx = p->in_lo[0], ly = p->in_lo[1], lz = p->in_lo[2];
    const float hx = p->in_hi[0], hy = p->in_hi[1], hz = p->in_hi[2];
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const bool in = inset_inside(lx, ly, lz, hx, hy, hz, so[k].x + mob.t[0], so[k].y + mob.t[1], so[k].z + mob.t[2]);
      if ((litm[k] & ~bal(in)) == 0ull) gate &= ~(1u << k);
    }
  }
#ifdef RTMI_DIAG_MESH1_CEIL  // timing only: no shadow gate for a pixel with a list
  if (all) gate = 0u;
#endif
  if (all && gate == 0u) {
    // the straight path: every sample a mesh hit whose shadow rays cannot
    // meet the mesh. What is left per light is the plane's shadow test and
    // the irradiance term — the operations of the code below, operand for
    // operand, with litm full, hm true and every mesh gate false.
    F3 E[S];
#pragma unroll
    for (int k = 0; k < S; ++k) E[k] = f3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int li = 0; li < NL; ++li) {
      p = params();
      const FLight L = at(p->lights, li);
      const F3 sd = f3(-L.v[0], -L.v[1], -L.v[2]);
      const float mulp = fabsf(sd.y) > 1e-6f ? rcp(sd.y) : __builtin_nanf("");
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const float tpl = -(so[k].y + pty) * mulp;
        const bool c = tpl >= 0.0f && tpl < finf();  // ts = +inf: the plane occludes
        hitl += c ? 1u : 0u;
        irr_add(E[k], L.ci, c ? 0.0f : fmaxf(dot3(N[k], sd), 0.0f));
      }
    }
    p = params();
    const RT_CONST FObjX& mx = at(p->objx, mesh);
    const F3 am = f3(mx.albedo_pi[0], mx.albedo_pi[1], mx.albedo_pi[2]);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const F3 a = mul3(am, E[k]);
      acc_add3(acc, a.x, a.y, a.z);
    }
    wi.v[STAT_PRIMARY] += (unsigned)(64 * S);
    wi.v[STAT_SHADOW] += (unsigned)(NL * 64 * S);
    wi.v[STAT_HITS] += wave_sum(hitl);
#if !defined(RTMI_DIAG_GEN_COUNT) && !defined(RTMI_DIAG_LANES)
    wi.v[STAT_LANE_TRIS] += 1u;  // rt_scene_last_mesh1 (a slot only counting launches write otherwise)
#endif
    return true;
  }
  // one shadow ray per distant light and lit sample
  F3 E[S];
#pragma unroll
  for (int k = 0; k < S; ++k) E[k] = f3(0.0f, 0.0f, 0.0f);
  const unsigned skipw = pinfo >> 24;
  if (anylit != 0ull) {
#pragma unroll
    for (int li = 0; li < NL; ++li) {
      p = params();
      const FLight L = at(p->lights, li);
      const F3 sd = f3(-L.v[0], -L.v[1], -L.v[2]);
      // the plane's shadow test (lean1q_loop's form: NaN multiplier when parallel)
      const float mulp = fabsf(sd.y) > 1e-6f ? rcp(sd.y) : __builtin_nanf("");
      float ts[S], tpl[S];
#pragma unroll
      for (int k = 0; k < S; ++k) {
        ts[k] = lane_in(litm[k]) ? finf() : 0.0f;
        tpl[k] = -(so[k].y + pty) * mulp;
      }
      auto shadow_plane = [&]() {
#pragma unroll
        for (int k = 0; k < S; ++k) {
          const bool c = tpl[k] >= 0.0f && tpl[k] < ts[k];
          ts[k] = c ? tpl[k] : ts[k];
          hitl += c ? 1u : 0u;
        }
      };
      // the mesh (gen_batch's search), false: the BVH would be needed
      auto shadow_mesh = [&]() -> bool {
        if (((skipw >> li) & 1u) != 0u || mob.root < 0) return true;
        F3 ro[S], rd[S];
        unsigned long long pm[S], anyp = 0ull;
#pragma unroll
        for (int k = 0; k < S; ++k) {
          ro[k] = f3(so[k].x + mob.t[0], so[k].y + mob.t[1], so[k].z + mob.t[2]);
          rd[k] = sd;
          pm[k] = ((gate >> k) & 1u) != 0u ? bal(lane_in(litm[k]) && mesh_gate(mob, slab_ray(ro[k], rd[k]))) : 0ull;
          anyp |= pm[k];
        }
        if (anyp == 0ull) return true;
        // the exact early exit's stop: the plane after the mesh (if it is)
        float stop[S], best[S];
#pragma unroll
        for (int k = 0; k < S; ++k) {
          stop[k] = finf();
          if (mesh == 0) stop[k] = tpl[k] >= 0.0f ? fminf(stop[k], tpl[k]) : stop[k];
        }
        if (!light_cell_search<S>(params(), li, ro, rd, ts, stop, pm, best, &wi)) return false;
#pragma unroll
        for (int k = 0; k < S; ++k) {  // found => 0 <= t < ts: the hit counts
          const bool c = lane_in(pm[k]) && __float_as_uint(best[k]) != __float_as_uint(ts[k]);
          ts[k] = c ? best[k] : ts[k];
          hitl += c ? 1u : 0u;
        }
        return true;
      };
      if (mesh == 0) {
        if (!shadow_mesh()) return false;
        shadow_plane();
      } else {
        shadow_plane();
        if (!shadow_mesh()) return false;
      }
#pragma unroll
      for (int k = 0; k < S; ++k) {  // unoccluded: shadeDiffuse (shader.nim:12-17)
        const bool vis = lane_in(litm[k]) && !(ts[k] < finf());
        irr_add(E[k], L.ci, vis ? fmaxf(dot3(N[k], sd), 0.0f) : 0.0f);
      }
    }
  }
  // the samples' colours in order: albedo / pi x E (the hit object's), the
  // background for the sky (every sample valid: not lit = sky)
  p = params();
  const RT_CONST FObjX& mx = at(p->objx, mesh);
  const RT_CONST FObjX& px_ = at(p->objx, po);
  const F3 am = f3(mx.albedo_pi[0], mx.albedo_pi[1], mx.albedo_pi[2]);
  const F3 ap = f3(px_.albedo_pi[0], px_.albedo_pi[1], px_.albedo_pi[2]);
  const F3 bg = f3(p->bg[0], p->bg[1], p->bg[2]);
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const bool lt = lane_in(litm[k]);
    const F3 alb = f3(hm[k] ? am.x : ap.x, hm[k] ? am.y : ap.y, hm[k] ? am.z : ap.z);
    const F3 a = mul3(alb, E[k]);
    acc_add3(acc, lt ? a.x : bg.x, lt ? a.y : bg.y, lt ? a.z : bg.z);
  }
  wi.v[STAT_PRIMARY] += (unsigned)(64 * S);
  wi.v[STAT_SHADOW] += (unsigned)NL * nlit;
  wi.v[STAT_HITS] += wave_sum(hitl);
  return true;
}

// gen1_batch for a ground pixel (rt_common.h kGenGroundBit: an empty camera
// list, and this call's build proved the pixel uniform-lit, rt_bins_geom.h
// uniform_class): every camera ray hits the plane at a positive finite t,
// the normal is (0, 1, 0), no shadow ray meets the plane (its t is a negative
// number: lit_ok), so a sample's colour depends on one bit per light whose
// skip bit is clear — whether its shadow ray meets the mesh. What is left of
// gen1_batch per sample: d, th and the shadow origin in its expressions (the
// FMAs with N = (0, 1, 0) included: every later bit depends on them), and
// per unskipped light the mesh gate, the cell and the cell loop (stop = the
// float below +inf either way round the two objects, the plane's t being
// negative). No camera select chain, hit masks, face normals, plane shadow
// test or albedo select; a skipped light costs its irradiance term. The
// same irr_add chain in light order, mul3 and acc_add3 in sample order, the
// same Stats (every sample a hit with NL shadow rays, + the occluded pairs)
// and the same fallback (false before anything is added). Frames and Stats
// bit-identical to gen1_batch (tests/test_gpu_ground.py, RT_FLAG_NO_GROUND1).
// S = RTMI_GROUND_BATCH samples per lane: 4 = the whole 256-sample pixel at
// once (iters % 4 == 0, rtmi.cpp lean1_ok), so a light cell the pixel's
// samples share is searched once for all of them.
#ifndef RTMI_GROUND_BATCH
#define RTMI_GROUND_BATCH 4
#endif
constexpr int kGroundBatch = RTMI_GROUND_BATCH;
static_assert(kGroundBatch == 1 || kGroundBatch == 2 || kGroundBatch == 4, "iters is a multiple of 4");
template <int S, int NL>
__device__ __forceinline__ bool ground1_batch(KP p, const GroupPix& gp, int it0, unsigned pinfo, Acc& acc,
                                              Stats32& wi) {
  p = params();
  const int mesh = p->shadow_mesh, po = 1 - mesh;
  const FObj mob = at(p->objs, mesh);
  F3 ro[S];  // the shadow origins in the mesh's frame (the same for every light)
  {
    const F3 o = f3(p->cam[0], p->cam[1], p->cam[2]);
    const float nroy = -(o.y + at(p->objs, po).t[1]), bias = p->bias;
    F3 dd[S];
    oneplane_dirs<S>(p, gp, it0, dd);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const F3 d = dd[k];
      const float th = nroy * rcp(d.y);
      const F3 hw = f3(__builtin_fmaf(d.x, th, o.x), __builtin_fmaf(d.y, th, o.y), __builtin_fmaf(d.z, th, o.z));
      const F3 so = f3(__builtin_fmaf(0.0f, bias, hw.x), __builtin_fmaf(1.0f, bias, hw.y),
                       __builtin_fmaf(0.0f, bias, hw.z));
      ro[k] = f3(so.x + mob.t[0], so.y + mob.t[1], so.z + mob.t[2]);
    }
  }
  // per light and sample: the lanes whose shadow ray meets the mesh
  unsigned long long occ[NL][S];
  unsigned nocc = 0u;
  const unsigned skipw = pinfo >> 24;
#pragma unroll
  for (int li = 0; li < NL; ++li) {
#pragma unroll
    for (int k = 0; k < S; ++k) occ[li][k] = 0ull;
    if (((skipw >> li) & 1u) != 0u || mob.root < 0) continue;
    p = params();
    const FLight L = at(p->lights, li);
    const F3 sd = f3(-L.v[0], -L.v[1], -L.v[2]);
    unsigned long long pm[S], anyp = 0ull;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      pm[k] = bal(mesh_gate(mob, slab_ray(ro[k], sd)));
      anyp |= pm[k];
    }
    if (anyp == 0ull) continue;
    F3 rd[S];
    float inf[S], best[S];  // limit and stop: +inf (the plane's t is negative)
#pragma unroll
    for (int k = 0; k < S; ++k) {
      rd[k] = sd;
      inf[k] = finf();
    }
    // (ground pixels count nothing in diagnostic builds)
    if (!light_cell_search<S>(params(), li, ro, rd, inf, inf, pm, best, nullptr)) return false;
#pragma unroll
    for (int k = 0; k < S; ++k) {  // found => 0 <= t < inf: the hit counts
      occ[li][k] = pm[k] & bal(__float_as_uint(best[k]) != __float_as_uint(finf()));
      nocc += pc(occ[li][k]);
    }
  }
  // the samples' colours in order: the plane's albedo / pi x E
  p = params();
  F3 E[S];
#pragma unroll
  for (int k = 0; k < S; ++k) E[k] = f3(0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int li = 0; li < NL; ++li) {
    const FLight L = at(p->lights, li);
    const float ndl = fmaxf(dot3(f3(0.0f, 1.0f, 0.0f), f3(-L.v[0], -L.v[1], -L.v[2])), 0.0f);
#pragma unroll
    for (int k = 0; k < S; ++k) irr_add(E[k], L.ci, lane_in(occ[li][k]) ? 0.0f : ndl);
  }
  const RT_CONST FObjX& px_ = at(p->objx, po);
  const F3 ap = f3(px_.albedo_pi[0], px_.albedo_pi[1], px_.albedo_pi[2]);
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const F3 a = mul3(ap, E[k]);
    acc_add3(acc, a.x, a.y, a.z);
  }
  wi.v[STAT_PRIMARY] += (unsigned)(64 * S);
  wi.v[STAT_SHADOW] += (unsigned)(NL * 64 * S);
  wi.v[STAT_HITS] += (unsigned)(64 * S) + nocc;
  return true;
}

}  // namespace fast
}  // namespace rtmi
