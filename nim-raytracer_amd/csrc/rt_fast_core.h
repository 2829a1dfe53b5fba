// rt_fast_core.h — the float32 kernels' ground layer (rt_fast.h has the map):
// feature bits, intrinsic wrappers, the kernel-argument pointer, small types,
// the analytic intersectors, face-record loads and tests, LDS slot helpers,
// wave reductions and the Stats plumbing every kernel shares.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_common.h"
#include "rt_sampling.h"

#ifndef RT_CONST
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_CONST __attribute__((address_space(4)))  // scalar (constant) loads
#else
#define RT_CONST
#endif
#endif

namespace rtmi {
namespace fast {

// Scene-feature mask of a kernel instantiation: code for a feature whose bit
// is clear is removed at compile time (the host picks the smallest
// instantiation covering the scene, rtmi.cpp feature_mask()).
enum : unsigned {
  F_SPHERE = 1u, F_BOX = 2u, F_PLANE = 4u, F_MESH = 8u,
  F_XF_GENERAL = 16u,  // rotations / scales (identity and translation always)
  F_POINT = 32u,       // point lights
  F_REFLECT = 64u,     // reflective materials
  F_STOCHASTIC = 128u, // jittered / (correlated) multi-jittered sampling
  F_ALL = 255u
};

template <class T>
__device__ __forceinline__ const RT_CONST T* cp(const T* p) {
  return (const RT_CONST T*)(p);
}

// Record i of a small scene array (objects, lights: < 2^25 records) at a
// 32-bit byte offset: s_load with an SGPR offset, one shift instead of the
// 64-bit address arithmetic per object / light visit.
template <class T>
__device__ __forceinline__ const RT_CONST T& at(const T* base, int i) {
  return *(const RT_CONST T*)((const RT_CONST char*)base + (unsigned)i * (unsigned)sizeof(T));
}

// Work items of a two-class launch's list: its entry count as this call's
// k_frame_records counted it on the device (n, rt_frame.h; per_item entries
// per item), or the host's item count when the list is not counted.
__device__ __forceinline__ int list_items(const int32_t* n, int host_items, int per_item) {
  return n ? (cp(n)[0] + per_item - 1) / per_item : host_items;
}

__device__ __forceinline__ unsigned long long bal(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// Lane masks straight from a v_cmp (llvm.amdgcn.fcmp: ordered >= / <) and a
// mask back to a per-lane predicate (llvm.amdgcn.inverse.ballot): a ballot of
// a compound bool otherwise materialises it in a VGPR (v_cndmask 0/1 +
// v_cmp_ne) before the popcount.
__device__ __forceinline__ unsigned long long m_ge(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 3); }
__device__ __forceinline__ unsigned long long m_lt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, 4); }
__device__ __forceinline__ bool lane_in(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ unsigned int pc(unsigned long long m) { return (unsigned int)__builtin_popcountll(m); }
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float finf() { return __builtin_huge_valf(); }

// Kernel parameters are read through this pointer into the kernarg segment,
// re-laundered (opaque to the optimizer) once per pixel group, sample and
// light: each field is then re-read with a scalar load near its use instead
// of being hoisted to the kernel entry and pinned in SGPRs for the whole
// kernel (which spilled ~100 SGPRs into VGPR lanes and cost a v_readlane per
// use). Inside traverse() the pointer is invariant, so the node / triangle
// base addresses stay hoisted off the fetch chain.
using KP = const RT_CONST FastParams*;
__device__ __forceinline__ KP params() {
  KP q = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(q));
  return q;
}

struct F3 {
  float x, y, z;
};

template <bool B>
struct Bool {
  static constexpr bool value = B;
};
__device__ __forceinline__ F3 f3(float x, float y, float z) { return F3{x, y, z}; }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return __builtin_fmaf(a.x, b.x, __builtin_fmaf(a.y, b.y, a.z * b.z)); }

struct Stats32 {
  unsigned int v[kStatSlots];
};

#ifdef RTMI_STAMPS
// Diagnostic build only (never the measured kernel): shader-clock stamps
// accumulated into the traversal counter slots 5..8.
__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define RT_STAMP(var) const unsigned long long var = stamp()
#define RT_ACC(slot, a, b) ws.v[slot] += (unsigned int)((b) - (a))
#else
#define RT_STAMP(var)
#define RT_ACC(slot, a, b)
#endif

struct Hit {
  int obj;
  int tri;
  float t;
};

// World -> object space (FObj.xf classification).
template <unsigned F>
__device__ __forceinline__ void to_object(KP p, const FObj& ob, int i, F3 o, F3 d, F3& ro,
                                          F3& rd) {
  // identity and translation alike: the identity's translation is 0 (three
  // adds instead of a scalar compare + selects per object visit)
  if (!(F & F_XF_GENERAL) || ob.xf != XF_GENERAL) {
    ro = f3(o.x + ob.t[0], o.y + ob.t[1], o.z + ob.t[2]);
    rd = d;
  } else {
    const RT_CONST FObjX& x = at(p->objx, i);
    const float* m = x.w2o;  // m[c*3 + r], c = 0..3
    ro = f3(__builtin_fmaf(m[0], o.x, __builtin_fmaf(m[3], o.y, __builtin_fmaf(m[6], o.z, m[9]))),
            __builtin_fmaf(m[1], o.x, __builtin_fmaf(m[4], o.y, __builtin_fmaf(m[7], o.z, m[10]))),
            __builtin_fmaf(m[2], o.x, __builtin_fmaf(m[5], o.y, __builtin_fmaf(m[8], o.z, m[11]))));
    rd = f3(__builtin_fmaf(m[0], d.x, __builtin_fmaf(m[3], d.y, m[6] * d.z)),
            __builtin_fmaf(m[1], d.x, __builtin_fmaf(m[4], d.y, m[7] * d.z)),
            __builtin_fmaf(m[2], d.x, __builtin_fmaf(m[5], d.y, m[8] * d.z)));
  }
}

// AABB.intersect (geom.nim:76-96) in IEEE min/max form; -inf = miss.
__device__ __forceinline__ float aabb(const float* lo, const float* hi, F3 o, F3 inv) {
  const float ax = (lo[0] - o.x) * inv.x, bx = (hi[0] - o.x) * inv.x;
  const float ay = (lo[1] - o.y) * inv.y, by = (hi[1] - o.y) * inv.y;
  const float az = (lo[2] - o.z) * inv.z, bz = (hi[2] - o.z) * inv.z;
  const float tmin = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  const float tmax = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * 1.00000024f;
  return tmin <= tmax ? tmin : -finf();
}

// Sphere.intersect (geom.nim:215-237) incl. the `/ 2*a` precedence.
__device__ __forceinline__ float sphere(float radius, F3 o, F3 d) {
  const float a = dot3(d, d);
  const float b = 2.0f * dot3(d, o);
  const float c = dot3(o, o) - radius * radius;
  const float delta = b * b - 4.0f * a * c;
  const float sb = b > 0.0f ? 1.0f : (b < 0.0f ? -1.0f : 0.0f);
  const float t1 = ((-b - sb * fsqrt(delta)) * 0.5f) * a;
  const float t2 = c * rcp(a * t1);
  const float t = t1 <= t2 ? t1 : t2;
  return delta >= 0.0f ? t : -finf();
}

// Plane.intersect (geom.nim:240-248): y = 0.
__device__ __forceinline__ float plane(F3 o, F3 d) {
  return fabsf(d.y) > 1e-6f ? -o.y * rcp(d.y) : -finf();
}

// A TriFast record as ONE s_load_dwordx16 (the compiler otherwise splits the
// record into per-field loads — up to eight SMEM instructions per face in
// the batched list searches — since a face test reads 13 of its 16 dwords):
// the pad dwords are marked live so the load stays whole.
struct TriRegs {
  float v0[3], e2[3], e1n[3], nn[3];
  unsigned int id;
};
__device__ __forceinline__ TriRegs load_tri(const RT_CONST TriFast* t) {
  using V16 = unsigned int __attribute__((ext_vector_type(16)));
  const V16 r = *(const RT_CONST V16*)t;
  asm volatile("" ::"s"(r[7]), "s"(r[11]), "s"(r[15]));
  TriRegs T;
  T.v0[0] = __uint_as_float(r[0]), T.v0[1] = __uint_as_float(r[1]), T.v0[2] = __uint_as_float(r[2]);
  T.id = r[3];
  T.e2[0] = __uint_as_float(r[4]), T.e2[1] = __uint_as_float(r[5]), T.e2[2] = __uint_as_float(r[6]);
  T.e1n[0] = __uint_as_float(r[8]), T.e1n[1] = __uint_as_float(r[9]), T.e1n[2] = __uint_as_float(r[10]);
  T.nn[0] = __uint_as_float(r[12]), T.nn[1] = __uint_as_float(r[13]), T.nn[2] = __uint_as_float(r[14]);
  return T;
}

// Closest hit as ONE 64-bit key: float bits of t in the high word, the
// triangle's face index in the low word. For t >= 0 the float bits order like
// unsigned integers, so key order is the reference's "smaller t, then lower
// face index" order (geom.nim:339-358 keeps the first, i.e. lowest-index,
// face on a tie); a negative or NaN t sorts above +inf and is never accepted.
// One v_cmp_lt_u64 + three v_cndmask replace the compare/tie-break mask
// algebra (which cost SALU s_and/s_or per triangle).
__device__ __forceinline__ unsigned long long tkey(float t, unsigned int lo) {
  return ((unsigned long long)__float_as_uint(t) << 32) | lo;
}

// rayTriangleIntersectFast (geom.nim:283-336), single-sided, on the TriFast
// record (rt_common.h): with c = (o - v0) x d and nn = -(e1 x e2),
//   det = d.nn, u*det = e2.c, v*det = (-e1).c, t = (o - v0).nn / (-det)
// (scalar triple-product identities of the reference's p = d x e2,
// q = tvec x e1 form). The barycentric range is tested unscaled in one min:
// u >= 0, v >= 0, u + v <= 1 (u <= 1 is implied), det >= 1e-6.
template <class TR>
__device__ __forceinline__ void tri_test(const TR& T, F3 o, F3 d, unsigned long long& key, float& tc) {
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
  const unsigned long long k = tkey(ts, (unsigned int)T.id);
  const bool acc = k < key;
  key = acc ? k : key;
  tc = acc ? ts : tc;
}

// Shadow-ray tests on a face's LTri record for the ray's distant light
// (rt_common.h): u, v, t are affine in the ray origin, so a test is 9 FMAs
// and the barycentric range in one min (u >= 0, v >= 0, u + v <= 1; the
// det >= 1e-6 cull is folded into the record). Every float32 path tests a
// shadow ray to a light with records this way (list searches, BVH leaves,
// batched and one-sample loops), so they all form the same t bit for bit.
struct LRegs {
  float p[3], cu, q[3], cv, tv[3], ct;
  unsigned int id;
};
__device__ __forceinline__ LRegs load_ltri(const RT_CONST LTri* t) {
  using V16 = unsigned int __attribute__((ext_vector_type(16)));
  const V16 r = *(const RT_CONST V16*)t;
  asm volatile("" ::"s"(r[13]), "s"(r[14]), "s"(r[15]));
  LRegs L;
  L.p[0] = __uint_as_float(r[0]), L.p[1] = __uint_as_float(r[1]), L.p[2] = __uint_as_float(r[2]);
  L.cu = __uint_as_float(r[3]);
  L.q[0] = __uint_as_float(r[4]), L.q[1] = __uint_as_float(r[5]), L.q[2] = __uint_as_float(r[6]);
  L.cv = __uint_as_float(r[7]);
  L.tv[0] = __uint_as_float(r[8]), L.tv[1] = __uint_as_float(r[9]), L.tv[2] = __uint_as_float(r[10]);
  L.ct = __uint_as_float(r[11]);
  L.id = r[12];
  return L;
}
// t of the hit, or -1 (no hit: outside the face, or det culled)
template <class LR>
__device__ __forceinline__ float ltri_t(const LR& L, F3 o) {
  const float u = __builtin_fmaf(L.p[0], o.x, __builtin_fmaf(L.p[1], o.y, __builtin_fmaf(L.p[2], o.z, L.cu)));
  const float v = __builtin_fmaf(L.q[0], o.x, __builtin_fmaf(L.q[1], o.y, __builtin_fmaf(L.q[2], o.z, L.cv)));
  const float t = __builtin_fmaf(L.tv[0], o.x, __builtin_fmaf(L.tv[1], o.y, __builtin_fmaf(L.tv[2], o.z, L.ct)));
  const float g = fminf(fminf(u, v), 1.0f - (u + v));
  return g >= 0.0f ? t : -1.0f;
}
template <class LR>
__device__ __forceinline__ void ltri_test(const LR& L, F3 o, unsigned long long& key, float& tc) {
  const float ts = ltri_t(L, o);
  const unsigned long long k = tkey(ts, (unsigned int)L.id);
  const bool acc = k < key;
  key = acc ? k : key;
  tc = acc ? ts : tc;
}
// the records of shadow rays to distant light `light` (byte offsets are the
// faces' TriFast offsets), or nullptr when the light has none
__device__ __forceinline__ const char* lrec_of(KP p, int light) {
  if (light < 0 || light >= 32 || !((p->lrec_mask >> light) & 1u)) return nullptr;
  return (const char*)(p->lrec_base + (uint64_t)light * (uint64_t)p->lrec_stride);
}

// The cell-ordered records of a light's grid, aligned with its entries
// (p->grid_ent + G.ent_base): list_search_batch's lb.
__device__ __forceinline__ const char* grid_rec_of(KP p, int light, const LightGrid& G) {
  return (const char*)(p->grid_rec + G.ent_base);
}

// A record of the float32 tree (FastParams.tree) at a byte offset: one scalar
// base + a 32-bit SGPR offset (s_load ... soffset), no 64-bit address
// arithmetic on the traversal's dependent chain.
template <class T>
__device__ __forceinline__ const RT_CONST T* rec(KP p, int off) {
  return (const RT_CONST T*)((const RT_CONST char*)p->tree + (unsigned)off);
}

// Per-lane LDS scratch of the shading loop, laid out [slot][lane] so a
// wave's access to one slot touches 64 consecutive dwords (no bank
// conflicts). Parking the reflected ray and the hit point here instead of in
// VGPRs takes them out of the register peak, which sits inside the
// shadow-ray traversal (DESIGN.md "Occupancy").
enum : int { LDS_RO = 0, LDS_RD = 3, LDS_HW = 6, LDS_ALB = 9, kLdsSlots = 12, LDS_SRC = 12 };
// LDS_SRC (reflective kernels only: one slot more): the plane a parked
// reflected ray left, -1 when it left another kind of object (trace's `src`).
template <unsigned F>
constexpr int lds_slots() {
  return (F & F_REFLECT) ? kLdsSlots + 1 : kLdsSlots;
}
// An LDS-typed pointer: 32-bit addresses with the slot offsets folded into
// the ds_* immediates (a generic float* here became a 64-bit flat address
// per slot, hoisted and pinned in VGPRs).
#if defined(__HIP_DEVICE_COMPILE__)
using LdsF = __attribute__((address_space(3))) float;
#else
using LdsF = float;
#endif

// Radiance accumulator of the lane's current pixel samples. Kept in VGPRs:
// LDS float atomics (ds_add_f32) measured ~50 % slower on C3 and a plain
// LDS read-modify-write no faster than the three registers.
struct Acc {
  F3 v;
};
__device__ __forceinline__ void acc_add3(Acc& a, float x, float y, float z) {
  a.v = f3(a.v.x + x, a.v.y + y, a.v.z + z);
}
// A shading level's radiance, in the reference's grouping (shade() sums the
// lights' shadeDiffuse terms, renderer.nim:93-104, and calcPixel adds each
// sample's colour, renderer.nim:149-157): per light E += ci * ndl (one FMA
// per channel), then the level adds albedo/pi * weight * E — rounded the same
// way by every instance of the sample loop (no contraction choices left to
// the compiler), so the batched lean samples below and the one-sample loop
// give bit-identical pixels.
__device__ __forceinline__ void irr_add(F3& e, const float* ci, float ndl) {
  e = f3(__builtin_fmaf(ci[0], ndl, e.x), __builtin_fmaf(ci[1], ndl, e.y), __builtin_fmaf(ci[2], ndl, e.z));
}
// A product the compiler may not fuse into a later add (-ffp-contract=fast
// contracts HIP's __fmul_rn, a plain `*`, wherever the add happens to be
// visible): the empty asm makes the product opaque, at no instruction cost.
__device__ __forceinline__ float mul_nc(float a, float b) {
  float r = a * b;
  asm("" : "+v"(r));
  return r;
}
__device__ __forceinline__ F3 mul3(F3 a, F3 b) { return f3(mul_nc(a.x, b.x), mul_nc(a.y, b.y), mul_nc(a.z, b.z)); }
// volatile: the value must really leave the registers (no store-to-load
// forwarding across the light loop)
__device__ __forceinline__ void lds_put3(LdsF* ls, int slot, F3 v) {
  volatile LdsF* q = ls;
  q[(slot + 0) * 64] = v.x;
  q[(slot + 1) * 64] = v.y;
  q[(slot + 2) * 64] = v.z;
}
__device__ __forceinline__ F3 lds_get3(LdsF* ls, int slot) {
  volatile LdsF* q = ls;
  return f3(q[(slot + 0) * 64], q[(slot + 1) * 64], q[(slot + 2) * 64]);
}
__device__ __forceinline__ void lds_put1(LdsF* ls, int slot, float v) {
  volatile LdsF* q = ls;
  q[slot * 64] = v;
}
__device__ __forceinline__ float lds_get1(LdsF* ls, int slot) {
  volatile LdsF* q = ls;
  return q[slot * 64];
}

// The lane id from an opaque instruction: values derived from it are
// recomputed inside the loops instead of hoisted to kernel scope, where
// they would stay live (and spill) across the whole sample loop.
__device__ __forceinline__ int lane_id_fresh() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// q = n / dv, r = n - q*dv for 0 <= n < 2^21 and dv >= 1 via the float
// reciprocal (exact: the quotient's fractional part keeps >= 0.5/dv from an
// integer, far above the fp32 product's error); no integer-division sequence.
__device__ __forceinline__ int div_small(int n, int dv, float inv_dv, int& r) {
  const int q = (int)(((float)n + 0.5f) * inv_dv);
  r = n - q * dv;
  return q;
}

// A pixel group's placement: tile (tx x ty pixels, L lanes each, powers of
// two) -> this lane's pixel (x, y), output row and validity.
struct GroupPix {
  int x, y, out_row, sub;
  bool valid;
};

// Sum of a per-lane count over the wave (DPP row sums, then the rows).
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
  v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false);  // row_shr:8 -> lane 15 of each row: its row's sum
  return (unsigned)__builtin_amdgcn_readlane((int)v, 15) + (unsigned)__builtin_amdgcn_readlane((int)v, 31) +
         (unsigned)__builtin_amdgcn_readlane((int)v, 47) + (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// Sum of a float over the wave, in lane 63's order-independent-of-data
// sequence (DPP row_shr scans, then row_bcast:15 / :31), returned uniform.
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xf, false));
}
// OR of a 32-bit value over the wave (the DPP tree of wave_total; lanes a
// row shift or broadcast does not reach contribute 0, the identity)
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned dpp_or(unsigned v) {
  return v | (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}
__device__ __forceinline__ unsigned wave_or(unsigned v) {
  v = dpp_or<0x111, 0xf>(v);
  v = dpp_or<0x112, 0xf>(v);
  v = dpp_or<0x114, 0xf>(v);
  v = dpp_or<0x118, 0xf>(v);
  v = dpp_or<0x142, 0xa>(v);
  v = dpp_or<0x143, 0xc>(v);
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ float wave_total(float v) {
  v = dpp_add<0x111, 0xf>(v);  // row_shr:1
  v = dpp_add<0x112, 0xf>(v);  // row_shr:2
  v = dpp_add<0x114, 0xf>(v);  // row_shr:4
  v = dpp_add<0x118, 0xf>(v);  // row_shr:8: lane 15 of each row holds its row's sum
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3: lane 63 holds the total
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// The wave's 32-bit Stats counters into its 64-bit LDS totals (lane k adds
// slot k), then cleared.
__device__ __forceinline__ void flush_stats(Stats32& ws, unsigned long long* tot, int lane) {
  unsigned int v = 0u;
#pragma unroll
  for (int k = 0; k < kStatSlots; ++k) v = lane == k ? ws.v[k] : v;
  if (lane < kStatSlots) tot[lane] += v;
#pragma unroll
  for (int k = 0; k < kStatSlots; ++k) ws.v[k] = 0u;
}

// Every render kernel's Stats prologue and epilogue. lds_tot: the block's
// per-wave 64-bit totals (__shared__ [4][kStatSlots], 256-thread blocks); ws:
// the wave's 32-bit counters, flushed into them every p->stat_flush items
// (before any can wrap) and at the end. Each kernel forms wib, the wave's
// index in its block, and the lane id in its own way, which matters to
// spills: k_render_gen1 / k_render_mix1 pass a readfirstlane scalar (from
// threadIdx.x, wib stayed a VGPR live across the whole item loop and spilled,
// as did the LDS address of lds_tot[wib]); the others' register allocation is
// settled with threadIdx.x >> 6. The prologue is a macro for the same reason:
// through a function's reference parameter the compiler stops sharing the LDS
// address with the epilogue's, and the VGPR / spill counts of 47 lean, wave
// and gen kernels move (rt_occupancy.h and the launch sizing rest on them).
#define RT_STATS_BEGIN(lds_tot, wib, lane, ws)                \
  do {                                                        \
    if ((lane) < kStatSlots) (lds_tot)[wib][lane] = 0ull;     \
    _Pragma("unroll") for (int k_ = 0; k_ < kStatSlots; ++k_)(ws).v[k_] = 0u; \
  } while (0)
// the last flush, then the wave's totals into its row of p->partials
// (k_reduce_stats sums the rows)
__device__ __forceinline__ void stats_end(KP p, Stats32& ws, unsigned long long (&lds_tot)[4][kStatSlots], int wib) {
  const int lane = (int)__lane_id();
  flush_stats(ws, lds_tot[wib], lane);
  const int wave = (int)(blockIdx.x * (blockDim.x >> 6)) + wib;
  if (lane < kStatSlots) p->partials[(size_t)wave * kStatSlots + lane] = lds_tot[wib][lane];
}

}  // namespace fast
}  // namespace rtmi
