// rt_kernels_query.hip — ray queries (include/rtmi.h rt_trace_rays* /
// rt_pick_pixels*): trace (renderer.nim:47-67) for caller-supplied rays and
// for picks through the camera, in the float64 arithmetic of the parity
// render. Built with -ffp-contract=off like rt_kernels_f64.hip, so every
// operation rounds as the reference's (and the oracle's) does.
#include <rocprim/device/device_radix_sort.hpp>

#include "rt_device.h"
#include "rt_query.h"
#include "rt_query_rays.h"

namespace rtmi {

// ---- k_trace_rays -----------------------------------------------------------
// One ray per lane, 64 consecutive slots of the (sorted) batch per wave and
// step, grid-stride over the waves of a grid sized by the device. trace() is
// wave-coherent — ballots, readlane, the traversal stack's entry i in lane i
// — so EVERY lane of a wave reaches every trace call: slots past n and
// degenerate rays go in with active = false (holding a harmless ray), and no
// lane leaves the loop early (its bounds are wave-uniform).
__global__ __launch_bounds__(256) void k_trace_rays(const RenderParams<double> params_by_value, const QueryParams q) {
  using R = double;
  (void)params_by_value;  // read through rparams()
  const RT_CONST RenderParams<R>& p = rparams<R>();
  const int lane = (int)__lane_id();
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + wib;
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const long long nsteps = (q.n + 63) >> 6;
  const bool shadow = q.any_hit != 0;
  WaveStats ws;
#pragma unroll
  for (int k = 0; k < kStatSlots; ++k) ws.v[k] = 0u;
  unsigned long long tot = 0ull;

  for (long long b = wave; b < nsteps; b += nwaves) {
    const long long slot = (b << 6) + lane;
    const bool in = slot < q.n;
    const long long i = in ? (q.order ? (long long)q.order[slot] : slot) : 0;
    V3<R> o{R(0), R(0), R(0)}, d{R(0), R(0), R(1)};
    R tn_given = pinf<R>();
    bool ok = false;
    if (in) ok = query_ray(p, q, i, o, d, tn_given);
    if (!ok) {  // a masked lane computes along with the wave: give it finite operands
      o = V3<R>{R(0), R(0), R(0)};
      d = V3<R>{R(0), R(0), R(1)};
    }
    const R tn = ok ? tn_given : pinf<R>();
    ws.v[STAT_PRIMARY] += popc32(ballot(ok));
    const Hit<R> h = trace<R, false>(p, o, d, tn, ok, shadow, ws);
    const bool lit = ok && h.obj >= 0;
    if (q.normals) {
      // hitNormal (renderer.nim:83-88): rt_device.h hit_normal
      const V3<R> N = hit_normal(p, o, d, h, lit);
      if (in) {
        R* out = q.normals + 3 * i;
        out[0] = N.x; out[1] = N.y; out[2] = N.z;
      }
    }
    if (in) {
      QueryHit r;
      // any-hit: only hit / no hit is the answer (t and face are whatever
      // face the early exit stopped at): t echoes t_near
      r.t = (lit && !shadow) ? h.t : tn_given;
      r.obj = lit ? h.obj : -1;
      r.face = (lit && !shadow) ? h.tri : -1;
      q.hits[i] = r;
    }
    flush_stats(ws, tot, lane);
  }
  if (lane < kStatSlots) q.partials[wave * kStatSlots + lane] = tot;
}

// The per-wave counter rows summed per slot (one block).
__global__ __launch_bounds__(256) void k_query_reduce(const unsigned long long* partials, int rows,
                                                      unsigned long long* acc) {
  __shared__ unsigned long long part[16][16];
  const int slot = (int)threadIdx.x & 15, grp = (int)threadIdx.x >> 4;
  unsigned long long s = 0ull;
  if (slot < kStatSlots)
    for (int r = grp; r < rows; r += 16) s += partials[(size_t)r * kStatSlots + slot];
  part[grp][slot] = s;
  __syncthreads();
  if ((int)threadIdx.x < kStatSlots) {
    unsigned long long t = 0ull;
    for (int g = 0; g < 16; ++g) t += part[g][threadIdx.x];
    acc[threadIdx.x] = t;
  }
}

// ---- RT_QUERY_SORT ----------------------------------------------------------
// doubles as unsigned integers of the same order (for atomicMin / atomicMax)
__device__ __forceinline__ unsigned long long ord_enc(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ord_dec(unsigned long long e) {
  const unsigned long long b = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
  return __longlong_as_double((long long)b);
}

// What the key quantises: a ray's origin, a pick's image position (z = 0).
__device__ __forceinline__ bool sort_point(const QueryParams& q, long long i, V3<double>& pt, V3<double>& d) {
  if (q.xy) {
    pt = V3<double>{q.xy[2 * i], q.xy[2 * i + 1], 0.0};
    d = V3<double>{0.0, 0.0, 0.0};
    return __builtin_isfinite(pt.x) && __builtin_isfinite(pt.y);
  }
  if (q.xy32) {  // float picks (rt_pick_pixels_f32*): the pick's key, from the float positions
    pt = V3<double>{(double)q.xy32[2 * i], (double)q.xy32[2 * i + 1], 0.0};
    d = V3<double>{0.0, 0.0, 0.0};
    return __builtin_isfinite(pt.x) && __builtin_isfinite(pt.y);
  }
  if (q.orig32) {  // float rays (rt_shade_rays_f32*, rt_trace_rays_f32*): the same key, from the float values (widening is exact)
    pt = V3<double>{(double)q.orig32[3 * i], (double)q.orig32[3 * i + 1], (double)q.orig32[3 * i + 2]};
    d = V3<double>{(double)q.dir32[3 * i], (double)q.dir32[3 * i + 1], (double)q.dir32[3 * i + 2]};
    const float tn32 = q.tnear32 ? q.tnear32[i] : 0.0f;
    const bool zero32 = d.x == 0.0 && d.y == 0.0 && d.z == 0.0;
    return finite3(pt) && finite3(d) && !zero32 && !(tn32 != tn32);
  }
  pt = V3<double>{q.orig[3 * i], q.orig[3 * i + 1], q.orig[3 * i + 2]};
  d = V3<double>{q.dir[3 * i], q.dir[3 * i + 1], q.dir[3 * i + 2]};
  const double tn = q.tnear ? q.tnear[i] : 0.0;
  const bool zero = d.x == 0.0 && d.y == 0.0 && d.z == 0.0;
  return finite3(pt) && finite3(d) && !zero && !(tn != tn);
}

__global__ __launch_bounds__(256) void k_query_bounds_init(unsigned long long* bounds) {
  if (threadIdx.x < 12) bounds[threadIdx.x] = threadIdx.x < 6 ? ~0ull : 0ull;
}

// bounds[0..2] / [6..8]: min / max of the points; [3..5] / [9..11]: unused
__global__ __launch_bounds__(256) void k_query_bounds(const QueryParams q, unsigned long long* bounds) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const double inf = __builtin_huge_val();
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < q.n; i += stride) {
    V3<double> pt, d;
    if (!sort_point(q, i, pt, d)) continue;
    lo[0] = fmin(lo[0], pt.x); lo[1] = fmin(lo[1], pt.y); lo[2] = fmin(lo[2], pt.z);
    hi[0] = fmax(hi[0], pt.x); hi[1] = fmax(hi[1], pt.y); hi[2] = fmax(hi[2], pt.z);
  }
  for (int k = 0; k < 3; ++k) {
    for (int off = 1; off < 64; off <<= 1) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], off));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], off));
    }
    if (__lane_id() == 0) {
      if (lo[k] <= hi[k]) {
        atomicMin(&bounds[k], ord_enc(lo[k]));
        atomicMax(&bounds[6 + k], ord_enc(hi[k]));
      }
    }
  }
}

__device__ __forceinline__ uint32_t spread3(uint32_t v) {  // 10 bits -> every third bit
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__device__ __forceinline__ uint32_t spread2(uint32_t v) {  // 15 bits -> every second bit
  v &= 0x7fffu;
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}
// x in [lo, hi] -> [0, levels - 1] (0 when the interval is a point)
__device__ __forceinline__ uint32_t quant(double x, double lo, double hi, int levels) {
  const double w = hi - lo;
  if (!(w > 0.0) || !__builtin_isfinite(w)) return 0u;
  double f = (x - lo) / w * (double)levels;
  f = fmin(fmax(f, 0.0), (double)(levels - 1));
  return (uint32_t)f;
}

// The 32-bit coherence key: rays — the direction's sign octant in bits 27-29,
// below it the 27-bit Morton code of the origin in the batch's origin bounds,
// or of the direction (scaled to its largest component) when every ray
// shares one origin; picks — the 30-bit Morton code of the image position.
// Degenerate rays get the largest key: they sort last.
__global__ __launch_bounds__(256) void k_query_keys(const QueryParams q, const unsigned long long* bounds,
                                                    uint32_t* key, uint32_t* idx) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const double lo[3] = {ord_dec(bounds[0]), ord_dec(bounds[1]), ord_dec(bounds[2])};
  const double hi[3] = {ord_dec(bounds[6]), ord_dec(bounds[7]), ord_dec(bounds[8])};
  const bool one_origin = lo[0] == hi[0] && lo[1] == hi[1] && lo[2] == hi[2];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < q.n; i += stride) {
    V3<double> pt, d;
    uint32_t k = 0xffffffffu;
    if (sort_point(q, i, pt, d)) {
      if (q.xy || q.xy32) {
        k = spread2(quant(pt.x, lo[0], hi[0], 1 << 15)) | (spread2(quant(pt.y, lo[1], hi[1], 1 << 15)) << 1);
      } else {
        const uint32_t oct = (d.x < 0.0 ? 1u : 0u) | (d.y < 0.0 ? 2u : 0u) | (d.z < 0.0 ? 4u : 0u);
        uint32_t m;
        if (one_origin) {
          const double s = fmax(fmax(fabs(d.x), fabs(d.y)), fabs(d.z));
          m = spread3(quant(d.x / s, -1.0, 1.0, 512)) | (spread3(quant(d.y / s, -1.0, 1.0, 512)) << 1) |
              (spread3(quant(d.z / s, -1.0, 1.0, 512)) << 2);
        } else {
          m = spread3(quant(pt.x, lo[0], hi[0], 512)) | (spread3(quant(pt.y, lo[1], hi[1], 512)) << 1) |
              (spread3(quant(pt.z, lo[2], hi[2], 512)) << 2);
        }
        k = (oct << 27) | (m & 0x07ffffffu);
      }
    }
    key[i] = k;
    idx[i] = (uint32_t)i;
  }
}

}  // namespace rtmi

extern "C" int rtmi_query_blocks_per_cu() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)rtmi::k_trace_rays, 256, 0) != hipSuccess) return 0;
  return n;
}

extern "C" int rtmi_launch_query(const rtmi::RenderParams<double>* p, const rtmi::QueryParams* q, int blocks,
                                 void* stream) {
  hipLaunchKernelGGL(rtmi::k_trace_rays, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, *q);
  return (int)hipGetLastError();
}

extern "C" int rtmi_launch_query_reduce(const unsigned long long* partials, int rows, unsigned long long* acc,
                                        void* stream) {
  hipLaunchKernelGGL(rtmi::k_query_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, rows, acc);
  return (int)hipGetLastError();
}

namespace {
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
}

extern "C" size_t rtmi_query_sort_bytes(long long n) {
  if (n <= 0 || n > 0x7fffffffLL) return 0;
  size_t tmp = 0;
  uint32_t* z = nullptr;
  if (rocprim::radix_sort_pairs(nullptr, tmp, z, z, z, z, (size_t)n, 0, 32, (hipStream_t) nullptr) != hipSuccess)
    return 0;
  return 4 * align256((size_t)n * sizeof(uint32_t)) + align256(12 * sizeof(unsigned long long)) + align256(tmp);
}

extern "C" void rtmi_query_sort_carve(void* base, long long n, rtmi::QuerySortBufs* out) {
  unsigned char* b = (unsigned char*)base;
  const size_t a = align256((size_t)n * sizeof(uint32_t));
  out->key = (uint32_t*)b;
  out->key2 = (uint32_t*)(b + a);
  out->idx = (uint32_t*)(b + 2 * a);
  out->idx2 = (uint32_t*)(b + 3 * a);
  out->bounds = (unsigned long long*)(b + 4 * a);
  out->tmp = b + 4 * a + align256(12 * sizeof(unsigned long long));
  size_t tmp = 0;
  uint32_t* z = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, tmp, z, z, z, z, (size_t)n, 0, 32, (hipStream_t) nullptr);
  out->tmp_bytes = tmp;
}

extern "C" int rtmi_query_sort(const rtmi::QueryParams* q, const rtmi::QuerySortBufs* b, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)std::min<long long>((q->n + 255) / 256, 2048);
  hipLaunchKernelGGL(rtmi::k_query_bounds_init, dim3(1), dim3(256), 0, st, b->bounds);
  hipLaunchKernelGGL(rtmi::k_query_bounds, dim3(blocks), dim3(256), 0, st, *q, b->bounds);
  hipLaunchKernelGGL(rtmi::k_query_keys, dim3(blocks), dim3(256), 0, st, *q, b->bounds, b->key, b->idx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  size_t tmp = b->tmp_bytes;
  e = rocprim::radix_sort_pairs(b->tmp, tmp, b->key, b->key2, b->idx, b->idx2, (size_t)q->n, 0, 32, st);
  return (int)e;
}
