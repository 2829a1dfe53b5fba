// rt_mesh_gpu.hip — the device passes of rt_scene_set_mesh_vertices (see
// rt_mesh_gpu.h): a mesh whose vertices changed keeps its faces, its tree's
// topology and its leaf order; bounds, normals, node boxes and binned faces
// are formed again on the device with the operations the host create path
// uses (-ffp-contract=off), so the results are the same bytes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "rt_mesh_gpu.h"

namespace rtmi {
namespace {

constexpr int kBlock = 256;

unsigned grid(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

__device__ __forceinline__ unsigned long long ord_bits(double x) {  // monotone double -> u64
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double unord_bits(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  memcpy(&x, &b, sizeof x);
  return x;
}

// scratch words (kMeshBoundsWords)
enum { W_FLO = 0, W_FHI = 3, W_BAD = 6, W_ALO = 8, W_AHI = 11, W_IDX = 16, W_OUT = 24 };

// min of keys [0, 3), max of keys [3, 6) over the block, then one atomic each
__device__ __forceinline__ void reduce6(const unsigned long long k[6], unsigned long long* out) {
  __shared__ unsigned long long s[6][kBlock];
  for (int a = 0; a < 6; ++a) s[a][threadIdx.x] = k[a];
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int a = 0; a < 3; ++a) {
        s[a][threadIdx.x] = min(s[a][threadIdx.x], s[a][threadIdx.x + w]);
        s[3 + a][threadIdx.x] = max(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + w]);
      }
    __syncthreads();
  }
  if (threadIdx.x == 0)
    for (int a = 0; a < 3; ++a) {
      atomicMin(&out[a], s[a][0]);
      atomicMax(&out[3 + a], s[3 + a][0]);
    }
}

// the bounds of the vertices the faces reference (the BVH margin, rt_bvh.cpp
// build_bvh) and whether any of their coordinates is not finite
__global__ __launch_bounds__(kBlock) void k_face_bounds(const double* v, const int32_t* f, long long nf,
                                                         unsigned long long* w) {
  unsigned long long k[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
  bool bad = false;
  for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < nf; t += (long long)gridDim.x * kBlock)
    for (int c = 0; c < 3; ++c) {
      const double* p = v + 3 * (size_t)f[3 * t + c];
      for (int a = 0; a < 3; ++a) {
        const double x = p[a];
        if (!(fabs(x) <= 1.7976931348623157e308)) {  // NaN or infinite
          bad = true;
          continue;
        }
        const unsigned long long kb = ord_bits(x);
        k[a] = min(k[a], kb);
        k[3 + a] = max(k[3 + a], kb);
      }
    }
  if (bad) atomicOr(&w[W_BAD], 1ull);
  reduce6(k, w + W_FLO);
}

// calcAABB, pass 1: the bounds as numbers over every vertex. A NaN is skipped
// as the host's `x < lo` / `x > hi` skip it, an infinity is taken; zeros are
// keyed as +0 (x + 0.0), their sign is pass 2's.
__global__ __launch_bounds__(kBlock) void k_all_bounds(const double* v, long long nv, unsigned long long* w) {
  unsigned long long k[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
  for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < nv; t += (long long)gridDim.x * kBlock)
    for (int a = 0; a < 3; ++a) {
      const double x = v[3 * t + a];
      if (!(x == x)) continue;
      const unsigned long long kb = ord_bits(x + 0.0);
      k[a] = min(k[a], kb);
      k[3 + a] = max(k[3 + a], kb);
    }
  reduce6(k, w + W_ALO);
}

// pass 2: the lowest vertex index that attains each bound (the host loop
// keeps the first one: -0.0 < +0.0 is false)
__global__ __launch_bounds__(kBlock) void k_all_first(const double* v, long long nv, unsigned long long* w) {
  double b[6];
  for (int a = 0; a < 6; ++a) b[a] = unord_bits(w[W_ALO + a]);
  for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < nv; t += (long long)gridDim.x * kBlock)
    for (int a = 0; a < 3; ++a) {
      const double x = v[3 * t + a];
      if (x == b[a]) atomicMin(&w[W_IDX + a], (unsigned long long)t);
      if (x == b[3 + a]) atomicMin(&w[W_IDX + 3 + a], (unsigned long long)t);
    }
}

// pass 3: those vertices' coordinates, bit for bit (no vertex: the host's start values)
__global__ void k_all_gather(const double* v, unsigned long long* w) {
  const int a = (int)threadIdx.x;
  if (a >= 6) return;
  const unsigned long long i = w[W_IDX + a];
  const double x = i == ~0ull ? (a < 3 ? INFINITY : -INFINITY) : v[3 * i + (a % 3)];
  w[W_OUT + a] = (unsigned long long)__double_as_longlong(x);
}

// calcNormals (the host loop of rt_scene_create), one face per thread
__global__ __launch_bounds__(kBlock) void k_normals(const double* v, const int32_t* f, const double* given,
                                                     long long nf, double* n64, float* n32) {
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= nf) return;
  double n[3];
  if (given) {
    for (int k = 0; k < 3; ++k) n[k] = given[3 * t + k];
  } else {
    const double* p0 = v + 3 * (size_t)f[3 * t + 0];
    const double* p1 = v + 3 * (size_t)f[3 * t + 1];
    const double* p2 = v + 3 * (size_t)f[3 * t + 2];
    const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    double dd = 0.0;
    dd = dd + cx * cx;
    dd = dd + cy * cy;
    dd = dd + cz * cz;
    const double len = sqrt(dd);
    n[0] = cx / len;
    n[1] = cy / len;
    n[2] = cz / len;
  }
  for (int k = 0; k < 3; ++k) {
    n64[3 * t + k] = n[k];
    n32[3 * t + k] = (float)n[k];
  }
}

__device__ __forceinline__ float load_agent(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void put_box(BvhNode* nodes, int32_t node, int slot, const float lo[3], const float hi[3]) {
  float* l = slot == 0 ? nodes[node].lo0 : nodes[node].lo1;
  float* h = slot == 0 ? nodes[node].hi0 : nodes[node].hi1;
  for (int a = 0; a < 3; ++a) {
    l[a] = lo[a];
    h[a] = hi[a];
  }
}

// One thread per node: its leaf children's boxes from their faces (k_leaves'
// rounding), then up the tree. A node is complete when its own thread and
// its inner children have arrived; the LAST arrival forms the node's box and
// carries it to the parent's slot, every other arrival ends — no thread waits
// for another (rt_bvh_gpu.hip k_collapse).
__global__ __launch_bounds__(kBlock) void k_refit(const double* v, const int32_t* f, const int32_t* order,
                                                   double inflate, int32_t node0, int32_t nnode, long long tri_base,
                                                   const int32_t* parent, int32_t* arrivals, BvhNode* n64,
                                                   BvhNode* n32) {
  const int32_t t = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (t >= nnode) return;
  int32_t node = node0 + t;
  {
    const int32_t cs[2] = {n64[node].c0, n64[node].c1}, ns[2] = {n64[node].n0, n64[node].n1};
    for (int slot = 0; slot < 2; ++slot) {
      if (ns[slot] <= 0) continue;
      double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (int32_t j = 0; j < ns[slot]; ++j) {
        const int32_t* fi = f + 3 * (size_t)order[(long long)cs[slot] - tri_base + j];
        for (int c = 0; c < 3; ++c) {
          const double* p = v + 3 * (size_t)fi[c];
          for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], p[a]);
            hi[a] = fmax(hi[a], p[a]);
          }
        }
      }
      float l32[3], h32[3];
      for (int a = 0; a < 3; ++a) {
        l32[a] = __double2float_rd(lo[a] - inflate);
        h32[a] = __double2float_ru(hi[a] + inflate);
      }
      put_box(n64, node, slot, l32, h32);
      put_box(n32, node, slot, l32, h32);
    }
  }
  for (;;) {
    const int32_t want = 1 + (n64[node].n0 == 0 && n64[node].c0 >= 0 ? 1 : 0) +
                         (n64[node].n1 == 0 && n64[node].c1 >= 0 ? 1 : 0);
    __threadfence();
    if (atomicAdd(&arrivals[node - node0], 1) + 1 != want) return;
    __threadfence();
    const int32_t p = parent[node];
    if (p < 0) return;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(load_agent(&n64[node].lo0[a]), load_agent(&n64[node].lo1[a]));
      hi[a] = fmaxf(load_agent(&n64[node].hi0[a]), load_agent(&n64[node].hi1[a]));
    }
    put_box(n64, p >> 1, p & 1, lo, hi);
    put_box(n32, p >> 1, p & 1, lo, hi);
    node = p >> 1;
  }
}

__global__ __launch_bounds__(kBlock) void k_bins(const double* v, const int32_t* f, const int32_t* order,
                                                  long long nf, long long rec0, DevBinTri* out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nf) return;
  const int32_t face = order[i];
  const int32_t* fi = f + 3 * (size_t)face;
  DevBinTri t;
  for (int c = 0; c < 3; ++c)
    for (int a = 0; a < 3; ++a) t.v[c][a] = v[3 * (size_t)fi[c] + a];
  t.rec = (int32_t)(rec0 + i * (long long)sizeof(TriFast));
  t.face = face;
  out[i] = t;
}

}  // namespace
}  // namespace rtmi

using namespace rtmi;

extern "C" int rtmi_mesh_bounds(const double* v, int64_t nv, const int32_t* f, int64_t nf, unsigned long long* scratch,
                                MeshBounds* out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  unsigned long long h[kMeshBoundsWords];
  std::memset(h, 0, sizeof h);
  for (int a = 0; a < 3; ++a) h[W_FLO + a] = h[W_ALO + a] = ~0ull;
  for (int a = 0; a < 6; ++a) h[W_IDX + a] = ~0ull;
  hipError_t e = hipMemcpyAsync(scratch, h, sizeof h, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  if (nf > 0) k_face_bounds<<<std::min(grid(nf), 2048u), kBlock, 0, st>>>(v, f, nf, scratch);
  if (nv > 0) {
    k_all_bounds<<<std::min(grid(nv), 2048u), kBlock, 0, st>>>(v, nv, scratch);
    k_all_first<<<std::min(grid(nv), 2048u), kBlock, 0, st>>>(v, nv, scratch);
  }
  k_all_gather<<<1, 64, 0, st>>>(v, scratch);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipMemcpyAsync(h, scratch, sizeof h, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;
  for (int a = 0; a < 3; ++a) {
    out->flo[a] = unord_bits(h[W_FLO + a]);
    out->fhi[a] = unord_bits(h[W_FHI + a]);
    std::memcpy(&out->alo[a], &h[W_OUT + a], sizeof(double));
    std::memcpy(&out->ahi[a], &h[W_OUT + 3 + a], sizeof(double));
  }
  out->nonfinite = h[W_BAD] != 0 ? 1 : 0;
  return 0;
}

extern "C" int rtmi_mesh_normals(const double* v, const int32_t* f, const double* given, int64_t nf, double* n64,
                                 float* n32, void* stream) {
  if (nf <= 0) return 0;
  k_normals<<<grid(nf), kBlock, 0, (hipStream_t)stream>>>(v, f, given, nf, n64, n32);
  return (int)hipGetLastError();
}

extern "C" int rtmi_mesh_refit(const double* v, const int32_t* f, const int32_t* order, double inflate, int32_t node0,
                               int32_t nnode, int64_t tri_base, const int32_t* parent, int32_t* arrivals,
                               BvhNode* nodes64, BvhNode* nodes32, void* stream) {
  if (nnode <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(arrivals, 0, (size_t)nnode * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  k_refit<<<grid(nnode), kBlock, 0, st>>>(v, f, order, inflate, node0, nnode, tri_base, parent, arrivals, nodes64,
                                          nodes32);
  return (int)hipGetLastError();
}

extern "C" int rtmi_mesh_bins(const double* v, const int32_t* f, const int32_t* order, int64_t nf, int64_t rec0,
                              DevBinTri* out, void* stream) {
  if (nf <= 0) return 0;
  k_bins<<<grid(nf), kBlock, 0, (hipStream_t)stream>>>(v, f, order, nf, rec0, out);
  return (int)hipGetLastError();
}
