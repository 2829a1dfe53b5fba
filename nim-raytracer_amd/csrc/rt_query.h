// rt_query.h — ray queries (include/rtmi.h rt_trace_rays* / rt_pick_pixels* /
// rt_shade_rays*): what the host library (rt_queries.cpp) and the query
// kernels (rt_kernels_query.hip, rt_kernels_shade.hip) share.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rt_common.h"

namespace rtmi {

// rt_hit of include/rtmi.h
struct QueryHit {
  double t;
  int32_t obj;
  int32_t face;
};
static_assert(sizeof(QueryHit) == 16, "rt_hit is 16 bytes");

// One batch (all pointers device memory). The scene, the camera and the
// image size of a pick travel in the RenderParams<double> next to it.
struct QueryParams {
  const double* orig;    // n * 3, or nullptr: picks
  const double* dir;     // n * 3
  const double* tnear;   // n, or nullptr: +inf
  const double* xy;      // picks: n * 2 image positions
  const uint32_t* order; // RT_QUERY_SORT: slot k traces ray order[k]; nullptr: ray k
  QueryHit* hits;        // n
  double* normals;       // n * 3, or nullptr
  unsigned long long* partials;  // [waves][kStatSlots]
  long long n;
  int32_t any_hit;       // RT_QUERY_ANY_HIT
  int32_t pad;
  // rt_shade_rays_f32*: the batch's float rays (n * 3 each) for RT_QUERY_SORT's
  // keys, instead of orig / dir; nullptr for every float64 query
  const float* orig32;
  const float* dir32;
  // rt_trace_rays_f32*: the rays' float t_near (n, or nullptr: +inf) beside
  // orig32 / dir32; rt_pick_pixels_f32*: the float image positions (n * 2)
  // instead of xy
  const float* tnear32;
  const float* xy32;
};

// Where k_shade_rays leaves ray i's colour (rt_shade_rays*): three float64 at
// rgb[3 i] and / or three float32 at rgb32[3 i] (device memory; nullptr: not
// written). A call with group > 1 points rgb at a temporary k_shade_reduce sums.
struct ShadeOut {
  double* rgb;
  float* rgb32;
};

// RT_QUERY_SORT's device temporaries, carved from one allocation of
// rtmi_query_sort_bytes(n) bytes: keys and ray indices (in and out of the
// radix sort), the batch's bounds, rocPRIM's temporary storage.
struct QuerySortBufs {
  uint32_t *key, *key2, *idx, *idx2;
  unsigned long long* bounds;  // 6 ordered-integer minima, then 6 maxima
  void* tmp;
  size_t tmp_bytes;
};

}  // namespace rtmi

extern "C" {
// resident blocks of k_trace_rays per CU (its grid: the device's CUs, not n)
int rtmi_query_blocks_per_cu();
int rtmi_launch_query(const rtmi::RenderParams<double>* p, const rtmi::QueryParams* q, int blocks, void* stream);
// rows of kStatSlots per-wave counters -> acc[kStatSlots]
int rtmi_launch_query_reduce(const unsigned long long* partials, int rows, unsigned long long* acc, void* stream);
// bytes of the sort's temporaries for n rays; 0 on failure
size_t rtmi_query_sort_bytes(long long n);
void rtmi_query_sort_carve(void* base, long long n, rtmi::QuerySortBufs* out);
// keys of the batch (q.orig / q.dir / q.tnear, or q.xy) and the sorted ray
// order at b.idx2
int rtmi_query_sort(const rtmi::QueryParams* q, const rtmi::QuerySortBufs* b, void* stream);
// k_shade_rays (rt_kernels_shade.hip): reflective = 0: the one-level
// instantiation, 1: kMaxShadeLevels. Resident blocks per CU, and the launch.
int rtmi_shade_blocks_per_cu(int reflective);
int rtmi_launch_shade(const rtmi::RenderParams<double>* p, const rtmi::QueryParams* q, const rtmi::ShadeOut* so,
                      int reflective, int blocks, void* stream);
// calcPixel's sum over each run of `group` ray colours: ngroups outputs
int rtmi_launch_shade_reduce(const double* ray_rgb, long long ngroups, int group, double inv_len, double* rgb,
                             float* rgb32, void* stream);
}
