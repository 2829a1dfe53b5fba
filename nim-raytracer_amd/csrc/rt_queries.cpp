// rt_queries.cpp — ray queries (rt_trace_rays* / rt_pick_pixels*): float64
// closest hit, any hit and pixel picking on a scene, beside its render calls;
// and radiance queries: the reference's colour along caller-supplied rays in
// float64 (rt_shade_rays*), the float32 render's in float32 (rt_shade_rays_f32*);
// and the float32 render's trace for float32 rays and picks
// (rt_trace_rays_f32* / rt_pick_pixels_f32*).
#include <cmath>
#include <cstring>

#include "rt_query.h"
#include "rt_scene.h"

namespace {

constexpr uint32_t kQueryFlags = RT_QUERY_ANY_HIT | RT_QUERY_SORT;

// What every query entry point checks before it takes the scene's lock.
int query_check(const rt_scene* s, int64_t n, uint32_t flags, const void* hits, const double* normals) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (flags & ~kQueryFlags) return fail(RT_E_INVALID, "unknown query flags 0x%x", flags & ~kQueryFlags);
  if ((flags & RT_QUERY_ANY_HIT) && normals)
    return fail(RT_E_INVALID, "normals are not available with RT_QUERY_ANY_HIT");
  if (n > 0 && !hits) return fail(RT_E_INVALID, "null hits");
  if (n > INT32_MAX) return fail(RT_E_UNSUPPORTED, "%lld rays in one batch (at most 2^31 - 1)", (long long)n);
  return RT_OK;
}

int pick_check(const rt_options* o) {
  if (!o) return fail(RT_E_INVALID, "null options");
  if (o->width <= 0 || o->height <= 0 || o->width > 65536 || o->height > 65536)
    return fail(RT_E_INVALID, "bad image size %dx%d", o->width, o->height);
  if (o->precision != RT_FP64)
    return fail(o->precision == RT_FP32 ? RT_E_UNSUPPORTED : RT_E_INVALID, "ray queries are float64 only (precision %d)",
                o->precision);
  return RT_OK;
}

// RenderParams<double> as the float64 render fills it, without a
// framebuffer, pixel records or lists: the scene, and for picks the camera
// and the image size castPrimaryRay reads (fill_params' operations).
void fill_query(const rt_scene* s, int width, int height, RenderParams<double>& p) {
  std::memset(&p, 0, sizeof p);
  p.objects = s->f64.objects.p;
  p.lights = s->f64.lights.p;
  p.meshes = s->f64.meshes.p;
  p.nodes = s->nodes.p;
  p.tris = s->f64.tris.p;
  p.normals = s->f64.normals.p;
  for (int k = 0; k < 16; ++k) p.c2w[k] = s->c2w[k];
  for (int k = 0; k < 3; ++k) p.bg[k] = s->bg[k];
  p.f = std::tan(s->fov * (3.14159265358979323846 / 180.0) / 2);
  p.aspect = (double)width / (double)height;
  p.inv_len = 1.0;
  p.nobj = s->nobj;
  p.nlight = s->nlight;
  p.width = width;
  p.height = height;
  p.grid_m = 1;
  p.spp = 1;
  p.shadow_mesh = s->shadow_mesh;
  p.lean_plane = -1;
  p.max_iters = (int32_t)std::min<int64_t>(INT32_MAX, 2 * s->num_nodes + 16);
}

// What every query does before its kernels (the scene's lock held, its device
// current): orders itself after a render still in flight on the scene, and
// after the last query (it shares this one's temporaries) unless this stream
// orders them anyway; makes sure of the per-wave Stats rows.
int query_begin(rt_scene* s, hipStream_t st) {
  if (!s->q_done) HIP_TRY(hipEventCreateWithFlags(&s->q_done.h, hipEventDisableTiming));
  if (st != s->done_stream) HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
  if (s->q_done_rec && st != s->q_stream) HIP_TRY(hipStreamWaitEvent(st, s->q_done, 0));
  const size_t rows = (size_t)s->max_waves;
  if (s->q_partials.n < (rows + 1) * kStatSlots) {
    if (int rc = s->q_partials.alloc((rows + 1) * kStatSlots)) return rc;
  }
  return RT_OK;
}

// RT_QUERY_SORT: q.order = the batch's coherence order (nullptr without the flag)
int query_order(rt_scene* s, QueryParams& q, uint32_t flags, hipStream_t st) {
  q.order = nullptr;
  if (!(flags & RT_QUERY_SORT)) return RT_OK;
  const size_t need = rtmi_query_sort_bytes(q.n);
  if (!need) return fail(RT_E_DEVICE, "sizing the ray sort failed");
  if (s->q_sort.n < need) {
    // an earlier query may still read the old buffer
    if (s->q_done_rec) HIP_TRY(hipEventSynchronize(s->q_done));
    if (int rc = s->q_sort.alloc(need)) return rc;
  }
  QuerySortBufs b;
  rtmi_query_sort_carve(s->q_sort.p, q.n, &b);
  if (const int e = rtmi_query_sort(&q, &b, st))
    return fail(RT_E_DEVICE, "ray sort failed: %s", hipGetErrorString((hipError_t)e));
  q.order = b.idx2;
  return RT_OK;
}

// the grid: the device's resident blocks, or fewer when the batch is small
int query_blocks(const rt_scene* s, long long n, int blocks_per_cu) {
  const long long steps = (n + 63) / 64;
  return (int)std::max(1LL, std::min({(steps + 3) / 4, (long long)blocks_per_cu * s->num_cus,
                                      (long long)s->max_waves / 4}));
}

// After a query's kernels: the Stats rows of its `blocks` blocks summed (when
// the caller reads them: h receives the kStatSlots sums, after a wait), and
// the query's completion recorded.
int query_end(rt_scene* s, int blocks, hipStream_t st, unsigned long long* h) {
  unsigned long long* acc = s->q_partials.p + (size_t)s->max_waves * kStatSlots;
  if (h) {
    if (const int e = rtmi_launch_query_reduce(s->q_partials.p, blocks * 4, acc, st))
      return fail(RT_E_DEVICE, "ray query stats reduction failed: %s", hipGetErrorString((hipError_t)e));
  }
  HIP_TRY(hipEventRecord(s->q_done, st));
  s->q_done_rec = true;
  s->q_stream = st;
  if (h) {
    HIP_TRY(hipMemcpyAsync(h, acc, kStatSlots * sizeof *h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return RT_OK;
}

// The device body of every hit query (the scene's lock held, its device
// current): q's ray, hit and normal pointers are device memory.
int query_device(rt_scene* s, const RenderParams<double>& p, QueryParams q, uint32_t flags, hipStream_t st,
                 rt_stats* out) {
  if (int rc = query_begin(s, st)) return rc;
  if (s->q_blocks_per_cu < 0) s->q_blocks_per_cu = rtmi_query_blocks_per_cu();
  if (s->q_blocks_per_cu <= 0) return fail(RT_E_DEVICE, "the ray query kernel is not resident on this device");
  q.any_hit = (flags & RT_QUERY_ANY_HIT) ? 1 : 0;
  q.partials = s->q_partials.p;
  if (int rc = query_order(s, q, flags, st)) return rc;
  const int blocks = query_blocks(s, q.n, s->q_blocks_per_cu);
  if (const int e = rtmi_launch_query(&p, &q, blocks, st))
    return fail(RT_E_DEVICE, "ray query launch failed: %s", hipGetErrorString((hipError_t)e));
  unsigned long long h[kStatSlots];
  if (int rc = query_end(s, blocks, st, out ? h : nullptr)) return rc;
  if (out) {
    *out = rt_stats{};
    out->num_primary_rays = q.xy ? h[STAT_PRIMARY] : 0;  // camera rays are a pick's; the kernel counts the rays it traced
    out->num_intersection_tests = h[STAT_TESTS];
    out->num_intersection_hits = h[STAT_HITS];
  }
  return RT_OK;
}

// Host form: the batch copied into the scene's staging buffer, queried on
// the scene's own stream, the answers copied back. in[k]: host arrays of
// in_bytes[k] bytes (nullptr: absent).
int query_host(rt_scene* s, const RenderParams<double>& p, int64_t n, const void* const in[4], const size_t in_bytes[4],
               uint32_t flags, rt_hit* hits, double* normals, rt_stats* out) {
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t off[6], total = 0;
  for (int k = 0; k < 4; ++k) {
    off[k] = total;
    total += in[k] ? al(in_bytes[k]) : 0;
  }
  off[4] = total;
  total += al((size_t)n * sizeof(rt_hit));
  off[5] = total;
  total += normals ? al((size_t)n * 3 * sizeof(double)) : 0;
  hipStream_t st = s->stream;
  if (s->q_stage.n < total) {
    if (s->q_done_rec) HIP_TRY(hipEventSynchronize(s->q_done));
    if (int rc = s->q_stage.alloc(total)) return rc;
  }
  unsigned char* base = s->q_stage.p;
  // the staging buffer's last user was a query on this stream, or has been waited for
  if (s->q_done_rec && st != s->q_stream) HIP_TRY(hipStreamWaitEvent(st, s->q_done, 0));
  for (int k = 0; k < 4; ++k)
    if (in[k]) HIP_TRY(hipMemcpyAsync(base + off[k], in[k], in_bytes[k], hipMemcpyHostToDevice, st));
  QueryParams q{};
  q.orig = in[0] ? (const double*)(base + off[0]) : nullptr;
  q.dir = in[1] ? (const double*)(base + off[1]) : nullptr;
  q.tnear = in[2] ? (const double*)(base + off[2]) : nullptr;
  q.xy = in[3] ? (const double*)(base + off[3]) : nullptr;
  q.hits = (QueryHit*)(base + off[4]);
  q.normals = normals ? (double*)(base + off[5]) : nullptr;
  q.n = n;
  if (int rc = query_device(s, p, q, flags, st, out)) return rc;
  HIP_TRY(hipMemcpyAsync(hits, base + off[4], (size_t)n * sizeof(rt_hit), hipMemcpyDeviceToHost, st));
  if (normals)
    HIP_TRY(hipMemcpyAsync(normals, base + off[5], (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RT_OK;
}

}  // namespace

static_assert(sizeof(rt_hit) == sizeof(QueryHit), "rt_hit layout");

extern "C" int rt_trace_rays_device(rt_scene* s, int64_t n, const double* d_orig, const double* d_dir,
                                    const double* d_tnear, uint32_t flags, rt_hit* d_hits, double* d_normals,
                                    void* stream, rt_stats* out) {
  if (int rc = query_check(s, n, flags, d_hits, d_normals)) return rc;
  if (n > 0 && (!d_orig || !d_dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  RenderParams<double> p;
  fill_query(s, 1, 1, p);
  QueryParams q{};
  q.orig = d_orig;
  q.dir = d_dir;
  q.tnear = d_tnear;
  q.hits = (QueryHit*)d_hits;
  q.normals = d_normals;
  q.n = n;
  return query_device(s, p, q, flags, (hipStream_t)stream, out);
}

extern "C" int rt_trace_rays(rt_scene* s, int64_t n, const double* orig, const double* dir, const double* tnear,
                             uint32_t flags, rt_hit* hits, double* normals, rt_stats* out) {
  if (int rc = query_check(s, n, flags, hits, normals)) return rc;
  if (n > 0 && (!orig || !dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  RenderParams<double> p;
  fill_query(s, 1, 1, p);
  const size_t v3 = (size_t)n * 3 * sizeof(double);
  const void* const in[4] = {orig, dir, tnear, nullptr};
  const size_t bytes[4] = {v3, v3, (size_t)n * sizeof(double), 0};
  return query_host(s, p, n, in, bytes, flags, hits, normals, out);
}

extern "C" int rt_pick_pixels_device(rt_scene* s, const rt_options* o, int64_t n, const double* d_xy, uint32_t flags,
                                     rt_hit* d_hits, double* d_normals, void* stream, rt_stats* out) {
  if (int rc = query_check(s, n, flags, d_hits, d_normals)) return rc;
  if (int rc = pick_check(o)) return rc;
  if (n > 0 && !d_xy) return fail(RT_E_INVALID, "null pixel positions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  RenderParams<double> p;
  fill_query(s, o->width, o->height, p);
  QueryParams q{};
  q.xy = d_xy;
  q.hits = (QueryHit*)d_hits;
  q.normals = d_normals;
  q.n = n;
  return query_device(s, p, q, flags, (hipStream_t)stream, out);
}

extern "C" int rt_pick_pixels(rt_scene* s, const rt_options* o, int64_t n, const double* xy, uint32_t flags,
                              rt_hit* hits, double* normals, rt_stats* out) {
  if (int rc = query_check(s, n, flags, hits, normals)) return rc;
  if (int rc = pick_check(o)) return rc;
  if (n > 0 && !xy) return fail(RT_E_INVALID, "null pixel positions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  RenderParams<double> p;
  fill_query(s, o->width, o->height, p);
  const void* const in[4] = {nullptr, nullptr, nullptr, xy};
  const size_t bytes[4] = {0, 0, 0, (size_t)n * 2 * sizeof(double)};
  return query_host(s, p, n, in, bytes, flags, hits, normals, out);
}

// ---- radiance queries (rt_shade_rays*) --------------------------------------
namespace {

// What both shade entry points check before they take the scene's lock.
int shade_check(const rt_scene* s, const rt_options* o, int64_t n, int32_t group, uint32_t flags, const void* rgb,
                const void* rgb32) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!o) return fail(RT_E_INVALID, "null options");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (flags & ~(uint32_t)RT_QUERY_SORT)
    return fail(RT_E_INVALID, "rt_shade_rays takes RT_QUERY_SORT only (flags 0x%x)", flags);
  if (group < 1) return fail(RT_E_INVALID, "group %d (at least 1)", group);
  if (n % group) return fail(RT_E_INVALID, "%lld rays are not a whole number of groups of %d", (long long)n, group);
  if (n > 0 && !rgb && !rgb32) return fail(RT_E_INVALID, "null rgb and rgb32");
  if (o->precision != RT_FP64)
    return fail(o->precision == RT_FP32 ? RT_E_UNSUPPORTED : RT_E_INVALID,
                "radiance queries are float64 only (precision %d)", o->precision);
  if (n > INT32_MAX) return fail(RT_E_UNSUPPORTED, "%lld rays in one batch (at most 2^31 - 1)", (long long)n);
  return RT_OK;
}

// The device body of both forms (the scene's lock held, its device current):
// q.orig / q.dir and the outputs are device memory.
int shade_device(rt_scene* s, const rt_options* o, QueryParams q, int32_t group, uint32_t flags, double* d_rgb,
                 float* d_rgb32, hipStream_t st, rt_stats* out) {
  // as check_options says it for a render (any_reflective: under the lock, rt_scene_set_objects may flip it)
  if (s->any_reflective && o->max_ray_depth > kMaxShadeLevels - 1)
    return fail(RT_E_UNSUPPORTED, "max_ray_depth %d > %d with reflective materials", o->max_ray_depth,
                kMaxShadeLevels - 1);
  RenderParams<double> p;
  fill_query(s, 1, 1, p);
  p.bias = o->bias;
  p.max_depth = o->max_ray_depth;
  if (int rc = query_begin(s, st)) return rc;
  // one level when no reflection ray can follow a hit (renderer.nim:104)
  const int reflective = s->any_reflective && o->max_ray_depth >= 1 ? 1 : 0;
  int& bpc = s->q_shade_blocks_per_cu[reflective];
  if (bpc < 0) bpc = rtmi_shade_blocks_per_cu(reflective);
  if (bpc <= 0) return fail(RT_E_DEVICE, "the radiance query kernel is not resident on this device");
  ShadeOut so{d_rgb, d_rgb32};
  if (group > 1) {
    // the rays' colours, summed per group by k_shade_reduce
    const size_t need = (size_t)q.n * 3;
    if (s->q_shade.n < need) {
      if (s->q_done_rec) HIP_TRY(hipEventSynchronize(s->q_done));  // an earlier query may still read the old buffer
      if (int rc = s->q_shade.alloc(need)) return rc;
    }
    so = ShadeOut{s->q_shade.p, nullptr};
  }
  q.partials = s->q_partials.p;
  if (int rc = query_order(s, q, flags, st)) return rc;
  const int blocks = query_blocks(s, q.n, bpc);
  if (const int e = rtmi_launch_shade(&p, &q, &so, reflective, blocks, st))
    return fail(RT_E_DEVICE, "radiance query launch failed: %s", hipGetErrorString((hipError_t)e));
  if (group > 1) {
    if (const int e = rtmi_launch_shade_reduce(so.rgb, q.n / group, group, 1.0 / (double)group, d_rgb, d_rgb32, st))
      return fail(RT_E_DEVICE, "radiance query group sum failed: %s", hipGetErrorString((hipError_t)e));
  }
  unsigned long long h[kStatSlots];
  if (int rc = query_end(s, blocks, st, out ? h : nullptr)) return rc;
  if (out) {
    out->num_primary_rays = h[STAT_PRIMARY];
    out->num_intersection_tests = h[STAT_TESTS];
    out->num_intersection_hits = h[STAT_HITS];
    out->num_shadow_rays = h[STAT_SHADOW];
    out->num_reflection_rays = h[STAT_REFL];
  }
  return RT_OK;
}

}  // namespace

extern "C" int rt_shade_rays_device(rt_scene* s, const rt_options* o, int64_t n, const double* d_orig,
                                    const double* d_dir, int32_t group, uint32_t flags, double* d_rgb, float* d_rgb32,
                                    void* stream, rt_stats* out) {
  if (int rc = shade_check(s, o, n, group, flags, d_rgb, d_rgb32)) return rc;
  if (n > 0 && (!d_orig || !d_dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  QueryParams q{};
  q.orig = d_orig;
  q.dir = d_dir;
  q.n = n;
  return shade_device(s, o, q, group, flags, d_rgb, d_rgb32, (hipStream_t)stream, out);
}

extern "C" int rt_shade_rays(rt_scene* s, const rt_options* o, int64_t n, const double* orig, const double* dir,
                             int32_t group, uint32_t flags, double* rgb, float* rgb32, rt_stats* out) {
  if (int rc = shade_check(s, o, n, group, flags, rgb, rgb32)) return rc;
  if (n > 0 && (!orig || !dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  // the batch copied into the scene's staging buffer, shaded on the scene's
  // own stream, the colours copied back (query_host's discipline)
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t v3 = (size_t)n * 3 * sizeof(double), ng = (size_t)(n / group);
  const size_t off_dir = al(v3), off_rgb = off_dir + al(v3);
  const size_t off_rgb32 = off_rgb + (rgb ? al(ng * 3 * sizeof(double)) : 0);
  const size_t total = off_rgb32 + (rgb32 ? al(ng * 3 * sizeof(float)) : 0);
  hipStream_t st = s->stream;
  if (s->q_stage.n < total) {
    if (s->q_done_rec) HIP_TRY(hipEventSynchronize(s->q_done));
    if (int rc = s->q_stage.alloc(total)) return rc;
  }
  unsigned char* base = s->q_stage.p;
  // the staging buffer's last user was a query on this stream, or has been waited for
  if (s->q_done_rec && st != s->q_stream) HIP_TRY(hipStreamWaitEvent(st, s->q_done, 0));
  HIP_TRY(hipMemcpyAsync(base, orig, v3, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(base + off_dir, dir, v3, hipMemcpyHostToDevice, st));
  QueryParams q{};
  q.orig = (const double*)base;
  q.dir = (const double*)(base + off_dir);
  q.n = n;
  double* d_rgb = rgb ? (double*)(base + off_rgb) : nullptr;
  float* d_rgb32 = rgb32 ? (float*)(base + off_rgb32) : nullptr;
  if (int rc = shade_device(s, o, q, group, flags, d_rgb, d_rgb32, st, out)) return rc;
  if (rgb) HIP_TRY(hipMemcpyAsync(rgb, d_rgb, ng * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (rgb32) HIP_TRY(hipMemcpyAsync(rgb32, d_rgb32, ng * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RT_OK;
}

// ---- float32 radiance queries (rt_shade_rays_f32*) --------------------------
namespace {

// What both float32 shade entry points check before they take the scene's lock.
int shade32_check(const rt_scene* s, const rt_options* o, int64_t n, int32_t group, uint32_t flags, const void* orig,
                  const void* dir, const void* rgb) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!o) return fail(RT_E_INVALID, "null options");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (flags & ~(uint32_t)RT_QUERY_SORT)
    return fail(RT_E_INVALID, "rt_shade_rays_f32 takes RT_QUERY_SORT only (flags 0x%x)", flags);
  if (group < 1) return fail(RT_E_INVALID, "group %d (at least 1)", group);
  if (n % group) return fail(RT_E_INVALID, "%lld rays are not a whole number of groups of %d", (long long)n, group);
  if (n > 0 && (!orig || !dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  if (n > 0 && !rgb) return fail(RT_E_INVALID, "null rgb");
  if (o->precision != RT_FP32)
    return fail(RT_E_INVALID, "rt_shade_rays_f32 is float32 only (precision %d): rt_shade_rays is the float64 query",
                o->precision);
  if (n > INT32_MAX) return fail(RT_E_UNSUPPORTED, "%lld rays in one batch (at most 2^31 - 1)", (long long)n);
  return RT_OK;
}

// The device body of both forms (the scene's lock held, its device current):
// q.orig / q.dir and d_rgb are device memory.
int shade32_device(rt_scene* s, const rt_options* o, Shade32Params q, int32_t group, uint32_t flags, float* d_rgb,
                   hipStream_t st, rt_stats* out) {
  // as check_options says it for a render (any_reflective: under the lock, rt_scene_set_objects may flip it)
  if (s->any_reflective && o->max_ray_depth > kMaxShadeLevels - 1)
    return fail(RT_E_UNSUPPORTED, "max_ray_depth %d > %d with reflective materials", o->max_ray_depth,
                kMaxShadeLevels - 1);
  // the scene's subset, as a render launches it (under the lock: rt_scene_set_lights / _set_objects flip bits)
  const unsigned sub = s->f32_subset & ~(unsigned)SUB_STOCHASTIC & 63u;
  // the scene words, bias, max_depth and the Stats rows; everything else
  // stays zero: no camera, mapping or per-call word is reachable
  FastParams p;
  std::memset(&p, 0, sizeof p);
  fast_scene_words(s, o->flags, p);
  p.bias = (float)o->bias;
  p.max_depth = o->max_ray_depth;
  if (int rc = query_begin(s, st)) return rc;
  p.partials = s->q_partials.p;
  int& bpc = s->q_shade32_blocks_per_cu[sub];
  if (bpc == 0) bpc = rtmi_shade_f32_blocks_per_cu(sub);
  if (bpc <= 0)
    return fail(RT_E_DEVICE, "the float32 radiance query kernel (subset %u) is not resident on this device", sub);
  q.rgb = d_rgb;
  if (group > 1) {
    // the rays' colours, summed per group by k_shade_reduce32
    const size_t need = (size_t)q.n * 3;
    if (s->q_shade32.n < need) {
      if (s->q_done_rec) HIP_TRY(hipEventSynchronize(s->q_done));  // an earlier query may still read the old buffer
      if (int rc = s->q_shade32.alloc(need)) return rc;
    }
    q.rgb = s->q_shade32.p;
  }
  QueryParams qs{};  // RT_QUERY_SORT: the float-ray form of the keys
  qs.orig32 = q.orig;
  qs.dir32 = q.dir;
  qs.n = q.n;
  if (int rc = query_order(s, qs, flags, st)) return rc;
  q.order = qs.order;
  const int blocks = query_blocks(s, q.n, bpc);
  if (const int e = rtmi_launch_shade_f32(&p, &q, sub, blocks, st))
    return fail(RT_E_DEVICE, "float32 radiance query launch failed: %s", hipGetErrorString((hipError_t)e));
  if (group > 1) {
    if (const int e = rtmi_launch_shade_reduce32(q.rgb, q.n / group, group, (float)(1.0 / (double)group), d_rgb, st))
      return fail(RT_E_DEVICE, "float32 radiance query group sum failed: %s", hipGetErrorString((hipError_t)e));
  }
  unsigned long long h[kStatSlots];
  if (int rc = query_end(s, blocks, st, out ? h : nullptr)) return rc;
  if (out) {
    // one test per object per trace call (renderer.nim:54-56); the float32
    // kernels leave the slot at 0 and the count is derived, as for a render
    const unsigned long long rays = h[STAT_PRIMARY] + h[STAT_SHADOW] + h[STAT_REFL];
    out->num_primary_rays = h[STAT_PRIMARY];
    out->num_intersection_tests = (unsigned long long)s->nobj * rays;
    out->num_intersection_hits = h[STAT_HITS];
    out->num_shadow_rays = h[STAT_SHADOW];
    out->num_reflection_rays = h[STAT_REFL];
  }
  return RT_OK;
}

}  // namespace

extern "C" int rt_shade_rays_f32_device(rt_scene* s, const rt_options* o, int64_t n, const float* d_orig,
                                        const float* d_dir, int32_t group, uint32_t flags, float* d_rgb, void* stream,
                                        rt_stats* out) {
  if (int rc = shade32_check(s, o, n, group, flags, d_orig, d_dir, d_rgb)) return rc;
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  Shade32Params q{};
  q.orig = d_orig;
  q.dir = d_dir;
  q.n = n;
  return shade32_device(s, o, q, group, flags, d_rgb, (hipStream_t)stream, out);
}

extern "C" int rt_shade_rays_f32(rt_scene* s, const rt_options* o, int64_t n, const float* orig, const float* dir,
                                 int32_t group, uint32_t flags, float* rgb, rt_stats* out) {
  if (int rc = shade32_check(s, o, n, group, flags, orig, dir, rgb)) return rc;
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  // the batch copied into the scene's staging buffer, shaded on the scene's
  // own stream, the colours copied back (query_host's discipline)
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t v3 = (size_t)n * 3 * sizeof(float), ng = (size_t)(n / group);
  const size_t off_dir = al(v3), off_rgb = off_dir + al(v3);
  const size_t total = off_rgb + al(ng * 3 * sizeof(float));
  hipStream_t st = s->stream;
  if (s->q_stage.n < total) {
    if (s->q_done_rec) HIP_TRY(hipEventSynchronize(s->q_done));
    if (int rc = s->q_stage.alloc(total)) return rc;
  }
  unsigned char* base = s->q_stage.p;
  // the staging buffer's last user was a query on this stream, or has been waited for
  if (s->q_done_rec && st != s->q_stream) HIP_TRY(hipStreamWaitEvent(st, s->q_done, 0));
  HIP_TRY(hipMemcpyAsync(base, orig, v3, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(base + off_dir, dir, v3, hipMemcpyHostToDevice, st));
  Shade32Params q{};
  q.orig = (const float*)base;
  q.dir = (const float*)(base + off_dir);
  q.n = n;
  float* d_rgb = (float*)(base + off_rgb);
  if (int rc = shade32_device(s, o, q, group, flags, d_rgb, st, out)) return rc;
  HIP_TRY(hipMemcpyAsync(rgb, d_rgb, ng * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RT_OK;
}

// ---- float32 ray queries and picks (rt_trace_rays_f32* / rt_pick_pixels_f32*) ----
static_assert(sizeof(rt_hit32) == sizeof(Hit32), "rt_hit32 layout");

namespace {

// What every float32 hit query checks before it takes the scene's lock.
int trace32_check(const rt_scene* s, int64_t n, uint32_t flags, const void* hits, const void* normals) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (flags & ~kQueryFlags) return fail(RT_E_INVALID, "unknown query flags 0x%x", flags & ~kQueryFlags);
  if ((flags & RT_QUERY_ANY_HIT) && normals)
    return fail(RT_E_INVALID, "normals are not available with RT_QUERY_ANY_HIT");
  if (n > 0 && !hits) return fail(RT_E_INVALID, "null hits");
  if (n > INT32_MAX) return fail(RT_E_UNSUPPORTED, "%lld rays in one batch (at most 2^31 - 1)", (long long)n);
  return RT_OK;
}

int pick32_check(const rt_options* o) {
  if (!o) return fail(RT_E_INVALID, "null options");
  if (o->width <= 0 || o->height <= 0 || o->width > 65536 || o->height > 65536)
    return fail(RT_E_INVALID, "bad image size %dx%d", o->width, o->height);
  if (o->precision != RT_FP32)
    return fail(RT_E_INVALID, "rt_pick_pixels_f32 is float32 only (precision %d): rt_pick_pixels is the float64 pick",
                o->precision);
  return RT_OK;
}

// The device body of every float32 hit query (the scene's lock held, its
// device current): q's ray, hit and normal pointers are device memory. pick:
// the image size of a pick (its width and height alone are read), nullptr for
// a trace.
int trace32_device(rt_scene* s, const rt_options* pick, Trace32Params q, uint32_t flags, hipStream_t st,
                   rt_stats* out) {
  if ((uintptr_t)q.hits & 15u) return fail(RT_E_INVALID, "hits must be 16-byte aligned device memory");
  // trace reads the geometry bits alone (under the lock: rt_scene_set_objects may flip them)
  const unsigned sub = s->f32_subset & 15u;
  // the scene words and the Stats rows, for picks the render's camera
  // constants; everything else stays zero: no grid, mapping or per-call word
  // is reachable (pix = -1, light = -1)
  FastParams p;
  std::memset(&p, 0, sizeof p);
  if (pick) {
    rt_options oc{};
    oc.width = pick->width;
    oc.height = pick->height;
    oc.aa_kind = RT_AA_NONE;
    fast_camera(s->c2w, s->fov, &oc, p);
  }
  fast_scene_words(s, RT_FLAG_NO_BINNING, p);
  if (int rc = query_begin(s, st)) return rc;
  p.partials = s->q_partials.p;
  int& bpc = s->q_trace32_blocks_per_cu[sub];
  if (bpc == 0) bpc = rtmi_trace_f32_blocks_per_cu(sub);
  if (bpc <= 0)
    return fail(RT_E_DEVICE, "the float32 ray query kernel (subset %u) is not resident on this device", sub);
  q.any_hit = (flags & RT_QUERY_ANY_HIT) ? 1 : 0;
  QueryParams qs{};  // RT_QUERY_SORT: the float forms of the keys
  qs.orig32 = q.orig;
  qs.dir32 = q.dir;
  qs.tnear32 = q.tnear;
  qs.xy32 = q.xy;
  qs.n = q.n;
  if (int rc = query_order(s, qs, flags, st)) return rc;
  q.order = qs.order;
  const int blocks = query_blocks(s, q.n, bpc);
  if (const int e = rtmi_launch_trace_f32(&p, &q, sub, blocks, st))
    return fail(RT_E_DEVICE, "float32 ray query launch failed: %s", hipGetErrorString((hipError_t)e));
  unsigned long long h[kStatSlots];
  if (int rc = query_end(s, blocks, st, out ? h : nullptr)) return rc;
  if (out) {
    // one test per object per trace call (renderer.nim:54-56): derived, as
    // shade32_device derives it; camera rays are a pick's
    *out = rt_stats{};
    out->num_primary_rays = pick ? h[STAT_PRIMARY] : 0;
    out->num_intersection_tests = (unsigned long long)s->nobj * h[STAT_PRIMARY];
    out->num_intersection_hits = h[STAT_HITS];
  }
  return RT_OK;
}

// Host form: the batch copied into the scene's staging buffer, queried on the
// scene's own stream, the answers copied back (query_host's discipline).
// in[k]: host arrays of in_bytes[k] bytes (nullptr: absent): orig, dir, tnear, xy.
int trace32_host(rt_scene* s, const rt_options* pick, int64_t n, const void* const in[4], const size_t in_bytes[4],
                 uint32_t flags, rt_hit32* hits, float* normals, rt_stats* out) {
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t off[6], total = 0;
  for (int k = 0; k < 4; ++k) {
    off[k] = total;
    total += in[k] ? al(in_bytes[k]) : 0;
  }
  off[4] = total;
  total += al((size_t)n * sizeof(rt_hit32));
  off[5] = total;
  total += normals ? al((size_t)n * 3 * sizeof(float)) : 0;
  hipStream_t st = s->stream;
  if (s->q_stage.n < total) {
    if (s->q_done_rec) HIP_TRY(hipEventSynchronize(s->q_done));
    if (int rc = s->q_stage.alloc(total)) return rc;
  }
  unsigned char* base = s->q_stage.p;
  // the staging buffer's last user was a query on this stream, or has been waited for
  if (s->q_done_rec && st != s->q_stream) HIP_TRY(hipStreamWaitEvent(st, s->q_done, 0));
  for (int k = 0; k < 4; ++k)
    if (in[k]) HIP_TRY(hipMemcpyAsync(base + off[k], in[k], in_bytes[k], hipMemcpyHostToDevice, st));
  Trace32Params q{};
  q.orig = in[0] ? (const float*)(base + off[0]) : nullptr;
  q.dir = in[1] ? (const float*)(base + off[1]) : nullptr;
  q.tnear = in[2] ? (const float*)(base + off[2]) : nullptr;
  q.xy = in[3] ? (const float*)(base + off[3]) : nullptr;
  q.hits = (Hit32*)(base + off[4]);
  q.normals = normals ? (float*)(base + off[5]) : nullptr;
  q.n = n;
  if (int rc = trace32_device(s, pick, q, flags, st, out)) return rc;
  HIP_TRY(hipMemcpyAsync(hits, base + off[4], (size_t)n * sizeof(rt_hit32), hipMemcpyDeviceToHost, st));
  if (normals)
    HIP_TRY(hipMemcpyAsync(normals, base + off[5], (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RT_OK;
}

}  // namespace

extern "C" int rt_trace_rays_f32_device(rt_scene* s, int64_t n, const float* d_orig, const float* d_dir,
                                        const float* d_tnear, uint32_t flags, rt_hit32* d_hits, float* d_normals,
                                        void* stream, rt_stats* out) {
  if (int rc = trace32_check(s, n, flags, d_hits, d_normals)) return rc;
  if (n > 0 && (!d_orig || !d_dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  Trace32Params q{};
  q.orig = d_orig;
  q.dir = d_dir;
  q.tnear = d_tnear;
  q.hits = (Hit32*)d_hits;
  q.normals = d_normals;
  q.n = n;
  return trace32_device(s, nullptr, q, flags, (hipStream_t)stream, out);
}

extern "C" int rt_trace_rays_f32(rt_scene* s, int64_t n, const float* orig, const float* dir, const float* tnear,
                                 uint32_t flags, rt_hit32* hits, float* normals, rt_stats* out) {
  if (int rc = trace32_check(s, n, flags, hits, normals)) return rc;
  if (n > 0 && (!orig || !dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  const size_t v3 = (size_t)n * 3 * sizeof(float);
  const void* const in[4] = {orig, dir, tnear, nullptr};
  const size_t bytes[4] = {v3, v3, (size_t)n * sizeof(float), 0};
  return trace32_host(s, nullptr, n, in, bytes, flags, hits, normals, out);
}

extern "C" int rt_pick_pixels_f32_device(rt_scene* s, const rt_options* o, int64_t n, const float* d_xy,
                                         uint32_t flags, rt_hit32* d_hits, float* d_normals, void* stream,
                                         rt_stats* out) {
  if (int rc = trace32_check(s, n, flags, d_hits, d_normals)) return rc;
  if (int rc = pick32_check(o)) return rc;
  if (n > 0 && !d_xy) return fail(RT_E_INVALID, "null pixel positions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  Trace32Params q{};
  q.xy = d_xy;
  q.hits = (Hit32*)d_hits;
  q.normals = d_normals;
  q.n = n;
  return trace32_device(s, o, q, flags, (hipStream_t)stream, out);
}

extern "C" int rt_pick_pixels_f32(rt_scene* s, const rt_options* o, int64_t n, const float* xy, uint32_t flags,
                                  rt_hit32* hits, float* normals, rt_stats* out) {
  if (int rc = trace32_check(s, n, flags, hits, normals)) return rc;
  if (int rc = pick32_check(o)) return rc;
  if (n > 0 && !xy) return fail(RT_E_INVALID, "null pixel positions");
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  const void* const in[4] = {nullptr, nullptr, nullptr, xy};
  const size_t bytes[4] = {0, 0, 0, (size_t)n * 2 * sizeof(float)};
  return trace32_host(s, o, n, in, bytes, flags, hits, normals, out);
}
