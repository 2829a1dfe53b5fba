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
#include "rt_stage.h"

namespace {

constexpr uint32_t kQueryFlags = RT_QUERY_ANY_HIT | RT_QUERY_SORT;

// What every hit query of either precision checks before it takes the scene's lock.
int query_check(const rt_scene* s, int64_t n, uint32_t flags, const void* hits, const void* normals) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (flags & ~kQueryFlags) return fail(RT_E_INVALID, "unknown query flags 0x%x", flags & ~kQueryFlags);
  if ((flags & RT_QUERY_ANY_HIT) && normals)
    return fail(RT_E_INVALID, "normals are not available with RT_QUERY_ANY_HIT");
  if (n > 0 && !hits) return fail(RT_E_INVALID, "null hits");
  if (n > INT32_MAX) return fail(RT_E_UNSUPPORTED, "%lld rays in one batch (at most 2^31 - 1)", (long long)n);
  return RT_OK;
}

// ... and a pick of `precision` (RT_FP64: rt_pick_pixels*, RT_FP32: rt_pick_pixels_f32*) besides
int pick_check(const rt_options* o, int32_t precision) {
  if (!o) return fail(RT_E_INVALID, "null options");
  if (o->width <= 0 || o->height <= 0 || o->width > 65536 || o->height > 65536)
    return fail(RT_E_INVALID, "bad image size %dx%d", o->width, o->height);
  if (o->precision == precision) return RT_OK;
  if (precision == RT_FP32)
    return fail(RT_E_INVALID, "rt_pick_pixels_f32 is float32 only (precision %d): rt_pick_pixels is the float64 pick",
                o->precision);
  return fail(o->precision == RT_FP32 ? RT_E_UNSUPPORTED : RT_E_INVALID, "ray queries are float64 only (precision %d)",
              o->precision);
}

// The frame of every query entry point, after its argument checks: a batch of
// no rays reports zero Stats; any other runs `body` with the scene's lock held
// and its device current.
template <class Body>
int query_call(rt_scene* s, int64_t n, rt_stats* out, Body body) {
  if (n == 0) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  return body();
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

// query_end's sums as the call's Stats. counted: the float64 kernels count
// their intersection tests; the float32 kernels leave the slot at 0 and the
// count is derived, as for a render: one test per object per trace call
// (renderer.nim:54-56). primary: the rays were camera rays (a pick's, a
// radiance query's), not a trace's — the kernels count the rays they traced
// in that slot either way.
rt_stats query_stats(const rt_scene* s, const unsigned long long* h, bool counted, bool primary) {
  const unsigned long long rays = h[STAT_PRIMARY] + h[STAT_SHADOW] + h[STAT_REFL];
  rt_stats r{};
  r.num_primary_rays = primary ? h[STAT_PRIMARY] : 0;
  r.num_intersection_tests = counted ? h[STAT_TESTS] : (unsigned long long)s->nobj * rays;
  r.num_intersection_hits = h[STAT_HITS];
  r.num_shadow_rays = h[STAT_SHADOW];
  r.num_reflection_rays = h[STAT_REFL];
  return r;
}

// The device body of every float64 hit query (the scene's lock held, its
// device current): q's ray, hit and normal pointers are device memory. pick:
// the image size of a pick (its width and height alone are read), nullptr for
// a trace.
int query_device(rt_scene* s, const rt_options* pick, QueryParams q, uint32_t flags, hipStream_t st, rt_stats* out) {
  RenderParams<double> p;
  fill_query(s, pick ? pick->width : 1, pick ? pick->height : 1, p);
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
  // camera rays are a pick's; the kernel counts the rays it traced
  if (out) *out = query_stats(s, h, true, q.xy != nullptr);
  return RT_OK;
}

// ---- radiance queries: checks and device bodies -----------------------------
// What the four radiance-query entry points check before they take the scene's
// lock. f32: rt_shade_rays_f32* (one output, rgb32), else rt_shade_rays* (rgb
// and / or rgb32). The float32 call names missing rays before a missing
// output and the wrong precision, the float64 call after them.
int shade_check(const rt_scene* s, const rt_options* o, int64_t n, int32_t group, uint32_t flags, bool f32,
                const void* orig, const void* dir, const void* rgb, const void* rgb32) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!o) return fail(RT_E_INVALID, "null options");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (flags & ~(uint32_t)RT_QUERY_SORT)
    return fail(RT_E_INVALID, "%s takes RT_QUERY_SORT only (flags 0x%x)", f32 ? "rt_shade_rays_f32" : "rt_shade_rays",
                flags);
  if (group < 1) return fail(RT_E_INVALID, "group %d (at least 1)", group);
  if (n % group) return fail(RT_E_INVALID, "%lld rays are not a whole number of groups of %d", (long long)n, group);
  const bool no_rays = n > 0 && (!orig || !dir);
  if (f32 && no_rays) return fail(RT_E_INVALID, "null ray origins or directions");
  if (n > 0 && !rgb && !rgb32) return fail(RT_E_INVALID, "%s", f32 ? "null rgb" : "null rgb and rgb32");
  if (f32 && o->precision != RT_FP32)
    return fail(RT_E_INVALID, "rt_shade_rays_f32 is float32 only (precision %d): rt_shade_rays is the float64 query",
                o->precision);
  if (!f32 && o->precision != RT_FP64)
    return fail(o->precision == RT_FP32 ? RT_E_UNSUPPORTED : RT_E_INVALID,
                "radiance queries are float64 only (precision %d)", o->precision);
  if (n > INT32_MAX) return fail(RT_E_UNSUPPORTED, "%lld rays in one batch (at most 2^31 - 1)", (long long)n);
  if (no_rays) return fail(RT_E_INVALID, "null ray origins or directions");
  return RT_OK;
}

// The device body of both forms of rt_shade_rays (the scene's lock held, its
// device current): q.orig / q.dir and the outputs are device memory.
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
  if (out) *out = query_stats(s, h, true, true);
  return RT_OK;
}

// The device body of both forms of rt_shade_rays_f32 (the scene's lock held,
// its device current): q.orig / q.dir and d_rgb are device memory.
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
  if (out) *out = query_stats(s, h, false, true);
  return RT_OK;
}

// ---- float32 ray queries and picks: the device body --------------------------
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
  if (out) *out = query_stats(s, h, false, pick != nullptr);  // camera rays are a pick's
  return RT_OK;
}

// ---- the host forms' staging (rt_stage.h) ------------------------------------
// A batch is copied into the scene's staging buffer, queried on the scene's
// own stream, and its answers copied back.

// The staging buffer with room for `total` bytes, `st` ordered after its last
// user: a query on this stream, or one that is waited for.
int stage_reserve(rt_scene* s, size_t total, hipStream_t st, unsigned char** base) {
  if (s->q_stage.n < total) {
    if (s->q_done_rec) HIP_TRY(hipEventSynchronize(s->q_done));
    if (int rc = s->q_stage.alloc(total)) return rc;
  }
  *base = s->q_stage.p;
  if (s->q_done_rec && st != s->q_stream) HIP_TRY(hipStreamWaitEvent(st, s->q_done, 0));
  return RT_OK;
}

// A host array of `count` T into its slot at `dst` (nullptr: absent, and
// *dev says so)
template <class T>
int stage_in(void* dst, const T* host, size_t count, hipStream_t st, const T** dev) {
  *dev = host ? (const T*)dst : nullptr;
  if (host) HIP_TRY(hipMemcpyAsync(dst, host, count * sizeof(T), hipMemcpyHostToDevice, st));
  return RT_OK;
}

// ... and `count` T of a slot back into the host array that wants them
template <class T>
int stage_out(T* host, const void* src, size_t count, hipStream_t st) {
  if (host) HIP_TRY(hipMemcpyAsync(host, src, count * sizeof(T), hipMemcpyDeviceToHost, st));
  return RT_OK;
}

// What a hit query's host form is made of in each precision
struct Hits64 {
  using Scalar = double;
  using Hit = rt_hit;
  using DevHit = QueryHit;
  using Params = QueryParams;
  static constexpr auto device = &query_device;
};
struct Hits32 {
  using Scalar = float;
  using Hit = rt_hit32;
  using DevHit = Hit32;
  using Params = Trace32Params;
  static constexpr auto device = &trace32_device;
};

// Host form of every hit query: orig / dir / tnear (a trace, pick = nullptr) or
// xy (a pick) are host arrays, nullptr where absent.
template <class K>
int query_host(rt_scene* s, const rt_options* pick, int64_t n, const typename K::Scalar* orig,
               const typename K::Scalar* dir, const typename K::Scalar* tnear, const typename K::Scalar* xy,
               uint32_t flags, typename K::Hit* hits, typename K::Scalar* normals, rt_stats* out) {
  using S = typename K::Scalar;
  static_assert(sizeof(typename K::Hit) == 16 && sizeof(typename K::DevHit) == 16, "hit_stage_layout's hits");
  const size_t N = (size_t)n;
  const StageLayout l = hit_stage_layout(N, sizeof(S), orig, dir, tnear, xy, normals);
  hipStream_t st = s->stream;
  unsigned char* base = nullptr;
  if (int rc = stage_reserve(s, l.total, st, &base)) return rc;
  typename K::Params q{};
  if (int rc = stage_in(base + l.off[0], orig, N * 3, st, &q.orig)) return rc;
  if (int rc = stage_in(base + l.off[1], dir, N * 3, st, &q.dir)) return rc;
  if (int rc = stage_in(base + l.off[2], tnear, N, st, &q.tnear)) return rc;
  if (int rc = stage_in(base + l.off[3], xy, N * 2, st, &q.xy)) return rc;
  q.hits = (typename K::DevHit*)(base + l.off[4]);
  q.normals = normals ? (S*)(base + l.off[5]) : nullptr;
  q.n = n;
  if (int rc = K::device(s, pick, q, flags, st, out)) return rc;
  if (int rc = stage_out(hits, q.hits, N, st)) return rc;
  if (int rc = stage_out(normals, q.normals, N * 3, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return RT_OK;
}

}  // namespace

static_assert(sizeof(rt_hit) == sizeof(QueryHit), "rt_hit layout");
static_assert(sizeof(rt_hit32) == sizeof(Hit32), "rt_hit32 layout");

// ---- ray queries and picks (rt_trace_rays* / rt_pick_pixels*, and their _f32 forms) ----
extern "C" int rt_trace_rays_device(rt_scene* s, int64_t n, const double* d_orig, const double* d_dir,
                                    const double* d_tnear, uint32_t flags, rt_hit* d_hits, double* d_normals,
                                    void* stream, rt_stats* out) {
  if (int rc = query_check(s, n, flags, d_hits, d_normals)) return rc;
  if (n > 0 && (!d_orig || !d_dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  return query_call(s, n, out, [&] {
    QueryParams q{};
    q.orig = d_orig;
    q.dir = d_dir;
    q.tnear = d_tnear;
    q.hits = (QueryHit*)d_hits;
    q.normals = d_normals;
    q.n = n;
    return query_device(s, nullptr, q, flags, (hipStream_t)stream, out);
  });
}

extern "C" int rt_trace_rays(rt_scene* s, int64_t n, const double* orig, const double* dir, const double* tnear,
                             uint32_t flags, rt_hit* hits, double* normals, rt_stats* out) {
  if (int rc = query_check(s, n, flags, hits, normals)) return rc;
  if (n > 0 && (!orig || !dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  return query_call(s, n, out, [&] {
    return query_host<Hits64>(s, nullptr, n, orig, dir, tnear, nullptr, flags, hits, normals, out);
  });
}

extern "C" int rt_pick_pixels_device(rt_scene* s, const rt_options* o, int64_t n, const double* d_xy, uint32_t flags,
                                     rt_hit* d_hits, double* d_normals, void* stream, rt_stats* out) {
  if (int rc = query_check(s, n, flags, d_hits, d_normals)) return rc;
  if (int rc = pick_check(o, RT_FP64)) return rc;
  if (n > 0 && !d_xy) return fail(RT_E_INVALID, "null pixel positions");
  return query_call(s, n, out, [&] {
    QueryParams q{};
    q.xy = d_xy;
    q.hits = (QueryHit*)d_hits;
    q.normals = d_normals;
    q.n = n;
    return query_device(s, o, q, flags, (hipStream_t)stream, out);
  });
}

extern "C" int rt_pick_pixels(rt_scene* s, const rt_options* o, int64_t n, const double* xy, uint32_t flags,
                              rt_hit* hits, double* normals, rt_stats* out) {
  if (int rc = query_check(s, n, flags, hits, normals)) return rc;
  if (int rc = pick_check(o, RT_FP64)) return rc;
  if (n > 0 && !xy) return fail(RT_E_INVALID, "null pixel positions");
  return query_call(s, n, out, [&] {
    return query_host<Hits64>(s, o, n, nullptr, nullptr, nullptr, xy, flags, hits, normals, out);
  });
}

extern "C" int rt_trace_rays_f32_device(rt_scene* s, int64_t n, const float* d_orig, const float* d_dir,
                                        const float* d_tnear, uint32_t flags, rt_hit32* d_hits, float* d_normals,
                                        void* stream, rt_stats* out) {
  if (int rc = query_check(s, n, flags, d_hits, d_normals)) return rc;
  if (n > 0 && (!d_orig || !d_dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  return query_call(s, n, out, [&] {
    Trace32Params q{};
    q.orig = d_orig;
    q.dir = d_dir;
    q.tnear = d_tnear;
    q.hits = (Hit32*)d_hits;
    q.normals = d_normals;
    q.n = n;
    return trace32_device(s, nullptr, q, flags, (hipStream_t)stream, out);
  });
}

extern "C" int rt_trace_rays_f32(rt_scene* s, int64_t n, const float* orig, const float* dir, const float* tnear,
                                 uint32_t flags, rt_hit32* hits, float* normals, rt_stats* out) {
  if (int rc = query_check(s, n, flags, hits, normals)) return rc;
  if (n > 0 && (!orig || !dir)) return fail(RT_E_INVALID, "null ray origins or directions");
  return query_call(s, n, out, [&] {
    return query_host<Hits32>(s, nullptr, n, orig, dir, tnear, nullptr, flags, hits, normals, out);
  });
}

extern "C" int rt_pick_pixels_f32_device(rt_scene* s, const rt_options* o, int64_t n, const float* d_xy,
                                         uint32_t flags, rt_hit32* d_hits, float* d_normals, void* stream,
                                         rt_stats* out) {
  if (int rc = query_check(s, n, flags, d_hits, d_normals)) return rc;
  if (int rc = pick_check(o, RT_FP32)) return rc;
  if (n > 0 && !d_xy) return fail(RT_E_INVALID, "null pixel positions");
  return query_call(s, n, out, [&] {
    Trace32Params q{};
    q.xy = d_xy;
    q.hits = (Hit32*)d_hits;
    q.normals = d_normals;
    q.n = n;
    return trace32_device(s, o, q, flags, (hipStream_t)stream, out);
  });
}

extern "C" int rt_pick_pixels_f32(rt_scene* s, const rt_options* o, int64_t n, const float* xy, uint32_t flags,
                                  rt_hit32* hits, float* normals, rt_stats* out) {
  if (int rc = query_check(s, n, flags, hits, normals)) return rc;
  if (int rc = pick_check(o, RT_FP32)) return rc;
  if (n > 0 && !xy) return fail(RT_E_INVALID, "null pixel positions");
  return query_call(s, n, out, [&] {
    return query_host<Hits32>(s, o, n, nullptr, nullptr, nullptr, xy, flags, hits, normals, out);
  });
}

// ---- radiance queries (rt_shade_rays* / rt_shade_rays_f32*) ------------------
extern "C" int rt_shade_rays_device(rt_scene* s, const rt_options* o, int64_t n, const double* d_orig,
                                    const double* d_dir, int32_t group, uint32_t flags, double* d_rgb, float* d_rgb32,
                                    void* stream, rt_stats* out) {
  if (int rc = shade_check(s, o, n, group, flags, false, d_orig, d_dir, d_rgb, d_rgb32)) return rc;
  return query_call(s, n, out, [&] {
    QueryParams q{};
    q.orig = d_orig;
    q.dir = d_dir;
    q.n = n;
    return shade_device(s, o, q, group, flags, d_rgb, d_rgb32, (hipStream_t)stream, out);
  });
}

extern "C" int rt_shade_rays(rt_scene* s, const rt_options* o, int64_t n, const double* orig, const double* dir,
                             int32_t group, uint32_t flags, double* rgb, float* rgb32, rt_stats* out) {
  if (int rc = shade_check(s, o, n, group, flags, false, orig, dir, rgb, rgb32)) return rc;
  return query_call(s, n, out, [&]() -> int {
    const size_t N = (size_t)n, ng = (size_t)(n / group);
    const StageLayout l = shade_stage_layout(N, (size_t)group, sizeof(double), rgb, rgb32);
    hipStream_t st = s->stream;
    unsigned char* base = nullptr;
    if (int rc = stage_reserve(s, l.total, st, &base)) return rc;
    QueryParams q{};
    if (int rc = stage_in(base + l.off[0], orig, N * 3, st, &q.orig)) return rc;
    if (int rc = stage_in(base + l.off[1], dir, N * 3, st, &q.dir)) return rc;
    q.n = n;
    double* d_rgb = rgb ? (double*)(base + l.off[2]) : nullptr;
    float* d_rgb32 = rgb32 ? (float*)(base + l.off[3]) : nullptr;
    if (int rc = shade_device(s, o, q, group, flags, d_rgb, d_rgb32, st, out)) return rc;
    if (int rc = stage_out(rgb, d_rgb, ng * 3, st)) return rc;
    if (int rc = stage_out(rgb32, d_rgb32, ng * 3, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
  });
}

extern "C" int rt_shade_rays_f32_device(rt_scene* s, const rt_options* o, int64_t n, const float* d_orig,
                                        const float* d_dir, int32_t group, uint32_t flags, float* d_rgb, void* stream,
                                        rt_stats* out) {
  if (int rc = shade_check(s, o, n, group, flags, true, d_orig, d_dir, nullptr, d_rgb)) return rc;
  return query_call(s, n, out, [&] {
    Shade32Params q{};
    q.orig = d_orig;
    q.dir = d_dir;
    q.n = n;
    return shade32_device(s, o, q, group, flags, d_rgb, (hipStream_t)stream, out);
  });
}

extern "C" int rt_shade_rays_f32(rt_scene* s, const rt_options* o, int64_t n, const float* orig, const float* dir,
                                 int32_t group, uint32_t flags, float* rgb, rt_stats* out) {
  if (int rc = shade_check(s, o, n, group, flags, true, orig, dir, nullptr, rgb)) return rc;
  return query_call(s, n, out, [&]() -> int {
    const size_t N = (size_t)n, ng = (size_t)(n / group);
    const StageLayout l = shade_stage_layout(N, (size_t)group, sizeof(float), false, true);
    hipStream_t st = s->stream;
    unsigned char* base = nullptr;
    if (int rc = stage_reserve(s, l.total, st, &base)) return rc;
    Shade32Params q{};
    if (int rc = stage_in(base + l.off[0], orig, N * 3, st, &q.orig)) return rc;
    if (int rc = stage_in(base + l.off[1], dir, N * 3, st, &q.dir)) return rc;
    q.n = n;
    float* d_rgb = (float*)(base + l.off[3]);
    if (int rc = shade32_device(s, o, q, group, flags, d_rgb, st, out)) return rc;
    if (int rc = stage_out(rgb, d_rgb, ng * 3, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
  });
}
