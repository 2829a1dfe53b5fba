// rt_hooks.cpp — the rtmi_test_* hooks (tests/, tools/; not part of
// include/rtmi.h): what the tests read of a scene's device state, and the
// host builders run for them on the scene's own data.
#include <cmath>
#include <cstring>

#include "rt_scene.h"

// Pixel-list slots per pixel, 2^lg (lg >= 0: used from the next call on; the
// buffers are re-allocated): a test forces lists past their slots (the
// pixels' camera rays then take the BVH). Returns the current lg (lg < 0:
// query only).
extern "C" int rtmi_test_slot_lg(rt_scene* s, int32_t lg) {
  if (!s || lg > 10) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  if (lg >= 0) s->fr.want_lg = s->fr2.want_lg = lg;
  return s->fr.slot_lg;
}

// Whether the last render call ran its build on the scene's build stream
// (pipelined, rt_scene::pipe), and the call's buffer set (0 / 1: which of the
// two it used; it alternates between pipelined calls).
extern "C" int rtmi_test_last_pipelined(rt_scene* s, int32_t* set) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  std::lock_guard<std::mutex> lk(s->mu);
  if (set) *set = s->fr.id;
  return s->pipe ? 1 : 0;
}

// The last render call's device-built camera-ray lists and pixel records
// (image-sized arrays; only the call's pixels are defined) as CSR: off:
// w*h + 1 (a pixel's true list length, overflowed ones included), ent: up to
// ent_cap entries (a pixel past its 2^lg slots contributes its first 2^lg
// entries and pads the rest with -1), info: w*h. Returns the entries
// copied, or a negative RT_E_* code.
extern "C" int64_t rtmi_test_frame_lists(rt_scene* s, int32_t* off, int32_t* ent, int64_t ent_cap, uint32_t* info) {
  if (!s || !off || !ent || !info) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  const rt_scene::Frame& f = s->fr;
  if (!f.slots.p || f.w == 0 || f.slot_lg < 0) return fail(RT_E_INVALID, "no per-call lists yet");
  const size_t npx = (size_t)f.w * (size_t)f.h;
  HIP_TRY(hipEventSynchronize(s->done));
  HIP_TRY(hipMemcpy(info, f.info.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<int32_t> slots(npx << f.slot_lg);
  HIP_TRY(hipMemcpy(slots.data(), f.slots.p, slots.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  const uint32_t K = 1u << f.slot_lg;
  int64_t n = 0;
  off[0] = 0;
  for (size_t p = 0; p < npx; ++p) {
    const uint32_t c = info[p] & kPixCount;
    for (uint32_t k = 0; k < c; ++k, ++n)
      if (n < ent_cap) ent[n] = k < K ? slots[(p << f.slot_lg) + k] : -1;
    off[p + 1] = (int32_t)n;
  }
  return std::min<int64_t>(n, ent_cap);
}

// The float32 kernel specialisation (SUB_* bits, rt_common.h) a render call
// with these options launches on this scene: f32_subset, as the launch reads it.
extern "C" int rtmi_test_f32_subset(rt_scene* s, const rt_options* o) {
  if (!s || !o) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  return (int)f32_subset(s, o);
}

// The specialisation of k_shade_rays_f32 a float32 radiance query
// (rt_shade_rays_f32*) launches on this scene: the scene's SUB_* bits without
// stochastic sampling, as shade32_device reads them.
extern "C" int rtmi_test_shade32_subset(rt_scene* s) {
  if (!s) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  return (int)(s->f32_subset & ~(unsigned)SUB_STOCHASTIC & 63u);
}

// The specialisation of k_trace_rays_f32 a float32 ray query or pick
// (rt_trace_rays_f32* / rt_pick_pixels_f32*) launches on this scene: the
// scene's geometry bits, as trace32_device reads them.
extern "C" int rtmi_test_trace32_subset(rt_scene* s) {
  if (!s) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  return (int)(s->f32_subset & 15u);
}

// Test hook: the LTri record (rt_common.h) of triangle v9 (v0, v1, v2 as 9
// doubles, mesh object space) for the shadow direction d (float64), as
// rt_scene_create builds it; out: 16 words.
extern "C" int rtmi_test_ltri(const double* v9, const double* d, int32_t face, void* out) {
  if (!v9 || !d || !out) return fail(RT_E_INVALID, "null argument");
  const double v[3][3] = {{v9[0], v9[1], v9[2]}, {v9[3], v9[4], v9[5]}, {v9[6], v9[7], v9[8]}};
  bg::make_ltri(v, d, face, (LTri*)out);
  return RT_OK;
}

// Test hook: the last call's pixel records (w*h words, rt_frame.h: list
// length | shadow skip bits << 24; only the call's pixels are defined).
extern "C" int rtmi_test_pixel_info(rt_scene* s, uint32_t* info) {
  if (!s || !info) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  const rt_scene::Frame& f = s->fr;
  if (!f.info.p || f.w == 0) return fail(RT_E_INVALID, "no per-call records yet");
  HIP_TRY(hipEventSynchronize(s->done));
  HIP_TRY(hipMemcpy(info, f.info.p, (size_t)f.w * (size_t)f.h * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RT_OK;
}

// Test hooks for the uniform-pixel proof (tests/test_uniform_cpu.py; no
// device): the FastParams camera words and the UniformCam of a one-plane call
// with this camera, image size, m x m grid and bias, formed by the functions
// a render call forms them with (fast_camera, uniform_cam). ty: the plane's
// world_to_object[13] and light_dirs: nl x 3 doubles, both rounded as
// fill_fast_records rounds them. cls: uniform_class of the pixels
// [x0, x1) x [y0, y1), row by row; cam10: cam_a, cam_b, cam_c, cam_d, c4,
// c7, c10, st, of, nroy.
static int uniform_hook_cam(const double* c2w, double fov, int32_t w, int32_t h, int32_t m, double ty, double bias,
                            const double* light_dirs, int32_t nl, bg::UniformCam& u) {
  if (!c2w || w <= 0 || h <= 0 || m <= 0 || nl < 0 || nl > 8 || (nl > 0 && !light_dirs))
    return fail(RT_E_INVALID, "bad argument");
  rt_options o;
  std::memset(&o, 0, sizeof o);
  o.width = w;
  o.height = h;
  o.aa_kind = RT_AA_GRID;
  o.grid_size = m;
  o.bias = bias;
  FastParams p;
  std::memset(&p, 0, sizeof p);
  fast_camera(c2w, fov, &o, p);
  p.nlight = nl;
  float vy[8];
  for (int l = 0; l < nl; ++l) vy[l] = (float)light_dirs[3 * l + 1];
  std::memset(&u, 0, sizeof u);
  uniform_cam((float)ty, vy, p, u);
  return RT_OK;
}

extern "C" int rtmi_test_uniform(const double* c2w, double fov, int32_t w, int32_t h, int32_t m, double ty,
                                 double bias, const double* light_dirs, int32_t nl, int32_t x0, int32_t y0, int32_t x1,
                                 int32_t y1, uint8_t* cls, int32_t* lit_ok, float* cam10) {
  bg::UniformCam u;
  if (int rc = uniform_hook_cam(c2w, fov, w, h, m, ty, bias, light_dirs, nl, u)) return rc;
  if (!cls || !lit_ok || !cam10 || x0 < 0 || y0 < 0 || x1 > w || y1 > h || x0 > x1 || y0 > y1)
    return fail(RT_E_INVALID, "bad argument");
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x) *cls++ = (uint8_t)bg::uniform_class(u, x, y);
  *lit_ok = u.lit_ok;
  const float c[10] = {u.cam_a, u.cam_b, u.cam_c, u.cam_d, u.c4, u.c7, u.c10, u.st, u.of, u.nroy};
  std::copy(c, c + 10, cam10);
  return RT_OK;
}

// Test hook for the mesh pixels' inset box (tests/test_mesh1_cpu.py; no
// device). box6: bg::inset_box of the float32 box lo / hi and the nl lights'
// FLight.v (in_lo, in_hi). Per case i of n, with the origin ro[3 i ..] in the
// mesh's frame and the reciprocals ni[3 i ..] given (so that the test can
// move them by an ulp, as v_rcp may): inside[i] = the kernel's inset_inside,
// gate[i] = rt_fast.h mesh_gate restated in float32 with fmaf where the
// kernel has an FMA (this unit is compiled without contraction).
extern "C" int rtmi_test_mesh1(const float* lo, const float* hi, const float* light_v, int32_t nl, float* box6,
                               int64_t n, const float* ro, const float* ni, uint8_t* inside, uint8_t* gate) {
  if (!lo || !hi || nl < 0 || (nl > 0 && !light_v) || !box6 || n < 0 || (n > 0 && (!ro || !ni || !inside || !gate)))
    return fail(RT_E_INVALID, "bad argument");
  bg::InsetBox b;
  bg::inset_box(lo, hi, light_v, nl, b);
  std::copy(b.lo, b.lo + 3, box6);
  std::copy(b.hi, b.hi + 3, box6 + 3);
  for (int64_t i = 0; i < n; ++i) {
    const float* o = ro + 3 * i;
    const float* r = ni + 3 * i;
    inside[i] = inset_inside(b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2], o[0], o[1], o[2]) ? 1 : 0;
    float a[3], c[3];
    for (int k = 0; k < 3; ++k) {
      const float oi = o[k] * r[k];
      a[k] = fmaf(lo[k], r[k], -oi);
      c[k] = fmaf(hi[k], r[k], -oi);
    }
    const float gmin = fmaxf(fmaxf(fminf(a[0], c[0]), fminf(a[1], c[1])), fminf(a[2], c[2]));
    const float gmax = fminf(fminf(fmaxf(a[0], c[0]), fmaxf(a[1], c[1])), fmaxf(a[2], c[2])) * 1.00000024f;
    gate[i] = gmin <= gmax && gmin >= 0.0f ? 1 : 0;
  }
  return RT_OK;
}

// The one-plane kernel's cx (m per pixel column), cy (m per pixel row) and N
// (m x m per pixel: pixels row by row, then the sample row j, then the sample
// column i) for every sample of the same rectangle: the expressions listed
// above rt_bins_geom.h uniform_class, with fmaf where the kernel has an fma
// (this file is compiled without contraction).
extern "C" int rtmi_test_uniform_samples(const double* c2w, double fov, int32_t w, int32_t h, int32_t m, double ty,
                                         double bias, int32_t x0, int32_t y0, int32_t x1, int32_t y1, float* cx,
                                         float* cy, float* n) {
  bg::UniformCam u;
  if (int rc = uniform_hook_cam(c2w, fov, w, h, m, ty, bias, nullptr, 0, u)) return rc;
  if (!cx || !cy || !n || x0 < 0 || y0 < 0 || x1 > w || y1 > h || x0 > x1 || y0 > y1)
    return fail(RT_E_INVALID, "bad argument");
  for (int x = x0; x < x1; ++x)
    for (int i = 0; i < m; ++i) {
      const float px = (float)x + fmaf((float)i, u.st, u.of);
      cx[(size_t)(x - x0) * m + i] = (px - u.cam_b) * u.cam_a;
    }
  for (int y = y0; y < y1; ++y)
    for (int j = 0; j < m; ++j) {
      const float py = (float)y + fmaf((float)j, u.st, u.of);
      cy[(size_t)(y - y0) * m + j] = (u.cam_d - py) * u.cam_c;
    }
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x)
      for (int j = 0; j < m; ++j) {
        const float cyj = cy[(size_t)(y - y0) * m + j];
        for (int i = 0; i < m; ++i)
          *n++ = fmaf(cyj, u.c7, fmaf(cx[(size_t)(x - x0) * m + i], u.c4, -u.c10));
      }
  return RT_OK;
}

// The host builders (rt_bins.cpp build_pixel_bins + build_shadow_skips) on
// this scene's faces, camera and light grids: the lists and records a render
// call of this image size and bias must build on the device. off: w*h + 1,
// info: w*h. Returns the number of entries (those past ent_cap not copied),
// -1 when the host builder declines the camera.
extern "C" int64_t rtmi_test_host_lists(rt_scene* s, int32_t w, int32_t h, double bias, int32_t* off, int32_t* ent,
                                        int64_t ent_cap, uint32_t* info) {
  if (!s || !off || !ent || !info || w <= 0 || h <= 0) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->binnable) return -1;
  PixelBinsHost hb;
  const char* why = "";
  if (refresh_bin_tris(s) != RT_OK) return -1;
  if (!build_pixel_bins(s->bin_tris, s->mesh_o2w, s->mesh_w2o, s->c2w, s->fov, w, h, &hb, &why)) return -1;
  const size_t npx = (size_t)w * (size_t)h;
  refresh_host_lists(s);  // (after a relight the prefix sums are on the device only)
  std::vector<uint32_t> sk;
  if (!(s->skippable && build_shadow_skips(hb.off, s->skip_planes, s->mesh_w2o, s->grid_occ, s->c2w, s->fov, w, h,
                                           bias, &sk, &why)))
    sk.assign((npx + 3) / 4, 0u);
  std::copy(hb.off.begin(), hb.off.end(), off);
  const int64_t total = hb.off.back();
  std::copy(hb.ent.begin(), hb.ent.begin() + std::min<int64_t>(total, std::max<int64_t>(0, ent_cap)), ent);
  for (size_t k = 0; k < npx; ++k) {
    const uint32_t n = (uint32_t)(hb.off[k + 1] - hb.off[k]);
    info[k] = std::min<uint32_t>(n, kPixCount) | (sk[k >> 2] >> (8 * (k & 3)) & 0xffu) << 24;
  }
  return total;
}

// rt_scene_set_lights' device-built arrays against the host path (the one
// rt_scene_create takes) on the scene's faces and current lights, byte for
// byte. out[k]: differing elements (a length difference counts each missing
// element) of 0 the grid headers and the scene's light flags, 1 off, 2 ent
// (padding included), 3 the occupancy prefix sums, 4 lrec, 5 grec, 6 the
// FLight records, 7 the DevLight<double> records.
namespace {
template <class T>
int64_t diff_dev(const DevBuf<T>& a, const DevBuf<T>& b) {
  std::vector<unsigned char> ha(a.bytes()), hb(b.bytes());
  if (a.p && !ha.empty() && hipMemcpy(ha.data(), a.p, ha.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (b.p && !hb.empty() && hipMemcpy(hb.data(), b.p, hb.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const size_t n = std::min(a.n, b.n);
  int64_t bad = (int64_t)(std::max(a.n, b.n) - n);
  for (size_t k = 0; k < n; ++k) bad += std::memcmp(&ha[k * sizeof(T)], &hb[k * sizeof(T)], sizeof(T)) != 0 ? 1 : 0;
  return bad;
}
}  // namespace

extern "C" int rtmi_test_relight_diff(rt_scene* s, int64_t out[8]) {
  if (!s || !out) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  HIP_TRY(hipDeviceSynchronize());
  LightState h;
  int rc = build_lights(s, s->light_desc.data(), s->nlight, false, &h);
  if (rc == RT_OK) {
    out[0] = diff_dev(s->grids, h.grids);
    out[0] += (s->has_grids != h.has_grids) + (s->lrec_mask != h.lrec_mask) + (s->skippable != h.skippable) +
              (s->lean64_plane != h.lean64_plane) + (s->has_point_light != h.has_point_light) +
              (std::memcmp(s->sat_off, h.sat_off, sizeof h.sat_off) != 0) + (s->lrec_ntri != h.lrec_ntri) +
              (s->has_obj_grids != h.has_obj_grids) + (s->grid_nent != h.grid_nent);
    for (size_t li = 0; li < h.grid_occ.size() && li < s->grid_occ.size(); ++li)
      out[0] += std::memcmp(&s->grid_occ[li].g, &h.grid_occ[li].g, sizeof(LightGrid)) != 0;
    out[1] = diff_dev(s->grid_off, h.grid_off);
    out[2] = diff_dev(s->grid_ent, h.grid_ent);
    out[3] = diff_dev(s->sat_dev, h.sat_dev);
    out[4] = diff_dev(s->lrec, h.lrec);
    out[5] = diff_dev(s->grec, h.grec);
    out[6] = diff_dev(s->f32.lights, h.f32_lights);
    out[7] = diff_dev(s->f64.lights, h.f64_lights);
    for (int k = 0; k < 8; ++k)
      if (out[k] < 0) rc = fail(RT_E_DEVICE, "reading the light arrays back failed");
  }
  return rc;
}

// enable: time the device builder's passes from the next relight on (events
// between them). ms (may be null): the passes of the last relight, summed
// over its lights (faces, count, scan, records, fill + order, prefix sums);
// zeros when it was not timed (tools/relight_bench.py).
extern "C" int rtmi_test_relight_passes(rt_scene* s, int32_t enable, float ms[6]) {
  if (!s) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  if (ms) std::copy(s->relight_ms, s->relight_ms + 6, ms);
  s->relight_timed = enable != 0;
  return RT_OK;
}

// ---- object updates (rt_scene_set_objects) --------------------------------

// What rt_scene_create forms from the scene's current objects (obj_desc), its
// meshes' boxes and its lights, on the host, against the device's arrays,
// byte for byte. out[k]: differing bytes (a length difference counts each
// missing byte) of 0 f64.objects, 1 f32.objs, 2 f32.objx, 3 objbox_dev, 4 the
// object-grid headers, 5 the object-grid masks, 6 off_grid, 7 the scalar
// state (f32_subset's object bits, any_reflective, lean64_plane, skippable,
// h_obj_ty, obj_meta, the host copy of f32.objs, the mesh object's transform).
namespace {
template <class T>
int64_t diff_host(const DevBuf<T>& a, const std::vector<T>& want, bool present) {
  const size_t nb = present ? want.size() * sizeof(T) : 0;
  const size_t na = a.p ? a.bytes() : 0;
  // (an empty upload still holds one element: DevBuf::alloc)
  const size_t have = present && want.empty() ? 0 : na;
  std::vector<unsigned char> ha(have);
  if (have && hipMemcpy(ha.data(), a.p, have, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const unsigned char* hb = reinterpret_cast<const unsigned char*>(want.data());
  const size_t n = std::min(have, nb);
  int64_t bad = (int64_t)(std::max(have, nb) - n);
  for (size_t k = 0; k < n; ++k) bad += ha[k] != hb[k] ? 1 : 0;
  return bad;
}
}  // namespace

extern "C" int rtmi_test_objects_diff(rt_scene* s, int64_t out[8]) {
  if (!s || !out) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  HIP_TRY(hipDeviceSynchronize());
  std::fill(out, out + 8, 0);
  const rt_object_desc* objs = s->obj_desc.data();
  const int32_t n = s->nobj;
  std::vector<DevObject<double>> o64;
  std::vector<FObj> fo;
  std::vector<FObjX> fx;
  fill_objects<double>(objs, n, o64);
  fill_fast_objects(objs, n, s->h_dm32, fo, fx);
  out[0] = diff_host(s->f64.objects, o64, true);
  out[1] = diff_host(s->f32.objs, fo, true);
  out[2] = diff_host(s->f32.objx, fx, true);
  std::vector<ObjBox> boxes;
  std::vector<DevObjBox> ob;
  const bool bins = n >= 4 && n <= 64;
  if (bins) {
    fill_obj_boxes(objs, n, s->h_dm64, boxes);
    dev_obj_boxes(boxes, ob);
  }
  out[3] = diff_host(s->objbox_dev, ob, bins) + (s->objbins != bins);
  // the object grids by the host builder, as build_lights(device = false) uploads them
  std::vector<LightGrid> gh((size_t)std::max(1, s->nlight), LightGrid{});
  std::vector<unsigned long long> gm;
  unsigned long long off_grid = 0;
  bool any = false;
  for (int li = 0; bins && li < s->nlight; ++li) {
    if (s->light_desc[(size_t)li].type == RT_POINT_LIGHT) continue;
    ObjGridHost og;
    const char* why = "";
    if (!build_object_light_grid(boxes, s->light_desc[(size_t)li].dir, &og, &why)) continue;
    if ((int64_t)gm.size() + (int64_t)og.masks.size() > INT32_MAX) break;
    og.g.off_base = (int32_t)gm.size();
    gm.insert(gm.end(), og.masks.begin(), og.masks.end());
    gh[(size_t)li] = og.g;
    off_grid = og.off_grid;
    any = true;
  }
  out[4] = diff_host(s->obj_grids, gh, any) + (s->has_obj_grids != any);
  out[5] = diff_host(s->obj_grid_mask, gm, any);
  for (int b = 0; b < 64; ++b) out[6] += ((s->obj_off_grid ^ off_grid) >> b) & 1ull;
  // the scalar state
  bool refl = false;
  const unsigned from_objects = (unsigned)SUB_XF_GENERAL | (unsigned)SUB_REFLECT | (unsigned)SUB_SPHERE |
                                (unsigned)SUB_BOX | (unsigned)SUB_MESH;
  const unsigned sub = object_subset(objs, n, &refl);
  out[7] += (s->f32_subset & from_objects) != sub;
  out[7] += s->any_reflective != refl;
  std::vector<rt_scene::ObjMeta> meta;
  fill_obj_meta(objs, n, meta);
  out[7] += meta.size() != s->obj_meta.size();
  for (size_t i = 0; i < meta.size() && i < s->obj_meta.size(); ++i)
    out[7] += std::memcmp(&meta[i], &s->obj_meta[i], sizeof meta[i]) != 0;
  out[7] += fo.size() != s->h_fo.size() || s->h_obj_ty.size() != fo.size();
  for (size_t i = 0; i < fo.size() && i < s->h_fo.size() && i < s->h_obj_ty.size(); ++i)
    out[7] += (std::memcmp(&fo[i], &s->h_fo[i], sizeof(FObj)) != 0) +
              (std::memcmp(&fo[i].t[1], &s->h_obj_ty[i], sizeof(float)) != 0);
  if (s->shadow_mesh >= 0)
    out[7] += (std::memcmp(s->mesh_o2w, objs[s->shadow_mesh].object_to_world, sizeof s->mesh_o2w) != 0) +
              (std::memcmp(s->mesh_w2o, objs[s->shadow_mesh].world_to_object, sizeof s->mesh_w2o) != 0);
  {  // lean64_plane and skippable, as build_lights derives them from obj_meta
    bool skippable = s->has_grids;
    for (int i = 0; skippable && i < n; ++i) skippable = i == s->shadow_mesh || objs[i].type == RT_PLANE;
    int32_t lean = -1;
    if (skippable && n == 2 && s->nlight >= 1 && s->nlight <= 8) {
      const int pl = 1 - s->shadow_mesh;
      bool ok = objs[pl].type == RT_PLANE && !(objs[pl].reflection > 0.0);
      for (int li = 0; li < s->nlight; ++li) ok = ok && s->light_desc[(size_t)li].type != RT_POINT_LIGHT;
      if (ok) lean = pl;
    }
    out[7] += (s->skippable != skippable) + (s->lean64_plane != lean);
    if (s->skippable && skippable) {
      size_t k = 0;
      for (int i = 0; i < n; ++i) {
        if (i == s->shadow_mesh) continue;
        out[7] += k >= s->skip_planes.size() ||
                  std::memcmp(s->skip_planes[k].o2w, objs[i].object_to_world, sizeof(double) * 16) != 0 ||
                  std::memcmp(s->skip_planes[k].w2o, objs[i].world_to_object, sizeof(double) * 16) != 0;
        ++k;
      }
    }
  }
  for (int k = 0; k < 8; ++k)
    if (out[k] < 0) return fail(RT_E_DEVICE, "reading the object arrays back failed");
  return RT_OK;
}

// The scene's object light grids as they lie on the device: headers (one
// 64-byte LightGrid per light, up to hdr_cap of them; gu == 0: none) and
// masks (up to mask_cap), off_grid. Returns the number of masks (0: no object
// grids), or a negative RT_E_* code.
extern "C" int64_t rtmi_test_object_grids(rt_scene* s, void* headers, int64_t hdr_cap, unsigned long long* masks,
                                          int64_t mask_cap, unsigned long long* off_grid) {
  if (!s || !headers || !masks || !off_grid) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  HIP_TRY(hipDeviceSynchronize());
  *off_grid = s->obj_off_grid;
  if (!s->has_obj_grids) return 0;
  const size_t nh = std::min<size_t>((size_t)std::max<int64_t>(0, hdr_cap), s->obj_grids.n);
  const size_t nm = std::min<size_t>((size_t)std::max<int64_t>(0, mask_cap), s->obj_grid_mask.n);
  if (nh) HIP_TRY(hipMemcpy(headers, s->obj_grids.p, nh * sizeof(LightGrid), hipMemcpyDeviceToHost));
  if (nm) HIP_TRY(hipMemcpy(masks, s->obj_grid_mask.p, nm * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return (int64_t)s->obj_grid_mask.n;
}

// host != 0: from the next device-path rebuild on (rt_scene_set_objects /
// _set_lights / _set_mesh_vertices) the object light grids are built by the
// host builder; 0: by the device builder (the default); < 0: query only. ms
// (may be null): wall time of the last rebuild's object-grid pass
// (tools/object_update_bench.py).
extern "C" int rtmi_test_objgrid_pass(rt_scene* s, int32_t host, double* ms) {
  if (!s) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  if (ms) *ms = s->objgrid_ms;
  if (host >= 0) s->objgrid_host = host != 0;
  return RT_OK;
}

// ---- mesh updates (rt_scene_set_mesh_vertices) ----------------------------

namespace {

struct AncBox {
  float lo[3], hi[3];
};

// faces below `node` whose float64 bounds, inflated, leave one of `anc`
int64_t uncontained(const BvhResult& r, const double* v, const int32_t* f, double inflate, int32_t node,
                    std::vector<AncBox>& anc) {
  int64_t bad = 0;
  const BvhNode& nd = r.nodes[(size_t)node];
  for (int slot = 0; slot < 2; ++slot) {
    const int32_t c = slot ? nd.c1 : nd.c0, n = slot ? nd.n1 : nd.n0;
    AncBox a;
    for (int k = 0; k < 3; ++k) {
      a.lo[k] = slot ? nd.lo1[k] : nd.lo0[k];
      a.hi[k] = slot ? nd.hi1[k] : nd.hi0[k];
    }
    anc.push_back(a);
    if (n == 0) {
      if (c > 0) bad += uncontained(r, v, f, inflate, c, anc);
    } else {
      for (int32_t j = c; j < c + n; ++j) {
        const int32_t* fi = &f[3 * (size_t)r.order[(size_t)j]];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
          double lo = INFINITY, hi = -INFINITY;
          for (int q = 0; q < 3; ++q) {
            lo = std::min(lo, v[3 * (size_t)fi[q] + k]);
            hi = std::max(hi, v[3 * (size_t)fi[q] + k]);
          }
          for (const AncBox& b : anc) ok = ok && (double)b.lo[k] <= lo - inflate && (double)b.hi[k] >= hi + inflate;
        }
        bad += ok ? 0 : 1;
      }
    }
    anc.pop_back();
  }
  return bad;
}

}  // namespace

// CPU only: a tree built by the host SAH builder on vertices A, refitted
// (refit_bvh) to vertices B. out[0]: validate_bvh passes (1 / 0); out[1]: the
// faces whose float64 bounds, inflated by B's margin, are not inside every
// ancestor's child box; out[2]: the node bytes that differ from the tree built
// on A (0 when B == A). RT_E_INVALID when the build or the refit declines.
extern "C" int rtmi_test_refit_host(const double* va, const double* vb, int64_t nv, const int32_t* faces, int64_t nf,
                                    int64_t out[3]) {
  if (!va || !vb || !faces || !out || nv <= 0 || nf <= 0) return fail(RT_E_INVALID, "bad argument");
  for (int64_t k = 0; k < 3 * nf; ++k)
    if (faces[k] < 0 || faces[k] >= nv) return fail(RT_E_INVALID, "face index out of range");
  BvhResult built;
  const char* err = "";
  BvhBuildParams prm;
  if (!build_bvh(va, faces, nf, prm, &built, &err)) return fail(RT_E_INVALID, "%s", err);
  BvhResult r = built;
  double inflate = 0.0;
  if (!refit_bvh(vb, faces, nf, &r, &err) || !bvh_margin(vb, faces, nf, &inflate)) return fail(RT_E_INVALID, "%s", err);
  out[0] = validate_bvh(r, nf, &err) ? 1 : 0;
  std::vector<AncBox> anc;
  out[1] = uncontained(r, vb, faces, inflate, 0, anc);
  out[2] = 0;
  const unsigned char* pa = reinterpret_cast<const unsigned char*>(built.nodes.data());
  const unsigned char* pb = reinterpret_cast<const unsigned char*>(r.nodes.data());
  for (size_t k = 0; k < built.nodes.size() * sizeof(BvhNode); ++k) out[2] += pa[k] != pb[k] ? 1 : 0;
  return RT_OK;
}

namespace {

template <class T>
bool download(const T* p, size_t n, std::vector<T>& h) {
  h.resize(n);
  return n == 0 || hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}

template <class T>
int64_t diff_bytes(const T& a, const T& b) {
  return std::memcmp(&a, &b, sizeof(T)) != 0 ? 1 : 0;
}

// equal bytes, or both NaN (a degenerate face's 0/0 normal: its sign bit
// differs between the host and the device, and nothing reads it)
template <class T>
int64_t diff_num(T a, T b) {
  return std::memcmp(&a, &b, sizeof(T)) != 0 && !(a != a && b != b) ? 1 : 0;
}

uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t k = 0; k < n; ++k) h = (h ^ b[k]) * 1099511628211ull;
  return h;
}

// One mesh's nodes of the scene's host copy (h_nodes) as its builder returned
// them: child and face references relative to the mesh.
BvhResult mesh_tree(const rt_scene* s, const rt_scene::MeshKeep& keep, const std::vector<int32_t>& order) {
  BvhResult r;
  r.order = order;
  r.nodes.assign(s->h_nodes.begin() + keep.node_base, s->h_nodes.begin() + keep.node_base + keep.node_count);
  for (BvhNode& nd : r.nodes) {
    if (nd.n0 == 0 && nd.c0 >= 0) nd.c0 -= keep.node_base;
    if (nd.n1 == 0 && nd.c1 >= 0) nd.c1 -= keep.node_base;
    if (nd.n0 > 0) nd.c0 -= (int32_t)keep.tri_base;
    if (nd.n1 > 0) nd.c1 -= (int32_t)keep.tri_base;
  }
  return r;
}

// refit_bvh of the topology `topo` (mesh_tree) on the vertices v against the
// boxes of three copies of the mesh's nodes: topo itself (host_boxes), the
// float64 kernels' node array (boxes64) and the float32 tree (boxes32), 48
// box bytes per node; children: the child references and counts of the two
// device copies against h_nodes. The counters are added to.
int refit_diff(const rt_scene* s, const rt_scene::MeshKeep& keep, const BvhResult& topo, const std::vector<double>& v,
               const std::vector<int32_t>& f, const std::vector<BvhNode>& nodes, const std::vector<BvhNode>& tree,
               int64_t* host_boxes, int64_t* boxes64, int64_t* boxes32, int64_t* children) {
  BvhResult r = topo;
  const char* err = "";
  if (!refit_bvh(v.data(), f.data(), keep.nf, &r, &err)) return fail(RT_E_INVALID, "%s", err);
  const int64_t nnodes = s->num_nodes;
  const int32_t kB = (int32_t)sizeof(BvhNode);
  for (int32_t k = 0; k < keep.node_count; ++k) {
    const BvhNode& want = r.nodes[(size_t)k];
    const BvhNode& topo_n = s->h_nodes[(size_t)(keep.node_base + k)];
    const BvhNode& a = nodes[(size_t)(keep.node_base + k)];
    const BvhNode& b = tree[(size_t)(keep.node_base + k)];
    *host_boxes += std::memcmp(topo_n.lo0, want.lo0, 12 * sizeof(float)) != 0 ? 1 : 0;
    *boxes64 += std::memcmp(a.lo0, want.lo0, 12 * sizeof(float)) != 0 ? 1 : 0;
    *boxes32 += std::memcmp(b.lo0, want.lo0, 12 * sizeof(float)) != 0 ? 1 : 0;
    *children += (a.c0 != topo_n.c0) + (a.c1 != topo_n.c1) + (a.n0 != topo_n.n0) + (a.n1 != topo_n.n1);
    *children += (b.c0 != (topo_n.n0 > 0 ? (int32_t)nnodes + topo_n.c0 : topo_n.c0) * kB) +
                 (b.c1 != (topo_n.n1 > 0 ? (int32_t)nnodes + topo_n.c1 : topo_n.c1) * kB) + (b.n0 != topo_n.n0) +
                 (b.n1 != topo_n.n1);
  }
  return RT_OK;
}

}  // namespace

// The host create path on the scene's current vertices (records, normals,
// calcAABB, object boxes, refit_bvh on the scene's topology) against the
// device-resident arrays, byte for byte (normals: any NaN equals any NaN).
// out[k]: differing elements of 0 TriFast, 1 TriF64, 2 the float32 normals,
// 3 the float64 normals, 4 bin_dev, 5 the float64 kernels' node boxes, 6 the
// float32 tree's node boxes, 7 child references and counts (both trees),
// 8 DevMesh<float> (host only: the source of FMesh / FObj), 9 DevMesh<double>,
// 10 FMesh, 11 FObj, 12 objbox_dev, 13 the bins' mesh box; 14, 15: zero.
extern "C" int rtmi_test_mesh_update_diff(rt_scene* s, int64_t out[16]) {
  if (!s || !out) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  HIP_TRY(hipDeviceSynchronize());
  std::fill(out, out + 16, 0);
  const int64_t nnodes = s->num_nodes, ntri = s->num_triangles;
  std::vector<BvhNode> tree, nodes;
  std::vector<TriF64> tris;
  std::vector<float> n32;
  std::vector<double> n64;
  std::vector<DevBinTri> bins;
  if (!download(s->f32.tree.p, (size_t)(nnodes + ntri), tree) || !download(s->nodes.p, (size_t)nnodes, nodes) ||
      !download(s->f64.tris.p, (size_t)ntri, tris) || !download(s->f32.normals.p, (size_t)ntri * 3, n32) ||
      !download(s->f64.normals.p, (size_t)ntri * 3, n64) ||
      !download(s->bin_dev.p, s->binnable ? s->bin_tris.size() : 0, bins))
    return fail(RT_E_DEVICE, "reading the mesh arrays back failed");
  const TriFast* fast = reinterpret_cast<const TriFast*>(tree.data() + nnodes);
  std::vector<DevMesh<float>> dm32(s->h_dm32);
  std::vector<DevMesh<double>> dm64(s->h_dm64);
  std::vector<FMesh> fm(s->h_fm);
  std::vector<FObj> fo(s->h_fo);
  std::vector<ObjBox> boxes(s->obj_boxes);
  const int32_t bin_mesh = s->shadow_mesh >= 0 && s->binnable ? s->obj_meta[(size_t)s->shadow_mesh].mesh : -1;
  for (int m = 0; m < s->nmesh; ++m) {
    const rt_scene::MeshKeep& keep = s->mesh_keep[(size_t)m];
    std::vector<double> v;
    std::vector<int32_t> f, order;
    if (!download(keep.verts.p, (size_t)keep.nv * 3, v) || !download(keep.faces.p, (size_t)keep.nf * 3, f) ||
        !download(keep.order.p, (size_t)keep.nf, order))
      return fail(RT_E_DEVICE, "reading the mesh arrays back failed");
    // calcAABB and the records that hold it
    double bb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < keep.nv; ++i)
      for (int k = 0; k < 3; ++k) {
        const double x = v[3 * (size_t)i + k];
        if (x < bb[k]) bb[k] = x;
        if (x > bb[3 + k]) bb[3 + k] = x;
      }
    for (int k = 0; k < 3; ++k) {
      dm32[(size_t)m].lo[k] = (float)bb[k];
      dm32[(size_t)m].hi[k] = (float)bb[3 + k];
      dm64[(size_t)m].lo[k] = bb[k];
      dm64[(size_t)m].hi[k] = bb[3 + k];
      fm[(size_t)m].lo[k] = dm32[(size_t)m].lo[k];
      fm[(size_t)m].hi[k] = dm32[(size_t)m].hi[k];
    }
    for (size_t i = 0; i < s->obj_meta.size(); ++i) {
      if (s->obj_meta[i].mesh != m) continue;
      for (int k = 0; k < 3; ++k) {
        fo[i].lo[k] = dm32[(size_t)m].lo[k];
        fo[i].hi[k] = dm32[(size_t)m].hi[k];
      }
      if (s->objbins) {
        boxes[i] = ObjBox{};
        world_obj_box(RT_MESH, s->obj_meta[i].w2o, bb, bb + 3, &boxes[i]);
      }
    }
    if (m == bin_mesh)
      for (int k = 0; k < 3; ++k) out[13] += diff_bytes(s->mesh_lo[k], bb[k]) + diff_bytes(s->mesh_hi[k], bb[3 + k]);
    // records and normals in leaf order (k_pack's and rt_scene_create's operations)
    for (int64_t i = 0; i < keep.nf; ++i) {
      const int32_t face = order[(size_t)i];
      const int32_t* fi = &f[3 * (size_t)face];
      const double* v0 = &v[3 * (size_t)fi[0]];
      const double* v1 = &v[3 * (size_t)fi[1]];
      const double* v2 = &v[3 * (size_t)fi[2]];
      double e1[3], e2[3];
      for (int k = 0; k < 3; ++k) {
        e1[k] = v1[k] - v0[k];
        e2[k] = v2[k] - v0[k];
      }
      const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                           e1[0] * e2[1] - e1[1] * e2[0]};
      TriFast t;
      TriF64 d;
      std::memset(&t, 0, sizeof t);
      std::memset(&d, 0, sizeof d);
      for (int k = 0; k < 3; ++k) {
        t.v0[k] = (float)v0[k];
        t.e2[k] = (float)e2[k];
        t.e1n[k] = (float)-e1[k];
        t.nn[k] = (float)-n[k];
        d.v0[k] = v0[k];
        d.e1[k] = e1[k];
        d.e2[k] = e2[k];
      }
      t.id = face;
      d.id = face;
      out[0] += diff_bytes(fast[keep.tri_base + i], t);
      out[1] += diff_bytes(tris[(size_t)(keep.tri_base + i)], d);
      if (m == bin_mesh) {
        DevBinTri b;
        std::memset(&b, 0, sizeof b);
        for (int q = 0; q < 3; ++q)
          for (int k = 0; k < 3; ++k) b.v[q][k] = v[3 * (size_t)fi[q] + k];
        b.rec = (int32_t)((nnodes + keep.tri_base + i) * (int64_t)sizeof(TriFast));
        b.face = face;
        out[4] += diff_bytes(bins[(size_t)i], b);
      }
    }
    for (int64_t fidx = 0; fidx < keep.nf; ++fidx) {
      const size_t at = 3 * (size_t)(keep.tri_base + fidx);
      double nr[3];
      if (keep.normals_given) {  // the caller's values are what the float64 array holds
        for (int k = 0; k < 3; ++k) nr[k] = n64[at + k];
      } else {
        const double* p0 = &v[3 * (size_t)f[3 * fidx + 0]];
        const double* p1 = &v[3 * (size_t)f[3 * fidx + 1]];
        const double* p2 = &v[3 * (size_t)f[3 * fidx + 2]];
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        double dd = 0.0;
        dd = dd + cx * cx;
        dd = dd + cy * cy;
        dd = dd + cz * cz;
        const double len = std::sqrt(dd);
        nr[0] = cx / len;
        nr[1] = cy / len;
        nr[2] = cz / len;
      }
      for (int k = 0; k < 3; ++k) {
        out[3] += diff_num(n64[at + k], nr[k]);
        out[2] += diff_num(n32[at + k], (float)nr[k]);
      }
    }
    // the host refit of this mesh's nodes as created
    if (keep.node_count > 0) {
      const BvhResult r = mesh_tree(s, keep, order);
      int64_t host_boxes = 0;
      if (int rc = refit_diff(s, keep, r, v, f, nodes, tree, &host_boxes, &out[5], &out[6], &out[7]))
        return fail(rc, "mesh %d: %s", m, rt_last_error());
    }
  }
  std::vector<DevMesh<double>> d_dm64;
  std::vector<FMesh> d_fm;
  std::vector<FObj> d_fo;
  std::vector<DevObjBox> d_ob, want_ob;
  if (!download(s->f64.meshes.p, dm64.size(), d_dm64) || !download(s->f32.meshes.p, fm.size(), d_fm) ||
      !download(s->f32.objs.p, fo.size(), d_fo) || !download(s->objbox_dev.p, s->objbins ? boxes.size() : 0, d_ob))
    return fail(RT_E_DEVICE, "reading the mesh arrays back failed");
  for (size_t k = 0; k < dm64.size(); ++k) {
    out[8] += diff_bytes(s->h_dm32[k], dm32[k]);
    out[9] += diff_bytes(d_dm64[k], dm64[k]);
    out[10] += diff_bytes(d_fm[k], fm[k]);
  }
  for (size_t k = 0; k < fo.size(); ++k) out[11] += diff_bytes(d_fo[k], fo[k]);
  if (s->objbins) {
    dev_obj_boxes(boxes, want_ob);
    for (size_t k = 0; k < want_ob.size(); ++k) out[12] += diff_bytes(d_ob[k], want_ob[k]);
  }
  return RT_OK;
}

// FNV-1a hashes of the device arrays a mesh update writes, for "nothing else
// changed" checks: 0 mesh's TriFast records, 1 its TriF64, 2 / 3 its float32 /
// float64 normals, 4 / 5 its nodes in the float64 / float32 tree, 6 bin_dev,
// 7 the mesh, object and object-box records of the whole scene.
extern "C" int rtmi_test_mesh_hash(rt_scene* s, int32_t mesh, uint64_t out[8]) {
  if (!s || !out || mesh < 0 || mesh >= s->nmesh) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  HIP_TRY(hipDeviceSynchronize());
  const rt_scene::MeshKeep& keep = s->mesh_keep[(size_t)mesh];
  const size_t nf = (size_t)keep.nf, nn = (size_t)keep.node_count;
  bool ok = true;
  const auto hash_dev = [&](const void* p, size_t bytes, uint64_t h = 1469598103934665603ull) {
    std::vector<unsigned char> buf;
    ok = ok && download(static_cast<const unsigned char*>(p), p ? bytes : 0, buf);
    return fnv(buf.data(), buf.size(), h);
  };
  out[0] = hash_dev(reinterpret_cast<const TriFast*>(s->f32.tree.p + s->num_nodes) + keep.tri_base, nf * sizeof(TriFast));
  out[1] = hash_dev(s->f64.tris.p + keep.tri_base, nf * sizeof(TriF64));
  out[2] = hash_dev(s->f32.normals.p + 3 * keep.tri_base, nf * 3 * sizeof(float));
  out[3] = hash_dev(s->f64.normals.p + 3 * keep.tri_base, nf * 3 * sizeof(double));
  out[4] = hash_dev(s->nodes.p + keep.node_base, nn * sizeof(BvhNode));
  out[5] = hash_dev(s->f32.tree.p + keep.node_base, nn * sizeof(BvhNode));
  out[6] = hash_dev(s->bin_dev.p, s->binnable ? s->bin_tris.size() * sizeof(DevBinTri) : 0);
  out[7] = hash_dev(s->f64.meshes.p, (size_t)s->nmesh * sizeof(DevMesh<double>));
  out[7] = hash_dev(s->f32.meshes.p, (size_t)s->nmesh * sizeof(FMesh), out[7]);
  out[7] = hash_dev(s->f32.objs.p, (size_t)s->nobj * sizeof(FObj), out[7]);
  out[7] = hash_dev(s->objbox_dev.p, s->objbins ? (size_t)s->nobj * sizeof(DevObjBox) : 0, out[7]);
  return ok ? RT_OK : fail(RT_E_DEVICE, "reading the mesh arrays back failed");
}

// enable: time the passes of the next updates (the stream is waited for after
// each). ms (may be null): the last timed update's copy-in, bounds, buffer
// copies, records + normals, refit + bins + box records, lights.
extern "C" int rtmi_test_mesh_update_passes(rt_scene* s, int32_t enable, float ms[6]) {
  if (!s) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  if (ms) std::copy(s->mesh_ms, s->mesh_ms + 6, ms);
  s->mesh_timed = enable != 0;
  return RT_OK;
}

// ---- tree checker (tests/test_bvh_corpus_cpu.py, tests/test_gpu_bvh.py) ----

namespace {

enum {  // out[] of the two checker hooks; 0 - 7 are counters a sound tree leaves at zero
  kChkInvalid = 0,    // validate_bvh fails, or the walk from the root does not reach every node once
  kChkUncontained,    // faces outside one of their ancestors' boxes (uncontained, the builders' margin)
  kChkBigLeaves,      // leaves of more than kLeafMax faces
  kChkLayout,         // inner children that are not at their depth-first index
  kChkHostBoxes,      // nodes whose 48 box bytes differ from refit_bvh of the same topology
  kChkBoxes64,        // the same for the float64 kernels' node array (device hook only)
  kChkBoxes32,        // the same for the float32 tree (device hook only)
  kChkChildren,       // child references and counts of the two device copies (device hook only)
  kChkLeafMax,        // the largest leaf
  kChkDepth,          // depth walked from the root (root = 1, inner nodes)
  kChkReported,       // the depth the builder / the scene reports
  kChkNodes,          // nodes
  kChkWords
};

double half_area(const float* lo, const float* hi) {
  const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
  return dx * dy + dy * dz + dz * dx;
}

// What is checked of the tree itself (no refit): counters 0 - 3, words 8, 9,
// 11, and the SAH cost with cost_node = cost_tri = 1: the sum over inner nodes
// of half-area(node) / half-area(root) plus the sum over leaves of
// n * half-area(leaf) / half-area(root); 0 when the root's area is 0. A node's
// box is the union of its two child boxes.
void check_tree(const BvhResult& r, const double* v, const int32_t* f, int64_t nf, int64_t* out, double* cost) {
  const char* err = "";
  *cost = 0.0;
  out[kChkNodes] = (int64_t)r.nodes.size();
  if (!validate_bvh(r, nf, &err)) {
    out[kChkInvalid] = 1;
    return;
  }
  const size_t nn = r.nodes.size();
  if (nn == 0) return;
  const bool single = nn == 1 && r.nodes[0].n0 > 0 && r.nodes[0].c0 == r.nodes[0].c1;
  // parents before children, every node once
  std::vector<int32_t> pre, depth(nn, 0), inner(nn, 0);
  std::vector<unsigned char> seen(nn, 0);
  pre.push_back(0);
  depth[0] = 1;
  seen[0] = 1;
  for (size_t k = 0; k < pre.size(); ++k) {
    const BvhNode& nd = r.nodes[(size_t)pre[k]];
    for (int slot = 0; slot < 2; ++slot) {
      const int32_t c = slot ? nd.c1 : nd.c0, n = slot ? nd.n1 : nd.n0;
      if (n > 0) continue;
      if (seen[(size_t)c]) {
        out[kChkInvalid] = 1;
        return;
      }
      seen[(size_t)c] = 1;
      depth[(size_t)c] = depth[(size_t)pre[k]] + 1;
      pre.push_back(c);
    }
  }
  if (pre.size() != nn) {
    out[kChkInvalid] = 1;
    return;
  }
  auto node_area = [&](const BvhNode& nd) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(nd.lo0[a], nd.lo1[a]);
      hi[a] = std::max(nd.hi0[a], nd.hi1[a]);
    }
    return half_area(lo, hi);
  };
  const double root_area = node_area(r.nodes[0]);
  double sum = 0.0;
  for (size_t k = nn; k-- > 0;) {
    const int32_t i = pre[k];
    const BvhNode& nd = r.nodes[(size_t)i];
    inner[(size_t)i] = 1 + (nd.n0 == 0 ? inner[(size_t)nd.c0] : 0) + (nd.n1 == 0 ? inner[(size_t)nd.c1] : 0);
    out[kChkDepth] = std::max<int64_t>(out[kChkDepth], depth[(size_t)i]);
    if (nd.n0 == 0 && nd.c0 != i + 1) ++out[kChkLayout];
    if (nd.n1 == 0 && nd.c1 != i + 1 + (nd.n0 == 0 ? inner[(size_t)nd.c0] : 0)) ++out[kChkLayout];
    sum += node_area(nd);
    for (int slot = 0; slot < (single ? 1 : 2); ++slot) {
      const int32_t n = slot ? nd.n1 : nd.n0;
      if (n == 0) continue;
      out[kChkLeafMax] = std::max<int64_t>(out[kChkLeafMax], n);
      if (n > kLeafMax) ++out[kChkBigLeaves];
      sum += (double)n * (slot ? half_area(nd.lo1, nd.hi1) : half_area(nd.lo0, nd.hi0));
    }
  }
  *cost = root_area > 0.0 ? sum / root_area : 0.0;
  double inflate = 0.0;
  std::vector<AncBox> anc;
  if (!bvh_margin(v, f, nf, &inflate)) {
    out[kChkInvalid] = 1;
    return;
  }
  out[kChkUncontained] = uncontained(r, v, f, inflate, 0, anc);
}

}  // namespace

// CPU only: the host SAH builder (build_bvh) on these arrays, its tree through
// the checker. out: 12 words (kChk* above; the device copies' counters stay
// zero), cost: 1. RT_E_INVALID, with the builder's message, when it declines.
// defect (0: none) spoils the tree before it is checked, to show what the
// checker sees: 1 the last node's first box ends below where it starts, 2 the
// root's two children change places, 4 the reported depth is one too many.
extern "C" int rtmi_test_bvh_check_host(const double* v, int64_t nv, const int32_t* faces, int64_t nf, int32_t defect,
                                        int64_t out[12], double cost[1]) {
  if (!v || !faces || !out || !cost || nv <= 0 || nf <= 0) return fail(RT_E_INVALID, "bad argument");
  for (int64_t k = 0; k < 3 * nf; ++k)
    if (faces[k] < 0 || faces[k] >= nv) return fail(RT_E_INVALID, "face index out of range");
  std::fill(out, out + kChkWords, 0);
  BvhResult r;
  const char* err = "";
  BvhBuildParams prm;
  if (!build_bvh(v, faces, nf, prm, &r, &err)) return fail(RT_E_INVALID, "%s", err);
  out[kChkReported] = r.max_depth + (defect == 4 ? 1 : 0);
  if (defect == 1) r.nodes.back().hi0[0] = r.nodes.back().lo0[0] - 1.0f;
  if (defect == 2) {
    BvhNode& n0 = r.nodes[0];
    std::swap(n0.c0, n0.c1);
    std::swap(n0.n0, n0.n1);
    for (int a = 0; a < 3; ++a) {
      std::swap(n0.lo0[a], n0.lo1[a]);
      std::swap(n0.hi0[a], n0.hi1[a]);
    }
  }
  check_tree(r, v, faces, nf, out, cost);
  BvhResult fit = r;
  if (!refit_bvh(v, faces, nf, &fit, &err)) return fail(RT_E_INVALID, "%s", err);
  for (size_t k = 0; k < r.nodes.size(); ++k)
    out[kChkHostBoxes] += std::memcmp(r.nodes[k].lo0, fit.nodes[k].lo0, 12 * sizeof(float)) != 0 ? 1 : 0;
  return RT_OK;
}

// One mesh of a live scene: its kept vertices, faces and leaf order, its nodes
// in h_nodes (rebased as rtmi_test_mesh_update_diff rebases them), in the
// float64 kernels' node array and in the float32 tree, through the checker.
// out: 12 words (kChk* above), cost: 1.
extern "C" int rtmi_test_bvh_check(rt_scene* s, int32_t mesh, int64_t out[12], double cost[1]) {
  if (!s || !out || !cost || mesh < 0 || mesh >= s->nmesh) return fail(RT_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  HIP_TRY(hipDeviceSynchronize());
  std::fill(out, out + kChkWords, 0);
  const rt_scene::MeshKeep& keep = s->mesh_keep[(size_t)mesh];
  std::vector<double> v;
  std::vector<int32_t> f, order;
  std::vector<BvhNode> tree, nodes;
  if (!download(keep.verts.p, (size_t)keep.nv * 3, v) || !download(keep.faces.p, (size_t)keep.nf * 3, f) ||
      !download(keep.order.p, (size_t)keep.nf, order) || !download(s->f32.tree.p, (size_t)s->num_nodes, tree) ||
      !download(s->nodes.p, (size_t)s->num_nodes, nodes))
    return fail(RT_E_DEVICE, "reading the mesh arrays back failed");
  const BvhResult r = mesh_tree(s, keep, order);
  out[kChkReported] = s->max_depth;
  check_tree(r, v.data(), f.data(), keep.nf, out, cost);
  if (out[kChkInvalid]) return RT_OK;
  return refit_diff(s, keep, r, v, f, nodes, tree, &out[kChkHostBoxes], &out[kChkBoxes64], &out[kChkBoxes32],
                    &out[kChkChildren]);
}

// The device builder alone (build_bvh_device, no scene) on these arrays, on
// the current device. out[0]: it accepts the mesh (1 / 0: rt_last_error has
// its reason), out[1]: the depth of the tree it formed, which it reports even
// when it declines the tree for that depth, out[2]: nodes.
extern "C" int rtmi_test_ploc_raw(const double* v, int64_t nv, const int32_t* faces, int64_t nf, int64_t out[3]) {
  if (!v || !faces || !out || nv <= 0 || nf <= 0) return fail(RT_E_INVALID, "bad argument");
  for (int64_t k = 0; k < 3 * nf; ++k)
    if (faces[k] < 0 || faces[k] >= nv) return fail(RT_E_INVALID, "face index out of range");
  DevBuf<double> dv;
  DevBuf<int32_t> df;
  if (int rc = dv.upload(v, (size_t)nv * 3)) return rc;
  if (int rc = df.upload(faces, (size_t)nf * 3)) return rc;
  BvhResult r;
  const char* err = "";
  BvhBuildParams prm;
  out[0] = build_bvh_device(dv.p, df.p, nf, prm, &r, &err) ? 1 : 0;
  out[1] = r.max_depth;
  out[2] = (int64_t)r.nodes.size();
  if (!out[0]) (void)fail(RT_E_DEVICE, "%s", err);
  return RT_OK;
}
