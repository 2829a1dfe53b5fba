// rtmi.cpp — C-ABI (include/rtmi.h) of the MI355X trace/shade backend.
//
// Replaces the reference's renderLine / initRenderer
// (src/renderer/renderer.nim:162-215) behind plain C entry points: the scene
// is flattened and uploaded once (rt_scene_create), then whole frames, row
// ranges (the pool's scanline messages, src/raytracer.nim:25-32) or
// multi-GPU bands are rendered by the gfx950 kernels in rt_device.h.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "rt_mesh_gpu.h"
#include "rt_scene.h"

static thread_local std::string g_err;

int rtmi::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int rtmi_fail_msg(int code, const char* msg) { return fail(code, "%s", msg ? msg : ""); }

extern "C" {

int rt_version(void) { return RTMI_ABI_VERSION; }

#ifndef RTMI_SOURCE_HASH
#define RTMI_SOURCE_HASH "unknown"
#endif
const char* rt_build_source_hash(void) { return RTMI_SOURCE_HASH; }

const char* rt_last_error(void) { return g_err.c_str(); }

int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int rt_init(int device) {
  const int n = rt_device_count();
  if (n <= 0) return fail(RT_E_DEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return fail(RT_E_INVALID, "device %d out of range [0, %d)", device, n);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(RT_E_DEVICE, "device %d is %s; librtmi.so is built for gfx950 (MI355X) only", device,
                prop.gcnArchName);
  return RT_OK;
}

int rt_mat4_inverse(const double m_[16], double out[16]) {
  if (!m_ || !out) return fail(RT_E_INVALID, "null matrix");
  // GLM compute_inverse (cofactors times 1/determinant), m[c][r] = m_[c*4+r]
  auto m = [&](int c, int r) { return m_[c * 4 + r]; };
  const double Coef00 = m(2, 2) * m(3, 3) - m(3, 2) * m(2, 3);
  const double Coef02 = m(1, 2) * m(3, 3) - m(3, 2) * m(1, 3);
  const double Coef03 = m(1, 2) * m(2, 3) - m(2, 2) * m(1, 3);
  const double Coef04 = m(2, 1) * m(3, 3) - m(3, 1) * m(2, 3);
  const double Coef06 = m(1, 1) * m(3, 3) - m(3, 1) * m(1, 3);
  const double Coef07 = m(1, 1) * m(2, 3) - m(2, 1) * m(1, 3);
  const double Coef08 = m(2, 1) * m(3, 2) - m(3, 1) * m(2, 2);
  const double Coef10 = m(1, 1) * m(3, 2) - m(3, 1) * m(1, 2);
  const double Coef11 = m(1, 1) * m(2, 2) - m(2, 1) * m(1, 2);
  const double Coef12 = m(2, 0) * m(3, 3) - m(3, 0) * m(2, 3);
  const double Coef14 = m(1, 0) * m(3, 3) - m(3, 0) * m(1, 3);
  const double Coef15 = m(1, 0) * m(2, 3) - m(2, 0) * m(1, 3);
  const double Coef16 = m(2, 0) * m(3, 2) - m(3, 0) * m(2, 2);
  const double Coef18 = m(1, 0) * m(3, 2) - m(3, 0) * m(1, 2);
  const double Coef19 = m(1, 0) * m(2, 2) - m(2, 0) * m(1, 2);
  const double Coef20 = m(2, 0) * m(3, 1) - m(3, 0) * m(2, 1);
  const double Coef22 = m(1, 0) * m(3, 1) - m(3, 0) * m(1, 1);
  const double Coef23 = m(1, 0) * m(2, 1) - m(2, 0) * m(1, 1);
  const double Fac0[4] = {Coef00, Coef00, Coef02, Coef03};
  const double Fac1[4] = {Coef04, Coef04, Coef06, Coef07};
  const double Fac2[4] = {Coef08, Coef08, Coef10, Coef11};
  const double Fac3[4] = {Coef12, Coef12, Coef14, Coef15};
  const double Fac4[4] = {Coef16, Coef16, Coef18, Coef19};
  const double Fac5[4] = {Coef20, Coef20, Coef22, Coef23};
  const double Vec0[4] = {m(1, 0), m(0, 0), m(0, 0), m(0, 0)};
  const double Vec1[4] = {m(1, 1), m(0, 1), m(0, 1), m(0, 1)};
  const double Vec2[4] = {m(1, 2), m(0, 2), m(0, 2), m(0, 2)};
  const double Vec3[4] = {m(1, 3), m(0, 3), m(0, 3), m(0, 3)};
  double inv[4][4];
  const double SignA[4] = {+1, -1, +1, -1}, SignB[4] = {-1, +1, -1, +1};
  for (int i = 0; i < 4; ++i) {
    inv[0][i] = (Vec1[i] * Fac0[i] - Vec2[i] * Fac1[i] + Vec3[i] * Fac2[i]) * SignA[i];
    inv[1][i] = (Vec0[i] * Fac0[i] - Vec2[i] * Fac3[i] + Vec3[i] * Fac4[i]) * SignB[i];
    inv[2][i] = (Vec0[i] * Fac1[i] - Vec1[i] * Fac3[i] + Vec3[i] * Fac5[i]) * SignA[i];
    inv[3][i] = (Vec0[i] * Fac2[i] - Vec1[i] * Fac4[i] + Vec2[i] * Fac5[i]) * SignB[i];
  }
  const double Row0[4] = {inv[0][0], inv[1][0], inv[2][0], inv[3][0]};
  double Dot0[4];
  for (int i = 0; i < 4; ++i) Dot0[i] = m(0, i) * Row0[i];
  const double Dot1 = (Dot0[0] + Dot0[1]) + (Dot0[2] + Dot0[3]);
  if (Dot1 == 0.0 || !std::isfinite(Dot1)) return fail(RT_E_INVALID, "singular matrix");
  const double one_over_det = 1.0 / Dot1;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) out[c * 4 + r] = inv[c][r] * one_over_det;
  return RT_OK;
}

int rt_load_geom(const char* path, int64_t* num_triangles, double* vertices) {
  if (!path || !num_triangles) return fail(RT_E_INVALID, "null argument");
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(RT_E_IO, "cannot open %s", path);
  int32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n < 0) {
    std::fclose(f);
    return fail(RT_E_IO, "%s: bad .geom header", path);
  }
  if (!vertices) {
    std::fclose(f);
    *num_triangles = n;
    return RT_OK;
  }
  if (*num_triangles < n) {
    std::fclose(f);
    return fail(RT_E_INVALID, "buffer holds %lld triangles, file has %d", (long long)*num_triangles, n);
  }
  std::vector<float> buf((size_t)n * 9);
  const size_t got = buf.empty() ? 0 : std::fread(buf.data(), sizeof(float), buf.size(), f);
  std::fclose(f);
  if (got != buf.size()) return fail(RT_E_IO, "%s: truncated (%zu of %zu floats)", path, got, buf.size());
  for (size_t i = 0; i < buf.size(); ++i) vertices[i] = (double)buf[i];
  *num_triangles = n;
  return RT_OK;
}

int rt_band_rows(int32_t height, int32_t band_h, int32_t world, int32_t* out_rows) {
  if (!out_rows || height <= 0 || band_h <= 0 || world <= 0) return fail(RT_E_INVALID, "bad band geometry");
  const int32_t nbands = (height + band_h - 1) / band_h;
  *out_rows = ((nbands + world - 1) / world) * band_h;
  return RT_OK;
}

}  // extern "C"

namespace {

template <class R>
void fill_precision(const rt_scene_desc* d, const std::vector<std::vector<double>>& normals,
                    const std::vector<BvhResult>& bvhs, const std::vector<int32_t>& node_base,
                    const std::vector<std::vector<double>>& aabbs, std::vector<DevObject<R>>& objs,
                    std::vector<DevLight<R>>& lights, std::vector<DevMesh<R>>& meshes,
                    std::vector<typename TriOf<R>::type>* tris, std::vector<R>& nrm) {
  fill_objects<R>(d->objects, d->num_objects, objs);
  fill_lights<R>(d->lights, d->num_lights, lights);
  meshes.assign((size_t)d->num_meshes, DevMesh<R>{});
  int64_t total = 0;
  for (int m = 0; m < d->num_meshes; ++m) total += d->meshes[m].num_faces;
  if (tris) tris->assign((size_t)total, typename TriOf<R>::type{});
  nrm.resize((size_t)total * 3);
  int32_t normal_base = 0;
  for (int m = 0; m < d->num_meshes; ++m) {
    const rt_mesh_desc& md = d->meshes[m];
    DevMesh<R>& dm = meshes[(size_t)m];
    for (int k = 0; k < 3; ++k) {
      dm.lo[k] = (R)aabbs[(size_t)m][k];
      dm.hi[k] = (R)aabbs[(size_t)m][3 + k];
    }
    dm.num_faces = (int32_t)md.num_faces;
    dm.normal_base = normal_base;
    dm.root = bvhs[(size_t)m].nodes.empty() ? -1 : node_base[(size_t)m];
    const std::vector<int32_t>& order = bvhs[(size_t)m].order;
    if (tris) {
      typename TriOf<R>::type* out = tris->data() + normal_base;
      parallel_for((int64_t)order.size(), [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i) {
          const int32_t face = order[(size_t)i];
          typename TriOf<R>::type& t = out[i];
          const int32_t* fi = &md.faces[3 * (size_t)face];
          const double* v0 = &md.vertices[3 * (size_t)fi[0]];
          const double* v1 = &md.vertices[3 * (size_t)fi[1]];
          const double* v2 = &md.vertices[3 * (size_t)fi[2]];
          for (int k = 0; k < 3; ++k) {
            t.v0[k] = (R)v0[k];
            t.e1[k] = (R)(v1[k] - v0[k]);  // v0v1 exactly as geom.nim:286-288
            t.e2[k] = (R)(v2[k] - v0[k]);  // v0v2 exactly as geom.nim:292-294
          }
          t.id = face;
        }
      });
    }
    const std::vector<double>& src = normals[(size_t)m];
    R* dst = nrm.data() + 3 * (size_t)normal_base;
    parallel_for((int64_t)src.size(), [&](int64_t b, int64_t e) {
      for (int64_t i = b; i < e; ++i) dst[i] = (R)src[(size_t)i];
    });
    normal_base += (int32_t)md.num_faces;
  }
  // pad so a kernel may read kLeafMax records from any leaf start
  if (tris)
    for (int k = 0; k < kLeafMax - 1; ++k) {
      typename TriOf<R>::type t{};
      t.id = -1;
      tris->push_back(t);
    }
}

// float32 kernel records (rt_common.h FObj/FObjX/FMesh/FLight).
void fill_fast_records(const rt_scene_desc* d, const std::vector<DevMesh<float>>& dm, std::vector<FObj>& fo,
                       std::vector<FObjX>& fx, std::vector<FMesh>& fm, std::vector<FLight>& fl) {
  fill_fast_objects(d->objects, d->num_objects, dm, fo, fx);
  fm.assign(dm.size(), FMesh{});
  for (size_t m = 0; m < dm.size(); ++m) {
    for (int k = 0; k < 3; ++k) {
      fm[m].lo[k] = dm[m].lo[k];
      fm[m].hi[k] = dm[m].hi[k];
    }
    fm[m].root = dm[m].root;
    fm[m].normal_base = dm[m].normal_base;
  }
  fill_fast_lights(d->lights, d->num_lights, fl);
}

}  // namespace

namespace rtmi {

// An object's bin box (rt_bins.h ObjBox): the world box of its object-space
// box lo..hi, through the inverse of the world_to_object the kernel
// transforms rays with. rt_scene_create and a mesh update form the same.
void world_obj_box(int32_t type, const double* w2o, const double lo[3], const double hi[3], ObjBox* out) {
  ObjBox& b = *out;
  double o2w[16];
  b.always = type == RT_PLANE || rt_mat4_inverse(w2o, o2w) != RT_OK;
  if (b.always) return;
  for (int k = 0; k < 3; ++k) {
    b.lo[k] = INFINITY;
    b.hi[k] = -INFINITY;
  }
  for (int c = 0; c < 8; ++c) {
    const double q[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
    for (int r = 0; r < 3; ++r) {
      const double w = o2w[0 * 4 + r] * q[0] + o2w[1 * 4 + r] * q[1] + o2w[2 * 4 + r] * q[2] + o2w[3 * 4 + r];
      b.corner[c][r] = w;
      b.lo[r] = std::min(b.lo[r], w);
      b.hi[r] = std::max(b.hi[r], w);
    }
  }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(b.lo[k]) || !std::isfinite(b.hi[k])) b.always = true;
}

void dev_obj_boxes(const std::vector<ObjBox>& boxes, std::vector<DevObjBox>& ob) {
  ob.assign(boxes.size(), DevObjBox{});
  for (size_t i = 0; i < boxes.size(); ++i) {
    const ObjBox& b = boxes[i];
    for (int k = 0; k < 3; ++k) {
      ob[i].lo[k] = b.lo[k];
      ob[i].hi[k] = b.hi[k];
    }
    ob[i].always = b.always ? 1 : 0;
    ob[i].pad = 0;
  }
}

int wait_for_calls(rt_scene* s) {
  hipError_t e = s->done ? hipEventSynchronize(s->done) : hipSuccess;
  if (e == hipSuccess && s->q_done_rec) e = hipEventSynchronize(s->q_done);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->bstream);
  if (e != hipSuccess) return fail(RT_E_DEVICE, "waiting for the scene's earlier calls: %s", hipGetErrorString(e));
  return RT_OK;
}

}  // namespace rtmi

extern "C" int rt_scene_create(const rt_scene_desc* d, rt_scene** out_scene) {
  if (!d || !out_scene) return fail(RT_E_INVALID, "null argument");
  *out_scene = nullptr;
  if (d->num_objects < 0 || d->num_lights < 0 || d->num_meshes < 0)
    return fail(RT_E_INVALID, "negative counts");
  if ((d->num_objects > 0 && !d->objects) || (d->num_lights > 0 && !d->lights) ||
      (d->num_meshes > 0 && !d->meshes))
    return fail(RT_E_INVALID, "null array with nonzero count");
  if (!affine(d->camera_to_world)) return fail(RT_E_UNSUPPORTED, "camera_to_world is not affine");
  const auto t0 = std::chrono::steady_clock::now();
  if (int orc = check_objects(d->objects, d->num_objects, d->num_meshes)) return orc;
  for (int i = 0; i < d->num_lights; ++i)
    if (d->lights[i].type != RT_DISTANT_LIGHT && d->lights[i].type != RT_POINT_LIGHT)
      return fail(RT_E_INVALID, "light %d: bad type", i);
  if (d->bvh_builder != RT_BVH_SAH && d->bvh_builder != RT_BVH_PLOC)
    return fail(RT_E_INVALID, "bad bvh_builder %d", d->bvh_builder);
  int dev = device_of_current();
  if (dev < 0 || rt_device_count() <= 0) return fail(RT_E_DEVICE, "no HIP device (call rt_init)");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(RT_E_DEVICE, "device %d is %s; librtmi.so is built for gfx950 only", dev, prop.gcnArchName);
  std::vector<std::vector<double>> normals((size_t)d->num_meshes), aabbs((size_t)d->num_meshes);
  std::vector<BvhResult> bvhs((size_t)d->num_meshes);
  // device copies of every mesh's arrays: the device builder and the
  // triangle-record packing (rt_bvh_gpu.hip) read them
  std::vector<DevBuf<double>> d_verts((size_t)d->num_meshes);
  std::vector<DevBuf<int32_t>> d_faces((size_t)d->num_meshes);
  std::vector<int32_t> node_base((size_t)d->num_meshes, 0);
  int64_t ntri = 0, nnodes = 0;
  int maxdepth = 0;
  std::vector<BvhNode> all_nodes;
  for (int m = 0; m < d->num_meshes; ++m) {
    const rt_mesh_desc& md = d->meshes[m];
    if (md.num_faces < 0 || md.num_vertices < 0 || (md.num_faces > 0 && (!md.faces || !md.vertices)))
      return fail(RT_E_INVALID, "mesh %d: bad arrays", m);
    for (int64_t k = 0; k < md.num_faces * 3; ++k)
      if (md.faces[k] < 0 || md.faces[k] >= md.num_vertices)
        return fail(RT_E_INVALID, "mesh %d: face index %d out of range", m, md.faces[k]);
    // face normals: given, or calcNormals (src/loaders/obj.nim:65-84)
    std::vector<double>& nr = normals[(size_t)m];
    nr.resize((size_t)md.num_faces * 3);
    parallel_for(md.num_faces, [&](int64_t fb, int64_t fe) {
    for (int64_t fidx = fb; fidx < fe; ++fidx) {
      if (md.normals) {
        for (int k = 0; k < 3; ++k) nr[3 * (size_t)fidx + k] = md.normals[3 * fidx + k];
        continue;
      }
      const double* p0 = &md.vertices[3 * (size_t)md.faces[3 * fidx + 0]];
      const double* p1 = &md.vertices[3 * (size_t)md.faces[3 * fidx + 1]];
      const double* p2 = &md.vertices[3 * (size_t)md.faces[3 * fidx + 2]];
      const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
      const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
      const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      double dd = 0.0;
      dd = dd + cx * cx;
      dd = dd + cy * cy;
      dd = dd + cz * cz;
      const double len = std::sqrt(dd);
      nr[3 * (size_t)fidx + 0] = cx / len;
      nr[3 * (size_t)fidx + 1] = cy / len;
      nr[3 * (size_t)fidx + 2] = cz / len;
    }
    });
    // calcAABB (geom.nim:175-188) over every vertex
    std::vector<double>& bb = aabbs[(size_t)m];
    bb = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t v = 0; v < md.num_vertices; ++v)
      for (int k = 0; k < 3; ++k) {
        const double x = md.vertices[3 * v + k];
        if (x < bb[(size_t)k]) bb[(size_t)k] = x;
        if (x > bb[3 + (size_t)k]) bb[3 + (size_t)k] = x;
      }
    int urc;
    if ((urc = d_verts[(size_t)m].upload(md.vertices, (size_t)md.num_vertices * 3)) ||
        (urc = d_faces[(size_t)m].upload(md.faces, (size_t)md.num_faces * 3)))
      return urc;
    const char* err = "BVH build failed";
    BvhBuildParams prm;
    // a face's vertices are finite under either builder (their min / max
    // pass over a NaN, so neither sees one; rt_scene_set_mesh_vertices declines it too)
    std::atomic<bool> finite{true};
    parallel_for(md.num_faces, [&](int64_t fb, int64_t fe) {
      bool all = true;
      for (int64_t k = 3 * fb; k < 3 * fe; ++k) {
        const double* p = &md.vertices[3 * (size_t)md.faces[k]];
        all = all && std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
      }
      if (!all) finite = false;
    });
    if (!finite) return fail(RT_E_INVALID, "mesh %d: mesh has non-finite vertices", m);
    bool device_built = d->bvh_builder == RT_BVH_PLOC;
    bool ok = device_built ? build_bvh_device(d_verts[(size_t)m].p, d_faces[(size_t)m].p, md.num_faces, prm,
                                              &bvhs[(size_t)m], &err)
                           : build_bvh(md.vertices, md.faces, md.num_faces, prm, &bvhs[(size_t)m], &err);
    // The clustering has no depth bound: boxes nested around a shared corner
    // (a fan of geometrically growing faces) merge one pair a round into a
    // chain as deep as their count. The host builder splits at the object
    // median past depth 38, so a mesh it accepts is never refused here.
    if (!ok && device_built && bvhs[(size_t)m].max_depth > kMaxBvhDepth) {
      device_built = false;
      ok = build_bvh(md.vertices, md.faces, md.num_faces, prm, &bvhs[(size_t)m], &err);
    }
    if (!ok) return fail(device_built ? RT_E_DEVICE : RT_E_INVALID, "mesh %d: %s", m, err);
    node_base[(size_t)m] = (int32_t)all_nodes.size();
    for (BvhNode nd : bvhs[(size_t)m].nodes) {
      if (nd.n0 == 0 && nd.c0 >= 0) nd.c0 += node_base[(size_t)m];
      if (nd.n1 == 0 && nd.c1 >= 0) nd.c1 += node_base[(size_t)m];
      if (nd.n0 > 0) nd.c0 += (int32_t)ntri;
      if (nd.n1 > 0) nd.c1 += (int32_t)ntri;
      all_nodes.push_back(nd);
    }
    ntri += md.num_faces;
    nnodes += (int64_t)bvhs[(size_t)m].nodes.size();
    maxdepth = std::max(maxdepth, bvhs[(size_t)m].max_depth);
  }
  if (ntri > INT32_MAX / 2) return fail(RT_E_UNSUPPORTED, "too many triangles");
  // the float32 kernel addresses its tree with signed 32-bit byte offsets
  if ((nnodes + ntri + kLeafMax) * (int64_t)sizeof(BvhNode) > (int64_t)INT32_MAX)
    return fail(RT_E_UNSUPPORTED, "%lld BVH nodes + %lld triangles exceed the float32 tree's 2 GiB offset range",
                (long long)nnodes, (long long)ntri);

  std::unique_ptr<rt_scene> s(new rt_scene());
  s->device = dev;
  s->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  s->nobj = d->num_objects;
  {
    int n_mesh_obj = 0;
    for (int i = 0; i < d->num_objects; ++i)
      if (d->objects[i].type == RT_MESH) {
        ++n_mesh_obj;
        s->shadow_mesh = i;
      }
    if (n_mesh_obj != 1) s->shadow_mesh = -1;
  }
  s->nmesh = d->num_meshes;
  // scene features -> the float32 kernel specialisation (rt_kernels_f32_part.hip); (SUB_POINT: adopt_lights)
  s->f32_subset = object_subset(d->objects, d->num_objects, &s->any_reflective);
  s->fov = d->fov;
  std::memcpy(s->c2w, d->camera_to_world, sizeof s->c2w);
  std::memcpy(s->bg, d->bg_color, sizeof s->bg);
  HIP_TRY(hipStreamCreateWithFlags(&s->stream.h, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&s->aux.h, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&s->fork.h, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&s->join.h, hipEventDisableTiming));
  for (Event& e : s->tev) HIP_TRY(hipEventCreate(&e.h));
  {
    // the build stream at the highest priority (rank 0 of 8 back to back:
    // 0.163 -> 0.161 ms against the default priority)
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess)
      HIP_TRY(hipStreamCreateWithPriority(&s->bstream.h, hipStreamNonBlocking, hi));
    else
      HIP_TRY(hipStreamCreateWithFlags(&s->bstream.h, hipStreamNonBlocking));
  }
  {
    // `built` only orders the build stream before the caller's stream on this
    // device: a device-scope release (no system-scope cache writeback) is
    // enough. `used` doubles as `done`, which the host waits on before
    // reading device memory and peers copy behind: system scope.
    for (rt_scene::Frame* f : {&s->fr, &s->fr2}) {
      HIP_TRY(hipEventCreateWithFlags(&f->built.h, hipEventDisableTiming | hipEventReleaseToDevice));
      HIP_TRY(hipEventCreateWithFlags(&f->used.h, hipEventDisableTiming));
    }
  }
  s->done = s->fr.used;
  s->fr2.id = 1;
  {
    const char* e = std::getenv("RTMI_PIPE");
    s->pipe_mode = e && *e ? (std::atoi(e) != 0 ? 1 : 0) : -1;
  }
  {
    std::vector<DevObject<float>> o;
    std::vector<DevLight<float>> l;
    std::vector<DevMesh<float>> m;
    std::vector<float> n;
    fill_precision<float>(d, normals, bvhs, node_base, aabbs, o, l, m, nullptr, n);
    std::vector<FObj> fo;
    std::vector<FObjX> fx;
    std::vector<FMesh> fm;
    std::vector<FLight> fl;
    fill_fast_records(d, m, fo, fx, fm, fl);
    for (const FObj& q : fo) s->h_obj_ty.push_back(q.t[1]);
    s->h_dm32 = m;
    s->h_fm = fm;
    s->h_fo = fo;
    int rc;
    std::vector<float> alb;
    fill_albedo32(d->objects, d->num_objects, alb);
    std::vector<double> alb64;
    fill_albedo64(d->objects, d->num_objects, alb64);
    if ((rc = s->f32.objs.upload(fo)) || (rc = s->f32.objx.upload(fx)) || (rc = s->f32.meshes.upload(fm)) ||
        (rc = s->f32.normals.upload(n)) || (rc = s->albedo32.upload(alb)) ||
        (rc = s->albedo64.upload(alb64)))
      return rc;
  }
  {
    std::vector<DevObject<double>> o;
    std::vector<DevLight<double>> l;
    std::vector<DevMesh<double>> m;
    std::vector<double> n;
    fill_precision<double>(d, normals, bvhs, node_base, aabbs, o, l, m, nullptr, n);
    s->h_dm64 = m;
    int rc;
    if ((rc = s->f64.objects.upload(o)) || (rc = s->f64.meshes.upload(m)) ||
        (rc = s->f64.normals.upload(n)))
      return rc;
  }
  {
    // triangle records in BVH leaf order, packed on the device; the float64
    // array carries kLeafMax - 1 padding records (id -1) so a kernel may
    // read kLeafMax records from any leaf start
    int rc;
    if ((rc = s->f32.tree.alloc((size_t)(nnodes + ntri))) || (rc = s->f64.tris.alloc((size_t)ntri + kLeafMax - 1)))
      return rc;
    TriFast* f32_tris = reinterpret_cast<TriFast*>(s->f32.tree.p + nnodes);
    std::vector<TriF64> pad((size_t)kLeafMax - 1);
    for (TriF64& t : pad) {
      std::memset(&t, 0, sizeof t);
      t.id = -1;
    }
    HIP_TRY(hipMemcpy(s->f64.tris.p + ntri, pad.data(), pad.size() * sizeof(TriF64), hipMemcpyHostToDevice));
    int64_t base = 0;
    s->mesh_keep.resize((size_t)d->num_meshes);
    for (int m = 0; m < d->num_meshes; ++m) {
      const int64_t nf = d->meshes[m].num_faces;
      // the leaf order stays on the device: a mesh update packs with it again
      rt_scene::MeshKeep& keep = s->mesh_keep[(size_t)m];
      DevBuf<int32_t>& order = keep.order;
      if ((rc = order.upload(bvhs[(size_t)m].order))) return rc;
      const bool ok = pack_triangles_device(d_verts[(size_t)m].p, d_faces[(size_t)m].p, order.p, nf,
                                            f32_tris + base, s->f64.tris.p + base, s->stream);
      HIP_TRY(hipStreamSynchronize(s->stream));
      if (!ok) return fail(RT_E_DEVICE, "mesh %d: triangle packing failed", m);
      keep.nv = d->meshes[m].num_vertices;
      keep.nf = nf;
      keep.tri_base = base;
      keep.node_base = node_base[(size_t)m];
      keep.node_count = (int32_t)bvhs[(size_t)m].nodes.size();
      keep.normals_given = d->meshes[m].normals != nullptr;
      base += nf;
    }
  }
  {
    // the refit's parent table: every inner child names its node and slot
    std::vector<int32_t> parent(all_nodes.size(), -1);
    for (size_t i = 0; i < all_nodes.size(); ++i) {
      const BvhNode& nd = all_nodes[i];
      if (nd.n0 == 0 && nd.c0 >= 0) parent[(size_t)nd.c0] = (int32_t)(2 * i);
      if (nd.n1 == 0 && nd.c1 >= 0) parent[(size_t)nd.c1] = (int32_t)(2 * i + 1);
    }
    int rc;
    if ((rc = s->refit_parent.upload(parent)) || (rc = s->refit_arrivals.alloc(all_nodes.size())) ||
        (rc = s->mesh_scratch.alloc((size_t)kMeshBoundsWords)))
      return rc;
    s->h_nodes = all_nodes;
  }
  int rc = s->nodes.upload(all_nodes);
  if (rc) return rc;
  {  // float32 tree: child refs -> byte offsets (leaves: past the nnodes node records)
    std::vector<BvhNode> fn(all_nodes);
    const int32_t kB = (int32_t)sizeof(BvhNode);
    for (BvhNode& nd : fn) {
      nd.c0 = (nd.n0 > 0 ? (int32_t)nnodes + nd.c0 : nd.c0) * kB;
      nd.c1 = (nd.n1 > 0 ? (int32_t)nnodes + nd.c1 : nd.c1) * kB;
    }
    if (!fn.empty())
      HIP_TRY(hipMemcpy(s->f32.tree.p, fn.data(), fn.size() * sizeof(BvhNode), hipMemcpyHostToDevice));
  }
  if (s->shadow_mesh >= 0) {  // bins of the only mesh object (rt_bins.h)
    const rt_object_desc& ob = d->objects[s->shadow_mesh];
    const int m = ob.mesh;
    const rt_mesh_desc& md = d->meshes[m];
    int64_t base = 0;
    for (int k = 0; k < m; ++k) base += d->meshes[k].num_faces;
    const std::vector<int32_t>& order = bvhs[(size_t)m].order;
    s->bin_tris.resize(order.size());
    parallel_for((int64_t)order.size(), [&](int64_t b, int64_t e) {
      for (int64_t i = b; i < e; ++i) {
        BinTri& t = s->bin_tris[(size_t)i];
        const int32_t* fi = &md.faces[3 * (size_t)order[(size_t)i]];
        for (int v = 0; v < 3; ++v)
          for (int k = 0; k < 3; ++k) t.v[v][k] = md.vertices[3 * (size_t)fi[v] + k];
        t.rec = (int32_t)((nnodes + base + i) * (int64_t)sizeof(TriFast));
        t.face = order[(size_t)i];
      }
    });
    std::memcpy(s->mesh_o2w, ob.object_to_world, sizeof s->mesh_o2w);
    std::memcpy(s->mesh_w2o, ob.world_to_object, sizeof s->mesh_w2o);
    s->binnable = !s->bin_tris.empty();
    static_assert(sizeof(BinTri) == sizeof(DevBinTri) && offsetof(BinTri, rec) == offsetof(DevBinTri, rec),
                  "BinTri and DevBinTri share one layout");
    if (s->binnable) {
      if ((rc = s->bin_dev.alloc(s->bin_tris.size()))) return rc;
      HIP_TRY(hipMemcpy(s->bin_dev.p, s->bin_tris.data(), s->bin_tris.size() * sizeof(BinTri), hipMemcpyHostToDevice));
      for (int k = 0; k < 3; ++k) {
        s->mesh_lo[k] = aabbs[(size_t)m][k];
        s->mesh_hi[k] = aabbs[(size_t)m][3 + k];
      }
    }
  }
  if (d->num_objects >= 4 && d->num_objects <= 64) {  // object bins (rt_bins.h)
    fill_obj_boxes(d->objects, d->num_objects, s->h_dm64, s->obj_boxes);
    s->objbins = true;
    std::vector<DevObjBox> ob;
    dev_obj_boxes(s->obj_boxes, ob);
    if ((rc = s->objbox_dev.upload(ob))) return rc;
  }
  // everything that depends on the lights (rt_scene_set_lights replaces it)
  s->num_triangles = ntri;
  s->num_nodes = nnodes;
  fill_obj_meta(d->objects, d->num_objects, s->obj_meta);
  s->obj_desc.assign(d->objects, d->objects + d->num_objects);
  {
    LightState ls;
    rc = build_lights(s.get(), d->lights, d->num_lights, false, &ls);
    if (rc) return rc;
    adopt_lights(s.get(), &ls);
  }
  s->max_waves = s->num_cus * 8 * 4;  // 8 blocks of 4 waves per CU at most
  // two kernels per two-class launch: their waves' partial counters side by side
  if ((rc = s->partials.alloc((size_t)2 * s->max_waves * kStatSlots))) return rc;
  if ((rc = s->queue.alloc(rt_scene::kQueueWords + 2 * (size_t)kStatSlots))) return rc;  // heads + Stats
  HIP_TRY(hipMemset(s->queue.p, 0, s->queue.bytes()));
  if ((rc = s->queue2.alloc(s->queue.n))) return rc;
  HIP_TRY(hipMemset(s->queue2.p, 0, s->queue2.bytes()));
  HIP_TRY(hipDeviceSynchronize());
  s->max_depth = maxdepth;
  for (int m = 0; m < d->num_meshes; ++m) {  // the scene keeps the meshes' device arrays (mesh updates)
    std::swap(s->mesh_keep[(size_t)m].verts, d_verts[(size_t)m]);
    std::swap(s->mesh_keep[(size_t)m].faces, d_faces[(size_t)m]);
  }
  s->build_ms =std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out_scene = s.release();
  return RT_OK;
}

extern "C" int rt_scene_destroy(rt_scene* s) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  DeviceGuard g(s->device);
  {
    // a call still inside the library on this scene (another thread) holds
    // s->mu: wait for it to leave before the scene goes. The caller must not
    // start new calls on a scene it destroys (rtmi.h); the Python / Nim
    // caches keep a per-scene count of calls in flight for that
    std::lock_guard<std::mutex> lk(s->mu);
    (void)wait_for_calls(s);  // the scene goes whatever they ended with
  }
  delete s;
  return RT_OK;
}

extern "C" int rt_scene_get_info(const rt_scene* s, rt_scene_info* out) {
  if (!s || !out) return fail(RT_E_INVALID, "null argument");
  out->num_objects = s->nobj;
  out->num_lights = s->nlight;
  out->num_meshes = s->nmesh;
  out->num_triangles = s->num_triangles;
  out->num_bvh_nodes = s->num_nodes;
  out->max_bvh_depth = s->max_depth;
  out->device = s->device;
  std::lock_guard<std::mutex> lk(const_cast<rt_scene*>(s)->mu);
  out->device_bytes = (int64_t)s->device_bytes();
  out->build_ms = s->build_ms;
  return RT_OK;
}

extern "C" int rt_scene_set_camera(rt_scene* s, const double c2w[16], double fov_deg) {
  if (!s || !c2w) return fail(RT_E_INVALID, "null argument");
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(c2w[k])) return fail(RT_E_INVALID, "camera_to_world[%d] is not finite", k);
  if (!(fov_deg > 0.0 && fov_deg < 180.0)) return fail(RT_E_INVALID, "fov %g outside (0, 180)", fov_deg);
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  // earlier calls may still read the launch orders measured for the old
  // camera, which clearing them frees. `done` alone covers those: only render
  // kernels read an order, and every render call ends by recording `done`.
  // Nothing else is freed here, so builds and queries (wait_for_calls) may run on
  const hipError_t e = hipEventSynchronize(s->done);
  std::memcpy(s->c2w, c2w, sizeof s->c2w);
  s->fov = fov_deg;
  s->orders.clear();    // measured per-group costs (launch order) too
  if (e != hipSuccess) return fail(RT_E_DEVICE, "waiting for the scene's earlier calls: %s", hipGetErrorString(e));
  return RT_OK;
}

extern "C" int rt_unshard_bands_device(const float* d_gathered, float* d_fb, int32_t width, int32_t height,
                                       int32_t band_h, int32_t world, void* stream) {
  if (!d_gathered || !d_fb || width <= 0 || height <= 0 || band_h <= 0 || world <= 0)
    return fail(RT_E_INVALID, "bad arguments");
  const int e = rtmi_launch_unshard(d_gathered, d_fb, width, height, band_h, world, stream);
  if (e) return fail(RT_E_DEVICE, "unshard launch failed: %s", hipGetErrorString((hipError_t)e));
  return RT_OK;
}

extern "C" int64_t rt_ppm_payload_bytes(int32_t width, int32_t height, int32_t bits) {
  if (width <= 0 || height <= 0 || bits < 1 || bits > 16) return fail(RT_E_INVALID, "bad ppm size / bits");
  return (int64_t)width * height * 3 * (bits <= 8 ? 1 : 2);
}

extern "C" int rt_ppm_header(int32_t width, int32_t height, int32_t bits, char* buf, int32_t buf_len) {
  if (width <= 0 || height <= 0 || bits < 1 || bits > 16 || !buf) return fail(RT_E_INVALID, "bad arguments");
  const int n = std::snprintf(buf, (size_t)std::max(0, buf_len), "P6 %d %d %d ", width, height, (1 << bits) - 1);
  if (n < 0 || n >= buf_len) return fail(RT_E_INVALID, "header buffer too small (%d bytes)", buf_len);
  return n;
}

extern "C" int rt_ppm_encode_device(const float* d_fb, int32_t width, int32_t height, int32_t bits, int32_t srgb,
                                    void* d_out, void* stream) {
  if (!d_fb || !d_out) return fail(RT_E_INVALID, "null buffer");
  if (rt_ppm_payload_bytes(width, height, bits) < 0) return RT_E_INVALID;
  if (((uintptr_t)d_fb & 15) || ((uintptr_t)d_out & 7)) return fail(RT_E_INVALID, "buffers must be 16-B (fb) / 8-B (out) aligned");
  const int e = rtmi_launch_ppm_encode(d_fb, (long long)width * height * 3, bits, srgb ? 1 : 0, d_out, stream);
  if (e) return fail(RT_E_DEVICE, "ppm encode launch failed: %s", hipGetErrorString((hipError_t)e));
  return RT_OK;
}

extern "C" int rt_rgba_encode_device(const float* d_fb, int32_t width, int32_t height, uint8_t alpha, void* d_out,
                                     void* stream) {
  if (!d_fb || !d_out) return fail(RT_E_INVALID, "null buffer");
  if (width <= 0 || height <= 0 || width > 65536 || height > 65536)
    return fail(RT_E_INVALID, "bad image size %dx%d", width, height);
  if (((uintptr_t)d_fb & 3) || ((uintptr_t)d_out & 3)) return fail(RT_E_INVALID, "buffers must be 4-B aligned");
  const int e = rtmi_launch_rgba_encode(d_fb, (long long)width * height, alpha, d_out, stream);
  if (e) return fail(RT_E_DEVICE, "rgba encode launch failed: %s", hipGetErrorString((hipError_t)e));
  return RT_OK;
}
