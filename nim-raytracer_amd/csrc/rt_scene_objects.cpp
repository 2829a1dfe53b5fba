// rt_scene_objects.cpp — everything of a scene that is formed from its
// objects' descriptions: the record fillers rt_scene_create and
// rt_scene_set_objects share, and rt_scene_set_objects itself, which builds
// the new records and the light state over them into buffers of their own and
// hands them to the scene by swapping once all of it succeeded.
#include <cmath>
#include <cstring>

#include "rt_scene.h"

namespace rtmi {

bool affine(const double* m) { return m[3] == 0.0 && m[7] == 0.0 && m[11] == 0.0 && m[15] == 1.0; }

// Identity / pure translation / general (float32 fast paths, DevObject.xf).
// Translation requires BOTH matrices to have an identity 3x3 block, so the
// normal transform (object_to_world * n) is the identity too.
int32_t classify_xf(const double* w2o, const double* o2w) {
  bool lin_id = true;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) {
      const double id = c == r ? 1.0 : 0.0;
      if (w2o[c * 4 + r] != id || o2w[c * 4 + r] != id) lin_id = false;
    }
  if (!lin_id) return XF_GENERAL;
  if (w2o[12] == 0.0 && w2o[13] == 0.0 && w2o[14] == 0.0) return XF_IDENTITY;
  return XF_TRANSLATE;
}

int check_objects(const rt_object_desc* objs, int32_t n, int32_t num_meshes) {
  for (int i = 0; i < n; ++i) {
    const rt_object_desc& o = objs[i];
    if (o.type < RT_SPHERE || o.type > RT_MESH) return fail(RT_E_INVALID, "object %d: bad type %d", i, o.type);
    if (o.type == RT_MESH && (o.mesh < 0 || o.mesh >= num_meshes))
      return fail(RT_E_INVALID, "object %d: mesh index %d out of range", i, o.mesh);
    if (!affine(o.object_to_world) || !affine(o.world_to_object))
      return fail(RT_E_UNSUPPORTED, "object %d: non-affine transform", i);
  }
  return RT_OK;
}

// The parity kernels' object records (DevObject).
template <class R>
void fill_objects(const rt_object_desc* objs, int32_t n, std::vector<DevObject<R>>& out) {
  out.assign((size_t)n, DevObject<R>{});
  for (int i = 0; i < n; ++i) {
    const rt_object_desc& s = objs[i];
    DevObject<R>& o = out[(size_t)i];
    for (int k = 0; k < 16; ++k) {
      o.w2o[k] = (R)s.world_to_object[k];
      o.o2w[k] = (R)s.object_to_world[k];
    }
    o.prm[0] = (R)(s.type == RT_SPHERE ? s.radius : s.box_min[0]);
    o.prm[1] = (R)s.box_min[1];
    o.prm[2] = (R)s.box_min[2];
    o.prm[4] = (R)s.box_max[0];
    o.prm[5] = (R)s.box_max[1];
    o.prm[6] = (R)s.box_max[2];
    for (int k = 0; k < 3; ++k) o.albedo[k] = (R)s.albedo[k];
    o.albedo[3] = (R)s.reflection;
    // albedo / PI in R, one correctly rounded IEEE division as the kernel's
    // (and the oracle's, rt_oracle.c shade) per-sample quotient
    for (int k = 0; k < 3; ++k) o.albp[k] = (R)s.albedo[k] / (R)3.14159265358979323846;
    o.type = s.type;
    o.mesh = s.type == RT_MESH ? s.mesh : 0;
    o.xf = classify_xf(s.world_to_object, s.object_to_world);
  }
}
template void fill_objects<float>(const rt_object_desc*, int32_t, std::vector<DevObject<float>>&);
template void fill_objects<double>(const rt_object_desc*, int32_t, std::vector<DevObject<double>>&);

// The float32 kernels' object records (rt_common.h FObj / FObjX).
void fill_fast_objects(const rt_object_desc* objs, int32_t n, const std::vector<DevMesh<float>>& dm,
                       std::vector<FObj>& fo, std::vector<FObjX>& fx) {
  const double kPi = 3.14159265358979323846;
  fo.assign((size_t)n, FObj{});
  fx.assign((size_t)n, FObjX{});
  for (int i = 0; i < n; ++i) {
    const rt_object_desc& s = objs[i];
    FObj& o = fo[(size_t)i];
    FObjX& x = fx[(size_t)i];
    o.type = s.type;
    o.xf = classify_xf(s.world_to_object, s.object_to_world);
    o.mesh = s.type == RT_MESH ? s.mesh : 0;
    for (int k = 0; k < 3; ++k) {
      o.t[k] = (float)s.world_to_object[12 + k];
      o.lo[k] = (float)(s.type == RT_MESH ? dm[(size_t)s.mesh].lo[k] : s.box_min[k]);
      o.hi[k] = (float)(s.type == RT_MESH ? dm[(size_t)s.mesh].hi[k] : s.box_max[k]);
    }
    // byte offset of the root node in FastData.tree
    o.root = s.type == RT_MESH && dm[(size_t)s.mesh].root >= 0 ? dm[(size_t)s.mesh].root * (int32_t)sizeof(BvhNode) : -1;
    o.r = (float)s.radius;
    for (int c = 0; c < 4; ++c)
      for (int r = 0; r < 3; ++r) x.w2o[c * 3 + r] = (float)s.world_to_object[c * 4 + r];
    for (int c = 0; c < 3; ++c)
      for (int r = 0; r < 3; ++r) x.o2w[c * 3 + r] = (float)s.object_to_world[c * 4 + r];
    for (int k = 0; k < 3; ++k) x.albedo_pi[k] = (float)(s.albedo[k] / kPi);
    x.refl = (float)s.reflection;
    x.normal_base = s.type == RT_MESH ? dm[(size_t)s.mesh].normal_base : 0;
  }
}

void fill_albedo32(const rt_object_desc* objs, int32_t n, std::vector<float>& out) {
  out.resize((size_t)n * 3);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = (float)objs[i].albedo[k];
}

void fill_albedo64(const rt_object_desc* objs, int32_t n, std::vector<double>& out) {
  out.resize((size_t)n * 3);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = objs[i].albedo[k];
}

void fill_obj_boxes(const rt_object_desc* objs, int32_t n, const std::vector<DevMesh<double>>& dm,
                    std::vector<ObjBox>& boxes) {
  boxes.assign((size_t)n, ObjBox{});
  for (int i = 0; i < n; ++i) {
    const rt_object_desc& ob = objs[i];
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int k = 0; k < 3 && ob.type != RT_PLANE; ++k) {
      lo[k] = ob.type == RT_SPHERE ? -std::fabs(ob.radius) : ob.type == RT_BOX ? ob.box_min[k] : dm[(size_t)ob.mesh].lo[k];
      hi[k] = ob.type == RT_SPHERE ? std::fabs(ob.radius) : ob.type == RT_BOX ? ob.box_max[k] : dm[(size_t)ob.mesh].hi[k];
    }
    world_obj_box(ob.type, ob.world_to_object, lo, hi, &boxes[(size_t)i]);
  }
}

void fill_obj_meta(const rt_object_desc* objs, int32_t n, std::vector<rt_scene::ObjMeta>& meta) {
  meta.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    rt_scene::ObjMeta& om = meta[(size_t)i];
    om.type = objs[i].type;
    om.mesh = objs[i].type == RT_MESH ? objs[i].mesh : -1;
    om.reflection = objs[i].reflection;
    std::memcpy(om.o2w, objs[i].object_to_world, sizeof om.o2w);
    std::memcpy(om.w2o, objs[i].world_to_object, sizeof om.w2o);
  }
}

unsigned object_subset(const rt_object_desc* objs, int32_t n, bool* any_reflective) {
  unsigned sub = 0;
  *any_reflective = false;
  for (int i = 0; i < n; ++i) {
    const rt_object_desc& ob = objs[i];
    if (ob.type == RT_SPHERE) sub |= SUB_SPHERE;
    if (ob.type == RT_BOX) sub |= SUB_BOX;
    if (ob.type == RT_MESH) sub |= SUB_MESH;
    if (classify_xf(ob.world_to_object, ob.object_to_world) == XF_GENERAL) sub |= SUB_XF_GENERAL;
    if (ob.reflection > 0.0) *any_reflective = true;
  }
  if (*any_reflective) sub |= SUB_REFLECT;
  return sub;
}

}  // namespace rtmi

namespace {

// Everything an object update builds before the scene changes; after the
// hand-over it holds the scene's previous state. Freed on every path.
struct ObjState {
  DevBuf<DevObject<double>> o64;
  DevBuf<FObj> fo;
  DevBuf<FObjX> fx;
  DevBuf<float> albedo32;
  DevBuf<double> albedo64;
  DevBuf<DevObjBox> objbox;
  std::vector<FObj> h_fo;
  std::vector<float> h_obj_ty;
  std::vector<rt_scene::ObjMeta> meta;
  std::vector<rt_object_desc> desc;
  std::vector<ObjBox> boxes;
  double mesh_o2w[16], mesh_w2o[16];
};

}  // namespace

extern "C" int rt_scene_set_objects(rt_scene* s, const rt_object_desc* objects, int32_t num_objects) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (num_objects < 0) return fail(RT_E_INVALID, "negative object count");
  if (num_objects > 0 && !objects) return fail(RT_E_INVALID, "null array with nonzero count");
  std::lock_guard<std::mutex> lk(s->mu);
  if (num_objects != s->nobj)
    return fail(RT_E_INVALID, "the scene has %d objects, not %d: an object update keeps the count", s->nobj,
                num_objects);
  for (int i = 0; i < num_objects; ++i) {
    const rt_scene::ObjMeta& om = s->obj_meta[(size_t)i];
    if (objects[i].type != om.type)
      return fail(RT_E_INVALID, "object %d: type %d differs from the type %d it was created with", i, objects[i].type,
                  om.type);
    if (om.type == RT_MESH && objects[i].mesh != om.mesh)
      return fail(RT_E_INVALID, "object %d: mesh %d differs from the mesh %d it was created with", i, objects[i].mesh,
                  om.mesh);
  }
  if (int rc = check_objects(objects, num_objects, s->nmesh)) return rc;
  DeviceGuard g(s->device);
  if (int rc = wait_for_calls(s)) return rc;  // they still read the old buffers
  // the records, as rt_scene_create fills them over the scene's current meshes
  int rc;
  ObjState ns;
  {
    std::vector<DevObject<double>> o64;
    std::vector<FObjX> fx;
    fill_objects<double>(objects, num_objects, o64);
    fill_fast_objects(objects, num_objects, s->h_dm32, ns.h_fo, fx);
    for (const FObj& q : ns.h_fo) ns.h_obj_ty.push_back(q.t[1]);
    std::vector<float> alb;
    fill_albedo32(objects, num_objects, alb);
    std::vector<double> alb64;
    fill_albedo64(objects, num_objects, alb64);
    if ((rc = ns.o64.upload(o64)) || (rc = ns.fo.upload(ns.h_fo)) || (rc = ns.fx.upload(fx)) ||
        (rc = ns.albedo32.upload(alb)) || (rc = ns.albedo64.upload(alb64)))
      return rc;
  }
  fill_obj_meta(objects, num_objects, ns.meta);
  ns.desc.assign(objects, objects + num_objects);
  if (s->objbins) {
    fill_obj_boxes(objects, num_objects, s->h_dm64, ns.boxes);
    std::vector<DevObjBox> ob;
    dev_obj_boxes(ns.boxes, ob);
    if ((rc = ns.objbox.upload(ob))) return rc;
  }
  std::memcpy(ns.mesh_o2w, s->mesh_o2w, sizeof ns.mesh_o2w);
  std::memcpy(ns.mesh_w2o, s->mesh_w2o, sizeof ns.mesh_w2o);
  if (s->shadow_mesh >= 0) {
    std::memcpy(ns.mesh_o2w, objects[s->shadow_mesh].object_to_world, sizeof ns.mesh_o2w);
    std::memcpy(ns.mesh_w2o, objects[s->shadow_mesh].world_to_object, sizeof ns.mesh_w2o);
  }
  // the lights over the new objects read these of the scene: staged, so that
  // a failure leaves the scene as it was
  const auto stage = [&] {
    std::swap(s->obj_meta, ns.meta);
    std::swap(s->obj_boxes, ns.boxes);
    for (int k = 0; k < 16; ++k) {
      std::swap(s->mesh_o2w[k], ns.mesh_o2w[k]);
      std::swap(s->mesh_w2o[k], ns.mesh_w2o[k]);
    }
  };
  stage();
  LightState ls;
  const bool was_timed = s->relight_timed;
  s->relight_timed = false;
  rc = build_lights(s, s->light_desc.data(), s->nlight, true, &ls);
  s->relight_timed = was_timed;
  if (rc != RT_OK) {
    stage();
    return rc;
  }
  const float keep_ms[6] = {s->relight_ms[0], s->relight_ms[1], s->relight_ms[2],
                            s->relight_ms[3], s->relight_ms[4], s->relight_ms[5]};
  adopt_lights(s, &ls);
  std::copy(keep_ms, keep_ms + 6, s->relight_ms);
  std::swap(s->f64.objects, ns.o64);
  std::swap(s->f32.objs, ns.fo);
  std::swap(s->f32.objx, ns.fx);
  std::swap(s->albedo32, ns.albedo32);
  std::swap(s->albedo64, ns.albedo64);
  if (s->objbins) std::swap(s->objbox_dev, ns.objbox);
  s->h_fo.swap(ns.h_fo);
  s->h_obj_ty.swap(ns.h_obj_ty);
  s->obj_desc.swap(ns.desc);
  bool refl = false;
  const unsigned sub = object_subset(objects, num_objects, &refl);
  const unsigned from_objects = (unsigned)SUB_XF_GENERAL | (unsigned)SUB_REFLECT;
  s->f32_subset = (s->f32_subset & ~from_objects) | (sub & from_objects);
  s->any_reflective = refl;
  s->sh64.release();  // formed from the old grids: rebuilt on demand
  s->sh64_ready = false;
  s->orders.clear();  // the measured launch orders were the old objects'
  return RT_OK;
}
