// rt_scene_mesh.cpp — rt_scene_set_mesh_vertices: a mesh's new vertices
// through the device passes of rt_mesh_gpu.hip into copies of the scene's
// arrays, handed to the scene by swapping once all of it succeeded.
#include <chrono>
#include <cmath>
#include <cstring>

#include "rt_mesh_gpu.h"
#include "rt_scene.h"

namespace {

// Everything a mesh update builds before the scene changes; after the
// hand-over it holds the scene's previous buffers. Freed on every path.
struct MeshState {
  DevBuf<double> verts, given;
  DevBuf<BvhNode> tree, nodes;
  DevBuf<TriF64> tris;
  DevBuf<float> n32;
  DevBuf<double> n64;
  DevBuf<DevBinTri> bin;
  DevBuf<DevMesh<double>> dm64;
  DevBuf<FMesh> fm;
  DevBuf<FObj> fo;
  DevBuf<DevObjBox> objbox;
};

template <class T>
int copy_dev(DevBuf<T>& dst, const DevBuf<T>& src, hipStream_t st) {
  if (int rc = dst.alloc(src.n)) return rc;
  if (src.p && src.n) HIP_TRY(hipMemcpyAsync(dst.p, src.p, src.bytes(), hipMemcpyDeviceToDevice, st));
  return RT_OK;
}

// rt_scene_set_mesh_vertices*: `vertices` / `normals` are host arrays
// (device == false) or device arrays read behind `caller`.
int set_mesh_vertices(rt_scene* s, int32_t mesh, const double* vertices, int64_t num_vertices, const double* normals,
                      bool device, hipStream_t caller) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!vertices) return fail(RT_E_INVALID, "null vertex array");
  std::lock_guard<std::mutex> lk(s->mu);
  if (mesh < 0 || mesh >= s->nmesh) return fail(RT_E_INVALID, "mesh index %d out of range (%d meshes)", mesh, s->nmesh);
  rt_scene::MeshKeep& keep = s->mesh_keep[(size_t)mesh];
  if (num_vertices != keep.nv)
    return fail(RT_E_INVALID, "mesh %d has %lld vertices, not %lld: a mesh update keeps the counts", mesh,
                (long long)keep.nv, (long long)num_vertices);
  DeviceGuard g(s->device);
  if (int wrc = wait_for_calls(s)) return wrc;  // they still read the old buffers
  const int64_t nf = keep.nf, nv = keep.nv;
  if (nf == 0) return RT_OK;
  const auto hip_fail = [](int err) {
    return fail(err == (int)hipErrorOutOfMemory ? RT_E_NOMEM : RT_E_DEVICE, "mesh update: %s",
                hipGetErrorString((hipError_t)err));
  };
  const bool timed = s->mesh_timed;
  float ms[6] = {};
  auto tp = std::chrono::steady_clock::now();
  const auto lap = [&](int k) {  // timed runs wait after every pass
    if (!timed) return;
    (void)hipStreamSynchronize(s->stream);
    const auto now = std::chrono::steady_clock::now();
    ms[k] += std::chrono::duration<float, std::milli>(now - tp).count();
    tp = now;
  };
  hipStream_t st = s->stream;
  int rc;
  MeshState ns;
  // the scene's own copy of the arrays: the caller's may be reused on return
  if ((rc = ns.verts.alloc((size_t)nv * 3))) return rc;
  if (normals && (rc = ns.given.alloc((size_t)nf * 3))) return rc;
  if (device) {
    HIP_TRY(hipMemcpyAsync(ns.verts.p, vertices, (size_t)nv * 3 * sizeof(double), hipMemcpyDeviceToDevice, caller));
    if (normals)
      HIP_TRY(hipMemcpyAsync(ns.given.p, normals, (size_t)nf * 3 * sizeof(double), hipMemcpyDeviceToDevice, caller));
    HIP_TRY(hipStreamSynchronize(caller));
  } else {
    HIP_TRY(hipMemcpy(ns.verts.p, vertices, (size_t)nv * 3 * sizeof(double), hipMemcpyHostToDevice));
    if (normals) HIP_TRY(hipMemcpy(ns.given.p, normals, (size_t)nf * 3 * sizeof(double), hipMemcpyHostToDevice));
  }
  lap(0);
  // 1. bounds and validation: read-only, nothing is written before it passes
  MeshBounds mb;
  if (int err = rtmi_mesh_bounds(ns.verts.p, nv, keep.faces.p, nf, s->mesh_scratch.p, &mb, st)) return hip_fail(err);
  double mag = 0.0, extent = 0.0;
  for (int a = 0; a < 3; ++a) {
    mag = std::max(mag, std::max(std::fabs(mb.flo[a]), std::fabs(mb.fhi[a])));
    extent = std::max(extent, mb.fhi[a] - mb.flo[a]);
  }
  if (mb.nonfinite || !std::isfinite(mag) || !std::isfinite(extent))
    return fail(RT_E_INVALID, "mesh %d: mesh has non-finite vertices", mesh);
  const double inflate = std::ldexp(std::max(extent, mag), -20) + 1e-30;  // = rt_bvh.cpp
  lap(1);
  // 2.-4. records, normals and node boxes into copies of the scene's arrays
  const int64_t nnodes = s->num_nodes;
  if ((rc = copy_dev(ns.tree, s->f32.tree, st)) || (rc = copy_dev(ns.nodes, s->nodes, st)) ||
      (rc = copy_dev(ns.tris, s->f64.tris, st)) || (rc = copy_dev(ns.n32, s->f32.normals, st)) ||
      (rc = copy_dev(ns.n64, s->f64.normals, st)))
    return rc;
  lap(2);
  TriFast* fast = reinterpret_cast<TriFast*>(ns.tree.p + nnodes) + keep.tri_base;
  if (!pack_triangles_device(ns.verts.p, keep.faces.p, keep.order.p, nf, fast, ns.tris.p + keep.tri_base, st))
    return fail(RT_E_DEVICE, "mesh %d: triangle packing failed", mesh);
  if (int err = rtmi_mesh_normals(ns.verts.p, keep.faces.p, normals ? ns.given.p : nullptr, nf,
                                  ns.n64.p + 3 * keep.tri_base, ns.n32.p + 3 * keep.tri_base, st))
    return hip_fail(err);
  lap(3);
  if (int err = rtmi_mesh_refit(ns.verts.p, keep.faces.p, keep.order.p, inflate, keep.node_base, keep.node_count,
                                keep.tri_base, s->refit_parent.p, s->refit_arrivals.p + keep.node_base, ns.nodes.p,
                                ns.tree.p, st))
    return hip_fail(err);
  lap(4);
  // 5. the binned faces, when this is the only mesh object's mesh
  const bool binned = s->shadow_mesh >= 0 && s->binnable && s->obj_meta[(size_t)s->shadow_mesh].mesh == mesh;
  if (binned) {
    if ((rc = ns.bin.alloc((size_t)nf))) return rc;
    if (int err = rtmi_mesh_bins(ns.verts.p, keep.faces.p, keep.order.p, nf,
                                 (nnodes + keep.tri_base) * (int64_t)sizeof(TriFast), ns.bin.p, st))
      return hip_fail(err);
  }
  // 6. the records that hold the mesh's box (calcAABB), as rt_scene_create fills them
  std::vector<DevMesh<float>> dm32(s->h_dm32);
  std::vector<DevMesh<double>> dm64(s->h_dm64);
  std::vector<FMesh> fm(s->h_fm);
  std::vector<FObj> fo(s->h_fo);
  std::vector<ObjBox> boxes(s->obj_boxes);
  for (int k = 0; k < 3; ++k) {
    dm32[(size_t)mesh].lo[k] = (float)mb.alo[k];
    dm32[(size_t)mesh].hi[k] = (float)mb.ahi[k];
    dm64[(size_t)mesh].lo[k] = mb.alo[k];
    dm64[(size_t)mesh].hi[k] = mb.ahi[k];
    fm[(size_t)mesh].lo[k] = dm32[(size_t)mesh].lo[k];
    fm[(size_t)mesh].hi[k] = dm32[(size_t)mesh].hi[k];
  }
  for (size_t i = 0; i < s->obj_meta.size(); ++i) {
    if (s->obj_meta[i].mesh != mesh) continue;
    for (int k = 0; k < 3; ++k) {
      fo[i].lo[k] = (float)dm32[(size_t)mesh].lo[k];
      fo[i].hi[k] = (float)dm32[(size_t)mesh].hi[k];
    }
    if (s->objbins) {
      boxes[i] = ObjBox{};
      world_obj_box(RT_MESH, s->obj_meta[i].w2o, mb.alo, mb.ahi, &boxes[i]);
    }
  }
  if ((rc = ns.dm64.upload(dm64)) || (rc = ns.fm.upload(fm)) || (rc = ns.fo.upload(fo))) return rc;
  if (s->objbins) {
    std::vector<DevObjBox> ob;
    dev_obj_boxes(boxes, ob);
    if ((rc = ns.objbox.upload(ob))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(st));
  lap(4);
  // 7. the lights over the new faces and boxes: staged, so that a failure
  // leaves the scene as it was
  double old_lo[3], old_hi[3];
  const double old_scale = s->bin_scale;
  const auto stage = [&] {
    if (binned) {
      std::swap(s->bin_dev, ns.bin);
      for (int k = 0; k < 3; ++k) {
        std::swap(s->mesh_lo[k], old_lo[k]);
        std::swap(s->mesh_hi[k], old_hi[k]);
      }
    }
    std::swap(s->obj_boxes, boxes);
  };
  for (int k = 0; k < 3; ++k) {
    old_lo[k] = mb.alo[k];
    old_hi[k] = mb.ahi[k];
  }
  stage();
  if (binned) s->bin_scale = 0.0;  // of the old faces: reduced again on demand
  LightState ls;
  const bool was_timed = s->relight_timed;
  s->relight_timed = false;
  rc = build_lights(s, s->light_desc.data(), s->nlight, true, &ls);
  s->relight_timed = was_timed;
  if (rc != RT_OK) {
    stage();
    s->bin_scale = old_scale;
    return rc;
  }
  const float keep_ms[6] = {s->relight_ms[0], s->relight_ms[1], s->relight_ms[2],
                            s->relight_ms[3], s->relight_ms[4], s->relight_ms[5]};
  adopt_lights(s, &ls);
  std::copy(keep_ms, keep_ms + 6, s->relight_ms);
  std::swap(s->f32.tree, ns.tree);
  std::swap(s->nodes, ns.nodes);
  std::swap(s->f64.tris, ns.tris);
  std::swap(s->f32.normals, ns.n32);
  std::swap(s->f64.normals, ns.n64);
  std::swap(s->f64.meshes, ns.dm64);
  std::swap(s->f32.meshes, ns.fm);
  std::swap(s->f32.objs, ns.fo);
  if (s->objbins) std::swap(s->objbox_dev, ns.objbox);
  std::swap(keep.verts, ns.verts);
  keep.normals_given = normals != nullptr;
  s->h_dm32.swap(dm32);
  s->h_dm64.swap(dm64);
  s->h_fm.swap(fm);
  s->h_fo.swap(fo);
  s->bin_tris_stale = s->bin_tris_stale || binned;
  s->sh64.release();  // formed from the old faces: rebuilt on demand
  s->sh64_ready = false;
  s->orders.clear();  // the measured launch orders were the old geometry's
  lap(5);
  if (timed) std::copy(ms, ms + 6, s->mesh_ms);
  return RT_OK;
}

}  // namespace

extern "C" int rt_scene_set_mesh_vertices(rt_scene* s, int32_t mesh, const double* vertices, int64_t num_vertices,
                                          const double* normals) {
  return set_mesh_vertices(s, mesh, vertices, num_vertices, normals, false, nullptr);
}

extern "C" int rt_scene_set_mesh_vertices_device(rt_scene* s, int32_t mesh, const double* d_vertices,
                                                 int64_t num_vertices, const double* d_normals, void* hip_stream) {
  return set_mesh_vertices(s, mesh, d_vertices, num_vertices, d_normals, true, (hipStream_t)hip_stream);
}
