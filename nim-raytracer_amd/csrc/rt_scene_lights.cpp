// rt_scene_lights.cpp — everything of a scene that depends on its lights:
// built by rt_scene_create and rt_scene_set_lights alike (build_lights) and
// handed to the scene by swapping (adopt_lights).
#include <chrono>
#include <cmath>
#include <cstring>

#include "rt_lights_gpu.h"
#include "rt_scene.h"

namespace rtmi {

// The lights' records of the parity kernels (DevLight) and of the float32
// kernels (FLight): rt_scene_create and rt_scene_set_lights form the same.
template <class R>
void fill_lights(const rt_light_desc* src, int32_t n, std::vector<DevLight<R>>& lights) {
  lights.assign((size_t)n, DevLight<R>{});
  for (int i = 0; i < n; ++i) {
    const rt_light_desc& s = src[i];
    DevLight<R>& l = lights[(size_t)i];
    // color * intensity, computed in float64 like light.nim:50,57
    for (int k = 0; k < 3; ++k) l.ci[k] = (R)(s.color[k] * s.intensity);
    for (int k = 0; k < 3; ++k) l.v[k] = (R)(s.type == RT_POINT_LIGHT ? s.pos[k] : s.dir[k]);
    l.type = s.type == RT_POINT_LIGHT ? LIGHT_POINT : LIGHT_DISTANT;
  }
}
template void fill_lights<float>(const rt_light_desc*, int32_t, std::vector<DevLight<float>>&);
template void fill_lights<double>(const rt_light_desc*, int32_t, std::vector<DevLight<double>>&);
void fill_fast_lights(const rt_light_desc* src, int32_t n, std::vector<FLight>& fl) {
  fl.assign((size_t)n, FLight{});
  for (int i = 0; i < n; ++i) {
    const rt_light_desc& s = src[i];
    fl[(size_t)i].type = s.type == RT_POINT_LIGHT ? LIGHT_POINT : LIGHT_DISTANT;
    for (int k = 0; k < 3; ++k) {
      fl[(size_t)i].ci[k] = (float)(s.color[k] * s.intensity);
      fl[(size_t)i].v[k] = (float)(s.type == RT_POINT_LIGHT ? s.pos[k] : s.dir[k]);
    }
  }
}

// bin_tris' vertices after a mesh update, for the host builders and the
// hooks that read them: bin_dev holds the same records.
int refresh_bin_tris(rt_scene* s) {
  if (!s->bin_tris_stale) return RT_OK;
  HIP_TRY(hipMemcpy(s->bin_tris.data(), s->bin_dev.p, s->bin_tris.size() * sizeof(BinTri), hipMemcpyDeviceToHost));
  s->bin_tris_stale = false;
  return RT_OK;
}

}  // namespace rtmi

namespace {

// The distant lights' mesh grids, records and prefix sums by the host
// builders (rt_bins.cpp): rt_scene_create's path.
int mesh_grids_host(rt_scene* s, const rt_light_desc* lights, int32_t nl, LightState* L, bool* any_out) {
  if (int rrc = refresh_bin_tris(s)) return rrc;
  const int64_t nnodes = s->num_nodes, ntri = s->num_triangles;
  int rc;
  std::vector<LightGrid> gh((size_t)std::max(1, nl), LightGrid{});
  std::vector<int32_t> goff, gent;
  bool any = false;
  for (int li = 0; s->binnable && li < nl; ++li) {
    if (lights[li].type == RT_POINT_LIGHT) continue;
    LightGridHost lg;
    const char* why = "";
    if (!build_light_grid(s->bin_tris, s->mesh_w2o, lights[li].dir, &lg, &why)) continue;
    if ((int64_t)goff.size() + (int64_t)lg.off.size() > INT32_MAX ||
        (int64_t)gent.size() + (int64_t)lg.ent.size() > INT32_MAX)
      break;
    lg.g.off_base = (int32_t)goff.size();
    lg.g.ent_base = (int32_t)gent.size();
    goff.insert(goff.end(), lg.off.begin(), lg.off.end());
    gent.insert(gent.end(), lg.ent.begin(), lg.ent.end());
    gh[(size_t)li] = lg.g;
    grid_occupancy(lg, &L->grid_occ[(size_t)li]);
    L->grid_nent[(size_t)li] = (int64_t)lg.ent.size();
    L->grid_host[(size_t)li] = std::move(lg);
    L->grid_occ[(size_t)li].lists = &L->grid_host[(size_t)li];
    any = true;
  }
  *any_out = any;
  if (!any) return RT_OK;
  if ((rc = L->grids.upload(gh)) || (rc = L->grid_off.upload(goff)) || (rc = L->grid_ent.upload(gent))) return rc;
  // the shadow-test records of the lights with a grid (the float32
  // kernels' every shadow ray to such a light tests these, on every path)
  const size_t nt = (size_t)ntri;  // indexed like the TriFast records: byte offset / 64 - nnodes
  // every slot starts as the culled sentinel make_ltri writes for a face
  // that can never pass (u = v = t = -1): an all-zero record would read
  // as a hit at t = 0 (u = v = 0 passes min(u, v, 1-u-v) >= 0) if a
  // future path read a slot of another mesh's face or of a light with
  // no grid
  const LTri culled = bg::culled_ltri();
  std::vector<LTri> lr((size_t)nl * nt, culled);
  for (int li = 0; li < nl; ++li) {
    if (gh[(size_t)li].gu <= 0) continue;
    const double* dir = lights[li].dir;
    double sd[3], ld[3];
    for (int k = 0; k < 3; ++k) sd[k] = -dir[k];
    bg::xform_dir(s->mesh_w2o, sd, ld);  // the shadow direction in the mesh's object space
    parallel_for((int64_t)s->bin_tris.size(), [&](int64_t b, int64_t e) {
      for (int64_t i = b; i < e; ++i) {
        const BinTri& t = s->bin_tris[(size_t)i];
        const int64_t slot = (int64_t)t.rec / (int64_t)sizeof(TriFast) - nnodes;
        bg::make_ltri(t.v, ld, t.face, &lr[(size_t)li * nt + (size_t)slot]);
      }
    });
  }
  if ((rc = L->lrec.upload(lr))) return rc;
  // the cell-ordered copy: entry e of light li's grid -> its face's record
  std::vector<LTri> gr(gent.size(), culled);
  for (int li = 0; li < nl; ++li) {
    if (gh[(size_t)li].gu <= 0) continue;
    const size_t e0 = (size_t)gh[(size_t)li].ent_base, ne = L->grid_host[(size_t)li].ent.size();
    parallel_for((int64_t)ne, [&](int64_t b, int64_t e) {
      for (int64_t k = b; k < e; ++k) {
        const int64_t slot = (int64_t)gent[e0 + (size_t)k] / (int64_t)sizeof(TriFast) - nnodes;
        gr[e0 + (size_t)k] = lr[(size_t)li * nt + (size_t)slot];
      }
    });
  }
  if ((rc = L->grec.upload(gr))) return rc;
  // the occupancy prefix sums the per-call shadow skips read (rt_frame.h)
  std::vector<int32_t> sat;
  for (int li = 0; li < std::min(8, nl); ++li) {
    L->sat_off[li] = (int64_t)sat.size();
    sat.insert(sat.end(), L->grid_occ[(size_t)li].sat.begin(), L->grid_occ[(size_t)li].sat.end());
  }
  if (sat.empty()) sat.push_back(0);
  return L->sat_dev.upload(sat);
}

// The same arrays, byte for byte, by the device builder (rt_lights_gpu.hip)
// from the resident faces: rt_scene_set_lights' path. Only each grid's header
// and entry count come back to the host.
int mesh_grids_device(rt_scene* s, const rt_light_desc* lights, int32_t nl, LightState* L, bool* any_out) {
  *any_out = false;
  if (!s->binnable) return RT_OK;
  bool distant = false;
  for (int li = 0; li < nl; ++li) distant = distant || lights[li].type != RT_POINT_LIGHT;
  if (!distant) return RT_OK;
  const int64_t ntri = s->num_triangles;
  const auto hip_fail = [](int e) {
    return fail(e == (int)hipErrorOutOfMemory ? RT_E_NOMEM : RT_E_DEVICE, "light grid build: %s",
                hipGetErrorString((hipError_t)e));
  };
  int rc;
  if (!(s->bin_scale > 0.0)) {  // the faces do not change: reduced once per scene
    double sc = 1.0;
    if (int e = rtmi_lights_scale(s->bin_dev.p, (int64_t)s->bin_tris.size(), &sc, s->stream)) return hip_fail(e);
    s->bin_scale = sc;
  }
  std::vector<LightGridDev> dg((size_t)nl);
  for (LightGridDev& g : dg) std::memset(&g, 0, sizeof g);
  struct FreeGrids {
    std::vector<LightGridDev>& v;
    ~FreeGrids() {
      for (LightGridDev& g : v) rtmi_lights_free(&g);
    }
  } free_grids{dg};
  if ((rc = L->lrec.alloc((size_t)nl * (size_t)ntri))) return rc;
  if (int e = rtmi_lights_fill_culled(L->lrec.p, (int64_t)nl * ntri, s->stream)) return hip_fail(e);
  const bool timed = s->relight_timed;
  std::vector<LightGrid> gh((size_t)std::max(1, nl), LightGrid{});
  int64_t noff = 0, nent = 0;
  bool any = false;
  for (int li = 0; li < nl; ++li) {
    if (lights[li].type == RT_POINT_LIGHT) continue;
    LightGridJob job;
    job.tris = s->bin_dev.p;
    job.n = (int64_t)s->bin_tris.size();
    job.rec0 = s->bin_tris[0].rec;
    std::memcpy(job.w2o, s->mesh_w2o, sizeof job.w2o);
    for (int k = 0; k < 3; ++k) job.dir[k] = lights[li].dir[k];
    job.scale = s->bin_scale;
    job.density = light_grid_density();
    job.nnodes = s->num_nodes;
    job.ntri = ntri;
    job.lrec = L->lrec.p + (size_t)li * (size_t)ntri;
    LightGridDev& g = dg[(size_t)li];
    if (int e = rtmi_light_grid_build(&job, &g, timed ? 1 : 0, s->stream)) return hip_fail(e);
    if (!g.built) continue;
    if (noff + g.noff > INT32_MAX || nent + g.nent > INT32_MAX) {
      // as the host: this light and every later one go without a grid
      if (int e = rtmi_lights_fill_culled(job.lrec, ntri, s->stream)) return hip_fail(e);
      rtmi_lights_free(&g);
      g.built = 0;
      break;
    }
    g.g.off_base = (int32_t)noff;
    g.g.ent_base = (int32_t)nent;
    noff += g.noff;
    nent += g.nent;
    gh[(size_t)li] = g.g;
    L->grid_occ[(size_t)li].g = g.g;
    L->grid_host[(size_t)li].g = g.g;
    L->grid_nent[(size_t)li] = g.nent;
    for (int k = 0; k < 6; ++k) L->ms[k] += g.ms[k];
    any = true;
  }
  *any_out = any;
  if (!any) {
    L->lrec.release();
    return RT_OK;
  }
  L->mirrors_stale = true;
  if ((rc = L->grids.upload(gh)) || (rc = L->grid_off.alloc((size_t)noff)) || (rc = L->grid_ent.alloc((size_t)nent)) ||
      (rc = L->grec.alloc((size_t)nent)))
    return rc;
  int64_t nsat = 0;
  for (int li = 0; li < std::min(8, nl); ++li) {
    L->sat_off[li] = nsat;
    if (dg[(size_t)li].built) nsat += dg[(size_t)li].nsat;
  }
  if ((rc = L->sat_dev.alloc((size_t)std::max<int64_t>(1, nsat)))) return rc;
  if (nsat == 0) HIP_TRY(hipMemset(L->sat_dev.p, 0, sizeof(int32_t)));
  for (int li = 0; li < nl; ++li) {
    const LightGridDev& g = dg[(size_t)li];
    if (!g.built) continue;
    HIP_TRY(hipMemcpy(L->grid_off.p + g.g.off_base, g.off, (size_t)g.noff * sizeof(int32_t), hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(L->grid_ent.p + g.g.ent_base, g.ent, (size_t)g.nent * sizeof(int32_t), hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(L->grec.p + g.g.ent_base, g.grec, (size_t)g.nent * sizeof(LTri), hipMemcpyDeviceToDevice));
    if (li < 8)
      HIP_TRY(hipMemcpy(L->sat_dev.p + L->sat_off[li], g.sat, (size_t)g.nsat * sizeof(int32_t), hipMemcpyDeviceToDevice));
  }
  HIP_TRY(hipDeviceSynchronize());
  return RT_OK;
}

// The object light grids (rt_bins.h) by the device builder
// (rt_objgrid_gpu.hip): the host plans every distant light's grid (header,
// cell rectangles, hulls: at most 64 objects each) and one launch writes all
// the masks; byte for byte what build_lights' host loop uploads.
int object_grids_device(rt_scene* s, const rt_light_desc* lights, int32_t nl, LightState* L) {
  std::vector<LightGrid> gh((size_t)std::max(1, nl), LightGrid{});
  std::vector<ObjGridLight> gl;
  std::vector<ObjGridRec> recs;
  int64_t nmask = 0;
  int32_t max_cells = 0;
  for (int li = 0; li < nl; ++li) {
    if (lights[li].type == RT_POINT_LIGHT) continue;
    ObjGridPlan pl;
    const char* why = "";
    if (!plan_object_light_grid(s->obj_boxes, lights[li].dir, &pl, &why)) continue;
    const int64_t ncell = (int64_t)pl.g.gu * (int64_t)pl.g.gv;
    if (nmask + ncell > INT32_MAX) break;  // as the host: this light and every later one go without
    pl.g.off_base = (int32_t)nmask;
    gh[(size_t)li] = pl.g;
    ObjGridLight q;
    std::memset(&q, 0, sizeof q);
    q.u0 = (double)pl.g.u0;
    q.v0 = (double)pl.g.v0;
    q.hc = 1.0 / (double)pl.g.inv_h;
    q.delta = pl.delta;
    q.gu = pl.g.gu;
    q.gv = pl.g.gv;
    q.mask_base = (int32_t)nmask;
    q.rec_base = (int32_t)recs.size();
    q.nrec = (int32_t)pl.rec.size();
    gl.push_back(q);
    recs.insert(recs.end(), pl.rec.begin(), pl.rec.end());
    nmask += ncell;
    max_cells = std::max(max_cells, (int32_t)ncell);
    L->obj_off_grid = pl.off_grid;  // the same set (the unbounded objects) for every light
  }
  if (gl.empty()) return RT_OK;
  int rc;
  DevBuf<ObjGridLight> d_gl;
  DevBuf<ObjGridRec> d_rec;
  if ((rc = L->obj_grids.upload(gh)) || (rc = L->obj_grid_mask.alloc((size_t)nmask)) || (rc = d_gl.upload(gl)) ||
      (rc = d_rec.upload(recs)))
    return rc;
  if (int e = rtmi_object_grids_build(d_gl.p, (int32_t)gl.size(), max_cells, d_rec.p, L->obj_off_grid,
                                      L->obj_grid_mask.p, s->stream))
    return fail(e == (int)hipErrorOutOfMemory ? RT_E_NOMEM : RT_E_DEVICE, "object grid build: %s",
                hipGetErrorString((hipError_t)e));
  L->has_obj_grids = true;
  return RT_OK;
}

}  // namespace

namespace rtmi {

// Builds the scene's light-dependent state for `lights` into *L; reads only
// what does not depend on the lights (the faces, the objects, the BVH sizes).
// device: the mesh light grids and the object light grids by the device
// builders, else by the host's.
int build_lights(rt_scene* s, const rt_light_desc* lights, int32_t nl, bool device, LightState* L) {
  int rc;
  L->desc.assign(lights, lights + nl);
  for (int i = 0; i < nl; ++i)
    if (lights[i].type == RT_POINT_LIGHT) L->has_point_light = 1;
  {
    std::vector<FLight> fl;
    std::vector<DevLight<double>> dl;
    fill_fast_lights(lights, nl, fl);
    fill_lights<double>(lights, nl, dl);
    for (const FLight& q : fl) {
      L->h_light_vy.push_back(q.v[1]);
      L->h_light_v.insert(L->h_light_v.end(), q.v, q.v + 3);
    }
    if ((rc = L->f32_lights.upload(fl)) || (rc = L->f64_lights.upload(dl))) return rc;
  }
  const int nobj = (int)s->obj_meta.size();
  if (s->shadow_mesh >= 0) {  // light grids of the distant lights over the only mesh object
    L->grid_occ.assign((size_t)nl, GridOcc{});
    L->grid_host.assign((size_t)nl, LightGridHost{});
    L->grid_nent.assign((size_t)nl, 0);
    bool any = false;
    if ((rc = device ? mesh_grids_device(s, lights, nl, L, &any) : mesh_grids_host(s, lights, nl, L, &any))) return rc;
    if (any) {
      L->has_grids = true;
      L->lrec_ntri = s->num_triangles;
      for (int li = 0; li < nl && li < 32; ++li)
        if (L->grid_occ[(size_t)li].g.gu > 0) L->lrec_mask |= 1u << li;
      // shadow skips: every other object a plane
      L->skippable = true;
      for (int i = 0; i < nobj; ++i) {
        const rt_scene::ObjMeta& o = s->obj_meta[(size_t)i];
        if (i == s->shadow_mesh) continue;
        SkipPlane sp;
        L->skippable = L->skippable && o.type == RT_PLANE;
        std::memcpy(sp.o2w, o.o2w, sizeof sp.o2w);
        std::memcpy(sp.w2o, o.w2o, sizeof sp.w2o);
        L->skip_planes.push_back(sp);
      }
      if (!L->skippable) L->skip_planes.clear();
      // k_render_px64's lean samples: one mesh + one non-reflective plane,
      // distant lights only (each with a skip bit)
      if (L->skippable && nobj == 2 && nl >= 1 && nl <= 8) {
        const int pl = 1 - s->shadow_mesh;
        bool ok = s->obj_meta[(size_t)pl].type == RT_PLANE && !(s->obj_meta[(size_t)pl].reflection > 0.0);
        for (int li = 0; li < nl; ++li) ok = ok && lights[li].type != RT_POINT_LIGHT;
        if (ok) L->lean64_plane = pl;
      }
    }
  }
  const auto t_obj = std::chrono::steady_clock::now();
  if (s->objbins && device && !s->objgrid_host) {
    if ((rc = object_grids_device(s, lights, nl, L))) return rc;
  } else if (s->objbins) {  // the object light grids (rt_bins.h): at most 64 boxes, built on the host
    std::vector<LightGrid> gh((size_t)std::max(1, nl), LightGrid{});
    std::vector<unsigned long long> gm;
    bool any = false;
    for (int li = 0; li < nl; ++li) {
      if (lights[li].type == RT_POINT_LIGHT) continue;
      ObjGridHost og;
      const char* why = "";
      if (!build_object_light_grid(s->obj_boxes, lights[li].dir, &og, &why)) continue;
      if ((int64_t)gm.size() + (int64_t)og.masks.size() > INT32_MAX) break;
      og.g.off_base = (int32_t)gm.size();
      gm.insert(gm.end(), og.masks.begin(), og.masks.end());
      gh[(size_t)li] = og.g;
      L->obj_off_grid = og.off_grid;  // the same set (the unbounded objects) for every light
      any = true;
    }
    if (any) {
      if ((rc = L->obj_grids.upload(gh)) || (rc = L->obj_grid_mask.upload(gm))) return rc;
      L->has_obj_grids = true;
    }
  }
  L->objgrid_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_obj).count();
  return RT_OK;
}

// Hands *L to the scene; *L takes the scene's previous state.
void adopt_lights(rt_scene* s, LightState* L) {
  s->nlight = (int32_t)L->desc.size();
  std::swap(s->light_desc, L->desc);
  s->has_point_light = L->has_point_light;
  s->f32_subset = (s->f32_subset & ~(unsigned)SUB_POINT) | (s->has_point_light ? (unsigned)SUB_POINT : 0u);
  std::swap(s->h_light_vy, L->h_light_vy);
  std::swap(s->h_light_v, L->h_light_v);
  std::swap(s->f32.lights, L->f32_lights);
  std::swap(s->f64.lights, L->f64_lights);
  std::swap(s->grids, L->grids);
  std::swap(s->lrec, L->lrec);
  std::swap(s->grec, L->grec);
  s->lrec_ntri = L->lrec_ntri;
  s->lrec_mask = L->lrec_mask;
  std::swap(s->grid_off, L->grid_off);
  std::swap(s->grid_ent, L->grid_ent);
  s->has_grids = L->has_grids;
  std::swap(s->grid_occ, L->grid_occ);
  std::swap(s->grid_host, L->grid_host);
  // the lists point into grid_host, which moved with its buffer
  for (size_t li = 0; li < s->grid_occ.size(); ++li)
    s->grid_occ[li].lists = s->grid_occ[li].lists ? &s->grid_host[li] : nullptr;
  std::swap(s->grid_nent, L->grid_nent);
  s->mirrors_stale = L->mirrors_stale;
  std::swap(s->skip_planes, L->skip_planes);
  s->skippable = L->skippable;
  s->lean64_plane = L->lean64_plane;
  std::swap(s->sat_dev, L->sat_dev);
  std::memcpy(s->sat_off, L->sat_off, sizeof s->sat_off);
  std::swap(s->obj_grids, L->obj_grids);
  std::swap(s->obj_grid_mask, L->obj_grid_mask);
  s->obj_off_grid = L->obj_off_grid;
  s->has_obj_grids = L->has_obj_grids;
  std::memcpy(s->relight_ms, L->ms, sizeof s->relight_ms);
  s->objgrid_ms = L->objgrid_ms;
}

// The bulky host mirrors of the light grids (cell lists, face boxes, prefix
// sums) after a relight, for the test hooks that read them: the host builder
// forms what the device built (rtmi_test_relight_diff checks that it does).
void refresh_host_lists(rt_scene* s) {
  if (!s->mirrors_stale) return;
  (void)refresh_bin_tris(s);
  for (size_t li = 0; li < s->grid_occ.size(); ++li) {
    const LightGrid kept = s->grid_occ[li].g;
    if (kept.gu <= 0) continue;
    LightGridHost lg;
    const char* why = "";
    if (!build_light_grid(s->bin_tris, s->mesh_w2o, s->light_desc[li].dir, &lg, &why)) continue;
    lg.g.off_base = kept.off_base;
    lg.g.ent_base = kept.ent_base;
    grid_occupancy(lg, &s->grid_occ[li]);
    s->grid_host[li] = std::move(lg);
    s->grid_occ[li].lists = &s->grid_host[li];
  }
  s->mirrors_stale = false;
}

}  // namespace rtmi

extern "C" int rt_scene_set_lights(rt_scene* s, const rt_light_desc* lights, int32_t num_lights) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (num_lights < 0) return fail(RT_E_INVALID, "negative light count");
  if (num_lights > 0 && !lights) return fail(RT_E_INVALID, "null array with nonzero count");
  for (int i = 0; i < num_lights; ++i)
    if (lights[i].type != RT_DISTANT_LIGHT && lights[i].type != RT_POINT_LIGHT)
      return fail(RT_E_INVALID, "light %d: bad type", i);
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  if (int rc = wait_for_calls(s)) return rc;  // they still read the old buffers
  // everything into new buffers; the scene changes only when all of it succeeded
  LightState ls;  // then the old state (or the failed build's), freed on return
  const int rc = build_lights(s, lights, num_lights, true, &ls);
  if (rc == RT_OK) {
    adopt_lights(s, &ls);
    s->sh64.release();  // sized by grid_ent, formed from the lights' directions: rebuilt on demand
    s->sh64_ready = false;
    s->orders.clear();  // the measured launch orders were the old lights'
  }
  return rc;
}
