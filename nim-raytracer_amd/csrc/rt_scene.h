// rt_scene.h — internal: struct rt_scene (the opaque handle of include/rtmi.h)
// and what the host units share of it: rtmi.cpp creates and destroys a scene,
// rt_scene_lights.cpp / rt_scene_mesh.cpp / rt_scene_objects.cpp change one, rt_render.cpp and
// rt_queries.cpp run calls on it, rt_hooks.cpp reads it for the tests. The
// standard headers below serve those units too.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/rtmi.h"
#include "rt_bins.h"
#include "rt_bvh.h"
#include "rt_common.h"
#include "rt_frame.h"
#include "rt_hip.h"

namespace rtmi {

template <class R>
struct PrecisionData {
  DevBuf<DevObject<R>> objects;
  DevBuf<DevLight<R>> lights;
  DevBuf<DevMesh<R>> meshes;
  DevBuf<typename TriOf<R>::type> tris;
  DevBuf<R> normals;
  size_t bytes() const {
    return objects.bytes() + lights.bytes() + meshes.bytes() + tris.bytes() + normals.bytes();
  }
};

struct FastData {
  DevBuf<FObj> objs;
  DevBuf<FObjX> objx;
  DevBuf<FMesh> meshes;
  DevBuf<FLight> lights;
  // the float32 kernel's BVH in ONE allocation: the nodes with child refs as
  // BYTE offsets into this buffer (inner child: its node, leaf: its first
  // TriFast record), then the TriFast records; one scalar base + a 32-bit
  // SGPR offset address every record (s_load ... soffset)
  DevBuf<BvhNode> tree;
  DevBuf<float> normals;
  size_t bytes() const {
    return objs.bytes() + objx.bytes() + meshes.bytes() + lights.bytes() + tree.bytes() + normals.bytes();
  }
};

// by image size: the most slots (a power of two, 2^kSlotLg .. 256) whose
// block stays within 2^27 entries
inline int slot_lg_for(int w, int h) {
  const unsigned long long npx = (unsigned long long)w * (unsigned long long)h;
  int lg = rtmi::kSlotLg;
  while (lg < 8 && (npx << (lg + 1)) <= (1ull << 27)) ++lg;
  // 4K and up: 128 (4.2 GB per buffer set at 4K). The 1M-face torus (C5)
  // lists up to 99 faces per pixel at 4K; with 64 slots its 64 fullest
  // pixels took the one-sample BVH loop at ~100x a mean pixel's cost, up
  // to ~12 ms of one wave — longer than a rank's whole call at N = 8, so
  // the 3 ranks holding the dearest of them ran 10-20 % long (rt_frame.h)
  if (npx >= (1ull << 22)) lg = std::max(lg, 7);
  return lg;
}

}  // namespace rtmi

// (internal header: every unit that includes it speaks namespace rtmi)
using namespace rtmi;

struct rt_scene {
  std::mutex mu;
  int device = 0;
  int num_cus = 256;
  // the owned streams come before every buffer: members are destroyed in
  // reverse order, so the streams outlive the buffers they worked on
  Stream stream;
  hipEvent_t done = nullptr;  // the last call's completion: its buffer set's `used` event (not owned)
  // two-class launches: the lean kernel runs on `aux`, forked from and
  // joined back into the caller's stream, so its waves take the general
  // kernel's slots as that kernel's waves drain (no tail between the two)
  Stream aux;
  Event fork, join;
  // Pipelined calls alternate between two sets of per-call buffers (Frame +
  // queue heads / Stats words): the call's camera-dependent build runs on
  // `bstream` (the device's highest stream priority), after only the call two
  // back that used the same set, so it overlaps the previous call's render
  // kernels; the render waits for its own build (Frame::built). The render's
  // persistent waves leave the build about one block per CU, so its first
  // launch stretches over the render and the other two follow it (rank 0 of
  // 8: 35 us of build in stream order, 23 us exposed when pipelined; a third
  // buffer set measured no better). A float32 call is pipelined when it renders at most
  // a third of the image (a multi-GPU rank's bands, a pool's scanlines: the
  // build is about fixed per call, the render shrinks with the launch); a
  // whole frame fills the GPU by itself and runs its build in stream order
  // (measured on C3: whole frame 0.906 ms serial vs 0.945 pipelined; rank 0
  // of 8 back to back 0.174 vs 0.163 ms). RTMI_PIPE=0 / 1 forces it off / on.
  Stream bstream;
  int pipe_mode = -1;    // RTMI_PIPE: -1 by launch size, 0 never, 1 always
  bool pipe = false;     // this call is pipelined
  // RT_FLAG_TIMING: call start, render kernels' start, call end
  Event tev[3];
  bool timed = false;
  int64_t last_lean = 0, last_general = 0;  // rt_scene_last_split
  // host copies of what the per-call uniform-pixel condition reads (uniform_cam):
  // every object's FObj.t[1], every light's FLight.v[1]
  std::vector<float> h_obj_ty, h_light_vy;
  // every light's FLight.v (3 floats each): the inset box's condition (rt_bins_geom.h inset_box)
  std::vector<float> h_light_v;
  // rt_scene_last_mesh1: the last call's general list went to gen1_loop
  // without RT_FLAG_NO_MESH1, and its straight-path batches (read_stats)
  bool mesh1 = false;
  int64_t last_straight = 0;
  int32_t last_lean_kind = 0;                // rt_scene_last_lean_kernel
  bool stats_kept = true;                    // the last call kept its Stats (no RT_FLAG_NO_STATS)
  // per-wave Stats rows of the last call not yet reduced into acc(): a call
  // whose caller does not read its Stats leaves them to the first reader
  // (rt_scene_last_stats / _last_counters), one launch fewer per call
  int32_t pending_reduce = 0;
  hipStream_t done_stream = nullptr;  // the stream `done` was last recorded on
  int64_t last_batched = 0, last_fallback = -1;  // rt_scene_last_batch
  int32_t nobj = 0, nlight = 0, nmesh = 0;
  int32_t shadow_mesh = -1;  // the only mesh object, or -1 (FastParams.shadow_mesh)
  int32_t lean64_plane = -1; // RenderParams.lean_plane of the scene (k_render_px64 lean samples)
  int32_t has_point_light = 0;
  unsigned f32_subset = 0;   // SUB_* feature bits of the scene (kernel specialisation)
  bool any_reflective = false;
  double fov = 50.0;
  double c2w[16];
  double bg[3];
  FastData f32;
  // (float)rt_object_desc.albedo of every object, nobj * 3: the feature-buffer
  // kernel's albedo channel (rt_fast_aov.h); filled by rt_scene_create,
  // refreshed by rt_scene_set_objects. aov_stage: rt_render_aovs' device
  // copies of the wanted channels.
  DevBuf<float> albedo32;
  DevBuf<unsigned char> aov_stage;
  // rt_object_desc.albedo of every object as given, nobj * 3: the float64
  // feature-buffer kernels' albedo channel (rt_kernels_aov64.hip; DevObject's
  // albp is already divided by PI); filled and refreshed as albedo32 is
  DevBuf<double> albedo64;
  PrecisionData<double> f64;
  DevBuf<BvhNode> nodes;
  DevBuf<unsigned long long> partials;
  // float32 work-queue heads (two sets of kQueueShards * kQueueStride: the
  // general and the lean kernel), then the Stats accumulator: one buffer so
  // a call clears both with one fill
  DevBuf<unsigned int> queue, queue2;  // queue2: the other set's (swapped with fr2)
  static constexpr size_t kQueueWords = (size_t)2 * kQueueShards * kQueueStride;
  unsigned long long* acc() const { return reinterpret_cast<unsigned long long*>(queue.p + kQueueWords); }
  DevBuf<double> f64_tables;       // float64 kernel per-lane stochastic sample tables
  DevBuf<float> refl_queue;        // k_render_wave's per-wave ray queues
  DevBuf<long long> refl_sec;      // k_render_wave's per-pixel secondary radiance (32.32)
  struct Order {                   // one launch mapping's measured costs -> launch order
    std::array<int64_t, 17> key;
    DevBuf<unsigned> cost;         // cycles per pixel group, written by the measuring launch
    DevBuf<int32_t> perm;          // the expensive-first order, once built
    std::vector<int32_t> host_perm;  // the same order on the host (two-class launches split it)
    Event measured;                // recorded after the measuring launch
  };
  std::vector<std::unique_ptr<Order>> orders;  // most recently used first, at most 8
  // bins of the float32 kernel (rt_bins.h), for the scene's only mesh object
  std::vector<BinTri> bin_tris;    // its faces (object space) + TriFast byte offsets
  double mesh_o2w[16], mesh_w2o[16];
  bool binnable = false;
  DevBuf<LightGrid> grids;         // per light (gu == 0: none)
  // per light with a grid: every face's shadow-test record for that light's
  // fixed direction (rt_common.h LTri, leaf order, ntri per light)
  DevBuf<LTri> lrec;
  DevBuf<LTri> grec;               // lrec in light-grid entry order (FastParams.grid_rec)
  // the float64 shadow records in light-grid entry order (RenderParams.sh64),
  // built by the first float64 call that searches the grids
  DevBuf<ShTri64> sh64;
  bool sh64_ready = false;
  int64_t lrec_ntri = 0;
  uint32_t lrec_mask = 0;          // the lights that have records
  DevBuf<int32_t> grid_off, grid_ent;
  bool has_grids = false;
  // shadow skips (rt_bins.h): scenes of the one mesh and planes
  std::vector<GridOcc> grid_occ;   // per light (g.gu == 0: none)
  std::vector<LightGridHost> grid_host;  // per light: the cell lists + face boxes the shadow lists gather from
  std::vector<SkipPlane> skip_planes;
  bool skippable = false;
  // rt_scene_set_lights: the current lights, and what build_lights reads of
  // the objects. After a relight only each grid's header (grid_occ[].g,
  // grid_host[].g) and entry count (grid_nent, padding included) are on the
  // host: the bulky mirrors (grid_host[].off / ent / box, grid_occ[].sat) are
  // stale until a test hook asks for them (refresh_host_lists).
  std::vector<rt_light_desc> light_desc;
  struct ObjMeta {
    int32_t type, mesh;
    double reflection, o2w[16], w2o[16];
  };
  std::vector<ObjMeta> obj_meta;
  // rt_scene_set_objects: the current objects as given (types and meshes as at
  // create); obj_meta and every object record are formed from them
  std::vector<rt_object_desc> obj_desc;
  std::vector<int64_t> grid_nent;
  bool mirrors_stale = false;
  double bin_scale = 0.0;          // the grids' length scale of bin_dev (0: not yet reduced)
  // rt_scene_set_mesh_vertices: what an update reads of every mesh (its
  // current vertices, its faces, its leaf order, where its records and nodes
  // lie), the tree's parent table (2 * parent + slot, -1: a root) with the
  // refit's arrival counters, and host copies of the records that hold a
  // mesh's box. bin_tris' vertices are stale after an update until a hook
  // asks for them (refresh_bin_tris). h_nodes: the nodes as created (the
  // child references; the hooks' host refit starts from them).
  struct MeshKeep {
    DevBuf<double> verts;
    DevBuf<int32_t> faces, order;
    int64_t nv = 0, nf = 0, tri_base = 0;
    int32_t node_base = 0, node_count = 0;
    bool normals_given = false;
  };
  std::vector<MeshKeep> mesh_keep;
  DevBuf<int32_t> refit_parent, refit_arrivals;
  DevBuf<unsigned long long> mesh_scratch;
  std::vector<BvhNode> h_nodes;
  std::vector<DevMesh<float>> h_dm32;
  std::vector<DevMesh<double>> h_dm64;
  std::vector<FMesh> h_fm;
  std::vector<FObj> h_fo;
  bool bin_tris_stale = false;
  bool mesh_timed = false;         // time the update's passes (rtmi_test_mesh_update_passes)
  float mesh_ms[6] = {};           // the last timed update's passes
  bool relight_timed = false;      // time the device builder's passes (rtmi_test_relight_passes)
  float relight_ms[6] = {};        // the last timed relight's passes
  // camera-dependent data of the float32 kernels (rt_frame.h): rebuilt on
  // the device by every render call; only the buffers outlive a call
  DevBuf<DevBinTri> bin_dev;       // the binned mesh's faces (float64, leaf order)
  double mesh_lo[3] = {0, 0, 0}, mesh_hi[3] = {0, 0, 0};  // its AABB (object space, calcAABB)
  DevBuf<int32_t> sat_dev;         // the light grids' occupancy prefix sums, back to back
  int64_t sat_off[8] = {};
  struct Frame {                   // per-call buffers of one image size
    int w = 0, h = 0;
    DevBuf<int32_t> cnt, slots, lean, heavy, ctr, orect;
    DevBuf<uint32_t> info, uni_cls;  // uni_cls: per tile row, the uniform classes' counts (RecordsLaunch.uni_cls)
    int uni_rows = 0;              // its words the last classifying launch wrote
    DevBuf<unsigned long long> omask, status;  // status: per-tile class counts (FrameLaunch.tile_cls)
    DevBuf<HugeFace> huge;
    DevBuf<unsigned char> tiles;   // per skip cell of a tile: shadow skips (k_frame_build1)
    int slot_lg = -1;              // slots allocated for 2^slot_lg entries per pixel (-1: none)
    int want_lg = -1;              // test hook (rtmi_test_slot_lg); -1: by image size
    uint32_t calls = 0;            // build launches (their parity picks the huge-list counter)
    bool counted = false;          // the last launch's lean / general lists were counted on the device
    bool listed = false;           // the last launch built camera-ray lists
    bool uniform = false;          // the last launch classified its lean pixels (rt_scene_last_uniform)
    bool ground = false;           // the last launch tagged its ground pixels (rt_scene_last_ground)
    Event built;                   // recorded on bstream after this set's builds of a call
    Event used;                    // recorded on the caller's stream at the end of a call that used this set
    bool used_rec = false;         // `used` has been recorded
    int id = 0;                    // which of the two sets (test hook)
    // forget the buffers: the next call re-allocates and re-zeroes them
    void invalidate() { w = h = 0; }
    size_t bytes() const {
      return cnt.bytes() + slots.bytes() + lean.bytes() + heavy.bytes() + ctr.bytes() + orect.bytes() +
             info.bytes() + uni_cls.bytes() + omask.bytes() + status.bytes() + huge.bytes() + tiles.bytes();
    }
  } fr, fr2;  // fr: this (or the last) call's set; fr2 the other one (swapped per call)
  // object bins (rt_bins.h ObjBox), scenes of 4..64 objects
  std::vector<ObjBox> obj_boxes;
  bool objbins = false;
  DevBuf<LightGrid> obj_grids;
  DevBuf<unsigned long long> obj_grid_mask;
  unsigned long long obj_off_grid = 0;
  bool has_obj_grids = false;
  bool objgrid_host = false;       // relights build the object grids on the host (rtmi_test_objgrid_pass)
  double objgrid_ms = 0.0;         // the last build's object-grid pass, wall time
  DevBuf<DevObjBox> objbox_dev;
  DevBuf<float> fb_scratch;
  // ray queries (rt_trace_rays* / rt_pick_pixels* / rt_shade_rays*): buffers of their own, so a
  // query leaves the last render call's rows, Stats and lists as they are.
  // Allocated by the first query that needs them, grown on demand (after
  // waiting for the queries that use them), released with the scene.
  DevBuf<unsigned long long> q_partials;  // [max_waves][kStatSlots] rows, then the batch's kStatSlots sums
  DevBuf<unsigned char> q_sort;           // RT_QUERY_SORT: keys, indices, bounds, rocPRIM's temporaries
  DevBuf<unsigned char> q_stage;          // host forms: the batch's device copy
  Event q_done;                           // the last query's completion (recorded on q_stream)
  hipStream_t q_stream = nullptr;
  bool q_done_rec = false;
  int q_blocks_per_cu = -1;               // k_trace_rays' resident blocks per CU
  // radiance queries (rt_shade_rays*) share all of the above, under the same
  // event discipline, and add:
  DevBuf<double> q_shade;                 // group > 1: the batch's per-ray colours (n * 3)
  int q_shade_blocks_per_cu[2] = {-1, -1};  // k_shade_rays' resident blocks per CU: one level, kMaxShadeLevels
  // float32 radiance queries (rt_shade_rays_f32*), likewise:
  DevBuf<float> q_shade32;                // group > 1: the batch's per-ray colours (n * 3)
  int q_shade32_blocks_per_cu[64] = {};   // k_shade_rays_f32's resident blocks per CU by subset; 0: not asked yet
  // float32 ray queries and picks (rt_trace_rays_f32* / rt_pick_pixels_f32*), likewise:
  int q_trace32_blocks_per_cu[16] = {};   // k_trace_rays_f32's resident blocks per CU by geometry subset; 0: not asked yet
  int max_waves = 0;
  int64_t num_triangles = 0, num_nodes = 0;
  int max_depth = 0;
  double build_ms = 0.0;

  // Everything the scene holds on the device (rt_scene_info.device_bytes):
  // the geometry and BVH of both precisions, the light grids and bins, the
  // per-call buffer sets (fr / fr2 are the bulk at 4K), what compacted
  // renders, queries and mesh updates allocated on demand, and the measured
  // launch orders. Nothing is left out: a DevBuf added above is added here.
  size_t device_bytes() const {
    size_t b = f32.bytes() + f64.bytes() + nodes.bytes() + partials.bytes() + sh64.bytes() + queue.bytes() +
               queue2.bytes() + f64_tables.bytes() + refl_queue.bytes() + refl_sec.bytes() + fb_scratch.bytes() +
               grids.bytes() + grid_off.bytes() + grid_ent.bytes() + obj_grids.bytes() + obj_grid_mask.bytes() +
               bin_dev.bytes() + sat_dev.bytes() + objbox_dev.bytes() + lrec.bytes() + grec.bytes() + fr.bytes() +
               fr2.bytes() + q_partials.bytes() + q_sort.bytes() + q_stage.bytes() + q_shade.bytes() + q_shade32.bytes() +
               refit_parent.bytes() +
               refit_arrivals.bytes() + mesh_scratch.bytes() + albedo32.bytes() + aov_stage.bytes() + albedo64.bytes();
    for (const MeshKeep& k : mesh_keep) b += k.verts.bytes() + k.faces.bytes() + k.order.bytes();
    for (const std::unique_ptr<Order>& o : orders) b += o->cost.bytes() + o->perm.bytes();
    return b;
  }
};

namespace rtmi {

// fn(begin, end) over [0, n) in contiguous chunks on up to 16 host threads
// (scene setup of million-face meshes: per-face record packing).
template <class Fn>
void parallel_for(int64_t n, Fn fn) {
  const int64_t kGrain = 1 << 15;
  const int hw = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const int nt = (int)std::min<int64_t>(hw, (n + kGrain - 1) / kGrain);
  if (nt <= 1) {
    if (n > 0) fn((int64_t)0, n);
    return;
  }
  std::vector<std::thread> pool;
  pool.reserve((size_t)nt);
  for (int t = 0; t < nt; ++t) pool.emplace_back([=, &fn] { fn(n * t / nt, n * (t + 1) / nt); });
  for (std::thread& th : pool) th.join();
}

// Everything of a scene that depends on its lights. rt_scene_create and
// rt_scene_set_lights both build one (build_lights) and hand it to the scene
// (adopt_lights), so the two cannot drift apart; after the hand-over it holds
// the scene's previous state, freed with it.
struct LightState {
  std::vector<rt_light_desc> desc;
  int32_t has_point_light = 0;
  std::vector<float> h_light_vy, h_light_v;
  DevBuf<FLight> f32_lights;
  DevBuf<DevLight<double>> f64_lights;
  DevBuf<LightGrid> grids;
  DevBuf<LTri> lrec, grec;
  int64_t lrec_ntri = 0;
  uint32_t lrec_mask = 0;
  DevBuf<int32_t> grid_off, grid_ent;
  bool has_grids = false;
  std::vector<GridOcc> grid_occ;
  std::vector<LightGridHost> grid_host;
  std::vector<int64_t> grid_nent;
  bool mirrors_stale = false;
  std::vector<SkipPlane> skip_planes;
  bool skippable = false;
  int32_t lean64_plane = -1;
  DevBuf<int32_t> sat_dev;
  int64_t sat_off[8] = {};
  DevBuf<LightGrid> obj_grids;
  DevBuf<unsigned long long> obj_grid_mask;
  unsigned long long obj_off_grid = 0;
  bool has_obj_grids = false;
  float ms[6] = {};
  double objgrid_ms = 0.0;
};

struct Mapping {
  int mode, y0, nrows, ncols, step, max_step, band_h, rank, world;
};

// rtmi.cpp
void world_obj_box(int32_t type, const double* w2o, const double lo[3], const double hi[3], ObjBox* out);
void dev_obj_boxes(const std::vector<ObjBox>& boxes, std::vector<DevObjBox>& ob);
// Waits for the scene's earlier calls, which may still read buffers the
// caller is about to replace or free: renders (done, the scene's stream), a
// pipelined call's build (bstream reads grids and sat_dev), queries.
int wait_for_calls(rt_scene* s);

// rt_scene_objects.cpp: everything of a scene that is formed from its objects'
// descriptions alone (and the meshes' boxes and roots). rt_scene_create and
// rt_scene_set_objects both fill through these, so the two cannot drift apart.
bool affine(const double* m);
int32_t classify_xf(const double* w2o, const double* o2w);
// RT_E_INVALID / RT_E_UNSUPPORTED with the object's index, as rt_scene_create reports them
int check_objects(const rt_object_desc* objs, int32_t n, int32_t num_meshes);
template <class R>
void fill_objects(const rt_object_desc* objs, int32_t n, std::vector<DevObject<R>>& out);
void fill_fast_objects(const rt_object_desc* objs, int32_t n, const std::vector<DevMesh<float>>& dm,
                       std::vector<FObj>& fo, std::vector<FObjX>& fx);
// (float)albedo[c] of every object, n * 3 (rt_scene::albedo32)
void fill_albedo32(const rt_object_desc* objs, int32_t n, std::vector<float>& out);
// albedo[c] of every object as given, n * 3 (rt_scene::albedo64)
void fill_albedo64(const rt_object_desc* objs, int32_t n, std::vector<double>& out);
// the bin boxes (rt_bins.h ObjBox); dm: the meshes' boxes in float64 (calcAABB)
void fill_obj_boxes(const rt_object_desc* objs, int32_t n, const std::vector<DevMesh<double>>& dm,
                    std::vector<ObjBox>& boxes);
void fill_obj_meta(const rt_object_desc* objs, int32_t n, std::vector<rt_scene::ObjMeta>& meta);
// the SUB_SPHERE / SUB_BOX / SUB_MESH / SUB_XF_GENERAL / SUB_REFLECT bits
unsigned object_subset(const rt_object_desc* objs, int32_t n, bool* any_reflective);

// rt_scene_lights.cpp
template <class R>
void fill_lights(const rt_light_desc* src, int32_t n, std::vector<DevLight<R>>& lights);
void fill_fast_lights(const rt_light_desc* src, int32_t n, std::vector<FLight>& fl);
int refresh_bin_tris(rt_scene* s);
int build_lights(rt_scene* s, const rt_light_desc* lights, int32_t nl, bool device, LightState* L);
void adopt_lights(rt_scene* s, LightState* L);
void refresh_host_lists(rt_scene* s);

// rt_render.cpp
void uniform_cam(float ty, const float* light_vy, const FastParams& p, bg::UniformCam& u);
void fast_camera(const double* c2w, double fov, const rt_options* o, FastParams& p);
unsigned f32_subset(const rt_scene* s, const rt_options* o);
// The words of a FastParams that depend on the scene alone: the geometry,
// lights, tree and normals, bg, the counts, has_point_light, shadow_mesh, the
// shadow-ray records and — unless opt_flags has RT_FLAG_NO_BINNING — the light
// and object grids. fill_fast (a render call) and shade32_device (a float32
// radiance query) both fill them here, so the two cannot drift apart.
void fast_scene_words(const rt_scene* s, uint32_t opt_flags, FastParams& p);

}  // namespace rtmi
