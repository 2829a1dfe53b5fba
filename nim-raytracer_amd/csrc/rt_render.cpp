// rt_render.cpp — the render calls: options, launch plan and order, the
// per-call camera-dependent build, the kernel launches (rt_render_*), and
// the readers of what the last call left (rt_scene_last_*).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rt_aov64.h"
#include "rt_scene.h"
#include "rt_stage.h"

namespace rtmi {

// The uniform-pixel proof's inputs (rt_bins_geom.h uniform_class): the
// float32 values lean1q_loop computes with, and the call's condition for
// uniform-lit pixels (in float32, as the kernel forms nroy).
// ty: the plane's FObj::t[1]; light_vy: every light's FLight::v[1].
void uniform_cam(float ty, const float* light_vy, const FastParams& p, bg::UniformCam& u) {
  const float oy = p.cam[1];
  const float nroy = -(oy + ty);
  u.on = 1;
  u.m = p.grid_m;
  u.cam_a = p.cam_a;
  u.cam_b = p.cam_b;
  u.cam_c = p.cam_c;
  u.cam_d = p.cam_d;
  u.c4 = p.cam[4];
  u.c7 = p.cam[7];
  u.c10 = p.cam[10];
  u.st = p.sample_step;
  u.of = p.sample_off;
  u.nroy = nroy;
  bool ok = p.bias >= 1e-30f &&
            (double)p.bias > 16.0 * 1.1920928955078125e-7 *
                                 ((double)std::fabs(oy) + (double)std::fabs(ty) + (double)std::fabs(nroy));
  for (int l = 0; l < p.nlight; ++l) {
    const float sdy = -light_vy[l];
    ok = ok && sdy > 1e-6f && sdy <= 1e6f;
  }
  u.lit_ok = ok ? 1 : 0;
}

// The camera, sample-grid and bias words of FastParams: what every float32
// kernel forms its camera rays from, and all the uniform-pixel proof reads of
// a call (uniform_cam; the test hook rtmi_test_uniform forms them here too).
void fast_camera(const double* c2w, double fov, const rt_options* o, FastParams& p) {
  // camera: origin = C2W * (0,0,0,1) = column 3; dir = C2W * normalize(cx, cy, -1, 0)
  for (int k = 0; k < 3; ++k) {
    p.cam[k] = (float)c2w[12 + k];
    p.cam[3 + k] = (float)c2w[0 + k];
    p.cam[6 + k] = (float)c2w[4 + k];
    p.cam[9 + k] = (float)c2w[8 + k];
  }
  const double f = std::tan(fov * (3.14159265358979323846 / 180.0) / 2);
  const double r = (double)o->width / (double)o->height;
  p.cam_a = (float)(2.0 * r * f / (double)o->width);  // cx = ((2 x r)/w - r) f = (x - w/2) 2rf/w
  p.cam_b = (float)(0.5 * (double)o->width);
  p.cam_c = (float)(2.0 * f / (double)o->height);     // cy = (1 - 2y/h) f = (h/2 - y) 2f/h
  p.cam_d = (float)(0.5 * (double)o->height);
  p.bias = (float)o->bias;
  const int m = o->aa_kind != RT_AA_NONE ? o->grid_size : 1;
  const int spp = m * m;
  p.inv_len = (float)(1.0 / (double)spp);
  p.sample_step = (float)(1.0 / (double)m);
  p.sample_off = (float)(1.0 / (double)m * 0.5);
  p.log2_grid_m = -1;
  for (int k = 0; k <= 12; ++k)
    if (m == (1 << k)) p.log2_grid_m = k;
  p.width = o->width;
  p.height = o->height;
  p.aa_kind = o->aa_kind;
  p.grid_m = m;
  p.spp = spp;
}

// The float32 kernel specialisation of a launch: the scene's features plus
// stochastic sampling when the options ask for it.
unsigned f32_subset(const rt_scene* s, const rt_options* o) {
  return s->f32_subset | (o->aa_kind >= RT_AA_JITTERED ? SUB_STOCHASTIC : 0u);
}

void fast_scene_words(const rt_scene* s, uint32_t opt_flags, FastParams& p) {
  p.objs = s->f32.objs.p;
  p.objx = s->f32.objx.p;
  p.meshes = s->f32.meshes.p;
  p.lights = s->f32.lights.p;
  p.tree = s->f32.tree.p;
  p.normals = s->f32.normals.p;
  for (int k = 0; k < 3; ++k) p.bg[k] = (float)s->bg[k];
  p.nobj = s->nobj;
  p.nlight = s->nlight;
  p.has_point_light = s->has_point_light;
  p.shadow_mesh = s->shadow_mesh;
  // the shadow-ray records: on every path (binned or not), so every path
  // tests a distant light's shadow rays with the same arithmetic
  if (s->lrec.p) {
    p.lrec_base = (uint64_t)(uintptr_t)s->lrec.p - (uint64_t)s->num_nodes * sizeof(TriFast);
    p.lrec_stride = s->lrec_ntri * (int64_t)sizeof(LTri);
    p.lrec_mask = s->lrec_mask;
    p.grid_rec = s->grec.p;
  }
  // binned searches (rt_bins.h) of shadow rays to distant lights
  if (!(opt_flags & RT_FLAG_NO_BINNING)) {
    if (s->has_grids) {
      p.grids = s->grids.p;
      p.grid_off = s->grid_off.p;
      p.grid_ent = s->grid_ent.p;
    }
    if (s->has_obj_grids) {
      p.obj_grids = s->obj_grids.p;
      p.obj_grid_mask = s->obj_grid_mask.p;
      p.obj_off_grid = s->obj_off_grid;
    }
  }
}

}  // namespace rtmi

namespace {

bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

int check_options(const rt_scene* s, const rt_options* o) {
  if (!o) return fail(RT_E_INVALID, "null options");
  if (o->width <= 0 || o->height <= 0 || o->width > 65536 || o->height > 65536)
    return fail(RT_E_INVALID, "bad image size %dx%d", o->width, o->height);
  if (o->aa_kind < RT_AA_NONE || o->aa_kind > RT_AA_CORRELATED_MULTI_JITTERED)
    return fail(RT_E_INVALID, "bad aa_kind %d", o->aa_kind);
  if (o->aa_kind != RT_AA_NONE && (o->grid_size < 1 || o->grid_size > 256))
    return fail(RT_E_INVALID, "grid_size %d out of range [1, 256]", o->grid_size);
  if (o->precision != RT_FP32 && o->precision != RT_FP64) return fail(RT_E_INVALID, "bad precision");
  // the float32 kernel builds a (multi-)jittered table in LDS per pixel:
  // 8 KB per wave at m = 32
  if (o->precision == RT_FP32 && o->aa_kind >= RT_AA_MULTI_JITTERED && o->grid_size > 32)
    return fail(RT_E_UNSUPPORTED, "float32 (multi-)jittered sampling supports grid_size <= 32 (got %d)",
                o->grid_size);
  if (s->any_reflective && o->max_ray_depth > kMaxShadeLevels - 1)
    return fail(RT_E_UNSUPPORTED, "max_ray_depth %d > %d with reflective materials", o->max_ray_depth,
                kMaxShadeLevels - 1);
  return RT_OK;
}

// Lanes per pixel of a float32 launch (a power of two, <= 64): as many as
// the samples fill; scenes of spheres / boxes / planes with distant lights
// and no reflection (k_render_fast's object-binned batches) use fewer, so a
// work item holds at least one batch of kObjBatch = 4 iterations (C2: 64 spp
// -> 16 lanes, 4 pixels per wave), but not fewer than 16 (8 for a batch of
// 8). The count does not depend on the binning / batching flags, so
// RT_FLAG_NO_BINNING and RT_FLAG_NO_OBJ_BATCH frames stay bit-identical (the
// same samples per lane, summed in the same order).
int f32_lanes(unsigned sub, int spp) {
  int L = 1;
  while (L * 2 <= std::min(spp, 64)) L *= 2;
  const bool ob_batch = !(sub & (SUB_MESH | SUB_REFLECT | SUB_POINT)) && (sub & (SUB_SPHERE | SUB_BOX));
  const int lmin = kObjBatch > 4 ? 8 : 16;  // <= 8 pixels per wave (the kernel's object-mask union)
  while (ob_batch && L > lmin && spp / L < kObjBatch) L /= 2;
  return L;
}

// Dynamic LDS of a float32 launch: the (multi-)jittered tables, 64/L
// pixels per wave x 2 x spp floats x 4 waves per block.
size_t f32_table_lds(const rt_options* o, int L) {
  if (o->aa_kind < RT_AA_MULTI_JITTERED) return 0;
  const int spp = o->grid_size * o->grid_size;
  return (size_t)4 * (64 / L) * 2 * (size_t)spp * sizeof(float);
}

// What a float32 call launches, decided once before its per-call build
// (plan_mapping, then plan_kernels): fill_fast hands the build the classes
// the chosen kernels understand, launch() launches the chosen kernels. The
// one thing known only after the build is whether the camera has pixel lists;
// without them a two-class plan falls back to the one-kernel launch.
// *_bpc: resident blocks per CU of a kernel the plan chose, asked of the
// runtime at most once per call (0: not asked, or no such kernel).
struct Plan {
  // the kernel specialisation (f32_subset) and its dynamic LDS
  unsigned sub;
  size_t shmem;
  // lanes per pixel (L), pixels per wave tile, number of wave groups; the
  // grid of the one-kernel launch, from fast_bpc
  int L, log2L, tx, ty, tiles_x, ngroups, blocks, fast_bpc;
  // the call builds camera-dependent data: binning on, a wave spans at most
  // 4 pixels, every sample inside its pixel
  bool build;
  // one-pixel groups (L == 64): the build writes pixel records
  bool records;
  // the call may run as a two-class launch: not for instrumented launches,
  // a measuring launch of a launch order or a cost dump, at most 8 lights
  bool want_split;
  // ... and does, when the build finds lists: want_split with records, no
  // launch order, and a lean kernel for the subset (lean_bpc > 0). Every
  // field below but `wave` is false / 0 without it.
  bool two_class;
  int lean_bpc;
  // lean1_ok: implies one mesh object (shadow_mesh >= 0) and no point light
  bool one_plane;
  // the general list goes to the batched kernel: RT_FLAG_NO_BATCH off, one
  // mesh object, light grids, no point light, a kernel for the subset
  // (gen_bpc > 0). (launch() also asked for pixel lists: a two-class launch
  // always has them.)
  bool gen;
  int gen_bpc;
  // ... to gen1_loop: gen && one_plane && !RT_FLAG_NO_GEN1
  bool gen1;
  // the lean list goes to lean1q_loop: one_plane && !RT_FLAG_NO_LEAN1
  bool lean1;
  // lanes per lean pixel: 4 or 16 with lean1 (64 / lp pixels per item), else
  // 64 (k_render_lean, runs of kLeanRun pixels)
  int lp;
  // both lists in one kernel (k_render_mix1): gen1 && lean1 && !RT_FLAG_NO_MIX
  bool mix;
  // the build tags lean entries with their uniform class, which only
  // lean1q_loop reads: lean1 && !RT_FLAG_NO_UNIFORM && the group index fits
  // below the class (ncols * nrows <= kLeanIdxMask)
  bool uniform;
  // the build tags general entries with the ground bit, which only gen1_loop
  // reads: gen1 && !RT_FLAG_NO_GROUND1 && ncols * nrows <= kLeanIdxMask
  bool ground;
  // the kernels a two-stream launch is sized from (mix: mix_bpc alone):
  // k_render_gen1 (gen1; else gen_bpc, or the mapping's grid), and the lean
  // list's kernel — k_render_lean1q<nl, lp> or k_render_lean
  int gen1_bpc, lean_list_bpc, mix_bpc;
  // one-kernel launches of reflective scenes: reflected rays compacted per
  // wave (k_render_wave, wave_bpc > 0). Never with two_class: the lean kernel
  // exists only for subsets without reflection.
  bool wave;
  int wave_bpc;
};

// aov: the plan of a feature-buffer call (rt_render_aovs*) — the render's
// lanes and tiles for these options, k_render_aov's subset and residency.
Plan plan_mapping(const rt_scene* s, const rt_options* o, const Mapping& mp, int spp, bool aov = false) {
  Plan pl{};
  pl.sub = f32_subset(s, o);
  // a pixel's samples spread over up to 64 lanes
  const int L = f32_lanes(pl.sub, spp);
  int lg = 0;
  while ((1 << lg) < L) ++lg;
  pl.shmem = f32_table_lds(o, L);
  const int P = 64 / L;
  int tx = 1, ty = 1;
  switch (P) {
    case 64: tx = 8; ty = 8; break;
    case 32: tx = 8; ty = 4; break;
    case 16: tx = 4; ty = 4; break;
    case 8: tx = 4; ty = 2; break;
    case 4: tx = 2; ty = 2; break;
    case 2: tx = 2; ty = 1; break;
    default: tx = 1; ty = 1; break;
  }
  pl.L = L;
  pl.log2L = lg;
  pl.tx = tx;
  pl.ty = ty;
  pl.tiles_x = (mp.ncols + tx - 1) / tx;
  const long long tiles_y = (mp.nrows + ty - 1) / ty;
  const long long ng = (long long)pl.tiles_x * tiles_y;
  pl.ngroups = (int)std::min<long long>(ng, INT32_MAX);
  const long long want = (ng + 3) / 4;
  // work-queue kernel: launch what is resident
  if (aov) {  // camera rays only: point lights and reflection cannot matter
    pl.sub &= 15u | (unsigned)SUB_STOCHASTIC;
    pl.fast_bpc = rtmi_aov_f32_blocks_per_cu(pl.sub, pl.shmem);
  } else {
    pl.fast_bpc = rtmi_render_f32_blocks_per_cu((o->flags & RT_FLAG_COUNT_TRAVERSAL) ? 1 : 0, pl.sub, pl.shmem);
  }
  const long long cap = std::min<long long>(s->max_waves / 4, (long long)pl.fast_bpc * s->num_cus);
  pl.blocks = (int)std::max(1LL, std::min<long long>(want, cap));
  return pl;
}

// Launch order of the pixel groups: expensive first, from measured costs.
// Per-pixel cost varies ~20x (sky vs bunny + its shadows) and the work queue
// hands groups out in index order, so a launch ends when the wave that drew
// the last expensive group finishes it: a fixed ~0.2 ms on every C3 launch
// (a group at 256 spp is one pixel, up to ~0.2 ms of a wave's time), 2.5 %
// of a frame on one GPU and ~17 % of each rank's share on 8. The first
// launch of a mapping (image size, rows, bands, sampling) runs in screen
// order and records each group's duration (s_memtime); later launches of the
// same mapping hand groups out longest-first (LPT), so the tail is cheap
// groups — for launches short enough that the tail matters (below). Scheduling only: every launch traces every ray, and the image and
// Stats do not depend on the order. Off with RT_FLAG_NO_REORDER.
constexpr long long kLptGroupsPerWave = 96;

struct OrderUse {
  const int32_t* order = nullptr;  // FastParams.order
  unsigned* cost = nullptr;        // FastParams.cost (the measuring launch)
  rt_scene::Order* entry = nullptr;
  const std::vector<int32_t>* host_order = nullptr;  // the order on the host
};

int order_policy() {
  static const int v = [] {
    // tuning knob: 0 off, 1 LPT, 2 LPT in half octaves, 3 heavy then light
    // (split at the RTMI_ORDER_P cost quantile, screen order within each),
    // 4 = 3 with the light part longest-first. Off by default (round 3): the
    // costs are measured on an earlier frame of the same camera, and no
    // camera-dependent data is carried from one call to the next; the
    // two-class launches already hand out the expensive (general) pixels
    // before the cheap (lean) ones.
    const char* e = rtmi::diag_env("RTMI_ORDER");
    return e ? std::atoi(e) : 0;
  }();
  return v;
}

double order_quantile() {
  static const double v = [] {
    const char* e = rtmi::diag_env("RTMI_ORDER_P");
    return e ? std::atof(e) : 0.5;
  }();
  return v;
}

OrderUse group_order(rt_scene* s, const rt_options* o, const Mapping& mp, const FastParams& p, int blocks) {
  OrderUse u;
  const int policy = order_policy();
  // LPT only where the tail outweighs locality: with >= ~128 groups per
  // resident wave, screen order's spatial coherence (neighbouring pixels
  // share BVH paths in the scalar caches) is worth more than the tail (C3:
  // whole frame 8.15 ms screen vs 8.36 LPT; half frame equal; quarter 2.22
  // vs 2.10; eighth 1.23 vs 1.07; 1/64 0.34 vs 0.26)
  const long long waves = (long long)blocks * 4;
  if (policy == 0 || (o->flags & RT_FLAG_NO_REORDER) || p.ngroups < waves || p.ngroups > kLptGroupsPerWave * waves)
    return u;
  const std::array<int64_t, 17> key = {o->width,   o->height,  mp.mode,     mp.y0,       mp.nrows,  mp.ncols,
                                       mp.step,    mp.max_step, mp.band_h,  mp.rank,     mp.world,  p.tile_x,
                                       p.tile_y,   p.ngroups,   o->aa_kind, o->grid_size, o->max_ray_depth};
  size_t i = 0;
  while (i < s->orders.size() && s->orders[i]->key != key) ++i;
  if (i == s->orders.size()) {  // new mapping: measure it
    std::unique_ptr<rt_scene::Order> e(new rt_scene::Order());
    e->key = key;
    if (e->cost.alloc((size_t)p.ngroups) != RT_OK ||
        hipEventCreateWithFlags(&e->measured.h, hipEventDisableTiming) != hipSuccess)
      return u;
    s->orders.insert(s->orders.begin(), std::move(e));
    if (s->orders.size() > 8) s->orders.pop_back();
    u.cost = s->orders[0]->cost.p;
    u.entry = s->orders[0].get();
    return u;
  }
  std::rotate(s->orders.begin(), s->orders.begin() + (long)i, s->orders.begin() + (long)i + 1);
  rt_scene::Order& e = *s->orders[0];
  if (!e.perm.p) {
    std::vector<unsigned> c((size_t)p.ngroups);
    if (hipEventSynchronize(e.measured) != hipSuccess ||
        hipMemcpy(c.data(), e.cost.p, c.size() * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
      return u;
    // stable counting sort, most expensive bucket first
    constexpr int kBuckets = 4096;
    unsigned cmax = 1;
    for (unsigned v : c) cmax = std::max(cmax, v);
    unsigned split = 0;  // policies 3/4: costs above this are "heavy"
    if (policy >= 3) {
      std::vector<unsigned> t(c);
      const size_t q = std::min(t.size() - 1, (size_t)(order_quantile() * (double)t.size()));
      std::nth_element(t.begin(), t.begin() + (long)q, t.end());
      split = t[q];
    }
    std::vector<uint16_t> bucket(c.size());
    std::vector<int32_t> start(kBuckets + 1, 0);
    for (size_t g = 0; g < c.size(); ++g) {
      int b;
      if (policy == 3) {
        b = c[g] > split ? kBuckets - 1 : 0;
      } else if (policy == 4) {
        b = c[g] > split ? kBuckets - 1 : (int)((uint64_t)c[g] * (kBuckets - 2) / std::max(split, 1u));
      } else if (policy == 2) {  // half-octave classes: keeps screen order within a class
        const unsigned v = std::max(c[g], 1u);
        const int l = 31 - __builtin_clz(v);
        b = 2 * l + (l > 0 ? (int)((v >> (l - 1)) & 1u) : 0);
      } else {
        b = (int)((uint64_t)c[g] * (kBuckets - 1) / cmax);
      }
      b = kBuckets - 1 - b;
      bucket[g] = (uint16_t)b;
      ++start[(size_t)b + 1];
    }
    for (int b = 0; b < kBuckets; ++b) start[(size_t)b + 1] += start[(size_t)b];
    std::vector<int32_t> perm(c.size());
    for (size_t g = 0; g < c.size(); ++g) perm[(size_t)start[bucket[g]]++] = (int32_t)g;
    if (e.perm.upload(perm) != RT_OK) return u;
    e.host_perm.swap(perm);
    e.cost.release();
  }
  u.order = e.perm.p;
  u.host_order = &e.host_perm;
  return u;
}

// ---- camera-dependent data, rebuilt by every float32 render call (rt_frame.h)

FrameRows frame_rows(const Mapping& mp, int height) {
  FrameRows r;
  r.mode = mp.mode;
  r.y0 = mp.y0;
  r.nrows = mp.nrows;
  r.step = mp.step;
  r.band_h = mp.band_h;
  r.rank = mp.rank;
  r.world = mp.world;
  r.height = height;
  return r;
}

// The per-call buffers of one image size (contents are rebuilt by each call).
int frame_buffers(rt_scene* s, int w, int h, hipStream_t st) {
  rt_scene::Frame& f = s->fr;
  const bool lists = s->binnable && !s->bin_tris.empty();
  // slots per pixel: 2^want_lg when set (the test hook), else
  // as many as 2^27 entries (512 MB) allow, 32 to 256: a mesh's per-pixel
  // lists are longer the fewer pixels it covers (the bunny: 28 faces at most
  // at 1080p, past 32 for 7 % of its pixels at 320x180); a pixel past its
  // slots takes the BVH (exact, slower)
  int lg = f.want_lg >= 0 ? f.want_lg : slot_lg_for(w, h);
  // slot indices are 32-bit (pixel << lg + slot, int in the kernels): a
  // requested lg (test hook) is clamped to keep the block below
  // 2^31 entries
  while (lg > 0 && (((unsigned long long)w * (unsigned long long)h) << lg) + kBinPad >= (1ull << 31)) --lg;
  if (f.w == w && f.h == h && (!lists || f.slot_lg == lg)) return RT_OK;
  // an earlier call may still read the old buffers: `st` (the build stream)
  // waits on the last call that used this set (its render kernels, and the
  // aux-stream kernels joined into it), so this one wait covers them all
  HIP_TRY(hipStreamSynchronize(st));
  const size_t npx = (size_t)w * (size_t)h;
  int rc;
  f.invalidate();
  if ((rc = f.cnt.alloc(npx + 1)) || (rc = f.info.alloc(npx)) || (rc = f.lean.alloc(npx + 64)) ||
      (rc = f.heavy.alloc(npx)) || (rc = f.ctr.alloc(FC_WORDS)) ||
      (rc = f.tiles.alloc((size_t)rtmi_frame_skip_cells(w, h))) ||
      (rc = f.status.alloc((size_t)rtmi_frame_tile_bytes(w, h))) ||
      (rc = f.uni_cls.alloc((size_t)rtmi_frame_tile_bytes(w, h) * 4)))
    return rc;
  if (s->objbins && ((rc = f.omask.alloc(npx)) || (rc = f.orect.alloc(kObjRectInts)))) return rc;
  if (lists) {
    // the slots hold valid record offsets from the start (the list search
    // reads up to kBinPad entries past a list's end)
    const size_t ns = (npx << lg) + kBinPad;
    if ((rc = f.slots.alloc(ns)) || (rc = f.huge.alloc(kHugeCap))) return rc;
    HIP_TRY(hipMemsetD32Async(f.slots.p, s->bin_tris[0].rec, ns, st));
    f.slot_lg = lg;
  }
  // the per-pixel counters are zero between calls (k_frame_build2 zeroes
  // the ones a call used)
  // (stream-ordered before the call's build launches on the same stream)
  HIP_TRY(hipMemsetAsync(f.cnt.p, 0, f.cnt.bytes(), st));
  HIP_TRY(hipMemsetAsync(f.ctr.p, 0, f.ctr.bytes(), st));
  HIP_TRY(hipMemsetAsync(f.info.p, 0, f.info.bytes(), st));  // (only read for the call's pixels; defined for the test hook)
  f.w = w;
  f.h = h;
  return RT_OK;
}

void uniform_cam(const rt_scene* s, const FastParams& p, bg::UniformCam& u) {
  const int po = p.shadow_mesh == 0 ? 1 : 0;  // the plane (lean1_ok: two objects, one the mesh)
  uniform_cam(s->h_obj_ty[(size_t)po], s->h_light_vy.data(), p, u);
}

// The call's pixel-record / list parameters (RecordsLaunch) for the
// launch's pixels.
void records_launch(rt_scene* s, const rt_options* o, const Mapping& mp, const FastParams& p, bool records,
                    bool split, bool uniform, bool ground, RecordsLaunch& r) {
  std::memset(&r, 0, sizeof r);
  r.mode = mp.mode;
  r.y0 = mp.y0;
  r.nrows = mp.nrows;
  r.ncols = mp.ncols;
  r.step = mp.step;
  r.max_step = mp.max_step;
  r.band_h = mp.band_h;
  r.rank = mp.rank;
  r.world = mp.world;
  r.width = o->width;
  r.height = o->height;
  r.ngroups = p.ngroups;
  r.info = s->fr.info.p;
  r.records = records ? 1 : 0;
  if (records && s->skippable && s->skip_planes.size() <= (size_t)kFrameMaxPlanes) {
    std::vector<bg::SkipPlaneC> pcs;
    if (skip_camera(s->skip_planes, s->mesh_w2o, s->c2w, s->fov, o->width, o->height, o->bias, &r.cam, &pcs)) {
      r.nplanes = (int32_t)pcs.size();
      std::copy(pcs.begin(), pcs.end(), r.planes);
      r.nl = std::min(8, s->nlight);
      for (int l = 0; l < r.nl; ++l) r.have |= s->grid_occ[(size_t)l].g.gu > 0 ? 1u << l : 0u;
      r.grids = s->grids.p;
      r.sat = s->sat_dev.p;
      for (int l = 0; l < 8; ++l) r.sat_off[l] = s->sat_off[l];
    }
  }
  r.split = split ? 1 : 0;
  r.full = s->nlight >= 32 ? ~0u : (1u << s->nlight) - 1u;
  r.lean = s->fr.lean.p;
  r.heavy = s->fr.heavy.p;
  r.ctr = s->fr.ctr.p;
  if (split && (uniform || ground)) {  // one proof for both classes
    uniform_cam(s, p, r.uni);
    r.uni.on = uniform ? 1 : 0;
    r.ground = ground ? 1 : 0;
    r.uni_cls = s->fr.uni_cls.p;
  }
}

// The mesh's camera-ray lists for the launch's pixels, their records
// (records: one-pixel groups) and with split the lean / general lists — the
// call's two build launches (rt_frame.h). *ok = false: no lists for this
// camera (a mesh vertex may lie at or behind the camera plane), the kernels
// traverse the BVH. zero (words, count): the render kernels' queue heads +
// Stats words, zeroed by the first build launch (*zeroed = true).
int frame_build(rt_scene* s, const rt_options* o, const Mapping& mp, const FastParams& p, bool records, bool split,
                bool uniform, bool ground, unsigned int* zero, int nzero, hipStream_t st, bool* ok, bool* zeroed) {
  *ok = false;
  *zeroed = false;
  if (!s->binnable || s->bin_tris.empty()) return RT_OK;
  FrameLaunch a;
  std::memset(&a, 0, sizeof a);
  if (!pixel_camera(s->mesh_o2w, s->mesh_w2o, s->c2w, s->fov, o->width, o->height, &a.cam)) return RT_OK;
  // every vertex strictly in front of the camera plane (face_pixel_rect's
  // test): the test's left side is convex in the point, so the mesh box's
  // corners bound it
  for (int c = 0; c < 8; ++c) {
    const double q[3] = {(c & 1) ? s->mesh_hi[0] : s->mesh_lo[0], (c & 2) ? s->mesh_hi[1] : s->mesh_lo[1],
                         (c & 4) ? s->mesh_hi[2] : s->mesh_lo[2]};
    double pw[3], pc[3];
    bg::xform_point(s->mesh_o2w, q, pw);
    bg::xform_point(a.cam.w2c, pw, pc);
    if (!(pc[2] < -1e-9 * (1.0 + std::fabs(pc[0]) + std::fabs(pc[1])))) return RT_OK;
  }
  int rc = frame_buffers(s, o->width, o->height, st);
  if (rc) return rc;
  rt_scene::Frame& f = s->fr;
  a.tris = s->bin_dev.p;
  a.nf = (int32_t)s->bin_tris.size();
  a.rows = frame_rows(mp, o->height);
  a.cnt = f.cnt.p;
  a.slots = f.slots.p;
  a.slot_lg = f.slot_lg;
  a.huge = f.huge.p;
  a.parity = (int32_t)(f.calls++ & 1u);
  records_launch(s, o, mp, p, records, split, uniform, ground, a.r);
  a.tile_bits = f.tiles.p;
  a.tile_cls = f.status.p;
  a.tiles_x = (mp.ncols + 63) / 64;
  a.ntiles = a.tiles_x * ((mp.nrows + 3) / 4);
  a.zero = zero;
  a.nzero = nzero;
  if ((rc = rtmi_frame_build(&a, st))) {
    // the first launch may have run (its counters non-zero, zeroed only by
    // the second): the next call re-allocates and re-zeroes the buffers
    f.invalidate();
    return fail(RT_E_DEVICE, "frame build launch failed: %s", hipGetErrorString((hipError_t)rc));
  }
  f.listed = true;
  f.uniform = a.r.uni.on != 0;
  f.ground = a.r.ground != 0;
  f.uni_rows = a.ntiles * 4;
  *zeroed = zero != nullptr;
  *ok = true;
  return RT_OK;
}

// Object masks of the launch's rows (k_frame_obj_masks).
int frame_obj_masks(rt_scene* s, const rt_options* o, const Mapping& mp, hipStream_t st, bool* ok) {
  *ok = false;
  ObjMaskLaunch a;
  std::memset(&a, 0, sizeof a);
  static const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  bg::PixCam pc;
  if (!pixel_camera(kIdentity, kIdentity, s->c2w, s->fov, o->width, o->height, &pc)) return RT_OK;
  int rc = frame_buffers(s, o->width, o->height, st);
  if (rc) return rc;
  a.objs = s->objbox_dev.p;
  a.nobj = s->nobj;
  a.width = o->width;
  a.height = o->height;
  std::memcpy(a.w2c, pc.w2c, sizeof a.w2c);
  a.cam_a = pc.cam_a;
  a.cam_c = pc.cam_c;
  a.margin = kPixelMargin;
  a.rows = frame_rows(mp, o->height);
  a.masks = s->fr.omask.p;
  a.rects = s->fr.orect.p;
  const int e = rtmi_frame_obj_masks(&a, st);
  if (e) return fail(RT_E_DEVICE, "object mask launch failed: %s", hipGetErrorString((hipError_t)e));
  *ok = true;
  return RT_OK;
}

// Every sample offset of the sampler lies in [0, 1) x [0, 1) of its pixel
// (sampling.nim:5-113, renderer.nim:135), the premise of the camera-ray bins
// (rt_bins.h kPixelMargin). A sampler outside this list gets no bins.
bool sampler_in_pixel(int32_t aa_kind) {
  switch (aa_kind) {
    case RT_AA_NONE:                    // the pixel corner: offset 0
    case RT_AA_GRID:                    // (i + 1/2) / m
    case RT_AA_JITTERED:                // (i + u) / m, u in [0, 1)
    case RT_AA_MULTI_JITTERED:          // (i + (j + u) / n) / m
    case RT_AA_CORRELATED_MULTI_JITTERED:
      return true;
    default:
      return false;
  }
}

// diagnostic builds (tools/cost_map.py): RTMI_COST_DUMP=<file> records every
// pixel group's duration (s_memtime cycles) of a launch into <file>
const char* cost_dump_path() {
  static const char* path = rtmi::diag_env("RTMI_COST_DUMP");
  return path;
}

// The lean pixels of a two-class launch go to lean1q_loop (rt_fast.h) when
// the scene's only analytic object is one plane and every transform a
// translation (the mesh + plane feature subset, nothing else), with one or
// two distant lights, and akGrid sampling with m | 64 whose samples fill
// whole 4-sample batches of every lane (spp a multiple of 256): every sample
// is valid and a lane's samples share one column. Off with RT_FLAG_NO_LEAN1.
// The general pixels of the same launches go to gen1_loop (off with
// RT_FLAG_NO_GEN1).
bool lean1_ok(const rt_scene* s, const FastParams& p, unsigned sub) {
  return sub == SUB_MESH && p.nobj == 2 && p.shadow_mesh >= 0 &&
         (p.nlight == 1 || p.nlight == 2) && !p.has_point_light && p.aa_kind == RT_AA_GRID &&
         p.log2_grid_m >= 0 && p.log2_grid_m <= 6 && p.lanes_per_px == 64 && p.spp % 256 == 0 &&
         p.iters * 64 == p.spp && p.iters % 4 == 0 && s->nobj == 2;
}

// The kernels of the call (Plan), from its mapping, its FastParams (the
// scene's counts, the sampling, the light grids, the launch order) and the
// flags. Two-class launch (one pixel per wave): the lean pixels — no camera
// ray can hit the mesh, every light a distant light whose shadow rays from
// the pixel provably miss it, no reflection — get a kernel of their own.
void plan_kernels(const rt_scene* s, const rt_options* o, const Mapping& mp, const FastParams& p, Plan& pl) {
  const uint32_t fl = o->flags;
  pl.build = !(fl & RT_FLAG_NO_BINNING) && pl.L >= 16 && sampler_in_pixel(o->aa_kind);
  pl.records = pl.L == 64;
  pl.want_split = !(fl & (RT_FLAG_NO_SPLIT | RT_FLAG_COUNT_TRAVERSAL)) && !p.cost && !cost_dump_path() && s->nlight <= 8;
  if (pl.build && pl.records && pl.want_split && !p.order) pl.lean_bpc = rtmi_lean_f32_blocks_per_cu(pl.sub, pl.shmem);
  pl.two_class = pl.lean_bpc > 0;
  pl.lp = 64;
  if (pl.two_class) {
    pl.one_plane = lean1_ok(s, p, pl.sub);
    if (!(fl & RT_FLAG_NO_BATCH) && p.shadow_mesh >= 0 && p.grids && !p.has_point_light)
      pl.gen_bpc = rtmi_gen_f32_blocks_per_cu(pl.sub, pl.shmem);
    pl.gen = pl.gen_bpc > 0;
    pl.gen1 = pl.gen && pl.one_plane && !(fl & RT_FLAG_NO_GEN1);
    pl.lean1 = pl.one_plane && !(fl & RT_FLAG_NO_LEAN1);
    int lean1q4_bpc = 0;
    if (pl.lean1) {
      // 16 pixels per item (lp = 4) unless the launch's groups make fewer
      // items than resident waves (a short launch, e.g. a scanline), then 4
      // (lp = 16). (Round 3 switched below 8 items per wave; a rank's bands at
      // N = 8 — 2 per wave — render faster at 16 pixels per item in a
      // back-to-back loop: 0.1605 -> 0.1539 ms, N = 4 0.278 -> 0.265 ms,
      // profiles/r4/ab/r4t_*)
      lean1q4_bpc = rtmi_lean1_f32_blocks_per_cu(p.nlight, 4);
      const long long lwaves4 = 4LL * std::min<long long>((long long)lean1q4_bpc * s->num_cus, s->max_waves / 4);
      pl.lp = (long long)(p.ngroups + 15) / 16 >= lwaves4 ? 4 : 16;
    }
    // one-plane launches: both lists in one kernel (k_render_mix1: the
    // general items first, then the lean ones) — one ramp and one tail
    pl.mix = pl.gen1 && pl.lean1 && !(fl & RT_FLAG_NO_MIX);
    const bool idx_fits = (long long)mp.ncols * mp.nrows <= (long long)kLeanIdxMask;
    pl.uniform = pl.lean1 && !(fl & RT_FLAG_NO_UNIFORM) && idx_fits;
    pl.ground = pl.gen1 && !(fl & RT_FLAG_NO_GROUND1) && idx_fits;
    if (pl.mix) {
      pl.mix_bpc = rtmi_mix1_f32_blocks_per_cu(p.nlight, pl.lp);
    } else {
      if (pl.gen1) pl.gen1_bpc = rtmi_gen1_f32_blocks_per_cu(p.nlight);
      pl.lean_list_bpc = !pl.lean1    ? pl.lean_bpc
                         : pl.lp == 4 ? lean1q4_bpc
                                      : rtmi_lean1_f32_blocks_per_cu(p.nlight, pl.lp);
    }
  } else {
    // RT_FLAG_COMPACT, reflective scenes: reflected rays compacted per wave
    // (k_render_wave); not for an instrumented launch or a progressive
    // pass that fills step x step blocks (its pixels' sums are stored
    // more than once)
    const long long span = (long long)mp.nrows * o->width;
    if ((pl.sub & SUB_REFLECT) && (fl & RT_FLAG_COMPACT) && !(fl & RT_FLAG_COUNT_TRAVERSAL) &&
        !(mp.mode == 0 && mp.step > 1) && span < (1ll << 27))
      pl.wave_bpc = rtmi_wave_f32_blocks_per_cu(pl.sub, pl.shmem);
    pl.wave = pl.wave_bpc > 0;
  }
}

// The mapping words of FastParams: which pixels the launch covers (Mapping)
// and how its pixel groups lie on the waves (the plan's lanes and tiles) —
// what group_pixel reads. A render and a feature-buffer call fill them here.
void mapping_words(const Mapping& mp, const Plan& pl, int spp, FastParams& p) {
  p.mode = mp.mode;
  p.y0 = mp.y0;
  p.nrows = mp.nrows;
  p.ncols = mp.ncols;
  p.step = mp.step;
  p.max_step = mp.max_step;
  p.band_h = mp.band_h;
  p.rank = mp.rank;
  p.world = mp.world;
  p.lanes_per_px = pl.L;
  p.log2_lanes = pl.log2L;
  p.tile_x = pl.tx;
  p.tile_y = pl.ty;
  p.log2_tile_x = 0;
  while ((1 << p.log2_tile_x) < pl.tx) ++p.log2_tile_x;
  p.inv_band_h = mp.band_h > 0 ? (float)(1.0 / (double)mp.band_h) : 0.0f;
  p.tiles_x = pl.tiles_x;
  p.ngroups = pl.ngroups;
  p.iters = (spp + pl.L - 1) / pl.L;
  {  // g / tiles_x by multiply-shift: m = floor(2^(31+s) / d) + 1, s = ceil(log2 d), exact for g < 2^31
    const uint64_t d = (uint64_t)std::max(1, pl.tiles_x);
    int sh = 0;
    while ((1ull << sh) < d) ++sh;
    p.tx_shift = 31 + sh;
    p.tx_magic = (uint32_t)((1ull << (31 + sh)) / d + 1ull);
  }
}

// This call's pixel lists (frame_build made them) for a float32 kernel; with
// one pixel per wave (records) its pixel records besides.
void pixel_lists(const rt_scene* s, bool records, FastParams& p) {
  p.pix_slots = s->fr.slots.p;
  p.pix_cnt = s->fr.info.p;
  p.slot_lg = s->fr.slot_lg;
  if (records) p.pix_info = s->fr.info.p;
}

// The float32 launch's parameters and plan, and this call's camera-dependent
// data built on the device (rt_frame.h) in stream order before the render
// kernels: the mesh's camera-ray lists (>= 16 samples per pixel), the object
// masks, and for one-pixel waves the pixel records — with pl.two_class, also
// the lean / general lists of a two-class launch (*split: they exist).
// zero / nzero: the render kernels' queue heads + Stats words; a call that
// builds pixel lists zeroes them in its first build launch (*zeroed), else
// the caller clears them.
int fill_fast(rt_scene* s, const rt_options* o, const Mapping& mp, float* fb, FastParams& p, Plan& pl,
              rt_scene::Order** measuring, hipStream_t st, bool* split, unsigned int* zero, int nzero, bool* zeroed) {
  std::memset(&p, 0, sizeof p);
  // the scene, its shadow-ray records and (binned searches, rt_bins.h) the
  // light and object grids of shadow rays to distant lights
  fast_scene_words(s, o->flags, p);
  p.fb = fb;
  p.partials = s->partials.p;
  p.queue = s->queue.p;
  fast_camera(s->c2w, s->fov, o, p);
  const int spp = p.spp;
  p.seed = o->seed;
  p.max_depth = o->max_ray_depth;
  p.flags = (int32_t)o->flags;
  pl = plan_mapping(s, o, mp, spp);
  mapping_words(mp, pl, spp, p);
  {  // the 32-bit wave counters stay in registers across work items and are
     // added to the 64-bit totals before any can wrap: per item at most
     // 64 lanes x iters samples x levels x (1 + lights) traces x objects hits
    const uint64_t levels = s->any_reflective ? (uint64_t)std::min(kMaxShadeLevels, std::max(1, o->max_ray_depth + 1)) : 1ull;
    const uint64_t per_item = 64ull * (uint64_t)p.iters * levels * (1ull + (uint64_t)s->nlight) *
                              (uint64_t)std::max(1, s->nobj);
    // diagnostic builds with wider counters (RTMI_DIAG_LANES): RTMI_STAT_FLUSH=1 flushes every item
    static const int flush_env = rtmi::diag_env("RTMI_STAT_FLUSH") ? std::atoi(rtmi::diag_env("RTMI_STAT_FLUSH")) : 0;
    p.stat_flush = (o->flags & RT_FLAG_COUNT_TRAVERSAL) ? 1
                   : flush_env > 0 ? flush_env
                                   : (int32_t)std::min<uint64_t>(1u << 20, std::max<uint64_t>(1, 0xFFFFFFFFull / per_item));
  }
  // (binned searches of camera rays, when a wave spans at most 4 pixels —
  // >= 16 samples per pixel — are this call's own: frame_build below)
  // one work item per dequeue: per-pixel cost varies ~10x (sky vs bunny +
  // shadows), so coarser chunks leave an expensive tail in every launch
  // (C3 whole frame: 4 groups per dequeue 9.79 ms, 1 9.49 ms; 2-way bands:
  // 5.22 vs 4.69 ms per half). With 8 sharded heads the dequeue rate stays
  // far below the ~90/us a head sustains.
  p.shards = std::min(kQueueShards, pl.blocks);
  const OrderUse ou = group_order(s, o, mp, p, pl.blocks);
  p.order = ou.order;
  p.cost = ou.cost;
  *measuring = ou.entry;
  *split = false;
  *zeroed = false;
  plan_kernels(s, o, mp, p, pl);
  s->mesh1 = pl.gen1 && !(o->flags & RT_FLAG_NO_MESH1);
  if (s->mesh1) {  // gen1_loop's inset box (rt_bins_geom.h inset_box): the kernel's own float32 values
    const FObj& mo = s->h_fo[(size_t)s->shadow_mesh];
    bg::InsetBox ib;
    bg::inset_box(mo.lo, mo.hi, s->h_light_v.data(), s->nlight, ib);
    for (int k = 0; k < 3; ++k) {
      p.in_lo[k] = ib.lo[k];
      p.in_hi[k] = ib.hi[k];
    }
  }
  if (!pl.build) return RT_OK;
  // this call's camera-dependent data (nothing of it is kept from earlier calls)
  int rc;
  bool lists = false, masks = false;
  // the build on the scene's build stream after the call two back (the last
  // user of this buffer set), joined into the caller's stream before the
  // render kernels: it overlaps the previous call's render
  hipStream_t bs = st;
  if (s->pipe) {
    bs = s->bstream;
    if (s->fr.used_rec) HIP_TRY(hipStreamWaitEvent(bs, s->fr.used, 0));
  }
  auto join = [&]() -> int {
    if (bs != st) {
      HIP_TRY(hipEventRecord(s->fr.built, bs));
      HIP_TRY(hipStreamWaitEvent(st, s->fr.built, 0));
    }
    return RT_OK;
  };
  if ((rc = frame_build(s, o, mp, p, pl.records, pl.two_class, pl.uniform, pl.ground, zero, nzero, bs, &lists, zeroed))) {
    join();
    return rc;
  }
  if (lists) {
    pixel_lists(s, pl.records, p);
    *split = pl.two_class;
  }
  if (s->objbins) {
    if ((rc = frame_obj_masks(s, o, mp, bs, &masks))) {
      join();
      return rc;
    }
    if (masks) p.obj_pix = s->fr.omask.p;
  }
  return join();
}

template <class R>
void fill_params(rt_scene* s, const PrecisionData<R>& pd, const rt_options* o, const Mapping& mp, float* fb,
                 RenderParams<R>& p, int* blocks) {
  std::memset(&p, 0, sizeof p);
  p.objects = pd.objects.p;
  p.lights = pd.lights.p;
  p.meshes = pd.meshes.p;
  p.nodes = s->nodes.p;
  p.tris = pd.tris.p;
  p.normals = pd.normals.p;
  p.fb = fb;
  p.partials = s->partials.p;
  for (int k = 0; k < 16; ++k) p.c2w[k] = (R)s->c2w[k];
  for (int k = 0; k < 3; ++k) p.bg[k] = (R)s->bg[k];
  // castPrimaryRay constants (renderer.nim:36-38), float64 on the host
  p.f = (R)std::tan(s->fov * (3.14159265358979323846 / 180.0) / 2);
  p.aspect = (R)((double)o->width / (double)o->height);
  p.bias = (R)o->bias;
  const int m = o->aa_kind != RT_AA_NONE ? o->grid_size : 1;
  const int spp = m * m;
  p.inv_len = (R)(1.0 / (double)spp);
  const double xs = 1.0 / (double)m;  // grid(): xs = 1/n, ys = 1/m (m = n)
  p.sample_step = (R)xs;
  p.sample_off = (R)(xs * 0.5);
  p.nobj = s->nobj;
  p.nlight = s->nlight;
  p.width = o->width;
  p.height = o->height;
  p.aa_kind = o->aa_kind;
  p.grid_m = m;
  p.spp = spp;
  p.max_depth = o->max_ray_depth;
  p.flags = (int32_t)o->flags;
  p.shadow_mesh = s->shadow_mesh;
  p.lean_plane = -1;
  p.seed = o->seed;
  p.sample_scratch = nullptr;
  p.max_iters = (int32_t)std::min<int64_t>(INT32_MAX, 2 * s->num_nodes + 16);
  p.mode = mp.mode;
  p.y0 = mp.y0;
  p.nrows = mp.nrows;
  p.ncols = mp.ncols;
  p.step = mp.step;
  p.max_step = mp.max_step;
  p.band_h = mp.band_h;
  p.rank = mp.rank;
  p.world = mp.world;
  // lanes per pixel: float64 parity mode keeps the reference's sequential
  // sample sum (one lane per pixel); float32 spreads samples over lanes.
  int L = 1;
  if (o->precision == RT_FP32) {
    while (L * 2 <= std::min(spp, 64)) L *= 2;
  }
  const int P = 64 / L;
  int tx = 1, ty = 1;
  switch (P) {
    case 64: tx = 8; ty = 8; break;
    case 32: tx = 8; ty = 4; break;
    case 16: tx = 4; ty = 4; break;
    case 8: tx = 4; ty = 2; break;
    case 4: tx = 2; ty = 2; break;
    case 2: tx = 2; ty = 1; break;
    default: tx = 1; ty = 1; break;
  }
  p.lanes_per_px = L;
  p.tile_x = tx;
  p.tile_y = ty;
  p.tiles_x = (mp.ncols + tx - 1) / tx;
  const long long tiles_y = (mp.nrows + ty - 1) / ty;
  p.ngroups = (long long)p.tiles_x * tiles_y;
  const long long want = (p.ngroups + 3) / 4;
  long long cap = s->max_waves / 4;
  if (o->aa_kind >= RT_AA_JITTERED) {  // per-lane sample tables: keep the scratch <= 256 MB
    const long long per_block = 256LL * 2 * spp * (long long)sizeof(R);
    cap = std::min(cap, std::max(1LL, (256LL << 20) / per_block));
  }
  *blocks = (int)std::max(1LL, std::min<long long>(want, cap));
}

// What a float64 call of either kind — a render (launch_f64) or a feature-buffer
// call (aov64_device) — prepares for its kernel after fill_params:
//  - the stochastic samplers' table scratch;
//  - this call's pixel records (the float32 path's build, one launch set) when
//    `binning` and the scene has skip planes: a pixel whose camera rays provably
//    miss the mesh skips their traversal, and its shadow rays to the lights its
//    skip bits clear skip theirs — the same answers (the traversal would find no
//    face), so frames and Stats stay bit-exact (tests/test_gpu_parity.py);
//  - with one pixel per wave (px_wave; akGrid with >= 64 samples per pixel): the
//    pixel lists its camera rays search, and the grid of a kernel that takes
//    `batch` pixels per item and keeps blocks_per_cu blocks resident.
// *lists: the pixel lists exist.
int prepare_f64(rt_scene* s, const rt_options* o, const Mapping& mp, bool binning, bool px_wave, int batch,
                int blocks_per_cu, RenderParams<double>& p, int* blocks, hipStream_t st, bool* lists) {
  if (p.aa_kind >= RT_AA_JITTERED) {
    const size_t need = (size_t)*blocks * 256 * 2 * (size_t)p.spp;
    if (s->f64_tables.n < need) {
      HIP_TRY(hipStreamSynchronize(st));  // an earlier launch may still use the old buffer
      int rc = s->f64_tables.alloc(need);
      if (rc) return rc;
    }
    p.sample_scratch = s->f64_tables.p;
  }
  *lists = false;
  if (binning && sampler_in_pixel(o->aa_kind) && s->skippable) {
    FastParams pf;
    std::memset(&pf, 0, sizeof pf);
    bool zeroed = false;
    if (int rc = frame_build(s, o, mp, pf, true, false, false, false, nullptr, 0, st, lists, &zeroed)) return rc;
    if (*lists) p.pix_info = s->fr.info.p;
  }
  if (!px_wave) return RT_OK;
  if (*lists) {
    p.pix_slots = s->fr.slots.p;
    p.slot_lg = s->fr.slot_lg;
  }
  p.tri_rec0 = (int32_t)s->num_nodes;
  const long long nbatch = ((long long)mp.nrows * mp.ncols + batch - 1) / batch;
  const long long resident = (long long)std::max(1, blocks_per_cu) * s->num_cus;
  *blocks = (int)std::max(1LL, std::min({(nbatch + 3) / 4, resident, (long long)s->max_waves / 4}));
  return RT_OK;
}

// One pixel per wave in float64 (k_render_px64, k_aov64_px): akGrid with >= 64
// samples per pixel, unless the caller keeps one pixel per lane.
bool f64_px_wave(const rt_options* o, int spp) {
  return o->aa_kind == RT_AA_GRID && spp >= 64 && !(o->flags & RT_FLAG_F64_PER_LANE);
}

// The float64 render: prepare_f64, then k_render_px64 (whose shadow rays to
// distant lights search the scene's light grids, rt_device.h mesh_lists) or
// k_render. *launched: blocks of the render kernel.
int launch_f64(rt_scene* s, const rt_options* o, const Mapping& mp, float* d_out, hipStream_t st, int* launched) {
  RenderParams<double> p;
  int blocks = 1;
  fill_params<double>(s, s->f64, o, mp, d_out, p, &blocks);
  s->last_general = p.ngroups;
  if (p.ngroups == 0) return RT_OK;
  const bool binning = !(o->flags & (RT_FLAG_NO_BINNING | RT_FLAG_COUNT_TRAVERSAL));
  const int px64 = f64_px_wave(o, p.spp) && !(o->flags & RT_FLAG_COUNT_TRAVERSAL)
                       ? (s->any_reflective && o->max_ray_depth >= 1 ? 2 : 1)
                       : 0;
  bool lists = false;
  if (int rc = prepare_f64(s, o, mp, binning, px64 != 0, rtmi_px64_batch(), px64 ? rtmi_px64_blocks_per_cu(px64) : 0, p,
                           &blocks, st, &lists))
    return rc;
  if (px64) {
    if (lists) p.lean_plane = s->lean64_plane;
    if (binning && s->has_grids) {
      p.grids = s->grids.p;
      p.grid_off = s->grid_off.p;
      p.grid_ent = s->grid_ent.p;
      if (!s->sh64_ready && s->shadow_mesh >= 0) {
        if (int rc = s->sh64.alloc(s->grid_ent.n)) return rc;
        for (int li = 0; li < s->nlight && li < (int)s->grid_host.size(); ++li) {
          const LightGrid& g = s->grid_host[(size_t)li].g;  // (the header and the count survive a relight)
          const int64_t ne = s->grid_nent[(size_t)li];
          if (g.gu <= 0 || ne <= 0) continue;
          const int e = rtmi_build_sh64(s->f64.objects.p, s->shadow_mesh, s->f64.lights.p, li,
                                        s->grid_ent.p + g.ent_base, (int)ne, s->f64.tris.p,
                                        (int32_t)s->num_nodes, s->sh64.p + g.ent_base, st);
          if (e) return fail(RT_E_DEVICE, "shadow record build failed: %s", hipGetErrorString((hipError_t)e));
        }
        s->sh64_ready = true;
      }
      if (s->sh64_ready) p.sh64 = s->sh64.p;
    }
  }
  if (o->flags & RT_FLAG_TIMING) HIP_TRY(hipEventRecord(s->tev[1], st));  // after the per-call build
  const int e = rtmi_launch_render_f64(&p, blocks, px64, st);
  if (e) return fail(RT_E_DEVICE, "render kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  *launched = blocks;
  return RT_OK;
}

// Two-class launch: the general kernel on its list and the lean kernel on its
// own, as one merged kernel (pl.mix) or on two streams. The lists and their
// entry counts come from this call's k_frame_build2 (the host never reads
// them: grids and items are sized for the launch's groups, the kernels stop
// at the device counts). *launched: blocks of all its kernels.
int launch_two_class(rt_scene* s, const Plan& pl, const FastParams& p, hipStream_t st, int* launched) {
  int32_t* const n_heavy = s->fr.ctr.p + FC_HEAVY;
  int32_t* const n_lean = s->fr.ctr.p + FC_LEAN;
  const int lp = pl.lp;
  FastParams ph = p, pn = p;
  // the general pixels: the batched kernel (k_render_gen) for scenes of one
  // mesh object with distant lights only, no reflection (the lean kernel's
  // subsets) when both camera lists and light grids exist
  ph.order = s->fr.heavy.p;
  ph.ngroups = p.ngroups;
  ph.list_n = n_heavy;
  // the lean pixels' work items: runs of kLeanRun pixels (k_render_lean),
  // 64 / lp pixels (k_render_lean1q, lp lanes per pixel)
  const int lrun = lp == 64 ? kLeanRun : 64 / lp;
  const int lruns = (p.ngroups + lrun - 1) / lrun;  // at most: the kernels stop at the device count
  pn.order = s->fr.lean.p;
  pn.ngroups = lruns;
  pn.list_n = n_lean;
  pn.stat_flush = std::max(1, p.stat_flush / lrun);
  pn.queue = s->queue.p + (size_t)kQueueShards * kQueueStride;
  if (pl.mix) {
    FastParams pm = ph;
    pm.order2 = pn.order;
    pm.ngroups2 = pn.ngroups;
    pm.list_n2 = n_lean;
    pm.stat_flush = std::min(ph.stat_flush, pn.stat_flush);
    const long long mcap = (long long)pl.mix_bpc * s->num_cus;
    const int mb = (int)std::max(1LL, std::min<long long>(std::min<long long>(mcap, pl.blocks),
                                                          ((long long)p.ngroups + lruns + 3) / 4));
    pm.shards = std::min(kQueueShards, mb);
    pm.shards2 = pm.shards;
    const int e = rtmi_launch_mix1_f32(&pm, p.nlight, lp, mb, st);
    if (e) return fail(RT_E_DEVICE, "render kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    *launched = mb;
    s->last_lean_kind = 3 | (3 << 2) | (lp << 8);
    s->last_batched = -1;  // = the general list (device count)
    return RT_OK;
  }
  const long long hcap =
      pl.gen ? std::min<long long>((long long)(pl.gen1 ? pl.gen1_bpc : pl.gen_bpc) * s->num_cus, pl.blocks) : pl.blocks;
  const int hb = (int)std::max(1LL, std::min<long long>(hcap, ((long long)p.ngroups + 3) / 4));
  ph.shards = std::min(kQueueShards, hb);
  const long long lcap = (long long)pl.lean_list_bpc * s->num_cus;
  const int lb = (int)std::max(1LL, std::min<long long>(std::min<long long>(lcap, s->max_waves / 4),
                                                        ((long long)lruns + 3) / 4));
  pn.shards = std::min(kQueueShards, lb);
  pn.partials = s->partials.p + (size_t)hb * 4 * kStatSlots;
  // general kernel first on the caller's stream, the lean kernel on the
  // scene's aux stream (forked after the caller's earlier work, joined
  // before its later work)
  HIP_TRY(hipEventRecord(s->fork, st));
  HIP_TRY(hipStreamWaitEvent(s->aux, s->fork, 0));
  int e = pl.gen1  ? rtmi_launch_gen1_f32(&ph, p.nlight, hb, st)
          : pl.gen ? rtmi_launch_gen_f32(&ph, pl.sub, hb, pl.shmem, st)
                   : rtmi_launch_render_f32(&ph, pl.sub, hb, pl.shmem, st);
  if (!e)
    e = pl.lean1 ? rtmi_launch_lean1_f32(&pn, p.nlight, lp, lb, s->aux)
                 : rtmi_launch_lean_f32(&pn, pl.sub, lb, pl.shmem, s->aux);
  if (e) return fail(RT_E_DEVICE, "render kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  HIP_TRY(hipEventRecord(s->join, s->aux));
  HIP_TRY(hipStreamWaitEvent(st, s->join, 0));
  *launched = hb + lb;
  s->last_lean_kind = (pl.lean1 ? 2 : 1) | ((pl.gen1 ? 2 : pl.gen ? 1 : 0) << 2) | (lp << 8);
  s->last_batched = pl.gen ? -1 : 0;
  return RT_OK;
}

// One-kernel launch: every group general — k_render_wave (pl.wave: reflected
// rays compacted per wave, then added to the framebuffer) or k_render_fast.
int launch_one_kernel(rt_scene* s, const rt_options* o, const Mapping& mp, const Plan& pl, FastParams& p, float* d_out,
                      hipStream_t st, int* launched) {
  if (!pl.wave) {
    const int e = rtmi_launch_render_f32(&p, pl.sub, pl.blocks, pl.shmem, st);
    if (e) return fail(RT_E_DEVICE, "render kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    *launched = pl.blocks;
    return RT_OK;
  }
  const long long span = (long long)mp.nrows * o->width;
  const int wb = (int)std::max(1LL, std::min<long long>(std::min<long long>((long long)pl.wave_bpc * s->num_cus,
                                                                            s->max_waves / 4),
                                                        ((long long)p.ngroups + 3) / 4));
  const size_t qfl = (size_t)wb * 4 * kReflQueue * kReflFields;
  const size_t nsec = (size_t)span * 3;
  if (s->refl_queue.n < qfl || s->refl_sec.n < nsec) {
    HIP_TRY(hipStreamSynchronize(st));  // an earlier launch may still use the old buffers
    int rc = s->refl_queue.n < qfl ? s->refl_queue.alloc(qfl) : RT_OK;
    if (!rc && s->refl_sec.n < nsec) rc = s->refl_sec.alloc(nsec);
    if (rc) return rc;
  }
  HIP_TRY(hipMemsetAsync(s->refl_sec.p, 0, nsec * sizeof(long long), st));
  p.rq = s->refl_queue.p;
  p.sec = s->refl_sec.p;
  p.sec_base = mp.mode == 0 ? (int64_t)mp.y0 * o->width : 0;
  p.shards = std::min(kQueueShards, wb);
  int e = rtmi_launch_wave_f32(&p, pl.sub, wb, pl.shmem, st);
  if (!e)
    e = rtmi_launch_sec_add(d_out + (size_t)p.sec_base * 3, p.sec, nsec, o->aa_kind != RT_AA_NONE ? p.inv_len : 1.0f,
                            s->num_cus, st);
  if (e) return fail(RT_E_DEVICE, "render kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  *launched = wb;
  s->last_lean_kind = 16;
  return RT_OK;
}

// After the render kernels of a float32 launch: the measuring launch of a
// launch order is marked, a cost dump written.
int launch_tail(hipStream_t st, int ngroups, rt_scene::Order* measuring, DevBuf<unsigned>& dbg_cost) {
  if (measuring) HIP_TRY(hipEventRecord(measuring->measured, st));
  if (dbg_cost.p) {
    std::vector<unsigned> c((size_t)ngroups);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(c.data(), dbg_cost.p, c.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    dbg_cost.release();
    if (FILE* f = std::fopen(cost_dump_path(), "wb")) {
      std::fwrite(c.data(), sizeof(unsigned), c.size(), f);
      std::fclose(f);
    }
  }
  return RT_OK;
}

// What rt_scene_last_split / _last_batch and their kin report describes THIS
// call, even when it returns early, runs the float64 kernel or
// renders feature buffers: every render-class call starts from here.
void reset_report(rt_scene* s) {
  s->fr.counted = false;
  s->fr.listed = false;
  s->fr.uniform = false;
  s->fr.ground = false;
  s->mesh1 = false;
  s->pending_reduce = 0;
  s->last_lean = 0;
  s->last_lean_kind = 0;
  s->last_general = 0;
  s->last_batched = 0;
}

// A render-class call's completion on stream st. One event per call: the
// buffer set's `used` is also the scene's `done`.
int record_done(rt_scene* s, hipStream_t st) {
  HIP_TRY(hipEventRecord(s->fr.used, st));
  s->fr.used_rec = true;
  s->done = s->fr.used;
  s->done_stream = st;
  return RT_OK;
}

// zero / nzero: the queue heads and / or Stats words every call clears
// before its render kernels (a float32 call that builds pixel lists clears
// them in its first build launch: one launch fewer).
int launch(rt_scene* s, const rt_options* o, const Mapping& mp, float* d_out, hipStream_t st, bool reduce,
           unsigned int* zero, int nzero) {
  auto clear = [&]() -> int {
    if (nzero > 0) HIP_TRY(hipMemsetAsync(zero, 0, (size_t)nzero * sizeof(unsigned int), st));
    return RT_OK;
  };
  reset_report(s);
  int launched = 0;  // blocks of the render kernels (0: nothing to render)
  if (o->precision == RT_FP64) {
    if (int rc = clear()) return rc;
    if (int rc = launch_f64(s, o, mp, d_out, st, &launched)) return rc;
  } else {
    if (mp.nrows == 0 || mp.ncols == 0) return clear();
    FastParams p;
    Plan pl;
    rt_scene::Order* measuring = nullptr;
    bool split = false, zeroed = false;
    int rc = fill_fast(s, o, mp, d_out, p, pl, &measuring, st, &split, zero, nzero, &zeroed);
    if (rc) return rc;
    s->mesh1 = s->mesh1 && split;  // (without lists the call is a one-kernel launch)
    if (!zeroed && (rc = clear())) return rc;
    if (o->flags & RT_FLAG_TIMING) HIP_TRY(hipEventRecord(s->tev[1], st));
    s->last_general = p.ngroups;
    if (p.ngroups == 0) return RT_OK;
    DevBuf<unsigned> dbg_cost;
    if (cost_dump_path() && !measuring && !p.cost) {
      if (dbg_cost.alloc((size_t)p.ngroups) == RT_OK) p.cost = dbg_cost.p;
    }
    s->fr.counted = split;
    rc = split ? launch_two_class(s, pl, p, st, &launched) : launch_one_kernel(s, o, mp, pl, p, d_out, st, &launched);
    if (rc) return rc;
    if ((rc = launch_tail(st, p.ngroups, measuring, dbg_cost))) return rc;
  }
  // the per-wave rows are reduced when the Stats are read (flush_reduce)
  if (reduce && launched > 0) s->pending_reduce = launched * 4;
  return RT_OK;
}

// The last call's Stats rows into acc(), on stream st (ordered after the
// call): at the end of a call whose caller reads its Stats, else by the
// first rt_scene_last_stats / _last_counters (the scene mutex is held; a
// later call replaces the rows and the pending count).
int flush_reduce(rt_scene* s, hipStream_t st) {
  if (s->pending_reduce <= 0) return RT_OK;
  const int e = rtmi_launch_reduce_stats(s->partials.p, s->pending_reduce, s->acc(), st);
  s->pending_reduce = 0;
  if (e) return fail(RT_E_DEVICE, "stats reduction launch failed: %s", hipGetErrorString((hipError_t)e));
  return RT_OK;
}

int read_stats(rt_scene* s, hipStream_t st, rt_stats* out) {
  unsigned long long h[kStatSlots];
  HIP_TRY(hipMemcpyAsync(h, s->acc(), sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  out->num_primary_rays = h[STAT_PRIMARY];
  // renderer.nim:54-56 counts one test per object per trace call, and every
  // trace call is a primary, shadow or reflection ray: the float32 kernel
  // leaves the slot at 0 and the count is derived; the float64 kernel still
  // counts it, which is checked here.
  const unsigned long long rays = h[STAT_PRIMARY] + h[STAT_SHADOW] + h[STAT_REFL];
  const unsigned long long tests = (unsigned long long)s->nobj * rays;
  if (h[STAT_TESTS] != 0 && h[STAT_TESTS] != tests)
    return fail(RT_E_DEVICE, "inconsistent intersection-test count (%llu vs %llu)", h[STAT_TESTS], tests);
  out->num_intersection_tests = tests;
  out->num_intersection_hits = h[STAT_HITS];
  out->num_shadow_rays = h[STAT_SHADOW];
  out->num_reflection_rays = h[STAT_REFL];
  s->last_fallback = (int64_t)h[STAT_GEN_FALLBACK];
  s->last_straight = (int64_t)h[STAT_LANE_TRIS];
  return RT_OK;
}

// Common device-side body: order after the previous call, clear the
// counters, launch, record completion. With RT_FLAG_NO_STATS (and no `out`,
// no traversal counting) the call's Stats are not reduced: it launches its
// render kernels and nothing else, and rt_scene_last_stats reports that.
int render_device(rt_scene* s, const rt_options* o, const Mapping& mp, float* d_out, hipStream_t st,
                  rt_stats* out, bool need_stats = false) {
  const bool reduce = need_stats || out || !(o->flags & RT_FLAG_NO_STATS) || (o->flags & RT_FLAG_COUNT_TRAVERSAL);
  s->stats_kept = reduce;
  // after the scene's previous call (a call on that call's own stream is
  // already ordered after it: no wait packet)
  if (st != s->done_stream) HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
  s->timed = (o->flags & RT_FLAG_TIMING) != 0;
  s->pipe = o->precision == RT_FP32 &&
            (s->pipe_mode == 1 ||
             (s->pipe_mode < 0 && 3LL * mp.nrows * mp.ncols <= (long long)o->width * (long long)o->height));
  if (s->pipe) {  // the other buffer set (the last call's stays intact for its readers until the next call)
    std::swap(s->fr, s->fr2);
    std::swap(s->queue, s->queue2);
  }
  if (s->timed) {  // (tev[1] again before the render kernels; here for launches with nothing to render)
    HIP_TRY(hipEventRecord(s->tev[0], st));
    HIP_TRY(hipEventRecord(s->tev[1], st));
  }
  // one fill: the queue heads (float32) and / or the Stats accumulator behind them
  const size_t q0 = o->precision == RT_FP32 ? 0 : rt_scene::kQueueWords;
  const size_t q1 = rt_scene::kQueueWords + (reduce ? 2 * (size_t)kStatSlots : 0);
  int rc = launch(s, o, mp, d_out, st, reduce, s->queue.p + q0, (int)(q1 - q0));
  if (rc) return rc;
  if ((out || need_stats || (o->flags & RT_FLAG_COUNT_TRAVERSAL)) && (rc = flush_reduce(s, st))) return rc;
  if (s->timed) HIP_TRY(hipEventRecord(s->tev[2], st));
  if (int rc = record_done(s, st)) return rc;
  if (out) return read_stats(s, st, out);
  return RT_OK;
}

int lines_mapping(const rt_options* o, int32_t y0, int32_t y1, int32_t step, int32_t max_step, Mapping* mp) {
  if (!is_pow2(step) || !is_pow2(max_step) || max_step < step)
    return fail(RT_E_INVALID, "step %d / maxStep %d must be powers of two with maxStep >= step", step, max_step);
  if (y0 < 0 || y1 > o->height || y0 > y1) return fail(RT_E_INVALID, "rows [%d, %d) outside [0, %d)", y0, y1, o->height);
  mp->mode = 0;
  mp->y0 = y0;
  mp->nrows = (y1 - y0 + step - 1) / step;
  mp->ncols = (o->width + step - 1) / step;
  mp->step = step;
  mp->max_step = max_step;
  mp->band_h = 1;
  mp->rank = 0;
  mp->world = 1;
  return RT_OK;
}

}  // namespace

extern "C" int rt_render_lines_device(rt_scene* s, const rt_options* o, float* d_fb, int32_t y0, int32_t y1,
                                      int32_t step, int32_t max_step, void* stream, rt_stats* out) {
  if (!s || !d_fb) return fail(RT_E_INVALID, "null argument");
  int rc = check_options(s, o);
  if (rc) return rc;
  Mapping mp;
  if ((rc = lines_mapping(o, y0, y1, step, max_step, &mp))) return rc;
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  return render_device(s, o, mp, d_fb, (hipStream_t)stream, out);
}

extern "C" int rt_render_lines(rt_scene* s, const rt_options* o, float* fb, int32_t fb_w, int32_t fb_h, int32_t y0,
                               int32_t y1, int32_t step, int32_t max_step, rt_stats* out) {
  if (!s || !fb) return fail(RT_E_INVALID, "null argument");
  int rc = check_options(s, o);
  if (rc) return rc;
  if (fb_w != o->width || fb_h != o->height)
    return fail(RT_E_INVALID, "framebuffer %dx%d does not match options %dx%d", fb_w, fb_h, o->width, o->height);
  Mapping mp;
  if ((rc = lines_mapping(o, y0, y1, step, max_step, &mp))) return rc;
  rt_stats local{};
  if (mp.nrows == 0) {
    if (out) *out = local;
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  const size_t need = (size_t)o->width * o->height * 3;
  if (s->fb_scratch.n < need && (rc = s->fb_scratch.alloc(need))) return rc;
  // rows the call may write: renderLine fills step x step blocks below y
  const int32_t last_y = y0 + (mp.nrows - 1) * step;
  const int32_t r0 = y0, r1 = std::min(last_y + step, o->height);
  const size_t off = (size_t)r0 * o->width * 3, cnt = (size_t)(r1 - r0) * o->width * 3;
  hipStream_t st = s->stream;
  HIP_TRY(hipMemcpyAsync(s->fb_scratch.p + off, fb + off, cnt * sizeof(float), hipMemcpyHostToDevice, st));
  if ((rc = render_device(s, o, mp, s->fb_scratch.p, st, nullptr, true))) return rc;
  HIP_TRY(hipMemcpyAsync(fb + off, s->fb_scratch.p + off, cnt * sizeof(float), hipMemcpyDeviceToHost, st));
  if ((rc = read_stats(s, st, &local))) return rc;
  if (out) *out = local;
  return RT_OK;
}

extern "C" int rt_render_bands_device(rt_scene* s, const rt_options* o, float* d_bands, int32_t band_h,
                                      int32_t rank, int32_t world, void* stream, rt_stats* out) {
  if (!s || !d_bands) return fail(RT_E_INVALID, "null argument");
  int rc = check_options(s, o);
  if (rc) return rc;
  if (band_h <= 0 || world <= 0 || rank < 0 || rank >= world)
    return fail(RT_E_INVALID, "bad band geometry band_h=%d rank=%d world=%d", band_h, rank, world);
  int32_t rows = 0;
  if ((rc = rt_band_rows(o->height, band_h, world, &rows))) return rc;
  Mapping mp;
  mp.mode = 1;
  mp.y0 = 0;
  mp.nrows = rows;
  mp.ncols = o->width;
  mp.step = 1;
  mp.max_step = 1;
  mp.band_h = band_h;
  mp.rank = rank;
  mp.world = world;
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  return render_device(s, o, mp, d_bands, (hipStream_t)stream, out);
}

// ---- feature buffers (rt_render_aovs*, rt_fast_aov.h; rt_render_aovs_f64*, rt_kernels_aov64.hip) ----
namespace {

// What all four entry points check before they take the scene's lock.
// precision: the frame's whose features the call renders. oc: the options the
// call goes by — bias, max_ray_depth and every flag outside `keep` are not the
// caller's to matter. *empty: no rows, nothing to do; otherwise a channel must
// be wanted (any).
int aov_check(const rt_scene* s, const rt_options* o, int32_t precision, uint32_t keep, bool any, int32_t y0, int32_t y1,
              rt_options* oc, Mapping* mp, bool* empty) {
  if (precision == RT_FP64 && o->precision == RT_FP32)
    return fail(RT_E_INVALID, "rt_render_aovs_f64 renders the feature buffers of an RT_FP64 frame: "
                              "rt_render_aovs is the RT_FP32 call");
  *oc = *o;
  oc->bias = 0.0;
  oc->max_ray_depth = 0;
  oc->flags = o->flags & keep;
  if (int rc = check_options(s, oc)) return rc;
  if (precision == RT_FP32 && o->precision != RT_FP32)
    return fail(RT_E_UNSUPPORTED, "rt_render_aovs renders the feature buffers of an RT_FP32 frame (precision %d)",
                o->precision);
  // one image row per mapping row
  if (int rc = lines_mapping(oc, y0, y1, 1, 1, mp)) return rc;
  *empty = mp->nrows == 0;
  if (!*empty && !any) return fail(RT_E_INVALID, "no feature buffer requested: every channel is null");
  return RT_OK;
}

// How a feature-buffer call of either precision enters the scene (its lock
// held, its device current): a render-class call — ordered after the scene's
// calls in flight, on the scene's current per-call buffer set, its Stats rows
// the scene's — that classifies nothing, measures no launch order and
// consumes none.
int aov_begin(rt_scene* s, hipStream_t st) {
  s->stats_kept = true;
  if (st != s->done_stream) HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
  // in stream order on the last call's buffer set (no swap: a pipelined
  // sequence of renders alternates as if this call were not there)
  s->timed = false;
  s->pipe = false;
  reset_report(s);
  return RT_OK;
}

// ... and leaves it: `blocks` blocks of four waves left their Stats rows.
int aov_end(rt_scene* s, hipStream_t st, int blocks, rt_stats* out) {
  s->pending_reduce = blocks * 4;
  if (out)
    if (int rc = flush_reduce(s, st)) return rc;
  if (int rc = record_done(s, st)) return rc;
  if (out) return read_stats(s, st, out);
  return RT_OK;
}

// The float32 device body. b's pointers are device memory.
int aov_device(rt_scene* s, const rt_options* o, const Mapping& mp, const rt_aov_buffers& b, hipStream_t st,
               rt_stats* out) {
  if (int rc = aov_begin(s, st)) return rc;
  FastParams p;
  std::memset(&p, 0, sizeof p);
  // the scene words; no light or object grid is reachable from a camera ray
  fast_scene_words(s, RT_FLAG_NO_BINNING, p);
  p.partials = s->partials.p;
  p.queue = s->queue.p;
  fast_camera(s->c2w, s->fov, o, p);
  p.seed = o->seed;
  const Plan pl = plan_mapping(s, o, mp, p.spp, true);
  if (pl.fast_bpc <= 0)
    return fail(RT_E_DEVICE, "the feature-buffer kernel (subset %u) is not resident on this device", pl.sub);
  mapping_words(mp, pl, p.spp, p);
  s->last_general = p.ngroups;
  // per item at most 64 lanes x iters samples x objects hits in one 32-bit counter
  p.stat_flush = (int32_t)std::min<uint64_t>(
      1u << 20, std::max<uint64_t>(1, 0xFFFFFFFFull / (64ull * (uint64_t)p.iters * (uint64_t)std::max(1, s->nobj))));
  p.shards = std::min(kQueueShards, pl.blocks);
  // the queue heads and the Stats accumulator behind them: one fill
  unsigned int* const zero = s->queue.p;
  const int nzero = (int)(rt_scene::kQueueWords + 2 * (size_t)kStatSlots);
  bool zeroed = false;
  // this call's face lists, pixel records and object masks, wherever an
  // RT_FP32 render of these options builds them (plan_kernels' pl.build)
  if (!(o->flags & RT_FLAG_NO_BINNING) && pl.L >= 16 && sampler_in_pixel(o->aa_kind)) {
    bool lists = false, masks = false;
    const bool records = pl.L == 64;
    if (int rc = frame_build(s, o, mp, p, records, false, false, false, zero, nzero, st, &lists, &zeroed)) return rc;
    if (lists) pixel_lists(s, records, p);
    if (s->objbins) {
      if (int rc = frame_obj_masks(s, o, mp, st, &masks)) return rc;
      if (masks) p.obj_pix = s->fr.omask.p;
    }
  }
  if (!zeroed) HIP_TRY(hipMemsetAsync(zero, 0, (size_t)nzero * sizeof(unsigned int), st));
  Aov32Params q;
  q.alpha = b.alpha;
  q.depth = b.depth;
  q.object = b.object;
  q.face = b.face;
  q.normal = b.normal;
  q.albedo = b.albedo;
  q.obj_albedo = s->albedo32.p;
  if (const int e = rtmi_launch_aov_f32(&p, &q, pl.sub, pl.blocks, pl.shmem, st))
    return fail(RT_E_DEVICE, "feature-buffer kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  return aov_end(s, st, pl.blocks, out);
}

// The float64 device body: the float64 render's preparation (prepare_f64) for
// camera rays alone — this call's pixel records and face lists under the
// render's conditions, and no light-grid shadow records: no shadow ray is traced.
int aov64_device(rt_scene* s, const rt_options* o, const Mapping& mp, const rt_aov_buffers64& b, hipStream_t st,
                 rt_stats* out) {
  if (int rc = aov_begin(s, st)) return rc;
  RenderParams<double> p;
  int blocks = 1;
  fill_params<double>(s, s->f64, o, mp, nullptr, p, &blocks);
  s->last_general = p.ngroups;
  const int px = f64_px_wave(o, p.spp) ? 1 : 0;
  bool lists = false;
  if (int rc = prepare_f64(s, o, mp, !(o->flags & RT_FLAG_NO_BINNING), px != 0, rtmi_aov64_batch(),
                           px ? rtmi_aov64_blocks_per_cu() : 0, p, &blocks, st, &lists))
    return rc;
  // the Stats accumulator (behind the queue heads, which no float64 kernel reads)
  HIP_TRY(hipMemsetAsync(s->queue.p + rt_scene::kQueueWords, 0, 2 * (size_t)kStatSlots * sizeof(unsigned int), st));
  Aov64Params q;
  q.alpha = b.alpha;
  q.depth = b.depth;
  q.object = b.object;
  q.face = b.face;
  q.normal = b.normal;
  q.albedo = b.albedo;
  q.obj_albedo = s->albedo64.p;
  if (const int e = rtmi_launch_aov_f64(&p, &q, px, blocks, st))
    return fail(RT_E_DEVICE, "feature-buffer kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  return aov_end(s, st, blocks, out);
}

// What the two precisions' entry points differ in: the buffer struct B, its
// channels' scalar type and bytes per pixel, the device body, and what
// aov_check wants and keeps.
template <class B>
struct Aov;
template <>
struct Aov<rt_aov_buffers> {
  using Scalar = float;
  static constexpr const size_t* px_bytes = kAovPxBytes32;
  static constexpr auto device = &aov_device;
  static constexpr int32_t precision = RT_FP32;
  static constexpr uint32_t keep = RT_FLAG_NO_BINNING;
};
template <>
struct Aov<rt_aov_buffers64> {
  using Scalar = double;
  static constexpr const size_t* px_bytes = kAovPxBytes64;
  static constexpr auto device = &aov64_device;
  static constexpr int32_t precision = RT_FP64;
  static constexpr uint32_t keep = RT_FLAG_NO_BINNING | RT_FLAG_F64_PER_LANE;
};

// The frame of both forms: the checks; no rows: zero Stats; else body(oc, mp)
// with the scene's lock held and its device current.
template <class B, class Body>
int aov_call(rt_scene* s, const rt_options* o, const B* b, int32_t y0, int32_t y1, rt_stats* out, Body body) {
  if (!s || !o || !b) return fail(RT_E_INVALID, "null argument");
  rt_options oc;
  Mapping mp;
  bool empty = false;
  const bool any = b->alpha || b->depth || b->object || b->face || b->normal || b->albedo;
  if (int rc = aov_check(s, o, Aov<B>::precision, Aov<B>::keep, any, y0, y1, &oc, &mp, &empty)) return rc;
  if (empty) {
    if (out) *out = rt_stats{};
    return RT_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  return body(oc, mp);
}

// Device form: d_out's pointers are device memory.
template <class B>
int aov_device_form(rt_scene* s, const rt_options* o, const B* d_out, int32_t y0, int32_t y1, void* stream,
                    rt_stats* out) {
  return aov_call(s, o, d_out, y0, y1, out, [&](const rt_options& oc, const Mapping& mp) {
    return Aov<B>::device(s, &oc, mp, *d_out, (hipStream_t)stream, out);
  });
}

// Host form: the wanted channels' device copies in the scene's staging buffer
// (rt_stage.h), rendered on the scene's own stream; rows [y0, y1) come back,
// then the call's Stats (which waits for the stream: the copies have landed).
template <class B>
int aov_host_form(rt_scene* s, const rt_options* o, const B* out_bufs, int32_t y0, int32_t y1, rt_stats* out) {
  using S = typename Aov<B>::Scalar;
  return aov_call(s, o, out_bufs, y0, y1, out, [&](const rt_options& oc, const Mapping& mp) -> int {
    void* const host[kAovChannels] = {out_bufs->alpha, out_bufs->depth,  out_bufs->object,
                                      out_bufs->face,  out_bufs->normal, out_bufs->albedo};
    const StageLayout l = aov_stage_layout(host, Aov<B>::px_bytes, (size_t)o->width * (size_t)o->height);
    // (the staging buffer's last user was a host call, which waited for its copies)
    if (s->aov_stage.n < l.total)
      if (int rc = s->aov_stage.alloc(l.total)) return rc;
    unsigned char* const base = s->aov_stage.p;
    B d{};
    d.alpha = host[0] ? (S*)(base + l.off[0]) : nullptr;
    d.depth = host[1] ? (S*)(base + l.off[1]) : nullptr;
    d.object = host[2] ? (int32_t*)(base + l.off[2]) : nullptr;
    d.face = host[3] ? (int32_t*)(base + l.off[3]) : nullptr;
    d.normal = host[4] ? (S*)(base + l.off[4]) : nullptr;
    d.albedo = host[5] ? (S*)(base + l.off[5]) : nullptr;
    hipStream_t st = s->stream;
    if (int rc = Aov<B>::device(s, &oc, mp, d, st, nullptr)) return rc;
    for (int c = 0; c < kAovChannels; ++c) {
      if (!host[c]) continue;
      size_t begin, count;
      aov_stage_rows(Aov<B>::px_bytes[c], o->width, y0, y1, &begin, &count);
      HIP_TRY(hipMemcpyAsync((unsigned char*)host[c] + begin, base + l.off[c] + begin, count, hipMemcpyDeviceToHost,
                             st));
    }
    rt_stats local{};
    if (int rc = flush_reduce(s, st)) return rc;
    if (int rc = read_stats(s, st, &local)) return rc;
    if (out) *out = local;
    return RT_OK;
  });
}

}  // namespace

extern "C" int rt_render_aovs_device(rt_scene* s, const rt_options* o, const rt_aov_buffers* d_out, int32_t y0,
                                     int32_t y1, void* stream, rt_stats* out) {
  return aov_device_form(s, o, d_out, y0, y1, stream, out);
}

extern "C" int rt_render_aovs(rt_scene* s, const rt_options* o, const rt_aov_buffers* out_bufs, int32_t y0, int32_t y1,
                              rt_stats* out) {
  return aov_host_form(s, o, out_bufs, y0, y1, out);
}

extern "C" int rt_render_aovs_f64_device(rt_scene* s, const rt_options* o, const rt_aov_buffers64* d_out, int32_t y0,
                                         int32_t y1, void* stream, rt_stats* out) {
  return aov_device_form(s, o, d_out, y0, y1, stream, out);
}

extern "C" int rt_render_aovs_f64(rt_scene* s, const rt_options* o, const rt_aov_buffers64* out_bufs, int32_t y0,
                                  int32_t y1, rt_stats* out) {
  return aov_host_form(s, o, out_bufs, y0, y1, out);
}

extern "C" int rt_scene_last_stats(rt_scene* s, rt_stats* out) {
  if (!s || !out) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->stats_kept) return fail(RT_E_INVALID, "the last render call set RT_FLAG_NO_STATS");
  DeviceGuard g(s->device);
  HIP_TRY(hipStreamWaitEvent(s->stream, s->done, 0));
  if (int rc = flush_reduce(s, s->stream)) return rc;
  return read_stats(s, s->stream, out);
}

extern "C" int rt_scene_last_timing(rt_scene* s, double* setup_ms, double* render_ms) {
  if (!s || !setup_ms || !render_ms) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->timed) return fail(RT_E_INVALID, "the last render call did not set RT_FLAG_TIMING");
  DeviceGuard g(s->device);
  float a = 0.0f, b = 0.0f;
  HIP_TRY(hipEventSynchronize(s->tev[2]));
  HIP_TRY(hipEventElapsedTime(&a, s->tev[0], s->tev[1]));
  HIP_TRY(hipEventElapsedTime(&b, s->tev[1], s->tev[2]));
  *setup_ms = a;
  *render_ms = b;
  return RT_OK;
}

namespace {
// The last launch's lean / general list lengths: counted on the device by
// its k_frame_build2 (read back here, after the call completed), or the
// host's (a one-kernel launch: every group general).
int last_lists(rt_scene* s, int64_t* lean, int64_t* general) {
  if (!s->fr.counted) {
    *lean = s->last_lean;
    *general = s->last_general;
    return RT_OK;
  }
  DeviceGuard g(s->device);
  int32_t c[FC_WORDS];
  HIP_TRY(hipEventSynchronize(s->done));
  HIP_TRY(hipMemcpy(c, s->fr.ctr.p, sizeof c, hipMemcpyDeviceToHost));
  *lean = c[FC_LEAN];
  *general = c[FC_HEAVY];
  return RT_OK;
}
}  // namespace

extern "C" int rt_scene_last_split(rt_scene* s, int64_t* lean_groups, int64_t* general_groups) {
  if (!s || !lean_groups || !general_groups) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  return last_lists(s, lean_groups, general_groups);
}

extern "C" int rt_scene_last_uniform(rt_scene* s, int32_t* lit, int32_t* sky) {
  if (!s || !lit || !sky) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  *lit = 0;
  *sky = 0;
  if (!s->fr.counted || !s->fr.uniform) return RT_OK;
  DeviceGuard g(s->device);
  std::vector<uint32_t> c((size_t)s->fr.uni_rows);
  HIP_TRY(hipEventSynchronize(s->done));
  HIP_TRY(hipMemcpy(c.data(), s->fr.uni_cls.p, c.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (const uint32_t v : c) {
    *lit += (int32_t)(v >> 16);
    *sky += (int32_t)(v & 0xffu);
  }
  return RT_OK;
}

extern "C" int rt_scene_last_ground(rt_scene* s, int32_t* ground) {
  if (!s || !ground) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  *ground = 0;
  if (!s->fr.counted || !s->fr.ground) return RT_OK;
  DeviceGuard g(s->device);
  std::vector<uint32_t> c((size_t)s->fr.uni_rows);
  HIP_TRY(hipEventSynchronize(s->done));
  HIP_TRY(hipMemcpy(c.data(), s->fr.uni_cls.p, c.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (const uint32_t v : c) *ground += (int32_t)((v >> 8) & 0xffu);
  return RT_OK;
}

extern "C" int rt_scene_last_mesh1(rt_scene* s, int64_t* straight_batches) {
  if (!s || !straight_batches) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->stats_kept) return fail(RT_E_INVALID, "the last render call set RT_FLAG_NO_STATS");
  // the slot is the straight-path count only where gen1_loop ran uninstrumented
  *straight_batches = s->mesh1 ? s->last_straight : 0;
  return RT_OK;
}

extern "C" int rt_scene_last_lean_kernel(rt_scene* s, int32_t* kind) {
  if (!s || !kind) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  *kind = s->last_lean_kind;
  return RT_OK;
}

extern "C" int rt_scene_last_batch(rt_scene* s, int64_t* batched_groups, int64_t* fallback_groups) {
  if (!s || !batched_groups || !fallback_groups) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  *batched_groups = s->last_batched;
  if (s->last_batched < 0) {  // the general list of a two-class launch, counted on the device
    int64_t lean = 0;
    const int rc = last_lists(s, &lean, batched_groups);
    if (rc) return rc;
  }
  *fallback_groups = s->last_fallback;
  return RT_OK;
}

extern "C" int rt_scene_last_counters(rt_scene* s, rt_traversal_counters* out) {
  if (!s || !out) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  // a call without Stats (RT_FLAG_NO_STATS) reduced nothing: its counters
  // are not in the accumulator
  if (!s->stats_kept) return fail(RT_E_INVALID, "the last render call set RT_FLAG_NO_STATS");
  DeviceGuard g(s->device);
  unsigned long long h[kStatSlots];
  HIP_TRY(hipStreamWaitEvent(s->stream, s->done, 0));
  if (int rc = flush_reduce(s, s->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(h, s->acc(), sizeof h, hipMemcpyDeviceToHost));
  out->wave_node_fetches = h[STAT_NODE_FETCH];
  out->wave_tri_fetches = h[STAT_TRI_FETCH];
  out->lane_node_visits = h[STAT_LANE_NODES];
  // (an uninstrumented gen1_loop launch keeps its straight-path batches in
  // this slot, rt_scene_last_mesh1: no traversal counter)
  out->lane_tri_tests = s->mesh1 ? 0 : h[STAT_LANE_TRIS];
  return RT_OK;
}
