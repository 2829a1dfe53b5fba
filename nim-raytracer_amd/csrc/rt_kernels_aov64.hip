// rt_kernels_aov64.hip — the feature buffers of an RT_FP64 frame
// (include/rtmi.h rt_render_aovs_f64*): per pixel the coverage, the closest
// sample's depth and ids, and the sums of the hit normals and albedos over
// the frame's own samples, in the float64 arithmetic of the parity render.
// Built with -ffp-contract=off like rt_kernels_f64.hip.
//
// Only camera rays are traced: castPrimaryRay and trace (renderer.nim:31-67)
// exactly as the RT_FP64 render runs them, then k_trace_rays' hitNormal
// (rt_device.h hit_normal), so a sample's hit is rt_pick_pixels' at its
// position bit for bit. The sums follow calcPixel's order (renderer.nim:
// 147-159): from +0, the hitting samples' values in sample-index order, one
// product with inv_len at the end — so a channel has one correct bit pattern
// whatever the layout. (A sum that starts at +0 is never -0, so adding +0 for
// a sample that misses leaves its bits alone: the one-pixel-per-wave layout
// does that.)
//
// Two layouts, the two float64 render kernels': k_aov64_lane is k_render's
// (one lane per pixel, the samples in order in that lane), k_aov64_px is
// k_render_px64's (one pixel per wave, lane l takes sample 64 it + l, the
// pixel's face list serves its rays, LDS rows carry the addends to a few
// lanes that add them in sample order).
#include "rt_aov64.h"
#include "rt_device.h"

#ifndef RTMI_AOV64_P
#define RTMI_AOV64_P 4  // pixels per wave batch (k_aov64_px)
#endif

namespace rtmi {

// A pixel's record says its list is empty: no camera ray of it can hit the mesh.
__device__ __forceinline__ bool aov64_cam_skip(unsigned pinfo) { return (pinfo & kPixCount) == 0u; }

// ---- layout 1: one lane per pixel -------------------------------------------
// k_render<double>'s tiles (8 x 8 pixels per wave), mode 0 with step 1, and
// its per-lane sample tables for the stochastic kinds.
__global__ __launch_bounds__(256) void k_aov64_lane(const RenderParams<double> params_by_value, const Aov64Params q) {
  using R = double;
  (void)params_by_value;  // read through rparams()
  const RT_CONST RenderParams<R>& p = rparams<R>();
  const int lane = (int)__lane_id();
  const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const int tpx = lane % p.tile_x, tpy = lane / p.tile_x;
  const bool grid_aa = p.aa_kind != 0;
  WaveStats ws;
#pragma unroll
  for (int k = 0; k < kStatSlots; ++k) ws.v[k] = 0u;
  unsigned long long tot = 0ull;
  // castPrimaryRay's origin: cameraToWorld * (0, 0, 0, 1), the same for every sample
  const V3<R> o = xform<R>(p.c2w, V3<R>{R(0), R(0), R(0)}, R(1));

  for (long long g = wave; g < p.ngroups; g += nwaves) {
    const int gx = (int)(g % p.tiles_x), gy = (int)(g / p.tiles_x);
    const int x = gx * p.tile_x + tpx;
    const int k = gy * p.tile_y + tpy;
    const int y = p.y0 + k;
    const bool valid = x < p.ncols && k < p.nrows;
    const unsigned pinfo = (p.pix_info && valid) ? p.pix_info[(size_t)y * p.width + x] : kPixCount;
    const bool no_mesh = aov64_cam_skip(pinfo);
    // stochastic kinds: this lane's pixel table, as k_render builds it
    R* tsx = nullptr;
    R* tsy = nullptr;
    if (p.aa_kind >= 2 && valid) {
      tsx = p.sample_scratch + (size_t)(wave * 64 + lane) * 2 * (size_t)p.spp;
      tsy = tsx + p.spp;
      sample_table_seq<R>(p.aa_kind, p.grid_m, rng_pixel_key(p.seed, x, y), tsx, tsy);
    }
    int hits = 0, bobj = -1, bface = -1;
    R bt = pinf<R>();
    V3<R> nsum{R(0), R(0), R(0)}, asum{R(0), R(0), R(0)};
    for (int s = 0; s < p.spp; ++s) {
      R px = R(x), py = R(y);
      if (tsx) {
        px = R(x) + tsx[s];
        py = R(y) + tsy[s];
      } else if (grid_aa) {  // grid() sampling.nim:5-18, p[j*m + i]
        const int si = s % p.grid_m, sj = s / p.grid_m;
        px = R(x) + (R(si) * p.sample_step + p.sample_off);
        py = R(y) + (R(sj) * p.sample_step + p.sample_off);
      }
      // castPrimaryRay (renderer.nim:31-44)
      const R cx = (Prec<R>::div(R(2) * px * p.aspect, R(p.width)) - p.aspect) * p.f;
      const R cy = (R(1) - Prec<R>::div(R(2) * py, R(p.height))) * p.f;
      const V3<R> dn = normalize_dir<R>(V3<R>{cx, cy, R(-1)});
      const V3<R> d = xform<R>(p.c2w, dn, R(0));
      ws.v[STAT_PRIMARY] += popc32(ballot(valid));
      const Hit<R> h = trace<R, false>(p, o, d, pinf<R>(), valid, false, ws, no_mesh);
      const bool lit = valid && h.obj >= 0;
      if (q.normal) {
        const V3<R> N = hit_normal(p, o, d, h, lit);
        if (lit) nsum = V3<R>{nsum.x + N.x, nsum.y + N.y, nsum.z + N.z};
      }
      if (q.albedo && lit) {
        const R* a = q.obj_albedo + 3 * (size_t)h.obj;
        asum = V3<R>{asum.x + a[0], asum.y + a[1], asum.z + a[2]};
      }
      if (lit) {
        ++hits;
        if (h.t < bt) {  // strict: a tie stays with the lower sample index
          bt = h.t;
          bobj = h.obj;
          bface = h.tri;
        }
      }
      if ((s & 63) == 63) flush_stats(ws, tot, lane);  // k_render's interval
    }
    flush_stats(ws, tot, lane);
    if (valid) {
      const size_t i = (size_t)y * p.width + x;
      if (q.alpha) q.alpha[i] = R(hits) * p.inv_len;
      if (q.depth) q.depth[i] = bt;
      if (q.object) q.object[i] = bobj;
      if (q.face) q.face[i] = bface;
      if (q.normal) {
        R* n = q.normal + 3 * i;
        n[0] = nsum.x * p.inv_len; n[1] = nsum.y * p.inv_len; n[2] = nsum.z * p.inv_len;
      }
      if (q.albedo) {
        R* a = q.albedo + 3 * i;
        a[0] = asum.x * p.inv_len; a[1] = asum.y * p.inv_len; a[2] = asum.z * p.inv_len;
      }
    }
  }
  if (lane < kStatSlots) p.partials[wave * kStatSlots + lane] = tot;
}

// ---- layout 2: one pixel per wave ---------------------------------------------
// akGrid with >= 64 samples per pixel. A wave takes P pixels at a time; step
// `it` of pixel j traces samples 64 it + lane through the pixel's face list
// and leaves each lane's six addends (normal, albedo; +0 for a miss) in the
// wave's LDS rows 6 j .. 6 j + 5; then lane 6 j + c adds row 6 j + c to its
// running sum in sample order, the 6 P chains side by side, before the next
// step overwrites the rows. A pixel none of whose 64 samples hit in a step
// stages nothing and its chains rest. The hit count is a popcount and the
// (t, sample) minimum an exact reduction: each lane keeps its own best (its
// samples come in rising order), the lanes are compared once per batch.
template <int P>
__global__ __launch_bounds__(256) void k_aov64_px(const RenderParams<double> params_by_value, const Aov64Params q) {
  using R = double;
  (void)params_by_value;  // read through rparams()
  const RT_CONST RenderParams<R>& p = rparams<R>();
  static_assert(6 * P <= 64, "one summing lane per pixel and addend: 6 P lanes of the wave");
  static_assert(kCacheCamO == 0, "cam_o is the head of trace()'s cache layout");
  constexpr int kRow = 66;  // k_render_px64's rows: 16-B aligned, 4 banks apart
  __shared__ __attribute__((aligned(16))) double sbuf[4][P * 6 * kRow];
  // trace()'s cache, its kCacheCamO part alone (no shadow ray reads the rest):
  // each object's view of the camera origin, formed once per block
  __shared__ double cam_o[4 * kCacheObj];
  const int lane = (int)__lane_id();
  const int wib = (int)(threadIdx.x >> 6);
  double* buf = sbuf[wib];
  const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + wib;
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const int iters = (p.spp + 63) / 64;
  const long long npx = (long long)p.nrows * p.ncols;
  const long long nbatch = (npx + P - 1) / P;
  WaveStats ws;
#pragma unroll
  for (int k = 0; k < kStatSlots; ++k) ws.v[k] = 0u;
  unsigned long long tot = 0ull;
  const V3<R> o = xform<R>(p.c2w, V3<R>{R(0), R(0), R(0)}, R(1));
  const bool use_cache = p.nobj <= kCacheObj;
  if (use_cache) {
    for (int i = (int)threadIdx.x; i < p.nobj; i += (int)blockDim.x) {
      const RT_CONST DevObject<R>& ob = cptr(p.objects)[i];
      const V3<R> ro = xform_xf<R, true>(ob.xf, ob.w2o, o);
      cam_o[4 * i + 0] = ro.x; cam_o[4 * i + 1] = ro.y; cam_o[4 * i + 2] = ro.z;
    }
    __syncthreads();
  }
  const double* cch = use_cache ? cam_o : nullptr;
  const int cj = lane / 6 < P ? lane / 6 : 0;  // the pixel of this lane's chain (lanes < 6 P)

  for (long long b = wave; b < nbatch; b += nwaves) {
    // the batch's pixels, pixel j in lane j < P: image position and record
    int bx = 0, by = 0;
    unsigned binfo = kPixCount;
    bool bok = false;
    if (lane < P) {
      const long long g = b * P + lane;
      bok = g < npx;
      if (bok) {
        bx = (int)(g % p.ncols);
        by = p.y0 + (int)(g / p.ncols);
        if (p.pix_info) binfo = p.pix_info[(size_t)by * p.width + bx];
      }
    }
    const unsigned long long okm = ballot(bok);
    R acc = R(0);  // lane 6 j + c: addend c of pixel j, summed in sample order
    int cnt = 0;   // lane j: pixel j's hitting samples
    // this lane's closest hit among its samples of pixel k
    R bt[P];
    int bobj[P], bface[P], bs[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      bt[k] = pinf<R>();
      bobj[k] = -1;
      bface[k] = -1;
      bs[k] = 0x7fffffff;
    }
    for (int it = 0; it < iters; ++it) {
      const int s = it * 64 + lane;
      const bool sv = s < p.spp;
      const int si = s % p.grid_m, sj = s / p.grid_m;
      unsigned staged = 0u;  // bit j: pixel j staged addends this step
      int cy_row = -1;
      R cy = R(0);
      for (int j = 0; j < P; ++j) {
        if (!((okm >> j) & 1ull)) continue;
        const int x = __builtin_amdgcn_readlane(bx, j), y = __builtin_amdgcn_readlane(by, j);
        const unsigned pinfo = (unsigned)__builtin_amdgcn_readlane((int)binfo, j);
        const int pix = y * p.width + x;
        // grid() sampling.nim:5-18, p[j*m + i]; castPrimaryRay (renderer.nim:31-44)
        const R px = R(x) + (R(si) * p.sample_step + p.sample_off);
        if (y != cy_row) {
          const R py = R(y) + (R(sj) * p.sample_step + p.sample_off);
          cy = (R(1) - Prec<R>::div(R(2) * py, R(p.height))) * p.f;
          cy_row = y;
        }
        const R cx = (Prec<R>::div(R(2) * px * p.aspect, R(p.width)) - p.aspect) * p.f;
        const V3<R> dn = normalize_dir<R>(V3<R>{cx, cy, R(-1)});
        const V3<R> d = xform<R>(p.c2w, dn, R(0));
        ws.v[STAT_PRIMARY] += popc32(ballot(sv));
        const Hit<R> h = trace<R, false, true>(rparams<R>(), o, d, pinf<R>(), sv, false, ws, aov64_cam_skip(pinfo), pix,
                                               pinfo, -1, cch, true);
        const bool lit = sv && h.obj >= 0;
        const unsigned long long litm = ballot(lit);
        if (litm == 0ull) continue;
        staged |= 1u << j;
        cnt += lane == j ? (int)popc32(litm) : 0;
        V3<R> N{R(0), R(0), R(0)}, A{R(0), R(0), R(0)};
        if (q.normal) N = hit_normal(rparams<R>(), o, d, h, lit);
        if (q.albedo && lit) {
          const R* a = q.obj_albedo + 3 * (size_t)h.obj;
          A = V3<R>{a[0], a[1], a[2]};
        }
        double* row = buf + j * 6 * kRow + lane;
        row[0 * kRow] = N.x; row[1 * kRow] = N.y; row[2 * kRow] = N.z;
        row[3 * kRow] = A.x; row[4 * kRow] = A.y; row[5 * kRow] = A.z;
#pragma unroll
        for (int k = 0; k < P; ++k) {
          const bool better = k == j && lit && h.t < bt[k];  // strict: this lane's samples rise with `it`
          bt[k] = better ? h.t : bt[k];
          bobj[k] = better ? h.obj : bobj[k];
          bface[k] = better ? h.tri : bface[k];
          bs[k] = better ? s : bs[k];
        }
      }
      // the rows are read by other lanes of this wave: LDS operations of one
      // wave complete in order, the barrier keeps the compiler from moving
      // the reads above the writes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (lane < 6 * P && ((staged >> cj) & 1u)) {
        const double* row = buf + lane * kRow;
        const int nv = min(64, p.spp - it * 64);
        if (nv == 64) {
          const double2* r2 = (const double2*)row;
#pragma unroll 8
          for (int k = 0; k < 32; ++k) {
            const double2 v = r2[k];
            acc = acc + v.x;
            acc = acc + v.y;
          }
        } else {
          for (int k = 0; k < nv; ++k) acc = acc + row[k];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // k_render_px64's interval: STAT_TESTS grows by 64 x nobj per trace, P traces per step
      if ((it & 15) == 15) flush_stats(ws, tot, lane);
    }
    flush_stats(ws, tot, lane);
    // pixel k's closest hit over the lanes — the smallest (t, sample index) —
    // to lane k
    R ft = pinf<R>();
    int fobj = -1, fface = -1;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      R t = bt[k];
      int sm = bs[k], ob = bobj[k], fa = bface[k];
      for (int off = 1; off < 64; off <<= 1) {
        const R t2 = __shfl_xor(t, off);
        const int s2 = __shfl_xor(sm, off), o2 = __shfl_xor(ob, off), f2 = __shfl_xor(fa, off);
        const bool take = t2 < t || (t2 == t && s2 < sm);
        t = take ? t2 : t;
        sm = take ? s2 : sm;
        ob = take ? o2 : ob;
        fa = take ? f2 : fa;
      }
      if (lane == k) {
        ft = t;
        fobj = ob;
        fface = fa;
      }
    }
    if (bok) {  // lanes j < P
      const size_t i = (size_t)by * p.width + bx;
      if (q.alpha) q.alpha[i] = R(cnt) * p.inv_len;
      if (q.depth) q.depth[i] = ft;
      if (q.object) q.object[i] = fobj;
      if (q.face) q.face[i] = fface;
    }
    // lane 6 j + c holds addend c of pixel j: normal 0..2, albedo 3..5
    const int ox = __shfl(bx, cj), oy = __shfl(by, cj);
    if (lane < 6 * P && ((okm >> cj) & 1ull)) {
      const size_t i = (size_t)oy * p.width + ox;
      const int c = lane - 6 * cj;
      R* dst = c < 3 ? q.normal : q.albedo;
      if (dst) dst[3 * i + (c < 3 ? c : c - 3)] = acc * p.inv_len;
    }
  }
  if (lane < kStatSlots) p.partials[wave * kStatSlots + lane] = tot;
}

template __global__ void k_aov64_px<RTMI_AOV64_P>(const RenderParams<double>, const Aov64Params);

}  // namespace rtmi

extern "C" int rtmi_launch_aov_f64(const rtmi::RenderParams<double>* p, const rtmi::Aov64Params* q, int px, int blocks,
                                   void* stream) {
  if (px)
    hipLaunchKernelGGL((rtmi::k_aov64_px<RTMI_AOV64_P>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, *q);
  else
    hipLaunchKernelGGL(rtmi::k_aov64_lane, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, *q);
  return (int)hipGetLastError();
}

extern "C" int rtmi_aov64_blocks_per_cu() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)rtmi::k_aov64_px<RTMI_AOV64_P>, 256, 0) != hipSuccess)
    return 0;
  return n;
}

extern "C" int rtmi_aov64_batch() { return RTMI_AOV64_P; }
