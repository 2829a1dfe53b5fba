// rt_kernels_f32.hip — float (performance mode) instantiation of the render
// kernel, plus the precision-independent helper kernels (stats reduction,
// multi-GPU band un-interleave). Built with FMA contraction on.
#include <algorithm>
#include <cstdlib>

#include "rt_fast.h"

namespace rtmi {

// Sum per-wave partial counters into acc (acc accumulates across launches
// until the host clears it). Each block folds kWavesPerBlock waves in
// registers, then one atomic per counter per block.
constexpr int kWavesPerBlock = 256;
__global__ __launch_bounds__(256) void k_reduce_stats(const unsigned long long* __restrict__ partials,
                                                      int num_waves, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long red[kStatSlots][256];
  const int w = blockIdx.x * kWavesPerBlock + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kStatSlots; ++k) red[k][threadIdx.x] = w < num_waves ? partials[(size_t)w * kStatSlots + k] : 0ull;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
#pragma unroll
      for (int k = 0; k < kStatSlots; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < kStatSlots) atomicAdd(&acc[threadIdx.x], red[threadIdx.x][0]);
}

// Rank-0 epilogue of the framebuffer gather: gathered = world compact band
// buffers back to back, each band_rows rows; image row y lives in band
// b = y / band_h owned by rank b % world as local band b / world.
__global__ __launch_bounds__(256) void k_unshard(const float4* __restrict__ gathered, float4* __restrict__ fb,
                                                 int row_f4, int height, int band_h, int world, int band_rows) {
  const int y = blockIdx.x;
  if (y >= height) return;
  const int b = y / band_h, r = y % band_h;
  const int owner = b % world, lb = b / world;
  const size_t src_row = (size_t)owner * band_rows + (size_t)lb * band_h + r;
  const float4* src = gathered + src_row * row_f4;
  float4* dst = fb + (size_t)y * row_f4;
  for (int i = threadIdx.x; i < row_f4; i += blockDim.x) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_unshard_scalar(const float* __restrict__ gathered, float* __restrict__ fb,
                                                        int row_f, int height, int band_h, int world, int band_rows) {
  const int y = blockIdx.x;
  if (y >= height) return;
  const int b = y / band_h, r = y % band_h;
  const int owner = b % world, lb = b / world;
  const size_t src_row = (size_t)owner * band_rows + (size_t)lb * band_h + r;
  for (int i = threadIdx.x; i < row_f; i += blockDim.x) fb[(size_t)y * row_f + i] = gathered[src_row * row_f + i];
}

// After k_render_wave: the framebuffer's pixels += their queued rays'
// radiance (p->sec, 32.32 fixed point), scaled like the pixel's level-0 sum
// (calcPixel's 1 / len, renderer.nim:159).
__global__ __launch_bounds__(256) void k_sec_add(float* __restrict__ fb, const long long* __restrict__ sec, size_t n,
                                                 float scale) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const long long v = sec[i];
    if (v != 0) fb[i] += (float)((double)v * 0x1p-32) * scale;
  }
}

// After k_shade_rays_f32 with group > 1: the render's pixel sum over each run
// of `group` ray colours — from +0, added in index order in float32 (one
// thread per output walks its run, never a tree, so the sum does not depend
// on how the batch was split), then one multiplication by inv_len. The adds
// and the multiply stay apart (nothing here can contract).
__global__ __launch_bounds__(256) void k_shade_reduce32(const float* __restrict__ ray_rgb, long long ngroups, int group,
                                                        float inv_len, float* __restrict__ rgb) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ngroups) return;
  const float* c = ray_rgb + 3 * k * group;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  for (int j = 0; j < group; ++j) {
    x = x + c[3 * j];
    y = y + c[3 * j + 1];
    z = z + c[3 * j + 2];
  }
  rgb[3 * k] = x * inv_len;
  rgb[3 * k + 1] = y * inv_len;
  rgb[3 * k + 2] = z * inv_len;
}

// the instrumented (RT_FLAG_COUNT_TRAVERSAL) kernel: all features
template __global__ void fast::k_render_fast<true, fast::F_ALL>(const FastParams);
// lean pixels of one-plane scenes (rt_render.cpp lean1_ok), one or two lights, 4 or 16 lanes per pixel
template __global__ void fast::k_render_lean1q<1, 4>(const FastParams);
template __global__ void fast::k_render_lean1q<2, 4>(const FastParams);
template __global__ void fast::k_render_lean1q<1, 16>(const FastParams);
template __global__ void fast::k_render_lean1q<2, 16>(const FastParams);
// general pixels of the same scenes
template __global__ void fast::k_render_gen1<1>(const FastParams);
template __global__ void fast::k_render_gen1<2>(const FastParams);
// both classes of a one-plane launch in one kernel
template __global__ void fast::k_render_mix1<1, 4>(const FastParams);
template __global__ void fast::k_render_mix1<2, 4>(const FastParams);
template __global__ void fast::k_render_mix1<1, 16>(const FastParams);
template __global__ void fast::k_render_mix1<2, 16>(const FastParams);

}  // namespace rtmi

// feature-subset specialisations: rt_kernels_f32_part.hip, 16 objects, each
// exporting the address of kernel (family, subset) for its 8 subsets
#define RTMI_PART_DECL(k) extern "C" const void* rtmi_f32_kernel_part##k(int, unsigned);
RTMI_PART_DECL(0) RTMI_PART_DECL(1) RTMI_PART_DECL(2) RTMI_PART_DECL(3)
RTMI_PART_DECL(4) RTMI_PART_DECL(5) RTMI_PART_DECL(6) RTMI_PART_DECL(7)
RTMI_PART_DECL(8) RTMI_PART_DECL(9) RTMI_PART_DECL(10) RTMI_PART_DECL(11)
RTMI_PART_DECL(12) RTMI_PART_DECL(13) RTMI_PART_DECL(14) RTMI_PART_DECL(15)
#undef RTMI_PART_DECL

namespace {

// Kernel (family: rt_common.h K32_*) of a feature subset; null: the family
// has none for the subset.
const void* subset_kernel(int family, unsigned subset) {
#define RTMI_K(k) rtmi_f32_kernel_part##k
  static const void* (*const kPart[16])(int, unsigned) = {
      RTMI_K(0), RTMI_K(1), RTMI_K(2),  RTMI_K(3),  RTMI_K(4),  RTMI_K(5),  RTMI_K(6),  RTMI_K(7),
      RTMI_K(8), RTMI_K(9), RTMI_K(10), RTMI_K(11), RTMI_K(12), RTMI_K(13), RTMI_K(14), RTMI_K(15)};
#undef RTMI_K
  return kPart[(subset >> 3) & 15u](family, subset & 127u);
}

// The one-plane kernels (rt_render.cpp lean1_ok) for nl (1 or 2) distant
// lights: lean (k_render_lean1q) and merged (k_render_mix1) with lp (4 or 16)
// lanes per lean pixel, and the batched general one; null: no such kernel.
const void* lean1_kernel(bool mix, int nl, int lp) {
  using namespace rtmi::fast;
  static const void* const k[2][2][2] = {
      {{(const void*)k_render_lean1q<1, 4>, (const void*)k_render_lean1q<1, 16>},
       {(const void*)k_render_lean1q<2, 4>, (const void*)k_render_lean1q<2, 16>}},
      {{(const void*)k_render_mix1<1, 4>, (const void*)k_render_mix1<1, 16>},
       {(const void*)k_render_mix1<2, 4>, (const void*)k_render_mix1<2, 16>}}};
  if ((nl != 1 && nl != 2) || (lp != 4 && lp != 16)) return nullptr;
  return k[mix ? 1 : 0][nl - 1][lp == 16 ? 1 : 0];
}

const void* gen1_kernel(int nl) {
  return nl == 1   ? (const void*)rtmi::fast::k_render_gen1<1>
         : nl == 2 ? (const void*)rtmi::fast::k_render_gen1<2>
                   : nullptr;
}

// Every float32 render kernel takes the FastParams by value, 256 threads per
// block. fn null: `missing`.
int launch_f32(const void* fn, hipError_t missing, const rtmi::FastParams* p, int blocks, size_t shmem, void* stream) {
  if (!fn) return (int)missing;
  void* args[] = {const_cast<rtmi::FastParams*>(p)};
  (void)hipLaunchKernel(fn, dim3(blocks), dim3(256), args, shmem, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// Resident 256-thread blocks per CU of a kernel (grid sizing for the
// work-queue loops: launch exactly what fits, waves pull items); 1 when the
// runtime cannot say. fn null: `missing`.
int blocks_per_cu(const void* fn, int missing, size_t shmem) {
  if (!fn) return missing;
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, shmem);
  return e == hipSuccess && nb > 0 ? nb : 1;
}

const void* count_kernel() { return (const void*)rtmi::fast::k_render_fast<true, rtmi::fast::F_ALL>; }

}  // namespace

// The reflection-compacting kernel of a reflective feature subset.
extern "C" int rtmi_launch_wave_f32(const rtmi::FastParams* p, unsigned subset, int blocks, size_t shmem,
                                    void* stream) {
  return launch_f32(subset_kernel(rtmi::K32_WAVE, subset), hipErrorInvalidDeviceFunction, p, blocks, shmem, stream);
}

// Resident blocks per CU of the reflection-compacting kernel; 0: none for the subset.
extern "C" int rtmi_wave_f32_blocks_per_cu(unsigned subset, size_t shmem) {
  return blocks_per_cu(subset_kernel(rtmi::K32_WAVE, subset), 0, shmem);
}

// fb[i] += sec[i] (32.32 fixed point) * scale where sec[i] != 0, i < n
extern "C" int rtmi_launch_sec_add(float* fb, const long long* sec, size_t n, float scale, int num_cus, void* stream) {
  const size_t want = (n + 255) / 256;
  const unsigned blocks = (unsigned)std::min<size_t>(want > 0 ? want : 1, (size_t)num_cus * 16);
  hipLaunchKernelGGL(rtmi::k_sec_add, dim3(blocks), dim3(256), 0, (hipStream_t)stream, fb, sec, n, scale);
  return (int)hipGetLastError();
}

// The batched general-pixel kernel of a feature subset (two-class launches).
extern "C" int rtmi_launch_gen_f32(const rtmi::FastParams* p, unsigned subset, int blocks, size_t shmem,
                                   void* stream) {
  return launch_f32(subset_kernel(rtmi::K32_GEN, subset), hipErrorInvalidDeviceFunction, p, blocks, shmem, stream);
}

// Resident blocks per CU of the batched general kernel; 0: none for the subset.
extern "C" int rtmi_gen_f32_blocks_per_cu(unsigned subset, size_t shmem) {
  return blocks_per_cu(subset_kernel(rtmi::K32_GEN, subset), 0, shmem);
}

// The float32 radiance-query kernel of a non-stochastic feature subset
// (rt_fast_shade.h): its arguments are the FastParams, then the batch.
extern "C" int rtmi_launch_shade_f32(const rtmi::FastParams* p, const rtmi::Shade32Params* q, unsigned subset,
                                     int blocks, void* stream) {
  const void* fn = subset < 64u ? subset_kernel(rtmi::K32_SHADE, subset) : nullptr;
  if (!fn) return (int)hipErrorInvalidDeviceFunction;
  void* args[] = {const_cast<rtmi::FastParams*>(p), const_cast<rtmi::Shade32Params*>(q)};
  (void)hipLaunchKernel(fn, dim3(blocks), dim3(256), args, 0, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// Resident blocks per CU of the radiance-query kernel; 0: none for the subset.
extern "C" int rtmi_shade_f32_blocks_per_cu(unsigned subset) {
  return blocks_per_cu(subset < 64u ? subset_kernel(rtmi::K32_SHADE, subset) : nullptr, 0, 0);
}

// The float32 ray-query kernel of a geometry subset (rt_fast_query.h): its
// arguments are the FastParams, then the batch.
extern "C" int rtmi_launch_trace_f32(const rtmi::FastParams* p, const rtmi::Trace32Params* q, unsigned subset,
                                     int blocks, void* stream) {
  const void* fn = subset < 16u ? subset_kernel(rtmi::K32_TRACE, subset) : nullptr;
  if (!fn) return (int)hipErrorInvalidDeviceFunction;
  void* args[] = {const_cast<rtmi::FastParams*>(p), const_cast<rtmi::Trace32Params*>(q)};
  (void)hipLaunchKernel(fn, dim3(blocks), dim3(256), args, 0, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// Resident blocks per CU of the ray-query kernel; 0: none for the subset.
extern "C" int rtmi_trace_f32_blocks_per_cu(unsigned subset) {
  return blocks_per_cu(subset < 16u ? subset_kernel(rtmi::K32_TRACE, subset) : nullptr, 0, 0);
}

// The feature-buffer kernel of a geometry subset, with or without stochastic
// sampling (rt_fast_aov.h): its arguments are the FastParams, then the outputs.
namespace {
const void* aov_kernel(unsigned subset) {
  return (subset & ~(15u | (unsigned)rtmi::SUB_STOCHASTIC)) == 0u ? subset_kernel(rtmi::K32_AOV, subset) : nullptr;
}
}  // namespace

extern "C" int rtmi_launch_aov_f32(const rtmi::FastParams* p, const rtmi::Aov32Params* q, unsigned subset, int blocks,
                                   size_t shmem, void* stream) {
  const void* fn = aov_kernel(subset);
  if (!fn) return (int)hipErrorInvalidDeviceFunction;
  void* args[] = {const_cast<rtmi::FastParams*>(p), const_cast<rtmi::Aov32Params*>(q)};
  (void)hipLaunchKernel(fn, dim3(blocks), dim3(256), args, shmem, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// Resident blocks per CU of the feature-buffer kernel; 0: none for the subset.
extern "C" int rtmi_aov_f32_blocks_per_cu(unsigned subset, size_t shmem) {
  return blocks_per_cu(aov_kernel(subset), 0, shmem);
}

extern "C" int rtmi_launch_shade_reduce32(const float* ray_rgb, long long ngroups, int group, float inv_len,
                                          float* rgb, void* stream) {
  const unsigned blocks = (unsigned)((ngroups + 255) / 256);
  hipLaunchKernelGGL(rtmi::k_shade_reduce32, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ray_rgb, ngroups, group,
                     inv_len, rgb);
  return (int)hipGetLastError();
}

// The lean-pixel kernel of a feature subset (two-class launches).
extern "C" int rtmi_launch_lean_f32(const rtmi::FastParams* p, unsigned subset, int blocks, size_t shmem,
                                    void* stream) {
  return launch_f32(subset_kernel(rtmi::K32_LEAN, subset), hipErrorInvalidDeviceFunction, p, blocks, shmem, stream);
}

// Resident blocks per CU of the lean-pixel kernel; 0: no lean kernel for the subset.
extern "C" int rtmi_lean_f32_blocks_per_cu(unsigned subset, size_t shmem) {
  return blocks_per_cu(subset_kernel(rtmi::K32_LEAN, subset), 0, shmem);
}

// The one-plane lean-pixel kernel for nl (1 or 2) distant lights, lp (4 or
// 16) lanes per pixel: 64 / lp pixels per work item.
extern "C" int rtmi_launch_lean1_f32(const rtmi::FastParams* p, int nl, int lp, int blocks, void* stream) {
  return launch_f32(lean1_kernel(false, nl, lp), hipErrorInvalidValue, p, blocks, 0, stream);
}

// Resident blocks per CU of k_render_lean1q<nl, lp>.
extern "C" int rtmi_lean1_f32_blocks_per_cu(int nl, int lp) { return blocks_per_cu(lean1_kernel(false, nl, lp), 1, 0); }

// The one-plane batched general-pixel kernel for nl (1 or 2) distant lights.
extern "C" int rtmi_launch_gen1_f32(const rtmi::FastParams* p, int nl, int blocks, void* stream) {
  return launch_f32(gen1_kernel(nl), hipErrorInvalidValue, p, blocks, 0, stream);
}

extern "C" int rtmi_gen1_f32_blocks_per_cu(int nl) { return blocks_per_cu(gen1_kernel(nl == 1 ? 1 : 2), 1, 0); }

// The one-plane merged kernel (general items, then lean items with lp lanes per pixel).
extern "C" int rtmi_launch_mix1_f32(const rtmi::FastParams* p, int nl, int lp, int blocks, void* stream) {
  return launch_f32(lean1_kernel(true, nl, lp), hipErrorInvalidValue, p, blocks, 0, stream);
}

// Resident blocks per CU of k_render_mix1<nl, lp> (each launched
// instantiation sized from its own register use).
extern "C" int rtmi_mix1_f32_blocks_per_cu(int nl, int lp) { return blocks_per_cu(lean1_kernel(true, nl, lp), 1, 0); }

// The render kernel of a feature subset, or the instrumented one (all features).
extern "C" int rtmi_launch_render_f32(const rtmi::FastParams* p, unsigned subset, int blocks, size_t shmem,
                                      void* stream) {
  const void* fn = (p->flags & rtmi::RT_DEV_FLAG_COUNT) ? count_kernel() : subset_kernel(rtmi::K32_FAST, subset);
  return launch_f32(fn, hipErrorInvalidDeviceFunction, p, blocks, shmem, stream);
}

extern "C" int rtmi_render_f32_blocks_per_cu(int count, unsigned subset, size_t shmem) {
  return blocks_per_cu(count ? count_kernel() : subset_kernel(rtmi::K32_FAST, subset), 1, shmem);
}

extern "C" int rtmi_launch_reduce_stats(const unsigned long long* partials, int num_waves,
                                        unsigned long long* acc, void* stream) {
  const int blocks = (num_waves + rtmi::kWavesPerBlock - 1) / rtmi::kWavesPerBlock;
  hipLaunchKernelGGL(rtmi::k_reduce_stats, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, (hipStream_t)stream, partials, num_waves, acc);
  return (int)hipGetLastError();
}

extern "C" int rtmi_launch_unshard(const float* gathered, float* fb, int width, int height, int band_h,
                                   int world, void* stream) {
  const int nbands = (height + band_h - 1) / band_h;
  const int band_rows = ((nbands + world - 1) / world) * band_h;
  const int row_f = width * 3;
  if ((row_f % 4) == 0 && (((uintptr_t)gathered | (uintptr_t)fb) & 15) == 0) {
    hipLaunchKernelGGL(rtmi::k_unshard, dim3(height), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)gathered, (float4*)fb, row_f / 4, height, band_h, world, band_rows);
  } else {
    hipLaunchKernelGGL(rtmi::k_unshard_scalar, dim3(height), dim3(256), 0, (hipStream_t)stream, gathered, fb,
                       row_f, height, band_h, world, band_rows);
  }
  return (int)hipGetLastError();
}
