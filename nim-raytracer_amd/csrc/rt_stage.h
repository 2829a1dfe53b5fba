// rt_stage.h — where the host forms of the query and feature-buffer calls
// (rt_trace_rays*, rt_pick_pixels*, rt_shade_rays*, rt_render_aovs*) keep
// their arrays in a scene's staging buffer, and which bytes of a feature
// channel come back. Plain arithmetic, no device code: tools/stage_check.cpp
// runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rtmi {

constexpr int kStageSlots = 6;

// Up to kStageSlots arrays in one allocation, each 256-byte aligned, in field
// order: off[k] is slot k's byte offset, total the allocation's size. A slot
// of 0 bytes (an absent array) takes no room.
struct StageLayout {
  size_t off[kStageSlots];
  size_t total;
};

inline StageLayout stage_layout(const size_t bytes[kStageSlots]) {
  StageLayout l{};
  for (int k = 0; k < kStageSlots; ++k) {
    l.off[k] = l.total;
    l.total += (bytes[k] + 255) & ~(size_t)255;
  }
  return l;
}

// Hit queries: ray origins, directions, t_near, image positions (each absent
// when its host array is: traces have no positions, picks nothing else), then
// the n hits and the wanted normals. scalar: 8 (rt_trace_rays / rt_pick_pixels,
// 16-byte rt_hit) or 4 (the _f32 calls, 16-byte rt_hit32).
inline StageLayout hit_stage_layout(size_t n, size_t scalar, bool orig, bool dir, bool tnear, bool xy, bool normals) {
  const size_t v3 = n * 3 * scalar;
  const size_t bytes[kStageSlots] = {orig ? v3 : 0,          dir ? v3 : 0, tnear ? n * scalar : 0,
                                     xy ? n * 2 * scalar : 0, n * 16,       normals ? v3 : 0};
  return stage_layout(bytes);
}

// Radiance queries: n ray origins and directions of `scalar` bytes a component,
// then the n / group colours in float64 (rt_shade_rays' rgb) and / or float32
// (its rgb32, rt_shade_rays_f32's rgb).
inline StageLayout shade_stage_layout(size_t n, size_t group, size_t scalar, bool rgb64, bool rgb32) {
  const size_t v3 = n * 3 * scalar, ng = n / group;
  const size_t bytes[kStageSlots] = {v3, v3, rgb64 ? ng * 3 * sizeof(double) : 0, rgb32 ? ng * 3 * sizeof(float) : 0,
                                     0,  0};
  return stage_layout(bytes);
}

constexpr int kAovChannels = kStageSlots;
// bytes per pixel of the channels in field order (alpha, depth, object, face,
// normal, albedo): rt_aov_buffers' and rt_aov_buffers64's
constexpr size_t kAovPxBytes32[kAovChannels] = {4, 4, 4, 4, 12, 12};
constexpr size_t kAovPxBytes64[kAovChannels] = {8, 8, 4, 4, 24, 24};

// Feature buffers: the wanted channels' device copies, each a whole frame of
// npx pixels (the kernels index by image pixel); unwanted channels take no room.
inline StageLayout aov_stage_layout(const void* const host[kAovChannels], const size_t px_bytes[kAovChannels],
                                    size_t npx) {
  size_t bytes[kStageSlots];
  for (int c = 0; c < kAovChannels; ++c) bytes[c] = host[c] ? npx * px_bytes[c] : 0;
  return stage_layout(bytes);
}

// Rows [y0, y1) of a channel of `width` pixels per row: the byte offset from
// the channel's start (the same in the staged copy and in the caller's
// array) and the byte count.
inline void aov_stage_rows(size_t px_bytes, int32_t width, int32_t y0, int32_t y1, size_t* begin, size_t* count) {
  const size_t row = (size_t)width * px_bytes;
  *begin = (size_t)y0 * row;
  *count = (size_t)(y1 - y0) * row;
}

}  // namespace rtmi
