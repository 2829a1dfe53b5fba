// rt_aov_stage.h — where the host forms of the feature-buffer calls
// (rt_render_aovs, rt_render_aovs_f64) keep the wanted channels in the
// scene's staging buffer, and which bytes of a channel come back. Plain
// arithmetic, no device code: tools/aov_stage_check.cpp runs it under the
// address and undefined-behaviour sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rtmi {

constexpr int kAovChannels = 6;
// bytes per pixel of the channels in field order (alpha, depth, object, face,
// normal, albedo): rt_aov_buffers' and rt_aov_buffers64's
constexpr size_t kAovPxBytes32[kAovChannels] = {4, 4, 4, 4, 12, 12};
constexpr size_t kAovPxBytes64[kAovChannels] = {8, 8, 4, 4, 24, 24};

// The wanted channels' device copies, each a whole frame of npx pixels (the
// kernels index by image pixel), 256-byte aligned, in field order: off[c] is
// channel c's byte offset (unwanted channels take no room); returns the
// buffer's size.
inline size_t aov_stage_offsets(const void* const host[kAovChannels], const size_t px_bytes[kAovChannels], size_t npx,
                                size_t off[kAovChannels]) {
  size_t total = 0;
  for (int c = 0; c < kAovChannels; ++c) {
    off[c] = total;
    if (host[c]) total += (npx * px_bytes[c] + 255) & ~(size_t)255;
  }
  return total;
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
