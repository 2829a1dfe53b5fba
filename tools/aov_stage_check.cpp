// aov_stage_check.cpp — the staging arithmetic of the feature-buffer host forms
// (csrc/rt_aov_stage.h) under the address and undefined-behaviour sanitizers,
// on the CPU, with no device and no library:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Inim-raytracer_amd/csrc tools/aov_stage_check.cpp -o /tmp/aov_stage_check && /tmp/aov_stage_check
//
// For both precisions, a set of image sizes (odd ones, one pixel, a long row),
// every one of the 64 channel selections and several row ranges it plays the
// host form through: the staging buffer is allocated at exactly the size
// aov_stage_offsets returns, a "kernel" fills each wanted channel's whole
// frame at its offset, rows [y0, y1) are copied into caller arrays of exactly
// width * height elements with aov_stage_rows' offsets, and every byte is
// compared. An offset or count that is off by one element reads or writes
// outside an allocation and stops the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_aov_stage.h"

using namespace rtmi;

static unsigned char pattern(int c, size_t byte) { return (unsigned char)(17 * (c + 1) + byte * 31 + (byte >> 8)); }

static long run(const size_t px_bytes[kAovChannels], int w, int h) {
  long checked = 0;
  const size_t npx = (size_t)w * (size_t)h;
  const int ranges[][2] = {{0, h}, {0, 0}, {h, h}, {0, 1}, {h - 1, h}, {h / 3, h - h / 4}};
  for (unsigned sel = 0; sel < 64; ++sel) {
    unsigned char* host[kAovChannels];
    const void* want[kAovChannels];
    for (int c = 0; c < kAovChannels; ++c) {
      host[c] = (sel >> c & 1) ? (unsigned char*)std::malloc(npx * px_bytes[c]) : nullptr;
      want[c] = host[c];
    }
    size_t off[kAovChannels];
    const size_t total = aov_stage_offsets(want, px_bytes, npx, off);
    unsigned char* stage = (unsigned char*)std::malloc(total ? total : 1);
    for (int c = 0; c < kAovChannels; ++c) {
      if (!host[c]) continue;
      if (off[c] % 256 != 0 || off[c] + npx * px_bytes[c] > total) {
        std::printf("channel %d: offset %zu of %zu\n", c, off[c], total);
        return -1;
      }
      for (size_t b = 0; b < npx * px_bytes[c]; ++b) stage[off[c] + b] = pattern(c, b);  // the kernel's whole frame
    }
    for (const auto& r : ranges) {
      const int y0 = r[0], y1 = r[1];
      if (y0 < 0 || y1 > h || y0 > y1) continue;
      for (int c = 0; c < kAovChannels; ++c) {
        if (!host[c]) continue;
        std::memset(host[c], 0xEE, npx * px_bytes[c]);
        size_t begin, count;
        aov_stage_rows(px_bytes[c], w, y0, y1, &begin, &count);
        std::memcpy(host[c] + begin, stage + off[c] + begin, count);  // the copy back
        for (size_t b = 0; b < npx * px_bytes[c]; ++b) {
          const bool in = b >= (size_t)y0 * w * px_bytes[c] && b < (size_t)y1 * w * px_bytes[c];
          const unsigned char expect = in ? pattern(c, b) : 0xEE;
          if (host[c][b] != expect) {
            std::printf("%dx%d sel %u channel %d rows [%d, %d): byte %zu\n", w, h, sel, c, y0, y1, b);
            return -1;
          }
        }
        ++checked;
      }
    }
    std::free(stage);
    for (int c = 0; c < kAovChannels; ++c) std::free(host[c]);
  }
  return checked;
}

int main() {
  const int sizes[][2] = {{1, 1}, {33, 19}, {96, 64}, {7, 1}, {1, 9}, {1021, 3}};
  long total = 0;
  for (const auto& s : sizes)
    for (const size_t* pb : {kAovPxBytes32, kAovPxBytes64}) {
      const long n = run(pb, s[0], s[1]);
      if (n < 0) return 1;
      total += n;
    }
  std::printf("aov_stage_check: %ld channel copies checked, all inside their allocations\n", total);
  return 0;
}
