// stage_check.cpp — the staging arithmetic of every host form (csrc/rt_stage.h:
// rt_trace_rays, rt_pick_pixels, rt_shade_rays, their _f32 forms, and
// rt_render_aovs / rt_render_aovs_f64) under the address and
// undefined-behaviour sanitizers, on the CPU, with no device and no library:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Inim-raytracer_amd/csrc tools/stage_check.cpp -o /tmp/stage_check && /tmp/stage_check
//
// Queries: for n in {0, 1, 63, 64, 65, 1000}, groups {1, 4} and every optional
// input and output present and absent, the staging buffer is allocated at
// exactly the layout's total and every slot is filled with memset at its
// offset and its array's size; slots are 256-byte aligned, in field order and
// disjoint.
//
// Feature buffers: for both precisions, a set of image sizes (odd ones, one
// pixel, a long row, 7x5, 64x64), every one of the 64 channel selections and
// several row ranges (empty, one row, the whole image) it plays the host form
// through: the staging buffer is allocated at exactly the layout's total, a
// "kernel" fills each wanted channel's whole frame at its offset, rows
// [y0, y1) are copied into caller arrays of exactly width * height elements
// with aov_stage_rows' offsets, and every byte is compared.
//
// An offset or count that is off by one element reads or writes outside an
// allocation and stops the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_stage.h"

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
    const StageLayout l = aov_stage_layout(want, px_bytes, npx);
    const size_t* const off = l.off;
    const size_t total = l.total;
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

// Every slot of layout l, of bytes[k] bytes (0: absent), written inside an
// allocation of exactly l.total bytes. Returns the slots written, -1 on a
// misplaced slot.
static long fill(const char* what, const StageLayout& l, const size_t bytes[kStageSlots]) {
  unsigned char* stage = (unsigned char*)std::malloc(l.total ? l.total : 1);
  long written = 0;
  size_t end = 0;  // of the slots so far: field order, no overlap
  for (int k = 0; k < kStageSlots; ++k) {
    if (!bytes[k]) continue;
    if (l.off[k] % 256 != 0 || l.off[k] < end || l.off[k] + bytes[k] > l.total) {
      std::printf("%s: slot %d at %zu (+%zu) of %zu, previous end %zu\n", what, k, l.off[k], bytes[k], l.total, end);
      return -1;
    }
    std::memset(stage + l.off[k], 0xA0 + k, bytes[k]);
    end = l.off[k] + bytes[k];
    ++written;
  }
  if (l.total % 256 != 0 || l.total - end >= 256) {
    std::printf("%s: total %zu for slots ending at %zu\n", what, l.total, end);
    return -1;
  }
  std::free(stage);
  return written;
}

// The four query families' layouts. Returns the slots written, -1 on failure.
static long run_queries() {
  long written = 0;
  const size_t counts[] = {0, 1, 63, 64, 65, 1000};
  for (const size_t n : counts) {
    for (const size_t scalar : {sizeof(double), sizeof(float)}) {
      const size_t v3 = n * 3 * scalar;
      // traces: orig, dir, optional tnear; picks: xy; both: hits, optional normals
      for (unsigned sel = 0; sel < 8; ++sel) {
        const bool pick = sel & 1, tnear = !pick && (sel & 2), normals = sel & 4;
        const size_t bytes[kStageSlots] = {pick ? 0 : v3,          pick ? 0 : v3, tnear ? n * scalar : 0,
                                           pick ? n * 2 * scalar : 0, n * 16,        normals ? v3 : 0};
        const long w = fill(pick ? "pick" : "trace",
                            hit_stage_layout(n, scalar, !pick, !pick, tnear, pick, normals), bytes);
        if (w < 0) return -1;
        written += w;
      }
      for (const size_t group : {(size_t)1, (size_t)4}) {
        if (n % group) continue;  // (the calls refuse such a batch)
        const size_t ng = n / group;
        // rt_shade_rays: rgb and / or rgb32; rt_shade_rays_f32: its float32 rgb
        for (unsigned sel = 1; sel < 4; ++sel) {
          const bool rgb64 = scalar == sizeof(double) && (sel & 1), rgb32 = scalar == sizeof(float) || (sel & 2);
          const size_t bytes[kStageSlots] = {v3, v3, rgb64 ? ng * 24 : 0, rgb32 ? ng * 12 : 0, 0, 0};
          const long w = fill("shade", shade_stage_layout(n, group, scalar, rgb64, rgb32), bytes);
          if (w < 0) return -1;
          written += w;
        }
      }
    }
  }
  return written;
}

int main() {
  const long slots = run_queries();
  if (slots < 0) return 1;
  const int sizes[][2] = {{1, 1}, {7, 5}, {64, 64}, {33, 19}, {96, 64}, {7, 1}, {1, 9}, {1021, 3}};
  long total = 0;
  for (const auto& s : sizes)
    for (const size_t* pb : {kAovPxBytes32, kAovPxBytes64}) {
      const long n = run(pb, s[0], s[1]);
      if (n < 0) return 1;
      total += n;
    }
  std::printf("stage_check: %ld query slots and %ld channel copies checked, all inside their allocations\n", slots,
              total);
  return 0;
}
