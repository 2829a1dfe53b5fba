// rt_hip.h — host-only: the library's error text and the owners of what it
// holds on the device. Device memory, streams and events are freed by the
// destructor of the member that holds them, never by a list. Every owner is
// move-only (std::swap between a scene and its staging state moves the
// handles), so an accidental copy does not compile.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <vector>

#include "../../include/rtmi.h"

namespace rtmi {

// Sets this thread's rt_last_error() text (printf style); returns code (rtmi.cpp).
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return ::rtmi::fail(RT_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) release(), p = o.p, n = o.n, o.p = nullptr, o.n = 0;
    return *this;
  }
  ~DevBuf() { release(); }
  int alloc(size_t count) {
    release();
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return fail(RT_E_NOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    }
    n = count;
    return RT_OK;
  }
  int upload(const std::vector<T>& h) { return upload(h.data(), h.size()); }
  int upload(const T* h, size_t count) {
    int rc = alloc(count);
    if (rc != RT_OK) return rc;
    if (count) HIP_TRY(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
  }
  void release() {  // drops the buffer early (the destructor does the same)
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  T* take() {  // hands the allocation to the caller (the extern "C" LightGridDev boundary)
    T* q = p;
    p = nullptr, n = 0;
    return q;
  }
  size_t bytes() const { return n * sizeof(T); }
};

// An owned stream or event: created into &x.h, destroyed with x; x converts
// to the raw handle wherever a HIP call takes one.
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) reset(), h = o.h, o.h = nullptr;
    return *this;
  }
  ~Owned() { reset(); }
  void reset() {
    if (h) (void)Destroy(h);
    h = nullptr;
  }
  operator H() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

template <class O>
constexpr bool kMoveOnly = !std::is_copy_constructible<O>::value && !std::is_copy_assignable<O>::value &&
                           std::is_nothrow_move_constructible<O>::value && std::is_nothrow_move_assignable<O>::value;
static_assert(kMoveOnly<DevBuf<int>> && kMoveOnly<Stream> && kMoveOnly<Event>,
              "owners cannot be copied, and move without throwing (std::swap, std::vector growth)");

inline int device_of_current() {
  int d = -1;
  (void)hipGetDevice(&d);
  return d;
}

// Makes `dev` the calling thread's device for a scope: switches only when
// another device is current, and restores only what it switched.
struct DeviceGuard {
  const int prev = device_of_current();
  const bool switched;
  explicit DeviceGuard(int dev) : switched(prev != dev) {
    if (switched) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (switched && prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace rtmi
