// dev_buf.h -- grow-only buffers that own their memory: DevBuf (hipMalloc) and PinBuf (hipHostMalloc, page-locked).
//
// A batch object keeps dozens of them and reuses them from call to call; they are freed by their destructors, so whoever
// deletes the object must have made its device current first.  ensure(n) keeps what is large enough and otherwise frees and
// asks for n + (n >> kShift) + kPad bytes: every site names its growth rule once, in the buffer's type.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>

#include "../../include/svdss_hip.h"

extern thread_local std::string g_svdss_hip_err;   // defined in index_api.hip (see hip_check.h)

struct DeviceMem {
  static hipError_t get(void** p, size_t n) { return hipMalloc(p, n); }
  static void put(void* p) { (void)hipFree(p); }
  static constexpr const char* what = "hipMalloc";
};
struct PinnedMem {
  static hipError_t get(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
  static void put(void* p) { (void)hipHostFree(p); }
  static constexpr const char* what = "hipHostMalloc";
};

// kSlack: ensure(n) is content only with n + kSlack bytes (but grows from n)
template <class Mem, unsigned kShift, size_t kPad, size_t kSlack = 0>
struct OwnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~OwnedBuf() { if (p) Mem::put(p); }
  // SVDSS_OK, or SVDSS_ENOMEM / SVDSS_EHIP with the thread's error string set (as HIPCHK leaves it)
  int ensure(size_t bytes) {
    if (bytes + kSlack <= cap && p) return SVDSS_OK;
    if (p) { Mem::put(p); p = nullptr; cap = 0; }
    const size_t want = bytes + (bytes >> kShift) + kPad;
    const hipError_t e = Mem::get(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      g_svdss_hip_err = std::string(Mem::what) + ": " + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP;
    }
    cap = want;
    return SVDSS_OK;
  }
};

template <unsigned kShift, size_t kPad>
struct DevBuf : OwnedBuf<DeviceMem, kShift, kPad> {};
template <unsigned kShift, size_t kPad, size_t kSlack = 0>
struct PinBuf : OwnedBuf<PinnedMem, kShift, kPad, kSlack> {};
