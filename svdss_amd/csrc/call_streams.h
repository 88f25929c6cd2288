// call_streams.h -- the streams of the call side (POA, realignment, chain-filter ratio): one process-wide pool.
//
// The runtime multiplexes a process's streams onto a handful of hardware queues (four unless the environment says
// otherwise), and streams that share a queue run in order -- behind each other and behind the persistent search kernel
// where they share its queue.  So a call-side entry point holds ONE stream for its duration (CallStreamLease): every
// copy, launch and wait of the call goes to it, and the number of call-side streams alive is the peak number of entry
// points that ran at once (three call threads in the bench, one per device thread in `SVDSS call`), not a number per
// batch object.  A wave of several launches that should run side by side (poa_wave.hip's rounds) borrows further
// leases while it lasts.
//
// Every call ends in a synchronise of its stream, so a stream goes back idle, and batch objects and arenas may see a
// different stream from call to call.  The streams are never destroyed: the pool is reachable until the process ends,
// and by then the HIP runtime may be gone already.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "hip_check.h"

constexpr int kCallStreamDevices = 64;

struct CallStreamPool {
  std::mutex mu;
  std::vector<hipStream_t> idle[kCallStreamDevices];
  int64_t live[kCallStreamDevices] = {0};   // streams of the device, leased or idle
  int64_t created = 0;                      // since load, all devices
  int64_t merged = 0;                       // first-stage POA launches that held both variants (poa.hip)
  int64_t borrowed = 0;                     // leases taken for side-by-side launches (poa.hip)
};

// (one pool per process: an inline function's static is one object in the library; leaked on purpose, see above)
inline CallStreamPool& call_stream_pool() {
  static CallStreamPool* const pool = new CallStreamPool();
  return *pool;
}

// A stream of `device` (the current device of the calling thread) for as long as the object lives.
class CallStreamLease {
 public:
  CallStreamLease() = default;
  CallStreamLease(const CallStreamLease&) = delete;
  CallStreamLease& operator=(const CallStreamLease&) = delete;
  CallStreamLease(CallStreamLease&& o) noexcept : device_(o.device_), st_(o.st_) { o.st_ = nullptr; }
  ~CallStreamLease() { release(); }

  hipError_t acquire(int32_t device, bool borrow = false) {
    release();
    if (device < 0 || device >= kCallStreamDevices) return hipErrorInvalidDevice;
    CallStreamPool& p = call_stream_pool();
    {
      std::lock_guard<std::mutex> lock(p.mu);
      if (borrow) ++p.borrowed;
      if (!p.idle[device].empty()) {
        st_ = p.idle[device].back();
        p.idle[device].pop_back();
        device_ = device;
        return hipSuccess;
      }
    }
    hipStream_t st = nullptr;
    const hipError_t e = svdss_make_stream(&st, "SVDSS_CALL_CUS");
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(p.mu);
    ++p.live[device];
    ++p.created;
    st_ = st;
    device_ = device;
    return hipSuccess;
  }

  void release() {
    if (!st_) return;
    CallStreamPool& p = call_stream_pool();
    std::lock_guard<std::mutex> lock(p.mu);
    p.idle[device_].push_back(st_);
    st_ = nullptr;
  }

  hipStream_t get() const { return st_; }

 private:
  int32_t device_ = -1;
  hipStream_t st_ = nullptr;
};
