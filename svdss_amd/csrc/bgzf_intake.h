// bgzf_intake.h -- how a batch of BGZF members gets into HBM, for every unit that reads them (bam_device.hip: the BAM front
// end; fastx_device.hip: `search --fastx`; ref_stream.hip: the reference): the members checked and packed on the host
// (bgzf_pack.h), uploaded, inflated (inflate.hip) and held against their footers' CRC32 (crc32_kernel, here).  Beside it
// the scaffolding those units share: the turn batches take in file order, the macros that leave an entry point through its
// run's fail(), and the hipcub call made twice.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bgzf_pack.h"
#include "crc_gf.h"
#include "dev_buf.h"
#include "hip_check.h"
#include "inflate_dev.h"

namespace {   // (every unit its own copy: no device-side linking)

__device__ __forceinline__ uint32_t ld32(const uint8_t* base, int64_t off) {
  const uint32_t* w = (const uint32_t*)(base + (off & ~(int64_t)3));
  return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(off & 3));
}

// ------------------------------------------------------------------ CRC32 of BGZF blocks (crc32_kernel, bgzf_footer_kernel)
// Tables of the CRC kernels, computed once on the host and copied to every device that asks:
//   [0]      the byte table of the CRC (state * x^8 for the state's low byte)
//   [1..4]   byte k of a state times x^2048: state * x^2048 = [1][b0] ^ [2][b1] ^ [3][b2] ^ [4][b3]
//   [5][l]   x^(32 (64 - l)), lane l's weight (entries 0..63)
__device__ uint32_t g_crc_tab[6][256];

// the tables, on the current device (once per device, unit and process)
hipError_t crc_tables_ready() {
  static std::mutex m;
  static bool done[64] = {false};
  static uint32_t h[6][256];
  static bool built = false;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(m);
  if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
  if (!built) {
    memset(h, 0, sizeof h);
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
      h[0][i] = c;
    }
    const uint32_t x2048 = gf_xpow8(256);
    for (int k = 0; k < 4; ++k)
      for (uint32_t i = 0; i < 256; ++i) h[1 + k][i] = gf_mul(i << (8 * k), x2048);
    for (uint32_t l = 0; l < 64; ++l) h[5][l] = gf_xpow8(4 * (64 - l));
    built = true;
  }
  e = hipMemcpyToSymbol(HIP_SYMBOL(g_crc_tab), h, sizeof h);
  if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
  return e;
}

// ------------------------------------------------------------------ CRC32 of the inflated blocks
// One wavefront per BGZF block.  The state of a CRC after words w_0 .. w_(m-1) is the sum of w_i x^(32 (m - i)) (the
// initial value folded into w_0): lane l takes the words l, l + 64, l + 128, ... -- every load of the wave is 256
// contiguous bytes -- with a <- a x^2048 + w (four table lookups, as many as the usual word step costs), and the lanes'
// sums meet weighted by x^(32 (64 - l)).  The bytes behind the last whole 256 (none in blocks of 0xff00 bytes, what htslib
// and bgzip write) go through the byte table on one lane.  (Until the second half of round 4 every lane walked its own
// kilobyte of the block: 64 cache lines per load instruction, 205 GB/s, 8 % of the GPU's time in `search` end to end.)
__global__ void __launch_bounds__(64) crc32_kernel(const uint8_t* __restrict__ data, const CrcBlk* __restrict__ blks, int32_t* bad) {
  __shared__ uint32_t T[5][256];
  const int lane = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) T[k][lane + 64 * i] = g_crc_tab[k][lane + 64 * i];
  const uint32_t weight = g_crc_tab[5][lane];
  __syncthreads();
  const CrcBlk b = blks[blockIdx.x];
  const int n = b.isize;
  if (n <= 0) return;
  const uint8_t* p = data + b.uoff;
  const int J = n >> 8;
  uint32_t state = 0xFFFFFFFFu;
  if (J > 0) {
    uint32_t a = 0;
    for (int j = 0; j < J; ++j) {
      // (the block's first byte is wherever the blocks before it end: the aligned-words-and-shift of ld32 on the offset
      // from the buffer's -- aligned -- start, not on a pointer that is not)
      uint32_t w = ld32(data, b.uoff + (int64_t)(j * 64 + lane) * 4);
      if (j == 0 && lane == 0) w ^= 0xFFFFFFFFu;
      a = T[1][a & 0xff] ^ T[2][(a >> 8) & 0xff] ^ T[3][(a >> 16) & 0xff] ^ T[4][a >> 24] ^ w;
    }
    uint32_t c = gf_mul(a, weight);
    for (int d = 32; d >= 1; d >>= 1) c ^= (uint32_t)__shfl_xor((int)c, d, 64);
    state = c;
  }
  if (lane == 0) {
    for (int i = J << 8; i < n; ++i) state = T[0][(state ^ p[i]) & 0xff] ^ (state >> 8);
    if (~state != b.crc) atomicAdd(bad, 1);
  }
}

// ------------------------------------------------------------------ the intake of one batch
// Part of a batch object (its buffers are reused from batch to batch).  The phases are apart so that the caller decides
// what else its stream does before the one wait: plan() on the host; enqueue() and enqueue_status_download() put work on
// the stream and do not wait; verdict() reads what came down once the caller has synchronised.  All return SVDSS_OK or a
// code with the message in the thread's error string (what RCHK passes on).
struct BgzfIntake {
  DevBuf<3, 4096> comp, blks, crcb, status;   // packed streams, block table, CRC table, n + 2 status words (the last but one: CRC mismatches)
  PinBuf<2, 4096> pin;                        // page-locked staging of the two tables
  std::vector<int32_t> h_status;
  std::vector<int64_t> chunk_off;
  BgzfPlan P;
  // the caller's arrays, as plan() was given them (read again by enqueue())
  int32_t n_chunks = 0;
  const uint8_t* const* src = nullptr;
  const int64_t* src_bytes = nullptr;
  const svdss_bgzf_block_t* const* src_blocks = nullptr;
  const uint32_t* const* src_crc = nullptr;
  const int64_t* src_n = nullptr;

  // the packed block table on the host (n + 1 entries, the last not written): as enqueue() left it
  const svdss_bgzf_block_t* h_blk() const { return (const svdss_bgzf_block_t*)pin.p; }

  int plan(int32_t n, const uint8_t* const* comp_, const int64_t* comp_bytes, const svdss_bgzf_block_t* const* blocks,
           const uint32_t* const* crc, const int64_t* n_blocks) {
    if (const char* m = bgzf_plan(n, comp_, comp_bytes, blocks, crc, n_blocks, P)) { g_svdss_hip_err = m; return SVDSS_EINVAL; }
    n_chunks = n; src = comp_; src_bytes = comp_bytes; src_blocks = blocks; src_crc = crc; src_n = n_blocks;
    return SVDSS_OK;
  }

  // the blocks inflate to dst + base + (the sizes in front), between events e0 and e1; their CRCs are taken behind
  int enqueue(hipStream_t st, hipEvent_t e0, hipEvent_t e1, uint8_t* dst, int64_t base) {
    const size_t n = (size_t)P.n_blocks;
    if (const int rc = comp.ensure((size_t)P.comp_bytes + 8192)) return rc;
    if (const int rc = blks.ensure(sizeof(svdss_bgzf_block_t) * (n + 1))) return rc;
    if (const int rc = crcb.ensure(sizeof(CrcBlk) * (n + 1))) return rc;
    if (const int rc = status.ensure(sizeof(int32_t) * (n + 2))) return rc;
    if (const int rc = pin.ensure((sizeof(svdss_bgzf_block_t) + sizeof(CrcBlk)) * (n + 1) + 4096)) return rc;
    try { chunk_off.resize((size_t)n_chunks); } catch (...) { g_svdss_hip_err = "out of memory"; return SVDSS_ENOMEM; }
    svdss_bgzf_block_t* h_blk = (svdss_bgzf_block_t*)pin.p;
    CrcBlk* h_crc = (CrcBlk*)(h_blk + (n + 1));
    bgzf_pack(n_chunks, src_bytes, src_blocks, src_crc, src_n, base, h_blk, h_crc, chunk_off.data());
    for (int32_t c = 0; c < n_chunks; ++c)
      if (src_bytes[c] > 0) HIPCHK(hipMemcpyAsync((uint8_t*)comp.p + chunk_off[(size_t)c], src[c], (size_t)src_bytes[c], hipMemcpyHostToDevice, st));
    int32_t* d_status = (int32_t*)status.p;
    HIPCHK(hipMemsetAsync(d_status, 0, sizeof(int32_t) * (n + 2), st));
    if (n == 0) return SVDSS_OK;
    HIPCHK(hipMemcpyAsync(blks.p, h_blk, sizeof(svdss_bgzf_block_t) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(crcb.p, h_crc, sizeof(CrcBlk) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e0, st));
    HIPCHK(svdss_inflate_enqueue(st, (const uint8_t*)comp.p, (const svdss_bgzf_block_t*)blks.p, P.n_blocks, dst, d_status));
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(crc_tables_ready());
    hipLaunchKernelGGL(crc32_kernel, dim3((unsigned)n), dim3(64), 0, st, (const uint8_t*)dst, (const CrcBlk*)crcb.p, d_status + n);
    HIPCHK(hipGetLastError());
    return SVDSS_OK;
  }

  int enqueue_status_download(hipStream_t st) {
    const size_t n = (size_t)P.n_blocks + 2;
    try { h_status.resize(n); } catch (...) { g_svdss_hip_err = "out of memory"; return SVDSS_ENOMEM; }
    HIPCHK(hipMemcpyAsync(h_status.data(), status.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    return SVDSS_OK;
  }

  // (the stream has been synchronised) what the kernels said, and how long the inflate kernel ran
  int verdict(hipEvent_t e0, hipEvent_t e1, double& inflate_ms) const {
    if (P.n_blocks > 0) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) inflate_ms = ms;
    }
    for (int64_t i = 0; i < P.n_blocks; ++i)
      if (h_status[(size_t)i] != 0) { g_svdss_hip_err = "BGZF inflate failed"; return SVDSS_EIO; }
    if (h_status[(size_t)P.n_blocks] != 0) { g_svdss_hip_err = "BGZF block CRC mismatch"; return SVDSS_EIO; }
    return SVDSS_OK;
  }
};

}  // namespace

// ------------------------------------------------------------------ the turn in file order
// Batches of a stream S (members m, cv, failed, err and the counter `turn` points at) take turns in file order.  The turn
// of batch `seq` is taken by wait_turn and given up by done_turn, on every path.
template <class S>
static inline bool wait_turn(S* s, int64_t S::*turn, int64_t seq) {
  std::unique_lock<std::mutex> lk(s->m);
  s->cv.wait(lk, [&] { return s->*turn == seq || s->failed; });
  return !s->failed;
}
template <class S>
static inline void done_turn(S* s, int64_t S::*turn, int fail_code, const std::string& msg) {
  {
    std::lock_guard<std::mutex> lk(s->m);
    if (fail_code && !s->failed) { s->failed = fail_code; s->err = msg; }
    ++(s->*turn);
  }
  s->cv.notify_all();
}
// a batch that fails before its turn still passes the turn on: the batches behind it wait for it (a stream that already
// failed has let everybody through)
template <class S>
static inline void pass_turn(S* s, int64_t S::*turn, int64_t seq, int code, const std::string& msg) {
  if (wait_turn(s, turn, seq)) done_turn(s, turn, code, msg);
}

// ------------------------------------------------------------------ the one way out of an entry point
// BCHK / RCHK return through fail() of the object named `run` in the calling function (BatchRun, FxRun, RsRun).
#define BCHK(expr)                                                                                    \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      g_svdss_hip_err = std::string(#expr) + ": " + hipGetErrorString(e_);                            \
      return run.fail(e_ == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP, g_svdss_hip_err);        \
    }                                                                                                 \
  } while (0)
#define RCHK(expr) do { const int rc_ = (expr); if (rc_ != SVDSS_OK) return run.fail(rc_, g_svdss_hip_err); } while (0)

// ------------------------------------------------------------------ a hipcub call, made twice
// call(nullptr, bytes, st, 0) says how much temporary storage it wants, tmp grows to that, call(tmp.p, bytes, st, k) runs
// for k = 0 .. times - 1 (calls of one size on different rows).  Returns a code, the message in the thread's error string.
template <class Buf, class F>
static inline int cub_twice(Buf& tmp, hipStream_t st, F call, int times = 1) {
  size_t tb = 0;
  HIPCHK(call(nullptr, tb, st, 0));
  if (const int rc = tmp.ensure(tb + 256)) return rc;
  for (int k = 0; k < times; ++k) {
    tb = tmp.cap;
    HIPCHK(call(tmp.p, tb, st, k));
  }
  return SVDSS_OK;
}
