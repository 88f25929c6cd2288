// bwt_invert.hip -- BWT inversion by marked LF walks on the GPU (bwt_invert.h), and svdss_bwt_strings.
//
// Three small kernels make the rank blocks of fmd_layout.h from the BWT bytes where they are walked (bit planes and
// per-block counts, a scan of the tile sums, the counts and the '$' rows in place); the walk kernel runs pass 1 and
// pass 2 with a walker per lane.  Segment lengths are roughly geometric with mean S, so the lanes of a wavefront finish
// at very different steps.  Two launch shapes: a plain grid, a lane per walker, where a wavefront waits for its slowest
// lane and the dispatcher brings the next workgroup -- the default: with millions of walkers it was the faster one at
// every stride but the largest (profiles/fmd_import.txt) -- and resident wavefronts whose lanes take the next walker
// when their walk ends (one ballot and one returning atomic per wavefront and refill, as the search kernel's tickets:
// SVDSS_INVERT_REFILL=1).
#include <hip/hip_runtime.h>

#include <omp.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bwt_invert.h"
#include "fmd_layout.h"
#include "hip_check.h"
#include "index_host.h"
#include "rld0.h"

namespace {

constexpr int TILE = 256;   // rank blocks per workgroup of the block builder (a thread each)

// ---- rank blocks from BWT bytes

// K1: bit planes of block b, its counts, and the counts of the blocks of its tile in front of it.  The in-tile prefixes
// (below 2^15 each) are parked in the blocks' count words -- '$' in the high half of quarter 0's -- until K3 adds the tile's.
__global__ void __launch_bounds__(TILE) invert_planes_kernel(const uint8_t* __restrict__ bwt, int64_t n, int64_t nb, svdss_u4* __restrict__ blocks,
                                                             unsigned long long* __restrict__ tile_acgt, uint32_t* __restrict__ tile_dollar,
                                                             int* __restrict__ bad) {
  __shared__ unsigned long long sh_a[TILE];
  __shared__ uint32_t sh_d[TILE];
  const int t = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * TILE + t;
  unsigned long long acgt = 0;   // four 16-bit counts
  uint32_t nd = 0;
  svdss_u4 q[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  if (b < nb) {
    const int64_t s = b << SVDSS_BLOCK_SHIFT;
    uint32_t cnt[4] = {0, 0, 0, 0};
    int wrong = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t y = 0, z = 0, w = 0;
      const int64_t s0 = s + 32 * j;
      uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (s0 + 32 <= n) {   // (bwt is 16-byte aligned and s0 a multiple of 32)
        const uint4 lo = *reinterpret_cast<const uint4*>(bwt + s0), hi = *reinterpret_cast<const uint4*>(bwt + s0 + 16);
        words[0] = lo.x; words[1] = lo.y; words[2] = lo.z; words[3] = lo.w;
        words[4] = hi.x; words[5] = hi.y; words[6] = hi.z; words[7] = hi.w;
      } else {
        for (int k = 0; k < 32; ++k)   // the BWT's tail: rows from n on count as nothing; 0xff marks them
          words[k >> 2] |= (uint32_t)(s0 + k < n ? bwt[s0 + k] : 0xffu) << (8 * (k & 3));
      }
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const uint32_t sym = (words[k >> 2] >> (8 * (k & 3))) & 0xffu;
        if (sym == 0xffu && s0 + k >= n) continue;
        if (sym > 5u) { wrong = 1; continue; }
        if (sym >= 1u && sym <= 4u) {
          const uint32_t code = sym - 1u;
          y |= (code & 1u) << k;
          z |= (code >> 1) << k;
          cnt[0] += code == 0u; cnt[1] += code == 1u; cnt[2] += code == 2u; cnt[3] += code == 3u;
        } else {
          w |= 1u << k;
          if (sym == 5u) y |= 1u << k; else ++nd;
        }
      }
      q[j].y = y; q[j].z = z; q[j].w = w;
    }
    if (wrong) atomicOr(bad, 1);
    acgt = (unsigned long long)cnt[0] | (unsigned long long)cnt[1] << 16 | (unsigned long long)cnt[2] << 32 | (unsigned long long)cnt[3] << 48;
  }
  // inclusive scan over the tile (a count is at most 128 * 256 = 2^15: the 16-bit fields never carry)
  sh_a[t] = acgt;
  sh_d[t] = nd;
  __syncthreads();
  for (int d = 1; d < TILE; d <<= 1) {
    const unsigned long long a = t >= d ? sh_a[t - d] : 0ull;
    const uint32_t e = t >= d ? sh_d[t - d] : 0u;
    __syncthreads();
    sh_a[t] += a;
    sh_d[t] += e;
    __syncthreads();
  }
  if (b < nb) {
    const unsigned long long ex = sh_a[t] - acgt;
    const uint32_t exd = sh_d[t] - nd;
    q[0].x = (uint32_t)(ex & 0xffffu) | exd << 16;
    q[1].x = (uint32_t)((ex >> 16) & 0xffffu);
    q[2].x = (uint32_t)((ex >> 32) & 0xffffu);
    q[3].x = (uint32_t)((ex >> 48) & 0xffffu);
#pragma unroll
    for (int j = 0; j < 4; ++j) blocks[4 * b + j] = q[j];
  }
  if (t == TILE - 1) {
    // (a whole tile of one symbol sums to 2^15 in its field: still 16 bits)
    tile_acgt[blockIdx.x] = sh_a[t];
    tile_dollar[blockIdx.x] = sh_d[t];
  }
}

// K2 (one workgroup): exclusive scan of the tile sums -- prefix[5 * tile + c] for A, C, G, T, '$' -- and the totals
__global__ void __launch_bounds__(256) invert_scan_kernel(const unsigned long long* __restrict__ tile_acgt, const uint32_t* __restrict__ tile_dollar,
                                                          int64_t n_tiles, unsigned long long* __restrict__ prefix, unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long sh[5][256];
  const int t = threadIdx.x;
  const int64_t per = (n_tiles + 255) / 256;
  const int64_t lo = std::min<int64_t>(n_tiles, t * per), hi = std::min<int64_t>(n_tiles, lo + per);
  unsigned long long s[5] = {0, 0, 0, 0, 0};
  for (int64_t k = lo; k < hi; ++k) {
    const unsigned long long a = tile_acgt[k];
    s[0] += a & 0xffffu; s[1] += (a >> 16) & 0xffffu; s[2] += (a >> 32) & 0xffffu; s[3] += a >> 48;
    s[4] += tile_dollar[k];
  }
  for (int c = 0; c < 5; ++c) sh[c][t] = s[c];
  __syncthreads();
  if (t == 0)
    for (int c = 0; c < 5; ++c) {
      unsigned long long run = 0;
      for (int k = 0; k < 256; ++k) { const unsigned long long v = sh[c][k]; sh[c][k] = run; run += v; }
      totals[c] = run;
    }
  __syncthreads();
  for (int c = 0; c < 5; ++c) s[c] = sh[c][t];
  for (int64_t k = lo; k < hi; ++k) {
    for (int c = 0; c < 5; ++c) prefix[5 * k + c] = s[c];
    const unsigned long long a = tile_acgt[k];
    s[0] += a & 0xffffu; s[1] += (a >> 16) & 0xffffu; s[2] += (a >> 32) & 0xffffu; s[3] += a >> 48;
    s[4] += tile_dollar[k];
  }
}

// K3: the counts of every block (tile prefix + in-tile prefix; all below 2^32, the host has looked at the totals) and
// the sorted '$' rows
__global__ void __launch_bounds__(TILE) invert_counts_kernel(svdss_u4* __restrict__ blocks, int64_t nb, const unsigned long long* __restrict__ prefix,
                                                             int64_t* __restrict__ dollar, int64_t m) {
  const int64_t b = (int64_t)blockIdx.x * TILE + threadIdx.x;
  if (b >= nb) return;
  const unsigned long long* tp = prefix + 5 * (int64_t)blockIdx.x;
  svdss_u4 q[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = blocks[4 * b + j];
  int64_t at = (int64_t)tp[4] + (int64_t)(q[0].x >> 16);
  q[0].x &= 0xffffu;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    blocks[4 * b + j].x = (uint32_t)(tp[j] + q[j].x);
    uint32_t d = q[j].w & ~q[j].y;
    while (d) {
      const int bit = __builtin_ctz(d);
      d &= d - 1;
      if (at < m) dollar[at] = (b << SVDSS_BLOCK_SHIFT) + 32 * j + bit;
      ++at;
    }
  }
}

// ---- the walks

struct InvertArgs {
  BwtInvertGeom g;
  int64_t max_steps;
  int64_t* len;
  int64_t* next;
  const int64_t* end;
  uint8_t* out;
  unsigned long long* ticket;   // the next walker nobody has taken
  int* over;
  int32_t refill;
};

template <int PASS, class Emit>
__device__ __forceinline__ void invert_begin(const InvertArgs& a, int64_t w, int64_t& i, int64_t& len, int64_t& limit, Emit& emit) {
  i = bwt_invert_row(a.g, w);
  len = 0;
  if constexpr (PASS == 2) {
    limit = a.len[w];
    emit.start(a.out + a.end[w]);
  } else {
    limit = a.max_steps;
  }
}

template <int PASS>
__global__ void __launch_bounds__(256) invert_walk_kernel(SvdssDevIndex ix, InvertArgs a) {
  using Emit = typename std::conditional<PASS == 2, BwtInvertPacker, BwtInvertNoEmit>::type;
  const int lane = threadIdx.x & 63;
  Emit emit;
  int64_t w = -1, i = 0, len = 0, limit = 0;
  bool active = false;
  bool dry = !a.refill;   // wave-uniform: nothing left to take
  if (!a.refill) {        // the plain grid: a walker per lane, the wavefront waits for its slowest
    w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < a.g.W) { invert_begin<PASS>(a, w, i, len, limit, emit); active = true; }
  }
  for (;;) {
    if (!dry) {
      const unsigned long long wm = __ballot(!active);
      if (wm) {
        const int c = __builtin_popcountll(wm);
        const int rank = __builtin_popcountll(wm & ((1ULL << lane) - 1ULL));
        const int leader = (int)__builtin_ctzll(wm);
        unsigned long long nb = 0;
        if (lane == leader) nb = atomicAdd(a.ticket, (unsigned long long)c);
        nb = (unsigned long long)__shfl((long long)nb, leader, 64);
        if (!active) {
          w = (int64_t)nb + rank;
          if (w < a.g.W) { invert_begin<PASS>(a, w, i, len, limit, emit); active = true; }
        }
        if ((int64_t)nb + c >= a.g.W) dry = true;
      }
    }
    if (!__ballot(active)) break;
    if (active) {
      int64_t next = -1;
      const int st = bwt_invert_step(ix, a.g, limit, i, len, next, emit);
      if (st != BWT_INVERT_GO) {
        if constexpr (PASS == 1) {
          a.len[w] = len;
          a.next[w] = next;
          if (st == BWT_INVERT_OVER) atomicOr(a.over, 1);
        } else {
          emit.finish();
        }
        active = false;
      }
    }
  }
}

struct DevPtr {
  void* p = nullptr;
  ~DevPtr() { if (p) (void)hipFree(p); }
  int get(size_t bytes) {
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      g_svdss_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP;
    }
    return SVDSS_OK;
  }
};
struct Events {
  hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

thread_local BwtInvertStats g_last;

}  // namespace

#define INV_TRY(expr) do { const int rc_ = (expr); if (rc_ != SVDSS_OK) return rc_; } while (0)

int bwt_invert_device(const uint8_t* bwt, int64_t n, int32_t device, int64_t stride, int64_t max_steps, uint8_t* out, int64_t out_cap,
                      int64_t* lens, int32_t lens_cap, int64_t* m_out, BwtInvertStats* stats) {
  HIPCHK(hipSetDevice(device));
  const int64_t nb = (n >> SVDSS_BLOCK_SHIFT) + 1, n_tiles = (nb + TILE - 1) / TILE;
  if (n_tiles >= ((int64_t)1 << 31)) return SVDSS_ERANGE;
  const int64_t S = stride < 1 ? 1 : stride;
  {
    // BWT bytes + rank blocks + output + the walkers' arrays (the '$' rows and the sentinel walkers come on top once m is known)
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double need = (double)n + (double)nb * SVDSS_BLOCK_BYTES + (double)n + 24.0 * (double)(n / S + 1) + 45.0 * (double)n_tiles + (double)(64 << 20);
    if ((double)free_b < need) return SVDSS_ENOMEM;
  }
  DevPtr d_bwt, d_blocks, d_tacgt, d_tdollar, d_prefix, d_small, d_dollar, d_len, d_next, d_end, d_out;
  INV_TRY(d_bwt.get((size_t)n + 64));
  INV_TRY(d_blocks.get((size_t)nb * SVDSS_BLOCK_BYTES));
  INV_TRY(d_tacgt.get((size_t)n_tiles * 8));
  INV_TRY(d_tdollar.get((size_t)n_tiles * 4));
  INV_TRY(d_prefix.get((size_t)n_tiles * 40));
  INV_TRY(d_small.get(64));   // totals[5] | ticket | bad, over
  Events ev;
  for (hipEvent_t& x : ev.e) HIPCHK(hipEventCreate(&x));
  unsigned long long* d_totals = (unsigned long long*)d_small.p;
  unsigned long long* d_ticket = d_totals + 5;
  int* d_bad = (int*)(d_totals + 6);
  int* d_over = d_bad + 1;
  HIPCHK(hipMemset(d_small.p, 0, 64));
  HIPCHK(hipMemcpy(d_bwt.p, bwt, (size_t)n, hipMemcpyHostToDevice));
  HIPCHK(hipEventRecord(ev.e[0], 0));
  hipLaunchKernelGGL(invert_planes_kernel, dim3((unsigned)n_tiles), dim3(TILE), 0, 0, (const uint8_t*)d_bwt.p, n, nb, (svdss_u4*)d_blocks.p,
                     (unsigned long long*)d_tacgt.p, (uint32_t*)d_tdollar.p, d_bad);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(invert_scan_kernel, dim3(1), dim3(256), 0, 0, (const unsigned long long*)d_tacgt.p, (const uint32_t*)d_tdollar.p, n_tiles,
                     (unsigned long long*)d_prefix.p, d_totals);
  HIPCHK(hipGetLastError());
  unsigned long long small[8];
  HIPCHK(hipMemcpy(small, d_small.p, sizeof small, hipMemcpyDeviceToHost));
  int flags[2];
  memcpy(flags, &small[6], sizeof flags);
  if (flags[0]) return SVDSS_EINVAL;   // a symbol above 5
  SvdssDevIndex ix;
  memset(&ix, 0, sizeof ix);
  int64_t acgt = 0;
  for (int c = 0; c < 4; ++c) {
    if (small[c] > 0xffffffffULL) return SVDSS_ERANGE;
    acgt += (int64_t)small[c];
  }
  const int64_t m = (int64_t)small[4];
  if (m > 0xffffffffLL || m >= ((int64_t)1 << 31)) return SVDSS_ERANGE;
  *m_out = m;
  if (m <= 0 || m > n) return SVDSS_EIO;
  if (m > lens_cap || n - m > out_cap) return SVDSS_ERANGE;
  ix.acc[0] = 0;
  ix.acc[1] = m;
  for (int c = 1; c <= 4; ++c) ix.acc[c + 1] = ix.acc[c] + (int64_t)small[c - 1];
  ix.acc[6] = n;   // the rest is N
  (void)acgt;
  INV_TRY(d_dollar.get((size_t)(m + 1) * 8));
  hipLaunchKernelGGL(invert_counts_kernel, dim3((unsigned)n_tiles), dim3(TILE), 0, 0, (svdss_u4*)d_blocks.p, nb, (const unsigned long long*)d_prefix.p,
                     (int64_t*)d_dollar.p, m);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e[1], 0));
  ix.blocks = (const svdss_u4*)d_blocks.p;
  ix.dollar = (const int64_t*)d_dollar.p;
  ix.n = n;
  ix.n_dollar = (int32_t)m;

  InvertArgs a;
  a.g = bwt_invert_geom(n, m, S);
  a.max_steps = max_steps;
  const int64_t W = a.g.W;
  INV_TRY(d_len.get((size_t)W * 8));
  INV_TRY(d_next.get((size_t)W * 8));
  INV_TRY(d_end.get((size_t)W * 8));
  INV_TRY(d_out.get((size_t)(n - m) + 64));
  a.len = (int64_t*)d_len.p;
  a.next = (int64_t*)d_next.p;
  a.end = (const int64_t*)d_end.p;
  a.out = (uint8_t*)d_out.p;
  a.ticket = d_ticket;
  a.over = d_over;
  a.refill = getenv("SVDSS_INVERT_REFILL") && atoi(getenv("SVDSS_INVERT_REFILL")) != 0;
  // refill: resident wavefronts that take walkers until none is left; plain: a lane per walker
  int n_cu = 256;
  { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount; }
  const int64_t lanes_blocks = (W + 255) / 256;
  if (lanes_blocks >= ((int64_t)1 << 31)) return SVDSS_ERANGE;
  const unsigned grid = (unsigned)(a.refill ? std::min<int64_t>(lanes_blocks, (int64_t)n_cu * 8) : lanes_blocks);
  hipLaunchKernelGGL(invert_walk_kernel<1>, dim3(grid), dim3(256), 0, 0, ix, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e[2], 0));
  std::vector<int64_t> len, next, end;
  try { len.resize((size_t)W); next.resize((size_t)W); end.resize((size_t)W); } catch (...) { return SVDSS_ENOMEM; }
  HIPCHK(hipMemcpy(len.data(), d_len.p, (size_t)W * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(next.data(), d_next.p, (size_t)W * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(flags, d_bad, sizeof flags, hipMemcpyDeviceToHost));
  if (flags[1]) return SVDSS_ERANGE;   // a walker passed the step limit
  INV_TRY(bwt_invert_chain(a.g, n, len.data(), next.data(), end.data(), lens));
  HIPCHK(hipMemcpy(d_end.p, end.data(), (size_t)W * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(d_ticket, 0, 8));
  HIPCHK(hipEventRecord(ev.e[3], 0));
  hipLaunchKernelGGL(invert_walk_kernel<2>, dim3(grid), dim3(256), 0, 0, ix, a);
  HIPCHK(hipGetLastError());
  float ms_blocks = 0, ms1 = 0, ms2 = 0;
  HIPCHK(hipEventRecord(ev.e[4], 0));
  HIPCHK(hipEventSynchronize(ev.e[4]));
  HIPCHK(hipEventElapsedTime(&ms_blocks, ev.e[0], ev.e[1]));
  HIPCHK(hipEventElapsedTime(&ms1, ev.e[1], ev.e[2]));
  HIPCHK(hipEventElapsedTime(&ms2, ev.e[3], ev.e[4]));
  HIPCHK(hipMemcpy(out, d_out.p, (size_t)(n - m), hipMemcpyDeviceToHost));
  if (stats) {
    stats->route = 1; stats->refill = a.refill; stats->stride = S; stats->walkers = W;
    stats->blocks_ms = ms_blocks; stats->pass1_ms = ms1; stats->pass2_ms = ms2;
  }
  return SVDSS_OK;
}

// the serial walk per string (rld0.cpp), flattened: what the callers take when a walker passed the step limit
static int strings_by_serial_walks(const uint8_t* bwt, int64_t n, int threads, uint8_t* out, int64_t out_cap, int64_t* lens, int32_t lens_cap, int64_t m) {
  if (m > lens_cap || n - m > out_cap) return SVDSS_ERANGE;
  std::vector<std::vector<uint8_t>> strings;
  INV_TRY(rld0_strings_of_bwt(bwt, n, threads, strings));
  int64_t total = 0;
  for (const auto& s : strings) total += (int64_t)s.size();
  if ((int64_t)strings.size() != m || total != n - m) return SVDSS_EIO;
  int64_t at = 0;
  for (size_t r = 0; r < strings.size(); ++r) {
    lens[r] = (int64_t)strings[r].size();
    if (!strings[r].empty()) memcpy(out + at, strings[r].data(), strings[r].size());
    at += lens[r];
  }
  return SVDSS_OK;
}

extern "C" int svdss_bwt_strings(const uint8_t* bwt, int64_t n, int32_t device, int64_t stride, uint8_t* out, int64_t out_cap,
                                 int64_t* lens, int32_t lens_cap, int32_t* n_strings) {
  if (!bwt || n <= 0 || !out || !lens || !n_strings || out_cap < 0 || lens_cap < 0) return SVDSS_EINVAL;
  g_last = BwtInvertStats();
  int threads = 1;
#ifdef _OPENMP
  threads = omp_get_max_threads();
#endif
  int64_t S = stride;
  if (S == 0 && getenv("SVDSS_INVERT_STRIDE")) S = atoll(getenv("SVDSS_INVERT_STRIDE"));
  if (S == 0) S = SVDSS_INVERT_STRIDE_DEFAULT;
  int64_t max_steps = getenv("SVDSS_INVERT_MAX_STEPS") ? atoll(getenv("SVDSS_INVERT_MAX_STEPS")) : 0;
  if (max_steps <= 0) max_steps = SVDSS_INVERT_MAX_STEPS_DEFAULT;
  int64_t m = 0;
  if (device >= 0 && S > 0) {
    const int rc = bwt_invert_device(bwt, n, device, S, max_steps, out, out_cap, lens, lens_cap, &m, &g_last);
    if (m > 0 && m < ((int64_t)1 << 31)) *n_strings = (int32_t)m;
    if (rc != SVDSS_ENOMEM) return rc;   // (no room in HBM: the same walk on the host)
  }
  // the host: symbols looked at and counted first
  {
    const int rc = rld0_count_sentinels(bwt, n, threads, &m);
    if (rc != SVDSS_OK) return rc;
  }
  if (m >= ((int64_t)1 << 31)) return SVDSS_ERANGE;
  *n_strings = (int32_t)m;
  if (m <= 0) return SVDSS_EIO;
  if (m > lens_cap || n - m > out_cap) return SVDSS_ERANGE;
  if (S < 0) {
    const auto t0 = std::chrono::steady_clock::now();
    g_last.route = 2;
    const int rc = strings_by_serial_walks(bwt, n, threads, out, out_cap, lens, lens_cap, m);
    g_last.pass1_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
  }
  g_last.route = 0;
  g_last.stride = S;
  g_last.walkers = bwt_invert_geom(n, m, S).W;
  double ms[3] = {0, 0, 0};
  const int rc = rld0_strings_marked(bwt, n, S, max_steps, threads, out, lens, ms);
  g_last.blocks_ms = ms[0]; g_last.pass1_ms = ms[1]; g_last.pass2_ms = ms[2];
  return rc;
}

extern "C" int svdss_bwt_strings_last(int32_t* route, int64_t* stride, int64_t* walkers, double* ms) {
  if (!route || !stride || !walkers || !ms) return SVDSS_EINVAL;
  *route = g_last.route;
  *stride = g_last.stride;
  *walkers = g_last.walkers;
  ms[0] = g_last.blocks_ms; ms[1] = g_last.pass1_ms; ms[2] = g_last.pass2_ms;
  return g_last.route < 0 ? SVDSS_ENODEV : SVDSS_OK;
}
