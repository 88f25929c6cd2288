// bwt_invert.h -- the strings of the collection a BWT stands for, by MARKED LF walks (bwt_invert.hip).
//
// Row r < m (m = acc[1] sentinels) is the suffix "$_r": walking LF from it spells string r backwards until the sentinel
// in front of the string comes up (rld0_strings_of_bwt: one serial walk per string, 250 M dependent rank steps for
// the longest of GRCh38's).  Here the walks are cut at rows fixed in advance: a row i is MARKED when i < m or
// i % S == 0, every marked row is a WALKER, and a walker walks until it reaches a string's start or the next marked row
// -- about S steps.  Marks and walker ids are arithmetic:
//     rows < m are walkers 0 .. m-1;  a marked row i >= m is walker  m + i / S - ceil(m / S)
// Pass 1 (a walker per lane) records len[w] and next[w] (the walker of the row it stopped at, -1 at a string's start);
// the chaining follows next from every walker r < m -- walker r's segment is the END of string r, every next the piece
// in front of it -- which gives the string lengths and every walker's end offset in the output; pass 2 makes the same
// walk and writes symbol k of walker w at out[end_w - 1 - k].
//
// What is here compiles for host and device: the walker arithmetic, the step, the store packer, the chaining, and a host
// driver that runs the two passes with the walkers in a loop -- the route without a GPU, the fallback where HBM has no
// room, and the way the kernels' logic is tested on a machine without a GPU (tests/bwt_invert_harness.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../../include/svdss_hip.h"
#include "fmd_layout.h"

// (the fastest of 1024 / 4096 / 16384 at GRCh38's length and at an eighth of it: profiles/fmd_import.txt, fmd_import_400Mb.txt)
#define SVDSS_INVERT_STRIDE_DEFAULT 1024
// (S ln(n / S), the longest segment to expect, is 16,000 steps at S = 1024 and GRCh38's length: the limit only keeps a
// crafted file from holding a lane for n steps)
#define SVDSS_INVERT_MAX_STEPS_DEFAULT ((int64_t)1 << 24)

struct BwtInvertGeom {
  int64_t m;        // sentinels = walkers that are string ends
  int64_t S;        // stride of the marked rows
  int64_t first;    // ceil(m / S): multiples of S below it are rows < m
  int64_t W;        // walkers
  int32_t shift;    // log2 S when S is a power of two, else -1
};

inline BwtInvertGeom bwt_invert_geom(int64_t n, int64_t m, int64_t S) {
  BwtInvertGeom g;
  g.m = m;
  g.S = S < 1 ? 1 : S;
  g.first = (m + g.S - 1) / g.S;
  const int64_t all = n > 0 ? (n - 1) / g.S + 1 : 0;   // multiples of S in [0, n)
  g.W = m + (all > g.first ? all - g.first : 0);
  g.shift = (g.S & (g.S - 1)) == 0 ? __builtin_ctzll((unsigned long long)g.S) : -1;
  return g;
}

SVDSS_HD int64_t bwt_invert_row(const BwtInvertGeom& g, int64_t w) { return w < g.m ? w : (w - g.m + g.first) * g.S; }

// the walker of row i, or -1 where the row is not marked
SVDSS_HD int64_t bwt_invert_walker(const BwtInvertGeom& g, int64_t i) {
  if (i < g.m) return i;
  if (g.shift >= 0) return (i & (g.S - 1)) ? -1 : g.m + (i >> g.shift) - g.first;
  const int64_t q = i / g.S;
  return q * g.S != i ? -1 : g.m + q - g.first;
}

// pass 1 writes nothing
struct BwtInvertNoEmit {
  SVDSS_HD void put(int64_t, int) {}
  SVDSS_HD void finish() {}
};

// pass 2: the symbols of one walker, from the segment's last byte down.  Four are collected in a register and stored
// as one aligned word; the bytes of a word the segment shares with its neighbours (head and tail) are stored one by one.
struct BwtInvertPacker {
  uint8_t* at;      // the address of the byte put last (one past the segment's end before the first)
  uint32_t word;
  int32_t have;
  SVDSS_HD void start(uint8_t* end) { at = end; word = 0; have = 0; }
  SVDSS_HD void flush() {
    if (have == 4) {
      __builtin_memcpy(__builtin_assume_aligned(at, 4), &word, 4);
    } else {
      for (int j = 0; j < have; ++j) at[j] = (uint8_t)(word >> (8 * (int)(((uintptr_t)at + (uintptr_t)j) & 3)));
    }
    word = 0;
    have = 0;
  }
  SVDSS_HD void put(int64_t, int c) {
    --at;
    const int b = (int)((uintptr_t)at & 3);
    word |= (uint32_t)c << (8 * b);
    ++have;
    if (b == 0) flush();
  }
  SVDSS_HD void finish() { if (have) flush(); }
};

#define BWT_INVERT_GO 0
#define BWT_INVERT_START 1     // stopped at a string's first symbol: next = -1
#define BWT_INVERT_MARKED 2    // stopped at a marked row: next = its walker
#define BWT_INVERT_OVER 3      // the step limit

// one step of a walker at row i with len symbols behind it
template <class Emit>
SVDSS_HD int bwt_invert_step(const SvdssDevIndex& ix, const BwtInvertGeom& g, int64_t limit, int64_t& i, int64_t& len,
                             int64_t& next, Emit& emit) {
  const svdss_u4* qp = ix.blocks + 4 * (i >> SVDSS_BLOCK_SHIFT);
  const svdss_u4 q[4] = {qp[0], qp[1], qp[2], qp[3]};   // the block: BWT[i] and the rank from one 64-byte line
  const int j = (int)((i >> 5) & 3), bit = (int)(i & 31);
  const uint32_t y = j == 0 ? q[0].y : j == 1 ? q[1].y : j == 2 ? q[2].y : q[3].y;
  const uint32_t z = j == 0 ? q[0].z : j == 1 ? q[1].z : j == 2 ? q[2].z : q[3].z;
  const uint32_t w = j == 0 ? q[0].w : j == 1 ? q[1].w : j == 2 ? q[2].w : q[3].w;
  const uint32_t p0 = (y >> bit) & 1u, p1 = (z >> bit) & 1u, p2 = (w >> bit) & 1u;
  const int c = p2 ? (p0 ? 5 : 0) : (int)(1u + (p1 << 1 | p0));
  if (c == 0) { next = -1; return BWT_INVERT_START; }
  if (len >= limit) return BWT_INVERT_OVER;
  emit.put(len, c);
  ++len;
  i = svdss_acc(ix, c) + svdss_rank_in_block(ix, q, c, i);   // >= m: c >= 1
  const int64_t id = bwt_invert_walker(g, i);
  if (id >= 0) { next = id; return BWT_INVERT_MARKED; }
  return BWT_INVERT_GO;
}

// The chaining: from len / next of pass 1 the length of every string (lens[m]) and the end offset of every walker's
// segment in the output (end[W]).  SVDSS_EIO unless every walker lies on exactly one chain and the lengths sum to
// n - m: the input is then not the BWT of a string collection.
inline int bwt_invert_chain(const BwtInvertGeom& g, int64_t n, const int64_t* len, const int64_t* next, int64_t* end, int64_t* lens) {
  std::vector<uint8_t> seen((size_t)g.W, 0);
  int64_t visited = 0, total = 0;
  for (int64_t r = 0; r < g.m; ++r) {
    int64_t l = 0;
    for (int64_t w = r; w >= 0; w = next[w]) {
      if (w >= g.W || seen[(size_t)w]) return SVDSS_EIO;
      seen[(size_t)w] = 1;
      ++visited;
      if (len[w] < 0 || len[w] > n) return SVDSS_EIO;
      l += len[w];
      if (l > n) return SVDSS_EIO;
    }
    lens[r] = l;
    total += l;
    if (total > n) return SVDSS_EIO;
  }
  if (visited != g.W || total != n - g.m) return SVDSS_EIO;
  int64_t off = 0;
  for (int64_t r = 0; r < g.m; ++r) {
    off += lens[r];
    int64_t e = off;
    for (int64_t w = r; w >= 0; w = next[w]) { end[w] = e; e -= len[w]; }
  }
  return SVDSS_OK;
}

// The host driver: both passes and the chaining with the walkers in a loop.  ix: rank blocks, '$' rows and acc (text, sa
// and table null); out: n - m bytes; lens: m.  SVDSS_OK, SVDSS_EIO (not the BWT of a collection), SVDSS_ERANGE (a
// walker passed max_steps), SVDSS_ENOMEM.  pass_ms (may be null): the milliseconds of pass 1 and of pass 2.
inline int bwt_invert_host(const SvdssDevIndex& ix, int64_t stride, int64_t max_steps, int threads, uint8_t* out, int64_t* lens,
                           double* pass_ms = nullptr) {
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t m = ix.acc[1];
  if (m <= 0 || m > ix.n) return SVDSS_EIO;
  const BwtInvertGeom g = bwt_invert_geom(ix.n, m, stride);
  std::vector<int64_t> len, next, end;
  try { len.assign((size_t)g.W, 0); next.assign((size_t)g.W, -1); end.assign((size_t)g.W, 0); } catch (...) { return SVDSS_ENOMEM; }
  int over = 0;
  (void)threads;
#pragma omp parallel for num_threads(threads < 1 ? 1 : threads) schedule(dynamic, 64)
  for (int64_t w = 0; w < g.W; ++w) {
    int64_t i = bwt_invert_row(g, w), l = 0, nx = -1;
    BwtInvertNoEmit none;
    int st;
    while ((st = bwt_invert_step(ix, g, max_steps, i, l, nx, none)) == BWT_INVERT_GO) {}
    if (st == BWT_INVERT_OVER) {
#pragma omp atomic write
      over = 1;
    }
    len[(size_t)w] = l;
    next[(size_t)w] = nx;
  }
  const auto t1 = std::chrono::steady_clock::now();
  if (pass_ms) pass_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
  if (over) return SVDSS_ERANGE;
  const int rc = bwt_invert_chain(g, ix.n, len.data(), next.data(), end.data(), lens);
  if (rc != SVDSS_OK) return rc;
  // (neighbouring segments share words only through the packer's byte stores: distinct bytes, no two threads write one)
#pragma omp parallel for num_threads(threads < 1 ? 1 : threads) schedule(dynamic, 64)
  for (int64_t w = 0; w < g.W; ++w) {
    int64_t i = bwt_invert_row(g, w), l = 0, nx = -1;
    BwtInvertPacker pk;
    pk.start(out + end[(size_t)w]);
    while (bwt_invert_step(ix, g, len[(size_t)w], i, l, nx, pk) == BWT_INVERT_GO) {}
    pk.finish();
  }
  if (pass_ms) pass_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  return SVDSS_OK;
}

// bwt_invert.hip: the same on a device (rank blocks made there from the BWT bytes).  SVDSS_OK; SVDSS_EINVAL (a symbol
// above 5), SVDSS_EIO, SVDSS_ERANGE (step limit, a symbol count of 2^32 or more, *m_out > lens_cap or n - m > out_cap);
// SVDSS_ENOMEM: no room in HBM (the caller takes the host driver); SVDSS_EHIP.
struct BwtInvertStats {
  int32_t route = -1;       // 0 host driver, 1 device, 2 the serial walk per string (rld0_strings_of_bwt)
  int32_t refill = 0;
  int64_t stride = 0;
  int64_t walkers = 0;
  double blocks_ms = 0, pass1_ms = 0, pass2_ms = 0;
};
int bwt_invert_device(const uint8_t* bwt, int64_t n, int32_t device, int64_t stride, int64_t max_steps, uint8_t* out, int64_t out_cap,
                      int64_t* lens, int32_t lens_cap, int64_t* m_out, BwtInvertStats* stats);
