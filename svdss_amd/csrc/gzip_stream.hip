// gzip_stream.hip -- ONE deflate stream inflated in parallel on the GPU (svdss_gzip_stream_*): plain gzip, what
// `gzip reads.fastq` writes, where inflate.hip takes the independent members of BGZF.  The way of Kerbiriou and Chikhi's
// pugz and of rapidgzip: a window of compressed bytes is cut into chunks; in every chunk a block start is searched by
// trying bit offsets; every chunk is decoded from its start, references into the unknown 32 KB in front of it kept as
// 16-bit symbols; the symbols are resolved once the chunk before is known.
//
//   gz_find_kernel     for every chunk but the first: the lowest bit offset whose bits are the header of a dynamic block
//                      -- BFINAL 0, BTYPE 2, HLIT / HDIST <= 29, a complete code-length code, lengths that decode to
//                      their count, a code for symbol 256, a complete literal/length code, a distance code that is
//                      complete or has at most one code.  64 offsets per wavefront and step, segments of a chunk side by
//                      side, an atomic minimum per chunk.
//   gz_measure_kernel  one wavefront per chunk with a start: block after block (stored, fixed, dynamic) until a block end
//                      IS the start of a later chunk m, a final block, or the window's last whole block; writes only
//                      (m, end bit, bytes, flags).  A walk from a false start dies at an invalid code: no error.
//   (host)             the chain 0 -> m0 -> m1 ..., output offsets by a scan over its byte counts.  Chunks off the chain
//                      are dead: one without a start, or with a false one, only made its predecessor run longer.
//   gz_decode_kernel   one wavefront per chain chunk: the same walk storing symbols -- 0..255 a byte, 256 + j byte j of
//                      the 32 KB in front of the chunk's first byte.  The recent 4,096 symbols live in an LDS ring and
//                      leave as dwords; a match further back reads the symbols the chunk itself wrote to HBM.
//   gz_window_kernel   one workgroup, the chain in order: dictionary k + 1 = the last 32 KB of chunk k's symbols resolved
//                      through dictionary k (kept in LDS), a chunk shorter than 32 KB takes the rest from dictionary k.
//   gz_resolve_kernel  every chain chunk in four pieces side by side: its dictionary in LDS, byte = sym < 256 ? sym :
//                      dict[sym - 256], aligned dwords out, and the CRC32 of the piece (256 lanes, each its own words,
//                      a <- a x^8192 + w; the host joins the pieces with gz_crc32_combine).
// The walk of measure and decode is one symbol at a time per wavefront (the tables are built by the wave, matches are
// copied by the wave): the parallelism is across chunks.  12 KB of LDS per decoding wavefront, 4 KB per measuring one.
// Nothing here is measured yet (see DESIGN).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "crc_gf.h"
#include "dev_buf.h"
#include "gzip_stream.h"
#include "hip_check.h"
#include "inflate_tables.h"

#define UNI(x) __builtin_amdgcn_readfirstlane(x)

namespace {

constexpr int RING = 4096, RM = RING - 1;   // the LDS ring of recent output, 16-bit symbols
constexpr int FLUSHN = 1024;                // the ring is written out whenever this many symbols are waiting
// a match's source symbol is read from the ring if it lies less than NEAR before the match's output position: the copy
// overwrites nothing that close (258 + 64 < RING - NEAR); everything further back is in HBM, because fewer than
// FLUSHN + 258 < NEAR symbols ever wait to be written out
constexpr int NEAR = RING - 320;
static_assert(FLUSHN + 258 + 2 < NEAR, "ring too small");
constexpr int LB = 9, DB = 8, CB = 7;       // bits of the direct tables (literal / length, distance, code lengths)
constexpr int PARTS = 4;                    // pieces of a chain chunk in gz_resolve_kernel
constexpr int64_t COMP_SLACK = 8192;        // readable (and zero) behind a window's last byte
constexpr uint64_t TAIL_BITS = 64;          // an invalid code this close to the window's end: the window ran out, no damage

template <bool STORE>
struct GzLds {
  uint16_t ring[STORE ? RING : 2];
  uint32_t lit[1 << LB];
  uint32_t dst[1 << DB];       // (its first 256 bytes also hold the code-length code's table while a header is read)
  uint8_t lens[320];
  uint16_t lsym[288];
  uint16_t dsym[32];
  uint16_t lcnt[16], dcnt[16];
};

struct GzWalk { int32_t m, flags; int64_t end_bit, bytes; };                         // flags: 1 final block, 2 invalid code
struct GzTask { int64_t start_bit, end_bit, out_off, n; int32_t hist, pad; };        // a chain chunk
struct GzPiece { uint32_t crc, pad; int64_t len; };

// 64 bits of the window from bit position pos (dword loads: the buffer is readable COMP_SLACK bytes past its end)
__device__ __forceinline__ uint64_t peek64(const uint32_t* __restrict__ c32, uint64_t pos) {
  const uint64_t i = pos >> 5;
  const uint32_t sh = (uint32_t)pos & 31u;
  const uint32_t w0 = c32[i], w1 = c32[i + 1], w2 = c32[i + 2];
  return ((uint64_t)__builtin_amdgcn_alignbit(w2, w1, sh) << 32) | __builtin_amdgcn_alignbit(w1, w0, sh);
}
// (the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 of a header's code lengths, five bits each)
__device__ __forceinline__ uint32_t cl_order(int i) {
  return i < 12 ? (uint32_t)((0x022caa324e804a30ull >> (5 * i)) & 31) : (uint32_t)((0x3c2e1346cull >> (5 * (i - 12))) & 31);
}

// ---- find: is bit position p the header of a dynamic, non-final block?  One lane, registers only: the code-length code
// is kept as 19 x 3 bits and its per-length counts as 8 x 8 bits, the 258..316 lengths behind it are never stored -- only
// the Kraft sums of the two codes they describe, the number of distance codes and whether symbol 256 has one.
__device__ bool gz_header_ok(const uint32_t* __restrict__ c32, uint64_t p, uint64_t end) {
  const uint64_t x = peek64(c32, p);
  if ((x & 7u) != 4u) return false;                                   // BFINAL 0, BTYPE 2
  const uint32_t hlit = (uint32_t)(x >> 3) & 31u, hdist = (uint32_t)(x >> 8) & 31u, ncode = ((uint32_t)(x >> 13) & 15u) + 4u;
  if (hlit > 29u || hdist > 29u) return false;
  if (p + 17u + 3u * ncode > end) return false;
  const uint64_t y = peek64(c32, p + 17u);
  uint64_t cl = 0, cnts = 0;
  uint32_t kraft = 0;
  for (int i = 0; i < 19; ++i) {
    if ((uint32_t)i < ncode) {
      const uint32_t v = (uint32_t)(y >> (3 * i)) & 7u;
      if (v) { kraft += 128u >> v; cnts += 1ull << (8 * v); }
      cl |= (uint64_t)v << (3 * cl_order(i));
    }
  }
  if (kraft != 128u) return false;                                    // the code-length code is complete
  uint64_t pos = p + 17u + 3u * ncode;
  const uint32_t nlen = hlit + 257u, n = nlen + hdist + 1u;
  uint32_t i = 0, prev = 0, klit = 0, kdist = 0, ndc = 0;
  bool has256 = false;
  auto put = [&](uint32_t val) {
    if (i < nlen) {
      if (val) klit += 32768u >> val;
      if (i == 256u) has256 = val != 0u;
    } else if (val) { kdist += 32768u >> val; ++ndc; }
    ++i;
  };
  while (i < n) {
    if (pos > end) return false;
    uint64_t b = peek64(c32, pos);
    // canonical decoding, at most 7 bits (the code is complete: one of them ends it)
    uint32_t code = 0, first = 0, idx = 0, l = 1;
    for (; l <= 7u; ++l) {
      code |= (uint32_t)b & 1u;
      b >>= 1;
      const uint32_t cnt = (uint32_t)(cnts >> (8 * l)) & 0xffu;
      if (code < first + cnt) { idx = code - first; break; }
      first = (first + cnt) << 1;
      code <<= 1;
    }
    if (l > 7u) return false;
    pos += l;
    uint32_t s = 0;
    for (uint32_t t = 0, c = 0; t < 19u; ++t)
      if (((uint32_t)(cl >> (3 * t)) & 7u) == l) {
        if (c == idx) { s = t; break; }
        ++c;
      }
    if (s < 16u) { put(s); prev = s; }
    else {
      uint32_t rep, val = 0;
      if (s == 16u) { if (i == 0u) return false; rep = 3u + ((uint32_t)b & 3u); pos += 2; val = prev; }
      else if (s == 17u) { rep = 3u + ((uint32_t)b & 7u); pos += 3; prev = 0; }
      else { rep = 11u + ((uint32_t)b & 127u); pos += 7; prev = 0; }
      if (i + rep > n) return false;
      for (uint32_t r = 0; r < rep; ++r) put(val);
    }
    if (klit > 32768u || kdist > 32768u) return false;
  }
  if (pos > end) return false;
  return has256 && klit == 32768u && (kdist == 32768u || ndc <= 1u);
}

// grid (chunks - 1, segments of a chunk): found[k] = the lowest bit offset of chunk k that passes (atomic minimum; a
// segment stops as soon as a lower one is known)
__global__ void __launch_bounds__(64) gz_find_kernel(const uint32_t* __restrict__ c32, int64_t n_bytes, int64_t chunk_bytes, int64_t seg_bytes,
                                                    unsigned long long* found) {
  const int lane = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x + 1;
  const int64_t lo = k * chunk_bytes + (int64_t)blockIdx.y * seg_bytes;
  int64_t hi = lo + seg_bytes;
  if (hi > (k + 1) * chunk_bytes) hi = (k + 1) * chunk_bytes;
  if (hi > n_bytes) hi = n_bytes;
  if (lo >= hi) return;
  const uint64_t end = 8ull * (uint64_t)n_bytes, p_hi = 8ull * (uint64_t)hi;
  for (uint64_t p0 = 8ull * (uint64_t)lo; p0 < p_hi; p0 += 64) {
    if (__hip_atomic_load(&found[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p0) return;
    const uint64_t p = p0 + (uint64_t)lane;
    const bool ok = p < p_hi && gz_header_ok(c32, p, end);
    const unsigned long long mask = __ballot(ok);
    if (mask) {
      if (lane == 0) atomicMin(&found[k], (unsigned long long)(p0 + (uint64_t)__builtin_ctzll(mask)));
      return;
    }
  }
}

// ---- the walk of measure (STORE false: counts) and decode (STORE true: symbols to out[0 .. cap)), by one wavefront, from
// the block start `start` of chunk k.  Everything that steers it is uniform over the wave.
template <bool STORE>
__device__ __forceinline__ void gz_walk(GzLds<STORE>& L, const uint32_t* __restrict__ c32, const uint8_t* __restrict__ comp, const uint64_t end_bits,
                                        const uint64_t start, const int64_t* __restrict__ starts, const int n_chunks, const int k,
                                        const uint64_t stop, uint16_t* out, const uint64_t cap, GzWalk* res) {
  const int lane = threadIdx.x;
  // ---- input: the wave holds 64 dwords of the window, lane l the dword blk_base + l; a 64-bit buffer is refilled from them
  uint64_t bb = 0, next_dw = 0, blk_base = ~0ull;
  int bc = 0;
  uint32_t blk = 0;
  auto refill = [&]() {     // at least 33 bits afterwards
    while (bc <= 32) {
      if ((next_dw & ~63ull) != blk_base) { blk_base = next_dw & ~63ull; blk = c32[blk_base + (uint64_t)lane]; }
      const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)blk, UNI((int)(next_dw & 63ull)));
      bb |= (uint64_t)w << bc;
      bc += 32;
      ++next_dw;
    }
  };
  auto seek = [&](uint64_t P) {
    next_dw = P >> 5;
    if ((next_dw & ~63ull) != blk_base) { blk_base = next_dw & ~63ull; blk = c32[blk_base + (uint64_t)lane]; }
    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)blk, UNI((int)(next_dw & 63ull)));
    const int sh = (int)(P & 31ull);
    bb = (uint64_t)(w >> sh);
    bc = 32 - sh;
    ++next_dw;
    refill();
  };
  auto pos = [&]() -> uint64_t { return next_dw * 32ull - (uint64_t)bc; };
  auto take = [&](int n) -> uint32_t { const uint32_t v = (uint32_t)(bb & ((1ull << n) - 1ull)); bb >>= n; bc -= n; return v; };

  // ---- output (STORE): the ring holds the most recent RING symbols; [flushed, wpos) is not in HBM yet
  uint64_t wpos = 0, flushed = 0;
  auto flush = [&](bool final) {
    if (!STORE) return;
    const uint64_t upto = wpos;
    if ((((uint64_t)(uintptr_t)(out + flushed)) & 2ull) && flushed < upto) {     // a single symbol until the address is dword-aligned
      if (lane == 0) out[flushed] = L.ring[flushed & RM];
      ++flushed;
    }
    const uint64_t nd = (upto - flushed) >> 1;
    uint32_t* const o32 = (uint32_t*)(out + flushed);
    for (uint64_t i = (uint64_t)lane; i < nd; i += 64) {
      const uint32_t r = (uint32_t)((flushed + 2 * i) & RM);
      o32[i] = (uint32_t)L.ring[r] | ((uint32_t)L.ring[(r + 1) & RM] << 16);
    }
    flushed += 2 * nd;
    if (final && flushed < upto) {
      if (lane == 0) out[flushed] = L.ring[flushed & RM];
      ++flushed;
    }
  };
  // a match of ml symbols at output position o, dd back, by the whole wave: every lane reads its up to five source symbols,
  // then writes them (an overlapping match repeats its first dd symbols, so no source is one of this copy's outputs).  A
  // source in front of the chunk's first symbol is the marker 256 + j; one further back than the ring keeps is read from
  // HBM, where an earlier flush put it.
  auto copy_match = [&](uint64_t o, uint32_t ml, uint32_t dd) {
    const int64_t from = (int64_t)o - (int64_t)dd, ring_lo = (int64_t)o - NEAR;
    if (from < ring_lo && ring_lo > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (this wave's own stores of long ago)
    uint16_t v[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const uint32_t i = (uint32_t)lane + 64u * (uint32_t)t;
      v[t] = 0;
      if (i < ml) {
        const int64_t sp = from + (int64_t)(dd >= ml ? i : i % dd);
        if (sp < 0) v[t] = (uint16_t)(256 + 32768 + sp);
        else if (sp < ring_lo) v[t] = __hip_atomic_load(out + sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else v[t] = L.ring[sp & RM];
      }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const uint32_t i = (uint32_t)lane + 64u * (uint32_t)t;
      if (i < ml) L.ring[(o + i) & RM] = v[t];
    }
  };

  uint64_t n_out = 0, last_end = start, last_n = 0;
  int m = -1, j = k + 1, flags = 0;
  uint32_t lstate = 0, dstate = 0;
  seek(start);
  for (;;) {
    const uint64_t P = pos();
    if (STORE && P == stop) break;
    if (P + 3 > end_bits) break;
    refill();
    const uint32_t bfinal = take(1), btype = take(2);
    int why = 0;          // 1: the window ran out inside the block; 2: an invalid code
    if (btype == 3u) why = 2;
    else if (btype == 0u) {
      // stored: to the byte boundary, LEN / NLEN, LEN bytes straight from the input
      uint64_t p = (pos() + 7ull) & ~7ull;
      if (p + 32 > end_bits) break;
      seek(p);
      const uint32_t len = take(16);
      refill();
      const uint32_t nlen = take(16);
      if ((len ^ 0xffffu) != nlen) why = 2;
      else {
        p += 32;
        if (p + 8ull * len > end_bits) break;
        if (STORE) {
          if (wpos + len > cap) { why = 2; }
          else {
            const uint8_t* src = comp + (p >> 3);
            for (uint32_t done = 0; done < len;) {
              const uint32_t n = len - done < (uint32_t)FLUSHN ? len - done : (uint32_t)FLUSHN;
              for (uint32_t i = (uint32_t)lane; i < n; i += 64) L.ring[(wpos + i) & RM] = (uint16_t)src[done + i];
              wpos += n;
              done += n;
              if (wpos - flushed >= (uint64_t)FLUSHN) flush(false);
            }
          }
        }
        if (!why) { n_out += len; seek(p + 8ull * len); }
      }
    } else {
      int nlen, ndist;
      if (btype == 1u) {
        for (int s = lane; s < 320; s += 64) L.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
        nlen = 288; ndist = 30;
      } else {
        nlen = (int)take(5) + 257;
        ndist = (int)take(5) + 1;
        const int ncode = (int)take(4) + 4;
        if (nlen > 286 || ndist > 30) why = 2;
        if (!why) {
          if (lane < 19) L.lens[lane] = 0;
          for (int i = 0; i < ncode; ++i) {
            refill();
            const uint32_t v = take(3);
            if (lane == 0) L.lens[cl_order(i)] = (uint8_t)v;
          }
          uint16_t* const ctab = (uint16_t*)L.dst;
          if (!build_table(L.lens, 19, ctab, CB, L.dcnt, L.dsym, lane, (uint16_t)0, LenEntry())) why = 2;
          uint8_t* const tmp = (uint8_t*)L.lsym;   // (free until the tables are built)
          int i = 0, prev = 0;
          while (!why && i < nlen + ndist) {
            refill();
            const uint32_t e = (uint32_t)UNI((int)ctab[bb & ((1u << CB) - 1)]);
            const int l = (int)(e & 15u);
            if (!l) { why = 2; break; }
            take(l);
            const int s = (int)(e >> 4);
            if (s < 16) { if (lane == 0) tmp[i] = (uint8_t)s; prev = s; ++i; continue; }
            int rep, val = 0;
            if (s == 16) { if (i == 0) { why = 2; break; } rep = 3 + (int)take(2); val = prev; }
            else if (s == 17) { rep = 3 + (int)take(3); prev = 0; }
            else { rep = 11 + (int)take(7); prev = 0; }
            if (i + rep > nlen + ndist) { why = 2; break; }
            for (int t = lane; t < rep; t += 64) tmp[i + t] = (uint8_t)val;
            i += rep;
            if (pos() > end_bits) why = 1;
          }
          if (!why) {
            for (int s = lane; s < 320; s += 64) {
              const int v = s < nlen ? tmp[s] : (s >= 288 && s - 288 < ndist) ? tmp[nlen + (s - 288)] : 0;
              L.lens[s] = (uint8_t)v;
            }
            if (UNI((int)L.lens[256]) == 0) why = 2;
            nlen = 288; ndist = 30;
          }
        }
      }
      if (!why && !build_table(L.lens, nlen, L.lit, LB, L.lcnt, L.lsym, lane, LIT_NONE, LitEntry(), &lstate)) why = 2;
      if (!why && !build_table(L.lens + 288, ndist, L.dst, DB, L.dcnt, L.dsym, lane, 0u, DstEntry(), &dstate)) why = 2;
      lstate = (uint32_t)UNI((int)lstate); dstate = (uint32_t)UNI((int)dstate);
      // ---- symbols, one after the other
      while (!why) {
        refill();
        const uint32_t lo = (uint32_t)bb;
        uint32_t E = L.lit[lo & ((1u << LB) - 1)];
        if ((E & 15u) == 0u) {
          const uint32_t r = long_code(lo, LB, lstate, L.lcnt, L.lsym);
          E = r == ~0u ? LIT_NONE : LitEntry()(r & 0xffffu, r >> 16);
        }
        E = (uint32_t)UNI((int)E);
        const uint32_t kind = (E >> 4) & 3u;
        if (kind == 3u) { why = 2; break; }
        take((int)(E & 15u));
        if (kind == 0u) {
          if (STORE) {
            if (wpos >= cap) { why = 2; break; }
            if (lane == 0) L.ring[wpos & RM] = (uint16_t)((E >> 9) & 511u);
            ++wpos;
            if (wpos - flushed >= (uint64_t)FLUSHN) flush(false);
          }
          ++n_out;
          if (pos() > end_bits) why = 1;
          continue;
        }
        if (kind == 2u) break;       // the end of the block
        const uint32_t ml = ((E >> 9) & 511u) + take((int)((E >> 6) & 7u));
        refill();
        const uint32_t dbits = (uint32_t)bb;
        uint32_t D = L.dst[dbits & ((1u << DB) - 1)];
        if ((D & 15u) == 0u) {
          const uint32_t r = long_code(dbits, DB, dstate, L.dcnt, L.dsym);
          D = r == ~0u ? 0u : DstEntry()(r & 0xffffu, r >> 16);
        }
        D = (uint32_t)UNI((int)D);
        if ((D & 15u) == 0u) { why = 2; break; }
        take((int)(D & 15u));
        const uint32_t dd = (D >> 8) + take((int)((D >> 4) & 15u));
        if (pos() > end_bits) { why = 1; break; }
        if (STORE) {
          if (wpos + ml > cap) { why = 2; break; }
          copy_match(wpos, ml, dd);
          wpos += ml;
          if (wpos - flushed >= (uint64_t)FLUSHN) flush(false);
        }
        n_out += ml;
      }
    }
    if (why == 2) { if (pos() + TAIL_BITS <= end_bits) flags |= 2; break; }
    if (why == 1 || pos() > end_bits) break;
    last_end = pos();
    last_n = n_out;
    if (bfinal) { flags |= 1; break; }
    if (!STORE) {
      // is this block end the start of a later chunk?  (their starts ascend: the pointer only moves on)
      while (j < n_chunks) {
        const int64_t s = starts[j];
        if (s >= 0 && (uint64_t)s >= last_end) break;
        ++j;
      }
      if (j < n_chunks && (uint64_t)starts[j] == last_end) { m = j; break; }
    }
  }
  if (STORE) flush(true);
  if (lane == 0 && res) { res->m = m; res->flags = flags; res->end_bit = (int64_t)last_end; res->bytes = (int64_t)last_n; }
}

__global__ void __launch_bounds__(64) gz_measure_kernel(const uint32_t* __restrict__ c32, const uint8_t* __restrict__ comp, int64_t n_bytes,
                                                       const int64_t* __restrict__ starts, int n_chunks, GzWalk* res) {
  __shared__ GzLds<false> L;
  const int k = blockIdx.x;
  const int64_t s = starts[k];
  if (s < 0) {
    if (threadIdx.x == 0) { res[k].m = -1; res[k].flags = 4; res[k].end_bit = -1; res[k].bytes = 0; }
    return;
  }
  gz_walk<false>(L, c32, comp, 8ull * (uint64_t)n_bytes, (uint64_t)s, starts, n_chunks, k, 0, nullptr, 0, res + k);
}

__global__ void __launch_bounds__(64) gz_decode_kernel(const uint32_t* __restrict__ c32, const uint8_t* __restrict__ comp, int64_t n_bytes,
                                                      const GzTask* __restrict__ tasks, uint16_t* sym, GzWalk* res) {
  __shared__ GzLds<true> L;
  const GzTask t = tasks[blockIdx.x];
  gz_walk<true>(L, c32, comp, 8ull * (uint64_t)n_bytes, (uint64_t)t.start_bit, nullptr, 0, 0, (uint64_t)t.end_bit, sym + t.out_off, (uint64_t)t.n,
                res + blockIdx.x);
}

// ---- dictionaries: dicts[c] = the 32 KB of text in front of chain chunk c (byte j of it = the byte 32768 - j before the
// chunk's first one).  One workgroup; the current dictionary stays in LDS.
__global__ void __launch_bounds__(1024) gz_window_kernel(const GzTask* __restrict__ tasks, int n, const uint16_t* __restrict__ sym,
                                                        const uint8_t* __restrict__ dict0, uint8_t* dicts) {
  __shared__ uint32_t DD[2][8192];     // the current dictionary and the next one
  const int t = threadIdx.x;
  for (int i = 0; i < 8; ++i) DD[0][t + 1024 * i] = ((const uint32_t*)dict0)[t + 1024 * i];
  __syncthreads();
  for (int c = 0; c < n; ++c) {
    const uint32_t* const D32 = DD[c & 1];
    const uint8_t* const D = (const uint8_t*)D32;
    uint32_t* const dst = (uint32_t*)dicts + (size_t)c * 8192;
    for (int i = 0; i < 8; ++i) dst[t + 1024 * i] = D32[t + 1024 * i];
    if (c == n - 1) break;      // (the text behind the last chunk is the host's to carry)
    const GzTask T = tasks[c];
    const int64_t keep = T.n >= 32768 ? 0 : 32768 - T.n;      // bytes of this dictionary that stay, moved to the front
#pragma unroll 2
    for (int i = 0; i < 8; ++i) {
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t jj = 4 * (t + 1024 * i) + b;
        uint32_t x;
        if (jj < keep) x = D[jj + T.n];
        else {
          const uint32_t s = sym[T.out_off + T.n - (32768 - jj)];
          x = s < 256u ? s : (uint32_t)D[(s - 256u) & 32767u];
        }
        w |= x << (8 * b);
      }
      DD[(c + 1) & 1][t + 1024 * i] = w;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ uint32_t crc_byte(uint32_t state, uint32_t b) {
  state ^= b;
  for (int i = 0; i < 8; ++i) state = (state >> 1) ^ ((state & 1u) ? 0xEDB88320u : 0u);
  return state;
}

// grid (chain chunks, PARTS): piece q of chunk c is the text [bnd(q), bnd(q + 1)), cut at multiples of 4 bytes.  CRC32 of
// the piece: the state after words w_0 .. w_(m-1) is the sum of w_i x^(32 (m - i)), the state before them folded into w_0;
// lane t takes the words t, t + 256, ... of the sequence with zero words put IN FRONT until their number is a multiple of
// 256 (zero words in front of w_0 change nothing), a <- a x^8192 + w, and the lanes' sums meet weighted by
// x^(32 (256 - t)).  The up to 3 bytes before the first aligned word and behind the last go through one lane.
__global__ void __launch_bounds__(256) gz_resolve_kernel(const GzTask* __restrict__ tasks, const uint16_t* __restrict__ sym,
                                                        const uint8_t* __restrict__ dicts, uint8_t* text, GzPiece* pieces, int32_t* bad) {
  __shared__ uint32_t D32[8192];
  __shared__ uint32_t T[4][256];
  __shared__ uint32_t red[4];
  __shared__ uint32_t head_state;
  const uint8_t* const D = (const uint8_t*)D32;
  const int t = threadIdx.x, c = blockIdx.x, q = blockIdx.y;
  const GzTask K = tasks[c];
  auto bnd = [&](int i) -> int64_t {
    if (i <= 0) return K.out_off;
    if (i >= PARTS) return K.out_off + K.n;
    const int64_t x = (K.out_off + K.n * i / PARTS) & ~(int64_t)3;
    return x < K.out_off ? K.out_off : x;
  };
  const int64_t a = bnd(q), b = bnd(q + 1);
  GzPiece* const piece = pieces + (size_t)c * PARTS + q;
  if (a >= b) {
    if (t == 0) { piece->crc = 0; piece->pad = 0; piece->len = 0; }
    return;
  }
  const uint32_t* const src = (const uint32_t*)dicts + (size_t)c * 8192;
  for (int i = 0; i < 32; ++i) D32[t + 256 * i] = src[t + 256 * i];
  {
    const uint32_t X = gf_xpow8(1024);       // x^8192
    for (int k = 0; k < 4; ++k) T[k][t] = gf_mul((uint32_t)t << (8 * k), X);
  }
  const uint32_t weight = gf_xpow8(4u * (256u - (uint32_t)t));
  __syncthreads();
  const uint32_t lo = (uint32_t)(32768 - K.hist);      // a marker below this points in front of the member's first byte
  bool wrong = false;
  auto R = [&](uint32_t s) -> uint32_t {
    if (s < 256u) return s;
    if (s - 256u < lo || s >= 256u + 32768u) wrong = true;
    return D[(s - 256u) & 32767u];
  };
  int64_t a4 = (a + 3) & ~(int64_t)3;
  if (a4 > b) a4 = b;
  int64_t b4 = b & ~(int64_t)3;
  if (b4 < a4) b4 = a4;
  if (t == 0) {
    uint32_t st = 0xFFFFFFFFu;
    for (int64_t i = a; i < a4; ++i) { const uint32_t v = R(sym[i]); text[i] = (uint8_t)v; st = crc_byte(st, v); }
    head_state = st;
  }
  __syncthreads();
  uint32_t state = head_state;
  const int64_t nd = (b4 - a4) >> 2;
  if (nd > 0) {
    const int64_t z = (256 - (nd & 255)) & 255, rows = (nd + z) >> 8;
    uint32_t* const t32 = (uint32_t*)(text + a4);
    uint32_t acc = 0;
    for (int64_t r = 0; r < rows; ++r) {
      const int64_t idx = r * 256 + t - z;
      uint32_t w = 0;
      if (idx >= 0) {
        const uint2 s2 = *(const uint2*)(sym + a4 + 4 * idx);
        w = R(s2.x & 0xffffu) | (R(s2.x >> 16) << 8) | (R(s2.y & 0xffffu) << 16) | (R(s2.y >> 16) << 24);
        t32[idx] = w;
        if (idx == 0) w ^= state;
      }
      acc = T[0][acc & 0xff] ^ T[1][(acc >> 8) & 0xff] ^ T[2][(acc >> 16) & 0xff] ^ T[3][acc >> 24] ^ w;
    }
    uint32_t cw = gf_mul(acc, weight);
    for (int d = 32; d >= 1; d >>= 1) cw ^= (uint32_t)__shfl_xor((int)cw, d, 64);
    if ((t & 63) == 0) red[t >> 6] = cw;
    __syncthreads();
    state = red[0] ^ red[1] ^ red[2] ^ red[3];
  }
  if (t == 0) {
    for (int64_t i = b4; i < b; ++i) { const uint32_t v = R(sym[i]); text[i] = (uint8_t)v; state = crc_byte(state, v); }
    piece->crc = ~state; piece->pad = 0; piece->len = b - a;
  }
  if (wrong) atomicAdd(bad, 1);
}

}  // namespace

struct svdss_gzip_stream {
  int device = -1;
  int64_t chunk = 0;
  int64_t fake = -1;                       // SVDSS_GZIP_TEST=fake:K
  hipStream_t st = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  GzCarry carry;
  DevBuf<2, 4096> comp, found, starts, walk, tasks, sym, text, dicts, pieces, dict0, bad;
  PinBuf<2, 4096> h_text, h_small;
  std::vector<unsigned long long> h_found;
  std::vector<int64_t> h_starts;
  std::vector<GzWalk> h_walk;
  std::vector<GzTask> h_tasks;
  std::vector<GzPiece> h_pieces;
  std::vector<uint8_t> tail;
  const uint8_t* text_ptr = nullptr;
  const uint8_t* d_text_ptr = nullptr;
  int64_t text_bytes = 0;
  int64_t windows = 0, n_chunks = 0, on_chain = 0, merged = 0, false_starts = 0, members = 0, device_bytes = 0;
  int32_t ended = 0, declined = 0;
  double ms[4] = {0, 0, 0, 0};
  std::string err;
};

#define GCHK(x)                                                                \
  do {                                                                         \
    const hipError_t e_ = (x);                                                 \
    if (e_ != hipSuccess) {                                                    \
      g_svdss_hip_err = std::string(#x) + ": " + hipGetErrorString(e_);        \
      s->err = g_svdss_hip_err;                                                \
      return e_ == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP;            \
    }                                                                          \
  } while (0)
#define RCHK(x) do { const int rc_ = (x); if (rc_ != SVDSS_OK) return rc_; } while (0)

extern "C" int svdss_gzip_stream_create(int32_t device, int64_t chunk_bytes, svdss_gzip_stream_t** out) {
  if (!out) return SVDSS_EINVAL;
  *out = nullptr;
  if (chunk_bytes < 1024 || chunk_bytes > ((int64_t)1 << 30)) return SVDSS_EINVAL;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { g_svdss_hip_err = "no GPU"; return SVDSS_EHIP; }
  if (device < 0 || device >= n_dev) return SVDSS_ENODEV;
  svdss_gzip_stream* s = new (std::nothrow) svdss_gzip_stream();
  if (!s) return SVDSS_ENOMEM;
  s->device = device;
  s->chunk = chunk_bytes;
  if (const char* e = getenv("SVDSS_GZIP_TEST"))
    if (!strncmp(e, "fake:", 5)) s->fake = atoll(e + 5);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
  for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&s->ev[i]);
  if (e != hipSuccess) {
    g_svdss_hip_err = std::string("svdss_gzip_stream_create: ") + hipGetErrorString(e);
    svdss_gzip_stream_free(s);
    return SVDSS_EHIP;
  }
  *out = s;
  return SVDSS_OK;
}

// the carried text: the last 32 KB of (what was carried + text)
static void carry_text(GzCarry& c, const uint8_t* text, int64_t n) {
  if (n >= 32768) { memcpy(c.dict, text + n - 32768, 32768); c.dict_len = 32768; return; }
  if (n <= 0) return;
  memmove(c.dict, c.dict + n, (size_t)(32768 - n));
  memcpy(c.dict + 32768 - n, text, (size_t)n);
  c.dict_len = (uint32_t)std::min<int64_t>(32768, (int64_t)c.dict_len + n);
}

extern "C" int svdss_gzip_stream_run(svdss_gzip_stream_t* s, const uint8_t* comp, int64_t comp_bytes, int32_t is_last, int64_t* consumed) {
  if (!s || !consumed || comp_bytes < 0 || (comp_bytes > 0 && !comp)) return SVDSS_EINVAL;
  *consumed = 0;
  s->text_ptr = nullptr; s->d_text_ptr = nullptr; s->text_bytes = 0;
  if (s->declined || s->ended) return SVDSS_EINVAL;
  if (!s->err.empty()) return SVDSS_EIO;
  GzCarry& c = s->carry;
  int64_t p = 0;
  auto done = [&]() { *consumed = p; c.byte_pos += p; return SVDSS_OK; };
  if (c.want_trailer) {
    if (comp_bytes < 8) {
      if (is_last) { s->err = "truncated trailer"; return SVDSS_EIO; }
      return done();
    }
    const uint32_t crc = (uint32_t)comp[0] | (uint32_t)comp[1] << 8 | (uint32_t)comp[2] << 16 | (uint32_t)comp[3] << 24;
    const uint32_t isize = (uint32_t)comp[4] | (uint32_t)comp[5] << 8 | (uint32_t)comp[6] << 16 | (uint32_t)comp[7] << 24;
    if (crc != c.crc) { s->err = "CRC32 mismatch"; return SVDSS_EIO; }
    if (isize != (uint32_t)c.count) { s->err = "ISIZE mismatch"; return SVDSS_EIO; }
    c.want_trailer = 0; c.in_member = 0;
    ++s->members;
    p = 8;
  }
  if (!c.in_member) {
    if (p == comp_bytes && is_last) { s->ended = 1; return done(); }
    const int64_t h = gz_parse_header(comp + p, comp_bytes - p);
    if (h == 0 && !is_last) return done();
    if (h <= 0) { s->declined = s->members ? SVDSS_GZIP_DECLINE_TRAILING : SVDSS_GZIP_DECLINE_HEADER; return done(); }
    p += h;
    c.in_member = 1; c.bit = 0; c.dict_len = 0; c.crc = 0; c.count = 0;
  }
  // ---- the window: comp[p ..), the stream at bit c.bit of its first byte
  const uint8_t* const win = comp + p;
  const int64_t n_bytes = comp_bytes - p;
  if (n_bytes == 0 && !is_last) return done();      // (the header ended the window)
  const int64_t C = s->chunk;
  const int64_t n_chunks64 = std::max<int64_t>(1, (n_bytes + C - 1) / C);
  if (n_chunks64 > (1 << 24)) return SVDSS_ERANGE;
  const int n = (int)n_chunks64;
  GCHK(hipSetDevice(s->device));
  hipStream_t st = s->st;
  RCHK(s->comp.ensure((size_t)(n_bytes + COMP_SLACK)));
  RCHK(s->found.ensure(sizeof(unsigned long long) * (size_t)n));
  RCHK(s->starts.ensure(sizeof(int64_t) * (size_t)n));
  RCHK(s->walk.ensure(sizeof(GzWalk) * (size_t)n));
  RCHK(s->dict0.ensure(32768));
  RCHK(s->bad.ensure(16));
  if (n_bytes) GCHK(hipMemcpyAsync(s->comp.p, win, (size_t)n_bytes, hipMemcpyHostToDevice, st));
  GCHK(hipMemsetAsync((uint8_t*)s->comp.p + n_bytes, 0, (size_t)COMP_SLACK, st));
  const uint32_t* const c32 = (const uint32_t*)s->comp.p;
  s->h_starts.assign((size_t)n, -1);
  s->h_starts[0] = c.bit;
  GCHK(hipEventRecord(s->ev[0], st));
  if (n > 1) {
    GCHK(hipMemsetAsync(s->found.p, 0xff, sizeof(unsigned long long) * (size_t)n, st));
    int64_t seg = 1024;
    while ((C + seg - 1) / seg > 32768) seg *= 2;
    hipLaunchKernelGGL(gz_find_kernel, dim3((unsigned)(n - 1), (unsigned)((C + seg - 1) / seg)), dim3(64), 0, st, c32, n_bytes, C, seg,
                       (unsigned long long*)s->found.p);
    GCHK(hipGetLastError());
    s->h_found.resize((size_t)n);
    GCHK(hipMemcpyAsync(s->h_found.data(), s->found.p, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost, st));
  }
  GCHK(hipEventRecord(s->ev[1], st));
  GCHK(hipStreamSynchronize(st));
  if (n > 1) {
    bool any = false;
    for (int k = 1; k < n; ++k)
      if (s->h_found[(size_t)k] != ~0ull) { s->h_starts[(size_t)k] = (int64_t)s->h_found[(size_t)k]; any = true; }
    // nothing to do in parallel: one wavefront would walk the whole window (stored or fixed blocks only)
    if (!any) { s->declined = SVDSS_GZIP_DECLINE_NO_START; return done(); }
    if (s->fake > 0 && s->fake < n && s->h_starts[(size_t)s->fake] >= 0) ++s->h_starts[(size_t)s->fake];
  }
  GCHK(hipMemcpyAsync(s->starts.p, s->h_starts.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(gz_measure_kernel, dim3((unsigned)n), dim3(64), 0, st, c32, (const uint8_t*)s->comp.p, n_bytes, (const int64_t*)s->starts.p, n,
                     (GzWalk*)s->walk.p);
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(s->ev[2], st));
  s->h_walk.resize((size_t)n);
  GCHK(hipMemcpyAsync(s->h_walk.data(), s->walk.p, sizeof(GzWalk) * (size_t)n, hipMemcpyDeviceToHost, st));
  GCHK(hipStreamSynchronize(st));
  {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) s->ms[0] += ms;
    if (hipEventElapsedTime(&ms, s->ev[1], s->ev[2]) == hipSuccess) s->ms[1] += ms;
  }
  // ---- the chain
  std::vector<int> chain(1, 0);
  for (;;) {
    const int m = s->h_walk[(size_t)chain.back()].m;
    if (m <= chain.back() || m >= n) break;
    chain.push_back(m);
  }
  if (chain.size() > 1 && s->h_walk[(size_t)chain.back()].end_bit == s->h_starts[(size_t)chain.back()]) chain.pop_back();
  const GzWalk last = s->h_walk[(size_t)chain.back()];
  if (last.end_bit <= s->h_starts[0]) {
    s->declined = (last.flags & 2) ? SVDSS_GZIP_DECLINE_DAMAGED : SVDSS_GZIP_DECLINE_NO_ADVANCE;
    return done();
  }
  const int64_t end_bit = last.end_bit;
  s->h_tasks.resize(chain.size());
  int64_t total = 0;
  for (size_t i = 0; i < chain.size(); ++i) {
    const GzWalk& w = s->h_walk[(size_t)chain[i]];
    GzTask& t = s->h_tasks[i];
    t.start_bit = s->h_starts[(size_t)chain[i]];
    t.end_bit = w.end_bit;
    t.out_off = total;
    t.n = w.bytes;
    t.hist = (int32_t)std::min<uint64_t>(32768, c.count + (uint64_t)total);
    t.pad = 0;
    if (w.bytes < 0 || w.end_bit < t.start_bit) { s->err = "internal: bad measure result"; return SVDSS_EIO; }
    total += w.bytes;
  }
  {
    size_t ci = 0;
    int64_t cov = 0, mer = 0, fs = 0;
    for (int k = 0; k < n; ++k) {
      const int64_t sk = s->h_starts[(size_t)k];
      if ((sk >= 0 ? sk : 8 * (int64_t)k * C) >= end_bit) continue;
      ++cov;
      while (ci < chain.size() && chain[ci] < k) ++ci;
      if (ci < chain.size() && chain[ci] == k) continue;
      if (sk < 0) ++mer; else ++fs;
    }
    ++s->windows; s->n_chunks += cov; s->on_chain += (int64_t)chain.size(); s->merged += mer; s->false_starts += fs;
  }
  const int nc = (int)chain.size();
  RCHK(s->tasks.ensure(sizeof(GzTask) * (size_t)nc));
  RCHK(s->sym.ensure(sizeof(uint16_t) * (size_t)(total + 8)));
  RCHK(s->text.ensure((size_t)(total + 16)));
  RCHK(s->dicts.ensure((size_t)32768 * (size_t)nc));
  RCHK(s->pieces.ensure(sizeof(GzPiece) * (size_t)nc * PARTS));
  RCHK(s->h_text.ensure((size_t)(total + 16)));
  RCHK(s->h_small.ensure(32768));
  GCHK(hipMemcpyAsync(s->tasks.p, s->h_tasks.data(), sizeof(GzTask) * (size_t)nc, hipMemcpyHostToDevice, st));
  // (dictionary 0: the carried text at the end of 32 KB, through page-locked memory)
  memset(s->h_small.p, 0, 32768);
  memcpy((uint8_t*)s->h_small.p + 32768 - c.dict_len, c.dict_data(), c.dict_len);
  GCHK(hipMemcpyAsync(s->dict0.p, s->h_small.p, 32768, hipMemcpyHostToDevice, st));
  GCHK(hipMemsetAsync(s->bad.p, 0, 16, st));
  GCHK(hipEventRecord(s->ev[3], st));
  // (the results of the decoding walks go where those of the measuring ones were: read and compared below)
  hipLaunchKernelGGL(gz_decode_kernel, dim3((unsigned)nc), dim3(64), 0, st, c32, (const uint8_t*)s->comp.p, n_bytes, (const GzTask*)s->tasks.p,
                     (uint16_t*)s->sym.p, (GzWalk*)s->walk.p);
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(s->ev[4], st));
  hipLaunchKernelGGL(gz_window_kernel, dim3(1), dim3(1024), 0, st, (const GzTask*)s->tasks.p, nc, (const uint16_t*)s->sym.p,
                     (const uint8_t*)s->dict0.p, (uint8_t*)s->dicts.p);
  GCHK(hipGetLastError());
  hipLaunchKernelGGL(gz_resolve_kernel, dim3((unsigned)nc, PARTS), dim3(256), 0, st, (const GzTask*)s->tasks.p, (const uint16_t*)s->sym.p,
                     (const uint8_t*)s->dicts.p, (uint8_t*)s->text.p, (GzPiece*)s->pieces.p, (int32_t*)s->bad.p);
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(s->ev[5], st));
  s->h_pieces.resize((size_t)nc * PARTS);
  int32_t h_bad = 0;
  std::vector<GzWalk> dec((size_t)nc);
  GCHK(hipMemcpyAsync(s->h_pieces.data(), s->pieces.p, sizeof(GzPiece) * (size_t)nc * PARTS, hipMemcpyDeviceToHost, st));
  GCHK(hipMemcpyAsync(dec.data(), s->walk.p, sizeof(GzWalk) * (size_t)nc, hipMemcpyDeviceToHost, st));
  GCHK(hipMemcpyAsync(&h_bad, s->bad.p, sizeof h_bad, hipMemcpyDeviceToHost, st));
  if (total) GCHK(hipMemcpyAsync(s->h_text.p, s->text.p, (size_t)total, hipMemcpyDeviceToHost, st));
  GCHK(hipStreamSynchronize(st));
  {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->ev[3], s->ev[4]) == hipSuccess) s->ms[2] += ms;
    if (hipEventElapsedTime(&ms, s->ev[4], s->ev[5]) == hipSuccess) s->ms[3] += ms;
  }
  for (int i = 0; i < nc; ++i)
    if (dec[(size_t)i].end_bit != s->h_tasks[(size_t)i].end_bit || dec[(size_t)i].bytes != s->h_tasks[(size_t)i].n) {
      s->err = "internal: the decoding walk left the measured one";
      return SVDSS_EIO;
    }
  if (h_bad) { s->err = "a match reaches in front of its member's first byte"; return SVDSS_EIO; }
  for (const GzPiece& pc : s->h_pieces) c.crc = gz_crc32_combine(c.crc, pc.crc, (uint64_t)pc.len);
  c.count += (uint64_t)total;
  carry_text(c, (const uint8_t*)s->h_text.p, total);
  s->text_ptr = (const uint8_t*)s->h_text.p;
  s->d_text_ptr = (const uint8_t*)s->text.p;
  s->text_bytes = total;
  s->device_bytes += total;
  if (last.flags & 1) {
    c.bit = 0;
    c.want_trailer = 1;
    p += (end_bit + 7) >> 3;
  } else {
    c.bit = (int32_t)(end_bit & 7);
    p += end_bit >> 3;
  }
  return done();
}

extern "C" int svdss_gzip_stream_result(const svdss_gzip_stream_t* s, svdss_gzip_result_t* out) {
  if (!s || !out) return SVDSS_EINVAL;
  out->text = s->text_ptr; out->d_text = s->d_text_ptr; out->text_bytes = s->text_bytes;
  out->windows = s->windows; out->n_chunks = s->n_chunks; out->chunks_on_chain = s->on_chain; out->chunks_merged = s->merged;
  out->false_starts = s->false_starts; out->members_finished = s->members; out->device_bytes = s->device_bytes;
  out->ended = s->ended; out->declined = s->declined;
  const GzCarry& c = s->carry;
  out->byte_pos = c.byte_pos; out->bit = c.bit; out->in_member = c.in_member; out->want_trailer = c.want_trailer;
  out->crc = c.crc; out->count = c.count; out->dict = c.dict_data(); out->dict_len = (int32_t)c.dict_len;
  out->find_ms = s->ms[0]; out->measure_ms = s->ms[1]; out->decode_ms = s->ms[2]; out->resolve_ms = s->ms[3];
  return SVDSS_OK;
}

extern "C" int svdss_gzip_stream_host_tail(svdss_gzip_stream_t* s, const uint8_t* comp, int64_t comp_bytes) {
  if (!s || comp_bytes < 0 || (comp_bytes > 0 && !comp)) return SVDSS_EINVAL;
  s->tail.clear();
  s->text_ptr = nullptr; s->d_text_ptr = nullptr; s->text_bytes = 0;
  int64_t at = 0;
  GzHostTail tail(s->carry, [&](uint8_t* dst, size_t cap) {
    const size_t n = (size_t)std::min<int64_t>((int64_t)cap, comp_bytes - at);
    if (n) memcpy(dst, comp + at, n);
    at += (int64_t)n;
    return n;
  });
  std::vector<uint8_t> buf((size_t)1 << 20);
  for (;;) {
    const int64_t n = tail.next(buf.data(), buf.size());
    if (n < 0) { s->err = tail.error(); return SVDSS_EIO; }
    if (n == 0) break;
    s->tail.insert(s->tail.end(), buf.data(), buf.data() + n);
  }
  s->text_ptr = s->tail.data();
  s->text_bytes = (int64_t)s->tail.size();
  s->ended = 1;
  return SVDSS_OK;
}

extern "C" const char* svdss_gzip_stream_error(const svdss_gzip_stream_t* s) { return s ? s->err.c_str() : ""; }

extern "C" void svdss_gzip_stream_free(svdss_gzip_stream_t* s) {
  if (!s) return;
  if (s->device >= 0) (void)hipSetDevice(s->device);
  for (hipEvent_t e : s->ev)
    if (e) (void)hipEventDestroy(e);
  if (s->st) (void)hipStreamDestroy(s->st);
  delete s;
}
