// rld0_plan.h -- where the blocks of an rld0 (`.fmd`) data stream begin, as a rule instead of as the trace of a serial
// encoder: what rld0_write (rld0.cpp) does run by run, restated so that the device encoder (rld0_dev.hip), the host and
// the tests share one set of functions.
//
//   runs     the maximal runs of the BWT; run r has length l = start[r + 1] - start[r] and symbol sym[r]
//   code     Elias delta of l, then the symbol in 3 bits: w(l) = 2 ilog2(ilog2(l) + 1) + 1 + ilog2(l) + 3 bits
//   blocks   8 words each.  Block b begins with hdr(type) words (2 for type 0, 4 for type 1) that hold the symbol counts of
//            block b - 1; it is one word short when (b + 1) * 8 is a multiple of the piece length (2^23 words); it takes
//            the longest prefix of the remaining runs whose widths sum to at most cap = 64 (8 - hdr - short) bits
//   types    the block after one with fewer than 0x4000 symbols has type 0, below 2^30 type 1, else type 2 (the host's)
//   ends     block 0 has type 0 and a zero header; after the last run comes one closing header
//
// So the only sequential dependency is the chain of block starts; a state is (first run, header type), and the block
// number matters at piece ends alone.  P is the exclusive prefix sum of the widths (P[0] = 0, R + 1 entries), start has
// R + 1 entries (start[R] = n).
#pragma once
#include <stdint.h>

#include "fmd_layout.h"

#define RLD0_BLOCK_WORDS 8
#define RLD0_PIECE_WORDS ((int64_t)1 << 23)
#define RLD0_MAX_BLOCK_RUNS 96          // 384 bits / 4 bits: the most runs a block holds
#define RLD0_TYPE1_SYMS ((int64_t)0x4000)
#define RLD0_TYPE2_SYMS ((int64_t)1 << 30)
#define RLD0_RUN_MASK (((int64_t)1 << 48) - 1)   // a block descriptor: first run | type << 62

SVDSS_HD int rld0_ilog2(uint64_t v) { return 63 - __builtin_clzll(v); }

// bits of the code of a run of l >= 1 symbols
SVDSS_HD int rld0_code_width(int64_t l) {
  const int y = rld0_ilog2((uint64_t)l);
  return 2 * rld0_ilog2((uint64_t)y + 1) + 1 + y + 3;
}

// the code itself (delta of l, then the symbol), right-aligned; *w its width
SVDSS_HD uint64_t rld0_code(int64_t l, int c, int* w) {
  const int y = rld0_ilog2((uint64_t)l);
  const int z = rld0_ilog2((uint64_t)y + 1);
  *w = 2 * z + 1 + y + 3;
  return ((((uint64_t)l ^ ((uint64_t)1 << y)) | ((uint64_t)(y + 1) << y)) << 3) | (uint64_t)c;
}

SVDSS_HD int rld0_hdr_words(int type) { return type == 0 ? 2 : type == 1 ? 4 : 7; }

// is block b the last of a piece (one word short)?  piece_words: a multiple of 8
SVDSS_HD bool rld0_block_short(int64_t b, int64_t piece_words) { return ((b + 1) * RLD0_BLOCK_WORDS) % piece_words == 0; }

SVDSS_HD int rld0_block_cap(int type, bool is_short) { return 64 * (RLD0_BLOCK_WORDS - rld0_hdr_words(type) - (is_short ? 1 : 0)); }

// header type of the block that follows one with `syms` symbols
SVDSS_HD int rld0_next_type(int64_t syms) { return syms < RLD0_TYPE1_SYMS ? 0 : syms < RLD0_TYPE2_SYMS ? 1 : 2; }

// does a block with `syms` symbols make the device decline the call?  (threshold: SVDSS_FMD_DECLINE_SYMS, at most 2^30)
SVDSS_HD bool rld0_declines(int64_t syms, int64_t threshold) { return syms >= threshold; }

// one past the last run of the block that starts at run r with `cap` bits of room: the largest e <= R with
// P[e] - P[r] <= cap (e > r: no code is wider than the smallest capacity)
SVDSS_HD int64_t rld0_block_end(const int64_t* P, int64_t R, int64_t r, int cap) {
  int64_t lo = r, hi = r + RLD0_MAX_BLOCK_RUNS < R ? r + RLD0_MAX_BLOCK_RUNS : R;   // P[lo] fits, answer in [lo, hi]
  const int64_t lim = P[r] + cap;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (P[mid] <= lim) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One step of the chain: the block that starts at run r with header `type`, block number b -> r, type of the next one.
// Returns the block's symbols.
SVDSS_HD int64_t rld0_step(const int64_t* start, const int64_t* P, int64_t R, int64_t piece_words, int64_t b, int64_t* r, int* type) {
  const int64_t e = rld0_block_end(P, R, *r, rld0_block_cap(*type, rld0_block_short(b, piece_words)));
  const int64_t syms = start[e] - start[*r];
  *r = e;
  *type = rld0_next_type(syms);
  return syms;
}

// number of the first short block at or after b
SVDSS_HD int64_t rld0_next_short(int64_t b, int64_t piece_words) {
  const int64_t pb = piece_words / RLD0_BLOCK_WORDS;
  return (b / pb) * pb + pb - 1;
}

// The blocks that start in [r, stop) from the state (r, type), none of them short: the state past `stop` and how many.
SVDSS_HD int32_t rld0_walk_plain(const int64_t* start, const int64_t* P, int64_t R, int64_t stop, int64_t* r, int* type) {
  int32_t blocks = 0;
  while (*r < stop) {
    const int64_t e = rld0_block_end(P, R, *r, rld0_block_cap(*type, false));
    *type = rld0_next_type(start[e] - start[*r]);
    if (*type > 1) *type = 1;   // (type 2 is the host's: such a plan is declined, the walk only has to end)
    *r = e;
    ++blocks;
  }
  return blocks;
}

// The 8 words of block (r0, r1, type): the header from the runs [rp, r0) of the block before it (rp == r0: zeros), then
// the codes of [r0, r1).  The closing header is the block with r0 == r1 == R (its first rld0_hdr_words(type) words count).
// type 0 or 1 only.
SVDSS_HD void rld0_emit_block(const int64_t* start, const uint8_t* sym, int64_t rp, int64_t r0, int64_t r1, int type, uint64_t* out) {
  uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
  for (int64_t r = rp; r < r0; ++r) {
    const uint64_t l = (uint64_t)(start[r + 1] - start[r]);
    const int s = sym[r];
    c0 += s == 0 ? l : 0; c1 += s == 1 ? l : 0; c2 += s == 2 ? l : 0;
    c3 += s == 3 ? l : 0; c4 += s == 4 ? l : 0; c5 += s == 5 ? l : 0;
  }
  const uint64_t all = c0 + c1 + c2 + c3 + c4 + c5;
  int p;
  if (type == 0) {
    out[0] = all | c0 << 16 | c1 << 32 | c2 << 48;
    out[1] = c3 | c4 << 16 | c5 << 32;
    p = 2;
  } else {
    out[0] = all | c0 << 32 | (uint64_t)1 << 62;
    out[1] = c1 | c2 << 32;
    out[2] = c3 | c4 << 32;
    out[3] = c5;
    p = 4;
  }
  uint64_t cur = 0;
  int room = 64;
  for (int64_t r = r0; r < r1; ++r) {
    int w;
    const uint64_t x = rld0_code(start[r + 1] - start[r], sym[r], &w);
    if (w > room) {
      w -= room;
      cur |= x >> w;
      if (p < RLD0_BLOCK_WORDS) out[p] = cur;
      ++p;
      room = 64 - w;
      cur = x << room;
    } else {
      room -= w;
      cur |= x << room;
    }
  }
  for (; p < RLD0_BLOCK_WORDS; ++p) { out[p] = cur; cur = 0; }
}

// ---- the chain in tiles of T runs (T >= 96): the stages the device runs as kernels, a lane per call

#define RLD0_ENTRY_STATES (2 * RLD0_MAX_BLOCK_RUNS)   // per tile: one of its first 96 runs x 2 header types
#define RLD0_NO_ENTRY 0xffffffffu

// table[tile * 192 + off * 2 + type] = blocks << 9 | exit offset into the next tile << 2 | exit type: the walk of the
// tile from that entry state, without block numbers (no short block)
SVDSS_HD uint32_t rld0_table_entry(const int64_t* start, const int64_t* P, int64_t R, int64_t T, int64_t tile, int e) {
  const int64_t stop = (tile + 1) * T < R ? (tile + 1) * T : R;
  int64_t r = tile * T + (e >> 1);
  int type = e & 1;
  if (r >= stop) return RLD0_NO_ENTRY;
  const int32_t blocks = rld0_walk_plain(start, P, R, stop, &r, &type);
  return (uint32_t)blocks << 9 | (uint32_t)(r - stop) << 2 | (uint32_t)type;
}

// the one walker over the tables: entry state (offset << 2 | type) and block number of every tile; res[0] = data blocks,
// res[1] = 1 if the chain left the tables (never, by the rule: a guard)
SVDSS_HD void rld0_walk_tables(const uint32_t* table, const int64_t* start, const int64_t* P, int64_t R, int64_t T, int64_t n_tiles,
                               int64_t piece_words, uint32_t* entry_state, int64_t* entry_block, int64_t* res) {
  int64_t r = 0, b = 0, bad = 0;
  int type = 0;
  for (int64_t t = 0; t < n_tiles; ++t) {
    const int64_t off = r - t * T;
    if (off < 0 || off > RLD0_MAX_BLOCK_RUNS) { bad = 1; break; }
    entry_state[t] = (uint32_t)off << 2 | (uint32_t)type;
    entry_block[t] = b;
    const int64_t stop = (t + 1) * T < R ? (t + 1) * T : R;
    if (r >= stop) continue;   // (the last block ended at R and covered this last tile: no block starts here)
    if (off >= RLD0_MAX_BLOCK_RUNS) { bad = 1; break; }
    const uint32_t e = table[t * RLD0_ENTRY_STATES + off * 2 + type];
    if (e == RLD0_NO_ENTRY) { bad = 1; break; }
    const int64_t cnt = e >> 9;
    if (b + cnt <= rld0_next_short(b, piece_words)) {
      r = stop + ((e >> 2) & 127);
      type = (int)(e & 3u);
      b += cnt;
    } else {   // a piece ends in this tile: block by block, with the short capacity where it applies
      while (r < stop) {
        (void)rld0_step(start, P, R, piece_words, b, &r, &type);
        if (type > 1) type = 1;
        ++b;
      }
    }
  }
  res[0] = b;
  res[1] = bad;
}

// tile t from its true entry: desc[b] = first run | type << 62 for every block that starts in it (the last tile adds the
// closing header's, desc[B]).  Returns bit 0: a block makes the device decline, bit 1: the walk disagrees with the walker.
SVDSS_HD int rld0_tile_desc(const int64_t* start, const int64_t* P, int64_t R, int64_t T, int64_t n_tiles, int64_t piece_words, int64_t t,
                            const uint32_t* entry_state, const int64_t* entry_block, int64_t B, int64_t decline_syms, int64_t* desc) {
  const int64_t stop = (t + 1) * T < R ? (t + 1) * T : R;
  int64_t r = t * T + (entry_state[t] >> 2), b = entry_block[t];
  int type = (int)(entry_state[t] & 3u);
  int out = 0;
  while (r < stop && b < B) {
    desc[b] = r | (int64_t)type << 62;
    const int64_t syms = rld0_step(start, P, R, piece_words, b, &r, &type);
    if (rld0_declines(syms, decline_syms)) out |= 1;
    if (type > 1) type = 1;
    ++b;
  }
  const int64_t b_next = t + 1 < n_tiles ? entry_block[t + 1] : B;
  if (b != b_next || r < stop) out |= 2;
  else if (t == n_tiles - 1) desc[B] = R | (int64_t)type << 62;
  return out;
}

// block b of B + 1 (the last: the closing header) from the descriptors
SVDSS_HD void rld0_emit_desc(const int64_t* start, const uint8_t* sym, int64_t R, const int64_t* desc, int64_t B, int64_t b, uint64_t* out) {
  const int64_t d = desc[b];
  const int64_t r0 = d & RLD0_RUN_MASK;
  const int64_t r1 = b < B ? desc[b + 1] & RLD0_RUN_MASK : R;
  const int64_t rp = b > 0 ? desc[b - 1] & RLD0_RUN_MASK : r0;
  rld0_emit_block(start, sym, rp, r0, r1, (int)((uint64_t)d >> 62), out + RLD0_BLOCK_WORDS * b);
}
