// bgzf_pack.h -- the host half of a batch's BGZF intake, free of HIP: the caller's chunks (compressed bytes, members, footer
// CRCs) checked, counted and laid out as the device reads them.  Compressed bytes go back to back, each chunk rounded up
// to 16; inflated bytes go back to back from a base offset.  (bgzf_intake.h is the device half; tests/bgzf_pack_harness.cpp
// runs this file alone.)
#pragma once
#include <cstdint>

#include "../../include/svdss_hip.h"

// a block as crc32_kernel reads it: where its inflated bytes are, how many, the CRC32 its footer promises
struct CrcBlk { int64_t uoff; int32_t isize; uint32_t crc; };

struct BgzfPlan {
  int64_t n_blocks = 0;     // of all chunks
  int64_t comp_bytes = 0;   // packed: every chunk rounded up to 16
  int64_t inflated = 0;
};

static inline int64_t bgzf_round16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// nullptr, or what is wrong with the six arguments as a whole
static inline const char* bgzf_check_args(int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                          const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks) {
  return n_chunks > 0 && (!comp || !comp_bytes || !blocks || !crc || !n_blocks) ? "bad argument" : nullptr;
}

// the totals of a batch; nullptr, or the first thing wrong with it (P is then unspecified)
static inline const char* bgzf_plan(int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                    const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks, BgzfPlan& P) {
  if (const char* m = bgzf_check_args(n_chunks, comp, comp_bytes, blocks, crc, n_blocks)) return m;
  P = BgzfPlan{};
  for (int32_t c = 0; c < n_chunks; ++c) {
    if (comp_bytes[c] < 0 || n_blocks[c] < 0 || (n_blocks[c] > 0 && (!comp[c] || !blocks[c] || !crc[c]))) return "bad chunk";
    P.n_blocks += n_blocks[c];
    P.comp_bytes += bgzf_round16(comp_bytes[c]);
    for (int64_t i = 0; i < n_blocks[c]; ++i) {
      const svdss_bgzf_block_t& k = blocks[c][i];
      if (k.coff < 0 || k.clen < 0 || k.isize < 0 || k.isize > 65536 || k.coff + k.clen > comp_bytes[c]) return "bad block";
      P.inflated += k.isize;
    }
  }
  return nullptr;
}

// the tables of a planned batch (room for P.n_blocks + 1 entries each; the entry behind the last is not written): block k
// reads its stream at the chunk's place in the packed buffer and writes at base + the sizes in front of it.
// chunk_off[c]: where chunk c begins in the packed buffer (n_chunks entries).
static inline void bgzf_pack(int32_t n_chunks, const int64_t* comp_bytes, const svdss_bgzf_block_t* const* blocks,
                             const uint32_t* const* crc, const int64_t* n_blocks, int64_t base,
                             svdss_bgzf_block_t* h_blk, CrcBlk* h_crc, int64_t* chunk_off) {
  int64_t k = 0, coff = 0, uoff = base;
  for (int32_t c = 0; c < n_chunks; ++c) {
    chunk_off[c] = coff;
    for (int64_t i = 0; i < n_blocks[c]; ++i, ++k) {
      h_blk[k] = blocks[c][i];
      h_blk[k].coff += coff;
      h_blk[k].uoff = uoff;
      h_crc[k] = CrcBlk{uoff, blocks[c][i].isize, crc[c][i]};
      uoff += blocks[c][i].isize;
    }
    coff += bgzf_round16(comp_bytes[c]);
  }
}
