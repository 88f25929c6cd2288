// rld0_plan_dump.cpp -- the block plan of the rld0 encoder (svdss_amd/csrc/rld0_plan.h) behind a C interface for
// tests/test_rld0_plan.py: the stages the device runs as kernels, a loop iteration per lane.  g++ only: the header has no
// HIP in it.  Test infrastructure only.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../svdss_amd/csrc/rld0_plan.h"

extern "C" {

int rld0_dump_code_width(int64_t l) { return rld0_code_width(l); }
int rld0_dump_cap(int type, int is_short) { return rld0_block_cap(type, is_short != 0); }
int rld0_dump_next_type(int64_t syms) { return rld0_next_type(syms); }
int rld0_dump_declines(int64_t syms, int64_t threshold) { return rld0_declines(syms, threshold) ? 1 : 0; }
int rld0_dump_short(int64_t b, int64_t piece_words) { return rld0_block_short(b, piece_words) ? 1 : 0; }

// The data words of the runs (lens, syms) with pieces of piece_words words.  T == 0: the chain block by block (rld0_step);
// T >= 96: in tiles of T runs -- tables, the one walker, the tiles' own walks -- as the device does it.  desc (R + 2
// entries): first run | type << 62 of every block and of the closing header.  words: 8 (R + 1) entries of room.
// Returns -1 on a bad argument, else bit 0: a block reached decline_syms, bit 1: the stages disagree; *k = data words,
// *n_blocks = data blocks.
int rld0_dump_encode(const int64_t* lens, const uint8_t* syms, int64_t R, int64_t piece_words, int64_t T, int64_t decline_syms,
                     int64_t* desc, uint64_t* words, int64_t* k, int64_t* n_blocks) {
  if (R <= 0 || piece_words < 16 || piece_words % 8 != 0 || (T != 0 && T < RLD0_MAX_BLOCK_RUNS)) return -1;
  std::vector<int64_t> start((size_t)R + 1, 0), P((size_t)R + 1, 0);
  for (int64_t r = 0; r < R; ++r) {
    start[(size_t)r + 1] = start[(size_t)r] + lens[r];
    P[(size_t)r + 1] = P[(size_t)r] + rld0_code_width(lens[r]);
  }
  int flags = 0;
  int64_t B = 0;
  if (T == 0) {
    int64_t r = 0;
    int type = 0;
    while (r < R) {
      desc[B] = r | (int64_t)type << 62;
      const int64_t s = rld0_step(start.data(), P.data(), R, piece_words, B, &r, &type);
      if (rld0_declines(s, decline_syms)) flags |= 1;
      if (type > 1) type = 1;
      ++B;
    }
    desc[B] = R | (int64_t)type << 62;
  } else {
    const int64_t n_tiles = (R + T - 1) / T;
    std::vector<uint32_t> table((size_t)(n_tiles * RLD0_ENTRY_STATES)), entry_state((size_t)n_tiles);
    std::vector<int64_t> entry_block((size_t)n_tiles);
    for (int64_t g = 0; g < n_tiles * RLD0_ENTRY_STATES; ++g)
      table[(size_t)g] = rld0_table_entry(start.data(), P.data(), R, T, g / RLD0_ENTRY_STATES, (int)(g % RLD0_ENTRY_STATES));
    int64_t res[2] = {0, 0};
    rld0_walk_tables(table.data(), start.data(), P.data(), R, T, n_tiles, piece_words, entry_state.data(), entry_block.data(), res);
    if (res[1] || res[0] <= 0 || res[0] > R) return 2;
    B = res[0];
    for (int64_t t = 0; t < n_tiles; ++t)
      flags |= rld0_tile_desc(start.data(), P.data(), R, T, n_tiles, piece_words, t, entry_state.data(), entry_block.data(), B, decline_syms, desc);
  }
  if (!(flags & 2))
    for (int64_t b = 0; b <= B; ++b) rld0_emit_desc(start.data(), syms, R, desc, B, b, words);
  *n_blocks = B;
  *k = B * RLD0_BLOCK_WORDS + rld0_hdr_words((int)((uint64_t)desc[B] >> 62));
  return flags;
}

}  // extern "C"
