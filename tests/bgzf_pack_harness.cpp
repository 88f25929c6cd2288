// bgzf_pack_harness.cpp -- csrc/bgzf_pack.h on the CPU, alone, under AddressSanitizer / UndefinedBehaviorSanitizer
// (tests/test_bgzf_pack_host.py builds and runs it).  Parts: `reject` -- every clause of the three rejections with its
// message, and that the first failing clause wins; `tables` -- totals and tables of the shapes the intake meets, entry
// by entry against a recomputation written out here.  Buffers have exactly the size the header promises to stay within.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../svdss_amd/csrc/bgzf_pack.h"

static int g_fail = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

// chunks as a caller holds them: every array exactly as long as it says (ASan sees one byte more)
struct Chunks {
  std::vector<std::unique_ptr<uint8_t[]>> bytes;
  std::vector<std::unique_ptr<svdss_bgzf_block_t[]>> blk;
  std::vector<std::unique_ptr<uint32_t[]>> crcs;
  std::vector<const uint8_t*> comp;
  std::vector<int64_t> comp_bytes, n_blocks;
  std::vector<const svdss_bgzf_block_t*> blocks;
  std::vector<const uint32_t*> crc;
  // members = {coff, clen, isize}; crc of member i of chunk c: 1000 c + i + 7
  void add(int64_t n_bytes, const std::vector<svdss_bgzf_block_t>& members) {
    const uint32_t c = (uint32_t)comp.size();
    bytes.emplace_back(new uint8_t[(size_t)n_bytes]);
    blk.emplace_back(new svdss_bgzf_block_t[members.size()]);
    crcs.emplace_back(new uint32_t[members.size()]);
    for (size_t i = 0; i < members.size(); ++i) { blk.back()[i] = members[i]; crcs.back()[i] = 1000u * c + (uint32_t)i + 7u; }
    comp.push_back(bytes.back().get()); comp_bytes.push_back(n_bytes); n_blocks.push_back((int64_t)members.size());
    blocks.push_back(blk.back().get()); crc.push_back(crcs.back().get());
  }
  int32_t n() const { return (int32_t)comp.size(); }
  const char* plan(BgzfPlan& P) const { return bgzf_plan(n(), comp.data(), comp_bytes.data(), blocks.data(), crc.data(), n_blocks.data(), P); }
};

static svdss_bgzf_block_t M(int64_t coff, int32_t clen, int32_t isize) { return svdss_bgzf_block_t{coff, clen, isize, -12345}; }
static bool says(const char* got, const char* want) { return got ? (want && !strcmp(got, want)) : !want; }

static void part_reject() {
  BgzfPlan P;
  int n_clauses = 0;
  // ---- "bad argument": each of the five arrays missing (with chunks to read); nothing is missing of zero chunks
  {
    Chunks C; C.add(64, {M(18, 10, 5)});
    for (int k = 0; k < 5; ++k, ++n_clauses) {
      const char* m = bgzf_plan(1, k == 0 ? nullptr : C.comp.data(), k == 1 ? nullptr : C.comp_bytes.data(), k == 2 ? nullptr : C.blocks.data(),
                                k == 3 ? nullptr : C.crc.data(), k == 4 ? nullptr : C.n_blocks.data(), P);
      EXPECT(says(m, "bad argument"));
      EXPECT(says(bgzf_check_args(1, k == 0 ? nullptr : C.comp.data(), k == 1 ? nullptr : C.comp_bytes.data(), k == 2 ? nullptr : C.blocks.data(),
                                  k == 3 ? nullptr : C.crc.data(), k == 4 ? nullptr : C.n_blocks.data()), "bad argument"));
    }
    EXPECT(says(bgzf_plan(0, nullptr, nullptr, nullptr, nullptr, nullptr, P), nullptr));
    EXPECT(says(bgzf_check_args(0, nullptr, nullptr, nullptr, nullptr, nullptr), nullptr));
    EXPECT(says(C.plan(P), nullptr));
  }
  // ---- "bad chunk": a negative size, a negative count, members without bytes / table / CRCs
  {
    Chunks C; C.add(64, {M(18, 10, 5)});
    C.comp_bytes[0] = -1; EXPECT(says(C.plan(P), "bad chunk")); C.comp_bytes[0] = 64; ++n_clauses;
    C.n_blocks[0] = -1; EXPECT(says(C.plan(P), "bad chunk")); C.n_blocks[0] = 1; ++n_clauses;
    const uint8_t* c0 = C.comp[0]; C.comp[0] = nullptr; EXPECT(says(C.plan(P), "bad chunk")); C.comp[0] = c0; ++n_clauses;
    const svdss_bgzf_block_t* b0 = C.blocks[0]; C.blocks[0] = nullptr; EXPECT(says(C.plan(P), "bad chunk")); C.blocks[0] = b0; ++n_clauses;
    const uint32_t* r0 = C.crc[0]; C.crc[0] = nullptr; EXPECT(says(C.plan(P), "bad chunk")); C.crc[0] = r0; ++n_clauses;
    EXPECT(says(C.plan(P), nullptr));
    // a chunk without members may come without any of the three
    C.n_blocks[0] = 0; C.comp[0] = nullptr; C.blocks[0] = nullptr; C.crc[0] = nullptr;
    EXPECT(says(C.plan(P), nullptr));
    EXPECT(P.n_blocks == 0 && P.comp_bytes == 64 && P.inflated == 0);
  }
  // ---- "bad block": each of the five clauses, and their edges on the good side
  {
    const svdss_bgzf_block_t bad[] = {M(-1, 10, 5), M(18, -1, 5), M(18, 10, -1), M(18, 10, 65537), M(55, 10, 5)};
    for (const svdss_bgzf_block_t& b : bad) {
      Chunks C; C.add(64, {M(18, 10, 5), b});
      EXPECT(says(C.plan(P), "bad block"));
      ++n_clauses;
    }
    Chunks C; C.add(64, {M(0, 0, 0), M(18, 10, 65536), M(54, 10, 5), M(64, 0, 0)});
    EXPECT(says(C.plan(P), nullptr));
    EXPECT(P.n_blocks == 4 && P.inflated == 65541);
  }
  // ---- the first failing clause wins: arguments before chunks, a chunk before its own blocks, chunk c's block before chunk c + 1
  {
    Chunks C; C.add(64, {M(-1, 10, 5)}); C.add(64, {M(18, 10, 5)});
    C.comp_bytes[1] = -1;
    EXPECT(says(C.plan(P), "bad block"));                       // chunk 0's block is met before chunk 1
    EXPECT(says(bgzf_plan(2, nullptr, C.comp_bytes.data(), C.blocks.data(), C.crc.data(), C.n_blocks.data(), P), "bad argument"));
    C.comp_bytes[0] = -1;
    EXPECT(says(C.plan(P), "bad chunk"));                       // chunk 0 itself before its block
    Chunks D; D.add(64, {M(18, 10, 5)}); D.add(64, {M(18, 10, 5)});
    D.n_blocks[1] = -1;
    EXPECT(says(D.plan(P), "bad chunk"));
  }
  printf("reject %s: %d clauses\n", g_fail ? "FAILED" : "ok", n_clauses);
}

// totals and tables of C at `base`, against the rules written out once more
static void check_tables(const Chunks& C, int64_t base, const std::vector<int64_t>& want_off, int64_t want_blocks, int64_t want_comp, int64_t want_inf) {
  BgzfPlan P;
  EXPECT(says(C.plan(P), nullptr));
  EXPECT(P.n_blocks == want_blocks && P.comp_bytes == want_comp && P.inflated == want_inf);
  const size_t n = (size_t)P.n_blocks;
  std::unique_ptr<svdss_bgzf_block_t[]> h_blk(new svdss_bgzf_block_t[n + 1]);
  std::unique_ptr<CrcBlk[]> h_crc(new CrcBlk[n + 1]);
  std::unique_ptr<int64_t[]> off(new int64_t[(size_t)C.n()]);
  const svdss_bgzf_block_t guard_b = M(-7, -7, -7);
  const CrcBlk guard_c{-7, -7, 7u};
  h_blk[n] = guard_b; h_crc[n] = guard_c;
  bgzf_pack(C.n(), C.comp_bytes.data(), C.blocks.data(), C.crc.data(), C.n_blocks.data(), base, h_blk.get(), h_crc.get(), off.get());
  EXPECT((int64_t)want_off.size() == C.n());
  size_t k = 0;
  int64_t at = 0, inf = 0;
  for (int32_t c = 0; c < C.n(); ++c) {
    EXPECT(off[c] == at && off[c] == want_off[(size_t)c] && at % 16 == 0);
    for (int64_t i = 0; i < C.n_blocks[(size_t)c]; ++i, ++k) {
      const svdss_bgzf_block_t& m = C.blocks[(size_t)c][i];
      EXPECT(h_blk[k].coff == at + m.coff && h_blk[k].clen == m.clen && h_blk[k].isize == m.isize && h_blk[k].uoff == base + inf);
      EXPECT(h_crc[k].uoff == base + inf && h_crc[k].isize == m.isize && h_crc[k].crc == 1000u * (uint32_t)c + (uint32_t)i + 7u);
      EXPECT(h_blk[k].coff + h_blk[k].clen <= want_comp);                 // every stream inside the packed buffer
      inf += m.isize;
    }
    at += (C.comp_bytes[(size_t)c] + 15) / 16 * 16;
  }
  EXPECT(k == n && at == want_comp && inf == want_inf);
  EXPECT(!memcmp(&h_blk[n], &guard_b, sizeof guard_b) && !memcmp(&h_crc[n], &guard_c, sizeof guard_c));   // the entry behind the last: not written
}

static void part_tables() {
  int n_shapes = 0;
  for (const int64_t base : {(int64_t)0, (int64_t)(1 << 20) + 4096, ((int64_t)3 << 30) + 5}) {
    { Chunks C; check_tables(C, base, {}, 0, 0, 0); ++n_shapes; }                                          // zero chunks
    { Chunks C; C.add(100, {}); check_tables(C, base, {0}, 0, 112, 0); ++n_shapes; }                       // bytes but no members
    { Chunks C; C.add(0, {}); C.add(40, {M(18, 14, 9)}); check_tables(C, base, {0, 0}, 1, 48, 9); ++n_shapes; }   // a chunk of 0 bytes
    { Chunks C; C.add(16, {M(0, 16, 3)}); C.add(32, {M(2, 30, 4)}); check_tables(C, base, {0, 16}, 2, 48, 7); ++n_shapes; }   // whole multiples of 16
    {                                                                                                      // isize 0 and 65536
      Chunks C; C.add(200, {M(18, 2, 0), M(46, 100, 65536), M(172, 2, 0), M(192, 8, 1)});
      check_tables(C, base, {0}, 4, 208, 65537); ++n_shapes;
    }
    {                                                                                                      // lengths 1, 17, 4099: offsets 0, 16, 48
      Chunks C; C.add(1, {M(0, 1, 1)}); C.add(17, {M(0, 9, 255), M(9, 8, 256)}); C.add(4099, {M(18, 4000, 0xff00), M(4045, 54, 257)});
      check_tables(C, base, {0, 16, 48}, 5, 16 + 32 + 4112, 1 + 255 + 256 + 0xff00 + 257); ++n_shapes;
    }
  }
  printf("tables %s: %d shapes\n", g_fail ? "FAILED" : "ok", n_shapes);
}

int main(int argc, char** argv) {
  const std::string part = argc > 1 ? argv[1] : "";
  if (part == "reject") part_reject();
  else if (part == "tables") part_tables();
  else { fprintf(stderr, "usage: %s reject|tables\n", argv[0]); return 2; }
  return g_fail ? 1 : 0;
}
