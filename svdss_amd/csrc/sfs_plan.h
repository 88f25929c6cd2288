// sfs_plan.h -- everything of svdss_sfs_search_batch_device (sfs_search.hip) that is arithmetic over the batch's shape: the
// knobs, the segment count, the BS / plain choice, the grid sizes, the heavy-first order, the buffer sizes and the step of
// the fallback ladder.  No HIP types and no HIP calls: g++ compiles it on its own (tests/native/sfs_plan_dump.cpp,
// tests/test_sfs_plan.py); nothing below SfsKnobs::from_env reads the environment.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

// ---------------------------------------------------------------------------------------------------------------- knobs
// Every environment variable of the search batch, read once per call of svdss_sfs_search_batch_device (README: "The knobs
// of the search batch") -- per call, not per process: callers change them between calls.  SVDSS_SEARCH_CUS belongs to
// svdss_make_stream.
struct SfsKnobs {
  bool use_set = true;            // SVDSS_SET parses to non-zero (0: walk the BWT where 2-4 occurrences could be followed in the text)
  int bs = -1;                    // SVDSS_BS: 0 / 1 when its first character is '0' / '1', else -1 (unset: the reference decides)
  double bs_deep = 0.35;          // SVDSS_BS_DEEP: the deep_frac from which the BS instantiation is launched
  int ticket_chunk = 8;           // SVDSS_TICKETS (> 0): work-item tickets a wavefront takes at a time
  bool segments_set = false;      // SVDSS_SEGMENTS: segments per read (then clamped like the default)
  int segments = 0;
  int blocks = 0;                 // SVDSS_BLOCKS (> 0): cap of the search grid; 0: no cap
  bool order = true;              // SVDSS_ORDER does not parse to 0 (0: the input order instead of heavy reads first)
  size_t extra_lds = 0;           // SVDSS_EXTRA_LDS (developer knob): unused dynamic LDS per block, to study the kernel at lower occupancy
  unsigned long long fallback_direct = 64;   // SVDSS_FALLBACK_DIRECT: up to this many unstitched reads go straight to one lane each
  bool debug = false;             // SVDSS_DEBUG

  static SfsKnobs from_env() {
    SfsKnobs k;
    if (const char* e = getenv("SVDSS_SET")) k.use_set = atoi(e) != 0;
    if (const char* e = getenv("SVDSS_BS")) if (*e == '0' || *e == '1') k.bs = *e == '1';
    if (const char* e = getenv("SVDSS_BS_DEEP")) k.bs_deep = atof(e);
    if (const char* e = getenv("SVDSS_TICKETS")) k.ticket_chunk = atoi(e) > 0 ? atoi(e) : 8;
    if (const char* e = getenv("SVDSS_SEGMENTS")) { k.segments_set = true; k.segments = atoi(e); }
    if (const char* e = getenv("SVDSS_BLOCKS")) k.blocks = atoi(e) > 0 ? atoi(e) : 0;
    if (const char* e = getenv("SVDSS_ORDER")) k.order = atoi(e) != 0;
    if (const char* e = getenv("SVDSS_EXTRA_LDS")) k.extra_lds = (size_t)atol(e);
    if (const char* e = getenv("SVDSS_FALLBACK_DIRECT")) k.fallback_direct = (unsigned long long)atoll(e);
    k.debug = getenv("SVDSS_DEBUG") != nullptr;
    return k;
  }
};

// ----------------------------------------------------------------------------------------------------------------- plan
// What the plan needs of the batch and the index.
struct SfsShape {
  int64_t n_reads = 0;
  int64_t total_syms = 0;
  int max_blocks = 0;          // CUs x 8: 8 x 256 threads = 32 waves per CU
  bool bs_possible = false;    // sfs_bs_possible
  double deep_frac = 0.0;      // svdss_index::deep_frac
  bool text_and_sa = false;    // text and suffix array resident (false: rank blocks alone, svdss_index_attach_blocks)
  int k = 0;                   // order of the k-mer table
};

// (BS needs the suffix array, a k-mer table, and few enough records for their '$' positions to sit in LDS: max_dollar is
// SV_BS_MAX_DOLLAR of sfs_core2.h)
inline bool sfs_bs_possible(bool have_sa, int k, int64_t n_dollar, int64_t max_dollar) {
  return have_sa && k > 0 && n_dollar > 0 && n_dollar <= max_dollar;
}

struct SfsPlan {
  bool use_bs = false;       // launch the BS instantiation
  int n_seg = 1;             // segments per read of the first pass; a power of two
  int cap_blocks = 0;        // most blocks of a search launch
  int gather_blocks = 1;     // grid of the gather kernel
  bool use_order = false;    // heavy reads first (sfs_order_kernel)
  bool tiny = false;         // the batch is searched in a padded copy
  int64_t rec_total = 0;     // records (uint2) of the default per-read regions
  // the segment buffers, in elements; zero when n_seg == 1
  int64_t seg_total = 0;     // seg_rec (uint4)
  int64_t seg_info_n = 0;    // seg_info (SvSegInfo)
  int64_t fallback_n = 0;    // fallback ids (int64_t)
  int64_t seg_take_n = 0;    // seg_take (int32_t)

  int blocks_for(int64_t items) const {
    const int64_t w = (items + 255) / 256;
    return (int)(w < 1 ? 1 : (w < cap_blocks ? w : cap_blocks));
  }
};

inline SfsPlan sfs_plan(const SfsKnobs& kn, const SfsShape& s) {
  SfsPlan pl;
  const int64_t n_reads = s.n_reads, total_syms = s.total_syms;
  // The BS instantiation is chosen by the reference (round 5; rounds 3-4: opt-in).  Measured at GRCh38 lengths with 45 % of
  // the bases in 40 repeat families (profiles/r04h_search_bs.txt, ms per 1,048,576 reads, plain -> BS kernel): copies 1 %
  // apart 408 -> 363, 5 % apart 197 -> 209, 15 % apart 103 -> 108, the headline reference 67.7 either way when the plain
  // kernel is the one launched.  svdss_index::deep_frac (the share of K-mer occurrences in K-mers with SV_BS_MIN or more
  // of them, sampled while the table is built) was 0.001 / 0.206 / 0.329 / 0.371 on the four: from 0.35 on the copies are
  // young enough for the binary search to pay.  Most of a real genome's repeats are old: it keeps the plain kernel.
  // SVDSS_BS=0|1 overrides, SVDSS_BS_DEEP moves the threshold.  Either kernel gives the same SFS and extension counts.
  pl.use_bs = s.bs_possible && s.deep_frac >= kn.bs_deep;
  if (kn.bs >= 0) pl.use_bs = s.bs_possible && kn.bs == 1;

  // (the kernel fetches a read's symbols 64 bytes at a time: a batch smaller than that is searched in a padded copy)
  pl.tiny = total_syms < 64;

  // Small batches cannot fill the GPU with one lane per read (256 CUs x 16 waves x 64 lanes):
  // cut every read into n_seg segments searched by separate lanes and stitch the chains.
  int n_seg = 1;
  {
    const int64_t lanes = (int64_t)s.max_blocks * 256 / 2;   // 4 waves per SIMD resident
    const int64_t want = 4 * lanes / (n_reads > 0 ? n_reads : 1);   // ~4 items per resident lane: short items bound the tail
    n_seg = (int)(want < 4 ? 1 : (want > 8 ? 8 : want));   // large batches fill the GPU with one lane per read; beyond 8
                                                              // the odd unstitchable read costs more than it saves
    // On the rank blocks alone (no text, no suffix array: svdss_index_attach_blocks) a read is thousands of dependent rank steps
    // whatever its segments do, and the reads such a search gets -- smoothed ones -- have too few SFS for their segments to be
    // stitched at (27 % searched again at 30x): from half a lane-load of reads on, one lane per read (`search` at 30x: the two
    // launches 0.44 -> 0.29 s, profiles/r06av_*)
    if (!s.text_and_sa && 2 * n_reads >= lanes) n_seg = 1;
    if (kn.segments_set) n_seg = kn.segments;
    if (n_seg < 1) n_seg = 1;
    if (n_seg > 16) n_seg = 16;
    while (n_seg & (n_seg - 1)) n_seg &= n_seg - 1;   // power of two: item -> (read, segment) by shift
    if (total_syms / (n_reads > 0 ? n_reads : 1) < 1024) n_seg = 1;
    if (n_reads * (int64_t)n_seg >= ((int64_t)1 << 31)) n_seg = 1;   // item tickets are 32-bit in the kernel
  }
  pl.n_seg = n_seg;

  pl.rec_total = (total_syms >> 3) + 8 * n_reads + 16;
  if (n_seg > 1) {
    pl.seg_total = (total_syms >> 3) + (8 + 24 * (int64_t)n_seg) * n_reads + 64;
    pl.seg_info_n = n_reads * n_seg;
    pl.fallback_n = n_reads;
    pl.seg_take_n = 2 * n_reads * n_seg;
  }

  pl.cap_blocks = kn.blocks > 0 ? kn.blocks : s.max_blocks;
  const int64_t gw = (n_reads + 3) / 4;  // 4 waves per block, one read per wave iteration
  pl.gather_blocks = (int)(gw < 4 * (int64_t)s.max_blocks ? (gw > 0 ? gw : 1) : 4 * (int64_t)s.max_blocks);

  // heavy reads first (see sfs_order_kernel); SVDSS_ORDER=0 keeps the input order
  pl.use_order = n_reads >= 1024 && s.k >= 8 && kn.order;
  return pl;
}

// The fallback ladder: reads whose chains could not be stitched are searched again with a quarter of the segments (their
// boundaries fall elsewhere), at the end one lane per read.
// (a handful of reads: one lane each at once -- a launch of so few lanes lasts as long as its longest read either
// way, and an intermediate level that fails again costs that time twice; SVDSS_FALLBACK_DIRECT moves the limit)
inline int sfs_next_level(int lvl_seg, unsigned long long n_fallback, unsigned long long direct) {
  return lvl_seg / 4 < 1 || n_fallback <= direct ? 1 : lvl_seg / 4;
}
