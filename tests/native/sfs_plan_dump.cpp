// sfs_plan_dump.cpp -- the knobs and the launch plan of the search batch (svdss_amd/csrc/sfs_plan.h) behind a C interface
// for tests/sfs_plan_lib.py.  g++ only: the header has no HIP in it.  Test infrastructure only.
// With -DSFS_PLAN_MAIN a stand-alone program that prints the default n_seg table (for a run under a sanitizer).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../svdss_amd/csrc/sfs_plan.h"

namespace {
const char* const kVars[] = {"SVDSS_SET", "SVDSS_BS", "SVDSS_BS_DEEP", "SVDSS_TICKETS", "SVDSS_SEGMENTS", "SVDSS_BLOCKS",
                             "SVDSS_ORDER", "SVDSS_EXTRA_LDS", "SVDSS_FALLBACK_DIRECT", "SVDSS_DEBUG"};

// SfsKnobs::from_env with exactly the variables of `env` set ("NAME=VALUE" lines; a variable of kVars that is not named is
// unset); the process's own values are put back before it returns
SfsKnobs knobs_with_env(const char* env) {
  std::vector<std::pair<bool, std::string>> saved;
  for (const char* v : kVars) {
    const char* e = getenv(v);
    saved.emplace_back(e != nullptr, e ? e : "");
    unsetenv(v);
  }
  std::string s = env ? env : "";
  for (size_t pos = 0; pos < s.size();) {
    size_t nl = s.find('\n', pos);
    if (nl == std::string::npos) nl = s.size();
    const std::string line = s.substr(pos, nl - pos);
    const size_t eq = line.find('=');
    if (eq != std::string::npos) setenv(line.substr(0, eq).c_str(), line.substr(eq + 1).c_str(), 1);
    pos = nl + 1;
  }
  const SfsKnobs k = SfsKnobs::from_env();
  for (size_t i = 0; i < saved.size(); ++i) {
    if (saved[i].first) setenv(kVars[i], saved[i].second.c_str(), 1);
    else unsetenv(kVars[i]);
  }
  return k;
}

SfsShape shape_of(const int64_t* sh, double deep_frac) {
  SfsShape s;
  s.n_reads = sh[0]; s.total_syms = sh[1]; s.max_blocks = (int)sh[2];
  s.bs_possible = sh[3] != 0; s.text_and_sa = sh[4] != 0; s.k = (int)sh[5];
  s.deep_frac = deep_frac;
  return s;
}
}  // namespace

// shape: n_reads, total_syms, max_blocks, bs_possible, text_and_sa, k.
// out: use_set, bs, ticket_chunk, segments_set, segments, blocks, order, extra_lds, fallback_direct, debug |
//      use_bs, n_seg, cap_blocks, gather_blocks, use_order, tiny, rec_total, seg_total, seg_info_n, fallback_n, seg_take_n
extern "C" void sfs_plan_eval(const char* env, const int64_t* shape, double deep_frac, int64_t* out, double* bs_deep) {
  const SfsKnobs k = knobs_with_env(env);
  const SfsPlan p = sfs_plan(k, shape_of(shape, deep_frac));
  const int64_t v[21] = {k.use_set, k.bs, k.ticket_chunk, k.segments_set, k.segments, k.blocks, k.order, (int64_t)k.extra_lds,
                         (int64_t)k.fallback_direct, k.debug,
                         p.use_bs, p.n_seg, p.cap_blocks, p.gather_blocks, p.use_order, p.tiny, p.rec_total, p.seg_total,
                         p.seg_info_n, p.fallback_n, p.seg_take_n};
  memcpy(out, v, sizeof v);
  *bs_deep = k.bs_deep;
}

extern "C" int sfs_plan_blocks_for(int cap_blocks, int64_t items) {
  SfsPlan p;
  p.cap_blocks = cap_blocks;
  return p.blocks_for(items);
}

extern "C" int sfs_plan_next_level(int lvl_seg, uint64_t n_fallback, uint64_t direct) { return sfs_next_level(lvl_seg, n_fallback, direct); }

extern "C" int sfs_plan_bs_possible(int have_sa, int k, int64_t n_dollar, int64_t max_dollar) {
  return sfs_bs_possible(have_sa != 0, k, n_dollar, max_dollar) ? 1 : 0;
}

#ifdef SFS_PLAN_MAIN
int main() {
  const int64_t reads[] = {1, 131071, 131072, 131073, 200000, 262144, 262145, 1048576};
  const char* const segs[] = {nullptr, "1", "2", "3", "4", "12", "16", "100", "0", "-5", "x"};
  for (const char* sg : segs) {
    const std::string env = sg ? std::string("SVDSS_SEGMENTS=") + sg : std::string();
    for (int full = 0; full < 2; ++full)
      for (int64_t n : reads) {
        const int64_t sh[6] = {n, n * 15000, 2048, 1, full, 12};
        int64_t out[21];
        double deep = 0;
        sfs_plan_eval(env.c_str(), sh, 0.4, out, &deep);
        printf("SEGMENTS=%s full=%d n_reads=%lld: n_seg %lld use_bs %lld blocks %d gather %lld seg_total %lld\n", sg ? sg : "-", full, (long long)n,
               (long long)out[11], (long long)out[10], sfs_plan_blocks_for((int)out[12], n * out[11]), (long long)out[13], (long long)out[17]);
      }
  }
  printf("ladder from 16: %d, then %d\n", sfs_plan_next_level(16, 1000, 64), sfs_plan_next_level(4, 1000, 64));
  return 0;
}
#endif
