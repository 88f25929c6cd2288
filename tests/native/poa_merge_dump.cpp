// poa_merge_dump.cpp -- which groups of a wave of first-stage launches become one launch (poa_merge_wave, poa_merged_group of
// svdss_amd/csrc/poa_plan.h) behind a C interface for tests/test_poa_merge.py: the answer comes back as JSON text.  g++ only:
// the header has no HIP in it.  Test infrastructure only.
#include <cstdint>
#include <string>
#include <vector>

#include "../../svdss_amd/csrc/poa_plan.h"

namespace {
thread_local std::string g_json;

void put(std::string& s, const char* name, const std::vector<int64_t>& v) {
  s += "\"" + std::string(name) + "\":[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
  s += "]";
}
}  // namespace

// n groups given by (gw, cols, wave, number of tasks).  Task i of group g: id 1000 g + i, nc = 10 + i (its consensus bytes),
// 100 + 7 g + i ints of workspace, max_len 50 (g + 1) + i.  merge: 0 / 1 the knob, -1 the knob as PoaKnobs::from_env reads it.
// Launches of groups [g0, g1): {c2, c1, single, n2, w32, w8, max_len, bundle_lds, ids, ws_off, cons_off} (the last six of the
// merged group, or of the single one).
extern "C" const char* poa_merge_json(const int32_t* gw, const int32_t* cols, const int32_t* wave, const int32_t* n_tasks, int n, int g0, int g1,
                                      int merge) {
  std::vector<PoaGroup> groups((size_t)n);
  for (int g = 0; g < n; ++g) {
    PoaGroup& G = groups[(size_t)g];
    G.gw = gw[g]; G.cols = cols[g]; G.wave = wave[g];
    for (int i = 0; i < n_tasks[g]; ++i) {
      PoaCand cd{};
      cd.c = 1000 * g + i;
      cd.t.nc = 10 + i;
      cd.t.max_len = 50 * (g + 1) + i;
      G.add(cd, 100 + 7 * g + i);
    }
  }
  PoaKnobs k = merge < 0 ? PoaKnobs::from_env() : PoaKnobs();
  if (merge >= 0) k.merge = merge != 0;
  const std::vector<PoaLaunch> ls = poa_merge_wave(k, groups, (size_t)g0, (size_t)g1);
  std::string& s = g_json;
  s = "[";
  for (size_t li = 0; li < ls.size(); ++li) {
    const PoaLaunch& L = ls[li];
    size_t n2 = 0;
    const PoaGroup m = L.single >= 0 ? groups[(size_t)L.single]
                                     : poa_merged_group(L.c2 >= 0 ? &groups[(size_t)L.c2] : nullptr, L.c1 >= 0 ? &groups[(size_t)L.c1] : nullptr, n2);
    s += (li ? ",{" : "{");
    s += "\"c2\":" + std::to_string(L.c2) + ",\"c1\":" + std::to_string(L.c1) + ",\"single\":" + std::to_string(L.single) +
         ",\"n2\":" + std::to_string(n2) + ",\"w32\":" + std::to_string(m.w32) + ",\"w8\":" + std::to_string(m.w8) +
         ",\"max_len\":" + std::to_string(m.max_len) + ",\"bundle_lds\":" + std::to_string(m.bundle_lds) + ",";
    std::vector<int64_t> ws, co, nc;
    for (const PoaWaveTask& t : m.tasks) { ws.push_back(t.ws_off); co.push_back(t.cons_off); nc.push_back(t.nc); }
    put(s, "ids", m.ids); s += ",";
    put(s, "ws_off", ws); s += ",";
    put(s, "cons_off", co); s += ",";
    put(s, "nc", nc);
    s += "}";
  }
  s += "]";
  return s.c_str();
}
