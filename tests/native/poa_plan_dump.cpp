// poa_plan_dump.cpp -- the planner of the POA batch (svdss_amd/csrc/poa_plan.h) behind a C interface for
// tests/poa_plan_lib.py: plans come back as JSON text.  g++ only: the header has no HIP in it.  Test infrastructure only.
#include <cstdint>
#include <cstdio>
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

// knobs: use_lds, use_quad, quad_gw (< 0: not set), quad_short, quad_minwork_pct, quad_rows16, quad_rows32, nc_pct, noprio, no_mix
PoaKnobs knobs_of(const int64_t* k) {
  PoaKnobs kn;
  kn.use_lds = k[0] != 0; kn.use_quad = k[1] != 0;
  kn.quad_gw_set = k[2] >= 0; kn.quad_gw = (int)k[2];
  kn.quad_short = k[3]; kn.quad_minwork_pct = k[4]; kn.quad_rows16 = k[5]; kn.quad_rows32 = k[6];
  kn.nc_pct = (int)k[7]; kn.noprio = k[8] != 0; kn.no_mix = k[9] != 0;
  return kn;
}
}  // namespace

// One round's plan for the sub-clusters ids[0..n_ids).  skip_round0 / round0_no_wider: one byte per cluster (the second is
// written in round -1).  Tasks: [nc, ec, max_len, ws, rs, ring, prio, ws_off, cons_off, n_seqs].
extern "C" const char* poa_plan_round_json(const int64_t* seq_off, const int64_t* cluster_off, int64_t n_clusters, const int64_t* ids, int64_t n_ids,
                                           int round, const int64_t* knobs, int n_cus, uint64_t ws_budget, const uint8_t* skip_round0,
                                           uint8_t* round0_no_wider) {
  PoaBatchIn in;
  in.seq_off = seq_off; in.cluster_off = cluster_off; in.n_clusters = n_clusters;
  in.knobs = knobs_of(knobs); in.n_cus = n_cus; in.ws_budget = (size_t)ws_budget;
  in.set_max_work();
  const std::vector<int64_t> cur(ids, ids + n_ids);
  const std::vector<uint8_t> skip(skip_round0, skip_round0 + n_clusters);
  std::vector<uint8_t> no_wider(round0_no_wider, round0_no_wider + n_clusters);
  const PoaRoundPlan p = poa_plan_round(in, round, cur, skip, no_wider);
  for (int64_t c = 0; c < n_clusters; ++c) round0_no_wider[c] = no_wider[(size_t)c];
  std::string& s = g_json;
  s = "{";
  put(s, "next", p.next); s += ",";
  put(s, "hbm", p.hbm); s += ",";
  put(s, "cuts", std::vector<int64_t>(p.cuts.begin(), p.cuts.end()));
  s += ",\"groups\":[";
  for (size_t gi = 0; gi < p.groups.size(); ++gi) {
    const PoaGroup& g = p.groups[gi];
    char head[256];
    snprintf(head, sizeof head, "%s{\"gw\":%d,\"cols\":%d,\"wave\":%d,\"max_len\":%d,\"lds\":%zu,\"bundle_lds\":%zu,\"w32\":%lld,\"w8\":%lld,\"bytes\":%zu,",
             gi ? "," : "", g.gw, g.cols, g.wave, g.max_len, g.lds, g.bundle_lds, (long long)g.w32, (long long)g.w8, g.bytes());
    s += head;
    put(s, "ids", g.ids);
    s += ",\"tasks\":[";
    for (size_t k = 0; k < g.tasks.size(); ++k) {
      const PoaWaveTask& t = g.tasks[k];
      put(s += (k ? ",{" : "{"), "t", {t.nc, t.ec, t.max_len, t.ws, t.rs, t.ring, t.prio, t.ws_off, t.cons_off, t.n_seqs});
      s += "}";
    }
    s += "]}";
  }
  s += "]}";
  return s.c_str();
}

// One sub-cluster in one round (the sizes of rounds 0-2 also where it does not fit them): out = {where (0 run, 1 next round, 2 HBM kernel), w_band, width, gw, cols, ws, rs, ring, nc, ec, lds}
extern "C" void poa_plan_size(const int64_t* seq_off, const int64_t* cluster_off, int64_t n_clusters, int64_t c, int round, const int64_t* knobs,
                              int64_t* out) {
  PoaBatchIn in;
  in.seq_off = seq_off; in.cluster_off = cluster_off; in.n_clusters = n_clusters;
  in.knobs = knobs_of(knobs);
  in.set_max_work();
  PoaCand cd{};
  uint8_t no_wider = 0;
  out[0] = poa_size_cluster(in, round, c, false, cd, no_wider);
  out[1] = poa_w_band(poa_cluster_shape(seq_off, cluster_off, c).maxl);
  const int64_t rest[9] = {cd.width, cd.gw, cd.cols, cd.t.ws, cd.t.rs, cd.t.ring, cd.t.nc, cd.t.ec, (int64_t)cd.lds};
  for (int k = 0; k < 9; ++k) out[2 + k] = rest[k];
}

// The launches of one pass of the HBM kernel over todo[0..n_todo).  Tasks: [cap_nodes, cap_edges, max_len, pool_cap, node_off,
// edge_off, dp_off, op_off, row_off64, base_off, cons_off]
extern "C" const char* poa_plan_hbm_json(const int64_t* seq_off, const int64_t* cluster_off, const int64_t* todo, int64_t n_todo, int pass) {
  const std::vector<int64_t> td(todo, todo + n_todo);
  std::string& s = g_json;
  s = "[";
  PoaHbmLaunch L;
  for (size_t pos = 0; pos < td.size();) {
    s += pos ? ",{" : "{";
    pos = poa_plan_hbm(seq_off, cluster_off, td, pos, pass, L);
    put(s, "ids", L.ids);
    s += ",\"w32\":" + std::to_string(L.w32) + ",\"w64\":" + std::to_string(L.w64) + ",\"w8\":" + std::to_string(L.w8) + ",\"tasks\":[";
    for (size_t k = 0; k < L.tasks.size(); ++k) {
      const PoaTask& t = L.tasks[k];
      put(s += (k ? ",{" : "{"), "t", {t.cap_nodes, t.cap_edges, t.max_len, t.pool_cap, t.node_off, t.edge_off, t.dp_off, t.op_off, t.row_off64, t.base_off, t.cons_off});
      s += "}";
    }
    s += "]}";
  }
  s += "]";
  return s.c_str();
}

extern "C" int64_t poa_plan_ws_ints(int nc, int ec, int max_len, int ws) { return poa_wave_ws_ints(nc, ec, max_len, ws); }
extern "C" int64_t poa_plan_wave_lds(int nc, int max_len, int rs, int ring) { return (int64_t)poa_wave_lds_bytes(nc, max_len, rs, ring); }
extern "C" int64_t poa_plan_bundle_lds(int nc) { return (int64_t)poa_bundle_lds_bytes(nc); }
extern "C" int64_t poa_plan_quad_lds(int gw, int cols, int max_len) { return (int64_t)poa_quad_lds_bytes(gw, cols, max_len); }
extern "C" int poa_plan_quad_supported(int gw, int cols) { return poa_quad_supported(gw, cols) ? 1 : 0; }
extern "C" uint64_t poa_plan_ws_budget(int64_t ws_gb, int have_mem_info, uint64_t free_bytes, uint64_t arena_cap) {
  PoaKnobs k;
  k.ws_gb = ws_gb;
  return poa_ws_budget(k, have_mem_info != 0, (size_t)free_bytes, (size_t)arena_cap);
}
