// poa_plan.h -- everything of svdss_poa_consensus_batch (poa.hip) that is arithmetic over the read lengths: the knobs, the
// sizes of a sub-cluster's graph / band / LDS / workspace for each stage, the packing of a round's sub-clusters into
// launches and of the launches into waves under the workspace budget, and the tasks of the HBM fallback.  No HIP types and
// no HIP calls: g++ compiles it on its own (tests/native/poa_plan_dump.cpp, tests/test_poa_plan.py); nothing below
// PoaKnobs::from_env reads the environment or the clock.
//
// The stages: round -1 is poa_quad.hip (several sub-clusters per wavefront); rounds 0-2 are poa_wave.hip with growing
// generosity -- ring rows of 2w + 33 columns and a graph of ~1.5 x the longest read (what nearly every sub-cluster needs),
// then the specification's widest band (2w + 129) and 3 x, then full-matrix rows (a band that lost the sink).  What is
// still left goes to the HBM kernel of poa.hip: pass 0 with a banded DP pool, pass 1 with a full-size one.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poa_quad_defs.h"
#include "poa_task.h"

#ifdef __HIPCC__
#define POA_HD __host__ __device__
#else
#define POA_HD
#endif

// ---------------------------------------------------------------------------------------------------------------- knobs
// Every environment variable of the POA host path, read once per call of svdss_poa_consensus_batch (README: "The knobs of
// the POA batch").  SVDSS_CALL_CUS belongs to svdss_make_stream.
struct PoaKnobs {
  bool use_lds = true;           // SVDSS_POA_HBM unset (set: every sub-cluster goes to the HBM kernel)
  bool use_quad = true;          // ... and SVDSS_POA_QUAD does not parse to 0 (0: no first stage, round 0 starts)
  bool quad_gw_set = false;      // SVDSS_POA_QUAD_GW: the group width of every sub-cluster of the first stage
  int quad_gw = 0;
  int64_t quad_short = 0;        // SVDSS_POA_QUAD_SHORT: reads up to this length share a wavefront four at a time
  int64_t quad_minwork_pct = 0;  // SVDSS_POA_QUAD_MINWORK: percent of the batch's largest reads x length below which the first stage is skipped
  int64_t quad_rows16 = 0, quad_rows32 = 0;   // SVDSS_POA_QUAD_ROWS16 / _ROWS32: reads x length up to which the group width is 16 / 32
  int nc_pct = 150;              // SVDSS_POA_NC: the first estimate of the graph, percent of the longest read (at least 100)
  bool noprio = false;           // SVDSS_POA_NOPRIO: no issue priority for the long chains
  bool no_mix = false;           // SVDSS_POA_NO_MIX: waves of launches are consecutive pieces of the sorted list
  int64_t ws_gb = 32;            // SVDSS_POA_WS_GB: workspace per wave of launches
  bool merge = true;             // SVDSS_POA_MERGE does not parse to 0 (0: every group of the first stage is a launch of its own, as before the merge)
  bool debug = false;            // SVDSS_DEBUG

  static PoaKnobs from_env() {
    PoaKnobs k;
    auto ll = [](const char* name, int64_t dflt) { const char* e = getenv(name); return e ? (int64_t)atoll(e) : dflt; };
    k.use_lds = getenv("SVDSS_POA_HBM") == nullptr;
    k.use_quad = k.use_lds && !(getenv("SVDSS_POA_QUAD") && atoi(getenv("SVDSS_POA_QUAD")) == 0);
    k.quad_gw_set = getenv("SVDSS_POA_QUAD_GW") != nullptr;
    if (k.quad_gw_set) k.quad_gw = atoi(getenv("SVDSS_POA_QUAD_GW"));
    k.quad_short = ll("SVDSS_POA_QUAD_SHORT", 0);
    k.quad_minwork_pct = ll("SVDSS_POA_QUAD_MINWORK", 0);
    k.quad_rows16 = ll("SVDSS_POA_QUAD_ROWS16", 0);
    k.quad_rows32 = ll("SVDSS_POA_QUAD_ROWS32", 0);
    if (getenv("SVDSS_POA_NC")) k.nc_pct = std::max(atoi(getenv("SVDSS_POA_NC")), 100);
    k.noprio = getenv("SVDSS_POA_NOPRIO") != nullptr;
    k.no_mix = getenv("SVDSS_POA_NO_MIX") != nullptr;
    k.ws_gb = ll("SVDSS_POA_WS_GB", 0) > 0 ? ll("SVDSS_POA_WS_GB", 0) : 32;
    k.merge = !(getenv("SVDSS_POA_MERGE") && atoi(getenv("SVDSS_POA_MERGE")) == 0);
    k.debug = getenv("SVDSS_DEBUG") != nullptr;
    return k;
  }
};

// bytes of workspace per wave of launches (default 32 GB: a whole genome's 21,500 sub-clusters want ~64 GB and run in two
// waves of ~75 ms; one wave needs an allocation that large on a device other processes have just left): at most half of
// what the device can give (free memory plus what the batch object already holds), at least 1 GB
inline size_t poa_ws_budget(const PoaKnobs& k, bool have_mem_info, size_t free_bytes, size_t arena_cap) {
  size_t budget = (size_t)k.ws_gb << 30;
  if (have_mem_info) budget = std::min(budget, (free_bytes + arena_cap) / 2);
  return std::max(budget, (size_t)1 << 30);
}

// ---------------------------------------------------------------------------------------------------------------- sizes
constexpr int kPoaRounds = 3;                         // of poa_wave.hip
constexpr size_t kPoaLdsMax = 160 * 1024 - 512;       // LDS a launch may ask for
constexpr int64_t kPoaGroupBudget32 = (int64_t)2 << 30;   // ints of workspace per launch of the LDS kernels
constexpr int64_t kPoaHbmBudget32 = (int64_t)3 << 30;     // ... of the HBM kernel (12 GiB)
// columns per lane poa_wave.hip is instantiated for
static const int kPoaWaveCols[4] = {1, 2, 3, 5};
static const int kPoaWaveNCols = 4;
// (group width, columns per lane) poa_quad.hip is instantiated for
static const int kPoaQuadVariants[10][2] = {{16, 3}, {16, 4}, {16, 5}, {16, 6}, {16, 7}, {32, 2}, {32, 3}, {32, 4}, {64, 1}, {64, 2}};
static const int kPoaQuadNVariants = 10;

// DevArena::padded (dev_arena.h), which poa.hip checks this against: what a take() of `bytes` costs at most
constexpr size_t poa_padded(size_t bytes) { return ((bytes + 255) & ~(size_t)255) + 256; }

// the int32 workspace of one sub-cluster of the LDS kernels (offsets in ints)
struct WsLayout {
  int64_t out_head, in_head, order, index, col, base;
  int64_t row_beg, row_end, hl, prow0, prow1, row_mpl, row_mpr;
  int64_t aln, scr, rinfo, keepf;
  int64_t e_from, e_to, e_w, e_next_out, e_next_in;
  int64_t op_node, op_q, path_use, path_aux;
  int64_t gdir, gH, gE1, gE2;
  int64_t total;
};

POA_HD inline WsLayout ws_layout(int nc, int ec, int max_len, int ws) {
  WsLayout w;
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t at = o; o += n; return at; };
  w.out_head = take(nc); w.in_head = take(nc); w.order = take(nc); w.index = take(nc); w.col = take(nc); w.base = take(nc);
  w.row_beg = take(nc); w.row_end = take(nc); w.hl = take(nc); w.prow0 = take(nc); w.prow1 = take(nc);
  w.row_mpl = take(nc); w.row_mpr = take(nc);
  w.aln = take(5 * (int64_t)nc);
  w.scr = take((int64_t)nc + 64);
  w.rinfo = take((int64_t)nc + 64); w.keepf = take((int64_t)nc + 64);
  w.e_from = take(ec); w.e_to = take(ec); w.e_w = take(ec); w.e_next_out = take(ec); w.e_next_in = take(ec);
  const int64_t opcap = (int64_t)nc + max_len + 4;
  w.op_node = take(opcap); w.op_q = take(opcap); w.path_use = take(opcap); w.path_aux = take(opcap);
  const int64_t pool = (int64_t)nc * ws;
  w.gdir = take(pool); w.gH = take(pool); w.gE1 = take(pool); w.gE2 = take(pool);
  w.total = o;
  return w;
}

inline int64_t poa_wave_ws_ints(int nc, int ec, int max_len, int ws) { return ws_layout(nc, ec, max_len, ws).total; }

inline size_t poa_wave_lds_bytes(int nc, int max_len, int rs, int ring) {
  (void)nc;
  const size_t ns = (size_t)ring + 2;
  return 12 * ns * ((size_t)rs + 8) + 16 * ns + 64 + (((size_t)max_len + 15) & ~(size_t)15) + 64 + 256;
}

inline size_t poa_bundle_lds_bytes(int nc) { return 12 * (size_t)nc + 64; }

inline bool poa_quad_supported(int gw, int cols) {
  for (int k = 0; k < kPoaQuadNVariants; ++k)
    if (kPoaQuadVariants[k][0] == gw && kPoaQuadVariants[k][1] == cols) return true;
  return false;
}

// max_len: the longest read of the launch (every group keeps the read being aligned in LDS)
inline size_t poa_quad_lds_bytes(int gw, int cols, int max_len) {
  const size_t rw = (size_t)(gw * cols + 2 * PQ_GD), g = (size_t)(64 / gw);
  return sizeof(int32_t) * (g * PQ_RING * 3 * rw + 3 * rw + 16) + g * (size_t)(((max_len + gw * cols + 24 + 15) & ~15));
}

// the band of the specification for reads of this length
inline int64_t poa_w_band(int64_t max_len) { return 10 + (int64_t)(0.01 * (double)max_len); }

// ----------------------------------------------------------------------------------------------------- the plan of a round
struct PoaShape { int64_t n, tot, maxl; };   // reads, their total and their greatest length

inline PoaShape poa_cluster_shape(const int64_t* seq_off, const int64_t* cluster_off, int64_t c) {
  PoaShape s{cluster_off[c + 1] - cluster_off[c], 0, 0};
  for (int64_t i = cluster_off[c]; i < cluster_off[c + 1]; ++i) {
    const int64_t l = seq_off[i + 1] - seq_off[i];
    s.tot += l;
    if (l > s.maxl) s.maxl = l;
  }
  return s;
}

struct PoaBatchIn {
  const int64_t *seq_off = nullptr, *cluster_off = nullptr;
  int64_t n_clusters = 0;
  PoaKnobs knobs;
  int n_cus = 256;
  size_t ws_budget = (size_t)32 << 30;
  int64_t max_work = 1;   // the batch's largest reads x length
  void set_max_work() {
    max_work = 1;
    for (int64_t c = 0; c < n_clusters; ++c) {
      const PoaShape s = poa_cluster_shape(seq_off, cluster_off, c);
      max_work = std::max(max_work, s.n * s.maxl);
    }
  }
};

struct PoaCand { int64_t c; size_t lds; int cols; int gw; int64_t width; PoaWaveTask t; };   // width: the widest row the stage has to hold
enum PoaWhere { POA_RUN, POA_NEXT, POA_HBM };   // this round / sent on to the next round / sent on to the HBM kernel

// One sub-cluster in one round.  skip_round0: see poa_plan_round; no_wider is written in round -1.
inline PoaWhere poa_size_cluster(const PoaBatchIn& in, int round, int64_t c, bool skip_round0, PoaCand& cd, uint8_t& no_wider) {
  const PoaKnobs& k = in.knobs;
  const PoaShape s = poa_cluster_shape(in.seq_off, in.cluster_off, c);
  const int64_t maxl = s.maxl;
  PoaWaveTask t;
  memset(&t, 0, sizeof t);
  t.seq_first = in.cluster_off[c];
  t.n_seqs = s.n;
  // the graph rarely grows beyond ~1.5 x the longest read (later rounds: 3 x); a cluster that outgrows its
  // allocation is redone.  SVDSS_POA_NC scales the first estimate (percent).
  const int nc_pct = round > 0 ? 300 : k.nc_pct;
  int64_t nc = std::min<int64_t>(s.tot + 2, maxl * nc_pct / 100 + 8 * t.n_seqs + 64);
  if (nc > 65000) nc = 65000;
  const int64_t ecap = std::min<int64_t>(nc + nc / (round > 0 ? 2 : 4) + t.n_seqs + 64, 100000);
  // widest row the ring holds: the band as it is in practice (round 0), as wide as the specification lets it
  // get (round 1), the full matrix (round 2, after the band lost the sink)
  // (round 0: 2w + 1 columns plus slack for the spread of the predecessors' maxima -- rounded up to 64 where that
  // leaves at least 8 of slack, so that a row is one column per lane: the C = 1 instantiation)
  const int64_t w_band = poa_w_band(maxl), w2 = 2 * w_band + 1;
  const int64_t wcap0 = w2 + 8 <= 64 ? 64 : w2 + 32;
  const int64_t wcap = std::min<int64_t>(round <= 0 ? wcap0 : round == 1 ? 2 * w_band + 129 : maxl + 1, maxl + 1);
  t.nc = (int32_t)nc; t.ec = (int32_t)ecap; t.max_len = (int32_t)maxl;
  if (round < 0) {
    // group width x columns per lane >= 2w + 1 columns plus 8 of slack for the spread of the predecessors' maxima
    // Group width: four short sub-clusters share a wavefront (a quarter of the wavefront slots for the latency-bound
    // traceback / graph-update phases); a long one gets the wavefront to itself -- the longest chains of a batch
    // decide when it ends, and a row of C = 2 columns per lane is the quickest there is.
    // (quad_rows16 / quad_rows32: a sub-cluster of at most that many reads x length shares its wavefront with three /
    // one other: its chain is short enough not to become the batch's tail at the slower lock-step pace)
    const int64_t chain = t.n_seqs * maxl;
    const int gw = k.quad_gw_set ? k.quad_gw : (maxl <= k.quad_short || chain <= k.quad_rows16) ? 16 : chain <= k.quad_rows32 ? 32 : 64;
    // quad_minwork_pct: only the long chains take this stage
    if (chain * 100 < k.quad_minwork_pct * in.max_work) return POA_NEXT;
    if (gw != 16 && gw != 32 && gw != 64) return POA_NEXT;
    const int64_t need = std::min<int64_t>(w2 + 8, maxl + 1);
    const int qc = (int)std::max<int64_t>((need + gw - 1) / gw, gw == 16 ? 3 : gw == 32 ? 2 : 1);
    if (!poa_quad_supported(gw, qc) || t.n_seqs <= 0 || t.n_seqs > 8191 || poa_bundle_lds_bytes((int)nc) > kPoaLdsMax ||
        poa_quad_lds_bytes(gw, qc, (int)maxl) > kPoaLdsMax)
      return POA_NEXT;
    t.ws = gw * qc; t.rs = 0; t.ring = 0;
    no_wider = wcap0 <= (int64_t)gw * qc ? 1 : 0;
    cd = PoaCand{c, poa_quad_lds_bytes(gw, qc, (int)maxl), qc, gw, need, t};
    return POA_RUN;
  }
  if (round == 0 && skip_round0 && kPoaRounds > 1) return POA_NEXT;
  int64_t ws = 64;
  while (ws < wcap) ws <<= 1;
  t.ws = (int32_t)ws; t.rs = (int32_t)((wcap + 3) & ~(int64_t)3); t.ring = 4;
  const size_t lds = poa_wave_lds_bytes(t.nc, t.max_len, t.rs, t.ring);
  cd = PoaCand{c, lds, wcap <= 64 ? 1 : wcap <= 128 ? 2 : wcap <= 192 ? 3 : 5, 0, wcap, t};
  const bool fits = lds <= kPoaLdsMax && poa_bundle_lds_bytes(t.nc) <= kPoaLdsMax && ws <= 4096 && t.n_seqs > 0 && t.n_seqs <= 8191;
  return k.use_lds && fits ? POA_RUN : POA_HBM;
}

// one launch: sub-clusters of one instantiation and LDS class
struct PoaGroup {
  int cols = 0, gw = 0, max_len = 0;   // gw != 0: a launch of poa_quad.hip
  int wave = 0;                        // groups of different `wave` never share a wave of launches
  size_t lds = 0, bundle_lds = 0;
  std::vector<PoaWaveTask> tasks;
  std::vector<int64_t> ids;
  int64_t w32 = 0, w8 = 0;             // ints / bytes of workspace
  size_t bytes() const {
    const size_t nt = tasks.size();
    return poa_padded(sizeof(PoaWaveTask) * nt) + poa_padded(sizeof(int32_t) * (size_t)w32) + poa_padded((size_t)w8) +
           2 * poa_padded(sizeof(int32_t) * nt);
  }
  void add(const PoaCand& cd, int64_t need) {
    PoaWaveTask t = cd.t;
    max_len = std::max(max_len, (int)t.max_len);
    t.ws_off = w32; w32 += need;
    t.cons_off = w8; w8 += t.nc;
    bundle_lds = std::max(bundle_lds, poa_bundle_lds_bytes(t.nc));
    tasks.push_back(t);
    ids.push_back(cd.c);
  }
};

inline int64_t poa_chain(const PoaCand& cd) { return cd.t.n_seqs * (int64_t)cd.t.max_len; }

// a sub-cluster is one chain of n_seqs x length dependent row steps: the longest chains of the batch decide
// when it ends, so they get the issue priority (s_setprio) over the short ones that fill the CUs beside them
inline void poa_set_prio(std::vector<PoaCand>& cands) {
  int64_t wmax = 1;
  for (const PoaCand& cd : cands) wmax = std::max(wmax, poa_chain(cd));
  for (PoaCand& cd : cands) {
    const int64_t wk = poa_chain(cd);
    cd.t.prio = wk * 2 > wmax ? 3 : wk * 4 > wmax ? 2 : wk * 8 > wmax ? 1 : 0;
  }
}

// First stage: wavefronts of sub-clusters that are alike (the groups of a wavefront walk in lock-step: it lasts as long as
// its longest), the longest first; one launch per variant.
// A batch beyond the workspace budget (a whole genome's sub-clusters at once) runs in several waves of launches, and
// every wave lasts at least as long as its longest chain: the sub-clusters are dealt to the waves longest first, one
// each in turn, so that every wave has its share of long chains and of short ones to fill the machine beside them
// (no_mix: consecutive pieces of the sorted list -- the first wave all long chains, the last all short).
inline void poa_pack_quad(const PoaBatchIn& in, const std::vector<PoaCand>& cands, std::vector<PoaGroup>& groups) {
  std::vector<int> wave_of(cands.size(), 0);
  size_t total = 0;
  for (const PoaCand& cd : cands) total += sizeof(int32_t) * (size_t)poa_wave_ws_ints(cd.t.nc, cd.t.ec, cd.t.max_len, cd.t.ws) + (size_t)cd.t.nc + 256;
  const size_t per_wave = in.ws_budget - in.ws_budget / 8;
  const size_t n_waves = std::max<size_t>(1, (total + per_wave - 1) / per_wave);
  if (n_waves > 1 && !in.knobs.no_mix) {
    std::vector<size_t> by_work(cands.size());
    for (size_t i = 0; i < by_work.size(); ++i) by_work[i] = i;
    std::sort(by_work.begin(), by_work.end(), [&](size_t x, size_t y) {
      const int64_t wx = poa_chain(cands[x]), wy = poa_chain(cands[y]);
      return wx != wy ? wx > wy : cands[x].c < cands[y].c;
    });
    for (size_t k = 0; k < by_work.size(); ++k) wave_of[by_work[k]] = (int)(k % n_waves);
  }
  std::vector<size_t> order(cands.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t xi, size_t yi) {
    const PoaCand &x = cands[xi], &y = cands[yi];
    if (wave_of[xi] != wave_of[yi]) return wave_of[xi] < wave_of[yi];
    if (x.gw != y.gw) return x.gw > y.gw;
    if (x.cols != y.cols) return x.cols > y.cols;
    const int64_t wx = poa_chain(x), wy = poa_chain(y);
    if (wx != wy) return wx > wy;
    return x.c < y.c;
  });
  PoaGroup* g = nullptr;
  for (size_t oi : order) {
    const PoaCand& cd = cands[oi];
    const int64_t need = poa_wave_ws_ints(cd.t.nc, cd.t.ec, cd.t.max_len, cd.t.ws);
    if (!g || g->wave != wave_of[oi] || g->gw != cd.gw || g->cols != cd.cols || g->w32 + need > kPoaGroupBudget32) {
      groups.emplace_back();
      g = &groups.back();
      g->cols = cd.cols; g->gw = cd.gw; g->lds = cd.lds; g->wave = wave_of[oi];
    }
    g->add(cd, need);
  }
}

// Rounds of poa_wave.hip: launches are grouped by instantiation and by LDS size class (cands: largest LDS first), so that
// small clusters are not charged the LDS of the largest one (LDS decides how many sub-clusters a CU keeps in flight)
inline void poa_pack_wave(const PoaBatchIn& in, const std::vector<PoaCand>& cands, std::vector<PoaGroup>& groups) {
  for (int ci = 0; ci < kPoaWaveNCols; ++ci) {
    PoaGroup* g = nullptr;
    size_t fill = 0;   // sub-clusters that fill the machine at the group's LDS size
    for (const PoaCand& cd : cands) {
      if (cd.cols != kPoaWaveCols[ci]) continue;
      const int64_t need = poa_wave_ws_ints(cd.t.nc, cd.t.ec, cd.t.max_len, cd.t.ws);
      // a new launch (with the smaller LDS of the clusters that follow) only once the current one fills all CUs
      if (!g || g->w32 + need > kPoaGroupBudget32 || g->tasks.size() >= fill) {
        groups.emplace_back();
        g = &groups.back();
        g->cols = kPoaWaveCols[ci];
        g->lds = cd.lds;
        fill = (size_t)in.n_cus * std::min<size_t>(32, std::max<size_t>(1, kPoaLdsMax / cd.lds));
      }
      g->add(cd, need);
    }
  }
}

struct PoaRoundPlan {
  std::vector<PoaGroup> groups;
  std::vector<int64_t> next, hbm;   // sent on without running: to the next round / to the HBM kernel
  std::vector<size_t> cuts;         // wave k of launches is groups [cuts[k], cuts[k + 1]): what fits the workspace budget
};

// The plan of one round for the sub-clusters `cur`.  A sub-cluster the first stage hands back because a row got wider than
// its lanes hold goes straight to the round that has wider rows when round 0's rows are no wider than the first stage's
// were (`call` at 30x: one such sub-cluster of 21,500 cost a round of 39 ms that could only fail the same way): round -1
// writes round0_no_wider, the collection of its statuses sets skip_round0, round 0 sends the marked ones on.
inline PoaRoundPlan poa_plan_round(const PoaBatchIn& in, int round, const std::vector<int64_t>& cur,
                                   const std::vector<uint8_t>& skip_round0, std::vector<uint8_t>& round0_no_wider) {
  PoaRoundPlan p;
  std::vector<PoaCand> cands;
  for (int64_t c : cur) {
    PoaCand cd;
    const PoaWhere where = poa_size_cluster(in, round, c, skip_round0[(size_t)c] != 0, cd, round0_no_wider[(size_t)c]);
    if (where == POA_RUN) cands.push_back(cd);
    else (where == POA_NEXT ? p.next : p.hbm).push_back(c);
  }
  std::sort(cands.begin(), cands.end(), [](const PoaCand& x, const PoaCand& y) { return x.lds > y.lds; });
  if (!in.knobs.noprio) poa_set_prio(cands);
  if (round < 0) poa_pack_quad(in, cands, p.groups);
  else poa_pack_wave(in, cands, p.groups);
  for (size_t gpos = 0; gpos < p.groups.size();) {
    p.cuts.push_back(gpos);
    size_t gend = gpos, tot_bytes = 0;
    while (gend < p.groups.size() && (gend == gpos || (p.groups[gend].wave == p.groups[gpos].wave && tot_bytes + p.groups[gend].bytes() <= in.ws_budget)))
      tot_bytes += p.groups[gend++].bytes();
    gpos = gend;
  }
  p.cuts.push_back(p.groups.size());
  return p;
}

// ------------------------------------------------------------------------------------------ the launches of a wave
// The plan stays one group per variant; what is merged is merged at launch time.  The two variants that give a long
// sub-cluster the wavefront to itself, (64, 2) and (64, 1), are one kernel with two bodies (poa_quad_pair_kernel): a launch
// costs a place in the stream's hardware queue, where it may wait behind another stream's kernel, and the second launch of a
// pair waited behind the first one's bundle kernel or beside it on another stream for nothing -- both fill the same CUs.
// c2 / c1: the wave's group of (64, 2) / (64, 1) sub-clusters, -1: none (a merged launch may have an empty half);
// single: any other group, a launch of its own.
struct PoaLaunch { int c2 = -1, c1 = -1, single = -1; };

inline bool poa_group_pairs(const PoaGroup& g) { return g.gw == 64 && (g.cols == 1 || g.cols == 2); }

// The launches of groups [g0, g1) of a plan, in the order of the groups (a merged launch where its first group stands).
// The k-th (64, 2) group of a wave pairs with the k-th (64, 1) group of the same wave.
inline std::vector<PoaLaunch> poa_merge_wave(const PoaKnobs& k, const std::vector<PoaGroup>& groups, size_t g0, size_t g1) {
  std::vector<PoaLaunch> out;
  std::vector<uint8_t> used(g1 > g0 ? g1 - g0 : 0, 0);
  for (size_t gi = g0; gi < g1; ++gi) {
    if (used[gi - g0]) continue;
    const PoaGroup& g = groups[gi];
    PoaLaunch L;
    if (!k.merge || !poa_group_pairs(g)) { L.single = (int)gi; out.push_back(L); continue; }
    (g.cols == 2 ? L.c2 : L.c1) = (int)gi;
    for (size_t gj = gi + 1; gj < g1; ++gj) {   // the first unused group of the other variant in the same wave
      const PoaGroup& h = groups[gj];
      if (used[gj - g0] || !poa_group_pairs(h) || h.cols == g.cols || h.wave != g.wave) continue;
      (h.cols == 2 ? L.c2 : L.c1) = (int)gj;
      used[gj - g0] = 1;
      break;
    }
    out.push_back(L);
  }
  return out;
}

// The tasks of a merged launch as ONE group: the C = 2 tasks first (blocks are dispatched in index order, and the long
// chains, which decide when the launch ends, are the C = 2 ones), then the C = 1 tasks with their workspace offsets moved
// behind the C = 2 group's.  n2: how many tasks are the first half's.  The int32 workspace of the two stays below 2^32
// ints (kPoaGroupBudget32 each), which the 32-bit offsets of the first stage need.
inline PoaGroup poa_merged_group(const PoaGroup* c2, const PoaGroup* c1, size_t& n2) {
  PoaGroup m;
  m.gw = 64; m.cols = 0;
  n2 = 0;
  if (c2) {
    m = *c2;
    m.cols = 0;
    n2 = c2->tasks.size();
  }
  if (c1) {
    if (!c2) m.wave = c1->wave;
    m.max_len = std::max(m.max_len, c1->max_len);
    m.lds = std::max(m.lds, c1->lds);
    m.bundle_lds = std::max(m.bundle_lds, c1->bundle_lds);
    for (size_t i = 0; i < c1->tasks.size(); ++i) {
      PoaWaveTask t = c1->tasks[i];
      t.ws_off += m.w32;
      t.cons_off += m.w8;
      m.tasks.push_back(t);
      m.ids.push_back(c1->ids[i]);
    }
    m.w32 += c1->w32;
    m.w8 += c1->w8;
  }
  return m;
}

// -------------------------------------------------------------------------------------------------- the HBM fallback
struct PoaHbmLaunch {
  std::vector<PoaTask> tasks;
  std::vector<int64_t> ids;
  int64_t w32 = 0, w64 = 0, w8 = 0;   // elements of the int32 / int64 / byte workspace
};

// One launch of the HBM kernel: the sub-clusters todo[pos...] that fit kPoaHbmBudget32 (at least one); returns where the
// next launch starts.  Pass 0: a DP pool of the widest band per graph node; pass 1: of the full matrix.
inline size_t poa_plan_hbm(const int64_t* seq_off, const int64_t* cluster_off, const std::vector<int64_t>& todo, size_t pos, int pass,
                           PoaHbmLaunch& L) {
  L = PoaHbmLaunch();
  for (; pos < todo.size(); ++pos) {
    const PoaShape s = poa_cluster_shape(seq_off, cluster_off, todo[pos]);
    PoaTask t;
    memset(&t, 0, sizeof t);
    t.seq_first = cluster_off[todo[pos]];
    t.n_seqs = s.n;
    t.cap_nodes = (int32_t)(s.tot + 2);
    t.cap_edges = (int32_t)(s.tot + t.n_seqs + 2);
    t.max_len = (int32_t)s.maxl;
    const int64_t wband = 2 * poa_w_band(s.maxl) + 129;
    t.pool_cap = (int64_t)t.cap_nodes * (pass == 0 && wband < s.maxl + 1 ? wband : s.maxl + 1);
    const int64_t ops = 2 * ((int64_t)t.cap_nodes + s.maxl + 4);
    const int64_t need32 = 17 * (int64_t)t.cap_nodes + 5 * (int64_t)t.cap_edges + 6 * t.pool_cap + ops;
    if (!L.tasks.empty() && L.w32 + need32 > kPoaHbmBudget32) break;
    t.node_off = L.w32; L.w32 += 17 * (int64_t)t.cap_nodes;
    t.edge_off = L.w32; L.w32 += 5 * (int64_t)t.cap_edges;
    t.dp_off = L.w32; L.w32 += 6 * t.pool_cap;
    t.op_off = L.w32; L.w32 += ops;
    t.row_off64 = L.w64; L.w64 += 2 * (int64_t)t.cap_nodes;
    t.base_off = L.w8; L.w8 += t.cap_nodes;
    t.cons_off = L.w8; L.w8 += t.cap_nodes;
    L.tasks.push_back(t);
    L.ids.push_back(todo[pos]);
  }
  return pos;
}
