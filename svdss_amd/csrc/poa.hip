// poa.hip -- gfx950 kernel + C-ABI for the partial-order-alignment consensus of `SVDSS call`.
//
// Replaces Caller::run_poa's abpoa_msa + consensus (/root/reference/caller.cpp:257-308, abPOA
// v1.5.3) for a batch of sub-clusters.  abPOA itself is not available (git-fetched), so the
// algorithm is the published one (POA with adaptive band, convex gap, heaviest-bundle consensus)
// under the deterministic specification written out in oracle/svdss_oracle_poa.c, which this
// kernel must reproduce bit for bit.
//
// Mapping: one wavefront per sub-cluster.  The reads of a cluster are aligned to the growing
// graph one after the other (inherently sequential); inside one alignment the rows (graph nodes
// in topological order) depend on their predecessors, but the columns of a row -- the band of
// ~2w+1 read positions -- are independent once the horizontal-gap state F is written as a
// prefix maximum, F(j) = max_{k<j}(H'(k) + k e) - o - j e, which is a wave-level scan.  So the 64
// lanes sweep the band; graph bookkeeping (topological sort, traceback, graph update, heaviest
// bundle) runs on lane 0.  Banded DP matrices, the graph and the traceback live in HBM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "call_streams.h"
#include "dev_arena.h"
#include "hip_check.h"
#include "poa_plan.h"
#include "poa_wave.h"
#include "poa_quad.h"

#define PNEG (-0x20000000)
#define P_O1 4
#define P_E1 2
#define P_O2 24
#define P_E2 1
#define P_MATCH 2
#define P_MISMATCH 4

struct PoaGraph {
  int n_nodes, n_edges, cap_nodes, cap_edges;
  uint8_t* base;
  int *out_head, *out_tail, *in_head, *in_tail, *order, *index, *deg, *best, *row_beg, *row_end, *mpl, *mpr, *aln;
  int *e_from, *e_to, *e_w, *e_next_out, *e_next_in;
  int64_t *row_off, *score;
};

__device__ __forceinline__ int p_score(int a, int b) { return (a >= 4 || b >= 4) ? 0 : (a == b ? P_MATCH : -P_MISMATCH); }

__device__ int g_new_node(PoaGraph& g, int base) {
  const int v = g.n_nodes++;
  g.base[v] = (uint8_t)base;
  g.out_head[v] = g.out_tail[v] = g.in_head[v] = g.in_tail[v] = -1;
  for (int b = 0; b < 5; ++b) g.aln[5 * v + b] = -1;
  return v;
}

__device__ void g_add_edge(PoaGraph& g, int u, int v) {
  for (int e = g.out_head[u]; e >= 0; e = g.e_next_out[e])
    if (g.e_to[e] == v) { g.e_w[e]++; return; }
  const int e = g.n_edges++;
  g.e_from[e] = u; g.e_to[e] = v; g.e_w[e] = 1;
  g.e_next_out[e] = -1; g.e_next_in[e] = -1;
  if (g.out_tail[u] < 0) g.out_head[u] = e; else g.e_next_out[g.out_tail[u]] = e;
  g.out_tail[u] = e;
  if (g.in_tail[v] < 0) g.in_head[v] = e; else g.e_next_in[g.in_tail[v]] = e;
  g.in_tail[v] = e;
}

__device__ void g_toposort(PoaGraph& g) {   // lane 0
  for (int v = 0; v < g.n_nodes; ++v) g.deg[v] = 0;
  for (int e = 0; e < g.n_edges; ++e) g.deg[g.e_to[e]]++;
  int qh = 0, qt = 0;
  g.order[qt++] = 0;
  while (qh < qt) {
    const int u = g.order[qh];
    g.index[u] = qh++;
    for (int e = g.out_head[u]; e >= 0; e = g.e_next_out[e])
      if (--g.deg[g.e_to[e]] == 0) g.order[qt++] = g.e_to[e];
  }
}

struct PoaDp { int32_t *H, *Hp, *E1, *E2, *F1, *F2; };

__device__ __forceinline__ int32_t dp_at(const int32_t* arr, const PoaGraph& g, int r, int j) {
  return (j < g.row_beg[r] || j > g.row_end[r]) ? PNEG : arr[g.row_off[r] + (j - g.row_beg[r])];
}

// wave-wide inclusive prefix maximum over the 64 lanes
__device__ __forceinline__ int32_t wave_scan_max(int32_t x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t y = __shfl_up(x, d, 64);
    if (lane >= d && y > x) x = y;
  }
  return x;
}

// Forward DP of one read against the graph (all 64 lanes).  Returns false if the DP arrays would
// overflow pool_cap.  *cells accumulates the number of DP cells.
__device__ bool poa_forward(PoaGraph& g, const PoaDp& dp, const uint8_t* q, int L, int w, int64_t pool_cap,
                            unsigned long long& cells) {
  const int lane = threadIdx.x & 63;
  const int n = g.n_nodes;
  int64_t used = 0;
  for (int r = 0; r < n; ++r) {
    const int v = g.order[r];
    if (v == 1) {
      if (lane == 0) { g.row_beg[r] = 0; g.row_end[r] = -1; g.row_off[r] = used; g.mpl[r] = 0; g.mpr[r] = 0; }
      __syncthreads();
      continue;
    }
    int beg, end;
    if (r == 0) { beg = 0; end = w < L ? w : L; }
    else {
      int lo = 1 << 30, hi = -1;
      for (int e = g.in_head[v]; e >= 0; e = g.e_next_in[e]) {
        const int ur = g.index[g.e_from[e]];
        const int a = g.mpl[ur], b = g.mpr[ur];
        if (a < lo) lo = a;
        if (b > hi) hi = b;
      }
      beg = lo + 1 - w; if (beg < 0) beg = 0;
      end = hi + 1 + w; if (end > L) end = L;
      if (end - beg + 1 > 2 * w + 129) end = beg + 2 * w + 128;
    }
    const int width = end - beg + 1;
    if (used + width > pool_cap) return false;   // uniform across lanes
    if (lane == 0) { g.row_beg[r] = beg; g.row_end[r] = end; g.row_off[r] = used; }
    const int64_t off = used;
    used += width;
    int32_t best = PNEG; int mpl = beg, mpr = beg;
    int32_t g1 = PNEG, g2 = PNEG;   // running prefix maxima of H'(k) + k e over finished chunks
    for (int j0 = beg; j0 <= end; j0 += 64) {
      const int j = j0 + lane;
      const bool in = j <= end;
      int32_t m = PNEG, e1 = PNEG, e2 = PNEG;
      if (in) {
        if (r == 0) m = (j == 0) ? 0 : PNEG;
        else {
          const int bv = g.base[v];
          for (int e = g.in_head[v]; e >= 0; e = g.e_next_in[e]) {
            const int ur = g.index[g.e_from[e]];
            if (j >= 1) {
              const int32_t h = dp_at(dp.H, g, ur, j - 1);
              if (h > PNEG / 2) { const int32_t x = h + p_score(bv, q[j - 1]); if (x > m) m = x; }
            }
            const int32_t h = dp_at(dp.H, g, ur, j);
            {
              const int32_t x = dp_at(dp.E1, g, ur, j);
              const int32_t a = h > PNEG / 2 ? h - P_O1 : PNEG, b = x > PNEG / 2 ? x : PNEG;
              int32_t c = a > b ? a : b;
              if (c > PNEG / 2) { c -= P_E1; if (c > e1) e1 = c; }
            }
            {
              const int32_t x = dp_at(dp.E2, g, ur, j);
              const int32_t a = h > PNEG / 2 ? h - P_O2 : PNEG, b = x > PNEG / 2 ? x : PNEG;
              int32_t c = a > b ? a : b;
              if (c > PNEG / 2) { c -= P_E2; if (c > e2) e2 = c; }
            }
          }
        }
      }
      int32_t hp = m; if (e1 > hp) hp = e1; if (e2 > hp) hp = e2;
      // F(j) = max_{k<j}(H'(k) + k e) - o - j e: exclusive prefix max = scan of the left neighbour
      const int32_t t1 = (in && hp > PNEG / 2) ? hp + j * P_E1 : PNEG;
      const int32_t t2 = (in && hp > PNEG / 2) ? hp + j * P_E2 : PNEG;
      const int32_t s1 = wave_scan_max(t1, lane), s2 = wave_scan_max(t2, lane);
      int32_t x1 = __shfl_up(s1, 1, 64), x2 = __shfl_up(s2, 1, 64);
      if (lane == 0) { x1 = PNEG; x2 = PNEG; }
      if (g1 > x1) x1 = g1;
      if (g2 > x2) x2 = g2;
      const int32_t f1 = x1 > PNEG / 2 ? x1 - P_O1 - j * P_E1 : PNEG;
      const int32_t f2 = x2 > PNEG / 2 ? x2 - P_O2 - j * P_E2 : PNEG;
      int32_t h = hp; if (f1 > h) h = f1; if (f2 > h) h = f2;
      if (in) {
        const int64_t o = off + (j - beg);
        dp.Hp[o] = hp; dp.E1[o] = e1; dp.E2[o] = e2; dp.F1[o] = f1; dp.F2[o] = f2; dp.H[o] = h;
      }
      // carry the chunk's maxima
      const int32_t c1 = __shfl(s1, 63, 64), c2 = __shfl(s2, 63, 64);
      if (c1 > g1) g1 = c1;
      if (c2 > g2) g2 = c2;
      // row maximum with its leftmost / rightmost column
      int32_t hm = in ? h : PNEG;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) { const int32_t y = __shfl_xor(hm, d, 64); if (y > hm) hm = y; }
      const unsigned long long eq = __ballot(in && h == hm);
      if (eq) {
        const int l = j0 + __builtin_ctzll(eq), rr = j0 + 63 - __builtin_clzll(eq);
        if (hm > best) { best = hm; mpl = l; mpr = rr; }
        else if (hm == best) mpr = rr;
      }
    }
    if (lane == 0) { g.mpl[r] = mpl; g.mpr[r] = mpr; }
    cells += (unsigned long long)width;
    __syncthreads();   // the row (and its geometry) is visible to every lane before its successors
  }
  return true;
}

// Traceback (lane 0): ops from the sink backwards, (node or -1, qpos or -1).  -1: sink unreachable.
__device__ int poa_traceback(const PoaGraph& g, const PoaDp& dp, const uint8_t* q, int L, int* op_node, int* op_q) {
  int bu = -1; int32_t bs = PNEG;
  for (int e = g.in_head[1]; e >= 0; e = g.e_next_in[e]) {
    const int32_t h = dp_at(dp.H, g, g.index[g.e_from[e]], L);
    if (h > bs) { bs = h; bu = g.e_from[e]; }
  }
  if (bu < 0 || bs <= PNEG / 2) return -1;
  int nops = 0, v = bu, j = L, state = 0;   // 0 H, 1 E1, 2 E2, 3 F1, 4 F2, 5 H' (no F)
  while (v != 0 || j > 0) {
    const int r = g.index[v];
    if (v == 0) { op_node[nops] = -1; op_q[nops] = j - 1; ++nops; --j; continue; }
    if (state == 0 || state == 5) {
      const int32_t h = state == 0 ? dp_at(dp.H, g, r, j) : dp_at(dp.Hp, g, r, j);
      bool moved = false;
      if (j >= 1) {
        for (int e = g.in_head[v]; e >= 0 && !moved; e = g.e_next_in[e]) {
          const int u = g.e_from[e];
          const int32_t x = dp_at(dp.H, g, g.index[u], j - 1);
          if (x > PNEG / 2 && x + p_score(g.base[v], q[j - 1]) == h) {
            op_node[nops] = v; op_q[nops] = j - 1; ++nops; v = u; --j; state = 0; moved = true;
          }
        }
      }
      if (moved) continue;
      if (dp_at(dp.E1, g, r, j) == h) { state = 1; continue; }
      if (dp_at(dp.E2, g, r, j) == h) { state = 2; continue; }
      if (state == 0 && dp_at(dp.F1, g, r, j) == h) { state = 3; continue; }
      if (state == 0 && dp_at(dp.F2, g, r, j) == h) { state = 4; continue; }
      return -1;
    } else if (state == 1 || state == 2) {
      const int32_t* E = state == 1 ? dp.E1 : dp.E2;
      const int o = state == 1 ? P_O1 : P_O2, ee = state == 1 ? P_E1 : P_E2;
      const int32_t x = dp_at(E, g, r, j);
      bool moved = false;
      for (int e = g.in_head[v]; e >= 0 && !moved; e = g.e_next_in[e]) {
        const int u = g.e_from[e];
        const int32_t h = dp_at(dp.H, g, g.index[u], j);
        if (h > PNEG / 2 && h - o - ee == x) { op_node[nops] = v; op_q[nops] = -1; ++nops; v = u; state = 0; moved = true; }
      }
      for (int e = g.in_head[v]; e >= 0 && !moved; e = g.e_next_in[e]) {
        const int u = g.e_from[e];
        const int32_t y = dp_at(E, g, g.index[u], j);
        if (y > PNEG / 2 && y - ee == x) { op_node[nops] = v; op_q[nops] = -1; ++nops; v = u; moved = true; }
      }
      if (!moved) return -1;
    } else {
      const int32_t* F = state == 3 ? dp.F1 : dp.F2;
      const int o = state == 3 ? P_O1 : P_O2, ee = state == 3 ? P_E1 : P_E2;
      const int32_t x = dp_at(F, g, r, j);
      op_node[nops] = -1; op_q[nops] = j - 1; ++nops;
      const int32_t hp = dp_at(dp.Hp, g, r, j - 1);
      if (hp > PNEG / 2 && hp - o - ee == x) state = 5;
      --j;
    }
  }
  return nops;
}

// status per cluster: 0 ok, 1 workspace too small (host retries with a larger DP pool)
__global__ void __launch_bounds__(64) poa_consensus_kernel(const PoaTask* tasks, const uint8_t* seqs, const int64_t* seq_off,
                                                          int32_t* ws32, int64_t* ws64, uint8_t* ws8,
                                                          int32_t* cons_len, int32_t* status, unsigned long long* cells) {
  const PoaTask T = tasks[blockIdx.x];
  const int lane = threadIdx.x;
  __shared__ int sh_flag;
  PoaGraph g;
  g.cap_nodes = T.cap_nodes; g.cap_edges = T.cap_edges; g.n_nodes = 0; g.n_edges = 0;
  int32_t* nb = ws32 + T.node_off;
  const int64_t cn = T.cap_nodes, ce = T.cap_edges;
  g.out_head = nb; g.out_tail = nb + cn; g.in_head = nb + 2 * cn; g.in_tail = nb + 3 * cn;
  g.order = nb + 4 * cn; g.index = nb + 5 * cn; g.deg = nb + 6 * cn; g.best = nb + 7 * cn;
  g.row_beg = nb + 8 * cn; g.row_end = nb + 9 * cn; g.mpl = nb + 10 * cn; g.mpr = nb + 11 * cn; g.aln = nb + 12 * cn;
  int32_t* eb = ws32 + T.edge_off;
  g.e_from = eb; g.e_to = eb + ce; g.e_w = eb + 2 * ce; g.e_next_out = eb + 3 * ce; g.e_next_in = eb + 4 * ce;
  g.row_off = ws64 + T.row_off64; g.score = ws64 + T.row_off64 + cn;
  g.base = ws8 + T.base_off;
  PoaDp dp;
  int32_t* db = ws32 + T.dp_off;
  dp.H = db; dp.Hp = db + T.pool_cap; dp.E1 = db + 2 * T.pool_cap; dp.E2 = db + 3 * T.pool_cap;
  dp.F1 = db + 4 * T.pool_cap; dp.F2 = db + 5 * T.pool_cap;
  int* op_node = ws32 + T.op_off;
  int* op_q = op_node + (T.cap_nodes + T.max_len + 4);
  uint8_t* cons = ws8 + T.cons_off;
  const int n = (int)T.n_seqs;
  if (n <= 0) { if (lane == 0) { cons_len[blockIdx.x] = 0; status[blockIdx.x] = 0; } return; }
  // all lanes track n_nodes / n_edges (they are needed for uniform control flow): lane 0 mutates
  // the graph in memory, then broadcasts the counters through LDS
  __shared__ int sh_nodes, sh_edges;
  unsigned long long my_cells = 0;
  if (lane == 0) {
    g_new_node(g, 4); g_new_node(g, 4);
    const uint8_t* q = seqs + seq_off[T.seq_first];
    const int L = (int)(seq_off[T.seq_first + 1] - seq_off[T.seq_first]);
    int last = 0;
    for (int j = 0; j < L; ++j) { const int v = g_new_node(g, q[j]); g.aln[5 * v + q[j]] = v; g_add_edge(g, last, v); last = v; }
    g_add_edge(g, last, 1);
    sh_nodes = g.n_nodes; sh_edges = g.n_edges;
  }
  __syncthreads();
  g.n_nodes = sh_nodes; g.n_edges = sh_edges;
  for (int i = 1; i < n; ++i) {
    const uint8_t* q = seqs + seq_off[T.seq_first + i];
    const int L = (int)(seq_off[T.seq_first + i + 1] - seq_off[T.seq_first + i]);
    if (lane == 0) g_toposort(g);
    __syncthreads();
    int w = 10 + (int)(0.01 * L);
    int nops = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
      const bool fit = poa_forward(g, dp, q, L, w, T.pool_cap, my_cells);
      if (!fit) { if (lane == 0) status[blockIdx.x] = 1; return; }
      if (lane == 0) sh_flag = poa_traceback(g, dp, q, L, op_node, op_q);
      __syncthreads();
      nops = sh_flag;
      __syncthreads();
      if (nops >= 0) break;
      w = L;   // the band lost the sink: full matrix
    }
    if (nops < 0) { if (lane == 0) status[blockIdx.x] = 2; return; }
    if (lane == 0) {
      int last = 0;
      for (int k = nops - 1; k >= 0; --k) {
        const int v = op_node[k], j = op_q[k];
        if (v >= 0 && j >= 0) {
          int use;
          if (g.base[v] == q[j]) use = v;
          else if (g.aln[5 * v + q[j]] >= 0) use = g.aln[5 * v + q[j]];
          else {
            use = g_new_node(g, q[j]);
            for (int b = 0; b < 5; ++b) {
              const int sib = g.aln[5 * v + b];
              g.aln[5 * use + b] = sib;
              if (sib >= 0) g.aln[5 * sib + q[j]] = use;
            }
            g.aln[5 * use + q[j]] = use;
          }
          g_add_edge(g, last, use); last = use;
        } else if (v < 0) {
          const int use = g_new_node(g, q[j]);
          g.aln[5 * use + q[j]] = use;
          g_add_edge(g, last, use); last = use;
        }
      }
      g_add_edge(g, last, 1);
      sh_nodes = g.n_nodes; sh_edges = g.n_edges;
    }
    __syncthreads();
    g.n_nodes = sh_nodes; g.n_edges = sh_edges;
  }
  if (lane == 0) {
    g_toposort(g);
    for (int r = g.n_nodes - 1; r >= 0; --r) {
      const int v = g.order[r];
      int bst = -1, bw = -1; int64_t bsc = -1;
      for (int e = g.out_head[v]; e >= 0; e = g.e_next_out[e]) {
        const int x = g.e_to[e];
        if (g.e_w[e] > bw || (g.e_w[e] == bw && g.score[x] > bsc)) { bw = g.e_w[e]; bsc = g.score[x]; bst = x; }
      }
      g.best[v] = bst;
      g.score[v] = bst >= 0 ? bw + bsc : 0;
    }
    int len = 0;
    for (int v = g.best[0]; v >= 0 && v != 1; v = g.best[v]) cons[len++] = g.base[v];
    cons_len[blockIdx.x] = len;
    status[blockIdx.x] = 0;
    atomicAdd(cells, my_cells);
  }
}

// ------------------------------------------------------------------- ABI

struct svdss_poa_batch {
  int64_t n_clusters = 0;
  int64_t n_hbm = 0;   // clusters the LDS kernel handed to the HBM kernel
  int64_t n_quad_back = 0;   // clusters poa_quad.hip handed to poa_wave.hip's rounds
  int64_t cells = 0;
  double kernel_ms = 0.0;
  std::vector<int64_t> cons_len;
  std::vector<uint8_t> cons;   // concatenated, symbols 0..4
  // device state kept between calls
  int device = -1;
  DevArena in_arena, ws_arena;
};

static_assert(poa_padded(0) == DevArena::padded(0) && poa_padded(1001) == DevArena::padded(1001), "poa_plan.h sizes what ws_arena hands out");

namespace {
struct EventPair {   // around the HBM kernel (created by fallback(), the only user)
  hipEvent_t a = nullptr, b = nullptr;
  int create() {
    if (!a) HIPCHK(hipEventCreate(&a));
    if (!b) HIPCHK(hipEventCreate(&b));
    return SVDSS_OK;
  }
  ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// One call of svdss_poa_consensus_batch: the members are what a stage hands to the next, the methods are the stages --
// upload, rounds (per round: the plan of poa_plan.h, then per wave of launches run_wave and collect), fallback, gather.
struct PoaBatchRun {
  svdss_poa_batch& b;
  const uint8_t* seqs;
  PoaBatchIn in;                                        // the lengths, the knobs (read here, once), CUs and workspace budget
  void *d_seqs = nullptr, *d_off = nullptr, *d_cells = nullptr;
  CallStreamLease lease;                                // the call's one stream, s0: every copy, launch and wait goes to it
  hipStream_t s0 = nullptr;
  EventPair ev;
  std::vector<std::vector<uint8_t>> results;            // the consensus of every sub-cluster that is done
  std::vector<int64_t> todo;                            // sub-clusters for the HBM kernel
  std::vector<uint8_t> round0_no_wider, skip_round0;    // poa_plan_round
  struct Mem { void *tasks, *w32, *w64, *w8, *len, *st; };   // a launch's share of ws_arena

  PoaBatchRun(svdss_poa_batch& batch, const uint8_t* s, const int64_t* seq_off, const int64_t* cluster_off, int64_t n_clusters)
      : b(batch), seqs(s), results((size_t)n_clusters), round0_no_wider((size_t)n_clusters, 0), skip_round0((size_t)n_clusters, 0) {
    in.seq_off = seq_off; in.cluster_off = cluster_off; in.n_clusters = n_clusters;
    in.knobs = PoaKnobs::from_env();
  }

  // ---- stage 1: the lengths checked, the reads on the device, the device sized up
  int upload(int32_t device) {
    const int64_t n_seqs_total = in.cluster_off[in.n_clusters];
    const int64_t total_syms = in.seq_off[n_seqs_total];
    for (int64_t i = 0; i < n_seqs_total; ++i) {
      const int64_t l = in.seq_off[i + 1] - in.seq_off[i];
      if (l < 0) return SVDSS_EINVAL;
      if (l >= (1 << 24)) return SVDSS_ERANGE;
    }
    if (total_syms > 0 && !seqs) return SVDSS_EINVAL;
    if (b.device != device) {   // (a batch object is normally used with one device)
      b.in_arena.drop(); b.ws_arena.drop();
      b.device = device;
    }
    const size_t off_bytes = sizeof(int64_t) * (size_t)(n_seqs_total + 1);
    HIPCHK(b.in_arena.reserve(DevArena::padded((size_t)total_syms) + DevArena::padded(off_bytes) + DevArena::padded(8)));
    d_seqs = b.in_arena.take((size_t)total_syms); d_off = b.in_arena.take(off_bytes); d_cells = b.in_arena.take(8);
    // every copy and launch of this call goes to ONE non-blocking stream of the call side's pool (call_streams.h) and
    // every wait is a wait for that stream: calls of different threads and a search running beside them overlap, and
    // the process has as few streams as that takes (the runtime multiplexes streams onto a handful of hardware queues,
    // and streams that share one run in order)
    HIPCHK(lease.acquire(device));
    s0 = lease.get();
    if (total_syms) HIPCHK(hipMemcpyAsync(d_seqs, seqs, (size_t)total_syms, hipMemcpyHostToDevice, s0));
    HIPCHK(hipMemcpyAsync(d_off, in.seq_off, off_bytes, hipMemcpyHostToDevice, s0));
    HIPCHK(hipMemsetAsync(d_cells, 0, 8, s0));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) in.n_cus = prop.multiProcessorCount;
    size_t free_b = 0, total_b = 0;
    const bool have = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    in.ws_budget = poa_ws_budget(in.knobs, have, free_b, b.ws_arena.cap);
    in.set_max_work();
    return SVDSS_OK;
  }

  bool empty(int64_t c) const { return in.cluster_off[c + 1] == in.cluster_off[c]; }

  Mem take(size_t task_bytes, size_t nt, int64_t w32, int64_t w64, int64_t w8) {
    Mem m;
    m.tasks = b.ws_arena.take(task_bytes * nt);
    m.w32 = b.ws_arena.take(sizeof(int32_t) * (size_t)w32);
    m.w64 = w64 ? b.ws_arena.take(sizeof(int64_t) * (size_t)w64) : nullptr;
    m.w8 = b.ws_arena.take((size_t)w8);
    m.len = b.ws_arena.take(sizeof(int32_t) * nt);
    m.st = b.ws_arena.take(sizeof(int32_t) * nt);
    return m;
  }

  // ---- stage 2: round -1 (poa_quad.hip; whatever it hands back starts round 0), then the rounds of poa_wave.hip
  int rounds() {
    std::vector<int64_t> cur((size_t)in.n_clusters), next;
    for (int64_t c = 0; c < in.n_clusters; ++c) cur[(size_t)c] = c;
    for (int round = in.knobs.use_quad ? -1 : 0; round < kPoaRounds && !cur.empty(); ++round) {
      const PoaRoundPlan p = poa_plan_round(in, round, cur, skip_round0, round0_no_wider);
      next = p.next;
      for (int64_t c : p.hbm) { todo.push_back(c); if (!empty(c)) ++b.n_hbm; }
      for (size_t w = 0; w + 1 < p.cuts.size(); ++w)
        if (const int rc = run_wave(round, p, p.cuts[w], p.cuts[w + 1], next)) return rc;
      cur.swap(next);
      if (round < 0) std::sort(cur.begin(), cur.end());
    }
    std::sort(todo.begin(), todo.end());
    return SVDSS_OK;
  }

  // one wave of launches, groups [g0, g1) of the plan.  The first stage's two whole-wavefront variants are ONE launch
  // (poa_merge_wave), and a wave of one launch -- every wave of a batch that finishes in the first stage -- is queued behind
  // its task upload on the call's stream with no host wait in between.  A wave that still has several launches runs them
  // side by side (one sub-cluster is a chain of dependent steps: the machine is filled by running many of them, whichever
  // launch they came from) on streams borrowed from the pool for as long as the wave lasts.
  int run_wave(int round, const PoaRoundPlan& p, size_t g0, size_t g1, std::vector<int64_t>& next) {
    const bool quad = round < 0;
    size_t tot_bytes = 0;
    for (size_t gi = g0; gi < g1; ++gi) tot_bytes += p.groups[gi].bytes();
    const auto ta = std::chrono::steady_clock::now();
    HIPCHK(b.ws_arena.reserve(tot_bytes));
    const double as = std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
    if (in.knobs.debug && as > 0.005) fprintf(stderr, "[poa] workspace of %.1f GB taken in %.3f s\n", (double)tot_bytes / 1073741824.0, as);
    const std::vector<PoaLaunch> launches = poa_merge_wave(in.knobs, p.groups, g0, g1);
    struct Unit { const PoaGroup* g; PoaGroup merged; size_t n2 = 0; int max_len2 = 0, max_len1 = 0; bool pair = false; Mem m; };
    std::vector<Unit> units(launches.size());
    for (size_t k = 0; k < launches.size(); ++k) {
      const PoaLaunch& L = launches[k];
      Unit& u = units[k];
      if (L.single >= 0) u.g = &p.groups[(size_t)L.single];
      else {
        const PoaGroup *c2 = L.c2 >= 0 ? &p.groups[(size_t)L.c2] : nullptr, *c1 = L.c1 >= 0 ? &p.groups[(size_t)L.c1] : nullptr;
        u.pair = true;
        u.merged = poa_merged_group(c2, c1, u.n2);
        u.max_len2 = c2 ? c2->max_len : 0;
        u.max_len1 = c1 ? c1->max_len : 0;
      }
    }
    for (Unit& u : units) {   // (units no longer moves: the merged groups stay where they are)
      if (u.pair) u.g = &u.merged;
      const size_t nt = u.g->tasks.size();
      u.m = take(sizeof(PoaWaveTask), nt, u.g->w32, 0, u.g->w8);
      HIPCHK(hipMemcpyAsync(u.m.tasks, u.g->tasks.data(), sizeof(PoaWaveTask) * nt, hipMemcpyHostToDevice, s0));
      HIPCHK(hipMemsetAsync(u.m.st, 0xff, sizeof(int32_t) * nt, s0));
    }
    // side by side: up to five further streams, as many as there are further launches
    std::vector<CallStreamLease> side(units.empty() ? 0 : std::min<size_t>(units.size() - 1, 5));
    for (CallStreamLease& l : side) HIPCHK(l.acquire(b.device, true));
    if (!side.empty()) HIPCHK(hipStreamSynchronize(s0));   // (the other streams must not start before the uploads are there)
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < units.size(); ++k) {
      const Unit& u = units[k];
      const PoaGroup& g = *u.g;
      const Mem& m = u.m;
      const size_t si = k % (side.size() + 1);
      const hipStream_t gs = si ? side[si - 1].get() : s0;
      const PoaWaveTask* d_tasks = (const PoaWaveTask*)m.tasks;
      const int nt = (int)g.tasks.size();
      if (u.pair) {
        HIPCHK(poa_quad_pair_launch(d_tasks, (int)u.n2, nt - (int)u.n2, u.max_len2, u.max_len1, (const uint8_t*)d_seqs, (const int64_t*)d_off,
                                     (int32_t*)m.w32, (int32_t*)m.len, (int32_t*)m.st, (unsigned long long*)d_cells, gs));
        HIPCHK(poa_bundle_launch(d_tasks, nt, g.bundle_lds, (int32_t*)m.w32, (uint8_t*)m.w8, (int32_t*)m.len, (const int32_t*)m.st, gs));
        if (u.n2 && (size_t)nt > u.n2) { std::lock_guard<std::mutex> lock(call_stream_pool().mu); ++call_stream_pool().merged; }
      } else if (g.gw) {
        HIPCHK(poa_quad_launch(g.gw, g.cols, d_tasks, nt, g.max_len, (const uint8_t*)d_seqs, (const int64_t*)d_off, (int32_t*)m.w32,
                                (int32_t*)m.len, (int32_t*)m.st, (unsigned long long*)d_cells, gs));
        HIPCHK(poa_bundle_launch(d_tasks, nt, g.bundle_lds, (int32_t*)m.w32, (uint8_t*)m.w8, (int32_t*)m.len, (const int32_t*)m.st, gs));
      } else
        HIPCHK(poa_wave_launch(g.cols, d_tasks, nt, g.lds, g.bundle_lds, (const uint8_t*)d_seqs, (const int64_t*)d_off, (int32_t*)m.w32,
                                (uint8_t*)m.w8, (int32_t*)m.len, (int32_t*)m.st, (unsigned long long*)d_cells, gs));
    }
    for (CallStreamLease& l : side) HIPCHK(hipStreamSynchronize(l.get()));
    HIPCHK(hipStreamSynchronize(s0));   // (for kernel_ms: collect's copies would wait for the kernels all the same)
    side.clear();                       // the borrowed streams are back before collect
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    b.kernel_ms += ms;   // wall time of the launches
    int why[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t n_run = 0;
    for (const Unit& u : units) {
      n_run += (int64_t)u.g->tasks.size();
      if (const int rc = collect(round, u.g->tasks, u.g->ids, u.m, u.g->w8, next, why)) return rc;
    }
    if (in.knobs.debug) {
      if (quad) poa_quad_debug_report(); else poa_wave_debug_report();
      fprintf(stderr, "[poa] %s round %d: %lld clusters in %zu launches, %.3f ms, not done: first-read %d preds %d width %d band %d capacity %d other %d\n",
              quad ? "quad" : "wave", round, (long long)n_run, units.size(), ms, why[1], why[2], why[3], why[4], why[5], why[0] + why[6] + why[7]);
    }
    return SVDSS_OK;
  }

  // Lengths, statuses and consensus bytes of one launch: what is finished goes to `results`; every other status is routed
  // here and nowhere else.  stage: -1 the first stage, 0-2 the rounds of poa_wave.hip, 3 / 4 the passes of the HBM kernel.
  // LDS kernels: status 3 | reason << 8 (why[reason] counts them); HBM kernel: 1 the DP pool was too small, 2 no alignment.
  template <class Task>
  int collect(int stage, const std::vector<Task>& tasks, const std::vector<int64_t>& ids, const Mem& m, int64_t w8, std::vector<int64_t>& next, int* why) {
    const size_t nt = tasks.size();
    std::vector<int32_t> lens(nt), st(nt);
    std::vector<uint8_t> h8((size_t)w8);
    HIPCHK(hipMemcpyAsync(lens.data(), m.len, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipMemcpyAsync(st.data(), m.st, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, s0));
    if (w8) HIPCHK(hipMemcpyAsync(h8.data(), m.w8, (size_t)w8, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipStreamSynchronize(s0));
    for (size_t k = 0; k < nt; ++k) {
      const int64_t id = ids[k];
      if (st[k] == 0) {
        const uint8_t* src = h8.data() + tasks[k].cons_off;
        results[(size_t)id].assign(src, src + lens[k]);
        continue;
      }
      const int reason = (st[k] >> 8) & 7;
      ++why[reason];
      if (stage < 0) {   // the first stage hands back: to round 0, or past it where round 0's rows are no wider (reason 3: width)
        next.push_back(id);
        ++b.n_quad_back;
        if (reason == 3 && round0_no_wider[(size_t)id]) skip_round0[(size_t)id] = 1;
      } else if (stage + 1 < kPoaRounds && (reason == 3 || reason == 4 || reason == 5)) next.push_back(id);   // width, band, capacity: the next round is roomier
      else if (stage < kPoaRounds) { todo.push_back(id); ++b.n_hbm; }
      else if (stage == kPoaRounds && st[k] == 1) next.push_back(id);   // pass 1 has the full-size DP pool
      else return SVDSS_ERANGE;   // internal inconsistency
    }
    return SVDSS_OK;
  }

  // ---- stage 3: what the LDS kernels left, on the HBM kernel (pass 0, then pass 1 for what outgrew pass 0's DP pool)
  int fallback() {
    for (int pass = 0; pass < 2 && !todo.empty(); ++pass) {
      std::vector<int64_t> next;
      PoaHbmLaunch L;
      for (size_t pos = 0; pos < todo.size();) {
        pos = poa_plan_hbm(in.seq_off, in.cluster_off, todo, pos, pass, L);
        const size_t nt = L.tasks.size();
        HIPCHK(b.ws_arena.reserve(poa_padded(sizeof(PoaTask) * nt) + poa_padded(sizeof(int32_t) * (size_t)L.w32) + poa_padded(sizeof(int64_t) * (size_t)L.w64) +
                                  poa_padded((size_t)L.w8) + 2 * poa_padded(sizeof(int32_t) * nt)));
        const Mem m = take(sizeof(PoaTask), nt, L.w32, L.w64, L.w8);
        HIPCHK(hipMemcpyAsync(m.tasks, L.tasks.data(), sizeof(PoaTask) * nt, hipMemcpyHostToDevice, s0));
        HIPCHK(hipMemsetAsync(m.st, 0xff, sizeof(int32_t) * nt, s0));
        if (const int rc = ev.create()) return rc;
        HIPCHK(hipEventRecord(ev.a, s0));
        hipLaunchKernelGGL(poa_consensus_kernel, dim3((unsigned)nt), dim3(64), 0, s0, (const PoaTask*)m.tasks, (const uint8_t*)d_seqs,
                           (const int64_t*)d_off, (int32_t*)m.w32, (int64_t*)m.w64, (uint8_t*)m.w8, (int32_t*)m.len, (int32_t*)m.st,
                           (unsigned long long*)d_cells);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.b, s0));
        HIPCHK(hipStreamSynchronize(s0));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
        b.kernel_ms += ms;
        int why[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (const int rc = collect(kPoaRounds + pass, L.tasks, L.ids, m, L.w8, next, why)) return rc;
      }
      todo.swap(next);
    }
    return SVDSS_OK;
  }

  // ---- stage 4
  int gather() {
    unsigned long long cells = 0;
    HIPCHK(hipMemcpyAsync(&cells, d_cells, 8, hipMemcpyDeviceToHost, s0));
    HIPCHK(hipStreamSynchronize(s0));
    b.cells = (int64_t)cells;
    for (int64_t c = 0; c < in.n_clusters; ++c) {
      b.cons_len[(size_t)c] = (int64_t)results[(size_t)c].size();
      b.cons.insert(b.cons.end(), results[(size_t)c].begin(), results[(size_t)c].end());
    }
    return SVDSS_OK;
  }
};
}  // namespace

extern "C" int svdss_poa_consensus_batch(const uint8_t* seqs, const int64_t* seq_off, const int64_t* cluster_off,
                                         int64_t n_clusters, int32_t device, svdss_poa_batch_t** out) {
  if (!out || n_clusters < 0 || device < 0) return SVDSS_EINVAL;
  if (n_clusters > 0 && (!seq_off || !cluster_off)) return SVDSS_EINVAL;
  HIPCHK(hipSetDevice(device));
  svdss_poa_batch* b = *out ? *out : new (std::nothrow) svdss_poa_batch();
  if (!b) return SVDSS_ENOMEM;
  *out = b;
  b->n_clusters = n_clusters;
  b->cells = 0;
  b->n_hbm = 0;
  b->n_quad_back = 0;
  b->kernel_ms = 0.0;
  b->cons_len.assign((size_t)n_clusters, 0);
  b->cons.clear();
  if (n_clusters == 0) return SVDSS_OK;
  PoaBatchRun run(*b, seqs, seq_off, cluster_off, n_clusters);
  int rc;
  if ((rc = run.upload(device)) || (rc = run.rounds()) || (rc = run.fallback())) return rc;
  return run.gather();
}

extern "C" int64_t svdss_poa_batch_nclusters(const svdss_poa_batch_t* b) { return b ? b->n_clusters : -1; }
extern "C" int64_t svdss_poa_batch_total(const svdss_poa_batch_t* b) { return b ? (int64_t)b->cons.size() : -1; }
extern "C" int64_t svdss_poa_batch_cells(const svdss_poa_batch_t* b) { return b ? b->cells : -1; }
extern "C" double svdss_poa_batch_kernel_ms(const svdss_poa_batch_t* b) { return b ? b->kernel_ms : -1.0; }
extern "C" int64_t svdss_poa_batch_hbm(const svdss_poa_batch_t* b) { return b ? b->n_hbm : -1; }
extern "C" int64_t svdss_poa_batch_quad_back(const svdss_poa_batch_t* b) { return b ? b->n_quad_back : -1; }
extern "C" int svdss_poa_batch_fetch(const svdss_poa_batch_t* b, int64_t* cons_len, uint8_t* cons) {
  if (!b) return SVDSS_EINVAL;
  if (cons_len) memcpy(cons_len, b->cons_len.data(), sizeof(int64_t) * b->cons_len.size());
  if (cons) memcpy(cons, b->cons.data(), b->cons.size());
  return SVDSS_OK;
}
extern "C" void svdss_poa_batch_free(svdss_poa_batch_t* b) { delete b; }

extern "C" int svdss_call_side_stat(int32_t device, int64_t out[4]) {
  if (!out || device < 0 || device >= kCallStreamDevices) return SVDSS_EINVAL;
  CallStreamPool& p = call_stream_pool();
  std::lock_guard<std::mutex> lock(p.mu);
  out[0] = p.live[device];
  out[1] = p.created;
  out[2] = p.merged;
  out[3] = p.borrowed;
  return SVDSS_OK;
}
