// poa_task.h -- task descriptors of the POA kernels: PoaWaveTask of the LDS-resident ones (poa_wave.hip, poa_quad.hip),
// PoaTask of the HBM kernel (poa.hip); no HIP types: the planner (poa_plan.h) and the CPU wave emulator of the tests
// include it too.
#pragma once
#include <cstdint>

struct PoaWaveTask {
  int64_t seq_first, n_seqs;
  int32_t nc, ec;          // node / edge capacity of the graph
  int32_t max_len;         // longest read of the cluster
  int32_t ws;              // HBM stride of a DP row: power of two >= the widest row
  int32_t rs;              // LDS stride of a ring row: >= the widest row
  int32_t ring;            // DP rows kept in LDS (power of two); two more slots stage rows read back from HBM
  int32_t prio;            // s_setprio level (0-3): the longest chains of a batch decide its duration
  int32_t pad_;
  int64_t ws_off;          // into the int32 workspace (poa_wave_ws_ints of it)
  int64_t cons_off;        // into the byte workspace, nc bytes
};

struct PoaTask {
  int64_t seq_first, n_seqs;   // reads of this cluster: seq_off[seq_first .. seq_first+n_seqs]
  int32_t cap_nodes, cap_edges, max_len;
  int64_t pool_cap;            // int32 cells per DP array
  // workspace offsets (elements of the respective typed pools)
  int64_t node_off;            // per-node int32 arrays (stride cap_nodes): out_head,out_tail,in_head,in_tail,order,index,deg,best,row_beg,row_end,mpl,mpr + aln[5]
  int64_t edge_off;            // per-edge int32 arrays (stride cap_edges): from,to,w,next_out,next_in
  int64_t dp_off;              // 6 arrays of pool_cap int32
  int64_t op_off;              // 2 arrays of (cap_nodes + max_len + 4) int32
  int64_t row_off64;           // per-node int64: row offset into the DP arrays; then score[cap_nodes]
  int64_t base_off;            // per-node uint8 base
  int64_t cons_off;            // output consensus (uint8), capacity cap_nodes
};
