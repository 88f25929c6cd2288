// poa_quad.h -- launcher of the several-sub-clusters-per-wavefront POA kernel (poa_quad.hip, poa_quad_core.h).  Tasks
// are poa_wave.hip's records with ws = group width x columns per lane; consecutive tasks of a launch share a wavefront
// (64 / group width of them).  The heaviest-bundle consensus is poa_wave.hip's poa_bundle_kernel (poa_bundle_launch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "poa_task.h"

// max_len: the longest read of the launch (poa_quad_lds_bytes of it must fit)
hipError_t poa_quad_launch(int gw, int cols, const PoaWaveTask* d_tasks, int n_tasks, int max_len, const uint8_t* d_seqs, const int64_t* d_seq_off,
                           int32_t* ws32, int32_t* d_len, int32_t* d_status, unsigned long long* d_cells, hipStream_t stream);
// One launch of both whole-wavefront variants: tasks [0, n2) are (64, 2) sub-clusters, tasks [n2, n2 + n1) are (64, 1) ones,
// d_len / d_status indexed like the tasks, the tasks' ws_off into the one ws32 (poa_merged_group of poa_plan.h);
// max_len2 / max_len1: the longest read of either half.  n2 or n1 may be 0.
hipError_t poa_quad_pair_launch(const PoaWaveTask* d_tasks, int n2, int n1, int max_len2, int max_len1, const uint8_t* d_seqs,
                                const int64_t* d_seq_off, int32_t* ws32, int32_t* d_len, int32_t* d_status, unsigned long long* d_cells,
                                hipStream_t stream);
void poa_quad_debug_report();
