// early_estimate.h -- what `SVDSS search` decides from the counters of its early front ends (sfs_units.h: EarlySearch), as
// plain arithmetic on plain numbers: no HIP, no library handle, so that a small program can call it (tests/native).
// One front end (one GPU) or one per region of the file (--gpus N): the process takes ONE decision, from their sum.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// what one front end has seen: records walked, reads it will search, compressed bytes read; the bytes of its part of the
// file; whether every feeding thread of it has ended
struct EarlyCounters {
  int64_t records = 0, searched = 0, comp_bytes = 0, file_bytes = 0;
  bool front_done = false;
};
// a front end is asked for its estimate when it has seen this many records (or all it has)
constexpr int64_t kEarlyEstimateRecords = 50000;
constexpr double kEarlyEstimateWaitSeconds = 1.5;

// reads there will be to search in one front end's part of the file, from the share it has seen (-1: nothing seen yet)
inline double estimate_reads_to_search(const EarlyCounters& c) {
  return c.records > 0 && c.comp_bytes > 0 ? (double)c.searched / (double)c.records * ((double)c.records * (double)c.file_bytes / (double)c.comp_bytes) : -1;
}
// ... in the whole file: the sum over its regions.  A region that has seen nothing contributes nothing (its -1 is not
// added); -1 when no region has seen anything.  N samples spread over the file instead of its first records: regions of
// equal make give exactly the one-region figure of the whole file, regions that differ are each counted as they are.
inline double summed_estimate(const std::vector<EarlyCounters>& regions) {
  double sum = 0;
  bool any = false;
  for (const EarlyCounters& c : regions) {
    const double e = estimate_reads_to_search(c);
    if (e >= 0) { sum += e; any = true; }
  }
  return any ? sum : -1;
}
// the wait for the estimate is over: every region has seen enough records or finished its front -- or time is up
inline bool estimate_wait_over(const std::vector<EarlyCounters>& regions, double waited_seconds) {
  if (waited_seconds > kEarlyEstimateWaitSeconds) return true;
  for (const EarlyCounters& c : regions)
    if (!c.front_done && c.records < kEarlyEstimateRecords) return false;
  return true;
}
// the index as a rank structure alone pays up to this many reads to search: SVDSS_SEARCH_LF_MAX, else 2 M per 6.18e9 BWT
// symbols (sfs_units.h: wants_rank_blocks_alone)
inline double rank_blocks_max_reads(bool lf_max_set, double lf_max, int64_t index_n) { return lf_max_set ? lf_max : 2e6 * (double)index_n / 6.18e9; }
// the choice itself, from the (summed) estimate
inline bool rank_blocks_alone_pay(double est, bool lf_max_set, double lf_max, int64_t index_n) {
  return est >= 0 && est <= rank_blocks_max_reads(lf_max_set, lf_max, index_n);
}
// HBM for the park of region g of n_regions on n_devices (region g lives on device g % n_devices): the whole of
// park_bytes when the region has its device to itself, an equal part of it when regions share the device
inline int64_t park_bytes_of_region(int64_t park_bytes, size_t n_regions, size_t n_devices, size_t g) {
  if (n_devices == 0 || g >= n_regions) return 0;
  const size_t d = g % n_devices;
  const size_t sharing = n_regions / n_devices + (d < n_regions % n_devices ? 1 : 0);   // regions g' with g' % n_devices == d
  return park_bytes / (int64_t)(sharing ? sharing : 1);
}
