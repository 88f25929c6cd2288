// early_estimate.cpp -- csrc/early_estimate.h from the command line, for tests/test_early_estimate.py:
//   estimate WAITED LF_MAX INDEX_N  records,searched,comp_bytes,file_bytes,front_done ...
//       -> "each e0 e1 ...", "sum S", "wait_over 0|1", "rank_blocks_alone 0|1"   (LF_MAX < 0: not set, the default per index size)
//   park PARK_BYTES N_REGIONS N_DEVICES
//       -> one line per region: "g device bytes"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../svdss_amd/csrc/early_estimate.h"

int main(int argc, char** argv) {
  if (argc >= 5 && !strcmp(argv[1], "estimate")) {
    const double waited = atof(argv[2]), lf_max = atof(argv[3]);
    const int64_t index_n = atoll(argv[4]);
    std::vector<EarlyCounters> regions;
    for (int k = 5; k < argc; ++k) {
      long long r, s, c, f;
      int done;
      if (sscanf(argv[k], "%lld,%lld,%lld,%lld,%d", &r, &s, &c, &f, &done) != 5) { fprintf(stderr, "bad region %s\n", argv[k]); return 2; }
      EarlyCounters e;
      e.records = r; e.searched = s; e.comp_bytes = c; e.file_bytes = f; e.front_done = done != 0;
      regions.push_back(e);
    }
    printf("each");
    for (const EarlyCounters& e : regions) printf(" %.17g", estimate_reads_to_search(e));
    const double sum = summed_estimate(regions);
    printf("\nsum %.17g\nwait_over %d\nrank_blocks_alone %d\n", sum, estimate_wait_over(regions, waited) ? 1 : 0,
           rank_blocks_alone_pay(sum, lf_max >= 0, lf_max, index_n) ? 1 : 0);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "park")) {
    const int64_t bytes = atoll(argv[2]);
    const size_t n_regions = (size_t)atoll(argv[3]), n_devices = (size_t)atoll(argv[4]);
    for (size_t g = 0; g < n_regions; ++g)
      printf("%zu %zu %lld\n", g, n_devices ? g % n_devices : 0, (long long)park_bytes_of_region(bytes, n_regions, n_devices, g));
    return 0;
  }
  fprintf(stderr, "usage: estimate WAITED LF_MAX INDEX_N r,s,c,f,done ... | park BYTES N_REGIONS N_DEVICES\n");
  return 2;
}
