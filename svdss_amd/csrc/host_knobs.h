// host_knobs.h -- every SVDSS_* variable smooth_host.cpp, call_host.cpp and run_host.cpp read, read once per run (README.md
// has the tables).  Not here, as for `search` (SearchKnobs, sfs_units.h): what the library, bam_device_select.h,
// bam_reader.h, the inflate / deflate hooks and effective_gpus (host_common.h) read themselves.
#pragma once
#include <utility>
#include "host_common.h"

struct SmoothKnobs {
  bool smooth_host = getenv("SVDSS_SMOOTH_HOST") != nullptr;                 // the host pipeline with the host walk: no GPU at all
  bool bam_device = env_switch("SVDSS_BAM_DEVICE") != 0;                     // 0: the host pipeline (GPU walk) although there is a GPU
  bool gpu_deflate = env_switch("SVDSS_GPU_DEFLATE") != 0;                   // 0: the host's deflate, which is the host pipeline's writer
  int64_t batch_bytes = env_from("SVDSS_BAM_BATCH_MB", 1, 64) << 20;         // inflated bytes per device batch (64 MB here)
  int feeders = (int)env_raised("SVDSS_SEARCH_FEEDERS", 1, 6);               // feeding threads per GPU (6)
  bool fasta_serial = getenv("SVDSS_FASTA_SERIAL") != nullptr;               // the FASTA line by line although it could be mapped
  bool serial_write = getenv("SVDSS_SMOOTH_SERIAL_WRITE") != nullptr;        // a regular file written in order, like a pipe
  int writers = (int)env_raised("SVDSS_SMOOTH_WRITERS", 1, 4);               // side-by-side writers of a regular file (4)
  bool clean_exit = getenv("SVDSS_CLEAN_EXIT") != nullptr;                   // orderly teardown instead of _exit (leak checkers)
  bool debug = getenv("SVDSS_DEBUG") != nullptr;                             // the `+%.3f s` lines and the stage seconds on stderr
  // why the device path cannot run: the setting that rules it out, or "" (deflates: the run writes a BAM)
  std::string no_device_path(bool deflates = true) const {
    return smooth_host ? "SVDSS_SMOOTH_HOST=1" : !bam_device ? "SVDSS_BAM_DEVICE=0" : deflates && !gpu_deflate ? "SVDSS_GPU_DEFLATE=0" : "";
  }
};

struct CallKnobs {
  int64_t batch_bytes = env_from("SVDSS_BAM_BATCH_MB", 1, 256) << 20;        // inflated bytes per device batch of the two BAM passes (256 MB)
  int pass2_threads = (int)env_from("SVDSS_CALL_PASS2_THREADS", 1, 0);       // host threads over the chunks an index names (0: the cores, at most 32)
  int feeders = (int)env_from("SVDSS_CALL_FEEDERS", 1, 3);                   // feeding threads per GPU of the two BAM passes (3)
  bool fasta_serial = getenv("SVDSS_FASTA_SERIAL") != nullptr;               // the FASTA line by line although it could be mapped
  bool bam_device = env_switch("SVDSS_BAM_DEVICE") != 0;                     // 0: the host reader although there is a GPU
  bool store = env_switch("SVDSS_CALL_STORE") != 0;                          // 0: no record store, two passes over the file
  // the record store: up to SVDSS_CALL_STORE_GB per GPU (160: a 30x human sample is ~50 GB), or SVDSS_CALL_STORE_MB (tests);
  // taken at once: SVDSS_CALL_STORE_INITIAL_MB, else what the file should need
  int64_t store_cap = env_from("SVDSS_CALL_STORE_MB", 1, env_from("SVDSS_CALL_STORE_GB", 1, 160) << 10) << 20;
  bool store_initial_set = getenv("SVDSS_CALL_STORE_INITIAL_MB") != nullptr;
  int64_t store_initial = store_initial_set ? atoll(getenv("SVDSS_CALL_STORE_INITIAL_MB")) << 20 : 0;
  bool cache_gb_set = getenv("SVDSS_CALL_CACHE_GB") != nullptr;              // the host reader's record cache for pass 2 ...
  double cache_gb = cache_gb_set ? atof(getenv("SVDSS_CALL_CACHE_GB")) : 0;  //     (default: 40 % of MemAvailable, at most 64)
  bool place_host = getenv("SVDSS_PLACE_HOST") != nullptr;                   // the SFS placed by host code, no chromosomes on the GPU
  bool no_bai = getenv("SVDSS_CALL_NO_BAI") != nullptr;                      // pass 2 ignores an index beside the BAM
  std::string pass2 = getenv("SVDSS_CALL_PASS2") ? getenv("SVDSS_CALL_PASS2") : "";   // bai | device: overrides the estimate
  bool debug = getenv("SVDSS_DEBUG") != nullptr;                             // more --verbose lines
  bool clean_exit = getenv("SVDSS_CLEAN_EXIT") != nullptr;                   // the record stores freed before the process ends
  // the store of a file (or region) of file_bytes: {cap, taken at once}.  Expected: the bases, two per byte, + names and
  // CIGARs -- at most ~2.5 x a well-compressed BAM
  std::pair<int64_t, int64_t> store_sizes(int64_t file_bytes) const {
    return {store_cap, store_initial_set ? store_initial : std::min(store_cap, file_bytes * 5 / 2 + ((int64_t)256 << 20))};
  }
};
