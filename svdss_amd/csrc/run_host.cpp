// run_host.cpp -- `SVDSS run`: run_svdss's chain -- smooth, search, call -- as ONE process and ONE pass over the BAM.
//
//   SVDSS smooth --reference FA --bam BAM > S;  SVDSS search --index FMD --bam S > T;  SVDSS call --reference FA --bam BAM --sfs T
//
// read the same alignments from disk three times.  Here the smoothing stage (SmoothRun's DevicePipeline with its SfsSide,
// smooth_host.cpp) searches the smoothed reads while they are in HBM, as `smooth --index --sfs` does, and deposits what
// `call` looks at of every ORIGINAL record in a record store (svdss_bam_smooth_set_store); the call stage (CallRun,
// call_host.cpp) parses the SFS text from memory and takes both of its passes from that store.  The VCF on stdout is the
// chain's, byte for byte; T and S are written only when --sfs / --smoothed ask for them.  This file drives the two units
// and holds nothing of either.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#define SVDSS_LOG_TAG "run"
#include "host_common.h"
#include "host_knobs.h"
#include "call_host.h"

int main_run(const CallOptions& o) {
  const SmoothKnobs smooth_knobs;
  const bool verbose = o.verbose || smooth_knobs.debug;
  // ---- what it cannot run on is said before anything is opened or written
  if (o.gpus != 1) die("run with --gpus other than 1 is out of scope: run it on one GPU");
  const std::string why = smooth_knobs.no_device_path(!o.smoothed.empty());
  if (why == "SVDSS_GPU_DEFLATE=0") die("run --smoothed deflates the smoothed BAM on the GPU: it does not run with " + why);
  if (!why.empty()) die("run needs the device path: it does not run with " + why);
  if (svdss_device_count() <= 0) die("no GPU found: SVDSS run smooths, searches and calls on the GPU");
  if (o.bsize <= 0) die("batch size smaller than the number of threads");
  struct stat stb;
  if (stat(o.bam.c_str(), &stb) != 0) die("cannot read " + o.bam);
  const auto t0 = std::chrono::steady_clock::now();
  auto t_last = t0;
  auto stage = [&](const char* what) {
    const auto now = std::chrono::steady_clock::now();
    if (verbose) fprintf(stderr, "[run] [time] %-28s %.3f s\n", what, std::chrono::duration<double>(now - t_last).count());
    t_last = now;
  };
  FILE* sfs_file = nullptr;
  if (!o.sfs.empty() && !(sfs_file = fopen(o.sfs.c_str(), "wb"))) die("cannot write " + o.sfs);
  int bam_fd = -1;
  if (!o.smoothed.empty() && (bam_fd = open(o.smoothed.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0) die("cannot write " + o.smoothed);
  // ---- the record store, sized by CallKnobs::store_sizes as `call` sizes its own (the arenas: SVDSS_STORE_ARENA_MB).  The
  // memory is taken from now on by the store's own thread, beside the FASTA and the index.
  svdss_bam_store* store = nullptr;
  const std::pair<int64_t, int64_t> store_size = CallKnobs().store_sizes((int64_t)stb.st_size);
  check(svdss_bam_store_create(0, store_size.first, std::max<int64_t>(0, store_size.second), &store), "svdss_bam_store_create");
  // ---- smooth + search: main_smooth's DevicePipeline; the smoothed BAM, when asked for, goes where stdout would have gone
  char* sfs_text = nullptr;
  size_t sfs_bytes = 0;
  SmoothHooks hooks;
  hooks.store = store;
  hooks.keep_alive = true;
  if (!(hooks.sfs_sink = open_memstream(&sfs_text, &sfs_bytes))) die("out of memory");
  {
    CallOptions so = o;
    so.sfs.clear();
    so.nobam = o.smoothed.empty();
    int saved_stdout = -1;
    if (bam_fd >= 0) {
      fflush(stdout);
      if ((saved_stdout = dup(STDOUT_FILENO)) < 0 || dup2(bam_fd, STDOUT_FILENO) < 0) die("cannot redirect the smoothed BAM to " + o.smoothed);
      close(bam_fd);
    }
    main_smooth(so, &hooks);
    if (saved_stdout >= 0) {
      fflush(stdout);
      if (dup2(saved_stdout, STDOUT_FILENO) < 0) die("cannot restore stdout");
      close(saved_stdout);
    }
  }
  if (!sfs_text) die("out of memory");
  if (sfs_file && ((sfs_bytes && fwrite(sfs_text, 1, sfs_bytes, sfs_file) != sfs_bytes) || fclose(sfs_file) != 0)) die("error writing " + o.sfs);
  stage("smooth + search");
  // ---- between the stages: the index, the park and the smoothing objects have left HBM (main_smooth); is the store whole?
  int32_t complete = 0;
  int64_t n_rec = 0, n_bytes = 0;
  const int64_t n_stored = svdss_bam_store_batches(store, &complete, &n_rec, &n_bytes);
  const bool whole = complete && n_stored == (int64_t)hooks.n_batches;
  if (verbose)
    fprintf(stderr, "[run] record store: %lld records, %lld bytes in %lld of %llu batches, %s\n", (long long)n_rec, (long long)n_bytes, (long long)n_stored,
            (unsigned long long)hooks.n_batches, whole ? "complete" : "incomplete: the call stage reads the file");
  CallPreset preset;
  preset.sfs_text = sfs_text;
  preset.sfs_bytes = sfs_bytes;
  preset.from_smooth = &hooks;
  if (whole) { preset.store = store; preset.store_batches = n_stored; }
  else svdss_bam_store_free(store);   // (`call`, over the file, takes its own)
  // ---- call: CallRun with its SFS map from the text and, with a whole store, both passes from HBM
  main_call(o, &preset);
  free(sfs_text);
  stage("call");
  if (verbose) fprintf(stderr, "[run] [time] %-28s %.3f s\n", "total", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}
