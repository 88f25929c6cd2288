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
//
// `SVDSS run --samples LIST` (run_samples.h) is the same body once per line of LIST, in one process: a session owns what does
// not depend on the BAM -- the chromosomes on the host and in HBM, the index, and with the process the HIP context, the call
// side's streams and the page-locked pools -- and hands it to every sample through the SmoothHooks; everything else (record
// store, park, regions, stopwatches, threads) begins and ends with its sample.  DESIGN.md section 4g.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#define SVDSS_LOG_TAG "run"
#include "host_common.h"
#include "host_knobs.h"
#include "call_host.h"
#include "run_samples.h"
#include "bam_input_index.h"

namespace {
// what `run` cannot run on: said before anything is opened or written, and before the GPU is looked for
void refuse_what_cannot_run(const CallOptions& o, const SmoothKnobs& smooth_knobs) {
  if (o.gpus != 1) die("run with --gpus other than 1 is out of scope: run it on one GPU");
  const std::string why = smooth_knobs.no_device_path(!o.smoothed.empty());
  if (why == "SVDSS_GPU_DEFLATE=0") die("run --smoothed deflates the smoothed BAM on the GPU: it does not run with " + why);
  if (!why.empty()) die("run needs the device path: it does not run with " + why);
}

// ---- `run --samples`: what the session looks at between stages and samples
int64_t free_hbm() {
  int64_t f = 0, t = 0;
  check(svdss_device_memory(0, &f, &t), "svdss_device_memory");
  return f;
}
long thread_count() {   // threads of this process, as /proc lists them (-1: no /proc)
  DIR* d = opendir("/proc/self/task");
  if (!d) return -1;
  long n = 0;
  while (const dirent* e = readdir(d)) n += e->d_name[0] != '.';
  closedir(d);
  return n;
}
// the index leaves HBM (and, where the resident handle is the one that holds the records, the host): the next sample makes
// it resident again, from the file
void drop_index(SmoothHooks& h) {
  if (h.index && h.index != h.index_host) svdss_index_free(h.index);
  else if (h.index) { svdss_index_free(h.index_host); h.index_host = nullptr; }
  h.index = nullptr;
  h.index_rank_only = false;
}

// one BAM through smooth + search and call.  hooks: what passes between the two stages -- and, with hooks.session, from one
// sample to the next (the VCF goes to stdout either way: the session points stdout at the sample's file)
void run_one(const CallOptions& o, SmoothHooks& hooks, bool verbose, int64_t index_min_free = 0) {
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
  hooks.store = store;
  hooks.keep_alive = true;
  hooks.n_batches = 0;
  // --write-bam-index FILE: the index of o.bam, folded from what the smoothing stage's reader sees of every batch
  InputIndexFold bam_index;
  if (!o.write_bam_index.empty()) {
    std::vector<int32_t> lens;
    std::string err;
    if (!bam_header_lengths(o.bam, lens, err)) die("cannot read " + o.bam + ": " + err);
    if (!bam_index.open(o.write_bam_index, lens, "--write-bam-index", err)) die(err);
    hooks.bam_index = &bam_index;
  }
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
  hooks.sfs_sink = nullptr;
  if (hooks.bam_index) {   // (an unsorted BAM: a warning and no index -- the index is a by-product)
    hooks.bam_index = nullptr;
    std::string err;
    if (bam_index.finish(o.bam, err)) { if (verbose) fprintf(stderr, "[run] index of %s written to %s\n", o.bam.c_str(), o.write_bam_index.c_str()); }
    else if (bam_index.unsorted()) fprintf(stderr, "[run] [warning] --write-bam-index: %s\n", err.c_str());
    else die(err);
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
  hooks.store = nullptr;
  // (`run --samples`: the index stays through the call stage -- the POA batch sizes its workspace from the HBM that is free --
  // unless too little is left beside it and the store)
  if (hooks.session && hooks.index && index_min_free > 0) {
    const int64_t f = free_hbm();
    if (f < index_min_free) {
      drop_index(hooks);
      if (verbose) fprintf(stderr, "[run] index: %lld bytes of HBM free before the call stage: the index leaves and is made resident again for the next sample\n", (long long)f);
    }
  }
  // ---- call: CallRun with its SFS map from the text and, with a whole store, both passes from HBM
  {
    CallOptions co = o;
    co.write_bam_index.clear();   // (written above: a call stage that reads the file itself does not index it again)
    main_call(co, &preset);
  }
  free(sfs_text);
  stage("call");
  if (verbose) fprintf(stderr, "[run] [time] %-28s %.3f s\n", "total", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

// ---- `run --samples`
bool same_file(const std::string& a, const std::string& b) {
  struct stat sa, sb;
  return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}
long vcf_records(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return -1;
  long n = 0;
  bool at_start = true;
  for (int c; (c = fgetc(f)) != EOF;) {
    if (at_start && c != '#' && c != '\n') ++n;
    at_start = c == '\n';
  }
  fclose(f);
  return n;
}
}  // namespace

int main_run(const CallOptions& o) {
  const SmoothKnobs smooth_knobs;
  // ---- what it cannot run on is said before anything is opened or written
  refuse_what_cannot_run(o, smooth_knobs);
  if (o.before_stages) {   // (--build-index: every refusal that needs no GPU comes before the index is built)
    struct stat stb;
    if (o.bsize <= 0) die("batch size smaller than the number of threads");
    if (stat(o.bam.c_str(), &stb) != 0) die("cannot read " + o.bam);
    o.before_stages(o);
  }
  if (svdss_device_count() <= 0) die("no GPU found: SVDSS run smooths, searches and calls on the GPU");
  if (o.bsize <= 0) die("batch size smaller than the number of threads");
  SmoothHooks hooks;
  run_one(o, hooks, o.verbose || smooth_knobs.debug);
  return 0;
}

int main_run_samples(const CallOptions& o, const std::string& list, const std::vector<std::string>& regions, const std::string& regions_file) {
  const SmoothKnobs smooth_knobs;
  const bool verbose = o.verbose || smooth_knobs.debug;
  // ---- refused before anything is opened for writing and before the GPU is looked for
  refuse_what_cannot_run(o, smooth_knobs);
  if (o.bsize <= 0) die("batch size smaller than the number of threads");
  std::vector<RunSample> samples;
  std::string err;
  std::vector<std::string> inputs{o.reference, o.index};
  if (!regions_file.empty()) inputs.push_back(regions_file);
  if (!load_run_samples(list, inputs, samples, err)) die(err);
  inputs.push_back(list);
  for (const RunSample& s : samples) {
    const std::string where = "--samples " + list + " line " + std::to_string(s.line) + ": ";
    struct stat stb;
    if (stat(s.bam.c_str(), &stb) != 0) die(where + "cannot read " + s.bam);
    // (another spelling of a path the run reads, or a link to it)
    for (const std::string* out : {&s.vcf, &s.sfs}) {
      if (out->empty()) continue;
      for (const std::string& in : inputs) if (same_file(*out, in)) die(where + "the output " + *out + " is an input of the run");
      for (const RunSample& t : samples) if (same_file(*out, t.bam)) die(where + "the output " + *out + " is an input of the run");
    }
  }
  if (o.before_stages) o.before_stages(o);   // (--build-index: once, before the first sample, after every refusal above)
  if (svdss_device_count() <= 0) die("no GPU found: SVDSS run smooths, searches and calls on the GPU");
  // (fewer MB of HBM free than this after a sample's smoothing stage: the index leaves for the call stage)
  const int64_t min_free = env_from("SVDSS_RUN_INDEX_MIN_FREE_MB", 0, 8192) << 20;
  SmoothHooks hooks;   // the session: chromosomes, their copy in HBM, the index
  hooks.session = true;
  for (size_t k = 0; k < samples.size(); ++k) {
    const RunSample& s = samples[k];
    const auto t0 = std::chrono::steady_clock::now();
    const std::string vcf_tmp = s.vcf + ".tmp", sfs_tmp = s.sfs.empty() ? "" : s.sfs + ".tmp";
    DieContext& dc = die_context();
    dc.prefix = "sample " + std::to_string(k + 1) + " (" + s.bam + "): ";
    dc.unlink = {vcf_tmp};
    if (!sfs_tmp.empty()) dc.unlink.push_back(sfs_tmp);
    if (verbose)
      fprintf(stderr, "[run] sample %zu of %zu: %s; %lld bytes of HBM free, %ld thread(s)\n", k + 1, samples.size(), s.bam.c_str(), (long long)free_hbm(), thread_count());
    // ---- the regions, against this sample's own header
    regions_reset();
    regions_in_force(regions, regions_file, s.bam, o.verbose);
    // ---- stdout is the sample's VCF while it runs
    const int vcf_fd = open(vcf_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (vcf_fd < 0) die("cannot write " + vcf_tmp);
    fflush(stdout);
    const int saved_stdout = dup(STDOUT_FILENO);
    if (saved_stdout < 0 || dup2(vcf_fd, STDOUT_FILENO) < 0) die("cannot redirect the VCF to " + vcf_tmp);
    close(vcf_fd);
    CallOptions so = o;
    so.bam = s.bam;
    so.sfs = sfs_tmp;
    run_one(so, hooks, verbose, min_free);
    const bool flushed = fflush(stdout) == 0;
    if (dup2(saved_stdout, STDOUT_FILENO) < 0) die("cannot restore stdout");
    close(saved_stdout);
    if (!flushed) die("error writing " + vcf_tmp);
    regions_report();
    const long n_vcf = vcf_records(vcf_tmp);
    if (!sfs_tmp.empty() && rename(sfs_tmp.c_str(), s.sfs.c_str()) != 0) die("cannot write " + s.sfs);
    if (rename(vcf_tmp.c_str(), s.vcf.c_str()) != 0) die("cannot write " + s.vcf);
    dc.unlink.clear();
    dc.prefix.clear();
    fprintf(stderr, "[run] sample %zu: %s -> %s: %ld VCF record(s), %.3f s\n", k + 1, s.bam.c_str(), s.vcf.c_str(), n_vcf,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  regions_reset();
  if (verbose)
    fprintf(stderr, "[run] %zu sample(s): the FASTA read %d time(s), the index file %d time(s), the chromosomes uploaded %d time(s)\n", samples.size(),
            hooks.n_fasta_reads, hooks.n_index_reads, hooks.n_ref_uploads);
  return 0;
}
