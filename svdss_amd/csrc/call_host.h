// call_host.h -- options of the `call`, `smooth` and `run` sub-commands (config.hpp:68-103 defaults), and the entry points of
// the sub-commands that have a file of their own.
#pragma once
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <string>
#include <unordered_map>
#include <vector>

struct CallOptions {
  std::string reference, bam, sfs;
  int threads = 4;
  unsigned min_cluster_weight = 2;   // (unsigned as in the reference, config.hpp:92-96: a negative value on the command
  unsigned min_sv_length = 25;       //  line is a huge one)
  unsigned min_mapq = 20;
  bool useht = true;
  float min_ratio = 0.97f;
  float accp = 0.98f;          // smooth only
  std::string write_index;     // smooth only: --write-index <FILE>, the output's BAI / CSI (bam_index_writer.h)
  int compress = 0;            // smooth only: --compress runs|lz, the GPU deflate's mode (0 runs, 1 lz; csrc/deflate.hip)
  // smooth only: --index FMD --sfs FILE, the text `SVDSS search` would write for the smoothed BAM (sfs above is FILE), with
  // search's own --bsize / --noputative / --noassemble; --nobam: no BAM on stdout
  std::string index;
  int bsize = 10000;
  bool putative = true, assemble = true, nobam = false;
  bool verbose = false;         // stage timings on stderr
  int gpus = 1;                 // --gpus N: POA / realignment batches shard by sub-cluster index
  std::string poa;             // --poa <FILE>: consensus alignments as SAM (caller.cpp:65-75)
  std::string clusters;        // --clusters <FILE>: the filled clusters (clusterer.cpp:613-626)
  bool clipped = false;        // --clipped: imprecise SVs from soft-clipped alignments (clipper.cpp; EXPERIMENTAL)
  std::string smoothed;        // run only: --smoothed <FILE>, the smoothed BAM (with write_index / compress above)
  std::string write_bam_index; // call, run: --write-bam-index <FILE>, the index of --bam (bam_input_index.h); bamindex: its -o
  // run --build-index: called once after run's own refusals (options, knobs, the samples list, BAMs that do not exist) and
  // before the GPU is looked for and anything is opened for writing -- builds a missing --index (svdss_main.cpp)
  void (*before_stages)(const CallOptions&) = nullptr;
};

// `SVDSS run` (run_host.cpp) drives the two units below; what passes between them:
struct svdss_bam_store;
struct svdss_ref;
struct svdss_index;
// ... into main_smooth's device path: the store every batch's records for `call` go into, where the SFS text goes instead
// of the file --sfs names, and what is handed over instead of freed when the stream is through
class InputIndexFold;                     // bam_input_index.h
struct SmoothHooks {
  svdss_bam_store* store = nullptr;      // svdss_bam_smooth_set_store, with the run's --min-mapq
  InputIndexFold* bam_index = nullptr;   // run --write-bam-index: the smoothing stage's reader folds the input's index into it
  FILE* sfs_sink = nullptr;              // the SFS text (closed when it is complete)
  bool keep_alive = false;               // return instead of ending the process: the GPU context stays up
  // out: batches of the stream; the chromosomes (FASTA order; upper-cased) and their copy on the GPU in BAM header order
  uint64_t n_batches = 0;
  std::vector<std::string> chrom_names;
  std::unordered_map<std::string, std::string> chrom_seqs;
  svdss_ref* dref = nullptr;
  std::vector<int32_t> tid_map;
  // `SVDSS run --samples` (the session of run_host.cpp): the hooks live through every sample, and what does not depend on
  // the BAM stays in them.  in: chrom_names / chrom_seqs of the sample before (non-empty: the FASTA is not read), dref with
  // tid_map as uploaded for a header of dref_names / dref_lens (the same header: not uploaded again), the index.  out: the
  // same, as this sample leaves them; `call` hands chromosomes and dref back instead of freeing them.
  bool session = false;
  std::vector<std::string> dref_names;
  std::vector<int32_t> dref_lens;
  // the index: index_host holds the records as svdss_index_load read them (once); `index` is what is resident -- a handle of
  // the rank blocks alone (index_rank_only) or index_host itself after the full restore.  The policy: a later
  // sample reuses what is resident, but the rank blocks alone give way to the full restore when its own estimate asks for
  // that; never the other way round.
  svdss_index* index_host = nullptr;
  svdss_index* index = nullptr;
  bool index_rank_only = false;
  int n_fasta_reads = 0, n_index_reads = 0, n_ref_uploads = 0;   // counted for the session's --verbose lines
};
// ... into CallRun: the SFS text in memory instead of the file, the filled store instead of the first pass over the file
// (nullptr: the file is read, exactly as `SVDSS call` does), the chromosomes main_smooth loaded
struct CallPreset {
  const char* sfs_text = nullptr;
  size_t sfs_bytes = 0;
  svdss_bam_store* store = nullptr;
  int64_t store_batches = 0;
  SmoothHooks* from_smooth = nullptr;
};

struct Options;   // cli_options.h

int main_search(const Options& o, time_t process_start);   // search_host.cpp
int main_call(const CallOptions& o, CallPreset* preset = nullptr);
int main_smooth(const CallOptions& o, SmoothHooks* hooks = nullptr);
int main_run(const CallOptions& o);                        // run_host.cpp
int main_bamindex(const CallOptions& o);                   // bamindex_host.cpp
// `SVDSS run --samples LIST` (run_host.cpp): o.bam is empty; regions / regions_file are resolved against every sample's header
int main_run_samples(const CallOptions& o, const std::string& list, const std::vector<std::string>& regions, const std::string& regions_file);
// --region / --regions-file against the header of `bam`, in force for every reader of the process from here on
// (svdss_main.cpp; `run --samples` calls it per sample, after regions_reset)
void regions_in_force(const std::vector<std::string>& regions, const std::string& regions_file, const std::string& bam, bool verbose);
void regions_reset();
void regions_report();   // bam_regions_report of bam_device_select.h, for the sample that has just ended
