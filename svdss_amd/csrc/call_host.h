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
};

// `SVDSS run` (run_host.cpp) drives the two units below; what passes between them:
struct svdss_bam_store;
struct svdss_ref;
// ... into main_smooth's device path: the store every batch's records for `call` go into, where the SFS text goes instead
// of the file --sfs names, and what is handed over instead of freed when the stream is through
struct SmoothHooks {
  svdss_bam_store* store = nullptr;      // svdss_bam_smooth_set_store, with the run's --min-mapq
  FILE* sfs_sink = nullptr;              // the SFS text (closed when it is complete)
  bool keep_alive = false;               // return instead of ending the process: the GPU context stays up
  // out: batches of the stream; the chromosomes (FASTA order; upper-cased) and their copy on the GPU in BAM header order
  uint64_t n_batches = 0;
  std::vector<std::string> chrom_names;
  std::unordered_map<std::string, std::string> chrom_seqs;
  svdss_ref* dref = nullptr;
  std::vector<int32_t> tid_map;
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
