// call_host.h -- options of the `call` and `smooth` sub-commands (config.hpp:68-103 defaults), and the entry points of the
// sub-commands that have a file of their own.
#pragma once
#include <ctime>
#include <string>

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
};

struct Options;   // cli_options.h

int main_search(const Options& o, time_t process_start);   // search_host.cpp
int main_call(const CallOptions& o);
int main_smooth(const CallOptions& o);
