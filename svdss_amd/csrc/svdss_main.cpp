// svdss_main.cpp -- `SVDSS` host CLI on top of libsvdss_hip.so.
//
// Keeps the process boundary B1 of SURVEY.md 8(b):
//   SVDSS index  [-i old.fmd] -d ref.fa [more.fa ...] [-o ref.fa.fmd] [-t T]   (/root/reference/main.cpp:34-37, run_svdss:142)
//   SVDSS smooth --reference R --bam B [--threads T] [--min-mapq N] [--accp F]      (main.cpp:69-77; smooth_host.cpp)
//   SVDSS search --index F --bam B | --fastx Q [--threads T] [--bsize N] [--noputative]
//                [--noassemble] [--omax N] [--verbose]  (config.cpp:30-55, main.cpp:62-68; search_host.cpp)
//   SVDSS call   --reference R --bam B --sfs S [...]    (main.cpp:55-61; call_host.cpp)
//   SVDSS run    --reference R --bam B --index F [...]  (run_host.cpp: smooth, search and call in one pass over the BAM)
//   SVDSS bamindex --bam B [-o FILE]                    (bamindex_host.cpp: the BAI / CSI of the input, `samtools index`)
//   SVDSS --version                                     (main.cpp:45-47)
// This file: the usage texts, the command line, `index`; the other sub-commands have a file each.
// Logs go to stderr (host_common.h), fatal conditions exit(1).
// Additions of this program: --gpus N (search, call, smooth), --io-threads N, --verbose stage timings, --write-index FILE (smooth),
// --compress runs|lz (smooth), --index FMD --sfs FILE [--nobam] (smooth: the search of the smoothed reads in the same pass),
// the sub-command `run` with its --smoothed FILE, --region REG / --regions-file BED (smooth, search --bam, call, run:
// bam_regions.h), --samples LIST (run: many BAMs in one process, run_samples.h and run_host.cpp), the sub-command `bamindex`
// and --write-bam-index FILE (call, run: the index of the input BAM as a by-product, bam_input_index.h).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <malloc.h>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <utime.h>
#include <vector>

#include "host_common.h"
#include "cli_options.h"
#include "call_host.h"
#include "fastx_reader.h"
#include "ref_loader.h"
#include "bam_device_select.h"
#include "bam_region_ranges.h"
#include "run_samples.h"
#include "bam_input_index.h"

static const char* VERSION = "v2.1.1";  // main.cpp:19

// (weak: a build of the binary from a source list without run_host.cpp -- the sanitized CPU build of tests/ -- still links;
// `run` then says so)
__attribute__((weak)) int main_run(const CallOptions& o);
__attribute__((weak)) int main_run_samples(const CallOptions& o, const std::string& list, const std::vector<std::string>& regions, const std::string& regions_file);
__attribute__((weak)) int main_bamindex(const CallOptions& o);

static const char* MAIN_USAGE =
    "Usage: SVDSS <index|smooth|search|call|run> --help\n"
    "  index   build the FM-index of a reference (FASTA, gz ok):  SVDSS index [-i old.fmd] -d ref.fa [more.fa ...] -o ref.fa.fmd [-t T]\n"
    "  search  extract sample-specific strings: SVDSS search --index ref.fa.fmd --bam reads.bam > specifics.txt\n"
    "  call    call SVs from the specific strings:    SVDSS call --reference ref.fa --bam reads.bam --sfs specifics.txt\n"
    "  smooth  smooth a BAM (reads equal the reference except at long indels): SVDSS smooth --reference ref.fa --bam in.bam > out.bam\n"
    "  run     smooth, search and call in one pass over the BAM: SVDSS run --reference ref.fa --bam reads.bam --index ref.fa.fmd > variations.vcf\n";

// the two options of smooth, search --bam, call and run (bam_regions.h), in one place for the four usage texts
#define REGION_HELP \
    "      --region <REG>        only the records that overlap REG: NAME, NAME:BEG-END, NAME:BEG- or NAME:BEG (1-based,\n" \
    "                            inclusive, commas ignored; NAME:BEG runs to the reference's end).  May be given several\n" \
    "                            times: the regions add up.  The command then behaves as on a BAM that holds those records alone\n" \
    "      --regions-file <BED>  the same for every line of a BED file (tab-separated, 0-based half-open); adds to --region.\n" \
    "                            With <BAM>.bai, <BAM>.csi or <stem>.bai not older than the BAM only the parts of the file\n" \
    "                            the index names are read, as one stream on one GPU whatever --gpus says; without one the\n" \
    "                            whole file is read.  Either way the records are tested on the GPU\n"

#define WRITE_BAM_INDEX_HELP \
    "      --write-bam-index <FILE>    also write the index of <BAM> itself (what `SVDSS bamindex` writes: CSI if FILE ends in\n" \
    "                                  .csi, else BAI), a by-product of the pass that reads it anyway.  Not with --region /\n" \
    "                                  --regions-file.  An unsorted BAM: a warning, no index, the output as without the option\n"

static const char* SMOOTH_USAGE =
    "Usage: SVDSS smooth --reference <FASTA> --bam <BAM> > smoothed.bam\n"
    "      --min-mapq <int>   minimum mapping quality (default: 20)\n"
    "      --accp <float>     accuracy percentile (default: 0.98)\n"
    "      --write-index <FILE>  also write the output's index: CSI if FILE ends in .csi, else BAI (as `samtools index`\n"
    "                            of a BAM written to a new file or a pipe; appended to a non-empty file, it indexes the\n"
    "                            appended stream only)\n"
    "      --compress <runs|lz>  how the GPU deflates the output (default: runs): runs codes literals and runs of equal\n"
    "                            bytes; lz also finds matches between overlapping reads (a smaller file, more GPU time).\n"
    "                            No effect where the host deflates (SVDSS_GPU_DEFLATE=0, SVDSS_SMOOTH_HOST=1)\n"
    "      --index <FMD> --sfs <FILE>  also search the smoothed reads while they are on the GPU: FILE receives what\n"
    "                            `SVDSS search --index FMD --bam smoothed.bam` writes to stdout, with the same --threads,\n"
    "                            --bsize, --noputative and --noassemble (one GPU, the device path)\n"
    "      --nobam               with --index --sfs: write FILE only, nothing to stdout\n"
    REGION_HELP;

static const char* CALL_USAGE =
    "Usage: SVDSS call --reference <FASTA> --bam <BAM> --sfs <SFS>\n"
    "      --threads <int>             kept for output-order compatibility (default: 4)\n"
    "      --min-cluster-weight <int>  minimum number of supporting superstrings for a call (default: 2)\n"
    "      --min-sv-length <int>       minimum length of reported SVs (default: 25, values < 25 ignored)\n"
    "      --min-mapq <int>            minimum mapping quality (default: 20)\n"
    "      --poa <FILE>                store POA consensus alignments in .sam format to this file\n"
    "      --clusters <FILE>           store clusters to this file\n"
    "      -l <float>                  minimum length ratio for sub-clusters and chain merging (default: 0.97)\n"
    "      --noht                      ignore the HP tag\n"
    "      --clipped                   also call imprecise SVs from soft-clipped alignments (EXPERIMENTAL)\n"
    WRITE_BAM_INDEX_HELP
    REGION_HELP;

static const char* RUN_USAGE =
    "Usage: SVDSS run --reference <FASTA> --bam <BAM> --index <FMD> > variations.vcf\n"
    "      smooth, search and call in one process and one pass over the BAM (one GPU, the device path); stdout receives the\n"
    "      VCF of `SVDSS smooth`, `SVDSS search` on its output and `SVDSS call` on <BAM> with the same option values\n"
    "      --sfs <FILE>          also write the specific strings (what `SVDSS search` writes to stdout)\n"
    "      --smoothed <FILE>     also write the smoothed BAM (what `SVDSS smooth` writes to stdout); without it nothing is deflated\n"
    "      --write-index <FILE>  with --smoothed: its index, CSI if FILE ends in .csi, else BAI\n"
    "      --compress <runs|lz>  with --smoothed: how the GPU deflates it (default: runs)\n"
    "      --threads <int> --min-mapq <int> --accp <float>                      as in smooth, search and call\n"
    "      --bsize <int> --noputative --noassemble                              as in search\n"
    "      --min-cluster-weight <int> --min-sv-length <int> -l <float> --noht   as in call\n"
    "      --poa <FILE> --clusters <FILE> --clipped                             as in call\n"
    "      --build-index         where <FMD> does not exist: build it first, as `SVDSS index -d <FASTA> -o <FMD> -t <threads>`\n"
    "                            does (<FMD> and <FMD>.svdss are written, once for all of --samples), then go on; where it\n"
    "                            exists nothing changes.  A build that fails leaves no file and ends the process\n"
    "      --verbose             stage timings and the record store's size on stderr\n"
    "      --samples <LIST>      instead of --bam: many BAMs in this one process, in the order of LIST; the reference, the index\n"
    "                            and the pools stay between them.  LIST: one sample per line, BAM<TAB>VCF[<TAB>SFS]; empty lines\n"
    "                            and lines that start with '#' are skipped.  VCF receives what `run --bam BAM` with the same\n"
    "                            options writes to stdout, SFS what --sfs writes; each is written as <path>.tmp and renamed when\n"
    "                            complete; stdout stays empty, stderr gets one line per finished sample.  Not with --sfs,\n"
    "                            --smoothed, --write-index, --compress, --poa or --clusters.  A sample that fails ends the\n"
    "                            process with a non-zero status: the samples before it are complete, it leaves no file, the\n"
    "                            samples after it are not started\n"
    WRITE_BAM_INDEX_HELP
    REGION_HELP;

static const char* BAMINDEX_USAGE =
    "Usage: SVDSS bamindex --bam <BAM> [-o <FILE>]\n"
    "      the index of <BAM> (sorted by coordinate), what `samtools index` writes: one pass over the file, the records\n"
    "      indexed on the GPU where they are inflated\n"
    "      -o <FILE>         the index (default: <BAM>.bai): CSI if FILE ends in .csi, else BAI (no reference longer than\n"
    "                        2^29 - 1 then).  Written as <FILE>.tmp and renamed when complete\n"
    "      --gpus <N|all>    the file's regions, one per GPU\n"
    "      --threads <int>   accepted as by the other sub-commands (the pass is bound by the inflate on the GPU)\n"
    "      --verbose         records, chunks, windows, compressed bytes read and seconds on stderr\n"
    "      SVDSS_BAM_DEVICE=0 runs the host reader instead (one thread); without a GPU and without it the command stops\n";

static const char* SEARCH_USAGE =
    "Usage: SVDSS search --index <FMD> --bam <BAM> | --fastx <FASTA/FASTQ>\n"
    "      --threads <int>   kept for output-order compatibility (default: 4)\n"
    "      --bsize <int>     batch size (default: 10000)\n"
    "      --noputative      search all reads, not only XF == 0\n"
    "      --noassemble      do not merge overlapping specific strings\n"
    REGION_HELP;

// do two paths name one file?  (the same text, or the same inode where both exist)
static bool same_file(const std::string& a, const std::string& b) {
  if (a == b) return true;
  struct stat sa, sb;
  return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

static Options parse(int argc, char** argv) {
  Options o;
  std::string err;
  if (!parse_options(argc, argv, 2, o, err)) die(err);
  if (o.gpus_all) o.gpus = svdss_device_count();
  return o;
}

// ---------------------------------------------------------------- index

// --region / --regions-file against the BAM header, before anything is opened for writing: the command's regions in
// force for every reader of the process (bam_regions.h), or a message that names the offending text
static void regions_in_force(const Options& o, const char* cmd) {
  if (o.regions.empty() && o.regions_file.empty()) return;
  if (!o.samples.empty() && !strcmp(cmd, "run")) return;   // (resolved per sample, against each sample's own header: run_host.cpp)
  if (o.bam.empty() && o.fastx.empty()) return;   // (the command's usage text follows)
  if (o.bam.empty() || !o.fastx.empty())
    die(std::string("--region / --regions-file select records of a BAM by position: not an option of `SVDSS ") + cmd + (o.fastx.empty() ? "`" : " --fastx`"));
  regions_in_force(o.regions, o.regions_file, o.bam, o.verbose);
}
// `run --samples`, between two samples: no regions in force, no plan, the counters of the next report at zero
void regions_reset() {
  bam_regions_in_force() = nullptr;
  bam_region_plan() = BamRegionPlan();
  BamRegionCounters& c = bam_region_counters();
  c.gated = 0; c.comp_bytes = 0; c.host_readers = 0; c.verbose = false;
  int64_t on_device = 0;
  (void)svdss_bam_gated_total(&on_device);
  c.device_base = on_device;
}
void regions_report() { bam_regions_report(); }
void regions_in_force(const std::vector<std::string>& regions, const std::string& regions_file, const std::string& bam, bool verbose) {
  if (regions.empty() && regions_file.empty()) return;
  int32_t n_ref = 0;
  int64_t skip = 0;
  std::string err;
  std::vector<std::string> names;
  if (!bam_header_probe(bam, n_ref, skip, err, &names)) die("cannot read " + bam + ": " + err);
  static BamRegionSet U;   // (one at a time: a sample of `run --samples` resolves its own over the one before)
  if (!resolve_regions(regions, regions_file, names, U, err)) die(err);
  bam_regions_in_force() = &U;
  // the bytes to read: what a BAI / CSI beside the BAM names for U (SVDSS_REGION_INDEX=0: the whole file, as without one)
  std::string index_path, stale;
  const bool want_index = !(getenv("SVDSS_REGION_INDEX") && atoi(getenv("SVDSS_REGION_INDEX")) == 0);
  if (want_index && find_bam_index(bam, index_path, stale)) {
    BaiIndex index;
    BamRegionPlan& plan = bam_region_plan();
    if (!index.load(index_path)) logmsg("warning", "cannot read the index " + index_path + ": the whole file is read");
    else if (!region_file_ranges(bam, index, U, plan.ranges, err)) logmsg("warning", err + ": the index is not used, the whole file is read");
    else { plan.active = true; plan.path = bam; plan.index_path = index_path; }
  }
  if (!stale.empty() && !bam_region_plan().active) logmsg("warning", "the index " + stale + " is older than " + bam + ": it is not used, the whole file is read");
  bam_region_counters().verbose = verbose;
}
static const char* INDEX_USAGE =
    "Usage: SVDSS index [-t threads] [-i <old.fmd>] -d <in.fa[.gz]> [<in2.fa[.gz]> ...] [-o <out.fmd>]\n"
    "      the FM-index of the records of every input and of their reverse complements, as `ropebwt3 build -d` writes it (rld0)\n"
    "      <in.fa> ...           one input or several (FASTA, gzip and BGZF ok): the records in command-line order, then file order\n"
    "      -i, --append <OLD>    the records of the index OLD first, then the inputs: from OLD.svdss where that is OLD's sidecar,\n"
    "                            else recovered from OLD's BWT on the GPU (an index of upstream `SVDSS index` / ropebwt3).  OLD is\n"
    "                            read completely before anything is written: -i x.fmd -o x.fmd works\n"
    "      -o <out.fmd>          the index, and beside it <out.fmd>.svdss (what `search` restores).  Without -o the .fmd goes to\n"
    "                            stdout (not a terminal) and no sidecar is written\n"
    "      -t <int>              threads of the host side (default: 4)\n"
    "      --verbose             where OLD's records came from, and how many\n";

static int build_index_files(const std::vector<std::string>& inputs, const std::string& old, const std::string& out, int threads, bool verbose);

static int main_index(int argc, char** argv) {
  // ropebwt3 `build` flags as run_svdss:142 passes them: -t T -d <fasta> -o <out>; -i <old> as ropebwt3 spells the index to
  // append to [UPSTREAM-UNVERIFIED], --append as the reference's config.hpp:22
  std::vector<std::string> inputs;
  std::string out, old;
  int threads = 4;
  bool verbose = false;
  for (int i = 2; i < argc; ++i) {
    if (!strcmp(argv[i], "--verbose")) verbose = true;
    else if (!strcmp(argv[i], "-t") && i + 1 < argc) threads = atoi(argv[++i]);
    else if (!strncmp(argv[i], "-t", 2) && argv[i][2]) threads = atoi(argv[i] + 2);
    else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
    else if ((!strcmp(argv[i], "-i") || !strcmp(argv[i], "--append")) && i + 1 < argc) old = argv[++i];
    else if (!strncmp(argv[i], "--append=", 9)) old = argv[i] + 9;
    else if (!strcmp(argv[i], "-d") || !strcmp(argv[i], "-b")) continue;  // output-format switches of ropebwt3
    else if (argv[i][0] == '-' && argv[i][1] == 'd' && argv[i][2]) continue;
    else if (argv[i][0] != '-') inputs.push_back(argv[i]);
  }
  if (inputs.empty() || (out.empty() && isatty(STDOUT_FILENO))) {
    fputs(INDEX_USAGE, stderr);
    return EXIT_FAILURE;
  }
  return build_index_files(inputs, old, out, threads, verbose);
}

// one line of `--verbose`: which encoder wrote the .fmd (svdss_fmd_encode_last)
static void report_fmd_encoder() {
  int32_t route = -1;
  int64_t runs = 0, blocks = 0, pieces = 0;
  double ms[6] = {0, 0, 0, 0, 0, 0};
  if (svdss_fmd_encode_last(&route, &runs, &blocks, &pieces, ms) != SVDSS_OK) return;
  if (route == SVDSS_FMD_DEVICE)
    fprintf(stderr, "fmd: encoded on the device: %lld runs, %lld blocks, %lld pieces; planes/plan/chain/emit/download %.1f/%.1f/%.1f/%.1f/%.1f ms\n",
            (long long)runs, (long long)blocks, (long long)pieces, ms[0], ms[1], ms[2], ms[3], ms[4]);
  else
    fprintf(stderr, "fmd: encoded on the host (%s)\n",
            route == SVDSS_FMD_DECLINED_EMPTY ? "the device declined: an empty BWT" :
            route == SVDSS_FMD_DECLINED_BLOCK ? "the device declined: a block of SVDSS_FMD_DECLINE_SYMS symbols or more" :
            route == SVDSS_FMD_DECLINED_MEMORY ? "the device declined: the plan does not fit in free HBM" :
            route == SVDSS_FMD_DECLINED_NO_GPU ? "the device declined: no GPU, or SVDSS_INDEX_CPU set" :
            "SVDSS_FMD_ENCODE_DEVICE=0");
}

// What `SVDSS index [-i old] -d inputs... [-o out] -t threads` does, for `index` and for `run --build-index` (out empty:
// the .fmd to stdout, no sidecar)
static int build_index_files(const std::vector<std::string>& inputs, const std::string& old, const std::string& out, int threads, bool verbose) {
  const bool to_stdout = out.empty();
  // The index is built in HBM.  Without a GPU the command fails instead of quietly taking the host builder (which
  // stays in the library for the texts the GPU builder refuses, and for SVDSS_INDEX_CPU=1: developer runs on a
  // machine without a GPU).
  if (svdss_device_count() <= 0 && !getenv("SVDSS_INDEX_CPU"))
    die("no GPU found: SVDSS index builds the index in HBM (SVDSS_INDEX_CPU=1 runs the host builder instead)");
  const bool dbg = getenv("SVDSS_DEBUG") != nullptr;
  const auto t_start = std::chrono::steady_clock::now();
  auto mark = [&](const char* what) {
    if (dbg) fprintf(stderr, "[index] %-28s at +%.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
  };
  std::vector<uint8_t> cat;
  std::vector<int64_t> lens;
  if (!old.empty()) {
    // OLD's records first -- read completely, and refused if it cannot be, before anything is opened for writing
    struct stat st;
    if (stat(old.c_str(), &st) != 0) die("cannot open " + old + " (the index to append to)");
    svdss_index_t* h = nullptr;
    int32_t source = -1;
    const int device = getenv("SVDSS_INDEX_CPU") || svdss_device_count() <= 0 ? -1 : 0;
    const int rc = svdss_index_records_open(old.c_str(), device, &h, &source);
    if (rc != SVDSS_OK) die(old + ": " + svdss_strerror(rc) + " " + svdss_last_hip_error());
    const uint8_t* rec = nullptr;
    const int64_t* rl = nullptr;
    int32_t nr = 0;
    check(svdss_index_records(h, &rec, &rl, &nr), "svdss_index_records");
    lens.assign(rl, rl + nr);
    int64_t total = 0;
    for (int64_t l : lens) total += l;
    cat.assign(rec, rec + total);
    svdss_index_free(h);
    if (verbose) {
      std::string from = source == 0 ? "its sidecar " + old + ".svdss" : source == 1 ? "this library's layout" : "";
      if (source >= 2) {
        int32_t route = -1;
        int64_t stride = 0, walkers = 0;
        double ms[3] = {0, 0, 0};
        (void)svdss_bwt_strings_last(&route, &stride, &walkers, ms);
        char buf[256];
        if (source == 4) snprintf(buf, sizeof buf, "its BWT by the host walk (one serial walk per string)");
        else snprintf(buf, sizeof buf, "its BWT by the %s walk (stride %lld, %lld walkers; pass 1 %.3f ms, pass 2 %.3f ms)", source == 2 ? "device" : "host",
                      (long long)stride, (long long)walkers, ms[1], ms[2]);
        from = buf;
      }
      logmsg("info", old + ": " + std::to_string(nr) + " record(s), " + std::to_string(total) + " bases from " + from);
    }
    mark("old index read");
  }
  for (const std::string& fasta : inputs) {
    const size_t had = lens.size();
    // a plain FASTA is mapped and read by several threads (fastx_reader.h, as `call` and `smooth` do), the records encoded
    // side by side into one buffer sized once; gzip / CRLF / FASTQ-like files go through the line reader as before
    std::vector<std::string> nm, sq;
    // (a BGZF file is inflated and parsed on the GPU first, ref_loader.h: upper-cased there, which svdss_nt6_encode does not mind)
    if (load_reference_device(fasta, threads < 8 ? 8 : threads, getenv("SVDSS_FASTA_SERIAL") != nullptr, verbose, "index", nm, sq, nullptr) ||
        (!getenv("SVDSS_FASTA_SERIAL") && load_fasta_mapped(fasta, std::max(1, std::min(threads < 8 ? 8 : threads, 16)), false, nm, sq))) {
      const size_t base = cat.size();
      std::vector<size_t> at(sq.size() + 1, base);
      for (size_t i = 0; i < sq.size(); ++i) { at[i + 1] = at[i] + sq[i].size(); lens.push_back((int64_t)sq[i].size()); }
      cat.resize(at.back());
      std::vector<std::thread> th;
      std::atomic<size_t> next(0);
      std::atomic<int> bad(0);
      for (int t = 0; t < (int)std::min<size_t>(sq.size(), 8); ++t)
        th.emplace_back([&] {
          for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= sq.size()) return;
            if (svdss_nt6_encode(sq[i].data(), (int64_t)sq[i].size(), cat.data() + at[i]) != SVDSS_OK) bad = 1;
            std::string().swap(sq[i]);
          }
        });
      for (std::thread& x : th) x.join();
      if (bad.load()) die("svdss_nt6_encode failed");
    } else {
      FastxReader fx(fasta);
      if (!fx.ok()) die("cannot open " + fasta);
      std::string name, seq;
      while (fx.next(name, seq)) {
        const size_t o = cat.size();
        cat.resize(o + seq.size());
        check(svdss_nt6_encode(seq.data(), (int64_t)seq.size(), cat.data() + o), "svdss_nt6_encode");
        lens.push_back((int64_t)seq.size());
      }
    }
    if (lens.size() == had) die("no sequence in " + fasta);
  }
  mark("FASTA read + nt6");
  logmsg("info", "Indexing " + std::to_string(lens.size()) + " record(s), " + std::to_string(cat.size()) + " bases..");
  svdss_index_t* ix = nullptr;
  check(svdss_index_build(cat.data(), lens.data(), (int32_t)lens.size(), threads, &ix), "svdss_index_build");
  mark("index built");
  // the file ropebwt3 build -d writes (rld0), so that the index serves upstream SVDSS as well -- and beside it the
  // records themselves (nt6), from which `search` rebuilds the index in HBM in less time than the text + suffix array
  // (19 bytes per base) take to read from any disk.  SVDSS_INDEX_FULL=1: the full layout instead (a plain read).
  // (the records sidecar is written beside the rld0 encoding, by a second thread: the two read different parts of the
  // index -- the BWT, the records -- and the encoder is one serial pass over six billion symbols at human scale)
  int rc_side = SVDSS_OK;
  std::thread side;
  if (to_stdout) {
    // no -o: the .fmd to stdout (rld0_write never seeks), no sidecar -- there is no name to put it under
    check(svdss_index_save_fmd(ix, "/dev/stdout"), "svdss_index_save_fmd");
    mark("rld0 .fmd written");
    if (verbose) report_fmd_encoder();
    svdss_index_free(ix);
    return 0;
  }
  const bool records_side = !getenv("SVDSS_INDEX_NO_CACHE") && !getenv("SVDSS_INDEX_FULL");
  // (an older sidecar must not outlive a failed rewrite of its .fmd: it goes first, and a failure takes the .tmp with it)
  if (!getenv("SVDSS_INDEX_NO_CACHE")) (void)unlink((out + ".svdss").c_str());
  // (round 6: behind the records the rank blocks -- the index as a rank structure alone, what a `search` with few reads to
  // search makes resident instead of rebuilding everything: svdss_index_attach_blocks; SVDSS_INDEX_NO_BLOCKS=1: records only)
  if (records_side) side = std::thread([&] {
    rc_side = svdss_index_save_records(ix, (out + ".svdss.tmp").c_str());
    if (rc_side == SVDSS_OK && !getenv("SVDSS_INDEX_NO_BLOCKS")) rc_side = svdss_index_append_blocks(ix, (out + ".svdss.tmp").c_str());
  });
  const int rc_fmd = svdss_index_save_fmd(ix, out.c_str());
  if (verbose && rc_fmd == SVDSS_OK) report_fmd_encoder();   // (this thread's encode: before anything else encodes here)
  if (side.joinable()) side.join();
  if (rc_fmd != SVDSS_OK || rc_side != SVDSS_OK) (void)unlink((out + ".svdss.tmp").c_str());
  check(rc_fmd, "svdss_index_save_fmd");
  mark("rld0 .fmd written");
  if (records_side) {
    check(rc_side, "svdss_index_save_records");
    // (renamed into place after the .fmd is complete: a sidecar is trusted only if it is not older than its .fmd)
    if (rename((out + ".svdss.tmp").c_str(), (out + ".svdss").c_str()) != 0 || utime((out + ".svdss").c_str(), nullptr) != 0)
      die("cannot write " + out + ".svdss");
  } else if (!getenv("SVDSS_INDEX_NO_CACHE")) {
    check(svdss_index_save(ix, (out + ".svdss").c_str()), "svdss_index_save");
  }
  mark("sidecar written");
  svdss_index_free(ix);
  return 0;
}

// `run --build-index`: the block run_svdss:136-147 of the reference's driver -- a missing index is built from the reference
// and stored, exactly as `SVDSS index -d FA -o FMD -t threads` would, before the smoothing stage starts.  An index that
// exists is not touched.  Refusals come before anything is opened for writing; a build that fails takes FMD, FMD.svdss and
// FMD.svdss.tmp with it (die_context) -- none of run's outputs exists at that point.  Called by main_run / main_run_samples
// (CallOptions::before_stages) after run's own refusals -- --gpus, the knobs it does not run with, a samples list that does
// not validate, a BAM that does not exist -- so that a command that is going to be refused does not build an index first.
static void build_missing_index(const CallOptions& o) {
  struct stat st;
  if (stat(o.index.c_str(), &st) == 0) return;
  if (access(o.reference.c_str(), R_OK) != 0) die("run --build-index: cannot read " + o.reference + " (the reference the index is built from)");
  const size_t slash = o.index.find_last_of('/');
  const std::string dir = slash == std::string::npos ? "." : slash == 0 ? "/" : o.index.substr(0, slash);
  if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || access(dir.c_str(), W_OK | X_OK) != 0)
    die("run --build-index: cannot write " + o.index + ": " + dir + " is not a directory that can be written to");
  if (svdss_device_count() <= 0 && !getenv("SVDSS_INDEX_CPU"))
    die("no GPU found: SVDSS index builds the index in HBM (SVDSS_INDEX_CPU=1 runs the host builder instead)");
  fprintf(stderr, "[run] [info] Building FMD index: %s\n", o.index.c_str());
  std::vector<std::string>& gone = die_context().unlink;
  const size_t had = gone.size();
  for (const char* suffix : {"", ".svdss", ".svdss.tmp"}) gone.push_back(o.index + suffix);
  if (build_index_files({o.reference}, "", o.index, o.threads, o.verbose) != 0) die("run --build-index: the index was not built");
  gone.resize(had);
}

int main(int argc, char** argv) {
  const time_t t0 = time(nullptr);
  // large blocks stay in the allocator instead of going back to the kernel with every free (with a hundred threads an
  // munmap is a stall for all of them)
  mallopt(M_MMAP_THRESHOLD, 32 << 20);
  mallopt(M_TRIM_THRESHOLD, 1 << 30);
  mallopt(M_TOP_PAD, 64 << 20);
  if (argc == 1) {
    fputs(MAIN_USAGE, stderr);
    return EXIT_FAILURE;
  }
  if (!strcmp(argv[1], "index")) {
    for (int i = 2; i < argc; ++i)
      if (!strncmp(argv[i], "--region", 8) && (argv[i][8] == 0 || argv[i][8] == '=' || !strncmp(argv[i] + 8, "s-file", 6)))
        die(std::string(argv[i]) + ": --region / --regions-file select records of a BAM by position: not an option of `SVDSS index`");
    for (int i = 2; i < argc; ++i)
      if (!strncmp(argv[i], "--write-bam-index", 17) && (argv[i][17] == 0 || argv[i][17] == '='))
        die("--write-bam-index is an option of `SVDSS call` and `SVDSS run` only, not of `SVDSS index`");
    for (int i = 2; i < argc; ++i)
      if (!strncmp(argv[i], "--build-index", 13) && (argv[i][13] == 0 || argv[i][13] == '='))
        die("--build-index is an option of `SVDSS run` only, not of `SVDSS index`");
    logmsg("info", "FM-index construction (stands for 'ropebwt3 build')");
    const int rc = main_index(argc, argv);
    if (rc) return rc;
  } else {
    for (int i = 1; i < argc; ++i)
      if (!strcmp(argv[i], "--version")) { printf("SVDSS, %s\n", VERSION); return EXIT_SUCCESS; }
    const Options o = parse(argc, argv);
    if (o.help) {   // Configuration::print_help(argv[1]), config.cpp:12-24: the mode's own usage text
      fputs(!strcmp(argv[1], "search") ? SEARCH_USAGE : !strcmp(argv[1], "call") ? CALL_USAGE :
            !strcmp(argv[1], "smooth") ? SMOOTH_USAGE : !strcmp(argv[1], "run") ? RUN_USAGE :
            !strcmp(argv[1], "bamindex") ? BAMINDEX_USAGE : MAIN_USAGE, stderr);
      return EXIT_SUCCESS;
    }
    if (o.nobam && strcmp(argv[1], "smooth") != 0) die(std::string("--nobam is an option of `SVDSS smooth` only, not of `SVDSS ") + argv[1] + "`");
    if (!o.write_index.empty() && strcmp(argv[1], "smooth") != 0 && strcmp(argv[1], "run") != 0)
      die(std::string("--write-index is an option of `SVDSS smooth` only, not of `SVDSS ") + argv[1] + "`");
    if (!o.smoothed.empty() && strcmp(argv[1], "run") != 0)
      die(std::string("--smoothed is an option of `SVDSS run` only, not of `SVDSS ") + argv[1] + "`");
    if (!o.samples.empty() && strcmp(argv[1], "run") != 0)
      die(std::string("--samples is an option of `SVDSS run` only, not of `SVDSS ") + argv[1] + "`");
    if (o.build_index && strcmp(argv[1], "run") != 0)
      die(std::string("--build-index is an option of `SVDSS run` only, not of `SVDSS ") + argv[1] + "`");
    // --write-bam-index FILE / bamindex -o FILE: what they do not go with, before anything is opened for writing
    const bool is_bamindex = !strcmp(argv[1], "bamindex");
    if (!o.out.empty() && !is_bamindex) die(std::string("-o is an option of `SVDSS bamindex` only, not of `SVDSS ") + argv[1] + "`");
    if (!o.write_bam_index.empty() && strcmp(argv[1], "call") != 0 && strcmp(argv[1], "run") != 0)
      die(std::string("--write-bam-index is an option of `SVDSS call` and `SVDSS run` only, not of `SVDSS ") + argv[1] + "`" +
          (is_bamindex ? " (its index is named by -o)" : ""));
    if (is_bamindex && o.bam.empty()) { fputs(BAMINDEX_USAGE, stderr); return EXIT_FAILURE; }
    const std::string bam_index_out = is_bamindex ? (o.out.empty() ? o.bam + ".bai" : o.out) : o.write_bam_index;
    if (!bam_index_out.empty()) {
      const char* opt = is_bamindex ? "bamindex -o" : "--write-bam-index";
      if (!o.regions.empty() || !o.regions_file.empty())
        die(std::string(opt) + " does not go with --region / --regions-file: a read bounded by an index sees part of the file, and the index is of the whole");
      if (!o.samples.empty()) die(std::string("run: --samples does not go with ") + opt + " (every sample's files are named by its line of the list)");
      for (const std::string* in : {&o.bam, &o.reference, &o.sfs, &o.index, &o.fastx})
        if (!in->empty() && same_file(*in, bam_index_out) && !(in == &o.sfs && !strcmp(argv[1], "run")))
          die(std::string(opt) + " " + bam_index_out + ": that is an input of the command");
      if (!is_bamindex && !o.bam.empty()) {   // (a BAI for a reference that is too long: said now, not after the pass)
        std::vector<int32_t> lens;
        std::string err;
        InputIndexFold probe;
        if (bam_header_lengths(o.bam, lens, err) && !probe.open(bam_index_out, lens, opt, err)) die(err);
      }
    }
    if (!strcmp(argv[1], "search") || !strcmp(argv[1], "call") || !strcmp(argv[1], "smooth") || !strcmp(argv[1], "run")) regions_in_force(o, argv[1]);
    if (!strcmp(argv[1], "search")) {
      if (o.index.empty() || (o.fastx.empty() && o.bam.empty())) { fputs(SEARCH_USAGE, stderr); return EXIT_FAILURE; }
      main_search(o, t0);
    } else if (!strcmp(argv[1], "call")) {
      if (o.reference.empty() || o.bam.empty() || o.sfs.empty()) { fputs(CALL_USAGE, stderr); return EXIT_FAILURE; }  // main.cpp:56-59
      CallOptions c;
      c.reference = o.reference; c.bam = o.bam; c.sfs = o.sfs; c.threads = o.threads; c.gpus = o.gpus;
      c.min_cluster_weight = o.min_cluster_weight; c.min_sv_length = o.min_sv_length; c.min_mapq = o.min_mapq;
      c.useht = o.useht; c.min_ratio = o.min_ratio; c.poa = o.poa; c.clusters = o.clusters; c.verbose = o.verbose;
      c.clipped = o.clipped; c.write_bam_index = o.write_bam_index;
      main_call(c);
    } else if (!strcmp(argv[1], "smooth")) {
      if (o.reference.empty() || o.bam.empty()) { fputs(SMOOTH_USAGE, stderr); return EXIT_FAILURE; }   // main.cpp:73-76
      // --index FMD --sfs FILE [--nobam]: refused here, before anything is opened or written
      if (o.sfs.empty() != o.index.empty()) die("smooth: --index and --sfs go together (--index <FMD> --sfs <FILE>)");
      if (o.nobam && o.sfs.empty()) die("smooth: --nobam needs --index <FMD> --sfs <FILE> (there would be no output at all)");
      if (o.nobam && !o.write_index.empty()) die("smooth: --nobam writes no BAM, so there is nothing for --write-index to index");
      CallOptions c;
      c.reference = o.reference; c.bam = o.bam; c.threads = o.threads; c.min_mapq = o.min_mapq; c.accp = o.accp; c.gpus = o.gpus;
      c.write_index = o.write_index; c.compress = o.compress;
      c.index = o.index; c.sfs = o.sfs; c.bsize = o.bsize; c.putative = o.putative; c.assemble = o.assemble; c.nobam = o.nobam;
      c.verbose = o.verbose;
      main_smooth(c);
    } else if (!strcmp(argv[1], "run")) {
      // --samples LIST: what it does not go with, before the list is looked at
      if (!o.samples.empty()) {
        const std::pair<const char*, bool> with[] = {{"--bam", !o.bam.empty()}, {"--sfs", !o.sfs.empty()}, {"--smoothed", !o.smoothed.empty()},
                                                     {"--write-index", !o.write_index.empty()}, {"--compress", o.compress_given}, {"--poa", !o.poa.empty()},
                                                     {"--clusters", !o.clusters.empty()}};
        for (const auto& w : with)
          if (w.second) die(std::string("run: --samples does not go with ") + w.first + " (every sample's files are named by its line of the list)");
      }
      if (o.reference.empty() || (o.bam.empty() && o.samples.empty()) || o.index.empty()) { fputs(RUN_USAGE, stderr); return EXIT_FAILURE; }
      if (!o.write_index.empty() && o.smoothed.empty()) die("run: --write-index needs --smoothed <FILE> (there is no BAM to index)");
      if (o.compress != 0 && o.smoothed.empty()) die("run: --compress needs --smoothed <FILE> (nothing is deflated without it)");
      CallOptions c;
      c.reference = o.reference; c.bam = o.bam; c.index = o.index; c.sfs = o.sfs; c.smoothed = o.smoothed; c.threads = o.threads; c.gpus = o.gpus;
      c.min_mapq = o.min_mapq; c.accp = o.accp; c.write_index = o.write_index; c.compress = o.compress;
      c.bsize = o.bsize; c.putative = o.putative; c.assemble = o.assemble;
      c.min_cluster_weight = o.min_cluster_weight; c.min_sv_length = o.min_sv_length; c.useht = o.useht; c.min_ratio = o.min_ratio;
      c.poa = o.poa; c.clusters = o.clusters; c.clipped = o.clipped; c.verbose = o.verbose; c.write_bam_index = o.write_bam_index;
      if (!main_run || !main_run_samples) die("this build of the binary has no `run` (run_host.cpp was left out)");
      if (o.build_index) c.before_stages = build_missing_index;
      if (o.samples.empty()) main_run(c);
      else main_run_samples(c, o.samples, o.regions, o.regions_file);
    } else if (is_bamindex) {
      CallOptions c;
      c.bam = o.bam; c.write_bam_index = bam_index_out; c.threads = o.threads; c.gpus = o.gpus; c.verbose = o.verbose;
      if (!main_bamindex) die("this build of the binary has no `bamindex` (bamindex_host.cpp was left out)");
      main_bamindex(c);
    } else {
      fputs(MAIN_USAGE, stderr);
      return EXIT_FAILURE;
    }
    bam_regions_report();
  }
  logmsg("info", "All done! Runtime: " + std::to_string((long)(time(nullptr) - t0)) + " seconds");
  return 0;
}
