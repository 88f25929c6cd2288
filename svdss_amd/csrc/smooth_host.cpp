// smooth_host.cpp -- `SVDSS smooth` (the reference's smoother.cpp): every primary, mapq-ok
// alignment is rewritten to equal the reference except at long (> 20 bp) indels and soft clips
// and tagged XF (0 smoothed & interesting, 1 too many mismatches, 2 nothing interesting); all
// other records are dropped; output order == input order; BAM on stdout.  A CIGAR walk with
// copies from the reference -- the reference has no alignment DP here.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <chrono>
#include <string>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <thread>
#include <unordered_map>
#include <vector>

#define SVDSS_LOG_TAG "smooth"
#include "host_common.h"
#include "host_knobs.h"
#include "bam_reader.h"
#include "bam_aux_walk.h"
#include "bam_device_select.h"
#include "bam_input_index.h"
#include "gpu_deflate_hook.h"
#include "gpu_inflate_hook.h"
#include "bam_writer.h"
#include "bam_index_writer.h"
#include "call_host.h"
#include "fastx_reader.h"
#include "ref_loader.h"
#include "sfs_units.h"

namespace {
const int MIN_INDEL = 20;   // config.hpp:95

bool is_m(uint32_t op) { return op == 0 || op == 7 || op == 8; }

// the walks of this file index ref[pos ..] and the read by the CIGAR: true if the alignment stays inside its contig and
// its CIGAR adds up to the read (what is not is passed through with XF = 3 and left out of the accuracy percentile)
void cigar_spans(const BamRecord& r, size_t& rl, size_t& ql) {   // bases of the reference / of the read the CIGAR covers
  rl = ql = 0;
  for (uint32_t c : r.cigar) {
    const uint32_t l = c >> 4, op = c & 0xf;
    if (is_m(op)) { rl += l; ql += l; }
    else if (op == 1 || op == 4) ql += l;
    else if (op == 2) rl += l;
    else break;
  }
}
bool cigar_fits(const BamRecord& r, size_t seq_len, size_t ref_len) {
  size_t rl, ql;
  cigar_spans(r, rl, ql);
  return r.pos >= 0 && (size_t)r.pos + rl <= ref_len && ql == seq_len;
}

// percentile() of smoother.cpp:246-255 (compute_maxaccuracy's threshold); sorts v; 0 for no values
double percentile(std::vector<double>& v, double p) {
  if (v.empty()) return 0.0;
  std::sort(v.begin(), v.end());
  const double id = (double)(v.size() - 1) * p;
  const double lo = floor(id), hi = ceil(id), h = id - lo;
  return (1.0 - h) * v[(size_t)lo] + h * v[(size_t)hi];
}

void mismatch_counts(const BamRecord& r, const std::string& seq, const std::string& ref, double& nm, double& nx) {
  size_t ref_off = (size_t)r.pos, q_off = 0;
  nm = nx = 0;
  for (uint32_t c : r.cigar) {
    const uint32_t l = c >> 4, op = c & 0xf;
    if (is_m(op)) {
      for (uint32_t j = 0; j < l; ++j) (ref[ref_off + j] == seq[q_off + j]) ? ++nm : ++nx;
      ref_off += l; q_off += l;
    } else if (op == 1 || op == 4) q_off += l;
    else if (op == 2) ref_off += l;
    else break;
  }
}

// bam_aux_update_int(aln, "XF", v): overwrite an existing integer XF, else append XF:C; an aux block the walk gives up on
// (bam_aux_walk.h) is left as it is
void set_xf(std::vector<uint8_t>& aux, int v) {
  int32_t n = 0;
  const int64_t at = svdss_aux_find_int(aux.data(), aux.data() + aux.size(), 'X', 'F', n);
  if (at == SVDSS_AUX_BAD) return;
  if (at >= 0) {
    memset(&aux[(size_t)at], 0, (size_t)n);
    aux[(size_t)at] = (uint8_t)v;
    return;
  }
  aux.push_back('X'); aux.push_back('F'); aux.push_back('C'); aux.push_back((uint8_t)v);
}

// grow-only buffer for what goes to / comes from the GPU in every batch: page-locked when the runtime gives it (the
// copies then run at PCIe speed), never zero-filled
struct PinBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
  bool pinned = false;
  ~PinBuf() { release(); }
  void release() {
    if (!p) return;
    if (pinned) svdss_host_free(p); else free(p);
    p = nullptr; cap = 0;
  }
  uint8_t* ensure(size_t n) {
    if (n <= cap) return p;
    release();
    const size_t want = n + n / 4 + 4096;
    void* q = nullptr;
    if (svdss_host_alloc((int64_t)want, &q) == SVDSS_OK && q) { p = (uint8_t*)q; pinned = true; }
    else { p = (uint8_t*)malloc(want); pinned = false; if (!p) { fprintf(stderr, "[smooth] [critical] out of memory\n"); exit(EXIT_FAILURE); } }
    cap = want;
    return p;
  }
};

struct ByteSink {
  std::vector<uint8_t> v;
  void write(const void* p, size_t n) { v.insert(v.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
};

// one record with the bases already in BAM's 4-bit form
void write_record_packed(ByteSink& w, const BamRecord& r, const uint32_t* cigar, size_t n_cigar, const uint8_t* packed,
                         int32_t l_seq, const uint8_t* qual, const std::vector<uint8_t>& aux) {
  // BAM keeps l_read_name in 8 bits and n_cigar_op in 16 (longer CIGARs live in a CG tag, which this writer does not
  // produce): refuse instead of writing a record that no longer parses
  if (r.qname.size() + 1 > 255) die("read name longer than 254 characters: " + r.qname);
  if (n_cigar > 65535) die("more than 65535 CIGAR operations (CG tag records are not supported): " + r.qname);
  const uint8_t l_name = (uint8_t)(r.qname.size() + 1);
  const uint16_t n_cig = (uint16_t)n_cigar;
  const size_t pbytes = ((size_t)l_seq + 1) / 2;
  const int32_t block = 32 + l_name + 4 * n_cig + (int32_t)pbytes + l_seq + (int32_t)aux.size();
  uint8_t core[36];
  memcpy(core, &block, 4);
  memcpy(core + 4, &r.tid, 4);
  memcpy(core + 8, &r.pos, 4);
  core[12] = l_name; core[13] = r.mapq;
  memcpy(core + 14, &r.bin, 2);
  memcpy(core + 16, &n_cig, 2);
  memcpy(core + 18, &r.flag, 2);
  memcpy(core + 20, &l_seq, 4);
  memcpy(core + 24, &r.mtid, 4);
  memcpy(core + 28, &r.mpos, 4);
  memcpy(core + 32, &r.isize, 4);
  w.v.reserve(w.v.size() + 4 + (size_t)block);   // (one allocation per record instead of a doubling series)
  w.write(core, 36);
  w.write(r.qname.c_str(), l_name);
  if (n_cig) w.write(cigar, 4u * n_cig);
  w.write(packed, pbytes);
  w.write(qual, (size_t)l_seq);
  w.write(aux.data(), aux.size());
}

void write_record(ByteSink& w, const BamRecord& r, const std::vector<uint32_t>& cigar, const std::string& seq,
                  const std::vector<uint8_t>& qual, const std::vector<uint8_t>& aux) {
  const int32_t l_seq = (int32_t)seq.size();
  std::vector<uint8_t> packed(((size_t)l_seq + 1) / 2, 0);
  static const struct Lut {   // (initialised once, before any worker thread runs: function-local static)
    uint8_t t[256];
    Lut() {
      memset(t, 15, sizeof t);
      const char* nt16 = "=ACMGRSVTWYHKDBN";
      for (int i = 0; i < 16; ++i) { t[(uint8_t)nt16[i]] = (uint8_t)i; t[(uint8_t)tolower(nt16[i])] = (uint8_t)i; }
    }
  } lut_obj;
  const uint8_t* lut = lut_obj.t;
  for (int32_t i = 0; i < l_seq; ++i) packed[(size_t)i >> 1] |= (uint8_t)(lut[(uint8_t)seq[(size_t)i]] << ((~i & 1) << 2));
  write_record_packed(w, r, cigar.data(), cigar.size(), packed.data(), l_seq, qual.data(), aux);
}

// ---- `smooth --index FMD --sfs FILE`: the search of the smoothed reads beside the smoothing.  The device path leaves, per
// batch, what `search`'s front end would have read from the smoothed BAM (svdss_bam_smooth_set_search): names and tags on
// the host, the reads to search in a park in HBM.  A side thread makes the index resident from process start on; until it
// is, the reads wait in the park (a full park: the feeding threads wait for the index); a drain thread searches the park's
// groups, one launch each; batches that found the index resident are searched by their feeding thread.  Finished batches
// go to the assembler in file order -- whenever they finish, without a bound: the BAM's hand-over never waits for a search
// -- and from there through search's own units, format_batch and ordered writer into FILE.
class SfsSide {
 public:
  SfsSide(const CallOptions& c, FILE* sink, bool debug, SmoothHooks* hooks = nullptr) : hooks_(hooks && hooks->session ? hooks : nullptr), sink_(sink) {
    o_.index = c.index; o_.bam = c.bam; o_.threads = std::max(1, c.threads); o_.bsize = c.bsize; o_.putative = c.putative; o_.assemble = c.assemble;
    o_.verbose = c.verbose || debug;
    flags_ = (o_.assemble ? SVDSS_SFS_ASSEMBLE : 0) | (o_.putative ? SVDSS_BAM_PUTATIVE : 0);
    struct stat stb;
    early_.file_bytes = stat(c.bam.c_str(), &stb) == 0 ? (int64_t)stb.st_size : 0;
    if (hooks_) svdss_index_kmer_limit(0);   // (process-wide, for tables built from now on: what the sample before learnt is not this one's)
    index_thread_ = std::thread([this] { make_index_resident(); });
  }
  int32_t flags() const { return flags_; }
  // the park, allocated before the stream starts (the device's context must be up)
  svdss_bam_park_t* create_park() {
    check(svdss_bam_park_create(0, knobs_.park_bytes, knobs_.park_bytes / 512 + 4096, &early_.park), "svdss_bam_park_create");
    return early_.park;
  }
  // the stream starts: the threads behind the feeders
  void begin() {
    writer_.reset(new OrderedWriter(units_.pool(), sink_));
    drain_ = std::thread([this] { drain_park(); });
    assembler_ = std::thread([this] { assemble(); });
    for (int k = 0; k < (knobs_.format_threads ? knobs_.format_threads : 5); ++k) fmt_.emplace_back([this] { units_.format_units(*writer_); });
  }
  // feeding thread, after a batch's smoothing run: a batch that found no room in the park waits for the index and is searched here
  int after_run(svdss_bam_batch_t* batch, int64_t comp_bytes) {
    int64_t grp = -1;
    check(svdss_bam_batch_parked(batch, &grp, nullptr, nullptr), "svdss_bam_batch_parked");
    svdss_bam_result_t r0;
    check(svdss_bam_batch_result(batch, &r0), "svdss_bam_batch_result");
    early_.note_batch(r0.n_records, r0.n_searched, comp_bytes);
    if (grp != -1) return SVDSS_OK;     // (parked, or nothing to search)
    ++n_direct_;
    return svdss_bam_smooth_search(batch, early_.wait_for_index());
  }
  // feeding thread, with the batch's results: to the assembler, or to wait for its group's search
  void collect(const svdss_bam_batch_t* batch, uint64_t seq) {
    int64_t grp = -1, first = 0, n_srch = 0;
    // (a batch its feeding thread has searched no longer answers svdss_bam_batch_parked: its front half is used up, it is
    // complete -- as in DevicePath::collect of search_host.cpp)
    const bool parked = svdss_bam_batch_parked(batch, &grp, &first, &n_srch) == SVDSS_OK && grp >= 0;
    svdss_bam_result_t r;
    check(svdss_bam_batch_result(batch, &r), "svdss_bam_batch_result");
    std::unique_ptr<DevOut> out = unpack_result(r, parked);
    if (parked) early_.add_pending(grp, EarlySearch::Pending{seq, std::move(out), first, n_srch});
    else deliver(seq, std::move(out));
  }
  // every batch of the file (n_batches of them) has been collected: the rest of the park, the rest of the text
  void finish(uint64_t n_batches) {
    early_.front_finished();
    index_thread_.join();
    drain_.join();
    { std::lock_guard<std::mutex> lk(m_); total_ = n_batches; total_known_ = true; }
    cv_.notify_all();
    assembler_.join();
    for (std::thread& t : fmt_) t.join();
    writer_->finish();
    if (writer_->failed() || fclose(sink_) != 0) die("error writing the SFS file");
    if (o_.verbose) {
      char buf[400];
      snprintf(buf, sizeof buf, "sfs: %lld reads parked in %lld batch(es), %lld group(s) searched (%.3f s), %lld batch(es) searched by their feeding thread; index resident "
               "at +%.3f s (%s); %llu SFS lines written; re-dealing %.3f s, format %.3f s, write %.3f s", (long long)n_parked_, (long long)n_parked_batches_,
               (long long)n_groups_, t_park_search_, (long long)n_direct_.load(), t_resident_, lf_only_ ? "rank blocks alone" : "full restore",
               (unsigned long long)writer_->lines(), t_.assemble, t_.format, writer_->busy_seconds());
      logmsg("debug", buf);
    }
  }
  // `SVDSS run`, after finish(): the index and the park leave HBM before `call` takes its workspaces
  // (`run --samples`: the index stays, through the call stage and for the next sample)
  void free_index_and_park() {
    svdss_index_t* const ix = early_.wait_for_offered_index();
    if (!hooks_) svdss_index_free(ix);
    svdss_bam_park_free(early_.park);
    early_.park = nullptr;
  }
 private:
  // the side thread: the index file, the form it becomes resident in (SVDSS_KMER, SVDSS_SEARCH_LF, SVDSS_SEARCH_LF_MAX as
  // for `search`; the estimate of the reads to search runs on the XF counts the batches bring), then to the feeders
  void make_index_resident() {
    if (hooks_) { make_session_index_resident(); return; }
    svdss_index_t* ix = nullptr;
    check(svdss_index_load(o_.index.c_str(), &ix), "svdss_index_load");
    early_.index_n.store(svdss_index_size(ix));
    const bool user_kmer = choose_kmer_order(o_.bam, true, ix, o_.verbose);
    lf_only_ = choose_rank_blocks_alone(knobs_, early_, ix, o_.index, user_kmer, o_.verbose, clock_);
    check(svdss_index_to_device(ix, 0), "svdss_index_to_device");
    t_resident_ = secs(clock_.t0, now());
    // (the rank blocks alone: held back from the feeders until the file is through or the park is full, so that what is
    // parked goes in large launches; the drain thread has the index at once)
    if (lf_only_) early_.offer_index_held_back(ix);
    if (knobs_.early_hold_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(knobs_.early_hold_ms));
    early_.release_index(ix);
  }
  // ... of `run --samples`: the index file is read by the first sample; what is resident is reused -- the rank blocks alone
  // only while this sample's own estimate still asks for them, else the full restore is made from the records kept on the
  // host and stays.  Reused, the index is there from the start: it is held back from the feeders as the rank blocks are, so
  // that the reads are parked and searched one launch per group, not one small segmented launch per device batch.
  void session_note(const std::string& m) const { if (o_.verbose) fprintf(stderr, "[run] index: %s\n", m.c_str()); }
  void make_session_index_resident() {
    SmoothHooks& h = *hooks_;
    if (!h.index_host) {
      check(svdss_index_load(o_.index.c_str(), &h.index_host), "svdss_index_load");
      ++h.n_index_reads;
      session_note("file read, " + std::to_string((long long)svdss_index_size(h.index_host)) + " symbols");
    }
    const int64_t n = svdss_index_size(h.index_host);
    early_.index_n.store(n);
    const bool reused_full = h.index && !h.index_rank_only;
    if (!reused_full) {
      const bool kmer_was_set = getenv("SVDSS_KMER") != nullptr;
      const bool user_kmer = choose_kmer_order(o_.bam, true, h.index_host, o_.verbose);
      double est = -1;
      std::string t_est;
      bool lf = wants_rank_blocks_alone(knobs_, early_, n, user_kmer, clock_, est, t_est);
      const std::string what = "~" + std::to_string((long long)std::max(0.0, est)) + " reads to search (known at +" + t_est + " s)";
      if (lf && !h.index) {
        const int rc = svdss_index_load_blocks(o_.index.c_str(), &h.index);
        if (rc == SVDSS_OK && svdss_index_size(h.index) != n) { svdss_index_free(h.index); h.index = nullptr; }
        else if (rc != SVDSS_OK && rc != SVDSS_EINVAL) check(rc, "svdss_index_load_blocks");
        if (h.index) {
          check(svdss_index_to_device(h.index, 0), "svdss_index_to_device");
          h.index_rank_only = true;
          session_note(what + ": rank blocks alone made resident");
        } else lf = false;    // (no such section in the file: restore as before)
      } else if (lf) session_note(what + ": resident index reused (rank blocks alone)");
      if (!lf) {
        if (h.index) {
          session_note(what + ": full restore replaces the rank blocks alone");
          svdss_index_free(h.index);
        }
        h.index = nullptr;
        check(svdss_index_to_device(h.index_host, 0), "svdss_index_to_device");
        h.index = h.index_host;
        h.index_rank_only = false;
        session_note("full restore made resident");
      }
      // (the order choose_kmer_order asked for was this sample's: the next full restore, if there is one, asks again)
      if (!kmer_was_set) unsetenv("SVDSS_KMER");
    } else session_note("resident index reused (full restore)");
    lf_only_ = h.index_rank_only;
    t_resident_ = secs(clock_.t0, now());
    early_.offer_index_held_back(h.index);
    if (knobs_.early_hold_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(knobs_.early_hold_ms));
    early_.release_index(h.index);
  }
  void deliver(uint64_t seq, std::unique_ptr<DevOut> out) {
    { std::lock_guard<std::mutex> lk(m_); ready_[seq] = std::move(out); }
    cv_.notify_all();
  }
  void assemble() {
    units_.begin();
    for (uint64_t want = 0;; ++want) {
      std::unique_ptr<DevOut> d;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return ready_.count(want) || (total_known_ && want >= total_); });
        auto it = ready_.find(want);
        if (it == ready_.end()) break;
        d = std::move(it->second);
        ready_.erase(it);
      }
      units_.deal(*d);
    }
    units_.end();
  }
  // the park's groups, ONE launch each: those that close while the index is held back from the feeders, and -- once the
  // feeders have it and the park is closed -- whatever is left (DevicePath::drain_park of search_host.cpp)
  void drain_park() {
    svdss_index_t* ix = early_.wait_for_offered_index();
    svdss_sfs_batch_t* sfs = nullptr;
    std::vector<int64_t> counts, prefix;
    std::vector<int32_t> qs, ln;
    bool closed = false;
    int64_t n_groups = 0;
    for (int64_t g = 0;; ++g) {
      for (;;) {
        if (!closed && early_.released()) {
          check(svdss_bam_park_close(early_.park), "svdss_bam_park_close");
          closed = true;
          n_groups = svdss_bam_park_groups(early_.park);
        }
        if (closed || svdss_bam_park_group_ready(early_.park, g)) break;
        early_.nap();
      }
      if (closed && g >= n_groups) break;
      int64_t nb = 0, nr = 0, ns = 0;
      check(svdss_bam_park_group(early_.park, g, &nb, &nr, &ns), "svdss_bam_park_group");
      const auto t0 = now();
      check(svdss_bam_park_search(early_.park, g, ix, flags_, &sfs), "svdss_bam_park_search");
      const int64_t total = svdss_sfs_batch_total(sfs);
      counts.resize((size_t)nr); qs.resize((size_t)total); ln.resize((size_t)total);
      check(svdss_sfs_batch_fetch(sfs, counts.data(), qs.data(), ln.data(), nullptr), "svdss_sfs_batch_fetch");
      t_park_search_ += secs(t0, now());
      prefix.assign((size_t)nr + 1, 0);
      for (int64_t i = 0; i < nr; ++i) prefix[(size_t)i + 1] = prefix[(size_t)i] + counts[(size_t)i];
      for (EarlySearch::Pending& P : early_.take_group(g, nb)) {
        fill_parked(P, counts, prefix, qs, ln);
        deliver(P.seq, std::move(P.out));
      }
      n_parked_ += nr; n_parked_batches_ += nb; ++n_groups_;
    }
    if (sfs) svdss_sfs_batch_free(sfs);
  }

  SmoothHooks* const hooks_;   // `run --samples` only: where the index lives between samples
  Options o_;
  const SearchKnobs knobs_{};
  const Stopwatch clock_{};
  FILE* const sink_;
  int32_t flags_ = 0;
  EarlySearch early_;
  StageSeconds t_;
  UnitAssembler units_{o_, t_};
  std::unique_ptr<OrderedWriter> writer_;
  std::mutex m_;
  std::condition_variable cv_;
  std::map<uint64_t, std::unique_ptr<DevOut>> ready_;   // finished batches the assembler has not reached yet
  uint64_t total_ = 0;
  bool total_known_ = false;
  bool lf_only_ = false;
  double t_resident_ = 0, t_park_search_ = 0;
  int64_t n_parked_ = 0, n_parked_batches_ = 0, n_groups_ = 0;
  std::atomic<int64_t> n_direct_{0};
  std::thread index_thread_, drain_, assembler_;
  std::vector<std::thread> fmt_;
};

// run f(t, nt) on nt threads, this one among them
template <class F>
void on_threads(size_t nt, F&& f) {
  if (nt <= 1) { f((size_t)0, (size_t)1); return; }
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nt; ++t) pool.emplace_back([&f, t, nt] { f(t, nt); });
  f((size_t)0, nt);
  for (std::thread& th : pool) th.join();
}

// the BAM's header as the host reader gives it, read beside the FASTA for the device path and --write-index
struct HeaderPre { std::string text, err; std::vector<std::string> names; std::vector<int32_t> lens; int32_t n_ref = 0; int64_t skip = 0; };

// `SVDSS smooth`, stage by stage; the members are what one stage hands to the next.
// hooks (`SVDSS run`, run_host.cpp): the device path also fills a record store for `call`, the SFS text goes to the hooks'
// sink, and run() returns -- the process and the GPU context stay -- with the chromosomes handed over
struct SmoothRun {
  const CallOptions& o;
  SmoothHooks* const hooks;
  const SmoothKnobs knobs{};
  std::unique_ptr<SfsSide> side;         // --index FMD --sfs FILE
  svdss_bam_park_t* park = nullptr;
  std::unordered_map<std::string, std::string> chrom;
  RefOnDevice ref_dev;                   // where the GPU read the FASTA (ref_loader.h): its output, for GPU 0's copy of the chromosomes
  HeaderPre hp;
  bool ix_csi = false;                   // --write-index FILE: the scheme, and what collects the index
  int ix_shift = 14, ix_depth = 5;
  std::unique_ptr<BamIndexBuilder> ixb;
  const TimePoint t_fasta0 = now();
  double fasta_s = 0;
  TimePoint t_start;                     // the clock of the `+%.3f s` debug lines
  double since() const { return secs(t_start, now()); }
  SmoothRun(const CallOptions& opt, SmoothHooks* h) : o(opt), hooks(h) {}
  bool eligible(const BamRecord& r, const std::vector<std::string>& names) const {
    if (r.flag & (4 | 2048 | 256)) return false;
    if ((unsigned)r.mapq < o.min_mapq || r.l_seq < 2) return false;
    if (r.tid < 0) die("core.tid < 0. Why are we here? Please check");
    return r.tid < (int)names.size() && chrom.count(names[(size_t)r.tid]) > 0;
  }
  // --index FMD --sfs FILE: what it cannot run on is said before FILE or anything else is created; then the index is on its
  // way from the first moment
  void refuse_and_open_sfs() {
    if (hooks && hooks->sfs_sink) { side.reset(new SfsSide(o, hooks->sfs_sink, knobs.debug, hooks)); return; }   // (`SVDSS run` has refused what cannot run)
    if (o.sfs.empty()) return;
    if (o.gpus != 1) die("smooth --index --sfs with --gpus other than 1 is out of scope: run it on one GPU");
    if (!knobs.no_device_path().empty())
      die("smooth --index --sfs needs the device path: it does not run with SVDSS_SMOOTH_HOST=1, SVDSS_BAM_DEVICE=0 or SVDSS_GPU_DEFLATE=0");
    if (svdss_device_count() <= 0) die("no GPU found: smooth --index --sfs searches the smoothed reads on the GPU");
    if (o.bsize <= 0) die("batch size smaller than the number of threads");
    FILE* f = fopen(o.sfs.c_str(), "wb");
    if (!f) die("cannot write " + o.sfs);
    side.reset(new SfsSide(o, f, knobs.debug));
  }
  // the HIP runtime and the device's context come up (a few tenths of a second), and the BAM's header is read (0.3 s through
  // the host reader: its workers, its first chunks), while this thread reads the FASTA (load_chromosomes, fastx_reader.h)
  void warm_up_and_load() {
    std::thread gpu_warm([] {
      void* q = nullptr;
      if (svdss_device_count() > 0 && svdss_host_alloc(1 << 20, &q) == SVDSS_OK && q) svdss_host_free(q);
    });
    std::thread header_pre([this] {
      BamReader hb(o.bam);
      if (!hb.ok() || !hb.read_header()) { hp.err = "cannot read " + o.bam + ": " + hb.error(); return; }
      hp.text = hb.header_text(); hp.names = hb.ref_names(); hp.lens = hb.ref_lens();
      std::string perr;
      if (!bam_header_probe(o.bam, hp.n_ref, hp.skip, perr, nullptr)) { hp.err = "cannot read " + o.bam + ": " + perr; return; }
      if ((size_t)hp.n_ref != hp.names.size()) hp.err = "cannot read " + o.bam + ": inconsistent header";
    });
    std::vector<std::string> names;
    if (hooks && hooks->session && !hooks->chrom_names.empty()) chrom = std::move(hooks->chrom_seqs);   // (read by a sample before)
    else {
      if (!load_chromosomes(o.reference, o.threads, knobs.fasta_serial, o.verbose, "smooth", names, chrom, &ref_dev)) die("cannot open " + o.reference);
      if (hooks) { hooks->chrom_names = std::move(names); ++hooks->n_fasta_reads; }
      if (hooks && hooks->session && (o.verbose || knobs.debug)) fprintf(stderr, "[run] reference: FASTA read, %zu sequence(s)\n", chrom.size());
    }
    gpu_warm.join();
    header_pre.join();
  }
  // --write-index FILE: the scheme from the header's references, refused before anything is written; the index goes to
  // FILE only once the BAM's EOF marker is out (any failure before leaves no index)
  void plan_index() {
    if (o.write_index.empty()) return;
    if (!hp.err.empty()) die(hp.err);
    std::string err;
    if (!bam_index_scheme(o.write_index, hp.lens, ix_csi, ix_shift, ix_depth, err)) die(err);
    ixb.reset(new BamIndexBuilder((int32_t)hp.lens.size(), ix_csi, ix_shift, ix_depth));
  }
  void write_index() {
    std::string err;
    if (ixb && !ixb->write(o.write_index, err)) die(err);
  }
  // The device path (csrc/bam_smooth.hip): compressed blocks up, compressed blocks down.  SVDSS_BAM_DEVICE=0 (or
  // SVDSS_SMOOTH_HOST=1): the host pipeline, which writes the same bytes; SVDSS_GPU_DEFLATE=0 asks for the host's deflate,
  // which is the host pipeline's writer (`SVDSS run` without --smoothed deflates nothing, on either side)
  bool takes_device_path() const { return svdss_device_count() > 0 && knobs.no_device_path(!(hooks && o.nobam)).empty(); }
  // the end of a pipeline's run(), with its objects still standing: back to `SVDSS run` with the chromosomes, or the end of
  // the process (the teardown of page-locked buffers is left to the OS, see main_search; SVDSS_CLEAN_EXIT: an orderly return)
  int finish_process() {
    if (hooks && hooks->keep_alive) { hooks->chrom_seqs = std::move(chrom); return 0; }
    if (knobs.clean_exit) return 0;
    bam_regions_report();
    fprintf(stderr, "[smooth] [info] All done!\n");
    fflush(stdout);
    fflush(stderr);
    _exit(0);
  }
  int run();
};

// The BGZF members of a batch come down into a page-locked buffer of this pool and are written from it: no copy on the
// way.  (The pool is the first region's: a later region's members wait in plain memory until the regions in front are
// written, and would hold every buffer of the pool while the first region's feeders wait for one.)
struct OutputPool {
  std::mutex m; std::condition_variable cv;
  std::vector<uint8_t*> buf; std::vector<int> free_;
  const size_t cap;
  const int max_n;
  int n_made = 0;
  bool broken = false;
  // (literals-only members: at most ~1.001 x the records, which grow by 4 bytes each)
  OutputPool(int64_t target, int feeders) : buf((size_t)feeders + 6, nullptr), cap((size_t)target + (size_t)target / 8 + ((size_t)32 << 20)), max_n(feeders + 6) {}
  // a free buffer; while fewer than max_n exist a new one is made instead of waiting (by the feeding thread that needs
  // it: page-locking a tenth of a gigabyte takes tens of milliseconds, and the feeders start one after the other)
  int take() {
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
      if (!free_.empty()) { const int k = free_.back(); free_.pop_back(); return k; }
      if (broken) return -1;
      if (n_made < max_n) {
        const int k = n_made++;
        lk.unlock();
        void* q = nullptr;
        const bool ok = svdss_host_alloc((int64_t)cap, &q) == SVDSS_OK && q;
        lk.lock();
        if (!ok) { broken = true; cv.notify_all(); return -1; }
        buf[(size_t)k] = (uint8_t*)q;
        return k;
      }
      cv.wait(lk);
    }
  }
  void give(int k) { { std::lock_guard<std::mutex> lk(m); free_.push_back(k); } cv.notify_all(); }
  void free_all() { for (uint8_t*& q : buf) if (q) { svdss_host_free(q); q = nullptr; } }
};

// The batches, in file order, to stdout.  When stdout is a regular file they are written side by side (pwrite at the
// offsets the ordered hand-over gives them: one thread copying into the page cache is slower than the GPU side); a pipe
// gets them in order.
class BatchWriter {
 public:
  BatchWriter(OutputPool& pool, bool nobam, const SmoothKnobs& knobs) : pool_(pool), nobam_(nobam), knobs_(knobs) {}
  void open() {
    fflush(stdout);
    const off_t pos0 = lseek(STDOUT_FILENO, 0, SEEK_CUR);
    struct stat sb;
    // (pwrite ignores its offset on an O_APPEND descriptor -- `SVDSS smooth ... >> out.bam` -- and the batches would land in
    // completion order: such a stdout takes the ordered path)
    const int fl = fcntl(STDOUT_FILENO, F_GETFL);
    seekable_ = !nobam_ && pos0 >= 0 && fstat(STDOUT_FILENO, &sb) == 0 && S_ISREG(sb.st_mode) && fl >= 0 && !(fl & O_APPEND) && !knobs_.serial_write;
    at_ = pos0 < 0 ? 0 : pos0;
    if (seekable_)
      for (int t = 0; t < knobs_.writers; ++t) writers_.emplace_back([this] { write_jobs(); });
  }
  void put(std::unique_ptr<SelectedBatch> b) {
    const size_t nb = b->ext ? b->ext_n : b->bytes.size();
    if (seekable_) q_.push(std::unique_ptr<Job>(new Job{std::move(b), at_}));
    else {
      const uint8_t* p = b->ext ? b->ext : b->bytes.data();
      if (nb && fwrite(p, 1, nb, stdout) != nb) ok_ = false;
      if (b->ext) pool_.give(b->ext_slot);
    }
    at_ += (off_t)nb;
  }
  void close() {
    q_.close();
    for (std::thread& t : writers_) t.join();
    if (seekable_ && lseek(STDOUT_FILENO, at_, SEEK_SET) < 0) ok_ = false;   // (the EOF marker goes behind the last batch)
  }
  void fail() { ok_ = false; }
  bool ok() const { return ok_; }
 private:
  struct Job { std::unique_ptr<SelectedBatch> b; off_t at; };
  void pwrite_all(const uint8_t* p, size_t n, off_t at) {
    while (n) {
      const ssize_t w = pwrite(STDOUT_FILENO, p, n, at);
      if (w <= 0) { ok_ = false; return; }
      p += w; n -= (size_t)w; at += w;
    }
  }
  void write_jobs() {
    while (std::unique_ptr<Job> j = q_.pop()) {
      if (j->b->ext) { pwrite_all(j->b->ext, j->b->ext_n, j->at); pool_.give(j->b->ext_slot); }
      else pwrite_all(j->b->bytes.data(), j->b->bytes.size(), j->at);
    }
  }
  OutputPool& pool_;
  const bool nobam_;
  const SmoothKnobs& knobs_;
  bool seekable_ = false;
  off_t at_ = 0;
  std::atomic<bool> ok_{true};   // (set by several writer threads)
  BoundedQueue<Job> q_{4};       // (the reader runs at most four batches ahead of the writers)
  std::vector<std::thread> writers_;
};

// The reader of the smoothing pass starts FIRST: its loaders page-lock their slabs and read ahead while the reference
// goes up and the accuracy pass runs; its feeding threads wait at this gate for the threshold.
struct Gate {
  std::mutex m; std::condition_variable cv; bool is_open = false;
  void wait() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return is_open; }); }
  void open() { { std::lock_guard<std::mutex> lk(m); is_open = true; } cv.notify_all(); }
};

// The device path (csrc/bam_smooth.hip): the records are filtered, measured, smoothed, rebuilt and deflated in HBM.  The
// stages are the member functions in the order run() calls them.
// --gpus N (round 6): the file's regions, one per GPU (ShardedBamSelect, bam_device_select.h: the machinery of `SVDSS call
// --gpus N`) -- every region has its own loaders, feeding threads and record stream, and every GPU its copy of the
// chromosomes; oversubscribed (effective_gpus), it puts the N regions on the GPUs there are.  The records and their order are those
// of one GPU's run; the BGZF members are not cut at the same bytes: a region ends with a short member where one GPU's
// stream would have gone on filling it, and the record a seam completes is a member of its own (`gzip -dc` of the two
// files is the same).
struct DevicePipeline {
  typedef DeviceBamSelect<SelectedBatch>::CollectFn CollectFn;
  SmoothRun& R;
  const CallOptions& o;
  SfsSide* const side;
  const HeaderPre& hp;
  const int64_t target;                  // inflated bytes per batch, feeding threads per GPU
  const int per_gpu;
  const std::vector<size_t> cuts;        // the regions of the file, and the GPUs they run on
  const size_t n_regions, n_sm;
  std::vector<svdss_bam_smooth_t*> sms;
  std::vector<svdss_ref_t*> drefs;
  std::vector<int32_t> tid_map;
  double al_accuracy = 0.0;
  Gate gate;
  svdss_bam_stream_t* stream = nullptr;
  OutputPool pool;
  BatchWriter writer;
  std::unique_ptr<DeviceBamSelect<SelectedBatch>> rd;
  std::unique_ptr<ShardedBamSelect<SelectedBatch>> rds;
  uint64_t n_batches = 0, n_rec = 0, n_kept = 0, n_xf[4] = {0, 0, 0, 0}, out_bytes = 0;
  double st_s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, inf_s = 0, t_write = 0;
  // A feeding thread's smooth_batch and collect for a batch run on the same thread: the pool buffer the first took
  // travels to the second in this thread-local (-1: none)
  inline static thread_local int tl_slot = -1;
  explicit DevicePipeline(SmoothRun& run)
      : R(run), o(run.o), side(run.side.get()), hp(run.hp), target(run.knobs.batch_bytes), per_gpu(run.knobs.feeders),
        cuts(effective_gpus(o.gpus) > 1 ? plan_bam_regions(o.bam, effective_gpus(o.gpus), hp.skip) : std::vector<size_t>{0, 0}),
        n_regions(cuts.size() - 1), n_sm(std::min<size_t>(n_regions, (size_t)std::max(1, svdss_device_count()))), sms(n_sm, nullptr),
        drefs(n_sm, nullptr), pool(target, per_gpu), writer(pool, o.nobam, run.knobs) {}
  void note(const char* what) const { if (R.knobs.debug) fprintf(stderr, "[smooth] %s at +%.3f s\n", what, R.since()); }
  InputIndexFold* bam_index() const { return R.hooks ? R.hooks->bam_index : nullptr; }
  // the output's header goes in front of the first batch's records
  void set_output_prefix() {
    if (svdss_bam_stream_create(hp.n_ref, &stream) != SVDSS_OK) die("out of memory");
    ByteSink hs;
    bam_write_header(hs, hp.text, hp.names, hp.lens);
    if (svdss_bam_stream_set_output_prefix(stream, hs.v.data(), (int64_t)hs.v.size()) != SVDSS_OK) die("out of memory");
    // (run --write-bam-index: the stream of the whole file, or of its first region, leaves the input's index fragments)
    if (bam_index() && svdss_bam_stream_set_input_index(stream, bam_index()->shift(), bam_index()->depth()) != SVDSS_OK) die("the input index cannot be switched on");
    note("BAM header read, output prefix set");
  }
  // feeding thread: one batch smoothed, its members down into a buffer of the pool, its reads to the SfsSide
  int smooth_batch(size_t g, bool use_pool, svdss_bam_stream_t* st, int64_t seq, int32_t last, int64_t sk, size_t, int32_t nc, const uint8_t* const* comp,
                   const int64_t* cb, const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* nb, svdss_bam_batch_t** batch) {
    gate.wait();
    tl_slot = use_pool ? pool.take() : -1;
    int rc = svdss_bam_smooth_run(st, seq, last, sk, sms[g % sms.size()], al_accuracy, tl_slot >= 0 ? pool.buf[(size_t)tl_slot] : nullptr,
                                  tl_slot >= 0 ? (int64_t)pool.cap : 0, nc, comp, cb, blocks, crc, nb, batch);
    if (rc == SVDSS_OK && side) {
      int64_t job_comp = 0;
      for (int32_t k = 0; k < nc; ++k) job_comp += cb[k];
      rc = side->after_run(*batch, job_comp);
    }
    if (rc != SVDSS_OK && tl_slot >= 0) { pool.give(tl_slot); tl_slot = -1; }
    return rc;
  }
  BamRunFn run_for(size_t g, bool use_pool) { return [this, g, use_pool](auto... a) { return smooth_batch(g, use_pool, a...); }; }
  // feeding thread, right behind smooth_batch: what the writer and the index need of the batch
  std::unique_ptr<SelectedBatch> collect(const svdss_bam_batch_t* b, uint64_t seq) {
    if (side) side->collect(b, seq);
    std::unique_ptr<SelectedBatch> out(new SelectedBatch);
    svdss_bam_smoothed_t r;
    (void)svdss_bam_batch_smoothed(b, &r);
    out->n_records = (uint64_t)r.n_records; out->n_kept = (uint64_t)r.n_kept;
    for (int k = 0; k < 4; ++k) out->n_xf[k] = (uint64_t)r.n_xf[k];
    if (tl_slot >= 0 && r.bgzf == pool.buf[(size_t)tl_slot]) { out->ext = r.bgzf; out->ext_n = (size_t)r.bgzf_bytes; out->ext_slot = tl_slot; }
    else {
      out->bytes.assign(r.bgzf, r.bgzf + r.bgzf_bytes);
      if (tl_slot >= 0) pool.give(tl_slot);
    }
    tl_slot = -1;
    for (int k = 0; k < 8; ++k) out->stage_s[k] = r.stage_ms[k] * 1e-3;
    out->inflate_kernel_s = r.inflate_kernel_ms * 1e-3;
    if (bam_index()) out->in_ix.take(b);
    if (R.ixb) {
      (void)svdss_bam_batch_index(b, &out->ix);
      out->ix_chunks.assign(out->ix.chunks, out->ix.chunks + out->ix.n_chunks);
      out->ix_windows.assign(out->ix.windows, out->ix.windows + out->ix.n_windows);
    }
    return out;
  }
  void start_reader() {
    const CollectFn coll = [this](const svdss_bam_batch_t* b, uint64_t seq) { return collect(b, seq); };
    if (n_regions == 1) rd.reset(new DeviceBamSelect<SelectedBatch>(o.bam, 1, hp.n_ref, hp.skip, per_gpu, target, run_for(0, !o.nobam), coll, stream));
    else {
      ShardedBamSelect<SelectedBatch>::Hooks hk;
      hk.run = [this](size_t g, bool seam) { return run_for(g, g == 0 && !seam); };
      hk.collect = [coll](size_t g, bool seam) {
        return CollectFn([coll, g, seam](const svdss_bam_batch_t* b, uint64_t seq) {
          std::unique_ptr<SelectedBatch> out = coll(b, seq);
          if (out) { out->in_ix.region = g; out->in_ix.seam = seam; }
          return out;
        });
      };
      // (the output's header is in front of the first region's stream; the first region never runs again)
      hk.stream = [this](size_t g) { svdss_bam_stream_t* st = g == 0 ? stream : nullptr; if (g == 0) stream = nullptr; return st; };
      rds.reset(new ShardedBamSelect<SelectedBatch>(o.bam, hk, hp.n_ref, hp.skip, per_gpu, target, cuts, 64, std::vector<BgzfScanner*>(), false,
                                                    bam_index() ? bam_index()->shift() : 0, bam_index() ? bam_index()->depth() : 0));
    }
    note("reader of the smoothing pass started");
  }
  // every GPU its copy of the chromosomes and its svdss_bam_smooth_t
  void upload_and_configure() {
    std::vector<int> rcs(n_sm, SVDSS_OK);
    on_threads(n_sm, [&](size_t d, size_t) {
      std::vector<int32_t> tm;
      int& rc = rcs[d];
      SmoothHooks* const h = R.hooks && R.hooks->session && d == 0 ? R.hooks : nullptr;
      if (h && h->dref && h->dref_names == hp.names && h->dref_lens == hp.lens) {   // (the same header: the copy in HBM serves again)
        drefs[0] = h->dref; h->dref = nullptr;
        tm = h->tid_map;
        rc = SVDSS_OK;
        if (o.verbose || R.knobs.debug) fprintf(stderr, "[run] reference: copy on the GPU reused\n");
      } else {
        if (h && h->dref) { svdss_ref_free(h->dref); h->dref = nullptr; }
        rc = d == 0 ? resident_chromosomes(&R.ref_dev, hp.names, R.chrom, tm, &drefs[d]) : upload_chromosomes(hp.names, R.chrom, (int)d, tm, &drefs[d]);
        if (h) ++h->n_ref_uploads;
        if (h && (o.verbose || R.knobs.debug)) fprintf(stderr, "[run] reference: uploaded to the GPU in the order of the BAM header\n");
      }
      if (rc == SVDSS_OK) rc = svdss_bam_smooth_create(drefs[d], tm.data(), (int32_t)tm.size(), (int32_t)o.min_mapq, &sms[d]);
      if (rc == SVDSS_OK && R.ixb) rc = svdss_bam_smooth_set_index(sms[d], R.ix_shift, R.ix_depth);
      if (rc == SVDSS_OK) rc = svdss_bam_smooth_set_deflate(sms[d], o.compress);
      if (rc == SVDSS_OK && side) rc = svdss_bam_smooth_set_search(sms[d], side->flags(), R.park);
      if (rc == SVDSS_OK && o.nobam) rc = svdss_bam_smooth_set_output(sms[d], 0);
      if (rc == SVDSS_OK && R.hooks && R.hooks->store) rc = svdss_bam_smooth_set_store(sms[d], R.hooks->store, (int32_t)std::min<unsigned>(o.min_mapq, 256u));
      if (d == 0) tid_map.swap(tm);
    });
    for (size_t d = 0; d < n_sm; ++d)
      if (rcs[d] != SVDSS_OK) die(std::string("chromosomes to GPU ") + std::to_string(d) + ": " + svdss_strerror(rcs[d]) + " " + svdss_last_hip_error());
    if (R.knobs.debug) fprintf(stderr, "[smooth] chromosomes uploaded at +%.3f s (%zu GPU(s), %zu region(s))\n", R.since(), n_sm, n_regions);
    if (R.knobs.debug) fprintf(stderr, "[smooth] reference read in %.3f s, on the device at +%.3f s\n", R.fasta_s, R.since());
  }
  // compute_maxaccuracy (smoother.cpp:259-346): the mismatch rates of the first 10,000 records that fit, their percentile
  void measure_accuracy() {
    std::vector<double> acc;
    BamRunFn mrun = [this](svdss_bam_stream_t* st, int64_t seq, int32_t last, int64_t sk, size_t, auto... chunks) {
      return svdss_bam_smooth_measure(st, seq, last, sk, sms[0], chunks...);
    };
    CollectFn mcollect = [](const svdss_bam_batch_t* b, uint64_t) {
      std::unique_ptr<SelectedBatch> out(new SelectedBatch);
      svdss_bam_smoothed_t r;
      (void)svdss_bam_batch_smoothed(b, &r);
      out->n_records = (uint64_t)r.n_records; out->n_kept = (uint64_t)r.n_kept;
      out->match_mismatch.assign(r.match_mismatch, r.match_mismatch + 2 * r.n_kept);
      out->fits.assign(r.fits, r.fits + r.n_kept);
      return out;
    };
    // (10,000 records are a few tens of megabytes: small batches, two feeders, and the reader is dropped as soon as it has them)
    DeviceBamSelect<SelectedBatch> pre(o.bam, 1, hp.n_ref, hp.skip, 2, std::min<int64_t>(target, (int64_t)48 << 20), mrun, mcollect);
    while (acc.size() < 10000) {
      std::unique_ptr<SelectedBatch> b = pre.next();
      if (!b) { if (!pre.error().empty()) die("error reading " + o.bam + ": " + pre.error()); break; }
      for (size_t k = 0; k < b->fits.size() && acc.size() < 10000; ++k) {
        if (!b->fits[k]) continue;
        acc.push_back((double)b->match_mismatch[2 * k + 1] / (double)b->match_mismatch[2 * k]);
      }
    }
    al_accuracy = percentile(acc, o.accp);
    if (R.knobs.debug) fprintf(stderr, "[smooth] accuracy threshold %.6g at +%.3f s\n", al_accuracy, R.since());
  }
  void stream_batches() {
    writer.open();
    if (R.knobs.debug) fprintf(stderr, "[smooth] streaming from +%.3f s\n", R.since());
    while (std::unique_ptr<SelectedBatch> b = rd ? rd->next() : rds->next()) {
      const TimePoint t0 = now();
      ++n_batches;
      if (R.ixb) {   // (the batches come in file order, reruns included: the batch's members start at out_bytes)
        b->ix.chunks = b->ix_chunks.data(); b->ix.windows = b->ix_windows.data();
        R.ixb->add_fragment(b->ix, (uint64_t)out_bytes);
      }
      if (bam_index()) { if (rds) bam_index()->add(b->in_ix, *rds); else bam_index()->add(b->in_ix); }
      n_rec += b->n_records; n_kept += b->n_kept; out_bytes += b->ext ? b->ext_n : b->bytes.size();
      for (int k = 0; k < 4; ++k) n_xf[k] += b->n_xf[k];
      for (int k = 0; k < 8; ++k) st_s[k] += b->stage_s[k];
      inf_s += b->inflate_kernel_s;
      writer.put(std::move(b));
      t_write += secs(t0, now());
    }
    writer.close();
  }
  void drop_readers() {
    const std::string rerr = rd ? rd->error() : rds->error();
    if (rds && R.knobs.debug)
      fprintf(stderr, "[smooth] %zu regions on %zu GPU(s): %lld seam(s) proved, %lld region(s) run again\n", rds->n_regions(), n_sm, (long long)rds->seams_run(),
              (long long)rds->regions_run_again());
    rd.reset();
    rds.reset();
    pool.free_all();
    if (!rerr.empty()) die("error reading " + o.bam + ": " + rerr);
  }
  void finish_sfs_and_report() {
    if (side) side->finish(n_batches);
    if (side && R.hooks) side->free_index_and_park();
    if (side ? !(R.knobs.debug || o.verbose) : !R.knobs.debug) return;
    char sfs_s[64] = "";
    if (side) snprintf(sfs_s, sizeof sfs_s, "sfs export + search %.3f ", st_s[7]);
    fprintf(stderr, "[smooth] device path: %llu records, %llu kept (XF 0/1/2/3: %llu %llu %llu %llu), %llu BGZF bytes; feeder seconds: front %.3f "
            "turn wait %.3f turn %.3f walk %.3f rebuild %.3f %soutput turn %.3f deflate + down %.3f (inflate kernels %.3f); writing %.3f\n",
            (unsigned long long)n_rec, (unsigned long long)n_kept, (unsigned long long)n_xf[0], (unsigned long long)n_xf[1],
            (unsigned long long)n_xf[2], (unsigned long long)n_xf[3], (unsigned long long)out_bytes, st_s[0], st_s[1], st_s[2], st_s[3],
            st_s[4], sfs_s, st_s[5], st_s[6], inf_s, t_write);
  }
  // the EOF marker; the smoothing objects go, the first GPU's chromosomes go to the hooks (for `call`'s placement kernel)
  void end_stream_and_hand_over() {
    static const uint8_t eof_marker[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!o.nobam && (fwrite(eof_marker, 1, 28, stdout) != 28 || fflush(stdout) != 0)) writer.fail();
    for (svdss_bam_smooth_t* q : sms) svdss_bam_smooth_free(q);
    if (R.hooks) {
      R.hooks->dref = drefs[0]; drefs[0] = nullptr;
      R.hooks->tid_map = tid_map;
      R.hooks->dref_names = hp.names; R.hooks->dref_lens = hp.lens;
      R.hooks->n_batches = n_batches;
    }
    for (svdss_ref_t* q : drefs) svdss_ref_free(q);
    if (!writer.ok()) die("error writing the BAM to stdout");
  }
  int run() {
    set_output_prefix();
    start_reader();
    upload_and_configure();
    measure_accuracy();
    if (side) side->begin();
    gate.open();
    stream_batches();
    drop_readers();
    finish_sfs_and_report();
    end_stream_and_hand_over();
    R.write_index();
    note("done");
    return R.finish_process();
  }
};

// ---- the host pipeline: batches of eligible records read in order, smoothed by T workers, written in order (the
// reference's batch loop, smoother.cpp:441-537).  Three stages run side by side, joined by short queues: a thread reads
// and filters the next batch (BGZF inflate on the GPU or the host workers), this thread smooths the current one (GPU kernel
// + T finishing threads, or T host workers), a thread deflates and writes the previous one (T workers).
struct Item { std::vector<BamRecord> batch; std::vector<ByteSink> outs; };
// --write-index: a record's (tid, pos, reference span) and where it starts and ends in the inflated stream
struct HostIxRec { int32_t tid, pos; int64_t span; uint64_t u0, u1; };

struct HostPipeline {
  SmoothRun& R;
  const CallOptions& o;
  const size_t T;
  double al_accuracy = 0.0;
  std::unique_ptr<BamReader> bam;
  std::unique_ptr<BgzfWriter> w;
  std::vector<HostIxRec> hix;
  std::vector<uint32_t> members;         // the writer's block table: turns hix into virtual offsets once the stream is complete
  svdss_ref_t* dref = nullptr;           // the chromosomes on the GPU, BAM header order (null: SVDSS_SMOOTH_HOST=1, the host walk)
  std::vector<int32_t> tid_map;
  BoundedQueue<Item> q_read{2}, q_write{2};
  double t_read = 0, t_proc = 0, t_write = 0;
  PinBuf pb_s4, pb_q, pb_cig, pb_o4, pb_oq, pb_ocig;   // the batch's packed bases / qualities / CIGARs, in and out
  explicit HostPipeline(SmoothRun& run) : R(run), o(run.o), T((size_t)std::max(1, run.o.threads)) {}
  const std::string& ref_of(const BamRecord& r) const { return R.chrom.at(bam->ref_names()[(size_t)r.tid]); }
  // compute_maxaccuracy (smoother.cpp:259-346)
  void measure_accuracy() {
    BamReader pre(o.bam);
    pre.set_ahead(2);   // (10,000 records are a few chunks)
    svdss_enable_gpu_inflate(pre);
    if (!pre.ok() || !pre.read_header()) die("cannot read " + o.bam + ": " + pre.error());
    std::vector<double> acc;
    BamRecord r;
    while (acc.size() < 10000 && pre.next(r) > 0) {
      if (!R.eligible(r, pre.ref_names())) continue;
      double nm, nx;
      const std::string& ref = R.chrom[pre.ref_names()[(size_t)r.tid]];
      // (a record the smoothing pass will refuse -- XF = 3 -- has no defined mismatch rate: the reference walks off its
      // buffers on it, smoother.cpp:259-346)
      if (!cigar_fits(r, (size_t)r.l_seq, ref.size())) continue;
      mismatch_counts(r, r.seq_string(), ref, nm, nx);
      acc.push_back(nx / nm);
    }
    al_accuracy = percentile(acc, o.accp);
    if (R.knobs.debug) fprintf(stderr, "[smooth] accuracy threshold at +%.3f s\n", R.since());
  }
  // reader and writer of the smoothing pass, the output's header, the chromosomes on the GPU for the walk
  void open() {
    bam.reset(new BamReader(o.bam));
    svdss_enable_gpu_inflate(*bam);
    if (!bam->ok() || !bam->read_header()) die("cannot read " + o.bam + ": " + bam->error());
    w.reset(new BgzfWriter(stdout, (int)T));
    svdss_enable_gpu_deflate(*w);   // (csrc/deflate.hip; SVDSS_GPU_DEFLATE=0: libdeflate / zlib on the host)
    if (R.ixb) w->record_members(&members);
    bam_write_header(*w, bam->header_text(), bam->ref_names(), bam->ref_lens());
    tid_map.assign(bam->ref_names().size(), -1);
    if (R.knobs.smooth_host) { R.ref_dev.drop(); return; }   // (a developer switch: the host code below)
    // (no GPU and no SVDSS_SMOOTH_HOST=1: the command fails rather than quietly running the host walk)
    if (svdss_device_count() <= 0) die("no GPU found: SVDSS smooth walks the alignments on the GPU (SVDSS_SMOOTH_HOST=1 runs the host code instead)");
    if (resident_chromosomes(&R.ref_dev, bam->ref_names(), R.chrom, tid_map, &dref) != SVDSS_OK) die(std::string("svdss_ref_upload: ") + svdss_last_hip_error());
  }
  // smooth_read (smoother.cpp:84-232) of one record into its serialised BAM bytes
  void smooth_one(const BamRecord& r, ByteSink& sink) const {
    const std::string& ref = ref_of(r);
    const std::string seq = r.seq_string();
    std::vector<uint8_t> aux = r.aux;
    // the walk below indexes ref[pos ..] and seq[..] by the CIGAR: an alignment that overhangs the contig end or whose
    // CIGAR does not add up to l_seq is passed through unchanged with XF = 3, the reference's tag for a record it could
    // not rebuild consistently (smoother.cpp:219-228)
    if (!cigar_fits(r, seq.size(), ref.size())) {
      set_xf(aux, 3);
      write_record(sink, r, r.cigar, seq, r.qual, aux);
      return;
    }
    std::string nseq;
    std::vector<uint8_t> nqual;
    std::vector<uint32_t> ncig;
    double nm = 0, nx = 0;
    size_t ref_off = (size_t)r.pos, q_off = 0;
    uint32_t m_diff = 0;
    bool ignore = true;
    auto qcopy = [&](size_t start, size_t len) {   // may run past the read end like the reference's memcpy
      for (size_t i = 0; i < len; ++i) nqual.push_back(start + i < r.qual.size() ? r.qual[start + i] : 255);
    };
    for (uint32_t c : r.cigar) {
      const uint32_t l = c >> 4, op = c & 0xf;
      if (is_m(op)) {
        nseq.append(ref, ref_off, l);
        qcopy(q_off, l);
        for (uint32_t j = 0; j < l; ++j) (ref[ref_off + j] == seq[q_off + j]) ? ++nm : ++nx;
        ref_off += l; q_off += l;
        if (!ncig.empty() && (ncig.back() & 0xf) == 0) ncig.back() += (l + m_diff) << 4;
        else ncig.push_back(((l + m_diff) << 4) | 0);
        m_diff = 0;
      } else if (op == 1) {
        if ((int)l > MIN_INDEL) { ignore = false; nseq.append(seq, q_off, l); qcopy(q_off, l); ncig.push_back(c); }
        q_off += l;
      } else if (op == 2) {
        if ((int)l <= MIN_INDEL) { nseq.append(ref, ref_off, l); qcopy(q_off, l); m_diff += l; }
        else { ignore = false; ncig.push_back(c); }
        ref_off += l;
      } else if (op == 4) {
        ignore = false;
        nseq.append(seq, q_off, l);
        qcopy(q_off, l);
        q_off += l;
        ncig.push_back(c);
      } else break;
    }
    if (nx / nm > al_accuracy) { set_xf(aux, 1); write_record(sink, r, r.cigar, seq, r.qual, aux); }
    else if (ignore) { set_xf(aux, 2); write_record(sink, r, r.cigar, seq, r.qual, aux); }
    else { set_xf(aux, 0); write_record(sink, r, ncig, nseq, nqual, aux); }
  }
  // the CIGAR walk of the whole batch on the GPU (csrc/place.hip, smooth_kernel: one wavefront per record); the host
  // keeps what is per record and tiny: the consistency check, the XF decision, the record header
  void gpu_walk(std::vector<BamRecord>& batch, std::vector<ByteSink>& outs) {
    std::vector<size_t> idx;                      // batch index of the records that go to the GPU
    std::vector<int32_t> tid, pos, lq;
    std::vector<int64_t> cig_off(1, 0), s4_off, q_off, cap_off(1, 0);
    // first the sizes (cheap, in order), then the bytes (T threads into page-locked buffers kept from batch to batch)
    size_t s4_bytes = 0, q_bytes = 0;
    for (size_t i = 0; i < batch.size(); ++i) {
      const BamRecord& r = batch[i];
      size_t rl = 0, qlen = 0;
      cigar_spans(r, rl, qlen);
      if (r.pos < 0 || (size_t)r.pos + rl > ref_of(r).size() || qlen != (size_t)r.l_seq || r.qual.size() != (size_t)r.l_seq) {
        smooth_one(r, outs[i]);                   // inconsistent record: the host path tags it XF = 3
        continue;
      }
      idx.push_back(i);
      tid.push_back(tid_map[(size_t)r.tid]);
      pos.push_back(r.pos);
      lq.push_back(r.l_seq);
      cig_off.push_back(cig_off.back() + (int64_t)r.cigar.size());
      s4_off.push_back((int64_t)s4_bytes);
      s4_bytes += r.seq4.size();
      q_off.push_back((int64_t)q_bytes);
      q_bytes += r.qual.size();
      cap_off.push_back(cap_off.back() + (int64_t)((qlen + rl + 1) & ~(size_t)1));
    }
    const size_t n = idx.size();
    if (!n) return;
    const size_t n_cig_in = (size_t)cig_off.back();
    uint8_t* s4 = pb_s4.ensure(s4_bytes + 16);
    uint8_t* ql = pb_q.ensure(q_bytes + 16);
    uint32_t* cig = (uint32_t*)pb_cig.ensure(4 * n_cig_in + 16);
    uint8_t* o4 = pb_o4.ensure((size_t)cap_off.back() / 2 + 8);
    uint8_t* oq = pb_oq.ensure((size_t)cap_off.back() + 8);
    uint32_t* ocig = (uint32_t*)pb_ocig.ensure(4 * (n_cig_in + 1) + 16);
    std::vector<uint8_t> oign(n);
    std::vector<int32_t> oncig(n), olen(n);
    std::vector<int64_t> onm(2 * n);
    on_threads(std::min<size_t>(T, std::max<size_t>(1, n / 64)), [&](size_t t, size_t nt) {
      for (size_t k = n * t / nt; k < n * (t + 1) / nt; ++k) {
        const BamRecord& r = batch[idx[k]];
        memcpy(s4 + s4_off[k], r.seq4.data(), r.seq4.size());
        memcpy(ql + q_off[k], r.qual.data(), r.qual.size());
        memcpy(cig + cig_off[k], r.cigar.data(), 4 * r.cigar.size());
      }
    });
    if (svdss_smooth_batch(dref, tid.data(), pos.data(), cig, cig_off.data(), s4, s4_off.data(), ql, q_off.data(), lq.data(), cap_off.data(), (int64_t)n,
                           o4, oq, ocig, oncig.data(), olen.data(), onm.data(), oign.data()) != SVDSS_OK)
      die(std::string("svdss_smooth_batch: ") + svdss_last_hip_error());
    on_threads(std::min<size_t>(T, n), [&](size_t t, size_t nt) {
      for (size_t k = t; k < n; k += nt) {
        const BamRecord& r = batch[idx[k]];
        std::vector<uint8_t> aux = r.aux;
        const double nm = (double)onm[2 * k], nx = (double)onm[2 * k + 1];
        if (nx / nm > al_accuracy) { set_xf(aux, 1); write_record(outs[idx[k]], r, r.cigar, r.seq_string(), r.qual, aux); }
        else if (oign[k]) { set_xf(aux, 2); write_record(outs[idx[k]], r, r.cigar, r.seq_string(), r.qual, aux); }
        else {
          set_xf(aux, 0);
          write_record_packed(outs[idx[k]], r, ocig + cig_off[k], (size_t)oncig[k], o4 + cap_off[k] / 2, olen[k], oq + cap_off[k], aux);
        }
      }
    });
  }
  void process(std::vector<BamRecord>& batch, std::vector<ByteSink>& outs) {
    outs.assign(batch.size(), ByteSink());
    if (dref && !batch.empty()) gpu_walk(batch, outs);
    else on_threads(std::min<size_t>(T, batch.size()), [&](size_t t, size_t nt) { for (size_t i = t; i < batch.size(); i += nt) smooth_one(batch[i], outs[i]); });
  }
  // reading thread: batches of eligible records; the others are dropped from the output (smoother.cpp:509-537)
  int read_batches() {
    const size_t batch_size = 4096;
    int rc = 1;
    while (rc > 0) {
      const TimePoint t0 = now();
      std::unique_ptr<Item> it(new Item);
      while (it->batch.size() < batch_size) {
        BamRecord r;
        rc = bam->next(r);
        if (rc <= 0) break;
        if (!R.eligible(r, bam->ref_names())) continue;
        it->batch.push_back(std::move(r));
      }
      t_read += secs(t0, now());
      if (!it->batch.empty()) q_read.push(std::move(it));
    }
    q_read.close();
    return rc;
  }
  // writing thread, --write-index: what the index needs of a serialised record that starts at the writer's position
  void note_for_index(const ByteSink& sk) {
    HostIxRec x;
    const uint8_t* p = sk.v.data();
    uint32_t l_name = p[12], w4;
    memcpy(&x.tid, p + 4, 4); memcpy(&x.pos, p + 8, 4); memcpy(&w4, p + 16, 4);
    if ((w4 >> 16) & 4u) die("--write-index: an unmapped record in the output");   // (eligible() drops them)
    x.span = 0;
    for (uint32_t j = 0; j < (w4 & 0xffffu) && 36 + l_name + 4 * (size_t)j + 4 <= sk.v.size(); ++j) {
      uint32_t c;
      memcpy(&c, p + 36 + l_name + 4 * (size_t)j, 4);
      if (ix_ref_op(c & 0xfu)) x.span += c >> 4;
    }
    x.u0 = w->bytes_in(); x.u1 = x.u0 + sk.v.size();
    hix.push_back(x);
  }
  bool write_batches() {
    while (std::unique_ptr<Item> it = q_write.pop()) {
      const TimePoint t0 = now();
      for (const ByteSink& sk : it->outs) {
        if (R.ixb && sk.v.size() >= 36) note_for_index(sk);
        w->write(sk.v.data(), sk.v.size());
      }
      t_write += secs(t0, now());
    }
    return w->finish();
  }
  // position u of the stream: the member that holds its byte; the end of the stream: the EOF marker's offset
  void index_records() {
    const uint64_t total = w->bytes_in(), n_data = (total + 0xff00 - 1) / 0xff00;
    if (members.size() < n_data + 1) die("--write-index: the writer's block table is incomplete");
    std::vector<uint64_t> coff(members.size() + 1, 0);
    for (size_t i = 0; i < members.size(); ++i) coff[i + 1] = coff[i] + members[i];
    auto voff = [&](uint64_t u) { return u < total ? coff[u / 0xff00] << 16 | (u % 0xff00) : coff[n_data] << 16; };
    for (const HostIxRec& x : hix) R.ixb->add_record(x.tid, x.pos, x.span, voff(x.u0), voff(x.u1));
  }
  int run() {
    measure_accuracy();
    open();
    int rc = 1;
    bool write_ok = true;
    std::thread reader([&] { rc = read_batches(); });
    std::thread writer([&] { write_ok = write_batches(); });
    if (R.knobs.debug) fprintf(stderr, "[smooth] reference on the device at +%.3f s\n", R.since());
    while (std::unique_ptr<Item> it = q_read.pop()) {
      const TimePoint t0 = now();
      process(it->batch, it->outs);
      t_proc += secs(t0, now());
      std::vector<BamRecord>().swap(it->batch);
      q_write.push(std::move(it));
    }
    q_write.close();
    reader.join();
    writer.join();
    if (R.knobs.debug)
      fprintf(stderr, "[smooth] done at +%.3f s; stage busy seconds: read + filter %.3f, smooth %.3f, deflate + write %.3f\n", R.since(), t_read, t_proc, t_write);
    svdss_ref_free(dref);
    if (rc < 0) die("error reading " + o.bam + ": " + bam->error());
    if (!write_ok) die("error writing the BAM to stdout");
    if (R.ixb) index_records();
    R.write_index();
    if (!R.knobs.clean_exit) bam->report();
    return R.finish_process();
  }
};

int SmoothRun::run() {
  refuse_and_open_sfs();
  warm_up_and_load();
  if (side) park = side->create_park();
  plan_index();
  fasta_s = secs(t_fasta0, now());
  t_start = now();
  if (!takes_device_path()) return HostPipeline(*this).run();
  if (!hp.err.empty()) die(hp.err);
  return DevicePipeline(*this).run();
}
}  // namespace

int main_smooth(const CallOptions& o, SmoothHooks* hooks) {
  SmoothRun run(o, hooks);
  return run.run();
}
