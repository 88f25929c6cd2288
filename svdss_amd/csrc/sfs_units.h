// sfs_units.h -- what `SVDSS search` (search_host.cpp) and `SVDSS smooth --index --sfs` (smooth_host.cpp) share on the host:
// the knobs, the batch objects and their pools, the text of a batch (format_batch) and its ordered writer, the reads of
// device batches dealt again into units of whole reference batches (UnitAssembler), the hand-over of parked batches
// (EarlySearch) and the choice of the form the index becomes resident in.  Every unit that includes it has its own copy.
#pragma once
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <vector>

#include "host_common.h"
#include "cli_options.h"
#include "early_estimate.h"

namespace {

typedef std::chrono::steady_clock::time_point TimePoint;
TimePoint now() { return std::chrono::steady_clock::now(); }
double secs(TimePoint a, TimePoint b) { return std::chrono::duration<double>(b - a).count(); }
struct Stopwatch {   // seconds since the run began, for the --verbose lines
  TimePoint t0 = now();
  std::string since() const { return std::to_string(secs(t0, now())); }
};

// ---- the knobs: every SVDSS_* variable this file reads, read once at the top of main_search (README.md has the table).
// Not here: SVDSS_KMER / SVDSS_NO_KMER_LIMIT (the library's; choose_kmer_order SETS the first), the oversubscribe knob of
// effective_gpus (host_common.h), and what bam_device_select.h, bam_reader.h and the library read themselves.
// (env_from / env_raised / env_switch: host_common.h)
struct SearchKnobs {
  int64_t batch_bytes = env_from("SVDSS_BAM_BATCH_MB", 1, 192) << 20;         // inflated bytes per device batch (192 MB; `smooth` has its own default)
  size_t slab_bytes = (size_t)env_from("SVDSS_BAM_SLAB_KB", 64, 16 << 10) << 10;   // the scanners' read unit (16 MB, at least 64 KB)
  int loaders = (int)env_raised("SVDSS_BAM_LOADERS", 1, 8);                   // file-reading threads per scanner (8)
  int feeders = (int)env_raised("SVDSS_SEARCH_FEEDERS", 1, 6);                // feeding threads per GPU, both paths (6)
  int format_threads = (int)env_raised("SVDSS_FORMAT_THREADS", 1, 0);         // device path's text formatters (0: five per GPU, as the cores allow)
  // what may be parked at most, in arenas allocated as they are needed: SVDSS_PARK_GB (32), or SVDSS_PARK_MB (tests)
  int64_t park_bytes = env_from("SVDSS_PARK_MB", 1, env_from("SVDSS_PARK_GB", 1, 32) << 10) << 20;
  bool bam_device = env_switch("SVDSS_BAM_DEVICE") != 0;                      // 0: the host path (BamReader) although there is a GPU
  int early = env_switch("SVDSS_SEARCH_EARLY");                               // front end beside the restore: 1 forces it, 0 forbids it
  int64_t early_min_mb = getenv("SVDSS_EARLY_MIN_MB") ? atoll(getenv("SVDSS_EARLY_MIN_MB")) : 800;   // ... else from this index size on (800)
  int early_hold_ms = (int)env_from("SVDSS_EARLY_HOLD_MS", 1, 0);             // tests: the index held back as if its restore took that long
  int lf = env_switch("SVDSS_SEARCH_LF");                                     // the rank blocks alone: 1 forces, 0 forbids
  bool lf_max_set = getenv("SVDSS_SEARCH_LF_MAX") != nullptr;                 // ... else up to this many reads to search
  double lf_max = lf_max_set ? atof(getenv("SVDSS_SEARCH_LF_MAX")) : 0;       //     (default: 2e6 per 6.18e9 BWT symbols)
  bool fastx_device = env_switch("SVDSS_FASTX_DEVICE") != 0;                  // 0: `--fastx` through the host reader although the file is eligible
  // text bytes per device batch of `--fastx` (192 MB; SVDSS_FASTX_BATCH_KB: the same knob for tests)
  int64_t fastx_batch_bytes = getenv("SVDSS_FASTX_BATCH_KB") ? env_from("SVDSS_FASTX_BATCH_KB", 1, 1) << 10 : env_from("SVDSS_FASTX_BATCH_MB", 1, 192) << 20;
  // plain (single-stream) gzip of `--fastx` inflated on the GPU (csrc/gzip_stream.hip): opt-in (1) until it is measured
  // against the host reader; the chunk a wavefront decodes (256 KB) and the window of compressed bytes per run (64 MB;
  // SVDSS_GZIP_WINDOW_KB: the same knob for tests)
  bool fastx_gzip_device = env_switch("SVDSS_FASTX_GZIP_DEVICE") == 1;
  int64_t gzip_chunk_bytes = std::min<int64_t>(env_from("SVDSS_GZIP_CHUNK_KB", 1, 256), 1 << 20) << 10;
  int64_t gzip_window_bytes = getenv("SVDSS_GZIP_WINDOW_KB") ? env_from("SVDSS_GZIP_WINDOW_KB", 1, 64) << 10 : std::min<int64_t>(env_from("SVDSS_GZIP_WINDOW_MB", 1, 64), 1024) << 20;
  bool prewarm = !getenv("SVDSS_NO_PREWARM");                                 // page-locked buffers allocated beside the restore
  bool clean_exit = getenv("SVDSS_CLEAN_EXIT") != nullptr;                    // orderly teardown instead of _exit (leak checkers)
};

// ---- batches

struct Read {
  std::string name;
  int hp = 0;
  int64_t len = 0;
  int64_t first = 0, count = 0;  // into the result arrays (-1: not searched)
};
// page-locked staging buffers (svdss_host_alloc), recycled between batches
struct PinnedPool {
  std::mutex m;
  std::vector<std::pair<uint8_t*, size_t>> free_;
  uint8_t* get(size_t bytes, size_t& cap) {
    {
      std::lock_guard<std::mutex> lk(m);
      for (size_t i = 0; i < free_.size(); ++i)
        if (free_[i].second >= bytes) {
          uint8_t* p = free_[i].first;
          cap = free_[i].second;
          free_.erase(free_.begin() + (long)i);
          return p;
        }
    }
    void* p = nullptr;
    cap = bytes + bytes / 8 + 4096;
    check(svdss_host_alloc((int64_t)cap, &p), "svdss_host_alloc");
    return (uint8_t*)p;
  }
  void put(uint8_t* p, size_t cap) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(m);
    free_.emplace_back(p, cap);
  }
  ~PinnedPool() { for (auto& f : free_) svdss_host_free(f.first); }
};

struct SearchBatch {
  uint64_t seq = 0;              // position in the input: batches are written in this order
  std::vector<Read> reads;
  std::vector<uint8_t> gbuf;     // nt6 bases of the searched reads, back to back (FASTX mode)
  // BAM mode: the 4-bit bases exactly as the records hold them, in page-locked memory; the GPU expands them
  uint8_t* seq4 = nullptr;
  size_t seq4_cap = 0;
  std::vector<int64_t> boff;     // byte offset of every searched read in seq4 (+ end)
  std::vector<int32_t> lseq;
  std::vector<int64_t> goff;
  std::vector<size_t> gidx;      // searched read -> index into reads
  std::vector<int32_t> qs, ln;   // results
  std::vector<int64_t> counts;
  std::string text;              // the batch's lines, formatted by the thread that searched it
  uint64_t n_lines = 0;
};
// batch objects go round: their vectors and text buffers keep their capacity (tens of MB each; a fresh allocation of
// that size is an mmap, a page fault per 4 KB and a munmap that stalls every other thread of the process)
class BatchPool {
 public:
  explicit BatchPool(size_t cap) : cap_(cap) {}
  std::unique_ptr<SearchBatch> get() {
    std::unique_ptr<SearchBatch> b;
    {
      std::lock_guard<std::mutex> lk(m_);
      if (!free_.empty()) { b = std::move(free_.back()); free_.pop_back(); }
    }
    if (!b) b.reset(new SearchBatch);
    b->reads.clear(); b->gbuf.clear(); b->boff.clear(); b->lseq.clear();
    b->goff.clear(); b->gidx.clear(); b->qs.clear(); b->ln.clear(); b->text.clear(); b->counts.clear();
    b->n_lines = 0; b->seq = 0;
    return b;
  }
  void put(std::unique_ptr<SearchBatch> b) {
    std::lock_guard<std::mutex> lk(m_);
    if (free_.size() < cap_) free_.push_back(std::move(b));
  }
 private:
  const size_t cap_;
  std::mutex m_;
  std::vector<std::unique_ptr<SearchBatch>> free_;
};
// Formatted batches arrive out of order (several threads finish them) and are written to the sink (stdout, or `smooth --sfs FILE`) in the order of their
// `seq`; a written batch goes back to the pool.
class OrderedWriter {
 public:
  explicit OrderedWriter(BatchPool& pool, FILE* sink = stdout) : pool_(pool), sink_(sink), thread_([this] { run(); }) {}
  // (bounded: a finished batch waits until fewer than 8 are waiting -- or it is in front of all of them)
  void put(std::unique_ptr<SearchBatch> b) {
    std::unique_lock<std::mutex> lk(m_);
    const uint64_t sq = b->seq;
    cv_.wait(lk, [&] { return done_.size() < 8 || done_.begin()->first > sq; });
    done_[sq] = std::move(b);
    lk.unlock();
    cv_.notify_all();
  }
  // nothing more will be put: returns when everything is written and flushed
  void finish() {
    { std::lock_guard<std::mutex> lk(m_); finished_ = true; }
    cv_.notify_all();
    thread_.join();
  }
  uint64_t lines() const { return lines_; }         // (after finish)
  double busy_seconds() const { return seconds_; }
  bool failed() const { return failed_; }           // (after finish: a write to the sink came back short)
 private:
  void run() {
    uint64_t want = 0;
    for (;;) {
      std::unique_ptr<SearchBatch> bt;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return done_.count(want) || (finished_ && done_.empty()); });
        auto it = done_.find(want);
        if (it == done_.end()) break;
        bt = std::move(it->second);
        done_.erase(it);
        ++want;
      }
      cv_.notify_all();
      const auto tw0 = now();
      if (fwrite(bt->text.data(), 1, bt->text.size(), sink_) != bt->text.size()) failed_ = true;
      lines_ += bt->n_lines;
      seconds_ += secs(tw0, now());
      pool_.put(std::move(bt));
    }
    if (fflush(sink_) != 0) failed_ = true;
  }
  BatchPool& pool_;
  FILE* const sink_;
  bool failed_ = false;
  std::mutex m_;
  std::condition_variable cv_;
  std::map<uint64_t, std::unique_ptr<SearchBatch>> done_;
  bool finished_ = false;
  uint64_t lines_ = 0;
  double seconds_ = 0;
  std::thread thread_;   // (the last member: it runs from the constructor on)
};
// busy seconds of the stages, summed over their threads (--verbose)
struct StageSeconds {
  std::mutex m;   // for the sums several threads add to:
  double gpu = 0, inflate_ms = 0, unpack = 0, format = 0, device[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t n_seen = 0, n_batches = 0;
  double assemble = 0, slice = 0, decode = 0;   // (one thread each: no lock)
};
// decimal text of v at w, returns the end
inline char* put_int(char* w, int64_t v) {
  if (v < 0) { *w++ = '-'; v = -v; }
  char tmp[24];
  int n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) *w++ = tmp[--n];
  return w;
}

template <class T>
class BoundedQueue {
 public:
  explicit BoundedQueue(size_t cap) : cap_(cap) {}
  void push(std::unique_ptr<T> v) {
    std::unique_lock<std::mutex> lk(m_);
    not_full_.wait(lk, [&] { return q_.size() < cap_; });
    q_.push_back(std::move(v));
    not_empty_.notify_one();
  }
  // nullptr = the producer closed the queue and it is drained
  std::unique_ptr<T> pop() {
    std::unique_lock<std::mutex> lk(m_);
    not_empty_.wait(lk, [&] { return !q_.empty() || closed_; });
    if (q_.empty()) return nullptr;
    std::unique_ptr<T> v = std::move(q_.front());
    q_.pop_front();
    not_full_.notify_one();
    return v;
  }
  void close() {
    std::lock_guard<std::mutex> lk(m_);
    closed_ = true;
    not_empty_.notify_all();
  }
 private:
  size_t cap_;
  std::deque<std::unique_ptr<T>> q_;
  std::mutex m_;
  std::condition_variable not_full_, not_empty_;
  bool closed_ = false;
};
// the text of one batch.  output_batch order: reference batches of bsize reads -> thread t takes reads n with
// n % T == t (ping_pong.cpp:59,101-104) -> std::map<qname, vector<SFS>> order (:217)
void format_batch(const Options& o, SearchBatch& b) {
  const std::vector<Read>& reads = b.reads;
  std::string& out = b.text;
  out.reserve(b.qs.size() * 24 + 1024);
  char num[64];
  for (size_t b0 = 0; b0 < reads.size(); b0 += (size_t)o.bsize) {
    const size_t b1 = std::min(reads.size(), b0 + (size_t)o.bsize);
    for (int t = 0; t < o.threads; ++t) {
      std::map<std::string, std::vector<size_t>> by_name;
      for (size_t n = b0 + (size_t)t; n < b1; n += (size_t)o.threads)
        if (reads[n].count >= 0) by_name[reads[n].name].push_back(n);
      for (const auto& kv : by_name) {
        bool first = true;
        for (size_t n : kv.second) {
          const Read& r = reads[n];
          for (int64_t k = 0; k < r.count; ++k) {
            if (first) out += r.name; else out += '*';
            char* w = num;                      // "\t<qs>\t<len>\t<hp>\t\n" without printf (11 M lines per GB of reads)
            *w++ = '\t'; w = put_int(w, b.qs[(size_t)(r.first + k)]);
            *w++ = '\t'; w = put_int(w, b.ln[(size_t)(r.first + k)]);
            *w++ = '\t'; w = put_int(w, r.hp);
            *w++ = '\t'; *w++ = '\n';
            out.append(num, (size_t)(w - num));
            first = false;
            ++b.n_lines;
          }
        }
      }
    }
  }
}
// One GPU launch covers many reference-sized batches; the text is still emitted batch by
// batch, thread slice by thread slice, read names in std::map order (ping_pong.cpp:215-217).
// (32 k reads keep the GPU efficient and let parsing, search and output of successive batches overlap)
int64_t reads_per_unit(const Options& o) { return std::max<int64_t>(o.bsize, 32768 / o.bsize * (int64_t)o.bsize); }

struct DevOut { std::vector<Read> reads; std::vector<int32_t> qs, ln; int64_t n_short = 0; std::vector<int32_t> sidx; };
// `SVDSS search` with the BAM front end started BEFORE the index is resident (include/svdss_hip.h, svdss_bam_park_*): while
// the feeders have no index they run the front half of their batches and park the unpacked reads in HBM; when the index is
// there the parked groups are searched one large launch each (the drain thread), and the feeders go on with whole batches.
//
// Who touches what: `park`, `device`, `park_bytes`, `file_bytes` and `regions` are set before the first feeder runs and
// only read then; the four counters are atomics, added to by the feeders and read by anyone; everything private is under
// `m_`, reached through the methods alone, and `cv_` is notified on every change somebody may wait for.
//
// --gpus N: one EarlySearch per region of the file, each with a park on its region's GPU and an index handle of its own
// (that GPU's replica); `regions` names all of them, and what the process decides ONCE -- the order of the k-mer table,
// the form the index becomes resident in -- comes from the sum over them (early_estimate.h).
class EarlySearch {
 public:
  struct Pending { uint64_t seq; std::unique_ptr<DevOut> out; int64_t first, n; };
  svdss_bam_park_t* park = nullptr;
  int32_t device = 0;                 // where the park lives and the front halves run
  int64_t park_bytes = 0;             // what the park was created with (a region that runs again gets a fresh one)
  int64_t file_bytes = 0;             // of the file, or of this front end's region of it
  const std::vector<EarlySearch*>* regions = nullptr;   // every region's, this one included (null: this is the only one)
  // what the front end has seen so far (the order of the k-mer table is chosen from it: svdss_index_kmer_limit)
  std::atomic<int64_t> records{0}, searched{0}, comp_bytes{0}, index_n{0};

  // feeder, before a batch: the index if the feeders have it (a whole batch) -- null: the front half, the reads parked
  svdss_index_t* index_for_feeders() { std::lock_guard<std::mutex> lk(m_); return ready_ ? ix_ : nullptr; }
  EarlyCounters counters() {
    EarlyCounters c;
    c.records = records.load(); c.searched = searched.load(); c.comp_bytes = comp_bytes.load(); c.file_bytes = file_bytes;
    c.front_done = front_is_finished();
    return c;
  }
  // how many reads there will be to search, from what has been seen (-1: nothing seen yet); both cost models use it
  double estimate_reads_to_search() { return ::estimate_reads_to_search(counters()); }
  // feeder, after a front half: the counters, and from them the order of the k-mer table (its build begins when the suffix
  // array is sorted; the limit is read then).  The limit is the process's: with several regions it comes from their sum,
  // once every region has seen enough to be asked.
  void note_batch(int64_t n_records, int64_t n_searched, int64_t batch_comp_bytes) {
    const int64_t recs = (records += n_records);
    searched += n_searched; comp_bytes += batch_comp_bytes;
    if (index_n.load() < ((int64_t)1 << 31) || recs < kEarlyEstimateRecords || getenv("SVDSS_KMER") || getenv("SVDSS_NO_KMER_LIMIT")) return;
    double est = -1;
    if (regions) {
      std::vector<EarlyCounters> all;
      for (EarlySearch* e : *regions) all.push_back(e->counters());
      if (!estimate_wait_over(all, 0)) return;
      est = summed_estimate(all);
    } else {
      est = estimate_reads_to_search();
    }
    if (est < 0) return;
    // build: 1.6 s at K = 16, a quarter of that per step down; kernel: 16 M reads/s at K = 16, half of that per step down
    // (profiles/r05i_restore_by_table_order.txt); its seconds count double, as in choose_kmer_order
    auto cost = [&](int k) { return 1.6 * std::pow(4.0, k - 16) + 2 * est / 16e6 * std::pow(2.2, 16 - k); };
    int best = 16;
    for (int k = 15; k >= 12; --k) if (cost(k) < cost(best)) best = k;
    if (cost(best) > 0.8 * cost(16)) best = 16;     // (a clear gain or none)
    static std::mutex limit_m;      // (the library's limit is one for the process: so is the last one given)
    static int kmer_limit = 0;
    std::lock_guard<std::mutex> lk(limit_m);
    if (best != kmer_limit) { kmer_limit = best; svdss_index_kmer_limit(best == 16 ? 0 : best); }
  }
  // feeder whose batch found no room in the park (or it has just been closed): the batch waits here for the index
  svdss_index_t* wait_for_index() {
    std::unique_lock<std::mutex> lk(m_);
    park_full_ = true;
    cv_.notify_all();
    return wait_for(lk, [&] { return ready_; });
  }
  // a parked batch's names and tags wait for its group's search / the drain thread takes a group's `n` batches
  void add_pending(int64_t group, Pending p) { change([&] { by_group_[group].push_back(std::move(p)); }); }
  std::vector<Pending> take_group(int64_t group, int64_t n) {
    std::unique_lock<std::mutex> lk(m_);
    wait_for(lk, [&] { return abandoned_ || (int64_t)by_group_[group].size() == n; });
    if (abandoned_) return std::vector<Pending>();
    return std::move(by_group_[group]);
  }
  // main thread: the index is resident but held back from the feeders (the rank blocks alone, resident long before the file
  // has been read) until the front end is through -- or the park is full --, so that what is parked goes in large launches,
  // one lane per read, instead of a small segmented launch per batch.  The drain thread has it at once and searches the
  // groups as they close.
  void offer_index_held_back(svdss_index_t* ix) {
    std::unique_lock<std::mutex> lk(m_);
    ix_ = ix; ix_avail_ = true;
    cv_.notify_all();
    wait_for(lk, [&] { return front_done_ || park_full_; });
  }
  // main thread: from now on the feeders run whole batches
  void release_index(svdss_index_t* ix) { change([&] { ix_ = ix; ready_ = true; }); }
  // every feeding thread has ended
  void front_finished() { change([&] { front_done_ = true; }); }
  bool front_is_finished() { std::lock_guard<std::mutex> lk(m_); return front_done_; }
  // drain thread: the index once it is offered or released; whether the feeders have it; a short wait for news
  svdss_index_t* wait_for_offered_index() { std::unique_lock<std::mutex> lk(m_); return wait_for(lk, [&] { return ready_ || ix_avail_ || abandoned_; }); }
  // the seam in front of a region (one small batch, on the thread that deals the regions): the index once the feeders have it
  svdss_index_t* wait_for_released_index() { std::unique_lock<std::mutex> lk(m_); return wait_for(lk, [&] { return ready_; }); }
  // A region whose first run has failed runs again (ShardedBamSelect): abandon() when its feeding threads have ended --
  // the drain thread returns at its next look, searching and delivering nothing more --, then, with the drain thread
  // joined and the park emptied, reset_for_rerun(): nothing pending, nothing counted (the sum over the regions counts a
  // region once), the front not finished.  What is known of the index stays.
  void abandon() { change([&] { abandoned_ = true; }); }
  bool abandoned() { std::lock_guard<std::mutex> lk(m_); return abandoned_; }
  void reset_for_rerun() {
    change([&] { by_group_.clear(); front_done_ = park_full_ = abandoned_ = false; });
    records.store(0); searched.store(0); comp_bytes.store(0);
  }
  bool released() { std::lock_guard<std::mutex> lk(m_); return ready_; }
  void nap() { std::unique_lock<std::mutex> lk(m_); cv_.wait_for(lk, std::chrono::milliseconds(2)); }
 private:
  template <class F> void change(F f) { { std::lock_guard<std::mutex> lk(m_); f(); } cv_.notify_all(); }
  template <class P> svdss_index_t* wait_for(std::unique_lock<std::mutex>& lk, P pred) { cv_.wait(lk, pred); return ix_; }
  std::mutex m_;
  std::condition_variable cv_;
  svdss_index_t* ix_ = nullptr;      // set once, with ready_ -- or before it, with ix_avail_
  bool ready_ = false, ix_avail_ = false;
  std::map<int64_t, std::vector<Pending>> by_group_;
  bool front_done_ = false, park_full_ = false, abandoned_ = false;
};

// what a batch object holds after its run -> reads with their SFS; of a parked batch names and tags only (counts and SFS
// follow when its group has been searched: fill_parked)
inline std::unique_ptr<DevOut> unpack_result(const svdss_bam_result_t& r, bool parked) {
  std::unique_ptr<DevOut> out(new DevOut);
  out->n_short = r.n_short;
  out->reads.resize((size_t)r.n_slots);
  if (parked) {
    // the front half only: names and tags; counts and SFS follow when the batch's group has been searched
    out->sidx.assign(r.sidx, r.sidx + r.n_slots);
  } else {
    out->qs.assign(r.qs, r.qs + r.total_sfs);
    out->ln.assign(r.len, r.len + r.total_sfs);
  }
  // (searched reads are numbered in slot order, so their SFS follow each other in slot order too)
  int64_t acc = 0;
  for (int64_t i = 0; i < r.n_slots; ++i) {
    Read& rd = out->reads[(size_t)i];
    rd.name.assign(r.names + r.name_off[i], (size_t)(r.name_off[i + 1] - r.name_off[i]));
    rd.hp = r.hp[i];
    rd.first = acc;
    rd.count = r.sidx[i] < 0 ? -1 : parked ? 0 : r.counts[r.sidx[i]];
    if (rd.count > 0) acc += rd.count;
  }
  return out;
}
// a parked batch when its group has been searched: counts (with their running sums `prefix`) and SFS of the group's reads
inline void fill_parked(EarlySearch::Pending& P, const std::vector<int64_t>& counts, const std::vector<int64_t>& prefix,
                        const std::vector<int32_t>& qs, const std::vector<int32_t>& ln) {
  DevOut& d = *P.out;
  int64_t acc = 0;
  for (size_t i = 0; i < d.reads.size(); ++i) {
    Read& rd = d.reads[i];
    rd.first = acc;
    if (d.sidx[i] < 0) { rd.count = -1; continue; }
    const size_t k = (size_t)(P.first + d.sidx[i]);
    rd.count = counts[k];
    d.qs.insert(d.qs.end(), qs.begin() + prefix[k], qs.begin() + prefix[k + 1]);
    d.ln.insert(d.ln.end(), ln.begin() + prefix[k], ln.begin() + prefix[k + 1]);
    acc += rd.count;
  }
  d.sidx.clear();
}

// The unit assembler: device batches end where a BGZF member ends, the text is defined on batches of --bsize reads
// (ping_pong.cpp:213-236) -- the reads of the device batches, in file order, are dealt again into units of whole reference
// batches; full units go to the formatters (format_units) and from them to the ordered writer.
class UnitAssembler {
 public:
  UnitAssembler(const Options& o, StageSeconds& t) : o_(o), t_(t), super_(reads_per_unit(o)) {}
  void begin() { unit_ = pool_.get(); }
  // the reads of a device batch into the unit being filled
  void deal(DevOut& d) {
    const auto ta = now();
    // (said when the batch is dealt, not when it was read: a region that runs twice says it once)
    for (int64_t k = 0; k < d.n_short; ++k) logmsg("warning", "Alignment filtered due to l_qseq. Why are we here? Please check");   // :70-75
    for (Read& r : d.reads) {
      const int64_t first = r.first;
      r.first = (int64_t)unit_->qs.size();
      if (r.count > 0) {
        unit_->qs.insert(unit_->qs.end(), d.qs.begin() + first, d.qs.begin() + first + r.count);
        unit_->ln.insert(unit_->ln.end(), d.ln.begin() + first, d.ln.begin() + first + r.count);
      }
      unit_->reads.push_back(std::move(r));
      if ((int64_t)unit_->reads.size() == super_) {
        unit_->seq = unit_seq_++;
        units_.push(std::move(unit_));
        unit_ = pool_.get();
      }
    }
    t_.assemble += secs(ta, now());
  }
  // the input has ended: the unit being filled is the last one
  void end() {
    if (!unit_->reads.empty()) { unit_->seq = unit_seq_++; units_.push(std::move(unit_)); }
    units_.close();
  }
  // a formatting thread: units -> text -> writer, until the assembler has ended
  void format_units(OrderedWriter& writer) {
    while (std::unique_ptr<SearchBatch> u = units_.pop()) {
      const auto tf = now();
      format_batch(o_, *u);
      { std::lock_guard<std::mutex> lk(t_.m); t_.format += secs(tf, now()); }
      writer.put(std::move(u));
    }
  }
  BatchPool& pool() { return pool_; }
 private:
  const Options& o_;
  StageSeconds& t_;
  const int64_t super_;
  BoundedQueue<SearchBatch> units_{4};
  BatchPool pool_{16};
  std::unique_ptr<SearchBatch> unit_;   // (the assembler's: the unit being filled)
  uint64_t unit_seq_ = 0;
};

// ---- the form the index becomes resident in.  Which one is used never changes results.
// The order K of the k-mer table trades its build time (4^K entries: 1.6 s at K = 16, a quarter of that per step
// down) against the search kernel's speed (about a third slower per step down).  The library's own choice (K = 16
// from 64 Mb on) is the one for a resident index that searches batch after batch; a process that restores the
// index for ONE input knows roughly how many reads are coming (a BAM is ~1 byte per base, a FASTQ ~2) and takes the
// K that minimises build + search.  Results never depend on K (tests/test_sfs_gpu.py, tests/test_scale_gpu.py).
// Returns true when the user chose the order (SVDSS_KMER; this function may set the variable itself).
inline bool choose_kmer_order(const std::string& input, bool bam_mode, svdss_index_t* ix, bool verbose) {
  if (getenv("SVDSS_KMER") != nullptr) return true;
  struct stat st;
  // (references above 2^31 symbols keep the library's K: nothing below 16 was measured there)
  const int64_t n = svdss_index_size(ix);
  if (stat(input.c_str(), &st) != 0 || st.st_size <= 0 || n >= ((int64_t)1 << 31)) return false;
  const double est_reads = (double)st.st_size / (bam_mode ? 15000.0 : 30000.0);
  int k_auto = 1;
  while (k_auto < 16 && ((int64_t)1 << (2 * k_auto)) <= n) ++k_auto;
  k_auto = std::min(16, k_auto + 2);
  int best = k_auto;
  double best_cost = 1e300;
  for (int k = k_auto; k >= std::max(8, k_auto - 5); --k) {
    // (the kernel's seconds count double: they are GPU time the BGZF inflate of the stream wants too)
    const double build = 1.6 * std::pow(4.0, k - 16), kernel = est_reads / 15e6 * std::pow(1.35, 16 - k);
    if (build + 2 * kernel < best_cost) { best_cost = build + 2 * kernel; best = k; }
  }
  if (best == k_auto) return false;
  setenv("SVDSS_KMER", std::to_string(best).c_str(), 0);
  if (verbose) logmsg("debug", "k-mer table of order " + std::to_string(best) + " for ~" + std::to_string((long long)est_reads) + " reads");
  return false;
}
// Few reads to search (the front end has seen enough to say: `search` on a smoothed BAM skips what `smooth` tagged XF != 0)
// and the sidecar carries the rank blocks: the index as a rank structure ALONE -- 3 GB uploaded instead of six billion
// suffixes sorted for a text, a suffix array and a k-mer table; ~1 M reads/s instead of 8 - 24 M, results identical
// (svdss_index_attach_blocks).  SVDSS_SEARCH_LF=0|1 forces the choice, SVDSS_SEARCH_LF_MAX moves the threshold (reads).
// True: the blocks are attached.
// The decision alone (`run --samples` takes it for every sample while the rank blocks alone are resident, and attaches
// nothing): est / t_est: the estimate it rests on and when it was known.
// early: one front end, or one per region of the file (--gpus N) -- ONE decision, from the sum over them, taken when
// every one of them has seen 50,000 records or finished its front, or after 1.5 s (early_estimate.h).
inline bool wants_rank_blocks_alone(const SearchKnobs& knobs, const std::vector<EarlySearch*>& early, int64_t index_n, bool user_kmer, const Stopwatch& clock,
                                    double& est, std::string& t_est) {
  if (user_kmer || knobs.lf == 0) return false;
  const bool forced = knobs.lf == 1;
  const auto w0 = now();
  std::vector<EarlyCounters> seen;
  auto look = [&] { seen.clear(); for (EarlySearch* e : early) seen.push_back(e->counters()); };
  for (look(); !forced && !estimate_wait_over(seen, secs(w0, now())); look()) std::this_thread::sleep_for(std::chrono::milliseconds(5));
  est = summed_estimate(seen);
  t_est = clock.since();
  // (what the rank structure alone saves is the rest of the restore -- ~4.5 s at GRCh38 lengths, in proportion for a
  // smaller reference --, what it costs is the search at ~1 M reads/s instead of 8 - 24 M: worth it below ~2 M reads
  // per 6.2e9 BWT symbols; profiles/r06q_*)
  return forced || rank_blocks_alone_pay(est, knobs.lf_max_set, knobs.lf_max, index_n);
}
inline bool wants_rank_blocks_alone(const SearchKnobs& knobs, EarlySearch& early, int64_t index_n, bool user_kmer, const Stopwatch& clock, double& est,
                                    std::string& t_est) {
  return wants_rank_blocks_alone(knobs, std::vector<EarlySearch*>(1, &early), index_n, user_kmer, clock, est, t_est);
}
// (n_gpus > 1: the blocks are read from the sidecar ONCE, here, and every GPU gets them from this one host copy)
inline bool choose_rank_blocks_alone(const SearchKnobs& knobs, const std::vector<EarlySearch*>& early, svdss_index_t* ix, const std::string& index_path,
                                     bool user_kmer, bool verbose, const Stopwatch& clock, int n_gpus = 1) {
  double est = -1;
  std::string t_est;
  if (!wants_rank_blocks_alone(knobs, early, svdss_index_size(ix), user_kmer, clock, est, t_est)) return false;
  const int rc = svdss_index_attach_blocks(ix, index_path.c_str());
  if (rc == SVDSS_OK) {
    if (verbose) logmsg("debug", "~" + std::to_string((long long)std::max(0.0, est)) + " reads to search (known at +" + t_est + " s): the index as a rank structure alone (blocks read" +
                                     (n_gpus > 1 ? " once for " + std::to_string(n_gpus) + " GPUs," : "") + " at +" + clock.since() + " s)");
    return true;
  }
  if (rc != SVDSS_EINVAL) check(rc, "svdss_index_attach_blocks");
  return false;
}
inline bool choose_rank_blocks_alone(const SearchKnobs& knobs, EarlySearch& early, svdss_index_t* ix, const std::string& index_path, bool user_kmer,
                                     bool verbose, const Stopwatch& clock) {
  return choose_rank_blocks_alone(knobs, std::vector<EarlySearch*>(1, &early), ix, index_path, user_kmer, verbose, clock);
}

}  // namespace
