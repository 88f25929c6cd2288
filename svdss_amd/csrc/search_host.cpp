// search_host.cpp -- `SVDSS search` (/root/reference/ping_pong.cpp; main.cpp:62-68): main_search is a SearchRun whose
// methods are the stages, in the order they happen.
//
// Three stages run concurrently, connected by bounded queues: (1) BGZF inflate + record parsing + nt6
// encoding into GPU-ready batches, (2) the GPU search of one batch, (3) formatting and writing the text of
// the previous batch.  The reference interleaves the same work inside one OpenMP loop
// (ping_pong.cpp:329-376: thread 0 loads and prints while the others search).
// SFS text goes to stdout exactly as PingPong::output_batch prints it (ping_pong.cpp:213-236).
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "host_common.h"
#include "bam_reader.h"
#include "bgzf_scanner.h"
#include "bam_device_select.h"
#include "gpu_inflate_hook.h"
#include "cli_options.h"
#include "call_host.h"
#include "fastx_reader.h"

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
// the value if it is set and at least `least` / if it is set, raised to `least` / -1 not set, 0 off, 1 on
int64_t env_from(const char* name, int64_t least, int64_t dflt) { const char* e = getenv(name); return e && atoll(e) >= least ? atoll(e) : dflt; }
int64_t env_raised(const char* name, int64_t least, int64_t dflt) { const char* e = getenv(name); return e ? std::max<int64_t>(least, atoll(e)) : dflt; }
int env_switch(const char* name) { const char* e = getenv(name); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }
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
// Formatted batches arrive out of order (several threads finish them) and are written to stdout in the order of their
// `seq`; a written batch goes back to the pool.
class OrderedWriter {
 public:
  explicit OrderedWriter(BatchPool& pool) : pool_(pool), thread_([this] { run(); }) {}
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
      fwrite(bt->text.data(), 1, bt->text.size(), stdout);
      lines_ += bt->n_lines;
      seconds_ += secs(tw0, now());
      pool_.put(std::move(bt));
    }
    fflush(stdout);
  }
  BatchPool& pool_;
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

// ---- `search --bam` with the records handled where they are inflated (csrc/bam_device.hip): the host reads the file,
// finds the BGZF members, hands runs of them to the GPUs and gets names, tags and SFS back -- through the front end that
// `call` and `smooth` read the file with as well (bam_device_select.h: scanner -> batcher -> feeding threads ->
// ordered hand-over, per region of the file).  Then, once for the file: assembler (device batches end where a BGZF member
// ends; the text is defined on batches of --bsize reads, ping_pong.cpp:213-236: the reads are dealt again into units of
// whole reference batches) -> formatting threads -> writer.  The same bytes as the host path.
//
// --gpus N (north_star: "BAM regions partition across the GPUs"; the per-shard loop of ping_pong.cpp:53-128): the file is
// cut at BGZF members into N regions of about equal size, every GPU reads, inflates, walks and searches its own region
// (ShardedBamSelect: a region's first record is guessed, and proved at the seam or the region runs again).  The reads of a
// region are dealt into units when everything before it has been (the unit a read belongs to depends on the reads in front
// of it), so the later regions' results wait in memory (~0.6 KB per read).
struct DevOut { std::vector<Read> reads; std::vector<int32_t> qs, ln; int64_t n_short = 0; std::vector<int32_t> sidx; };
// the file as the device path reads it: its regions (plan_bam_regions) and one scanner per region, opened before the index is
// restored and kept open to the end (the process ends with _exit: their page-locked slabs are never handed back one by one)
struct DeviceBamInput {
  std::vector<size_t> cuts;
  std::vector<std::unique_ptr<BgzfScanner>> scanners;
  std::vector<BgzfScanner*> scanner_ptrs;
  int32_t n_ref = 0;
  int64_t skip = 0;
  size_t n_regions() const { return cuts.size() - 1; }
};
// `SVDSS search` with the BAM front end started BEFORE the index is resident (include/svdss_hip.h, svdss_bam_park_*): while
// the feeders have no index they run the front half of their batches and park the unpacked reads in HBM; when the index is
// there the parked groups are searched one large launch each (the drain thread), and the feeders go on with whole batches.
//
// Who touches what: `park` and `file_bytes` are set before the first feeder runs and only read then; the four counters are
// atomics, added to by the feeders and read by anyone; everything private is under `m_`, reached through the methods alone,
// and `cv_` is notified on every change somebody may wait for.
class EarlySearch {
 public:
  struct Pending { uint64_t seq; std::unique_ptr<DevOut> out; int64_t first, n; };
  svdss_bam_park_t* park = nullptr;
  int64_t file_bytes = 0;
  // what the front end has seen so far (the order of the k-mer table is chosen from it: svdss_index_kmer_limit)
  std::atomic<int64_t> records{0}, searched{0}, comp_bytes{0}, index_n{0};

  // feeder, before a batch: the index if the feeders have it (a whole batch) -- null: the front half, the reads parked
  svdss_index_t* index_for_feeders() { std::lock_guard<std::mutex> lk(m_); return ready_ ? ix_ : nullptr; }
  // how many reads there will be to search, from what has been seen (-1: nothing seen yet); both cost models use it
  double estimate_reads_to_search() const {
    const int64_t recs = records.load(), srch = searched.load(), cb = comp_bytes.load();
    return recs > 0 && cb > 0 ? (double)srch / (double)recs * ((double)recs * (double)file_bytes / (double)cb) : -1;
  }
  // feeder, after a front half: the counters, and from them the order of the k-mer table (its build begins when the suffix
  // array is sorted; the limit is read then)
  void note_batch(int64_t n_records, int64_t n_searched, int64_t batch_comp_bytes) {
    const int64_t recs = (records += n_records);
    searched += n_searched; comp_bytes += batch_comp_bytes;
    if (index_n.load() < ((int64_t)1 << 31) || recs < 50000 || getenv("SVDSS_KMER") || getenv("SVDSS_NO_KMER_LIMIT")) return;
    const double est = estimate_reads_to_search();
    if (est < 0) return;
    // build: 1.6 s at K = 16, a quarter of that per step down; kernel: 16 M reads/s at K = 16, half of that per step down
    // (profiles/r05i_restore_by_table_order.txt); its seconds count double, as in choose_kmer_order
    auto cost = [&](int k) { return 1.6 * std::pow(4.0, k - 16) + 2 * est / 16e6 * std::pow(2.2, 16 - k); };
    int best = 16;
    for (int k = 15; k >= 12; --k) if (cost(k) < cost(best)) best = k;
    if (cost(best) > 0.8 * cost(16)) best = 16;     // (a clear gain or none)
    std::lock_guard<std::mutex> lk(m_);
    if (best != kmer_limit_) { kmer_limit_ = best; svdss_index_kmer_limit(best == 16 ? 0 : best); }
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
    wait_for(lk, [&] { return (int64_t)by_group_[group].size() == n; });
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
  svdss_index_t* wait_for_offered_index() { std::unique_lock<std::mutex> lk(m_); return wait_for(lk, [&] { return ready_ || ix_avail_; }); }
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
  bool front_done_ = false, park_full_ = false;
  int kmer_limit_ = 0;               // the last limit given
};

class DevicePath {
 public:
  DevicePath(const Options& o, const SearchKnobs& knobs, const std::vector<svdss_index_t*>& replicas, const DeviceBamInput& in,
             const Stopwatch& clock, EarlySearch* early = nullptr)
      : o_(o), knobs_(knobs), replicas_(replicas), in_(in), clock_(clock), early_(early), super_(reads_per_unit(o)),
        flags_((o.assemble ? SVDSS_SFS_ASSEMBLE : 0) | (o.putative ? SVDSS_BAM_PUTATIVE : 0)) {}
  void run();
 private:
  BamRunFn run_on(size_t r);
  std::unique_ptr<DevOut> collect(const svdss_bam_batch_t* batch, uint64_t seq);
  std::unique_ptr<DevOut> next() { return one_ ? one_->next() : sharded_->next(); }
  void deal(DevOut& d);
  void assemble();
  void format_units();
  void drain_park();
  void report();

  const Options& o_;
  const SearchKnobs& knobs_;
  const std::vector<svdss_index_t*> replicas_;
  const DeviceBamInput& in_;
  const Stopwatch& clock_;
  EarlySearch* const early_;
  const int64_t super_;
  const int32_t flags_;
  StageSeconds t_;
  // units of whole reference batches, formatted by a few threads, written in order
  BoundedQueue<SearchBatch> units_{4};
  BatchPool pool_{16};
  std::unique_ptr<SearchBatch> unit_;   // (the assembler's: the unit being filled)
  uint64_t unit_seq_ = 0;
  // the file's batches in file order: one region (every replica's feeders take its batches) or one region per replica
  std::unique_ptr<DeviceBamSelect<DevOut>> one_;
  std::unique_ptr<ShardedBamSelect<DevOut>> sharded_;
  std::unique_ptr<OrderedWriter> writer_;
};
// a batch through the device on replica (r + dev): the whole of it -- or, early, while the index is not resident, its front
// half, the reads parked
BamRunFn DevicePath::run_on(size_t r) {
  return BamRunFn([this, r](svdss_bam_stream_t* st, int64_t seq, int32_t last, int64_t sk, size_t dev, int32_t nc, const uint8_t* const* comp, const int64_t* cb,
                            const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* nb, svdss_bam_batch_t** batch) {
    const auto t0 = now();
    svdss_index_t* ix = early_ ? early_->index_for_feeders() : replicas_[(r + dev) % replicas_.size()];
    int rc = ix ? svdss_bam_batch_run(st, seq, last, sk, ix, nc, comp, cb, blocks, crc, nb, flags_, batch)
                : svdss_bam_batch_front(st, seq, last, sk, 0, early_->park, nc, comp, cb, blocks, crc, nb, flags_, batch);
    if (rc == SVDSS_OK && !ix) {
      int64_t grp = -1;
      check(svdss_bam_batch_parked(*batch, &grp, nullptr, nullptr), "svdss_bam_batch_parked");
      svdss_bam_result_t r0;
      check(svdss_bam_batch_result(*batch, &r0), "svdss_bam_batch_result");
      int64_t job_comp = 0;
      for (int32_t k = 0; k < nc; ++k) job_comp += cb[k];
      early_->note_batch(r0.n_records, r0.n_searched, job_comp);
      if (grp == -1) rc = svdss_bam_batch_search(*batch, early_->wait_for_index());   // no room in the park
      // (grp == -2: nothing to search in this batch, its results are complete)
    }
    std::lock_guard<std::mutex> lk(t_.m);
    t_.gpu += secs(t0, now());
    return rc;
  });
}
// what a batch object holds after its run -> reads with their SFS.  A batch whose reads went into the park has names and
// tags only: it waits in the EarlySearch, and drain_park delivers it when its group has been searched.
std::unique_ptr<DevOut> DevicePath::collect(const svdss_bam_batch_t* batch, uint64_t seq) {
  const auto t1 = now();
  int64_t grp = -1, first = 0, n_srch = 0;
  const bool parked = early_ && svdss_bam_batch_parked(batch, &grp, &first, &n_srch) == SVDSS_OK && grp >= 0;
  svdss_bam_result_t r;
  check(svdss_bam_batch_result(batch, &r), "svdss_bam_batch_result");
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
  {
    std::lock_guard<std::mutex> lk(t_.m);
    t_.unpack += secs(t1, now()); t_.inflate_ms += r.inflate_kernel_ms;
    t_.n_seen += (uint64_t)r.n_records; ++t_.n_batches;
    for (int k = 0; k < 8; ++k) t_.device[k] += r.stage_ms[k] * 1e-3;
  }
  if (!parked) return out;
  early_->add_pending(grp, EarlySearch::Pending{seq, std::move(out), first, n_srch});
  return nullptr;
}
// the reads of a device batch into the unit being filled; full units go to the formatters
void DevicePath::deal(DevOut& d) {
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
void DevicePath::assemble() {
  unit_ = pool_.get();
  while (std::unique_ptr<DevOut> d = next()) deal(*d);
  const BamRunError e = one_ ? one_->failure() : sharded_->failure();
  if (e.failed()) {
    if (e.msg.find("core.tid") != std::string::npos) die(e.msg);                       // ping_pong.cpp:76-79
    if (e.rc == SVDSS_EIO) die("error reading " + o_.bam + ": " + e.msg);
    die(std::string("svdss_bam_batch_run: ") + svdss_strerror(e.rc) + " " + e.msg + " " + e.hip);
  }
  if (!unit_->reads.empty()) { unit_->seq = unit_seq_++; units_.push(std::move(unit_)); }
  units_.close();
}
// early: once the index is resident, the parked groups -- ONE launch each, one lane per read -- and their batches' results
void DevicePath::drain_park() {
  svdss_index_t* ix = early_->wait_for_offered_index();
  svdss_sfs_batch_t* sfs = nullptr;
  std::vector<int64_t> counts, prefix;
  std::vector<int32_t> qs, ln;
  int64_t n_parked = 0, n_parked_batches = 0, n_groups = 0, n_early_groups = 0;
  double t_search = 0;
  bool closed = false;
  for (int64_t g = 0;; ++g) {
    // the next group: one that has closed while the index is held back from the feeders, or -- once the feeders have the
    // index and the park is closed -- whatever is left
    for (;;) {
      if (!closed && early_->released()) {
        check(svdss_bam_park_close(early_->park), "svdss_bam_park_close");
        closed = true;
        n_groups = svdss_bam_park_groups(early_->park);
      }
      if (closed || svdss_bam_park_group_ready(early_->park, g)) break;
      early_->nap();
    }
    if (closed && g >= n_groups) break;
    if (!closed) ++n_early_groups;
    int64_t nb = 0, nr = 0, ns = 0;
    check(svdss_bam_park_group(early_->park, g, &nb, &nr, &ns), "svdss_bam_park_group");
    const auto t0 = now();
    check(svdss_bam_park_search(early_->park, g, ix, flags_, &sfs), "svdss_bam_park_search");
    const int64_t total = svdss_sfs_batch_total(sfs);
    counts.resize((size_t)nr); qs.resize((size_t)total); ln.resize((size_t)total);
    check(svdss_sfs_batch_fetch(sfs, counts.data(), qs.data(), ln.data(), nullptr), "svdss_sfs_batch_fetch");
    t_search += secs(t0, now());
    prefix.assign((size_t)nr + 1, 0);
    for (int64_t i = 0; i < nr; ++i) prefix[(size_t)i + 1] = prefix[(size_t)i] + counts[(size_t)i];
    for (EarlySearch::Pending& P : early_->take_group(g, nb)) {
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
      one_->deliver(P.seq, std::move(P.out));
    }
    n_parked += nr; n_parked_batches += nb;
  }
  if (sfs) svdss_sfs_batch_free(sfs);
  { std::lock_guard<std::mutex> lk(t_.m); t_.device[5] += t_search; }
  if (o_.verbose)
    logmsg("debug", "front end beside the index restore: " + std::to_string(n_parked_batches) + " batches (" + std::to_string(early_->records.load()) +
                        " records) had been read when the index was resident; their " + std::to_string(n_parked) + " reads searched in " +
                        std::to_string(n_groups) + " launch(es), " + std::to_string(t_search) + " s" +
                        (n_early_groups ? " (" + std::to_string(n_early_groups) + " of them while the file was still being read)" : "") + ", done at +" + clock_.since() + " s");
}
void DevicePath::format_units() {
  while (std::unique_ptr<SearchBatch> u = units_.pop()) {
    const auto tf = now();
    format_batch(o_, *u);
    { std::lock_guard<std::mutex> lk(t_.m); t_.format += secs(tf, now()); }
    writer_->put(std::move(u));
  }
}
void DevicePath::run() {
  const size_t pending = 8;       // (results of the region being dealt that may wait for the assembler)
  auto collect_fn = [this](const svdss_bam_batch_t* batch, uint64_t seq) { return collect(batch, seq); };
  if (in_.n_regions() == 1) {
    DeviceBamSelect<DevOut>::Region rg;
    rg.pending = pending;
    one_.reset(new DeviceBamSelect<DevOut>(o_.bam, replicas_.size(), in_.n_ref, in_.skip, knobs_.feeders, knobs_.batch_bytes, run_on(0), collect_fn, nullptr, rg,
                                           in_.scanner_ptrs[0]));
  } else {
    ShardedBamSelect<DevOut>::Hooks hk;
    hk.run = [this](size_t g, bool) { return run_on(g); };
    hk.collect = [collect_fn](size_t, bool) { return DeviceBamSelect<DevOut>::CollectFn(collect_fn); };
    hk.again = [this](size_t g, const std::string& why) {
      if (o_.verbose) logmsg("debug", "region " + std::to_string(g) + " runs again from the end of region " + std::to_string(g - 1) +
                                          (why.empty() ? std::string(" (its first record was not where the chain arrives)") : " (" + why + ")"));
    };
    sharded_.reset(new ShardedBamSelect<DevOut>(o_.bam, hk, in_.n_ref, in_.skip, knobs_.feeders, knobs_.batch_bytes, in_.cuts, pending, in_.scanner_ptrs));
  }
  std::thread assembler([this] { assemble(); });
  writer_.reset(new OrderedWriter(pool_));
  // (formatting the text costs about one core-second per million reads: five threads per GPU, as many as the cores allow)
  const int n_fmt = knobs_.format_threads ? knobs_.format_threads : (int)std::max<size_t>(5, std::min<size_t>(5 * replicas_.size(), effective_cpus()));
  std::vector<std::thread> fmt;
  for (int k = 0; k < n_fmt; ++k) fmt.emplace_back([this] { format_units(); });
  if (early_) {
    std::thread drain([this] { drain_park(); });
    one_->wait_finished();
    early_->front_finished();
    drain.join();
  }
  assembler.join();
  for (std::thread& th : fmt) th.join();
  writer_->finish();
  if (o_.verbose) report();
}
void DevicePath::report() {
  int64_t n_seg = 0;
  const int64_t n_rewalk = one_ ? one_->segments_walked_again(&n_seg) : sharded_->segments_walked_again(&n_seg);
  logmsg("debug", std::to_string(t_.n_seen) + " records read, " + std::to_string(writer_->lines()) + " SFS written at +" + clock_.since() + " s");
  if (sharded_)
    logmsg("debug", std::to_string(sharded_->n_regions()) + " regions of the file, one per GPU: " + std::to_string(sharded_->seams_run()) + " seam(s) run, " +
                        std::to_string(sharded_->regions_run_again()) + " region(s) run again");
  logmsg("debug", "device path: " + std::to_string(t_.n_batches) + " batches, " + std::to_string(n_seg) + " segments (" + std::to_string(n_rewalk) +
                      " walked again); busy seconds: GPU batches " + std::to_string(t_.gpu) + " (inflate kernels " + std::to_string(t_.inflate_ms * 1e-3) +
                      "), result unpacking " + std::to_string(t_.unpack) + ", re-dealing " + std::to_string(t_.assemble) + ", format " + std::to_string(t_.format) +
                      ", write " + std::to_string(writer_->busy_seconds()));
  char buf[480];
  snprintf(buf, sizeof buf, "device batches, seconds summed: upload+inflate+crc+walk %.3f, waiting for the turn %.3f, turn (carry, link) %.3f, "
           "fields+scans %.3f, unpack %.3f, search %.3f, results down %.3f; the batchers waited %.3f s for the file's loaders and %.3f s for the feeding threads",
           t_.device[0], t_.device[1], t_.device[2], t_.device[3], t_.device[4], t_.device[5], t_.device[6], one_ ? one_->waited_for_file() : sharded_->waited_for_file(),
           one_ ? one_->waited_for_feeders() : sharded_->waited_for_feeders());
  logmsg("debug", buf);
}

// ---- the host path: `search --fastx`, and `search --bam` through BamReader (SVDSS_BAM_DEVICE=0, or no regular file):
// producer (records sliced and decoded, or FASTX parsed) -> GPU workers (search + text) -> writer
class HostPath {
 public:
  HostPath(const Options& o, const SearchKnobs& knobs, const std::vector<svdss_index_t*>& replicas, BamReader* bam, FastxReader* fx, const Stopwatch& clock)
      : o_(o), knobs_(knobs), replicas_(replicas), bam_(bam), fx_(fx), clock_(clock), super_(reads_per_unit(o)) {}
  void run();
 private:
  void parallel_for(size_t n, const std::function<void(size_t, size_t)>& body);
  bool fill_from_bam(SearchBatch& bt);     // (false: the input has ended)
  bool fill_from_fastx(SearchBatch& bt);
  void produce();
  void gpu_worker(svdss_index_t* ix);

  const Options& o_;
  const SearchKnobs& knobs_;
  const std::vector<svdss_index_t*>& replicas_;
  BamReader* const bam_;
  FastxReader* const fx_;
  const Stopwatch& clock_;
  const int64_t super_;
  // (threads of the small per-batch loops -- tag decoding, the copy of the packed bases; --io-threads sizes the inflate pool)
  const int n_workers_ = (int)std::max(1u, std::min(16u, effective_cpus()));
  StageSeconds t_;
  BoundedQueue<SearchBatch> parsed_{4};
  BatchPool pool_{32};
  PinnedPool pinned_;
  // searched batches wait here for their turn: the GPU threads finish them out of order
  std::unique_ptr<OrderedWriter> writer_;
};
// items [0, n) over the worker threads, contiguous slices
void HostPath::parallel_for(size_t n, const std::function<void(size_t, size_t)>& body) {
  const size_t nt = std::min<size_t>((size_t)n_workers_, std::max<size_t>(1, n / 64));
  if (nt <= 1) { body(0, n); return; }
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nt; ++t) pool.emplace_back(body, n * t / nt, n * (t + 1) / nt);
  body(0, n / nt);
  for (std::thread& th : pool) th.join();
}
// locate the records of one batch in the inflated chunks (sequential, no copies: the chunks are kept
// alive until the batch is decoded), then decode them in parallel
bool HostPath::fill_from_bam(SearchBatch& bt) {
  bool more = true;
  std::vector<BamReader::RawView> recs;
  std::vector<std::shared_ptr<BamReader::Bytes>> keep_chunks;
  uint64_t seen_chunk = ~0ull;
  const auto ts0 = now();
  while ((int64_t)recs.size() < super_) {
    BamReader::RawView rr;
    const int rc = bam_->next_view(rr);
    if (rc == 0) { more = false; break; }
    if (rc < 0) die("error reading " + o_.bam + ": " + bam_->error());
    if (bam_->chunk_id() != seen_chunk) { seen_chunk = bam_->chunk_id(); keep_chunks.push_back(bam_->chunk()); }
    ++t_.n_seen;
    bool keep = !(rr.flag & (4 | 2048 | 256));                     // ping_pong.cpp:66-69
    if (keep && rr.l_seq < 100) {                                  // :70-75
      logmsg("warning", "Alignment filtered due to l_qseq. Why are we here? Please check");
      keep = false;
    }
    if (keep && rr.tid < 0) die("core.tid < 0. Why are we here? Please check");  // :76-79
    if (!keep) continue;
    recs.push_back(std::move(rr));
  }
  const auto ts1 = now();
  t_.slice += secs(ts0, ts1);
  const size_t n = recs.size();
  bt.reads.resize(n);
  parallel_for(n, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      const BamReader::RawView& rr = recs[i];
      Read& r = bt.reads[i];
      r.name.assign((const char*)rr.name(), rr.l_name ? rr.l_name - 1 : 0);
      int64_t xf = 0, hp = 0;
      BamReader::aux_int(rr.aux(), rr.l_aux, "XF", xf);   // :196-201, missing => 0
      BamReader::aux_int(rr.aux(), rr.l_aux, "HP", hp);
      r.hp = (int)hp;
      if (o_.putative && xf != 0) { r.count = -1; r.len = 0; }                 // :202-203
      else r.len = rr.l_seq;
    }
  });
  for (size_t i = 0; i < n; ++i) {
    if (bt.reads[i].count < 0) continue;
    bt.gidx.push_back(i);
    bt.goff.push_back(bt.goff.back() + bt.reads[i].len);
  }
  bt.boff.assign(1, 0);
  bt.lseq.resize(bt.gidx.size());
  for (size_t k = 0; k < bt.gidx.size(); ++k) {
    const int32_t l = recs[bt.gidx[k]].l_seq;
    bt.lseq[k] = l;
    bt.boff.push_back(bt.boff.back() + ((int64_t)l + 1) / 2);
  }
  // the packed bases of the batch, back to back in page-locked memory; the inflated chunks go back to the reader
  // at once (they are page-locked too when the GPU inflates: few should be in flight)
  if (!bt.gidx.empty()) {
    bt.seq4 = pinned_.get((size_t)bt.boff.back() + 16, bt.seq4_cap);
    parallel_for(bt.gidx.size(), [&](size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; ++k)
        memcpy(bt.seq4 + bt.boff[k], recs[bt.gidx[k]].seq4(), (size_t)(bt.boff[k + 1] - bt.boff[k]));
    });
  }
  t_.decode += secs(ts1, now());
  return more;
}
bool HostPath::fill_from_fastx(SearchBatch& bt) {
  while ((int64_t)bt.reads.size() < super_) {
    Read r;
    std::string seq;
    if (!fx_->next(r.name, seq)) return false;
    ++t_.n_seen;
    r.len = (int64_t)seq.size();
    const size_t at = bt.gbuf.size();
    bt.gbuf.resize(at + seq.size());
    svdss_nt6_encode(seq.data(), (int64_t)seq.size(), bt.gbuf.data() + at);
    bt.goff.push_back((int64_t)bt.gbuf.size());
    bt.gidx.push_back(bt.reads.size());
    bt.reads.push_back(std::move(r));
  }
  return true;
}
void HostPath::produce() {
  uint64_t next_seq = 0;
  for (bool more = true; more;) {
    std::unique_ptr<SearchBatch> bt = pool_.get();
    bt->goff.assign(1, 0);
    more = bam_ ? fill_from_bam(*bt) : fill_from_fastx(*bt);
    if (!bt->reads.empty()) { bt->seq = next_seq++; parsed_.push(std::move(bt)); }
  }
  parsed_.close();
}
// the thread that searched a batch also formats its text, the writer only writes
void HostPath::gpu_worker(svdss_index_t* ix) {
  svdss_sfs_batch_t* res = nullptr;
  while (std::unique_ptr<SearchBatch> bt = parsed_.pop()) {
    const auto tg0 = now();
    if (!bt->gidx.empty()) {
      std::vector<int64_t>& counts = bt->counts;
      counts.assign(bt->gidx.size(), 0);
      if (bam_)
        check(svdss_sfs_search_batch_bam(ix, bt->seq4, bt->boff.data(), bt->lseq.data(), (int64_t)bt->gidx.size(),
                                         o_.assemble ? SVDSS_SFS_ASSEMBLE : 0, &res), "svdss_sfs_search_batch_bam");
      else
        check(svdss_sfs_search_batch(ix, bt->gbuf.data(), bt->goff.data(), (int64_t)bt->gidx.size(),
                                     o_.assemble ? SVDSS_SFS_ASSEMBLE : 0, &res), "svdss_sfs_search_batch");
      bt->qs.resize((size_t)svdss_sfs_batch_total(res));
      bt->ln.resize(bt->qs.size());
      check(svdss_sfs_batch_fetch(res, counts.data(), bt->qs.data(), bt->ln.data(), nullptr), "svdss_sfs_batch_fetch");
      int64_t acc = 0;
      for (size_t k = 0; k < bt->gidx.size(); ++k) {
        bt->reads[bt->gidx[k]].first = acc;
        bt->reads[bt->gidx[k]].count = counts[k];
        acc += counts[k];
      }
    }
    bt->gbuf.clear();
    pinned_.put(bt->seq4, bt->seq4_cap);
    bt->seq4 = nullptr;
    const auto tg1 = now();
    format_batch(o_, *bt);
    { std::lock_guard<std::mutex> lk(t_.m); t_.gpu += secs(tg0, tg1); t_.format += secs(tg1, now()); }
    writer_->put(std::move(bt));
  }
  svdss_sfs_batch_free(res);
}
void HostPath::run() {
  std::thread producer([this] { produce(); });
  writer_.reset(new OrderedWriter(pool_));
  {
    // (several feeding threads per GPU, each with its own batch object and stream: upload, search, download and the
    // text formatting of different batches overlap; formatting alone needs four to five threads at a million reads/s)
    std::vector<std::thread> gpu_threads;
    for (size_t d = 0; d < replicas_.size(); ++d)
      for (int k = 0; k < knobs_.feeders; ++k)
        if (d || k) gpu_threads.emplace_back([this, d] { gpu_worker(replicas_[d]); });
    gpu_worker(replicas_[0]);
    for (std::thread& th : gpu_threads) th.join();
  }
  producer.join();
  writer_->finish();
  if (o_.verbose) {
    logmsg("debug", std::to_string(t_.n_seen) + " records read, " + std::to_string(writer_->lines()) + " SFS written at +" + clock_.since() + " s");
    logmsg("debug", "stage busy seconds: inflate+slice " + std::to_string(t_.slice) + ", decode " + std::to_string(t_.decode) +
                        ", GPU search + copies " + std::to_string(t_.gpu) + ", format " + std::to_string(t_.format) + ", write " + std::to_string(writer_->busy_seconds()));
  }
}

// ---- the run, stage by stage
struct SearchRun {
  SearchRun(const Options& opts, time_t process_start) : o(opts), t_process(process_start) {}
  void open_input();
  void start_front_end_early();
  void load_index();
  void choose_kmer_order();
  void choose_rank_blocks_alone();
  void index_to_device();
  void release_index_to_front_end();
  void replicate();
  void run_device_path();
  void run_host_path();
  int finish();

  const Options& o;
  const time_t t_process;              // process start (the final log line)
  const SearchKnobs knobs{};
  const Stopwatch clock{};
  const bool bam_mode = !o.bam.empty();
  // BAM records handled on the GPU (csrc/bam_device.hip; the default when there is one): only compressed bytes go up.
  // SVDSS_BAM_DEVICE=0: the host path (BamReader: chunks inflated on the GPU or by the host pool, records sliced
  // on the host, packed bases uploaded) -- the tested fallback, and what a reader of stdin-like inputs needs.
  const bool dev_bam = bam_mode && svdss_device_count() > 0 && knobs.bam_device;
  const int n_dev = std::max(1, svdss_device_count());
  const int n_gpus = effective_gpus(o.gpus);
  DeviceBamInput in;                   // dev_bam
  std::unique_ptr<BamReader> bam;      // BAM on the host path
  std::unique_ptr<FastxReader> fx;
  std::thread prewarm;
  std::unique_ptr<EarlySearch> early;
  std::thread front_end;
  svdss_index_t* ix = nullptr;
  bool user_kmer = false, lf_only = false;
  std::vector<svdss_index_t*> replicas;
};
void SearchRun::open_input() {
  if (dev_bam) {
    std::string herr;
    if (!bam_header_probe(o.bam, in.n_ref, in.skip, herr, nullptr)) die("cannot read " + o.bam + ": " + herr);
    BgzfScanner::Hooks hooks;
    hooks.host_alloc = svdss_host_alloc;
    hooks.host_free = svdss_host_free;
    // slabs alive at once: those the loaders read ahead + those of the batches being fed, queued and cut
    const size_t per_batch = (size_t)knobs.batch_bytes / knobs.slab_bytes + 2;
    // the file's regions, one per GPU (one region for a small file, or SVDSS_REGION_SHARDS=0: every GPU's feeders take its batches)
    in.cuts = plan_bam_regions(o.bam, n_gpus, in.skip);
    const size_t n_regions = in.n_regions();
    const int loaders = n_regions > 1 ? std::max(2, std::min(knobs.loaders, (int)effective_cpus() / (int)n_regions)) : knobs.loaders;
    const size_t feeders_per_region = n_regions > 1 ? (size_t)knobs.feeders : (size_t)(n_gpus * knobs.feeders);
    const size_t pool_chunks = (size_t)loaders + (feeders_per_region + 3) * per_batch;
    for (size_t g = 0; g < n_regions; ++g) {
      in.scanners.emplace_back(new BgzfScanner(o.bam, hooks, knobs.slab_bytes, loaders, pool_chunks, in.cuts[g], in.cuts[g + 1]));
      if (!in.scanners.back()->ok()) die("cannot open " + o.bam);
      in.scanner_ptrs.push_back(in.scanners.back().get());
    }
    if (knobs.prewarm)
      prewarm = std::thread([this] {
        std::vector<std::thread> th;
        for (std::unique_ptr<BgzfScanner>& sc : in.scanners) th.emplace_back([&sc] { sc->prewarm(); });
        for (std::thread& t : th) t.join();
      });
  } else if (bam_mode) {
    // the reader's page-locked chunk buffers are allocated while the index is restored (BamReader::prewarm)
    bam.reset(new BamReader(o.bam, o.io_threads));
    // (BGZF blocks inflated on the GPU, csrc/inflate.hip, on every GPU of --gpus in turn; SVDSS_GPU_INFLATE)
    svdss_enable_gpu_inflate(*bam, 0, std::min(n_gpus, n_dev));
    if (bam->ok() && knobs.prewarm) prewarm = std::thread([this] { bam->prewarm(); });
  }   // (FASTX: opened when the index is resident, run_host_path)
}
// One GPU, one region: the BAM front end starts NOW, beside the index restore (EarlySearch; SVDSS_SEARCH_EARLY=0: the index
// first, as PingPong::run does, ping_pong.cpp:245,329).  The park's first arena is allocated before the restore begins.
void SearchRun::start_front_end_early() {
  // (It pays when the restore takes seconds: an index of a chr20-length reference is resident in 0.4 s, and sharing the GPU
  // with the front end meanwhile only delays it -- 1.87 against 1.55 s per 1.03 M reads, profiles/r06t_*.  The sidecar holds
  // a byte per BWT symbol (records + rank blocks): from 800 MB on -- ~0.8 G symbols, a restore of ~0.7 s -- the front end starts first;
  // SVDSS_SEARCH_EARLY=1 forces it, SVDSS_EARLY_MIN_MB moves the threshold.)
  bool early_pays = knobs.early == 1;
  if (!early_pays) {
    struct stat sti;
    if (stat((o.index + ".svdss").c_str(), &sti) == 0 || stat(o.index.c_str(), &sti) == 0) early_pays = (int64_t)sti.st_size >= (knobs.early_min_mb << 20);
  }
  if (!(dev_bam && early_pays && in.n_regions() == 1 && n_gpus == 1 && knobs.early != 0)) return;
  if (o.bsize <= 0) die("batch size smaller than the number of threads");
  early.reset(new EarlySearch);
  struct stat stb;
  early->file_bytes = stat(o.bam.c_str(), &stb) == 0 ? (int64_t)stb.st_size : 0;
  // (on a thread of its own from the first moment: this one goes straight to the index file)
  front_end = std::thread([this] {
    check(svdss_bam_park_create(0, knobs.park_bytes, knobs.park_bytes / 512 + 4096, &early->park), "svdss_bam_park_create");
    if (prewarm.joinable()) prewarm.join();
    DevicePath(o, knobs, std::vector<svdss_index_t*>(1, nullptr), in, clock, early.get()).run();
  });
}
// (Tried: the rank blocks of the sidecar read beside the records, on a thread of their own, so that they are in memory when
// the choice falls.  Two 3 GB reads and the front end's start share the process's cores: the front end's estimate came
// 0.4 s later and the blocks no sooner -- 5x `search` 2.4 -> 2.7 s.  They are read when they are wanted.)
void SearchRun::load_index() {
  check(svdss_index_load(o.index.c_str(), &ix), "svdss_index_load");
  if (early) early->index_n.store(svdss_index_size(ix));
  if (o.verbose) logmsg("debug", "index file read at +" + clock.since() + " s");
}
void SearchRun::choose_kmer_order() {
  user_kmer = getenv("SVDSS_KMER") != nullptr;      // (this function may set the variable itself)
  if (user_kmer) return;
  // The order K of the k-mer table trades its build time (4^K entries: 1.6 s at K = 16, a quarter of that per step
  // down) against the search kernel's speed (about a third slower per step down).  The library's own choice (K = 16
  // from 64 Mb on) is the one for a resident index that searches batch after batch; a process that restores the
  // index for ONE input knows roughly how many reads are coming (a BAM is ~1 byte per base, a FASTQ ~2) and takes the
  // K that minimises build + search.  Results never depend on K (tests/test_sfs_gpu.py, tests/test_scale_gpu.py).
  struct stat st;
  const std::string& input = bam_mode ? o.bam : o.fastx;
  // (references above 2^31 symbols keep the library's K: nothing below 16 was measured there)
  const int64_t n = svdss_index_size(ix);
  if (stat(input.c_str(), &st) != 0 || st.st_size <= 0 || n >= ((int64_t)1 << 31)) return;
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
  if (best == k_auto) return;
  setenv("SVDSS_KMER", std::to_string(best).c_str(), 0);
  if (o.verbose) logmsg("debug", "k-mer table of order " + std::to_string(best) + " for ~" + std::to_string((long long)est_reads) + " reads");
}
// Few reads to search (the front end has seen enough to say: `search` on a smoothed BAM skips what `smooth` tagged XF != 0)
// and the sidecar carries the rank blocks: the index as a rank structure ALONE -- 3 GB uploaded instead of six billion
// suffixes sorted for a text, a suffix array and a k-mer table; ~1 M reads/s instead of 8 - 24 M, results identical
// (svdss_index_attach_blocks).  SVDSS_SEARCH_LF=0|1 forces the choice, SVDSS_SEARCH_LF_MAX moves the threshold (reads).
void SearchRun::choose_rank_blocks_alone() {
  if (!early || user_kmer || knobs.lf == 0) return;
  const bool forced = knobs.lf == 1;
  const auto w0 = now();
  while (!forced && !early->front_is_finished() && early->records.load() < 50000 && secs(w0, now()) <= 1.5)
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
  const double est = early->estimate_reads_to_search();
  const std::string t_est = clock.since();
  // (what the rank structure alone saves is the rest of the restore -- ~4.5 s at GRCh38 lengths, in proportion for a
  // smaller reference --, what it costs is the search at ~1 M reads/s instead of 8 - 24 M: worth it below ~2 M reads
  // per 6.2e9 BWT symbols; profiles/r06q_*)
  const double lf_max = knobs.lf_max_set ? knobs.lf_max : 2e6 * (double)svdss_index_size(ix) / 6.18e9;
  if (!forced && !(est >= 0 && est <= lf_max)) return;
  const int rc = svdss_index_attach_blocks(ix, o.index.c_str());
  if (rc == SVDSS_OK) {
    lf_only = true;
    if (o.verbose) logmsg("debug", "~" + std::to_string((long long)std::max(0.0, est)) + " reads to search (known at +" + t_est + " s): the index as a rank structure alone (blocks read at +" + clock.since() + " s)");
  } else if (rc != SVDSS_EINVAL) check(rc, "svdss_index_attach_blocks");
}
void SearchRun::index_to_device() {
  check(svdss_index_to_device(ix, 0), "svdss_index_to_device");
  if (o.verbose) logmsg("debug", "index and k-mer table on the device at +" + clock.since() + " s" +
                                     (lf_only ? " (rank blocks alone: few reads to search)"
                                      : early && svdss_index_kmer(ix) < 16 ? " (table of order " + std::to_string(svdss_index_kmer(ix)) + ": few reads to search)" : ""));
}
// the early path's second half: the front end gets the index, searches what it parked and goes on with whole batches
void SearchRun::release_index_to_front_end() {
  if (lf_only) early->offer_index_held_back(ix);
  logmsg("info", "Extracting SFS strings on the GPU (output order as with " + std::to_string(o.threads) + " threads)..");
  // (SVDSS_EARLY_HOLD_MS, for the tests: the index is held back that long, as if its restore had taken seconds)
  if (knobs.early_hold_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(knobs.early_hold_ms));
  early->release_index(ix);
  front_end.join();
  replicas.assign(1, ix);
}
// --gpus N: one replica of the index per GPU; the batches of reads go to whichever GPU is free, the
// text is written in input order whatever GPU searched a batch -- the same bytes as with one GPU
// (more replicas than GPUs, effective_gpus: replica d on GPU d % count -- exercises the path on a one-GPU box)
void SearchRun::replicate() {
  replicas.assign((size_t)n_gpus, ix);
  // every replica is built in the HBM of its own GPU from the records (or copied there), all of them at once
  std::vector<std::thread> th;
  std::vector<int> rcs((size_t)n_gpus, SVDSS_OK);
  for (int d = 1; d < n_gpus; ++d)
    th.emplace_back([this, &rcs, d] { rcs[(size_t)d] = svdss_index_replicate(ix, d % n_dev, &replicas[(size_t)d]); });
  for (std::thread& t : th) t.join();
  for (int d = 1; d < n_gpus; ++d) check(rcs[(size_t)d], "svdss_index_replicate");
  if (n_gpus > 1) logmsg("info", "Index replicated on " + std::to_string(n_gpus) + " GPUs");
}
void SearchRun::run_device_path() {
  if (prewarm.joinable()) prewarm.join();
  if (o.bsize <= 0) die("batch size smaller than the number of threads");
  logmsg("info", "Extracting SFS strings on the GPU (output order as with " + std::to_string(o.threads) + " threads)..");
  // region g on GPU g (one region: every GPU's feeders take its batches)
  if (o.verbose && in.n_regions() > 1) {
    std::string m = "file regions (bytes):";
    for (size_t g = 0; g + 1 < in.cuts.size(); ++g) m += " " + std::to_string(in.cuts[g + 1] - in.cuts[g]);
    logmsg("debug", m);
  }
  DevicePath(o, knobs, replicas, in, clock).run();
}
void SearchRun::run_host_path() {
  if (bam_mode) {
    if (prewarm.joinable()) prewarm.join();
    if (!bam->ok() || !bam->read_header()) die("cannot read " + o.bam + ": " + bam->error());
  } else {
    logmsg("warning", "FASTX mode is not optimized (higher running times and larger SFSs set).");
    fx.reset(new FastxReader(o.fastx));
    if (!fx->ok()) die("cannot open " + o.fastx);
  }
  if (o.bsize <= 0) die("batch size smaller than the number of threads");
  logmsg("info", "Extracting SFS strings on the GPU (output order as with " + std::to_string(o.threads) + " threads)..");
  HostPath(o, knobs, replicas, bam.get(), fx.get(), clock).run();
}
// Everything is written.  Giving back gigabytes of page-locked buffers and the index on the device one by one takes
// half a second that the operating system spends anyway when the process ends: end it here (SVDSS_CLEAN_EXIT=1 keeps
// the orderly teardown, for leak checkers; main says "All done" then).
int SearchRun::finish() {
  if (!knobs.clean_exit) {
    if (bam) bam->report();
    logmsg("info", "All done! Runtime: " + std::to_string((long)(time(nullptr) - t_process)) + " seconds");
    fflush(stdout);
    fflush(stderr);
    _exit(0);
  }
  if (early) svdss_bam_park_free(early->park);
  for (svdss_index_t* r : replicas) svdss_index_free(r);
  return 0;
}

}  // namespace

int main_search(const Options& o, time_t process_start) {
  logmsg("info", "Restoring index..");
  SearchRun run(o, process_start);
  run.open_input();
  run.start_front_end_early();
  run.load_index();
  run.choose_kmer_order();
  run.choose_rank_blocks_alone();
  run.index_to_device();
  if (run.early) {
    run.release_index_to_front_end();
  } else {
    run.replicate();
    if (run.dev_bam) run.run_device_path(); else run.run_host_path();
  }
  return run.finish();
}
