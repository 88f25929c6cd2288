// bam_device_select.h -- host side of the device path (csrc/bam_device.hip) for `SVDSS search`, `call` and `smooth`: the BAM
// header probe, and a reader that runs the batches of a file -- or of its regions, one per GPU -- through a device entry
// point of the caller's and hands out what each batch left, in file order.  Scanner (loader threads) -> batcher -> feeding
// threads (one batch object each) -> ordered hand-over with back-pressure.
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bam_reader.h"
#include "bgzf_scanner.h"

// The BAM header read on the host (the first BGZF members, zlib / libdeflate): number of reference sequences and the
// length of the header in the inflated stream -- where the first record begins (sam_hdr_read, ping_pong.cpp:248).
inline bool bam_header_probe(const std::string& path, int32_t& n_ref, int64_t& skip, std::string& err, std::vector<std::string>* ref_names) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { err = "cannot open file"; return false; }
  std::vector<uint8_t> comp, buf;
  size_t pos = 0;
  bool eof = false;
  BgzfInflater inf;
  auto more = [&]() -> bool {        // one more member inflated onto buf
    for (;;) {
      if (pos + 18 <= comp.size()) {
        const uint8_t* h = comp.data() + pos;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) { err = "not a BAM file"; return false; }
        uint16_t xlen;
        memcpy(&xlen, h + 10, 2);
        int bsize = -1;
        if (pos + 12 + xlen <= comp.size()) {
          for (size_t o = 0; o + 4 <= xlen;) {
            const uint8_t* x = h + 12 + o;
            uint16_t slen;
            memcpy(&slen, x + 2, 2);
            if (x[0] == 'B' && x[1] == 'C' && slen == 2 && o + 6 <= xlen) { uint16_t v; memcpy(&v, x + 4, 2); bsize = v; break; }
            o += 4u + slen;
          }
          if (bsize < 0 || (size_t)bsize + 1 < 12u + xlen + 8u) { err = "BGZF block without BC field"; return false; }
          if (pos + (size_t)bsize + 1 <= comp.size()) {
            const size_t clen = (size_t)bsize + 1 - 12 - xlen - 8;
            uint32_t crc, isize;
            memcpy(&crc, h + 12 + xlen + clen, 4);
            memcpy(&isize, h + 12 + xlen + clen + 4, 4);
            if (isize > 65536u) { err = "bad BGZF block"; return false; }
            const size_t at = buf.size();
            buf.resize(at + isize);
            if (isize) if (const char* e = inf.run(h + 12 + xlen, clen, buf.data() + at, isize, crc)) { err = e; return false; }
            pos += (size_t)bsize + 1;
            return true;
          }
        }
      }
      if (eof) { err = "truncated header"; return false; }
      const size_t at = comp.size();
      comp.resize(at + ((size_t)256 << 10));
      const size_t got = fread(comp.data() + at, 1, (size_t)256 << 10, f);
      comp.resize(at + got);
      if (got == 0) eof = true;
    }
  };
  auto need = [&](size_t n) -> bool { while (buf.size() < n) if (!more()) return false; return true; };
  bool ok = false;
  do {
    if (!need(12)) break;
    if (memcmp(buf.data(), "BAM\1", 4) != 0) { err = "not a BAM file"; break; }
    int32_t l_text;
    memcpy(&l_text, buf.data() + 4, 4);
    if (l_text < 0) { err = "corrupt header"; break; }
    if (!need(12 + (size_t)l_text)) break;
    memcpy(&n_ref, buf.data() + 8 + l_text, 4);
    if (n_ref < 0) { err = "corrupt header"; break; }
    size_t o = 12 + (size_t)l_text;
    bool bad = false;
    for (int32_t i = 0; i < n_ref && !bad; ++i) {
      if (!need(o + 4)) { bad = true; break; }
      int32_t l_name;
      memcpy(&l_name, buf.data() + o, 4);
      if (l_name < 0) { err = "corrupt header"; bad = true; break; }
      if (!need(o + 4 + (size_t)l_name + 4)) { bad = true; break; }
      if (ref_names) {
        std::string nm((const char*)buf.data() + o + 4, (size_t)l_name);
        if (!nm.empty() && nm.back() == '\0') nm.pop_back();
        ref_names->push_back(nm);
      }
      o += 4 + (size_t)l_name + 4;
    }
    if (bad) break;
    skip = (int64_t)o;
    ok = true;
  } while (false);
  fclose(f);
  return ok;
}


// --region / --regions-file (bam_regions.h): the command's regions given to a record stream of the device path before its
// batch 0 (svdss_bam_stream_set_regions); none in force: nothing to do
inline int bam_stream_apply_regions(svdss_bam_stream_t* s) {
  const BamRegionSet* U = bam_regions_in_force();
  return U ? svdss_bam_stream_set_regions(s, (int64_t)U->size(), U->tid.data(), U->beg.data(), U->end.data()) : SVDSS_OK;
}

// --verbose with regions in force: one line when the command is done (main, and the commands that end the process themselves).
// Every pass over the file counts: `smooth` measures before it runs, `call` may read a file twice.
inline void bam_regions_report() {
  const BamRegionSet* U = bam_regions_in_force();
  if (!U || !bam_region_counters().verbose) return;
  bam_region_counters().verbose = false;   // (once)
  int64_t on_device = 0;
  (void)svdss_bam_gated_total(&on_device);
  on_device -= bam_region_counters().device_base;
  const BamRegionPlan& plan = bam_region_plan();
  // (the host readers -- SVDSS_BAM_DEVICE=0, SVDSS_SMOOTH_HOST=1, pass 1 of a `call` without the device path -- take no
  // ranges: they read the whole file, and the bytes figure counts the device path's alone)
  if (const long long h = (long long)bam_region_counters().host_readers.load())
    fprintf(stderr, "[regions] %lld host reader(s) read the WHOLE file through the gate, with or without an index; their bytes are not in the figure below\n", h);
  if (plan.active)
    fprintf(stderr, "[regions] %zu interval(s); %zu range(s) of %zu bytes named by %s, %lld compressed bytes read, %lld records gated out\n", U->size(),
            plan.ranges.size(), plan.bytes(), plan.index_path.c_str(), (long long)bam_region_counters().comp_bytes.load(),
            (long long)(bam_region_counters().gated.load() + on_device));
  else
    fprintf(stderr, "[regions] %zu interval(s); no usable index: the whole file goes through the record gate, 1 range, %lld compressed bytes read, "
                    "%lld records gated out\n", U->size(), (long long)bam_region_counters().comp_bytes.load(),
            (long long)(bam_region_counters().gated.load() + on_device));
}

// a batch's input-side index fragments (svdss_bam_batch_input_index), copied off the batch object: what travels with the
// batch's result to whoever folds the index (bam_input_index.h); region / seam: which region of the file the batch is of,
// and whether it is the seam in front of it (ShardedBamSelect)
struct InputFragCopy {
  svdss_bam_input_frag_t f{};
  std::vector<svdss_bam_input_chunk_t> chunks;
  std::vector<svdss_bam_input_window_t> windows;
  size_t region = 0;
  bool seam = false;
  void take(const svdss_bam_batch_t* b, size_t g = 0, bool is_seam = false) {
    region = g; seam = is_seam;
    if (svdss_bam_batch_input_index(b, &f) != SVDSS_OK) { f = svdss_bam_input_frag_t{}; return; }
    chunks.assign(f.chunks, f.chunks + f.n_chunks);
    windows.assign(f.windows, f.windows + f.n_windows);
    f.chunks = nullptr; f.windows = nullptr;
  }
  svdss_bam_input_frag_t frag() const { svdss_bam_input_frag_t r = f; r.chunks = chunks.data(); r.windows = windows.data(); return r; }
};

// the kept records of one device batch, in file order: record k = bytes[off[k] + 4 ..), block_size at bytes[off[k]]
struct SelectedBatch {
  std::vector<uint8_t> bytes;   // (smoothing: the batch's BGZF members)
  std::vector<int64_t> off;
  uint64_t n_records = 0;       // records of the batch, kept or not
  bool slim = false;            // the kept records are slim ones (svdss_bam_selection_t::slim)
  // smoothing (svdss_bam_smooth_run / _measure): kept records, by XF value; matches / mismatches and "CIGAR fits" per kept record
  uint64_t n_kept = 0, n_xf[4] = {0, 0, 0, 0};
  std::vector<int64_t> match_mismatch;
  std::vector<uint8_t> fits;
  const uint8_t* ext = nullptr;   // smoothing: the BGZF members in a page-locked buffer of the caller's pool (ext_n bytes) ...
  size_t ext_n = 0;
  int ext_slot = -1;              // ... and which one, for its return
  double stage_s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, inflate_kernel_s = 0;
  // smoothing with an index asked for: the batch's index fragments (svdss_bam_batch_index; ix's pointers are set by the
  // consumer, into the two vectors)
  std::vector<svdss_bam_index_chunk_t> ix_chunks;
  std::vector<svdss_bam_index_window_t> ix_windows;
  svdss_bam_index_frag_t ix{};
  // --write-bam-index: the batch's input-side fragments (f.on 0: not asked for)
  InputFragCopy in_ix;
};

// a record's view (BamReader::RawView: the zero-copy form the host readers hand out) over bytes that hold it
inline bool view_of_record(const uint8_t* rec, size_t avail, BamReader::RawView& v, bool slim = false) {
  if (avail < 36) return false;
  int32_t block_size;
  memcpy(&block_size, rec, 4);
  if (block_size < 32 || (size_t)block_size + 4 > avail) return false;
  const uint8_t* core = rec + 4;
  v.own.reset();
  v.p = core;
  uint16_t n_cigar;
  memcpy(&v.tid, core, 4);
  memcpy(&v.pos, core + 4, 4);
  v.l_name = core[8];
  v.mapq = core[9];
  memcpy(&n_cigar, core + 12, 2);
  v.n_cigar = n_cigar;
  memcpy(&v.flag, core + 14, 2);
  memcpy(&v.l_seq, core + 16, 4);
  if (v.l_seq < 0) return false;
  const size_t head = 32 + (size_t)v.l_name + 4u * v.n_cigar + ((size_t)v.l_seq + 1) / 2 + (slim ? 0 : (size_t)v.l_seq);
  if (head > (size_t)block_size) return false;
  v.noqual = slim;
  v.l_aux = (uint32_t)((size_t)block_size - head);
  return true;
}

// What a feeding thread does with a batch: one of the device path's entry points (svdss_bam_select_store_run,
// svdss_bam_smooth_run, svdss_bam_batch_run, ...) for device slot `dev` of the reader
typedef std::function<int(svdss_bam_stream_t*, int64_t seq, int32_t is_last, int64_t skip, size_t dev, int32_t n_chunks, const uint8_t* const* comp,
                          const int64_t* comp_bytes, const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                          svdss_bam_batch_t** batch)> BamRunFn;

// why a run failed: the entry point's return code, the batch's or the stream's message (may be empty) and the HIP error
// the failing thread saw
struct BamRunError {
  int rc = SVDSS_OK;
  std::string msg, hip;
  bool failed() const { return rc != SVDSS_OK; }
  std::string text() const { return !failed() ? std::string() : !msg.empty() ? msg : std::string(svdss_strerror(rc)) + " " + hip; }
};

// A region of the file (ShardedBamSelect below): [begin, end) at member starts (end = 0: the file's end); open_start: the
// region begins inside a record nobody has located (svdss_bam_stream_region: the chain starts at a guess, to be proved at
// the seam); open_end: it may end inside one; carry: the incomplete record in front of it when the region runs from a known
// start; pending: batches that may wait for the caller while it reads this region (current: from the start; a later region
// is not bounded until it becomes current -- its results wait until the regions in front are handed out); on_fed: called
// once, by the last feeding thread as it ends (no more batches will be run; results may still be delivered); small_start:
// the run's first batch is cut at a quarter of the batch size and the second at half of it, so that the device has work --
// and whoever counts what the batches hold has figures, and batch 0's head is final -- after a quarter of the bytes
// ix_shift / ix_depth: the stream's input index is switched on (svdss_bam_stream_set_input_index); has_carry_v / carry_v: where
// `carry` begins in the file, relative to the region's first member (svdss_bam_stream_set_input_carry)
struct BamSelectRegion { size_t begin = 0, end = 0; bool open_start = false, open_end = false; std::vector<uint8_t> carry; int loaders = 8; size_t pending = 64; bool current = true;
                         std::function<void()> on_fed; bool small_start = false;
                         int ix_shift = 0, ix_depth = 0; bool has_carry_v = false; int64_t carry_v = 0; };

// One region of a BAM through the device path, batch results handed out in file order as `Out`: scanner (loader threads)
// -> batcher -> feeding threads (n_devices x feeders, one batch object each; `run` is told the device slot) -> ordered
// hand-over with back-pressure.  `collect` turns a batch's result into an Out; it may return nullptr: that batch's result
// is delivered later, by deliver(seq, result) -- it does not count against the pending bound, and the run is not over
// until it has come.
template <class Out>
class DeviceBamSelect {
 public:
  typedef std::function<std::unique_ptr<Out>(const svdss_bam_batch_t*, uint64_t seq)> CollectFn;
  typedef BamSelectRegion Region;
  // scanner: one the caller opened for the region and keeps open past this object (nullptr: one is opened here)
  DeviceBamSelect(const std::string& path, size_t n_devices, int32_t n_ref, int64_t skip, int feeders, int64_t batch_bytes, BamRunFn run,
                  CollectFn collect, svdss_bam_stream_t* prepared_stream = nullptr, const Region& region = Region(), BgzfScanner* scanner = nullptr)
      : skip_(skip), target_(batch_bytes), run_(run), collect_(collect), sc_(scanner), stream_(prepared_stream), max_pending_(region.pending),
        current_(region.current), on_fed_(region.on_fed), small_start_(region.small_start) {
    feeders = std::max(1, feeders);
    if (!sc_) {
      BgzfScanner::Hooks hooks;
      hooks.host_alloc = svdss_host_alloc;
      hooks.host_free = svdss_host_free;
      const size_t slab = (getenv("SVDSS_BAM_SLAB_KB") && atoll(getenv("SVDSS_BAM_SLAB_KB")) >= 64 ? (size_t)atoll(getenv("SVDSS_BAM_SLAB_KB")) << 10 : (size_t)16 << 20);
      const size_t per_batch = (size_t)target_ / slab + 2;
      own_sc_.reset(new BgzfScanner(path, hooks, slab, region.loaders, (size_t)region.loaders + (n_devices * (size_t)feeders + 3) * per_batch, region.begin,
                                    region.end));
      sc_ = own_sc_.get();
    }
    if (!sc_->ok()) { err_ = BamRunError{SVDSS_EIO, "cannot open file", ""}; return; }
    // --region with an index (bam_region_plan): the scanner reads the index's ranges; the first record is where the first
    // range says, and the stream may end inside the record its last range cuts
    const bool ranged = sc_->ranged();
    if (ranged) skip_ = sc_->first_skip();
    if (!stream_ && svdss_bam_stream_create(n_ref, &stream_) != SVDSS_OK) { err_ = BamRunError{SVDSS_ENOMEM, "out of memory", ""}; return; }
    if (const int rc = bam_stream_apply_regions(stream_)) { err_ = BamRunError{rc, "the regions do not fit the BAM header", ""}; return; }
    if (region.open_start || region.open_end || ranged || !region.carry.empty())
      if (svdss_bam_stream_region(stream_, region.open_start ? 1 : 0, region.open_end || ranged ? 1 : 0, region.carry.data(), (int64_t)region.carry.size()) != SVDSS_OK) {
        err_ = BamRunError{SVDSS_ENOMEM, "out of memory", ""}; return;
      }
    if (region.ix_shift > 0 && (svdss_bam_stream_set_input_index(stream_, region.ix_shift, region.ix_depth) != SVDSS_OK ||
                                (region.has_carry_v && svdss_bam_stream_set_input_carry(stream_, region.carry_v) != SVDSS_OK))) {
      err_ = BamRunError{SVDSS_EINVAL, "the input index cannot be switched on", ""}; return;
    }
    n_feeders_ = n_devices * (size_t)feeders;
    batcher_ = std::thread([this] { batch_loop(); });
    for (size_t d = 0; d < n_devices; ++d)
      for (int k = 0; k < feeders; ++k) feeders_.emplace_back([this, d] { feed_loop(d); });
  }
  ~DeviceBamSelect() {
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
    cv_.notify_all();
    if (batcher_.joinable()) batcher_.join();
    for (std::thread& t : feeders_) t.join();
    if (stream_) svdss_bam_stream_free(stream_);
  }
  DeviceBamSelect(const DeviceBamSelect&) = delete;
  DeviceBamSelect& operator=(const DeviceBamSelect&) = delete;

  // the next batch in file order; nullptr at the end of the file or on an error (error() says which)
  std::unique_ptr<Out> next() {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return done_.count(want_) || err_.failed() || (fed() && deferred_ == 0 && done_.empty()); });
    if (err_.failed()) return nullptr;
    auto it = done_.find(want_);
    if (it == done_.end()) return nullptr;
    std::unique_ptr<Out> b = std::move(it->second);
    done_.erase(it);
    ++want_;
    lk.unlock();
    cv_.notify_all();
    return b;
  }
  // the result of batch `seq`, whose collect returned nullptr
  void deliver(uint64_t seq, std::unique_ptr<Out> out) {
    { std::lock_guard<std::mutex> lk(m_); done_[seq] = std::move(out); --deferred_; }
    cv_.notify_all();
  }
  std::string error() const { return failure().text(); }
  BamRunError failure() const { std::lock_guard<std::mutex> lk(m_); return err_; }
  // the caller reads this region now: its feeders are held to the pending bound from here on
  void make_current() {
    { std::lock_guard<std::mutex> lk(m_); current_ = true; }
    cv_.notify_all();
  }
  // blocks until batch 0 has had its turn (svdss_bam_stream_head is final), the file has ended or the run has failed
  // (first_run_: batch 0 has been through `run`, though its result may be one that is delivered later)
  void wait_first() {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return want_ > 0 || done_.count(0) || first_run_ || err_.failed() || fed(); });
  }
  // blocks until every feeding thread has ended (the stream's tail is final; results still to be delivered may follow)
  void wait_finished() {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return fed(); });
  }
  svdss_bam_stream_t* stream() const { return stream_; }
  // seconds the batcher waited for the file's loaders / for a feeding thread to take a batch
  double waited_for_file() const { std::lock_guard<std::mutex> lk(m_); return wait_file_s_; }
  double waited_for_feeders() const { std::lock_guard<std::mutex> lk(m_); return wait_feed_s_; }
  int64_t segments_walked_again(int64_t* n_segments) const { return stream_ ? svdss_bam_stream_rewalked(stream_, n_segments) : 0; }

 private:
  struct Job { uint64_t seq = 0; bool last = false; bool restart = false; int64_t skip = 0; std::vector<std::unique_ptr<CompChunk>> chunks; };
  bool fed() const { return feeders_done_ == n_feeders_; }
  void fail(const BamRunError& e) {
    { std::lock_guard<std::mutex> lk(m_); if (!err_.failed()) err_ = e; }
    cv_.notify_all();
  }
  void batch_loop() {
    std::unique_ptr<Job> cur(new Job);
    int64_t acc = 0;
    int64_t target = small_start_ ? std::max<int64_t>(1, target_ / 4) : target_;   // (of the batch in hand: doubles to target_)
    uint64_t seq = 0;
    bool any_last = false;
    double w_file = 0;
    auto push = [&](std::unique_ptr<Job> j) {
      const auto w0 = std::chrono::steady_clock::now();
      std::unique_lock<std::mutex> lk(m_);
      cv_.wait(lk, [&] { return jobs_.size() < 2 || stop_ || err_.failed(); });
      wait_feed_s_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
      wait_file_s_ += w_file;
      w_file = 0;
      if (stop_ || err_.failed()) return false;
      jobs_.push_back(std::move(j));
      lk.unlock();
      cv_.notify_all();
      return true;
    };
    for (;;) {
      const auto w0 = std::chrono::steady_clock::now();
      std::unique_ptr<CompChunk> c = sc_->next();
      w_file += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
      if (!c) break;
      if (bam_regions_in_force()) {   // (--verbose: the BGZF members read, header and footer of 26 bytes each included)
        int64_t cb = 0;
        for (const svdss_bgzf_block_t& k : c->blocks) cb += (int64_t)k.clen + 26;
        bam_region_counters().comp_bytes.fetch_add(cb, std::memory_order_relaxed);
      }
      // a range of its own begins with this slab: the batch in hand ends here, the next one starts the chain again
      if (c->range_start && !cur->chunks.empty()) {
        cur->seq = seq++;
        if (!push(std::move(cur))) return;
        cur.reset(new Job);
        acc = 0;
      }
      if (c->range_start) { cur->restart = true; cur->skip = c->skip; }
      acc += c->inflated;
      const bool last = c->last;
      cur->chunks.push_back(std::move(c));
      if (acc >= target || last) {
        cur->seq = seq++;
        cur->last = last;
        any_last = any_last || last;
        if (!push(std::move(cur))) return;
        cur.reset(new Job);
        acc = 0;
        target = std::min(target_, target * 2);
      }
    }
    if (!sc_->error().empty()) { fail(BamRunError{SVDSS_EIO, sc_->error(), ""}); return; }
    if (!any_last) { cur->seq = seq++; cur->last = true; if (!push(std::move(cur))) return; }   // (an empty region)
    { std::lock_guard<std::mutex> lk(m_); jobs_closed_ = true; wait_file_s_ += w_file; }
    cv_.notify_all();
  }
  void feed_loop(size_t d) {
    svdss_bam_batch_t* batch = nullptr;
    std::vector<const uint8_t*> comp;
    std::vector<int64_t> comp_bytes, n_blocks;
    std::vector<const svdss_bgzf_block_t*> blocks;
    std::vector<const uint32_t*> crcs;
    for (;;) {
      std::unique_ptr<Job> job;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return !jobs_.empty() || jobs_closed_ || stop_ || err_.failed(); });
        if (stop_ || err_.failed() || jobs_.empty()) break;
        job = std::move(jobs_.front());
        jobs_.erase(jobs_.begin());
      }
      cv_.notify_all();
      comp.clear(); comp_bytes.clear(); n_blocks.clear(); blocks.clear(); crcs.clear();
      for (const std::unique_ptr<CompChunk>& c : job->chunks) {
        comp.push_back(c->data); comp_bytes.push_back((int64_t)c->n_bytes); n_blocks.push_back((int64_t)c->blocks.size());
        blocks.push_back(c->blocks.data()); crcs.push_back(c->crc.data());
      }
      const int64_t skip = job->restart && job->seq > 0 ? (job->skip | SVDSS_BAM_SKIP_RESTART) : job->seq == 0 ? skip_ : 0;
      const int rc = run_(stream_, (int64_t)job->seq, job->last ? 1 : 0, skip, d, (int32_t)comp.size(), comp.data(), comp_bytes.data(),
                          blocks.data(), crcs.data(), n_blocks.data(), &batch);
      for (std::unique_ptr<CompChunk>& c : job->chunks) sc_->recycle(std::move(c));
      if (rc != SVDSS_OK) {
        std::string msg = batch ? svdss_bam_batch_error(batch) : "";
        if (msg.empty()) msg = svdss_bam_stream_error(stream_);
        fail(BamRunError{rc, msg, svdss_last_hip_error()});
        break;
      }
      std::unique_ptr<Out> out = collect_(batch, job->seq);
      {
        std::unique_lock<std::mutex> lk(m_);
        const uint64_t sq = job->seq;
        if (sq == 0) first_run_ = true;
        if (!out) ++deferred_;
        else {
          cv_.wait(lk, [&] { return stop_ || !current_ || done_.size() < max_pending_ || done_.begin()->first > sq; });
          done_[sq] = std::move(out);
        }
      }
      cv_.notify_all();
    }
    if (batch) svdss_bam_batch_free(batch);
    bool all = false;
    { std::lock_guard<std::mutex> lk(m_); ++feeders_done_; all = fed(); }
    if (all && on_fed_) on_fed_();      // (before the waiters of wait_finished hear of it)
    cv_.notify_all();
  }

  int64_t skip_ = 0, target_ = 0;
  double wait_file_s_ = 0, wait_feed_s_ = 0;
  BamRunFn run_;
  CollectFn collect_;
  std::unique_ptr<BgzfScanner> own_sc_;
  BgzfScanner* sc_ = nullptr;
  svdss_bam_stream_t* stream_ = nullptr;
  size_t max_pending_ = 64;
  bool current_ = true, first_run_ = false;
  std::function<void()> on_fed_;
  bool small_start_ = false;
  std::thread batcher_;
  std::vector<std::thread> feeders_;
  mutable std::mutex m_;
  std::condition_variable cv_;
  std::vector<std::unique_ptr<Job>> jobs_;
  bool jobs_closed_ = false, stop_ = false;
  size_t feeders_done_ = 0, n_feeders_ = 0;
  int64_t deferred_ = 0;        // results collect left for deliver() (below 0 for a moment when one comes first)
  std::map<uint64_t, std::unique_ptr<Out>> done_;
  uint64_t want_ = 0;
  BamRunError err_;
};


// where `n` regions of a file begin (member starts; [0] = 0, back() = file size): fewer than n for a small file
// (SVDSS_REGION_MIN_KB, default 64 MB per region; SVDSS_REGION_SHARDS=0: one region)
inline std::vector<size_t> plan_bam_regions(const std::string& path, int n, int64_t header_inflated) {
  struct stat st;
  std::vector<size_t> cuts{0};
  if (stat(path.c_str(), &st) != 0 || st.st_size <= 0) return {0, 0};
  const size_t fsize = (size_t)st.st_size;
  // (--region with an index: the ranges the index names are read as one stream, on one GPU)
  if (bam_region_plan().active && bam_region_plan().path == path) return {0, fsize};
  const size_t min_bytes = getenv("SVDSS_REGION_MIN_KB") && atoll(getenv("SVDSS_REGION_MIN_KB")) > 0 ? (size_t)atoll(getenv("SVDSS_REGION_MIN_KB")) << 10
                                                                                                         : (size_t)64 << 20;
  // (the first region holds the whole BAM header)
  const size_t first_min = (size_t)header_inflated + ((size_t)header_inflated >> 6) + ((size_t)128 << 10);
  if (getenv("SVDSS_REGION_SHARDS") && atoi(getenv("SVDSS_REGION_SHARDS")) == 0) n = 1;
  n = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, fsize / min_bytes));
  for (int g = 1; g < n; ++g) {
    const size_t approx = std::max(first_min, (size_t)((unsigned __int128)fsize * (unsigned)g / (unsigned)n));
    if (approx >= fsize) break;
    const size_t c = BgzfScanner::member_start_near(path, approx);
    if (c > cuts.back() && c < fsize) cuts.push_back(c);
  }
  cuts.push_back(fsize);
  return cuts;
}

// `SVDSS search / call / smooth --gpus N` (the BAM's regions partition across the GPUs): the file is cut at
// BGZF members into one region per GPU, and every region has its own DeviceBamSelect -- scanner (loader threads), batcher,
// feeding threads, record stream -- and whatever its caller's hooks give it (a filter and a record store, an index
// replica): nothing is shared on the way in.  A region that does not begin the file begins inside a record: its chain
// starts at a guess (svdss_bam_stream_region) that is PROVED when the region in front has been handed out -- its leftover +
// the bytes this region set aside must be a chain of whole records (the seam: a batch of its own through the same entry
// point); if they are not, or the region failed in any way, it runs again from the known carry.  The caller sees the
// batches of the file in file order, as from one DeviceBamSelect; the region it reads holds `pending` results at most.
template <class Out>
class ShardedBamSelect {
 public:
  typedef typename DeviceBamSelect<Out>::CollectFn CollectFn;
  struct Shard { svdss_bam_filter_t* filter = nullptr; svdss_bam_store_t* store = nullptr; svdss_bam_store_t* seam_store = nullptr; };
  // What a region's batches go through (`SVDSS call`: the select / store entry point of the constructor below).
  // run(g, seam) / collect(g, seam): for the feeding threads of region g, or (seam = true) for the one batch of the seam in
  // front of it, run on the caller's thread with is_last = 1 (its collect may not leave the result for later); stream(g): a
  // prepared record stream for region g's run (nullptr or no hook: a plain one) -- asked again if the region runs again;
  // again(g, why): the region runs again (forget what its first run left; why: its failure, empty when the seam did not
  // fit); seam_kept(g): the seam's batch stays somewhere the caller looks for it (region_has_seam); fed(g): a run of region
  // g has run its last batch (called by its last feeding thread as it ends; once per run of the region); abandon(g): the
  // first run of region g has failed and its feeding threads have ended -- whoever delivers results of that run
  // (deliver) stops doing so before this returns: the run's reader is dropped next, then again(g) is called
  struct Hooks {
    std::function<BamRunFn(size_t g, bool seam)> run;
    std::function<CollectFn(size_t g, bool seam)> collect;
    std::function<svdss_bam_stream_t*(size_t g)> stream;
    std::function<void(size_t g, const std::string& why)> again;
    std::function<bool(size_t g)> seam_kept;
    std::function<void(size_t g)> fed;
    std::function<void(size_t g)> abandon;
  };
  // ix_shift / ix_depth (both constructors): every region's stream, and every seam's, has its input index switched on
  // (svdss_bam_stream_set_input_index); the results then carry their fragments (SelectedBatch::in_ix), seam_voffsets says
  // where a seam's record is in the file
  ShardedBamSelect(const std::string& path, const std::vector<Shard>& shards, int32_t n_ref, int64_t skip, int feeders, int64_t batch_bytes,
                   const std::vector<size_t>& cuts, int ix_shift = 0, int ix_depth = 0)
      : path_(path), n_ref_(n_ref), skip_(skip), feeders_(feeders), batch_bytes_(batch_bytes), ix_shift_(ix_shift), ix_depth_(ix_depth) {
    hooks_.run = [shards](size_t g, bool seam) {
      const Shard S = shards[g % shards.size()];
      svdss_bam_store_t* store = seam ? S.seam_store : S.store;
      return BamRunFn([S, store, seam](svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, size_t, int32_t n_chunks, const uint8_t* const* comp,
                                       const int64_t* comp_bytes, const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                       svdss_bam_batch_t** batch) {
        if (seam && store) svdss_bam_store_reset(store);
        return svdss_bam_select_store_run(s, seq, is_last, skip, S.filter, store, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, batch);
      });
    };
    hooks_.collect = [](size_t g, bool seam) {
      return CollectFn([g, seam](const svdss_bam_batch_t* batch, uint64_t) {
        std::unique_ptr<Out> out(new Out);
        svdss_bam_selection_t r;
        (void)svdss_bam_batch_selection(batch, &r);
        out->in_ix.take(batch, g, seam);
        out->n_records = (uint64_t)r.n_records;
        out->slim = r.slim != 0;
        out->off.assign(r.rec_off, r.rec_off + r.n_selected + 1);
        out->bytes.assign(r.bytes, r.bytes + r.n_bytes);
        for (int k = 0; k < 8; ++k) out->stage_s[k] = r.stage_ms[k] * 1e-3;
        out->inflate_kernel_s = r.inflate_kernel_ms * 1e-3;
        return out;
      });
    };
    hooks_.again = [shards](size_t g, const std::string&) { if (shards[g % shards.size()].store) svdss_bam_store_reset(shards[g % shards.size()].store); };
    hooks_.seam_kept = [shards](size_t g) { return shards[g % shards.size()].seam_store != nullptr; };
    start(cuts, std::vector<BgzfScanner*>());
  }
  // scanners: those of the regions' first runs, opened by the caller and kept open past this object (none given: each
  // region opens its own)
  ShardedBamSelect(const std::string& path, const Hooks& hooks, int32_t n_ref, int64_t skip, int feeders, int64_t batch_bytes, const std::vector<size_t>& cuts,
                   size_t pending = 64, const std::vector<BgzfScanner*>& scanners = std::vector<BgzfScanner*>(), bool small_start = false,
                   int ix_shift = 0, int ix_depth = 0)
      : path_(path), hooks_(hooks), n_ref_(n_ref), skip_(skip), feeders_(feeders), batch_bytes_(batch_bytes), pending_(pending), small_start_(small_start),
        ix_shift_(ix_shift), ix_depth_(ix_depth) {
    start(cuts, scanners);
  }
  size_t n_regions() const { return regions_.size(); }
  int64_t seams_run() const { return n_seams_; }
  int64_t regions_run_again() const { return n_reruns_; }
  // the store keys of the file's batches in file order: (shard, seam?) per region: the seam's store holds key 0
  bool region_has_seam(size_t g) const { return regions_[g].seam_stored; }
  int64_t region_batches(size_t g) const { return regions_[g].n_batches; }
  // (input index) the record the seam in front of region g completes: it begins where the carry of the region in front
  // begins and ends at the first record start of region g -- both as virtual offsets of the FILE
  void seam_voffsets(size_t g, uint64_t& v_beg, uint64_t& v_end) const { v_beg = regions_[g].seam_vb; v_end = regions_[g].seam_ve; }
  size_t region_begin(size_t g) const { return regions_[g].begin; }

  std::unique_ptr<Out> next() {
    for (;;) {
      if (cur_ >= regions_.size()) return nullptr;
      Reg& R = regions_[cur_];
      if (!R.entered) {
        R.entered = true;
        if (cur_ > 0 && !enter(cur_)) return nullptr;
        R.sel->make_current();
        if (R.seam) return std::move(R.seam);
      }
      std::unique_ptr<Out> b = R.sel->next();
      if (b) { ++R.n_batches; return b; }
      if (R.sel->failure().failed()) { err_ = R.sel->failure(); return nullptr; }
      ++cur_;
    }
  }
  // the result of batch `seq` of region g's run, whose collect returned nullptr (any thread; not for a run that abandon(g)
  // has been called for)
  void deliver(size_t g, uint64_t seq, std::unique_ptr<Out> out) {
    std::unique_lock<std::mutex> lk(sel_m_);
    sel_cv_.wait(lk, [&] { return regions_[g].sel != nullptr; });     // (a feeding thread of a run may be through before launch() has returned)
    regions_[g].sel->deliver(seq, std::move(out));
  }
  std::string error() const { return err_.text(); }
  const BamRunError& failure() const { return err_; }
  // summed over every run of every region (valid once the regions have been read)
  double waited_for_file() const { double s = wait_file_s_; for (const Reg& R : regions_) if (R.sel) s += R.sel->waited_for_file(); return s; }
  double waited_for_feeders() const { double s = wait_feed_s_; for (const Reg& R : regions_) if (R.sel) s += R.sel->waited_for_feeders(); return s; }
  int64_t segments_walked_again(int64_t* n_segments) const {
    int64_t seg = n_seg_, rew = n_rewalk_;
    for (const Reg& R : regions_)
      if (R.sel) { int64_t n = 0; rew += R.sel->segments_walked_again(&n); seg += n; }
    if (n_segments) *n_segments = seg;
    return rew;
  }

 private:
  struct Reg {
    size_t begin = 0, end = 0;
    std::unique_ptr<DeviceBamSelect<Out>> sel;
    std::unique_ptr<Out> seam;
    bool entered = false, seam_stored = false;
    int64_t n_batches = 0;
    uint64_t seam_vb = 0, seam_ve = 0;
  };
  void start(const std::vector<size_t>& cuts, const std::vector<BgzfScanner*>& scanners) {
    const size_t n = cuts.size() - 1;
    regions_.resize(n);
    for (size_t g = 0; g < n; ++g) {
      regions_[g].begin = cuts[g]; regions_[g].end = g + 1 < n ? cuts[g + 1] : 0;
      launch(g, g > 0, std::vector<uint8_t>(), g < scanners.size() ? scanners[g] : nullptr);
    }
  }
  void launch(size_t g, bool open_start, const std::vector<uint8_t>& carry, BgzfScanner* scanner = nullptr, bool has_carry_v = false, int64_t carry_v = 0) {
    typename DeviceBamSelect<Out>::Region rg;
    rg.ix_shift = ix_shift_; rg.ix_depth = ix_depth_; rg.has_carry_v = has_carry_v; rg.carry_v = carry_v;
    rg.begin = regions_[g].begin; rg.end = regions_[g].end;
    rg.open_start = open_start; rg.open_end = g + 1 < regions_.size();
    rg.carry = carry;
    rg.loaders = regions_.size() > 1 ? std::max(2, 8 / (int)std::min<size_t>(regions_.size(), 4)) : 8;
    rg.pending = pending_;
    rg.current = g == cur_;
    if (hooks_.fed) rg.on_fed = [this, g] { hooks_.fed(g); };
    rg.small_start = small_start_;
    std::unique_ptr<DeviceBamSelect<Out>> sel(new DeviceBamSelect<Out>(path_, 1, n_ref_, g == 0 ? skip_ : 0, feeders_, batch_bytes_, hooks_.run(g, false),
                                                                         hooks_.collect(g, false), hooks_.stream ? hooks_.stream(g) : nullptr, rg, scanner));
    { std::lock_guard<std::mutex> lk(sel_m_); regions_[g].sel = std::move(sel); }
    sel_cv_.notify_all();
  }
  // a region's run is over (its feeding threads have ended): what it counted goes into the sums
  void drop(Reg& R) {
    int64_t n = 0;
    n_rewalk_ += R.sel->segments_walked_again(&n);
    n_seg_ += n;
    wait_file_s_ += R.sel->waited_for_file();
    wait_feed_s_ += R.sel->waited_for_feeders();
    std::unique_ptr<DeviceBamSelect<Out>> gone;
    { std::lock_guard<std::mutex> lk(sel_m_); gone = std::move(R.sel); }
  }
  // the seam in front of region g, proved; false = the run has failed (err_)
  bool enter(size_t g) {
    Reg& P = regions_[g - 1];
    Reg& R = regions_[g];
    P.sel->wait_finished();
    const uint8_t *tail = nullptr, *head = nullptr;
    const int64_t n_tail = svdss_bam_stream_tail(P.sel->stream(), &tail);
    const std::vector<uint8_t> carry(tail, tail + (n_tail > 0 ? n_tail : 0));
    // (input index) where that carry begins: relative to the member right behind region g - 1, which is region g's first
    int32_t has_carry = 0;
    int64_t carry_v = 0, head_v = 0, unused = 0;
    if (ix_shift_ > 0) (void)svdss_bam_stream_input_seam(P.sel->stream(), &has_carry, &carry_v, &unused);
    R.sel->wait_first();
    const BamRunError why = R.sel->failure();
    bool good = !why.failed();
    if (good) {
      const int64_t n_head = svdss_bam_stream_head(R.sel->stream(), &head);
      if (ix_shift_ > 0) {
        int32_t hc = 0;
        (void)svdss_bam_stream_input_seam(R.sel->stream(), &hc, &unused, &head_v);
        R.seam_vb = ((uint64_t)R.begin << 16) + (uint64_t)carry_v;
        R.seam_ve = ((uint64_t)R.begin << 16) + (uint64_t)head_v;
      }
      if ((int64_t)carry.size() + n_head > 0) { good = run_seam(g, carry, head, n_head); ++n_seams_; }
    }
    if (!good) {
      if (err_.failed()) return false;
      // not proved (or the region failed): once more, from the record the region in front ended in
      R.sel->wait_finished();
      if (hooks_.abandon) hooks_.abandon(g);
      drop(R);
      R.seam.reset();
      if (hooks_.again) hooks_.again(g, why.text());
      ++n_reruns_;
      launch(g, false, carry, nullptr, ix_shift_ > 0 && has_carry != 0, carry_v);
    }
    drop(P);       // (its stream's tail has been copied)
    return true;
  }
  // the seam's bytes as a stream of their own: stored deflate blocks through the region's entry point.  false: not a
  // chain of whole records (the guess was wrong), or the run has failed (err_)
  bool run_seam(size_t g, const std::vector<uint8_t>& tail, const uint8_t* head, int64_t n_head) {
    std::vector<uint8_t> bytes(tail);
    if (n_head > 0) bytes.insert(bytes.end(), head, head + n_head);
    std::vector<uint8_t> comp;
    std::vector<svdss_bgzf_block_t> blk;
    std::vector<uint32_t> crc;
    for (size_t off = 0; off < bytes.size(); off += 0xff00) {
      const size_t len = std::min<size_t>(0xff00, bytes.size() - off);
      while (comp.size() & 15) comp.push_back(0);
      svdss_bgzf_block_t b;
      b.coff = (int64_t)comp.size(); b.clen = (int32_t)(5 + len); b.isize = (int32_t)len; b.uoff = 0;
      comp.push_back(1);   // BFINAL, stored
      comp.push_back((uint8_t)(len & 0xff)); comp.push_back((uint8_t)(len >> 8));
      comp.push_back((uint8_t)(~len & 0xff)); comp.push_back((uint8_t)((~len >> 8) & 0xff));
      comp.insert(comp.end(), bytes.begin() + (long)off, bytes.begin() + (long)(off + len));
      blk.push_back(b);
      crc.push_back((uint32_t)crc32(crc32(0L, Z_NULL, 0), bytes.data() + off, (uInt)len));
    }
    comp.resize(comp.size() + 64);
    svdss_bam_stream_t* st = nullptr;
    if (svdss_bam_stream_create(n_ref_, &st) != SVDSS_OK) { err_ = BamRunError{SVDSS_ENOMEM, "out of memory", ""}; return false; }
    if (const int rc = bam_stream_apply_regions(st)) { err_ = BamRunError{rc, "the regions do not fit the BAM header", ""}; svdss_bam_stream_free(st); return false; }
    if (ix_shift_ > 0) (void)svdss_bam_stream_set_input_index(st, ix_shift_, ix_depth_);
    svdss_bam_batch_t* batch = nullptr;
    const uint8_t* cp = comp.data();
    const int64_t cb = (int64_t)comp.size(), nb = (int64_t)blk.size();
    const svdss_bgzf_block_t* bp = blk.data();
    const uint32_t* rp = crc.data();
    const int rc = hooks_.run(g, true)(st, 0, 1, 0, 0, 1, &cp, &cb, &bp, &rp, &nb, &batch);
    bool ok = rc == SVDSS_OK;
    if (ok && ix_shift_ > 0) {
      // (input index) a seam's offsets are derived for the ONE record it completes (seam_voffsets): a guess that left several
      // records in front of it counts as one that did not fit, and the region runs again from the known carry
      svdss_bam_input_frag_t f;
      if (svdss_bam_batch_input_index(batch, &f) != SVDSS_OK || f.n_records != 1) ok = false;
    }
    if (ok) {
      regions_[g].seam = hooks_.collect(g, true)(batch, 0);
      regions_[g].seam_stored = hooks_.seam_kept && hooks_.seam_kept(g);
    } else if (rc != SVDSS_OK && rc != SVDSS_EIO) {
      err_ = BamRunError{rc, std::string("seam: ") + svdss_strerror(rc) + " " + (batch ? svdss_bam_batch_error(batch) : "") + " " + svdss_last_hip_error(),
                         svdss_last_hip_error()};
    }
    if (batch) svdss_bam_batch_free(batch);
    svdss_bam_stream_free(st);
    return ok;
  }

  std::string path_;
  Hooks hooks_;
  int32_t n_ref_ = 0;
  int64_t skip_ = 0;
  int feeders_ = 3;
  int64_t batch_bytes_ = 0;
  size_t pending_ = 64;
  bool small_start_ = false;         // (every run of every region: BamSelectRegion::small_start)
  int ix_shift_ = 0, ix_depth_ = 0;  // the input index of every stream (0: off)
  std::vector<Reg> regions_;
  std::mutex sel_m_;                 // (who may come from another thread -- deliver -- meets a region's `sel` under it)
  std::condition_variable sel_cv_;
  size_t cur_ = 0;
  int64_t n_seams_ = 0, n_reruns_ = 0, n_seg_ = 0, n_rewalk_ = 0;
  double wait_file_s_ = 0, wait_feed_s_ = 0;
  BamRunError err_;
};
