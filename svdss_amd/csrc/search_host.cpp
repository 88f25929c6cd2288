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
#include "fastx_device.h"
#include "gzip_stream.h"
#include "sfs_units.h"

namespace {

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
//
// Early (the front end beside the index restore): an EarlySearch per region -- `early` is empty, or has one for every region
// of the file --, each with a park on its region's GPU and a drain thread that searches its parked groups on that GPU's
// replica.  A region is released when ITS replica is resident; no region waits for another's front end or index.
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
class DevicePath {
 public:
  DevicePath(const Options& o, const SearchKnobs& knobs, const std::vector<svdss_index_t*>& replicas, const DeviceBamInput& in,
             const Stopwatch& clock, const std::vector<EarlySearch*>& early = std::vector<EarlySearch*>())
      : o_(o), knobs_(knobs), replicas_(replicas), in_(in), clock_(clock), early_(early),
        flags_((o.assemble ? SVDSS_SFS_ASSEMBLE : 0) | (o.putative ? SVDSS_BAM_PUTATIVE : 0)) {}
  void run();
 private:
  BamRunFn run_on(size_t r, bool seam = false);
  std::unique_ptr<DevOut> collect(size_t r, const svdss_bam_batch_t* batch, uint64_t seq);
  std::unique_ptr<DevOut> next() { return one_ ? one_->next() : sharded_->next(); }
  void assemble();
  void drain_park(size_t r);
  void run_again(size_t r);
  void report();

  const Options& o_;
  const SearchKnobs& knobs_;
  const std::vector<svdss_index_t*> replicas_;
  const DeviceBamInput& in_;
  const Stopwatch& clock_;
  const std::vector<EarlySearch*> early_;
  std::vector<std::thread> drains_;       // early: one per region (a region that runs again: joined and started anew by the assembler)
  const int32_t flags_;
  StageSeconds t_;
  // units of whole reference batches, formatted by a few threads, written in order
  UnitAssembler units_{o_, t_};
  // the file's batches in file order: one region (every replica's feeders take its batches) or one region per replica
  std::unique_ptr<DeviceBamSelect<DevOut>> one_;
  std::unique_ptr<ShardedBamSelect<DevOut>> sharded_;
  std::unique_ptr<OrderedWriter> writer_;
};
// a batch of region r through the device on replica (r + dev): the whole of it -- or, early, while the region's index is not
// released, its front half, the reads parked.  seam: the one small batch in front of a region, on the assembler's thread:
// a whole batch, when the region's replica is there.
BamRunFn DevicePath::run_on(size_t r, bool seam) {
  return BamRunFn([this, r, seam](svdss_bam_stream_t* st, int64_t seq, int32_t last, int64_t sk, size_t dev, int32_t nc, const uint8_t* const* comp, const int64_t* cb,
                                  const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* nb, svdss_bam_batch_t** batch) {
    const auto t0 = now();
    EarlySearch* const es = early_.empty() ? nullptr : early_[r];
    svdss_index_t* ix = !es ? replicas_[(r + dev) % replicas_.size()] : seam ? es->wait_for_released_index() : es->index_for_feeders();
    int rc = ix ? svdss_bam_batch_run(st, seq, last, sk, ix, nc, comp, cb, blocks, crc, nb, flags_, batch)
                : svdss_bam_batch_front(st, seq, last, sk, es->device, es->park, nc, comp, cb, blocks, crc, nb, flags_, batch);
    if (rc == SVDSS_OK && !ix) {
      int64_t grp = -1;
      check(svdss_bam_batch_parked(*batch, &grp, nullptr, nullptr), "svdss_bam_batch_parked");
      svdss_bam_result_t r0;
      check(svdss_bam_batch_result(*batch, &r0), "svdss_bam_batch_result");
      int64_t job_comp = 0;
      for (int32_t k = 0; k < nc; ++k) job_comp += cb[k];
      es->note_batch(r0.n_records, r0.n_searched, job_comp);
      if (grp == -1) rc = svdss_bam_batch_search(*batch, es->wait_for_index());   // no room in the park
      // (grp == -2: nothing to search in this batch, its results are complete)
    }
    std::lock_guard<std::mutex> lk(t_.m);
    t_.gpu += secs(t0, now());
    return rc;
  });
}
// what a batch object holds after its run -> reads with their SFS.  A batch whose reads went into the park has names and
// tags only: it waits in its region's EarlySearch, and drain_park delivers it when its group has been searched.
std::unique_ptr<DevOut> DevicePath::collect(size_t region, const svdss_bam_batch_t* batch, uint64_t seq) {
  const auto t1 = now();
  EarlySearch* const es = early_.empty() ? nullptr : early_[region];
  int64_t grp = -1, first = 0, n_srch = 0;
  const bool parked = es && svdss_bam_batch_parked(batch, &grp, &first, &n_srch) == SVDSS_OK && grp >= 0;
  svdss_bam_result_t r;
  check(svdss_bam_batch_result(batch, &r), "svdss_bam_batch_result");
  std::unique_ptr<DevOut> out = unpack_result(r, parked);
  {
    std::lock_guard<std::mutex> lk(t_.m);
    t_.unpack += secs(t1, now()); t_.inflate_ms += r.inflate_kernel_ms;
    t_.n_seen += (uint64_t)r.n_records; ++t_.n_batches;
    for (int k = 0; k < 8; ++k) t_.device[k] += r.stage_ms[k] * 1e-3;
  }
  if (!parked) return out;
  es->add_pending(grp, EarlySearch::Pending{seq, std::move(out), first, n_srch});
  return nullptr;
}
void DevicePath::assemble() {
  units_.begin();
  while (std::unique_ptr<DevOut> d = next()) units_.deal(*d);
  const BamRunError e = one_ ? one_->failure() : sharded_->failure();
  if (e.failed()) {
    if (e.msg.find("core.tid") != std::string::npos) die(e.msg);                       // ping_pong.cpp:76-79
    if (e.rc == SVDSS_EIO) die("error reading " + o_.bam + ": " + e.msg);
    die(std::string("svdss_bam_batch_run: ") + svdss_strerror(e.rc) + " " + e.msg + " " + e.hip);
  }
  units_.end();
}
// early, region r: once its index is resident, its parked groups -- ONE launch each, one lane per read -- and their batches'
// results.  A region whose run has failed is abandoned: the thread returns at its next look and delivers nothing more.
void DevicePath::drain_park(size_t r) {
  EarlySearch* const es = early_[r];
  svdss_index_t* ix = es->wait_for_offered_index();
  svdss_sfs_batch_t* sfs = nullptr;
  std::vector<int64_t> counts, prefix;
  std::vector<int32_t> qs, ln;
  int64_t n_parked = 0, n_parked_batches = 0, n_groups = 0, n_early_groups = 0;
  double t_search = 0;
  bool closed = false, abandoned = es->abandoned();
  for (int64_t g = 0; !abandoned; ++g) {
    // the next group: one that has closed while the index is held back from the feeders, or -- once the feeders have the
    // index and the park is closed -- whatever is left
    for (;;) {
      if ((abandoned = es->abandoned())) break;
      if (!closed && es->released()) {
        check(svdss_bam_park_close(es->park), "svdss_bam_park_close");
        closed = true;
        n_groups = svdss_bam_park_groups(es->park);
      }
      if (closed || svdss_bam_park_group_ready(es->park, g)) break;
      es->nap();
    }
    if (abandoned || (closed && g >= n_groups)) break;
    if (!closed) ++n_early_groups;
    int64_t nb = 0, nr = 0, ns = 0;
    check(svdss_bam_park_group(es->park, g, &nb, &nr, &ns), "svdss_bam_park_group");
    // (every batch of the group has handed in its names and tags -- or the region's run has failed meanwhile)
    std::vector<EarlySearch::Pending> pending = es->take_group(g, nb);
    if ((abandoned = es->abandoned())) break;
    const auto t0 = now();
    check(svdss_bam_park_search(es->park, g, ix, flags_, &sfs), "svdss_bam_park_search");
    const int64_t total = svdss_sfs_batch_total(sfs);
    counts.resize((size_t)nr); qs.resize((size_t)total); ln.resize((size_t)total);
    check(svdss_sfs_batch_fetch(sfs, counts.data(), qs.data(), ln.data(), nullptr), "svdss_sfs_batch_fetch");
    t_search += secs(t0, now());
    prefix.assign((size_t)nr + 1, 0);
    for (int64_t i = 0; i < nr; ++i) prefix[(size_t)i + 1] = prefix[(size_t)i] + counts[(size_t)i];
    for (EarlySearch::Pending& P : pending) {
      fill_parked(P, counts, prefix, qs, ln);
      if (one_) one_->deliver(P.seq, std::move(P.out)); else sharded_->deliver(r, P.seq, std::move(P.out));
    }
    n_parked += nr; n_parked_batches += nb;
  }
  if (sfs) svdss_sfs_batch_free(sfs);
  { std::lock_guard<std::mutex> lk(t_.m); t_.device[5] += t_search; }
  if (o_.verbose && !abandoned)
    logmsg("debug", (sharded_ ? "region " + std::to_string(r) + ": " : std::string()) + "front end beside the index restore: " + std::to_string(n_parked_batches) +
                        " batches (" + std::to_string(es->records.load()) + " records) had been read when the index was resident; their " + std::to_string(n_parked) +
                        " reads searched in " + std::to_string(n_groups) + " launch(es), " + std::to_string(t_search) + " s" +
                        (n_early_groups ? " (" + std::to_string(n_early_groups) + " of them while the file was still being read)" : "") + ", done at +" + clock_.since() + " s");
}
// early: region r runs again (its first run's feeding threads have ended, its drain thread has been told: abandon).  What
// the failed run parked and left pending is discarded -- a fresh park, nothing pending, nothing counted -- and a new drain
// thread waits for the second run's groups.
void DevicePath::run_again(size_t r) {
  EarlySearch* const es = early_[r];
  svdss_bam_park_free(es->park);
  es->park = nullptr;
  check(svdss_bam_park_create(es->device, es->park_bytes, es->park_bytes / 512 + 4096, &es->park), "svdss_bam_park_create");
  es->reset_for_rerun();
  drains_[r] = std::thread([this, r] { drain_park(r); });
}
void DevicePath::run() {
  const size_t pending = 8;       // (results of the region being dealt that may wait for the assembler)
  auto collect_fn = [this](const svdss_bam_batch_t* batch, uint64_t seq) { return collect(0, batch, seq); };
  drains_.resize(early_.size());
  if (in_.n_regions() == 1) {
    DeviceBamSelect<DevOut>::Region rg;
    rg.pending = pending;
    one_.reset(new DeviceBamSelect<DevOut>(o_.bam, replicas_.size(), in_.n_ref, in_.skip, knobs_.feeders, knobs_.batch_bytes, run_on(0), collect_fn, nullptr, rg,
                                           in_.scanner_ptrs[0]));
  } else {
    ShardedBamSelect<DevOut>::Hooks hk;
    hk.run = [this](size_t g, bool seam) { return run_on(g, seam); };
    hk.collect = [this](size_t g, bool) {
      return DeviceBamSelect<DevOut>::CollectFn([this, g](const svdss_bam_batch_t* batch, uint64_t seq) { return collect(g, batch, seq); });
    };
    if (!early_.empty()) {
      // (a region's front is finished when the last feeding thread of its run ends; a run that failed is abandoned first)
      hk.fed = [this](size_t g) { early_[g]->front_finished(); };
      hk.abandon = [this](size_t g) { early_[g]->abandon(); if (drains_[g].joinable()) drains_[g].join(); };
    }
    hk.again = [this](size_t g, const std::string& why) {
      if (o_.verbose) logmsg("debug", "region " + std::to_string(g) + " runs again from the end of region " + std::to_string(g - 1) +
                                          (why.empty() ? std::string(" (its first record was not where the chain arrives)") : " (" + why + ")"));
      if (!early_.empty()) run_again(g);
    };
    // (early: a region's first batches are small -- a quarter, then half of a batch.  Its GPU has work, its counters have
    // figures for the sum the process decides from, and its guessed head is final after a quarter of the bytes; with the
    // index first, as before, every batch is a whole one)
    sharded_.reset(new ShardedBamSelect<DevOut>(o_.bam, hk, in_.n_ref, in_.skip, knobs_.feeders, knobs_.batch_bytes, in_.cuts, pending, in_.scanner_ptrs,
                                                !early_.empty()));
    // (from here on the assembler alone touches drains_ -- the hooks above run on its thread -- until it has ended)
    for (size_t g = 0; g < early_.size(); ++g) drains_[g] = std::thread([this, g] { drain_park(g); });
  }
  std::thread assembler([this] { assemble(); });
  writer_.reset(new OrderedWriter(units_.pool()));
  // (formatting the text costs about one core-second per million reads: five threads per GPU, as many as the cores allow)
  const int n_fmt = knobs_.format_threads ? knobs_.format_threads : (int)std::max<size_t>(5, std::min<size_t>(5 * replicas_.size(), effective_cpus()));
  std::vector<std::thread> fmt;
  for (int k = 0; k < n_fmt; ++k) fmt.emplace_back([this] { units_.format_units(*writer_); });
  if (one_ && !early_.empty()) {
    drains_[0] = std::thread([this] { drain_park(0); });
    one_->wait_finished();
    early_[0]->front_finished();
    drains_[0].join();
  }
  // (regions: the assembler has dealt everything when every drain thread has delivered everything)
  assembler.join();
  if (sharded_) for (std::thread& th : drains_) if (th.joinable()) th.join();
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

// ---- `search --fastx` with the records found on the GPU (csrc/fastx_device.hip; fastx_device.h cuts the file): feeding
// threads (batch -> upload / inflate -> records -> search) -> results in file order -> assembler -> formatting threads ->
// writer, the back half of the BAM device path.  A batch the parser declines ends the device's part: the records it proved
// are dealt, then the assembler reads on with FastxReader over the text the batches hand down (the feeders still inflate
// them) and searches what it finds through the host-buffer entry point -- the same bytes as the host path for every file.
class FastxDevicePath {
 public:
  FastxDevicePath(const Options& o, const SearchKnobs& knobs, const std::vector<svdss_index_t*>& replicas, FastxKind kind, const Stopwatch& clock)
      : o_(o), knobs_(knobs), replicas_(replicas), kind_(kind), clock_(clock), flags_(o.assemble ? SVDSS_SFS_ASSEMBLE : 0) {}
  void run();
 private:
  struct Out { DevOut d; bool declined = false; std::string text; };
  void feeder(size_t replica);
  void deliver(int64_t seq, bool last, std::unique_ptr<Out> out);
  std::unique_ptr<Out> next_out();          // in file order; nullptr behind the last batch
  void assemble();
  void host_tail(std::unique_ptr<Out> first);
  void gzip_source();                       // FastxKind::Gzip: the file inflated window by window, its text put() to the batcher

  const Options& o_;
  const SearchKnobs& knobs_;
  const std::vector<svdss_index_t*>& replicas_;
  const FastxKind kind_;
  const Stopwatch& clock_;
  const int32_t flags_;
  StageSeconds t_;
  UnitAssembler units_{o_, t_};
  std::unique_ptr<FastxBatcher> batcher_;
  svdss_fastx_stream_t* stream_ = nullptr;
  std::unique_ptr<OrderedWriter> writer_;
  std::mutex m_;
  std::condition_variable cv_;
  std::map<int64_t, std::unique_ptr<Out>> done_;
  int64_t want_ = 0, last_seq_ = -1;
  int64_t n_device_ = 0, n_host_ = 0, n_records_ = 0;   // (the assembler's)
  double parse_ms_ = 0, text_bytes_ = 0;                // (under t_.m)
  std::string gzip_line_;                               // (the source thread's, read after it is joined)
};
// `search --fastx reads.fastq.gz`, plain gzip: the source thread reads the file in windows of compressed bytes, has each
// inflated on GPU 0 (svdss_gzip_stream_run) and hands the text to the batcher, whose batches the feeders take as plain text.
// Where the unit declines, zlib reads on from the carried state (GzHostTail) and the batches go on unchanged.
void FastxDevicePath::gzip_source() {
  const std::string& path = o_.fastx;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) die("cannot open " + path);
  svdss_gzip_stream_t* gz = nullptr;
  check(svdss_gzip_stream_create(0, knobs_.gzip_chunk_bytes, &gz), "svdss_gzip_stream_create");
  const size_t depth = replicas_.size() * (size_t)knobs_.feeders + 2;
  std::vector<uint8_t> buf((size_t)knobs_.gzip_window_bytes);
  size_t have = 0;
  bool eof = false;
  svdss_gzip_result_t r;
  for (;;) {
    while (have < buf.size() && !eof) {
      const size_t k = fread(buf.data() + have, 1, buf.size() - have, f);
      if (k == 0) { if (ferror(f)) die("error reading " + path + ": short read"); eof = true; }
      have += k;
    }
    int64_t used = 0;
    const int rc = svdss_gzip_stream_run(gz, buf.data(), (int64_t)have, eof ? 1 : 0, &used);
    if (rc == SVDSS_EIO) die("error reading " + path + ": " + svdss_gzip_stream_error(gz));
    if (rc != SVDSS_OK) die(std::string("svdss_gzip_stream_run: ") + svdss_strerror(rc) + " " + svdss_last_hip_error());
    check(svdss_gzip_stream_result(gz, &r), "svdss_gzip_stream_result");
    if (r.text_bytes) batcher_->put(r.text, (size_t)r.text_bytes, depth);
    memmove(buf.data(), buf.data() + used, have - (size_t)used);
    have -= (size_t)used;
    if (r.declined || r.ended) break;
    if (used == 0 && r.text_bytes == 0) {
      if (eof) die("error reading " + path + ": truncated gzip stream");
      buf.resize(buf.size() * 2);      // (a member header longer than the window)
    }
  }
  int64_t host_bytes = 0;
  if (r.declined) {
    GzCarry c;
    c.byte_pos = r.byte_pos; c.bit = r.bit; c.in_member = r.in_member; c.want_trailer = r.want_trailer;
    c.crc = r.crc; c.count = r.count; c.dict_len = (uint32_t)r.dict_len;
    memcpy(c.dict + 32768 - c.dict_len, r.dict, c.dict_len);
    size_t at = 0;
    GzHostTail tail(c, [&](uint8_t* dst, size_t cap) -> size_t {
      if (at < have) {          // (what the last window held behind the carried position)
        const size_t n = std::min(cap, have - at);
        memcpy(dst, buf.data() + at, n);
        at += n;
        return n;
      }
      const size_t n = fread(dst, 1, cap, f);
      if (n == 0 && ferror(f)) die("error reading " + path + ": short read");
      return n;
    });
    std::vector<uint8_t> text((size_t)4 << 20);
    for (;;) {
      const int64_t n = tail.next(text.data(), text.size());
      if (n < 0) die("error reading " + path + ": " + tail.error());
      if (n == 0) break;
      host_bytes += n;
      batcher_->put(text.data(), (size_t)n, depth);
    }
  }
  batcher_->finish();
  fclose(f);
  static const char* const why[] = {"", "not a gzip header", "no dynamic block start in a window", "no whole block in a window", "an invalid code",
                                    "trailing bytes that are no gzip header"};
  char line[640];
  int n = snprintf(line, sizeof line, "fastx: gzip on the device: %lld windows, %lld chunks (%lld merged, %lld false starts), %lld bytes, "
                   "find/measure/decode/resolve %.3f/%.3f/%.3f/%.3f ms", (long long)r.windows, (long long)r.n_chunks, (long long)r.chunks_merged,
                   (long long)r.false_starts, (long long)r.device_bytes, r.find_ms, r.measure_ms, r.decode_ms, r.resolve_ms);
  if (r.declined && n > 0 && (size_t)n < sizeof line)
    snprintf(line + n, sizeof line - (size_t)n, "; the host (zlib) took over at byte %lld bit %d (%s): %lld bytes", (long long)r.byte_pos, (int)r.bit,
             why[r.declined >= 1 && r.declined <= 5 ? r.declined : 0], (long long)host_bytes);
  gzip_line_ = line;
  svdss_gzip_stream_free(gz);
}
void FastxDevicePath::feeder(size_t replica) {
  svdss_index_t* ix = replicas_[replica];
  svdss_fastx_batch_t* batch = nullptr;
  std::vector<uint8_t> slab;
  FILE* f = kind_ == FastxKind::Plain ? fopen(o_.fastx.c_str(), "rb") : nullptr;
  if (kind_ == FastxKind::Plain && !f) die("cannot open " + o_.fastx);
  FastxJob job;
  while (batcher_->next(job)) {
    const auto t0 = now();
    if (kind_ == FastxKind::Plain) {
      slab.resize((size_t)job.plain_bytes);
      size_t got = 0;
      while (got < slab.size()) {
        const ssize_t k = pread(fileno(f), slab.data() + got, slab.size() - got, (off_t)(job.plain_off + (int64_t)got));
        if (k <= 0) die("error reading " + o_.fastx + ": short read");
        got += (size_t)k;
      }
    }
    const uint8_t* const plain = kind_ == FastxKind::Gzip ? job.text->data() : slab.data();
    const int rc = svdss_fastx_batch_run(stream_, job.seq, job.last ? 1 : 0, ix, (int32_t)job.comp.size(), job.comp.data(), job.comp_bytes.data(),
                                         job.blocks.data(), job.crc.data(), job.n_blocks.data(), plain, job.plain_bytes, flags_, &batch);
    if (rc != SVDSS_OK) {
      const std::string why = batch && *svdss_fastx_batch_error(batch) ? svdss_fastx_batch_error(batch) : svdss_fastx_stream_error(stream_);
      if (rc == SVDSS_EIO) die("error reading " + o_.fastx + ": " + why);
      die(std::string("svdss_fastx_batch_run: ") + svdss_strerror(rc) + " " + why + " " + svdss_last_hip_error());
    }
    const auto t1 = now();
    svdss_fastx_result_t r;
    check(svdss_fastx_batch_result(batch, &r), "svdss_fastx_batch_result");
    std::unique_ptr<Out> out(new Out);
    out->declined = r.declined != 0;
    if (out->declined) out->text.assign((const char*)r.text, (size_t)r.text_bytes);
    out->d.reads.resize((size_t)r.n_records);
    out->d.qs.assign(r.qs, r.qs + r.total_sfs);
    out->d.ln.assign(r.len, r.len + r.total_sfs);
    int64_t acc = 0;
    for (int64_t i = 0; i < r.n_records; ++i) {
      Read& rd = out->d.reads[(size_t)i];
      rd.name.assign(r.names + r.name_off[i], (size_t)(r.name_off[i + 1] - r.name_off[i]));
      rd.len = r.seq_len[i];
      rd.first = acc;
      rd.count = r.counts[i];
      acc += rd.count;
    }
    {
      std::lock_guard<std::mutex> lk(t_.m);
      t_.gpu += secs(t0, t1); t_.unpack += secs(t1, now()); t_.inflate_ms += r.inflate_kernel_ms; parse_ms_ += r.parse_kernel_ms;
      if (!out->declined) text_bytes_ += (double)r.n_text_bytes;
      for (int k = 0; k < 8; ++k) t_.device[k] += r.stage_ms[k] * 1e-3;
    }
    const int64_t seq = job.seq;
    const bool last = job.last;
    job.clear();     // (the slabs go back to the scanner)
    deliver(seq, last, std::move(out));
  }
  if (!batcher_->error().empty()) die("error reading " + o_.fastx + ": " + batcher_->error());
  if (f) fclose(f);
  svdss_fastx_batch_free(batch);
}
void FastxDevicePath::deliver(int64_t seq, bool last, std::unique_ptr<Out> out) {
  std::unique_lock<std::mutex> lk(m_);
  cv_.wait(lk, [&] { return done_.size() < 8 || seq == want_; });
  done_[seq] = std::move(out);
  if (last) last_seq_ = seq;
  lk.unlock();
  cv_.notify_all();
}
std::unique_ptr<FastxDevicePath::Out> FastxDevicePath::next_out() {
  std::unique_lock<std::mutex> lk(m_);
  cv_.wait(lk, [&] { return done_.count(want_) || (last_seq_ >= 0 && want_ > last_seq_); });
  auto it = done_.find(want_);
  if (it == done_.end()) return nullptr;
  std::unique_ptr<Out> out = std::move(it->second);
  done_.erase(it);
  ++want_;
  lk.unlock();
  cv_.notify_all();
  return out;
}
void FastxDevicePath::assemble() {
  units_.begin();
  while (std::unique_ptr<Out> out = next_out()) {
    n_records_ += (int64_t)out->d.reads.size();
    units_.deal(out->d);
    if (out->declined) { host_tail(std::move(out)); break; }
    ++n_device_;
  }
  units_.end();
}
// from the first unparsed byte of the batch that declined to the end of the input: FastxReader over the batches' text, the
// reads searched as HostPath searches them
void FastxDevicePath::host_tail(std::unique_ptr<Out> first) {
  FastxReader fx([&](std::string& buf) {
    std::unique_ptr<Out> out = first ? std::move(first) : next_out();
    if (!out) return false;
    ++n_host_;
    buf = std::move(out->text);
    return true;
  });
  const int64_t super = reads_per_unit(o_);
  svdss_sfs_batch_t* res = nullptr;
  std::vector<uint8_t> gbuf;
  std::vector<int64_t> goff, counts;
  std::string seq;
  for (bool more = true; more;) {
    DevOut d;
    gbuf.clear();
    goff.assign(1, 0);
    while ((int64_t)d.reads.size() < super) {
      Read r;
      if (!fx.next(r.name, seq)) { more = false; break; }
      r.len = (int64_t)seq.size();
      const size_t at = gbuf.size();
      gbuf.resize(at + seq.size());
      svdss_nt6_encode(seq.data(), (int64_t)seq.size(), gbuf.data() + at);
      goff.push_back((int64_t)gbuf.size());
      d.reads.push_back(std::move(r));
    }
    if (d.reads.empty()) break;
    check(svdss_sfs_search_batch(replicas_[0], gbuf.data(), goff.data(), (int64_t)d.reads.size(), flags_, &res), "svdss_sfs_search_batch");
    counts.assign(d.reads.size(), 0);
    d.qs.resize((size_t)svdss_sfs_batch_total(res));
    d.ln.resize(d.qs.size());
    check(svdss_sfs_batch_fetch(res, counts.data(), d.qs.data(), d.ln.data(), nullptr), "svdss_sfs_batch_fetch");
    int64_t acc = 0;
    for (size_t k = 0; k < d.reads.size(); ++k) { d.reads[k].first = acc; d.reads[k].count = counts[k]; acc += counts[k]; }
    n_records_ += (int64_t)d.reads.size();
    units_.deal(d);
  }
  svdss_sfs_batch_free(res);
}
void FastxDevicePath::run() {
  const size_t n_feeders = replicas_.size() * (size_t)knobs_.feeders;
  const size_t per_batch = (size_t)knobs_.fastx_batch_bytes / knobs_.slab_bytes + 2;
  batcher_.reset(new FastxBatcher(o_.fastx, kind_, knobs_.fastx_batch_bytes, knobs_.slab_bytes, knobs_.loaders, (size_t)knobs_.loaders + (n_feeders + 3) * per_batch));
  if (!batcher_->ok()) die("cannot open " + o_.fastx);
  // (a record is carried to the next batch whole: one longer than a batch declines)
  check(svdss_fastx_stream_create(0, knobs_.fastx_batch_bytes, &stream_), "svdss_fastx_stream_create");
  std::thread assembler([this] { assemble(); });
  writer_.reset(new OrderedWriter(units_.pool()));
  const int n_fmt = knobs_.format_threads ? knobs_.format_threads : (int)std::max<size_t>(5, std::min<size_t>(5 * replicas_.size(), effective_cpus()));
  std::vector<std::thread> fmt, feeders;
  for (int k = 0; k < n_fmt; ++k) fmt.emplace_back([this] { units_.format_units(*writer_); });
  for (size_t d = 0; d < replicas_.size(); ++d)
    for (int k = 0; k < knobs_.feeders; ++k) feeders.emplace_back([this, d] { feeder(d); });
  std::thread source;
  if (kind_ == FastxKind::Gzip) source = std::thread([this] { gzip_source(); });
  for (std::thread& th : feeders) th.join();
  if (source.joinable()) source.join();
  assembler.join();
  for (std::thread& th : fmt) th.join();
  writer_->finish();
  svdss_fastx_stream_free(stream_);
  if (!o_.verbose) return;
  logmsg("debug", std::to_string(n_records_) + " records read, " + std::to_string(writer_->lines()) + " SFS written at +" + clock_.since() + " s");
  if (!gzip_line_.empty()) logmsg("debug", gzip_line_);
  logmsg("debug", "FASTX device path: " + std::to_string(n_device_) + " batches on the device, " + std::to_string(n_host_) + " through the host reader, " +
                      std::to_string(n_records_) + " records");
  char buf[480];
  snprintf(buf, sizeof buf, "FASTX device batches, seconds summed: upload+inflate+crc %.3f (inflate kernels %.3f), waiting for the turn %.3f, turn (lines, shape, carry) %.3f, "
           "records+names+bases %.3f, search %.3f, results down %.3f; parse kernels %.3f ms over %.0f text bytes; re-dealing %.3f, format %.3f, write %.3f",
           t_.device[0], t_.inflate_ms * 1e-3, t_.device[1], t_.device[2], t_.device[3], t_.device[5], t_.device[6], parse_ms_, text_bytes_, t_.assemble, t_.format,
           writer_->busy_seconds());
  logmsg("debug", buf);
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
  void release_replicas_to_front_ends();
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
  // the early path: one EarlySearch (one GPU, one region) or one per region of the file, region g on GPU g % n_dev
  std::vector<std::unique_ptr<EarlySearch>> earlies;
  std::vector<EarlySearch*> early;     // (the same, as the decision and the device path take them; empty: the index first)
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
// The BAM front end starts NOW, beside the index restore (EarlySearch; SVDSS_SEARCH_EARLY=0: the index first, as
// PingPong::run does, ping_pong.cpp:245,329) -- on one GPU with the file as one region, and with --gpus N when the file
// has been cut into one region per GPU: every region then has its own park, on its own GPU, allocated before the restore
// begins.  Everything else stays index-first, as it was: SVDSS_REGION_SHARDS=0 or a file too small for N regions (one
// region, all GPUs' feeders), --region with a BAI (one stream on one GPU), SVDSS_BAM_DEVICE=0, --fastx, and
// SVDSS_SEARCH_EARLY=0 -- the order every test of the early path is compared with.  (`smooth`, `call` and `run` have
// their own hosts and do not come here.)
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
  const size_t n_regions = dev_bam ? in.n_regions() : 0;
  const bool shaped = n_gpus == 1 ? n_regions == 1 : n_regions == (size_t)n_gpus;
  if (!(dev_bam && early_pays && shaped && knobs.early != 0)) return;
  if (o.bsize <= 0) die("batch size smaller than the number of threads");
  for (size_t g = 0; g < n_regions; ++g) {
    earlies.emplace_back(new EarlySearch);
    early.push_back(earlies.back().get());
    EarlySearch& es = *earlies.back();
    es.device = (int32_t)(g % (size_t)n_dev);
    // (regions that share a GPU -- more --gpus than devices, SVDSS_GPUS_OVERSUBSCRIBE -- share its park bytes)
    es.park_bytes = park_bytes_of_region(knobs.park_bytes, n_regions, (size_t)n_dev, g);
    if (n_regions == 1) {
      struct stat stb;
      es.file_bytes = stat(o.bam.c_str(), &stb) == 0 ? (int64_t)stb.st_size : 0;
    } else {
      es.file_bytes = (int64_t)(in.cuts[g + 1] - in.cuts[g]);
      es.regions = &early;
    }
  }
  // (on a thread of its own from the first moment: this one goes straight to the index file)
  front_end = std::thread([this] {
    for (EarlySearch* es : early) check(svdss_bam_park_create(es->device, es->park_bytes, es->park_bytes / 512 + 4096, &es->park), "svdss_bam_park_create");
    if (prewarm.joinable()) prewarm.join();
    if (o.verbose && in.n_regions() > 1) {
      std::string m = "file regions (bytes):";
      for (size_t g = 0; g + 1 < in.cuts.size(); ++g) m += " " + std::to_string(in.cuts[g + 1] - in.cuts[g]);
      logmsg("debug", m + "; every region's front end runs beside the index restore");
    }
    // (no replica yet: each region's EarlySearch hands its feeders theirs; one slot per GPU, for what is sized per GPU)
    DevicePath(o, knobs, std::vector<svdss_index_t*>(early.size(), nullptr), in, clock, early).run();
  });
}
// (Tried: the rank blocks of the sidecar read beside the records, on a thread of their own, so that they are in memory when
// the choice falls.  Two 3 GB reads and the front end's start share the process's cores: the front end's estimate came
// 0.4 s later and the blocks no sooner -- 5x `search` 2.4 -> 2.7 s.  They are read when they are wanted.)
void SearchRun::load_index() {
  check(svdss_index_load(o.index.c_str(), &ix), "svdss_index_load");
  for (EarlySearch* es : early) es->index_n.store(svdss_index_size(ix));
  if (o.verbose) logmsg("debug", "index file read at +" + clock.since() + " s");
}
void SearchRun::choose_kmer_order() { user_kmer = ::choose_kmer_order(bam_mode ? o.bam : o.fastx, bam_mode, ix, o.verbose); }   // (sfs_units.h)
void SearchRun::choose_rank_blocks_alone() {
  // (one decision for the process, from the sum over the regions' front ends; the blocks are read once: sfs_units.h)
  if (!early.empty()) lf_only = ::choose_rank_blocks_alone(knobs, early, ix, o.index, user_kmer, o.verbose, clock, n_gpus);
}
void SearchRun::index_to_device() {
  check(svdss_index_to_device(ix, 0), "svdss_index_to_device");
  if (o.verbose) logmsg("debug", "index and k-mer table on the device at +" + clock.since() + " s" +
                                     (lf_only ? " (rank blocks alone: few reads to search)"
                                      : !early.empty() && svdss_index_kmer(ix) < 16 ? " (table of order " + std::to_string(svdss_index_kmer(ix)) + ": few reads to search)" : ""));
}
// the early path's second half: the front end gets the index, searches what it parked and goes on with whole batches
void SearchRun::release_index_to_front_end() {
  EarlySearch* const es = early[0];
  if (lf_only) es->offer_index_held_back(ix);
  logmsg("info", "Extracting SFS strings on the GPU (output order as with " + std::to_string(o.threads) + " threads)..");
  // (SVDSS_EARLY_HOLD_MS, for the tests: the index is held back that long, as if its restore had taken seconds)
  if (knobs.early_hold_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(knobs.early_hold_ms));
  es->release_index(ix);
  front_end.join();
  replicas.assign(1, ix);
}
// ... with --gpus N: every GPU's replica is made resident at once -- svdss_index_to_device on GPU 0, svdss_index_replicate
// for the others (the rank blocks alone: uploads from the ONE host copy; else a build per GPU from the records) -- on a
// thread per region, which then hands ITS region its replica: held back until that region's front end is through or its
// park is full when the index is the rank blocks alone (offer_index_held_back blocks: hence the thread), then released.
// Region 0 does not wait for the other replicas, and no region for another region's front end.
void SearchRun::release_replicas_to_front_ends() {
  logmsg("info", "Extracting SFS strings on the GPU (output order as with " + std::to_string(o.threads) + " threads)..");
  replicas.assign((size_t)n_gpus, ix);
  // (which form was taken is said once: choose_rank_blocks_alone says the other)
  if (o.verbose && !lf_only) logmsg("debug", "the index as a full restore on each of " + std::to_string(n_gpus) + " GPUs, built beside the regions' front ends from +" + clock.since() + " s");
  // (more replicas than GPUs, SVDSS_GPUS_OVERSUBSCRIBE: full builds that share a GPU go one after the other -- the
  // buffers of two suffix sorts are not meant to fit side by side, and one GPU gains nothing from two at once)
  std::mutex m;
  std::condition_variable cv;
  std::vector<char> resident((size_t)n_gpus, 0);
  std::vector<std::thread> th;
  for (int d = 0; d < n_gpus; ++d)
    th.emplace_back([this, &m, &cv, &resident, d] {
      if (!lf_only && d >= n_dev) { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return resident[(size_t)(d - n_dev)] != 0; }); }
      const int rc = d == 0 ? svdss_index_to_device(ix, 0) : svdss_index_replicate(ix, d % n_dev, &replicas[(size_t)d]);
      if (rc != SVDSS_OK) check(rc, d == 0 ? "svdss_index_to_device" : "svdss_index_replicate");     // (the regions' feeders wait for it: the run ends here)
      { std::lock_guard<std::mutex> lk(m); resident[(size_t)d] = 1; }
      cv.notify_all();
      svdss_index_t* mine = replicas[(size_t)d];
      if (o.verbose) logmsg("debug", "GPU " + std::to_string(d % n_dev) + ": replica " + std::to_string(d) + " of the index resident at +" + clock.since() + " s" +
                                         (lf_only ? " (rank blocks alone, uploaded from the one host copy)"
                                          : svdss_index_kmer(mine) < 16 ? " (table of order " + std::to_string(svdss_index_kmer(mine)) + ")" : ""));
      EarlySearch* const es = early[(size_t)d];
      if (lf_only) es->offer_index_held_back(mine);
      // (SVDSS_EARLY_HOLD_MS, for the tests: the index is held back that long, as if its restore had taken seconds)
      if (knobs.early_hold_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(knobs.early_hold_ms));
      es->release_index(mine);
    });
  for (std::thread& t : th) t.join();
  logmsg("info", "Index replicated on " + std::to_string(n_gpus) + " GPUs");
  front_end.join();
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
    // an eligible file (regular; BGZF, not compressed, or -- SVDSS_FASTX_GZIP_DEVICE=1 -- plain gzip) has its records found on
    // the GPU; SVDSS_FASTX_DEVICE=0: the host reader
    const FastxKind kind = knobs.fastx_device && svdss_device_count() > 0 ? fastx_device_kind(o.fastx, knobs.fastx_gzip_device) : FastxKind::None;
    if (kind != FastxKind::None) {
      if (o.bsize <= 0) die("batch size smaller than the number of threads");
      logmsg("info", "Extracting SFS strings on the GPU (output order as with " + std::to_string(o.threads) + " threads)..");
      FastxDevicePath(o, knobs, replicas, kind, clock).run();
      return;
    }
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
    bam_regions_report();
    logmsg("info", "All done! Runtime: " + std::to_string((long)(time(nullptr) - t_process)) + " seconds");
    fflush(stdout);
    fflush(stderr);
    _exit(0);
  }
  for (EarlySearch* es : early) svdss_bam_park_free(es->park);
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
  if (run.early.size() > 1) {
    run.release_replicas_to_front_ends();
  } else if (!run.early.empty()) {
    run.index_to_device();
    run.release_index_to_front_end();
  } else {
    run.index_to_device();
    run.replicate();
    if (run.dev_bam) run.run_device_path(); else run.run_host_path();
  }
  return run.finish();
}
