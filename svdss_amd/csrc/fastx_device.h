// fastx_device.h -- the input side of `SVDSS search --fastx` on the device (csrc/fastx_device.hip): which files are
// eligible, and the file cut into batches -- runs of consecutive BGZF members found by BgzfScanner, slabs of a plain
// file, or (plain gzip, inflated by csrc/gzip_stream.hip in a source thread of the caller's) slabs of text put().  The batches are numbered in file order; whoever takes one (the feeding threads of search_host.cpp's
// FastxDevicePath) hands it to svdss_fastx_batch_run.  Nothing is inflated or parsed here.
#pragma once
#include <sys/stat.h>
#include <unistd.h>

#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bgzf_scanner.h"

enum class FastxKind { None, Plain, Bgzf, Gzip };

// A regular file that is BGZF (a gzip header with the BC extra field, what bgzip writes) or not compressed at all; pipes and
// everything else stay with the host reader.  Plain single-stream gzip (magic, CM = 8, not BGZF) is FastxKind::Gzip where the
// caller asks for it (`search --fastx`), and stays with the host reader otherwise (the reference FASTA).
inline FastxKind fastx_device_kind(const std::string& path, bool gzip_too = false) {
  struct stat st;
  if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return FastxKind::None;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return FastxKind::None;
  uint8_t h[4096];
  const size_t n = fread(h, 1, sizeof h, f);
  fclose(f);
  if (n >= 2 && h[0] == 0x1f && h[1] == 0x8b) {
    size_t total = 0, doff = 0, dlen = 0;
    if (BgzfScanner::parse_member(h, n, total, doff, dlen) == 1) return FastxKind::Bgzf;
    return gzip_too && n >= 3 && h[2] == 8 ? FastxKind::Gzip : FastxKind::None;
  }
  return FastxKind::Plain;
}

// one batch of the input: consecutive BGZF members piece by piece (a piece = members of one slab), or a range of a plain file
struct FastxJob {
  int64_t seq = 0;
  bool last = false;
  std::vector<std::shared_ptr<CompChunk>> keep;            // the slabs stay with the job until it has run
  std::vector<std::vector<svdss_bgzf_block_t>> tables;     // every piece's members, coff relative to the piece's first byte
  std::vector<const uint8_t*> comp;
  std::vector<int64_t> comp_bytes, n_blocks;
  std::vector<const svdss_bgzf_block_t*> blocks;
  std::vector<const uint32_t*> crc;
  int64_t plain_off = 0, plain_bytes = 0;
  std::shared_ptr<std::vector<uint8_t>> text;              // FastxKind::Gzip: the plain_bytes of this batch, already inflated
  void clear() {
    keep.clear(); tables.clear(); comp.clear(); comp_bytes.clear(); n_blocks.clear(); blocks.clear(); crc.clear();
    plain_off = plain_bytes = 0; last = false; text.reset();
  }
};

class FastxBatcher {
 public:
  FastxBatcher(const std::string& path, FastxKind kind, int64_t batch_bytes, size_t slab_bytes, int loaders, size_t pool_chunks)
      : kind_(kind), batch_(batch_bytes < 1 ? 1 : batch_bytes) {
    if (kind == FastxKind::Bgzf) {
      BgzfScanner::Hooks hooks;
      hooks.host_alloc = svdss_host_alloc;
      hooks.host_free = svdss_host_free;
      scanner_.reset(new BgzfScanner(path, hooks, slab_bytes, loaders, pool_chunks));
      ok_ = scanner_->ok();
    } else if (kind == FastxKind::Gzip) {
      ok_ = true;
    } else {
      struct stat st;
      ok_ = stat(path.c_str(), &st) == 0;
      size_ = ok_ ? (int64_t)st.st_size : 0;
    }
  }
  bool ok() const { return ok_; }
  // the next batch in file order (any thread); false: there is none -- the input has ended, or error() says what failed
  bool next(FastxJob& job) {
    std::lock_guard<std::mutex> lk(m_);
    job.clear();
    if (ended_) return false;
    if (kind_ == FastxKind::Gzip) return next_text(job);
    job.seq = seq_++;
    if (kind_ == FastxKind::Plain) {
      job.plain_off = off_;
      job.plain_bytes = std::min(batch_, size_ - off_);
      off_ += job.plain_bytes;
      job.last = ended_ = off_ >= size_;
      return true;
    }
    int64_t acc = 0;
    while (acc < batch_) {
      if (!cur_ || at_ == cur_->blocks.size()) {
        cur_.reset();
        at_ = 0;
        std::unique_ptr<CompChunk> c = scanner_->next();
        if (!c) {
          if (!scanner_->error().empty()) { err_ = scanner_->error(); ended_ = true; return false; }
          job.last = ended_ = true;        // (the last batch may be empty: it closes the stream)
          break;
        }
        BgzfScanner* sc = scanner_.get();
        cur_ = std::shared_ptr<CompChunk>(c.release(), [sc](CompChunk* p) { sc->recycle(std::unique_ptr<CompChunk>(p)); });
        if (cur_->blocks.empty()) continue;
      }
      // members [at_, e) of the slab, as many as the batch still takes
      size_t e = at_;
      while (e < cur_->blocks.size() && acc < batch_) acc += cur_->blocks[e++].isize;
      const int64_t c0 = cur_->blocks[at_].coff, c1 = cur_->blocks[e - 1].coff + cur_->blocks[e - 1].clen;
      job.tables.emplace_back(cur_->blocks.begin() + (long)at_, cur_->blocks.begin() + (long)e);
      for (svdss_bgzf_block_t& b : job.tables.back()) b.coff -= c0;
      job.keep.push_back(cur_);
      job.comp.push_back(cur_->data + c0);
      job.comp_bytes.push_back(c1 - c0);
      job.n_blocks.push_back((int64_t)(e - at_));
      job.crc.push_back(cur_->crc.data() + at_);
      at_ = e;
    }
    for (const std::vector<svdss_bgzf_block_t>& t : job.tables) job.blocks.push_back(t.data());
    return true;
  }
  const std::string& error() const { return err_; }
  int64_t batch_bytes() const { return batch_; }
  // FastxKind::Gzip: the source thread's side.  Text in file order, cut into batches of batch_bytes; at most `depth`
  // batches wait (put blocks); finish() closes the stream with the last -- possibly empty -- batch.
  void put(const uint8_t* text, size_t n, size_t depth) {
    while (n) {
      if (!filling_) { filling_.reset(new std::vector<uint8_t>()); filling_->reserve((size_t)batch_); }
      const size_t k = std::min(n, (size_t)batch_ - filling_->size());
      filling_->insert(filling_->end(), text, text + k);
      text += k;
      n -= k;
      if (filling_->size() == (size_t)batch_) push(depth, false);
    }
  }
  void finish() {
    if (!filling_) filling_.reset(new std::vector<uint8_t>());
    push(~(size_t)0, true);
  }

 private:
  void push(size_t depth, bool last) {
    std::unique_lock<std::mutex> lk(qm_);
    qcv_.wait(lk, [&] { return queue_.size() < depth; });
    queue_.emplace_back(std::move(filling_), last);
    filling_.reset();
    lk.unlock();
    qcv_.notify_all();
  }
  // (m_ is held: the batch's number follows the queue's order)
  bool next_text(FastxJob& job) {
    std::unique_lock<std::mutex> lk(qm_);
    qcv_.wait(lk, [&] { return !queue_.empty(); });
    job.text = std::move(queue_.front().first);
    job.last = ended_ = queue_.front().second;
    queue_.pop_front();
    lk.unlock();
    qcv_.notify_all();
    job.seq = seq_++;
    job.plain_bytes = (int64_t)job.text->size();
    return true;
  }
  std::mutex qm_;
  std::condition_variable qcv_;
  std::deque<std::pair<std::shared_ptr<std::vector<uint8_t>>, bool>> queue_;
  std::shared_ptr<std::vector<uint8_t>> filling_;
  const FastxKind kind_;
  const int64_t batch_;
  bool ok_ = false, ended_ = false;
  std::mutex m_;
  std::unique_ptr<BgzfScanner> scanner_;
  std::shared_ptr<CompChunk> cur_;
  size_t at_ = 0;
  int64_t seq_ = 0, off_ = 0, size_ = 0;
  std::string err_;
};
