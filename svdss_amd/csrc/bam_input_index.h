// bam_input_index.h -- the BAI / CSI index of the BAM a command is GIVEN (`SVDSS bamindex`, `call / run --write-bam-index FILE`):
// what `samtools index` does in a pass of its own in front of the chain.  The device path reduces every batch of the input on
// the GPU (in_ix_* kernels, csrc/bam_device.hip; svdss_bam_stream_set_input_index) and InputIndexFold folds the fragments in
// file order through BamIndexBuilder (bam_index_writer.h) -- over the regions of `--gpus N` as well; the host reader
// (index_bam_on_host) feeds the same builder record by record and writes the same bytes.
#pragma once
#include <sys/stat.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bam_device_select.h"
#include "bam_index_writer.h"
#include "bgzf_inflater.h"
#include "bgzf_scanner.h"

// where the stream of a BGZF file ends for an index: the offset of its EOF marker (a last member of 28 bytes that holds
// nothing), the file's size where it has none
inline uint64_t bam_end_offset(const std::string& path) {
  struct stat st;
  if (stat(path.c_str(), &st) != 0 || st.st_size < 0) return 0;
  const uint64_t size = (uint64_t)st.st_size;
  if (size < 28) return size;
  uint8_t t[28];
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return size;
  const bool got = fseeko(f, (off_t)(size - 28), SEEK_SET) == 0 && fread(t, 1, 28, f) == 28;
  fclose(f);
  if (!got) return size;
  size_t total = 0, doff = 0, dlen = 0;
  uint32_t isize;
  memcpy(&isize, t + 24, 4);
  return BgzfScanner::parse_member(t, 28, total, doff, dlen) == 1 && total == 28 && isize == 0 ? size - 28 : size;
}

// the reference lengths of a BAM header, in order (the host reader's own header walk)
inline bool bam_header_lengths(const std::string& path, std::vector<int32_t>& lens, std::string& err) {
  BamReader r(path);
  if (!r.ok() || !r.read_header()) { err = r.ok() ? r.error() : "cannot open file"; return false; }
  lens = r.ref_lens();
  return true;
}

// The fold of a command's input index: the scheme from FILE's name and the header, the batches of the device path in file
// order (ShardedBamSelect hands them out so: a region's seam, then its batches), the index written at the end.
class InputIndexFold {
 public:
  // false and a message: FILE cannot hold the references (a BAI for one longer than 2^29 - 1)
  bool open(const std::string& index_path, const std::vector<int32_t>& ref_lens, const char* option, std::string& err) {
    path_ = index_path;
    bool csi = false;
    if (!bam_index_scheme(index_path, ref_lens, csi, shift_, depth_, err)) {
      const std::string was = "--write-index ";
      if (err.compare(0, was.size(), was) == 0) err = std::string(option) + " " + err.substr(was.size());
      return false;
    }
    b_.reset(new BamIndexBuilder((int32_t)ref_lens.size(), csi, shift_, depth_));
    return true;
  }
  bool on() const { return b_ != nullptr; }
  int shift() const { return shift_; }
  int depth() const { return depth_; }
  // one batch's result; `sel`: where it came from (the regions' offsets, a seam's record)
  template <class Sel>
  void add(const InputFragCopy& c, const Sel& sel) {
    if (!b_ || !c.f.on) return;
    const svdss_bam_input_frag_t f = c.frag();
    records_ += (uint64_t)f.n_records;
    if (c.seam) {
      uint64_t vb = 0, ve = 0;
      sel.seam_voffsets(c.region, vb, ve);
      b_->add_input_seam(f, vb, ve);
      return;
    }
    if (!have_region_ || c.region != region_) { have_region_ = true; region_ = c.region; base_ = (uint64_t)sel.region_begin(c.region); }
    b_->add_input_fragment(f, base_);
    base_ += (uint64_t)f.comp_bytes;
  }
  // one stream over the whole file (no regions)
  void add(const InputFragCopy& c) {
    if (!b_ || !c.f.on) return;
    const svdss_bam_input_frag_t f = c.frag();
    records_ += (uint64_t)f.n_records;
    b_->add_input_fragment(f, base_);
    base_ += (uint64_t)f.comp_bytes;
  }
  BamIndexBuilder* builder() { return b_.get(); }
  void count_record() { ++records_; }
  uint64_t records() const { return records_; }
  bool unsorted() const { return b_ && b_->unsorted(); }
  // the index into FILE (FILE.tmp, renamed when complete); false and a message -- "not sorted" among them -- otherwise
  bool finish(const std::string& bam_path, std::string& err) {
    b_->finish_input(bam_end_offset(bam_path));
    if (b_->unsorted()) { err = "the records of " + bam_path + " are not sorted by coordinate: no index written"; return false; }
    return b_->write(path_, err);
  }

 private:
  std::string path_;
  std::unique_ptr<BamIndexBuilder> b_;
  int shift_ = 0, depth_ = 0;
  bool have_region_ = false;
  size_t region_ = 0;
  uint64_t base_ = 0, records_ = 0;
};

// The host reader of the input index (SVDSS_BAM_DEVICE=0): the file member by member, inflated on this thread, every record
// to the builder with the virtual offsets of the same convention -- a position at a member boundary is the start of the next
// member that holds a byte, the end of the stream is the EOF marker.  comp_bytes: the bytes of the members read.
inline bool index_bam_on_host(const std::string& path, InputIndexFold& fold, uint64_t& comp_bytes, std::string& err) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { err = "cannot open file"; return false; }
  const uint64_t end_off = bam_end_offset(path);
  struct Member { uint64_t coff; int64_t ustart; };       // the members that hold a byte: file offset, place in the inflated stream
  std::deque<Member> members;
  std::vector<uint8_t> buf;        // the inflated stream from position buf0 on
  int64_t buf0 = 0, total = 0;     // total: inflated bytes so far
  uint64_t fpos = 0;
  bool eof = false, ok = true;
  BgzfInflater inf;
  std::vector<uint8_t> comp(1 << 17);
  auto more = [&]() -> bool {      // one more member onto buf; false at the end of the file or on an error
    uint8_t h[18];
    const size_t got = fread(h, 1, 18, f);
    if (got == 0) { eof = true; return false; }
    size_t tot = 0, doff = 0, dlen = 0;
    if (got < 18 || BgzfScanner::parse_member(h, 18, tot, doff, dlen) != 1 || doff != 18) { err = got < 18 ? "truncated BGZF block" : "bad BGZF block"; ok = false; return false; }
    if (fread(comp.data(), 1, tot - 18, f) != tot - 18) { err = "truncated BGZF block"; ok = false; return false; }
    uint32_t crc, isize;
    memcpy(&crc, comp.data() + dlen, 4);
    memcpy(&isize, comp.data() + dlen + 4, 4);
    if (isize > 65536u) { err = "bad BGZF block"; ok = false; return false; }
    if (isize) {
      const size_t at = buf.size();
      buf.resize(at + isize);
      if (const char* e = inf.run(comp.data(), dlen, buf.data() + at, isize, crc)) { err = e; ok = false; return false; }
      members.push_back(Member{fpos, total});
      total += isize;
    }
    fpos += tot;
    comp_bytes += tot;
    return true;
  };
  // bytes [u, u + n) of the stream in buf; false: the stream ends before (or an error)
  auto need = [&](int64_t u, int64_t n) -> bool { while (total < u + n) if (!more()) return false; return true; };
  auto voff = [&](int64_t u) -> uint64_t {   // (the caller has made the byte at u visible, or the stream has ended at u)
    while (members.size() > 1 && members[1].ustart <= u) members.pop_front();
    if (members.empty() || u >= total) return end_off << 16;
    return (members.front().coff << 16) | (uint64_t)(u - members.front().ustart);
  };
  auto at = [&](int64_t u) -> const uint8_t* { return buf.data() + (u - buf0); };
  do {
    // the header
    if (!need(0, 12) || memcmp(at(0), "BAM\1", 4) != 0) { if (ok) err = "not a BAM file"; ok = false; break; }
    int32_t l_text, n_ref;
    memcpy(&l_text, at(4), 4);
    if (l_text < 0 || !need(0, 12 + (int64_t)l_text)) { if (ok) err = "truncated header"; ok = false; break; }
    memcpy(&n_ref, at(8 + l_text), 4);
    int64_t u = 12 + (int64_t)l_text;
    for (int32_t i = 0; i < n_ref && ok; ++i) {
      int32_t l_name;
      if (!need(u, 4)) { if (ok) err = "truncated header"; ok = false; break; }
      memcpy(&l_name, at(u), 4);
      if (l_name < 0 || !need(u, 8 + (int64_t)l_name)) { if (ok) err = "truncated header"; ok = false; break; }
      u += 8 + l_name;
    }
    if (!ok) break;
    // the records
    for (;;) {
      if (!need(u, 4)) {
        if (ok && total != u) { err = "truncated record"; ok = false; }
        break;
      }
      int32_t bs;
      memcpy(&bs, at(u), 4);
      if (bs < 32) { err = "truncated record"; ok = false; break; }
      // (the byte behind the record as well, where there is one: its end is addressed by the member that holds that byte)
      if (!need(u, 4 + (int64_t)bs)) { if (ok) err = "truncated record"; ok = false; break; }
      (void)need(u, 4 + (int64_t)bs + 1);
      if (!ok) break;
      const uint8_t* r = at(u);
      int32_t tid, pos, l_seq;
      uint16_t n_cig, flag;
      memcpy(&tid, r + 4, 4); memcpy(&pos, r + 8, 4);
      const uint32_t l_name = r[12];
      memcpy(&n_cig, r + 16, 2); memcpy(&flag, r + 18, 2); memcpy(&l_seq, r + 20, 4);
      const int64_t head = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)(l_seq < 0 ? 0 : l_seq) + 1) / 2 + (l_seq < 0 ? 0 : l_seq);
      if (l_seq < 0 || head > (int64_t)bs) { err = "corrupt record"; ok = false; break; }
      int64_t span = 0;
      for (uint32_t k = 0; k < n_cig; ++k) {
        uint32_t c;
        memcpy(&c, r + 36 + l_name + 4 * (size_t)k, 4);
        if (ix_ref_op(c & 15u)) span += c >> 4;
      }
      const uint64_t v0 = voff(u), v1 = voff(u + 4 + (int64_t)bs);
      fold.builder()->add_input_record(tid, pos, flag, span, v0, v1);
      fold.count_record();
      u += 4 + (int64_t)bs;
      // what lies in front of u is done with
      if (u - buf0 > ((int64_t)4 << 20)) { buf.erase(buf.begin(), buf.begin() + (u - buf0)); buf0 = u; }
    }
  } while (false);
  fclose(f);
  (void)eof;
  return ok;
}
