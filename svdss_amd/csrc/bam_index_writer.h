// bam_index_writer.h -- the BAI / CSI index of the BAM `SVDSS smooth` writes (`smooth --write-index FILE`, what
// `samtools index` of the output gives; SAM specification 5.2 / 5.3).
//
// The device path reduces every batch on the GPU (csrc/bam_smooth.hip: chunks = runs of consecutive records with the same
// (tid, bin), the 16 kb windows the batch's records reach into first) and BamIndexBuilder folds those fragments in file
// order; the host paths feed it one record at a time.  Both give the same bytes for the same BAM.
//
// The same builder indexes the BAM a command is GIVEN (`SVDSS bamindex`, `call / run --write-bam-index`; the input side:
// add_input_fragment / add_input_seam / add_input_record / finish_input).  There every record counts: records with flag 4
// and a position are indexed and counted as unmapped in the pseudo-bin, records without a reference are counted in the
// trailing n_no_coor, and a record's end at the last byte of a batch waits for the next non-empty member of the file.
//
// Virtual offsets: a position is addressed by the member that holds its byte, so a record that starts exactly at a block
// boundary is "start of block k + 1", and the end of the last record is the offset right after the last data member (the
// EOF marker) -- what htslib's bgzf_tell gives while reading.  They count from the first byte `smooth` writes to stdout.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/svdss_hip.h"
#include "bam_writer.h"

#if defined(__HIPCC__)
#define SVDSS_IX_HD __host__ __device__
#else
#define SVDSS_IX_HD
#endif

// positions a (min_shift, depth) scheme can bin: [0, 2^(min_shift + 3 depth))
SVDSS_IX_HD inline int64_t ix_limit(int min_shift, int depth) { return (int64_t)1 << (min_shift + 3 * depth); }

// a record's [beg, end) as the index sees it: end = beg + max(reference span of the CIGAR, 1), both kept inside the
// scheme's range (a record past it -- a position beyond its contig -- is binned at the range's end instead of refused)
SVDSS_IX_HD inline void ix_extent(int32_t pos, int64_t span, int min_shift, int depth, int64_t& beg, int64_t& end) {
  const int64_t lim = ix_limit(min_shift, depth);
  beg = pos < 0 ? 0 : (int64_t)pos;
  if (beg >= lim) beg = lim - 1;
  end = beg + (span < 1 ? 1 : span);
  if (end > lim) end = lim;
}

// SAM specification 5.3: the smallest bin that holds [beg, end)
SVDSS_IX_HD inline uint32_t ix_reg2bin(int64_t beg, int64_t end, int min_shift, int depth) {
  --end;
  int s = min_shift;
  int64_t t = (((int64_t)1 << (depth * 3)) - 1) / 7;
  for (int l = depth; l > 0; --l) {
    if (beg >> s == end >> s) return (uint32_t)(t + (beg >> s));
    s += 3;
    t -= (int64_t)1 << ((l - 1) * 3);
  }
  return 0;
}

SVDSS_IX_HD inline bool ix_ref_op(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// the scheme of an index file: a name ending in ".csi" gets CSIv1 with min_shift 14 and the smallest depth >= 5 whose range
// covers the longest reference (+ 256, as htslib sizes n_lvls); anything else BAI, which cannot hold a reference longer than
// 2^29 - 1.  false and a message if the references do not fit.
inline bool bam_index_scheme(const std::string& path, const std::vector<int32_t>& lens, bool& csi, int& min_shift, int& depth,
                             std::string& err) {
  csi = path.size() >= 4 && path.compare(path.size() - 4, 4, ".csi") == 0;
  min_shift = 14;
  depth = 5;
  int64_t max_len = 0;
  for (int32_t l : lens) max_len = std::max<int64_t>(max_len, l);
  if (!csi) {
    if (max_len > ((int64_t)1 << 29) - 1) {
      err = "--write-index " + path + ": a reference is " + std::to_string(max_len) +
            " bases long, more than a BAI index can hold (2^29 - 1); name the index *.csi to write a CSI index";
      return false;
    }
    return true;
  }
  while (ix_limit(min_shift, depth) < max_len + 256) ++depth;
  return true;
}

class BamIndexBuilder {
 public:
  BamIndexBuilder(int32_t n_ref, bool csi, int min_shift, int depth) : refs_((size_t)(n_ref < 0 ? 0 : n_ref)), csi_(csi), min_shift_(min_shift), depth_(depth) {}

  // the device path: one batch's fragments (svdss_bam_batch_index), batches in file order; base = compressed offset of the
  // batch's first member in the output
  void add_fragment(const svdss_bam_index_frag_t& f, uint64_t base) {
    if (f.unsorted) unsorted_ = true;
    if (f.n_chunks == 0) return;
    order(f.first_tid, f.first_beg);
    order(f.last_tid, f.last_beg);
    const uint64_t sh = base << 16;
    for (int64_t i = 0; i < f.n_chunks; ++i) {
      const svdss_bam_index_chunk_t& c = f.chunks[i];
      add_chunk(c.tid, c.bin, c.n_rec, c.v_beg + sh, c.v_end + sh);
    }
    for (int64_t i = 0; i < f.n_windows; ++i) {
      const svdss_bam_index_window_t& w = f.windows[i];
      add_window(w.tid, w.window, w.v_beg + sh);
    }
  }

  // the host paths: one record, in file order, with its reference span and virtual offsets
  void add_record(int32_t tid, int32_t pos, int64_t span, uint64_t v_beg, uint64_t v_end) {
    int64_t beg, end;
    ix_extent(pos, span, min_shift_, depth_, beg, end);
    order(tid, beg);
    if (tid < 0 || (size_t)tid >= refs_.size()) { unsorted_ = true; return; }
    add_chunk(tid, ix_reg2bin(beg, end, min_shift_, depth_), 1, v_beg, v_end);
    // the windows no earlier record reached (what the device path's windows are, batch by batch)
    Ref& r = refs_[(size_t)tid];
    const int64_t w0 = beg >> min_shift_, w1 = (end - 1) >> min_shift_;
    for (int64_t w = std::max<int64_t>(w0, r.max_win + 1); w <= w1; ++w) add_window(tid, (int32_t)w, v_beg);
  }

  // ---- the input side
  // the device path: one batch's fragments (svdss_bam_batch_input_index), batches in file order; base = file offset of the
  // batch's first member (a region of the file: the region's offset + the members of its batches so far)
  void add_input_fragment(const svdss_bam_input_frag_t& f, uint64_t base) {
    if (!f.on) return;
    // an end the batch in front left at its last byte: the first member of this one that holds a byte
    if (f.first_data >= 0) resolve_pending((base + (uint64_t)f.first_data) << 16);
    if (f.unsorted) unsorted_ = true;
    n_no_coor_ += (uint64_t)f.n_no_coor;
    if (f.n_records > 0) { order_input(f.first_tid, f.first_beg); order_input(f.last_tid, f.last_beg); }
    const uint64_t sh = base << 16;
    for (int64_t i = 0; i < f.n_chunks; ++i) {
      const svdss_bam_input_chunk_t& c = f.chunks[i];
      add_chunk(c.tid, c.bin, c.n_rec - c.n_unmapped, c.v_beg + sh, c.v_end + sh, c.n_unmapped);
    }
    for (int64_t i = 0; i < f.n_windows; ++i) {
      const svdss_bam_input_window_t& w = f.windows[i];
      add_window(w.tid, w.window, w.v_beg + sh);
    }
    pending_ = f.ends_at_boundary != 0 && f.n_chunks > 0 && have_last_;
  }
  // the ONE record a seam between two regions of the file completes (f: the seam's batch, whose own offsets mean nothing
  // in the file): it starts at v_beg, where the carry of the region in front begins, and ends at v_end, the first record
  // start of the region behind
  void add_input_seam(const svdss_bam_input_frag_t& f, uint64_t v_beg, uint64_t v_end) {
    if (!f.on) return;
    if (f.n_records != 1) { unsorted_ = true; return; }    // (the caller runs such a region again instead)
    n_no_coor_ += (uint64_t)f.n_no_coor;
    order_input(f.first_tid, f.first_beg);
    for (int64_t i = 0; i < f.n_chunks; ++i) add_chunk(f.chunks[i].tid, f.chunks[i].bin, 1 - f.chunks[i].n_unmapped, v_beg, v_end, f.chunks[i].n_unmapped);
    for (int64_t i = 0; i < f.n_windows; ++i) add_window(f.windows[i].tid, f.windows[i].window, v_beg);
    pending_ = false;
  }
  // the host reader: one record of the input, in file order, with its flag, reference span and final virtual offsets
  void add_input_record(int32_t tid, int32_t pos, uint32_t flag, int64_t span, uint64_t v_beg, uint64_t v_end) {
    int64_t beg, end;
    ix_extent(pos, span, min_shift_, depth_, beg, end);
    order_input(tid, tid < 0 ? 0 : beg);
    if (tid < 0) { ++n_no_coor_; return; }
    if ((size_t)tid >= refs_.size()) { unsorted_ = true; return; }
    const bool unm = (flag & 4u) != 0;
    add_chunk(tid, ix_reg2bin(beg, end, min_shift_, depth_), unm ? 0 : 1, v_beg, v_end, unm ? 1 : 0);
    Ref& r = refs_[(size_t)tid];
    const int64_t w0 = beg >> min_shift_, w1 = (end - 1) >> min_shift_;
    for (int64_t w = std::max<int64_t>(w0, r.max_win + 1); w <= w1; ++w) add_window(tid, (int32_t)w, v_beg);
  }
  // the input has ended: end_offset = where its EOF marker is (the file's size where it has none)
  void finish_input(uint64_t end_offset) { resolve_pending(end_offset << 16); }
  bool unsorted() const { return unsorted_; }
  uint64_t n_no_coor() const { return n_no_coor_; }
  uint64_t n_chunks() const { uint64_t n = 0; for (const Ref& r : refs_) for (const auto& kv : r.bins) n += kv.second.size(); return n; }
  uint64_t n_windows() const { uint64_t n = 0; for (const Ref& r : refs_) n += r.lin.size(); return n; }

  // the index into `path` (through path + ".tmp", renamed into place when complete); false and a message otherwise
  bool write(const std::string& path, std::string& err) const {
    if (unsorted_) { err = "--write-index: the records are not sorted by coordinate; no index written"; return false; }
    const std::string tmp = path + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) { err = "cannot write " + tmp; return false; }
    bool ok = encode(f);
    ok = fclose(f) == 0 && ok;
    if (ok && rename(tmp.c_str(), path.c_str()) != 0) ok = false;
    if (!ok) { unlink(tmp.c_str()); err = "cannot write " + path; }
    return ok;
  }
  // the file's bytes into f (BGZF for CSI); the caller has looked at unsorted()
  bool encode(FILE* f) const {
    std::vector<uint8_t> out;
    auto put = [&](const void* p, size_t n) { out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
    auto p32 = [&](uint32_t v) { put(&v, 4); };
    auto p64 = [&](uint64_t v) { put(&v, 8); };
    const uint32_t meta = csi_ ? (uint32_t)((((int64_t)1 << (3 * depth_ + 3)) - 1) / 7 + 1) : 37450u;
    if (csi_) { put("CSI\1", 4); p32((uint32_t)min_shift_); p32((uint32_t)depth_); p32(0); }
    else put("BAI\1", 4);
    p32((uint32_t)refs_.size());
    for (const Ref& r : refs_) {
      p32((uint32_t)(r.bins.size() + (r.any ? 1 : 0)));
      // CSI: per bin the start of the first record that reaches into its range = the window entry of the first window of
      // the range any record reaches (the entries grow with the window: the records are sorted)
      std::vector<int64_t> covered;
      if (csi_)
        for (size_t w = 0; w < r.lin.size(); ++w)
          if (r.lin[w] != kNone) covered.push_back((int64_t)w);
      for (const auto& kv : r.bins) {
        p32(kv.first);
        if (csi_) {
          int l = 0;
          while (first_bin(l + 1) <= (int64_t)kv.first) ++l;
          const int64_t w_lo = ((int64_t)kv.first - first_bin(l)) << (3 * (depth_ - l));
          const auto it = std::lower_bound(covered.begin(), covered.end(), w_lo);
          p64(it == covered.end() ? 0 : r.lin[(size_t)*it]);
        }
        p32((uint32_t)kv.second.size());
        for (const auto& c : kv.second) { p64(c.first); p64(c.second); }
      }
      if (r.any) {
        // htslib's metadata pseudo-bin: the span of the reference's records in the file, mapped / unmapped counts
        // (`smooth` writes mapped records only: unmapped ones are dropped with the other filters; an input BAM may hold
        // records with flag 4 and a position)
        p32(meta);
        if (csi_) p64(0);
        p32(2);
        p64(r.first); p64(r.last);
        p64(r.n_mapped); p64(r.n_unmapped);
      }
      if (!csi_) {
        p32((uint32_t)r.lin.size());
        uint64_t last = 0;
        for (uint64_t v : r.lin) { if (v != kNone) last = v; p64(last); }
      }
    }
    p64(n_no_coor_);
    if (csi_) {
      BgzfWriter w(f, 1);
      w.write(out.data(), out.size());
      return w.finish();
    }
    return fwrite(out.data(), 1, out.size(), f) == out.size() && fflush(f) == 0;
  }

 private:
  static constexpr uint64_t kNone = ~(uint64_t)0;
  struct Ref {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
    std::vector<uint64_t> lin;      // per window: the first record's start (kNone: no record reaches into it)
    int64_t max_win = -1;
    uint64_t n_mapped = 0, n_unmapped = 0, first = 0, last = 0;
    bool any = false;               // a record of the reference has been added (the pseudo-bin is written)
  };
  static int64_t first_bin(int l) { return (((int64_t)1 << (3 * l)) - 1) / 7; }

  void order(int32_t tid, int64_t beg) {
    if (have_prev_ && (tid < prev_tid_ || (tid == prev_tid_ && beg < prev_beg_))) unsorted_ = true;
    have_prev_ = true; prev_tid_ = tid; prev_beg_ = beg;
  }
  // (the input side: tid < 0 sorts behind every reference)
  void order_input(int32_t tid, int64_t beg) { order(tid < 0 ? 0x7fffffff : tid, tid < 0 ? 0 : beg); }
  void resolve_pending(uint64_t v) {
    if (!pending_) return;
    pending_ = false;
    Ref& r = refs_[(size_t)last_tid_];
    r.bins[last_bin_].back().second = v;
    r.last = v;
  }
  void add_chunk(int32_t tid, uint32_t bin, int64_t n, uint64_t v0, uint64_t v1, int64_t n_unm = 0) {
    if (tid < 0 || (size_t)tid >= refs_.size()) { unsorted_ = true; return; }
    Ref& r = refs_[(size_t)tid];
    std::vector<std::pair<uint64_t, uint64_t>>& ch = r.bins[bin];
    // a run that continues the previous one (the first chunk of a batch after the last of the batch before)
    if (have_last_ && last_tid_ == tid && last_bin_ == bin && !ch.empty() && ch.back().second == v0) ch.back().second = v1;
    else ch.emplace_back(v0, v1);
    have_last_ = true; last_tid_ = tid; last_bin_ = bin;
    if (!r.any) r.first = v0;
    r.any = true;
    r.last = v1;
    r.n_mapped += (uint64_t)n;
    r.n_unmapped += (uint64_t)n_unm;
  }
  void add_window(int32_t tid, int32_t w, uint64_t v) {
    if (tid < 0 || (size_t)tid >= refs_.size() || w < 0) return;
    Ref& r = refs_[(size_t)tid];
    if ((size_t)w >= r.lin.size()) r.lin.resize((size_t)w + 1, kNone);
    if (r.lin[(size_t)w] == kNone) r.lin[(size_t)w] = v;
    if (w > r.max_win) r.max_win = w;
  }

  std::vector<Ref> refs_;
  bool csi_;
  int min_shift_, depth_;
  bool unsorted_ = false, have_prev_ = false, have_last_ = false;
  bool pending_ = false;            // the last chunk's end is the last byte of its batch: waits for the next non-empty member
  uint64_t n_no_coor_ = 0;
  int32_t prev_tid_ = -1, last_tid_ = -1;
  int64_t prev_beg_ = 0;
  uint32_t last_bin_ = 0;
};
