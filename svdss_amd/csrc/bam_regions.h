// bam_regions.h -- `--region REG` / `--regions-file BED`: the texts turned into intervals of the BAM header's references,
// and the record test every reader of the binary applies (the host readers here; the device path through
// svdss_bam_stream_set_regions, csrc/bam_device.hip: gate_kernel).
//
// The meaning, in one place: with the union U of the regions a command behaves as it does on a BAM with the same header
// that holds exactly the records with tid >= 0 whose [pos, bam_endpos) overlaps an interval of U on their reference, in
// file order, each once.  bam_endpos = pos + the reference length of the CIGAR, pos + 1 where that length is 0 (as in
// select_kernel).  A record whose fields do not fit its block_size is never tested: every reader checks a record's sizes
// BEFORE it asks the gate (BamReader::next*_any, bam_scan_chunks) or keeps it for the kernel that raises the error
// (gate_kernel), so a damaged record ends the run with "corrupt record" on every path, inside a region or not.  Stands where `samtools view -b in.bam REG...` in front of the command would stand.
// No HIP, no library: tests compile this header alone.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// sorted, merged intervals (0-based, half open) of the references of one BAM header: those of reference t are
// [off[t], off[t + 1]) of beg / end
struct BamRegionSet {
  int32_t n_ref = 0;
  std::vector<int64_t> off;
  std::vector<int32_t> tid, beg, end;

  size_t size() const { return beg.size(); }
  // from intervals in any order, overlapping or not (empty ones are dropped)
  void assign(int32_t n_ref_, std::vector<std::pair<int32_t, std::pair<int32_t, int32_t>>> iv) {
    n_ref = n_ref_;
    tid.clear(); beg.clear(); end.clear();
    std::sort(iv.begin(), iv.end());
    for (const auto& x : iv) {
      if (x.second.second <= x.second.first) continue;
      if (!tid.empty() && tid.back() == x.first && x.second.first <= end.back()) { end.back() = std::max(end.back(), x.second.second); continue; }
      tid.push_back(x.first); beg.push_back(x.second.first); end.push_back(x.second.second);
    }
    off.assign((size_t)n_ref + 1, 0);
    for (int32_t t : tid) ++off[(size_t)t + 1];
    for (int32_t t = 0; t < n_ref; ++t) off[(size_t)t + 1] += off[(size_t)t];
  }
  // does [a_beg, a_end) on reference t overlap an interval?
  bool overlaps(int32_t t, int64_t a_beg, int64_t a_end) const {
    if (t < 0 || t >= n_ref) return false;
    // the first interval that ends behind a_beg overlaps iff it begins before a_end
    const int32_t* e0 = end.data() + off[(size_t)t];
    const int32_t* e1 = end.data() + off[(size_t)t + 1];
    const int32_t* it = std::upper_bound(e0, e1, a_beg, [](int64_t v, int32_t e) { return v < (int64_t)e; });
    return it != e1 && (int64_t)beg[(size_t)(it - end.data())] < a_end;
  }
  // a record by its core fields and its CIGAR (n_cigar little-endian words, unaligned)
  bool keeps(int32_t t, int32_t pos, const uint8_t* cigar, uint32_t n_cigar) const {
    if (t < 0 || t >= n_ref || off[(size_t)t + 1] == off[(size_t)t]) return false;
    int64_t ref_len = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
      uint32_t c;
      memcpy(&c, cigar + 4 * (size_t)k, 4);
      const uint32_t op = c & 15u;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += c >> 4;
    }
    return overlaps(t, pos, (int64_t)pos + (ref_len ? ref_len : 1));
  }
};

namespace bam_regions_detail {
// digits with commas ignored; false: empty, something else, or beyond int64
inline bool to_coord(const std::string& s, int64_t& out) {
  int64_t v = 0;
  size_t digits = 0;
  for (char c : s) {
    if (c == ',') continue;
    if (c < '0' || c > '9') return false;
    if (v > (INT64_MAX - 9) / 10) return false;
    v = v * 10 + (c - '0');
    ++digits;
  }
  out = v;
  return digits > 0;
}
inline int32_t clamp31(int64_t v) { return (int32_t)std::min<int64_t>(v, INT32_MAX); }
inline int find_name(const std::vector<std::string>& names, const std::string& n) {
  for (size_t t = 0; t < names.size(); ++t)
    if (names[t] == n) return (int)t;
  return -1;
}
}  // namespace bam_regions_detail

// One --region text against the header's names: NAME | NAME:BEG-END | NAME:BEG- | NAME:BEG (1-based, inclusive; NAME:BEG runs
// to the end of the reference, as samtools reads it).  A text that IS a name of the header is that whole reference (names
// may hold ':'); any other is split at its last ':'.
inline bool parse_region_text(const std::string& text, const std::vector<std::string>& names, int32_t& tid, int32_t& beg, int32_t& end, std::string& err) {
  using namespace bam_regions_detail;
  int t = find_name(names, text);
  if (t >= 0) { tid = t; beg = 0; end = INT32_MAX; return true; }
  const size_t colon = text.rfind(':');
  if (colon == std::string::npos) { err = "--region " + text + ": the BAM header has no reference of that name"; return false; }
  const std::string name = text.substr(0, colon), range = text.substr(colon + 1);
  t = find_name(names, name);
  if (t < 0) { err = "--region " + text + ": the BAM header has no reference named " + name; return false; }
  const size_t dash = range.find('-');
  int64_t b = 0, e = INT32_MAX;
  const std::string bs = range.substr(0, dash);
  if (!range.empty() && range[0] == '-') { err = "--region " + text + ": BEG must be at least 1"; return false; }
  if (!to_coord(bs, b)) { err = "--region " + text + ": cannot read BEG in '" + range + "'"; return false; }
  if (dash != std::string::npos && dash + 1 < range.size() && !to_coord(range.substr(dash + 1), e)) {
    err = "--region " + text + ": cannot read END in '" + range + "'";
    return false;
  }
  if (b < 1) { err = "--region " + text + ": BEG must be at least 1"; return false; }
  if (e < b) { err = "--region " + text + ": END is below BEG"; return false; }
  tid = t; beg = clamp31(b - 1); end = clamp31(e);
  return true;
}

// --region texts and / or a BED file (at least three tab-separated columns, 0-based half open; lines that start with '#',
// "track" or "browser" and empty lines are skipped) into U.  false and a message that names the offending text.
inline bool resolve_regions(const std::vector<std::string>& texts, const std::string& bed_path, const std::vector<std::string>& names, BamRegionSet& U,
                            std::string& err) {
  using namespace bam_regions_detail;
  std::vector<std::pair<int32_t, std::pair<int32_t, int32_t>>> iv;
  for (const std::string& t : texts) {
    int32_t tid, b, e;
    if (!parse_region_text(t, names, tid, b, e, err)) return false;
    iv.push_back({tid, {b, e}});
  }
  if (!bed_path.empty()) {
    FILE* f = fopen(bed_path.c_str(), "rb");
    if (!f) { err = "--regions-file " + bed_path + ": cannot open the file"; return false; }
    std::string line;
    int c = 0;
    long n_line = 0;
    while (c != EOF) {
      line.clear();
      while ((c = fgetc(f)) != EOF && c != '\n') line.push_back((char)c);
      ++n_line;
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
      const std::string where = "--regions-file " + bed_path + " line " + std::to_string(n_line) + " '" + line + "': ";
      const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
      if (t2 == std::string::npos) { err = where + "fewer than three tab-separated columns"; fclose(f); return false; }
      const size_t t3 = line.find('\t', t2 + 1);
      int64_t b = 0, e = 0;
      const std::string bs = line.substr(t1 + 1, t2 - t1 - 1), es = line.substr(t2 + 1, t3 == std::string::npos ? t3 : t3 - t2 - 1);
      if (bs.find(',') != std::string::npos || es.find(',') != std::string::npos || !to_coord(bs, b) || !to_coord(es, e)) {
        err = where + "coordinates that are not numbers"; fclose(f); return false;
      }
      if (e < b) { err = where + "the end is below the start"; fclose(f); return false; }
      const int t = find_name(names, line.substr(0, t1));
      if (t < 0) { err = where + "the BAM header has no reference named " + line.substr(0, t1); fclose(f); return false; }
      iv.push_back({(int32_t)t, {clamp31(b), clamp31(e)}});
    }
    fclose(f);
  }
  U.assign((int32_t)names.size(), std::move(iv));
  return true;
}

// The command's regions, set once by main() before anything is opened (nullptr: none given, every record is in): every
// reader of the process -- BamReader, bam_scan_chunks, the record streams of DeviceBamSelect -- applies them.
inline const BamRegionSet*& bam_regions_in_force() { static const BamRegionSet* u = nullptr; return u; }
// what the host readers counted for --verbose (bam_regions_report, bam_device_select.h): records gated out by BamReader /
// bam_scan_chunks (the device path counts its own: svdss_bam_gated_total), compressed bytes the device path read
// host_readers: BamReader objects that read the file with the regions in force (they read the whole file: no ranges)
// device_base: what the device path had counted when the regions came into force (`run --samples`: one report per sample)
struct BamRegionCounters { std::atomic<int64_t> gated{0}, comp_bytes{0}, host_readers{0}; bool verbose = false; int64_t device_base = 0; };
inline BamRegionCounters& bam_region_counters() { static BamRegionCounters c; return c; }

// The byte ranges of the BAM that a BAI / CSI names for the regions in force (bam_region_ranges.h computes them, main puts
// them here): [begin, end) at BGZF member starts, disjoint and ascending, `skip` = where the first record the index names
// begins in the range's first member.  active: the device path's scanner of `path` reads these ranges alone, as one
// stream (bgzf_scanner.h, DeviceBamSelect); not active: the whole file goes through the gate.
struct BamFileRange { size_t begin = 0, end = 0; int64_t skip = 0; };
struct BamRegionPlan {
  bool active = false;
  std::string path, index_path;
  std::vector<BamFileRange> ranges;
  size_t bytes() const { size_t b = 0; for (const BamFileRange& r : ranges) b += r.end - r.begin; return b; }
};
inline BamRegionPlan& bam_region_plan() { static BamRegionPlan p; return p; }
