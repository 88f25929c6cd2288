// bam_region_ranges.h -- `--region` / `--regions-file`: the parts of the BAM a BAI / CSI names for the regions.
// For every merged interval of U, BaiIndex::query lists the chunks that may hold its records: the smallest chunk begin and
// the largest chunk end bound them.  A range is cut at BGZF members -- from the member of the begin offset (skip = the
// offset inside it: a record starts there, exactly) to the end of the member of the end offset -- and ranges whose members
// touch or overlap are merged, so no member is read twice and no record is seen twice.  The record gate stays the
// definition of what is in; the ranges only bound the bytes read: each costs at most its chunks plus two members.
#pragma once
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "bai_index.h"
#include "bam_regions.h"

// the ranges of `U` in the file `bam_path` as `index` names them: disjoint, ascending; false: the file cannot be read
inline bool region_file_ranges(const std::string& bam_path, const BaiIndex& index, const BamRegionSet& U, std::vector<BamFileRange>& out, std::string& err) {
  out.clear();
  FILE* f = fopen(bam_path.c_str(), "rb");
  if (!f) { err = "cannot open " + bam_path; return false; }
  struct stat st;
  const size_t fsize = fstat(fileno(f), &st) == 0 ? (size_t)st.st_size : 0;
  std::vector<std::pair<uint64_t, uint64_t>> spans;     // virtual offsets: first record's start, last record's end
  for (size_t k = 0; k < U.size(); ++k) {
    std::vector<std::pair<uint64_t, uint64_t>> chunks;
    index.query(U.tid[k], U.beg[k], U.end[k], chunks);
    if (chunks.empty()) continue;                        // (an interval that names no chunk: nothing to read for it)
    uint64_t lo = chunks[0].first, hi = chunks[0].second;
    for (const auto& c : chunks) { lo = std::min(lo, c.first); hi = std::max(hi, c.second); }
    if (hi > lo) spans.emplace_back(lo, hi);
  }
  std::sort(spans.begin(), spans.end());
  bool ok = true;
  for (const auto& sp : spans) {
    BamFileRange r;
    r.begin = (size_t)(sp.first >> 16);
    r.skip = (int64_t)(sp.first & 0xffff);
    r.end = (size_t)(sp.second >> 16);
    if (sp.second & 0xffff) {                            // the member the last record ends in: to its end
      uint8_t h[18];
      if (r.end + 18 > fsize || pread(fileno(f), h, 18, (off_t)r.end) != 18 || h[0] != 31 || h[1] != 139 || h[12] != 'B' || h[13] != 'C') {
        err = "the index names an offset of " + bam_path + " where no BGZF member starts";
        ok = false;
        break;
      }
      uint16_t bsize;
      memcpy(&bsize, h + 16, 2);
      r.end += (size_t)bsize + 1;
    }
    if (r.begin >= fsize || r.end > fsize || r.end <= r.begin) { err = "the index names offsets beyond the end of " + bam_path; ok = false; break; }
    if (!out.empty() && r.begin <= out.back().end) out.back().end = std::max(out.back().end, r.end);   // (sorted: the earlier start and its skip stay)
    else out.push_back(r);
  }
  fclose(f);
  if (!ok) out.clear();
  return ok;
}

// <bam>.bai, <bam>.csi or <stem>.bai, the first that exists; not older than the BAM, or `stale` names it and none is used
inline bool find_bam_index(const std::string& bam_path, std::string& index_path, std::string& stale) {
  struct stat sb, si;
  if (stat(bam_path.c_str(), &sb) != 0) return false;
  std::vector<std::string> cand{bam_path + ".bai", bam_path + ".csi"};
  if (bam_path.size() > 4 && bam_path.compare(bam_path.size() - 4, 4, ".bam") == 0) cand.push_back(bam_path.substr(0, bam_path.size() - 4) + ".bai");
  for (const std::string& c : cand) {
    if (stat(c.c_str(), &si) != 0) continue;
    const bool older = si.st_mtim.tv_sec < sb.st_mtim.tv_sec || (si.st_mtim.tv_sec == sb.st_mtim.tv_sec && si.st_mtim.tv_nsec < sb.st_mtim.tv_nsec);
    if (older) { if (stale.empty()) stale = c; continue; }
    index_path = c;
    return true;
  }
  return false;
}
