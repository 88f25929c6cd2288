// call_host.cpp -- host side of `SVDSS call` (the reference's caller.cpp, clusterer.cpp, sv.cpp).
//
// Integer/interval bookkeeping restated from the reference;
// the three DP seams go to the GPU through the C-ABI in three batched calls:
//   svdss_poa_consensus_batch (abPOA, caller.cpp:291), svdss_align_global_batch (ksw_extd2_sse,
//   caller.cpp:348), svdss_indel_ratio_batch (rapidfuzz::fuzz::ratio, caller.cpp:456,458).
// Thread-count dependent orderings of the reference are replayed with T = --threads.
// BAM access: the reference streams the BAM once (placement) and then issues one BAI region query
// per cluster; here the second phase is a second sequential pass that hands every alignment to
// the clusters it overlaps -- same alignments per cluster, same (file) order, no index needed.
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#define SVDSS_LOG_TAG "call"
#include "host_common.h"
#include "host_knobs.h"
#include "bai_index.h"
#include "bam_reader.h"
#include "bam_device_select.h"
#include "bam_input_index.h"
#include "gpu_inflate_hook.h"
#include "sfs_file.h"
#include "sv_record.h"
#include "call_host.h"
#include "fastx_reader.h"
#include "ref_loader.h"

namespace {


struct ESFS {   // SFS after placement (sfs.hpp:52-62)
  std::string chrom, qname;
  int rs, re, qs, qe, htag;
  bool operator<(const ESFS& c) const { return chrom == c.chrom ? rs < c.rs : chrom < c.chrom; }  // sfs.hpp:66-73
};

struct SubRead { std::string name, seq; int htag; };

struct Cluster {   // clusterer.hpp:38-139
  std::string chrom;
  int s = 0, e = 0, cov = 0, cov0 = 0, cov1 = 0, cov2 = 0;
  std::vector<ESFS> sfss;
  std::vector<std::pair<int, int>> reads;
  std::vector<SubRead> subreads;
  Cluster() {}
  Cluster(const std::string& c, int s_, int e_, int cov_, int c0, int c1, int c2)
      : chrom(c), s(s_), e(e_), cov(cov_), cov0(c0), cov1(c1), cov2(c2) {}
  size_t size() const { return subreads.size(); }
  int get_len() const {
    unsigned l = 0, n = 0;
    for (const auto& sr : subreads) { ++n; l += (unsigned)sr.seq.size(); }
    return (int)(l / n);
  }
  Cluster cleared_copy() const { return Cluster(chrom, s, e, cov, cov0, cov1, cov2); }  // copy ctor drops `reads`
};

typedef std::vector<std::pair<int, int>> Pairs;

// bam.cpp:92-134
Pairs get_aligned_pairs(const BamRecord& a) {
  Pairs res;
  int ref_pos = a.pos, read_pos = 0;
  for (uint32_t c : a.cigar) {
    const int l = (int)(c >> 4), op = (int)(c & 0xf);
    if (op == 0 || op == 7 || op == 8) {
      for (int i = 0; i < l; ++i) res.emplace_back(read_pos + i, ref_pos + i);
      read_pos += l; ref_pos += l;
    } else if (op == 1 || op == 4) {
      for (int i = 0; i < l; ++i) res.emplace_back(read_pos + i, -1);
      read_pos += l;
    } else if (op == 2 || op == 3) {
      for (int i = 0; i < l; ++i) res.emplace_back(-1, ref_pos + i);
      ref_pos += l;
    }
  }
  return res;
}

// clusterer.cpp:351-405
std::pair<int, int> get_unique_kmers(const Pairs& al, size_t k, bool from_end, const std::string& cseq) {
  if (al.size() < k) return {-1, -1};
  std::map<std::string, int> kmers;
  size_t i = 0;
  while (i < al.size() - k + 1) {
    bool skip = false;
    for (size_t j = i; j < i + k; ++j)
      if (al[j].first == -1 || al[j].second == -1) { skip = true; i = j + 1; break; }
    if (skip) continue;
    ++kmers[cseq.substr((size_t)al[i].second, k)];
    ++i;
  }
  std::pair<int, int> last(-1, -1);
  i = 0;
  while (i < al.size() - k + 1) {
    size_t offset = from_end ? al.size() - k - i : i;
    bool skip = false;
    for (size_t j = offset; j < offset + k; ++j)
      if (al[j].first == -1 || al[j].second == -1) { skip = true; i += (j - offset); break; }
    if (skip) { ++i; continue; }
    last = al[offset];
    if (kmers[cseq.substr((size_t)al[offset].second, k)] == 1) break;
    ++i;
  }
  return last;
}

struct Ctx {
  CallOptions o;
  std::vector<std::string> chrom_names;
  std::unordered_map<std::string, std::string> chrom_seqs;
  std::unordered_map<std::string, std::vector<RawSFS>> sfs;
  // statistics (bumped from the worker threads of pass 1)
  std::atomic<long> unplaced{0}, s_unplaced{0}, e_unplaced{0}, unknown{0}, unextended{0}, small{0}, small2{0};
};

// a soft clip next to SFS that could not be placed on one side (clipper.hpp:21-42)
struct Clip {
  std::string name, chrom;
  unsigned p = 0, l = 0;
  bool starting = false;   // leading clip (the read continues to the right of p)
  unsigned w = 0;
};

// clusterer.cpp:159-346; clips: --clipped bookkeeping (:207-226, :338-345), nullptr without the option
void extend_alignment(Ctx& C, const BamRecord& aln, const std::string& chrom, std::vector<ESFS>& out,
                      std::vector<Clip>* clips = nullptr) {
  auto cs = C.chrom_seqs.find(chrom);
  if (cs == C.chrom_seqs.end()) return;
  const std::string& cseq = cs->second;
  const Pairs al = get_aligned_pairs(aln);
  const int k = 7, flank = 100;   // config.hpp:89-90, not settable
  size_t last_pos = 0;
  std::vector<ESFS> local;
  unsigned lclip_p = 0, lclip_l = 0, rclip_p = 0, rclip_l = 0;
  for (const RawSFS& sfs : C.sfs.at(aln.qname)) {
    const int s = sfs.qs, e = sfs.qs + sfs.l - 1;
    int aln_start = -1, aln_end = -1, refs = -1, refe = -1;
    for (size_t i = last_pos; i < al.size(); ++i) {
      const int q = al[i].first, r = al[i].second;
      if (q == -1 || r == -1) continue;
      else if (q < s) { last_pos = i; refs = r; aln_start = (int)i; }
      else if (q > e) { refe = r; aln_end = (int)i; break; }
    }
    if (refs == -1 && refe == -1) { ++C.unplaced; continue; }
    else if (refs == -1) {
      // the SFS starts in front of the first placed base: with --clipped a leading soft clip is remembered instead of
      // counting the SFS (every such SFS of the alignment sets the same pair)
      const uint32_t c0 = aln.cigar.empty() ? 0u : aln.cigar.front();
      if (clips && (c0 & 0xf) == 4) { lclip_p = (unsigned)aln.pos; lclip_l = c0 >> 4; }
      else ++C.s_unplaced;
      continue;
    } else if (refe == -1) {
      const uint32_t c1 = aln.cigar.empty() ? 0u : aln.cigar.back();
      if (clips && (c1 & 0xf) == 4) { rclip_p = (unsigned)aln.endpos(); rclip_l = c1 >> 4; }
      else ++C.e_unplaced;
      continue;
    }
    Pairs loc;
    int last_r = refs - 1;
    for (int i = aln_start; i <= aln_end; ++i) {
      const int q = al[(size_t)i].first, r = al[(size_t)i].second;
      if (r == -1) { if (refs <= last_r && last_r <= refe) loc.emplace_back(q, r); }
      else { last_r = r; if (refs <= r && r <= refe) loc.emplace_back(q, r); }
      if (q != -1 && r != -1 && r >= refe) break;
    }
    Pairs pre, post;
    for (int i = aln_start - 1; i >= 0; --i) { pre.push_back(al[(size_t)i]); if ((int)pre.size() == flank) break; }
    std::reverse(pre.begin(), pre.end());
    for (size_t i = (size_t)aln_end + 1; i < al.size(); ++i) { post.push_back(al[i]); if ((int)post.size() == flank) break; }
    std::pair<int, int> prek = get_unique_kmers(pre, (size_t)k, true, cseq);
    std::pair<int, int> postk = get_unique_kmers(post, (size_t)k, false, cseq);
    if (prek.first == -1 || prek.second == -1) prek = loc.front();
    if (postk.first == -1 || postk.second == -1) postk = loc.back();
    if (prek.first == -1 || prek.second == -1 || postk.first == -1 || postk.second == -1) { ++C.unknown; continue; }
    if ((unsigned)prek.second > (unsigned)(postk.second + k)) continue;   // warning only (:301-303)
    local.push_back(ESFS{chrom, aln.qname, prek.second, postk.second + k, prek.first, postk.first + k, sfs.htag});
  }
  std::vector<ESFS> merged;   // :314-336
  for (const ESFS& x : local) {
    size_t j;
    for (j = 0; j < merged.size(); ++j)
      if ((x.rs <= merged[j].rs && merged[j].rs <= x.re) || (merged[j].rs <= x.rs && x.rs <= merged[j].re)) break;
    if (j < merged.size()) {
      merged[j].rs = std::min(merged[j].rs, x.rs); merged[j].re = std::max(merged[j].re, x.re);
      merged[j].qs = std::min(merged[j].qs, x.qs); merged[j].qe = std::max(merged[j].qe, x.qe);
    } else merged.push_back(x);
  }
  out.insert(out.end(), merged.begin(), merged.end());
  if (clips) {   // clusterer.cpp:338-345
    if (lclip_l > 0) clips->push_back(Clip{aln.qname, chrom, lclip_p, lclip_l, true, 0});
    if (rclip_l > 0) clips->push_back(Clip{aln.qname, chrom, rclip_p, rclip_l, false, 0});
  }
}

float len_ratio(float cl, float sl) { return std::min(cl, sl) / std::max(cl, sl); }

// caller.cpp:78-97
std::vector<Cluster> split_by_len(const Cluster& c, float min_ratio) {
  std::vector<Cluster> subs;
  for (const SubRead& sr : c.subreads) {
    size_t i;
    for (i = 0; i < subs.size(); ++i)
      if (len_ratio((float)subs[i].get_len(), (float)(unsigned)sr.seq.size()) >= min_ratio) break;
    if (i == subs.size()) subs.push_back(c.cleared_copy());
    subs[i].subreads.push_back(sr);
  }
  return subs;
}

int largest(const std::vector<Cluster>& v) {
  unsigned vmax = 0; int imax = -1;
  for (size_t i = 0; i < v.size(); ++i) if (v[i].size() > vmax) { vmax = (unsigned)v[i].size(); imax = (int)i; }
  return imax;
}

// caller.cpp:100-255 (int-typed best_ratio included)
std::vector<Cluster> split_cluster(const Cluster& cluster, bool useht, float min_ratio) {
  Cluster c0 = cluster.cleared_copy(), c1 = cluster.cleared_copy(), c2 = cluster.cleared_copy();
  for (const SubRead& sr : cluster.subreads) {
    if (useht && sr.htag == 1) c1.subreads.push_back(sr);
    else if (useht && sr.htag == 2) c2.subreads.push_back(sr);
    else c0.subreads.push_back(sr);
  }
  c0.cov1 = c0.cov2 = -1; c1.cov0 = c1.cov2 = -1; c2.cov0 = c2.cov1 = -1;
  std::vector<Cluster> out;
  if (c1.size() == 0 && c2.size() == 0) {
    std::vector<Cluster> subs = split_by_len(c0, min_ratio);
    int i1 = -1, i2 = -1; unsigned v1 = 0, v2 = 0;
    for (unsigned i = 0; i < subs.size(); ++i) {
      if (subs[i].size() > v1) { v2 = v1; i2 = i1; v1 = (unsigned)subs[i].size(); i1 = (int)i; }
      else if (subs[i].size() > v2) { v2 = (unsigned)subs[i].size(); i2 = (int)i; }
    }
    if (i1 != -1) out.push_back(subs[(size_t)i1]);
    if (i2 != -1) out.push_back(subs[(size_t)i2]);
    return out;
  }
  const int both = (c1.size() > 0 ? 1 : 0) + (c2.size() > 0 ? 2 : 0);
  std::vector<Cluster> s1 = split_by_len(c1, min_ratio), s2 = split_by_len(c2, min_ratio);
  Cluster nc(cluster.chrom, cluster.s, cluster.e, cluster.cov, cluster.cov0, -1, -1);
  for (const SubRead& sr : c0.subreads) {
    const float sl = (float)(unsigned)sr.seq.size();
    int best_1 = -1, best_ratio_1 = -1, best_2 = -1, best_ratio_2 = -1;
    for (unsigned i = 0; i < s1.size(); ++i) {
      const float r = len_ratio((float)s1[i].get_len(), sl);
      if (r >= min_ratio && r > best_ratio_1) { best_1 = (int)i; best_ratio_1 = (int)r; }
    }
    for (unsigned i = 0; i < s2.size(); ++i) {
      const float r = len_ratio((float)s2[i].get_len(), sl);
      if (r >= min_ratio && r > best_ratio_2) { best_2 = (int)i; best_ratio_2 = (int)r; }
    }
    if (both == 1) {
      if (best_1 == -1) nc.subreads.push_back(sr);
      else { s1[(size_t)best_1].subreads.push_back(sr); ++s1[(size_t)best_1].cov1; --nc.cov0; }
    } else if (both == 2) {
      if (best_2 == -1) nc.subreads.push_back(sr);
      else { s2[(size_t)best_2].subreads.push_back(sr); ++s2[(size_t)best_2].cov2; --nc.cov0; }
    } else {
      if (best_1 != -1 && best_ratio_1 > best_ratio_2) { s1[(size_t)best_1].subreads.push_back(sr); ++s1[(size_t)best_1].cov1; --nc.cov0; }
      else if (best_2 != -1 && best_ratio_2 > best_ratio_1) { s2[(size_t)best_2].subreads.push_back(sr); ++s2[(size_t)best_2].cov2; --nc.cov0; }
    }
  }
  int i = largest(s1);
  if (i != -1) out.push_back(s1[(size_t)i]);
  i = largest(s2);
  if (i != -1) out.push_back(s2[(size_t)i]);
  if (both != 3 && nc.size() > 0) {
    std::vector<Cluster> ns = split_by_len(nc, min_ratio);
    i = largest(ns);
    if (i != -1) {
      if (both == 1) ns[(size_t)i].cov1 = -1; else ns[(size_t)i].cov2 = -1;
      out.push_back(ns[(size_t)i]);
    }
  }
  return out;
}

// ---- imprecise SVs from soft clips (--clipped; Clipper, clipper.cpp) -------------------------------------------
//
// What the reference computes, stage by stage, with its quirks kept where they are defined behaviour:
//   * a side's clips (leading / trailing) -> first clip per read name (:5-15) -> one breakpoint per (chromosome,
//     position) with the longest clip and the number of reads (:17-52), listed chromosome slot by slot (i % 4, the
//     slots concatenated back to front) and inside a chromosome in the iteration order of a
//     std::unordered_map<uint, ...> filled in list order -- the same container here, hence the same order as a
//     reference built against libstdc++;
//   * breakpoints seen by fewer than two reads are dropped (:54-63), so are those within the +-1,000 bp window of
//     a called SV of ANY chromosome (the interval tree has no chromosome, caller.cpp:39-41, clipper.cpp:93-102);
//   * greedy grouping in list order (:66-91): a breakpoint within 1,000 bp of existing centres adds its reads to
//     ALL of them, otherwise it becomes a centre; `centre - 1000` is unsigned arithmetic, so a centre below 1,000
//     never absorbs anything (and is overwritten by a breakpoint at its own position);
//   * insertions (:170-194): every leading centre looks up a trailing centre with the search of :104-124 and calls
//     <INS> when the two are less than 1,000 bp apart; deletions (:196-214): every trailing centre looks up a leading
//     one 2,000 to 50,000 bp to its right, at least five reads; positions of different chromosomes are compared as
//     plain numbers;
//   * rows leave per OpenMP slot (i % threads; insertions before deletions), the slots back to front (caller.cpp:45-50).
// Where the reference is undefined this code is defined: the search of :104-124 walks off the
// array when the query lies left of every centre of the other side (`m - 1` on an unsigned 0: it reads two billion
// entries past the list) -- here it returns what its comment says it looks for, the first centre right of the query; the
// record's COV0 / COV1 / COV2 / GQ are printed from fields nothing ever set (sv.cpp:5-27) -- 0 here; a reference base
// beyond the chromosome's end (positions of two chromosomes mixed) is 'N'.
namespace clipper {

std::vector<Clip> breakpoints(const std::vector<Clip>& side, const std::vector<std::string>& chromosomes,
                              const std::vector<std::pair<int, int>>& called) {
  std::vector<const Clip*> first;
  {
    std::set<std::string> seen;
    for (const Clip& c : side)
      if (seen.insert(c.name).second) first.push_back(&c);
  }
  std::unordered_map<std::string, std::unordered_map<unsigned, std::vector<const Clip*>>> at;
  for (const Clip* c : first) at[c->chrom][c->p].push_back(c);
  std::vector<Clip> slot[4];
  for (size_t i = 0; i < chromosomes.size(); ++i) {
    const auto chrom = at.find(chromosomes[i]);
    if (chrom == at.end()) continue;
    for (const auto& bp : chrom->second) {
      Clip b;
      b.chrom = chromosomes[i];
      b.p = bp.first;
      for (const Clip* c : bp.second) b.l = std::max(b.l, c->l);
      b.starting = bp.second.front()->starting;
      b.w = (unsigned)bp.second.size();
      slot[i % 4].push_back(b);
    }
  }
  std::map<unsigned, Clip> centres;
  for (int k = 3; k >= 0; --k)
    for (const Clip& b : slot[k]) {
      if (b.w < 2) continue;
      bool near_call = false;
      for (const auto& iv : called)
        if (iv.first <= (int)b.p + 1 && (int)b.p <= iv.second) { near_call = true; break; }
      if (near_call) continue;
      bool absorbed = false;
      for (auto& kv : centres)
        if (kv.first - 1000u <= b.p && b.p <= kv.first + 1000u) {
          absorbed = true;
          kv.second.l = std::max(kv.second.l, b.l);
          kv.second.w += b.w;
        }
      if (!absorbed) centres[b.p] = b;
    }
  std::vector<Clip> out;
  for (const auto& kv : centres) out.push_back(kv.second);
  return out;   // ascending position (std::map), what the sort of :151,158 leaves
}

// clipper.cpp:104-124 on a list sorted by position: the entry after one at the query's position (that entry itself
// when it is the last), else the first entry to the right of the query whose left neighbour lies left of it; -1
// when there is none; a query left of every entry gets entry 0 (the reference's recursion leaves the array there)
int partner(const std::vector<Clip>& v, unsigned q) {
  if (v.empty()) return -1;
  size_t lo = 0, hi = v.size() - 1;
  for (;;) {
    if (lo > hi || lo >= v.size()) return -1;
    const size_t m = (lo + hi) / 2;
    if (v[m].p == q) return (int)(m + 1 < v.size() ? m + 1 : m);
    if (v[m].p > q) {
      if (m > 0 && v[m - 1].p < q) return (int)m;
      if (m == 0) return 0;               // (the reference goes on with end = UINT_MAX)
      hi = m - 1;
    } else lo = m + 1;
  }
}

}  // namespace clipper

// Clipper::call + the caller's collection (clipper.cpp:126-215, caller.cpp:36-53): rows in output order
std::vector<SV> call_clipped(const std::vector<Clip>& clips, const std::vector<std::string>& chromosomes,
                             const std::unordered_map<std::string, std::string>& chrom_seqs, int T,
                             const std::vector<std::pair<int, int>>& called) {
  std::vector<Clip> lead, trail;
  for (const Clip& c : clips) (c.starting ? lead : trail).push_back(c);
  const std::vector<Clip> rc = clipper::breakpoints(trail, chromosomes, called);
  const std::vector<Clip> lc = clipper::breakpoints(lead, chromosomes, called);
  std::vector<std::vector<SV>> per_slot((size_t)T);
  if (!lc.empty() && !rc.empty()) {
    auto base_at = [&](const std::string& chrom, unsigned p) {
      const auto it = chrom_seqs.find(chrom);
      return std::string(1, it != chrom_seqs.end() && p < it->second.size() ? it->second[p] : 'N');
    };
    for (size_t i = 0; i < lc.size(); ++i) {
      const Clip& l = lc[i];
      const int k = clipper::partner(rc, l.p);
      if (k < 0) continue;
      const Clip& r = rc[(size_t)k];
      if (r.w == 0) continue;
      if (std::abs((int)r.p - (int)l.p) < 1000) {
        const unsigned s = l.w > r.w ? l.p : r.p;
        SV v = make_sv("INS", l.chrom, (int)s, base_at(l.chrom, s), "<INS>", std::max(l.w, r.w), 0, 0, 0,
                       (int)std::max(l.l, r.l), ".");
        v.imprecise = true;
        per_slot[i % (size_t)T].push_back(v);
      }
    }
    for (size_t i = 0; i < rc.size(); ++i) {
      const Clip& r = rc[i];
      const int k = clipper::partner(lc, r.p);
      if (k < 0) continue;
      const Clip& l = lc[(size_t)k];
      if (l.w == 0) continue;
      const unsigned gap = l.p - r.p;     // (unsigned: a leading centre left of the trailing one is out of range)
      if (gap >= 2000 && gap <= 50000 && std::max(l.w, r.w) >= 5) {
        SV v = make_sv("DEL", r.chrom, (int)r.p, base_at(r.chrom, r.p), "<DEL>", std::max(l.w, r.w), 0, 0, 0,
                       (int)(gap + 1), ".");
        v.imprecise = true;
        per_slot[i % (size_t)T].push_back(v);
      }
    }
  }
  std::vector<SV> rows;
  for (size_t t = (size_t)T; t-- > 0;) rows.insert(rows.end(), per_slot[t].begin(), per_slot[t].end());
  return rows;
}

const char* VCF_INFO[][4] = {
    {"VARTYPE", "A", "String", "Variant class"}, {"SVTYPE", "1", "String", "Variant type"},
    {"SVLEN", "1", "Integer", "Difference in length between REF and ALT alleles"},
    {"END", "1", "Integer", "End position of the variant described in this record"},
    {"WEIGHT", "1", "Integer", "Number of alignments supporting this record"},
    {"COV", "1", "Integer", "Total number of alignments covering this locus"},
    {"COV0", "1", "Integer", "Total number of alignments covering this locus (no HP)"},
    {"COV1", "1", "Integer", "Total number of alignments covering this locus (HP=1)"},
    {"COV2", "1", "Integer", "Total number of alignments covering this locus (HP=2)"},
    {"AS", "1", "Integer", "Alignment score"}, {"NV", "1", "Integer", "Number of variations on same consensus"},
    {"IMPRECISE", "0", "Flag", "Imprecise structural variation"}, {"CIGAR", "A", "String", "CIGAR of consensus"},
    {"READS", ".", "String", "Reads identifiers supporting the call"},
    {"RVEC", ".", "String", "Reads vector used by genotyper"}};

uint8_t enc26(char c) {   // caller.hpp:25-37
  switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
               case 'T': case 't': return 3; default: return 4; }
}

}  // namespace

namespace {

// One pass over the BAM, record after record in file order: the records the device path keeps (sel; its filters, one per
// region of the file, decide which), every record of the host reader (bam), or -- `SVDSS run`, whose smoothing stage has
// left every record `call` looks at in HBM -- the records filters[0] keeps of a filled record store, stored batch after
// stored batch (store).  next: 1 = record, 0 = end of the file, -1 = error (err says which).
struct RecordFeed {
  std::unique_ptr<ShardedBamSelect<SelectedBatch>> sel;
  std::vector<svdss_bam_filter_t*> filters;
  svdss_bam_store_t* store = nullptr;
  int64_t store_batches = 0, store_at = 0;
  svdss_bam_batch_t* store_obj = nullptr;
  std::unique_ptr<BamReader> bam;
  // host reader: called with every chunk it inflates, before the first record of the chunk is handed out (the record
  // views point into it)
  std::function<void(const std::shared_ptr<BamReader::Bytes>&)> on_chunk;
  uint64_t seen_chunk = ~0ull;
  // device path: called with every batch as it is taken from the reader, in file order (--write-bam-index folds its fragments)
  std::function<void(const SelectedBatch&)> on_batch;
  // device path: the batch being handed out; what pass 1's log sums over the batches
  std::unique_ptr<SelectedBatch> cur;
  size_t k = 0;
  uint64_t n_batches = 0, n_records = 0;
  double stage_s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wait_s = 0;
  std::string err;

  ~RecordFeed() {
    sel.reset();   // (its threads use the filters)
    if (store_obj) svdss_bam_batch_free(store_obj);
    for (svdss_bam_filter_t* f : filters) svdss_bam_filter_free(f);
  }

  // the next stored batch's selection (svdss_bam_store_select: slim records, file order); null at the end or on error
  std::unique_ptr<SelectedBatch> next_from_store() {
    if (store_at >= store_batches) return nullptr;
    const int rc = svdss_bam_store_select(store, store_at++, filters[0], &store_obj);
    if (rc != SVDSS_OK) { err = std::string("record store: ") + svdss_strerror(rc) + " " + svdss_last_hip_error(); return nullptr; }
    svdss_bam_selection_t r;
    (void)svdss_bam_batch_selection(store_obj, &r);
    std::unique_ptr<SelectedBatch> out(new SelectedBatch);
    out->bytes.assign(r.bytes, r.bytes + r.n_bytes);
    out->off.assign(r.rec_off, r.rec_off + r.n_selected + 1);
    out->n_records = (uint64_t)r.n_records;
    out->slim = true;
    for (int s = 0; s < 8; ++s) out->stage_s[s] = r.stage_ms[s] * 1e-3;
    return out;
  }

  int next(BamReader::RawView& rr) {
    if (bam) {
      const int rc = bam->next_view(rr);
      if (rc < 0) err = bam->error();
      if (rc > 0 && on_chunk && bam->chunk_id() != seen_chunk) { seen_chunk = bam->chunk_id(); on_chunk(bam->chunk()); }
      return rc;
    }
    while (!cur || k + 1 >= cur->off.size()) {
      const auto tw0 = std::chrono::steady_clock::now();
      cur = store ? next_from_store() : sel->next();
      wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count();
      k = 0;
      if (!cur) { if (sel) err = sel->error(); return err.empty() ? 0 : -1; }
      if (on_batch) on_batch(*cur);
      n_records += cur->n_records;
      for (int s = 0; s < 8; ++s) stage_s[s] += cur->stage_s[s];
      stage_s[7] += cur->inflate_kernel_s; ++n_batches;
    }
    const size_t at = (size_t)cur->off[k], end = (size_t)cur->off[k + 1];
    ++k;
    if (!view_of_record(cur->bytes.data() + at, end - at, rr, cur->slim)) { err = "corrupt record"; return -1; }
    return 1;
  }
};

// what one alignment does to one cluster it overlaps (pass 2); applied in BAM order
struct Ev { size_t ci; int hp; bool in_reads, unext; std::string name, sub; };

// The clusters as pass 2 (Clusterer::fill_clusters, clusterer.cpp:477-610) looks them up, built once: per cluster the
// names of its reads and its region; the clusters with enough reads per chromosome, sorted by region start, with the
// running maximum of their ends; and their regions merged per chromosome -- what the record store's filter, the index
// query and the device path's filter all take.
struct ClusterRegions {
  const size_t n_ref;
  const unsigned min_mapq;
  std::vector<std::set<std::string>> reads;
  std::vector<int> min_s, max_e;
  std::vector<char> live;
  long n_small = 0;                                      // clusters with too few reads
  std::map<std::string, std::vector<size_t>> by_chrom;   // cluster indices per chrom, sorted by region start
  std::map<std::string, std::vector<int>> run_max_end;   // per chrom: running maximum of the region ends, same order
  // per reference id: the clusters of that chromosome (sorted by start) and the running maximum of their ends
  std::vector<const std::vector<size_t>*> tid_clusters;
  std::vector<const std::vector<int>*> tid_run_max;
  std::vector<int32_t> rt, rb, re;                       // the merged regions: reference id, [begin, end)

  // (the clusters with enough reads get their region as coordinates)
  ClusterRegions(std::vector<Cluster>& clusters, const std::vector<std::string>& ref_names, unsigned min_weight, unsigned mapq)
      : n_ref(ref_names.size()), min_mapq(mapq), reads(clusters.size()), min_s(clusters.size()), max_e(clusters.size()),
        live(clusters.size(), 0), tid_clusters(n_ref, nullptr), tid_run_max(n_ref, nullptr) {
    for (size_t i = 0; i < clusters.size(); ++i) {
      int mn = std::numeric_limits<int>::max(), mx = 0;
      for (const ESFS& s : clusters[i].sfss) { mn = std::min(mn, s.rs); mx = std::max(mx, s.re); reads[i].insert(s.qname); }
      min_s[i] = mn; max_e[i] = mx;
      if (reads[i].size() < (size_t)min_weight) { ++n_small; continue; }
      clusters[i].s = mn; clusters[i].e = mx;
      live[i] = 1;
      by_chrom[clusters[i].chrom].push_back(i);
    }
    for (auto& kv : by_chrom) {
      std::sort(kv.second.begin(), kv.second.end(), [&](size_t a, size_t b) { return min_s[a] < min_s[b]; });
      std::vector<int>& rm = run_max_end[kv.first];
      int m = 0;
      for (size_t ci : kv.second) { m = std::max(m, max_e[ci]); rm.push_back(m); }
    }
    for (size_t t = 0; t < n_ref; ++t) {
      auto it = by_chrom.find(ref_names[t]);
      if (it == by_chrom.end()) continue;
      tid_clusters[t] = &it->second;
      tid_run_max[t] = &run_max_end[it->first];
      for (size_t ci : it->second) {   // (by start: a region overlaps the last one of the chromosome or starts a new one)
        if (!rt.empty() && rt.back() == (int32_t)t && beg0(ci) <= re.back()) re.back() = std::max(re.back(), max_e[ci]);
        else { rt.push_back((int32_t)t); rb.push_back(beg0(ci)); re.push_back(max_e[ci]); }
      }
    }
  }

  // region "chrom:min_s-max_e" = 0-based half-open [min_s-1, max_e)
  int beg0(size_t ci) const { return std::max(min_s[ci] - 1, 0); }

  // the merged regions as the device path's record filter, on GPU dev
  svdss_bam_filter_t* filter(int32_t dev) const {
    svdss_bam_filter_t* f = nullptr;
    check(svdss_bam_filter_create(dev, (int32_t)std::min<unsigned>(min_mapq, 256u), (int32_t)n_ref, nullptr, nullptr, 0, rt.data(), rb.data(),
                                  re.data(), (int64_t)rt.size(), &f), "svdss_bam_filter_create");
    return f;
  }

  // What one alignment does to the clusters it overlaps, handed to sink as one Ev per cluster.  Records stay in their raw
  // form: the end position and the two query positions the reference reads off the aligned-pairs vector (bam.cpp:92-134,
  // clusterer.cpp:555-580) are functions of the CIGAR blocks alone, and only the bases of the extracted sub-read are decoded.
  template <class Sink>
  void process(const BamReader::RawView& rr, std::string& qname, Sink&& sink) const {
    static const char NT16[] = "=ACMGRSVTWYHKDBN";
    if (rr.tid < 0 || rr.tid >= (int)n_ref || !tid_clusters[(size_t)rr.tid]) return;
    if (rr.flag & (4 | 2048 | 256)) return;        // clusterer.cpp:535-540: such a record touches no cluster
    if ((unsigned)rr.mapq < min_mapq) return;
    const uint8_t* cg = rr.name() + rr.l_name;
    auto cig = [&](uint32_t i) { uint32_t c; memcpy(&c, cg + 4u * i, 4); return c; };
    int32_t ref_len = 0;
    for (uint32_t i = 0; i < rr.n_cigar; ++i) {
      const uint32_t c = cig(i), op = c & 0xf;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += (int32_t)(c >> 4);
    }
    const int a_beg = rr.pos, a_end = rr.pos + (ref_len ? ref_len : 1);   // bam_endpos
    const std::vector<size_t>& cl_ids = *tid_clusters[(size_t)rr.tid];
    // clusters before `first` end at or before the alignment's start: none of them can overlap it
    const std::vector<int>& rm = *tid_run_max[(size_t)rr.tid];
    const size_t first = (size_t)(std::upper_bound(rm.begin(), rm.end(), a_beg) - rm.begin());
    bool have_tags = false;
    int64_t hp = 0;
    for (size_t k = first; k < cl_ids.size(); ++k) {
      const size_t ci = cl_ids[k];
      const int b0 = beg0(ci), end0 = max_e[ci];
      if (b0 >= a_end) break;   // clusters are sorted by start
      if (!(a_beg < end0 && a_end > b0)) continue;
      if (!have_tags) {
        have_tags = true;
        BamReader::aux_int(rr.aux(), rr.l_aux, "HP", hp);
        qname.assign((const char*)rr.name(), rr.l_name ? rr.l_name - 1 : 0);
      }
      Ev ev{ci, (int)hp, false, false, std::string(), std::string()};
      if (reads[ci].find(qname) == reads[ci].end()) { sink(ev); continue; }
      ev.in_reads = true;
      // qs: query position of the last aligned (M/=/X) pair with reference position <= min_s;
      // qe: of the first one with reference position >= max_e
      int qs = -1, qe = -1, ref_pos = rr.pos, read_pos = 0;
      for (uint32_t i = 0; i < rr.n_cigar; ++i) {
        const uint32_t c = cig(i), op = c & 0xf;
        const int l = (int)(c >> 4);
        if (op == 0 || op == 7 || op == 8) {
          if (l > 0) {
            if (ref_pos <= min_s[ci]) qs = read_pos + (std::min(min_s[ci], ref_pos + l - 1) - ref_pos);
            if (qe == -1 && ref_pos + l - 1 >= max_e[ci]) qe = read_pos + (std::max(max_e[ci], ref_pos) - ref_pos);
          }
          read_pos += l; ref_pos += l;
        } else if (op == 1 || op == 4) read_pos += l;
        else if (op == 2 || op == 3) ref_pos += l;
      }
      if (qs == -1 || qe == -1) ev.unext = true;
      else {
        if (qs > rr.l_seq) die("corrupt alignment: sub-read start past the end of read " + qname);   // (std::string::substr throws in the reference)
        const int n = std::max(0, std::min(qe - qs + 1, rr.l_seq - qs));
        const uint8_t* sq = rr.seq4();
        std::string sub((size_t)n, 'N');
        for (int i = 0; i < n; ++i) { const int q = qs + i; sub[(size_t)i] = NT16[(sq[q >> 1] >> ((~q & 1) << 2)) & 0xf]; }
        ev.name = qname;
        ev.sub = std::move(sub);
      }
      sink(ev);
    }
  }
};

// Pass 2 over n_units units of consecutive records (in file order) on n_threads threads: unit(state, k, sink) hands what
// the records of unit k do to the clusters to sink and returns "" or what went wrong (the run then ends with `fail` and
// the first error in unit order); `state` belongs to the thread, and goes when the thread is done.  The events come back
// per unit: applied unit after unit, they are in the order of the single scan.
template <class State, class Unit>
std::vector<std::vector<Ev>> scan_units(size_t n_units, size_t n_threads, const std::string& fail, Unit&& unit) {
  std::vector<std::vector<Ev>> evs(n_units);
  std::vector<std::string> errs(n_units);
  std::atomic<size_t> next(0);
  auto work = [&]() {
    State state;
    for (size_t k; (k = next.fetch_add(1)) < n_units;) {
      auto sink = [&evs, k](Ev& e) { evs[k].push_back(std::move(e)); };
      errs[k] = unit(state, k, sink);
    }
  };
  std::vector<std::thread> pool;
  for (size_t w = 1; w < n_threads; ++w) pool.emplace_back(work);
  work();
  for (std::thread& th : pool) th.join();
  for (const std::string& e : errs)
    if (!e.empty()) die(fail + e);
  return evs;
}

// `SVDSS call`, stage by stage in the order of Caller::run / Clusterer::run (caller.cpp:12-57, clusterer.cpp:12-54); the
// members are what one stage hands to the next.
struct CallRun {
  const CallOptions& o;
  const CallKnobs knobs{};               // every SVDSS_* variable this file reads (host_knobs.h)
  Ctx C;
  const int T;
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  std::vector<std::string> ref_names;    // BAM header order
  std::vector<ESFS> extended;            // pass 1: every placed SFS
  std::vector<Clip> clips;               // --clipped
  std::thread fasta_loader;              // load_chromosomes, beside the SFS file and the start of pass 1
  RefOnDevice ref_dev;                   // where the GPU read the FASTA (ref_loader.h): its output, kept in HBM until the BAM header's order is known
  // ONE pass over the BAM (round 6): what pass 2 needs of every record stays in HBM while pass 1 runs (svdss_bam_store_t)
  // (--gpus N: the file's regions, one per GPU, each with a store of its own in that GPU's HBM -- and a small one for the
  // records of the seam in front of it; ShardedBamSelect, bam_device_select.h)
  std::vector<svdss_bam_store_t*> stores, seam_stores;
  std::vector<size_t> bam_cuts;            // where the regions begin (plan_bam_regions); one region: {0, file size}
  std::vector<int64_t> region_batches;     // after pass 1: batches per region, and whether a seam batch precedes it
  std::vector<char> region_seam;
  int32_t n_ref_hdr = 0;
  std::thread store_alloc;
  double store_alloc_s = 0;
  void reference_ready() { if (fasta_loader.joinable()) fasta_loader.join(); }
  bool dev_pass = false;                 // the BAM is read through the device path (csrc/bam_device.hip): no record cache
  int64_t bam_skip = 0;                  // the BAM header's length in the inflated stream
  // host threads that scan the file chunks an index names for pass 2 (SVDSS_CALL_PASS2_THREADS; 1: the single scan)
  size_t pass2_threads(size_t n_chunks) const {
    const size_t want = knobs.pass2_threads ? (size_t)knobs.pass2_threads : std::min<size_t>((size_t)effective_cpus(), 32);
    return std::max<size_t>(1, std::min(want, n_chunks / 4 + 1));
  }
  std::vector<BamReader::RawView> cache_views;   // the record cache of the host reader (align_and_extend)
  std::vector<std::shared_ptr<BamReader::Bytes>> cache_chunks;
  size_t cache_bytes = 0, cache_limit = 0;
  bool cache_ok = true;
  std::thread cache_release;
  std::vector<Cluster> clusters;
  int n_dev = 1, G = 1;                  // GPUs present / GPUs in use (--gpus): regions of the file, shards of the DP batches
  struct Sub { size_t parent; Cluster cl; };
  std::vector<Sub> subs;                 // sub-clusters after split_cluster, in the reference's order
  std::vector<std::string> consensus;    // one per sub-cluster
  std::vector<SV> svs;
  std::vector<std::vector<std::string>> sam_rows;   // per reference thread, --poa only

  // `SVDSS run` (run_host.cpp): the SFS text in memory, the filled record store, the chromosomes -- what the smoothing and
  // search stages of the same process left (null: `SVDSS call`)
  CallPreset* const preset;
  bool from_store() const { return preset && preset->store; }
  // `SVDSS run --samples`: the process goes on to the next sample -- chromosomes and their copy in HBM go back to the hooks,
  // the record stores are freed
  SmoothHooks* session() const { return preset && preset->from_smooth && preset->from_smooth->session ? preset->from_smooth : nullptr; }

  explicit CallRun(const CallOptions& opt, CallPreset* p = nullptr) : o(opt), T(std::max(1, opt.threads)), preset(p) { C.o = opt; }

  void stage(const char* what) {   // --verbose: seconds since the previous stage mark
    if (!o.verbose) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[call] [time] %-28s %.3f s\n", what, std::chrono::duration<double>(now - t_last).count());
    t_last = now;
  }

  // load_chromosomes + parse_sfsfile (chromosomes.cpp:9-27, sfs.cpp:5-30)
  void load_inputs() {
    // ---- load_chromosomes (chromosomes.cpp:9-27): upper-cased, FASTA order.  On a thread of its own: the SFS file is
    // parsed and pass 1 starts reading the BAM beside it; the first use of the chromosomes waits (reference_ready)
    if (preset && preset->from_smooth) {   // (read once, by the smoothing stage)
      C.chrom_names = std::move(preset->from_smooth->chrom_names);
      C.chrom_seqs = std::move(preset->from_smooth->chrom_seqs);
    } else {
      if (FILE* f = fopen(o.reference.c_str(), "rb")) fclose(f); else die("cannot open " + o.reference);
      fasta_loader = std::thread([this] {
        if (!load_chromosomes(o.reference, T, knobs.fasta_serial, o.verbose, "call", C.chrom_names, C.chrom_seqs, &ref_dev)) die("cannot open " + o.reference);
      });
    }
    // the record store(s) of the ONE pass over the BAM (round 6, align_and_extend / fill_clusters below): the memory is taken
    // NOW, on a thread of its own, beside the FASTA and the SFS file -- tens of GB that the driver clears before it hands them out
    {
      // (effective_gpus: oversubscribed, more shards than GPUs, shard g on GPU g % count -- exercises the sharding on a one-GPU box)
      n_dev = std::max(1, svdss_device_count());
      G = effective_gpus(o.gpus);
      // Records handled on the GPU (csrc/bam_device.hip, svdss_bam_select_run; the default when there is a GPU and the
      // input is a regular file): only the primary, mapq-ok alignments of reads that HAVE SFS come back to the host --
      // the records clusterer.cpp:108-145 keeps -- instead of every inflated byte.  No record cache then: pass 2 takes the
      // records kept in HBM, goes through the BAI index, or reads the file again through the same path with the cluster
      // regions as the filter.  SVDSS_BAM_DEVICE=0: the host reader (chunks inflated on the GPU or the host, records sliced here).
      dev_pass = svdss_device_count() > 0 && knobs.bam_device;
      if (dev_pass) {
        std::string herr;
        if (!bam_header_probe(o.bam, n_ref_hdr, bam_skip, herr, &ref_names)) die("cannot read " + o.bam + ": " + herr);
        bam_cuts = plan_bam_regions(o.bam, G, bam_skip);
      }
      if (from_store()) {   // (filled already: one region, no seam)
        if (!dev_pass) die("the record store needs the device path");
        stores.assign(1, preset->store);
        seam_stores.assign(1, nullptr);
      } else if (dev_pass && knobs.store) {
        // (sized by CallKnobs::store_sizes; more than fits: the file is read again, as before)
        const size_t n_reg = bam_cuts.size() - 1;
        stores.assign(n_reg, nullptr);
        seam_stores.assign(n_reg, nullptr);
        store_alloc = std::thread([this, n_reg] {
          const auto t0 = std::chrono::steady_clock::now();
          for (size_t g = 0; g < n_reg; ++g) {
            // (--region with an index: the store holds the ranges' records, and is sized by their bytes)
            const bool ranged = bam_region_plan().active && bam_region_plan().path == o.bam;
            const std::pair<int64_t, int64_t> sz = knobs.store_sizes(ranged ? (int64_t)bam_region_plan().bytes() : (int64_t)(bam_cuts[g + 1] - bam_cuts[g]));
            if (svdss_bam_store_create((int32_t)(g % (size_t)n_dev), sz.first, sz.second, &stores[g]) != SVDSS_OK) stores[g] = nullptr;
            if (g > 0 && svdss_bam_store_create((int32_t)(g % (size_t)n_dev), (int64_t)64 << 20, 0, &seam_stores[g]) != SVDSS_OK) seam_stores[g] = nullptr;
          }
          store_alloc_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        });
      }
    }
    // ---- parse_sfsfile (sfs.cpp:5-30)
    // (csrc/sfs_file.h: the file mapped and parsed by T threads; a file that cannot be opened leaves the map empty, as
    // the reference's ifstream does)
    if (preset && preset->sfs_text) (void)sfs_parse_buffer(preset->sfs_text, preset->sfs_bytes, T, C.sfs);
    else (void)sfs_parse_file(o.sfs.c_str(), T, C.sfs);
    stage("reference + sfs file");
  }

  // the device path over the file's regions (bam_cuts): one filter per region, filter(dev) on the region's GPU; with_stores:
  // the slim form of every record that passes the flag / mapq filters also stays in the region's record store
  // input_index: the streams' input index is on (pass 1 with --write-bam-index: the batches carry their fragments)
  void open_select(RecordFeed& f, int32_t n_ref, bool with_stores, const std::function<svdss_bam_filter_t*(int32_t)>& filter, bool input_index = false) {
    std::vector<ShardedBamSelect<SelectedBatch>::Shard> shards(bam_cuts.size() - 1);
    for (size_t g = 0; g < shards.size(); ++g) {
      f.filters.push_back(shards[g].filter = filter((int32_t)(g % (size_t)n_dev)));
      if (with_stores && !stores.empty()) { shards[g].store = stores[g]; shards[g].seam_store = seam_stores[g]; }
    }
    f.sel.reset(new ShardedBamSelect<SelectedBatch>(o.bam, shards, n_ref, bam_skip, knobs.feeders, knobs.batch_bytes, bam_cuts,
                                                    input_index ? bam_ix.shift() : 0, input_index ? bam_ix.depth() : 0));
    if (input_index) f.on_batch = [this, &f](const SelectedBatch& b) { bam_ix.add(b.in_ix, *f.sel); };
  }

  // --write-bam-index FILE: the index of --bam, folded from the fragments pass 1's batches carry (the host reader: a pass of
  // index_bam_on_host's own, one thread, beside nothing).  An unsorted BAM: a warning and no index -- the index is a by-product
  InputIndexFold bam_ix;
  void open_bam_index() {
    if (o.write_bam_index.empty() || from_store()) return;
    std::vector<int32_t> lens;
    std::string err;
    if (!bam_header_lengths(o.bam, lens, err)) die("cannot read " + o.bam + ": " + err);
    if (!bam_ix.open(o.write_bam_index, lens, "--write-bam-index", err)) die(err);
  }
  void write_bam_index() {
    if (!bam_ix.on()) return;
    std::string err;
    if (!dev_pass) {
      uint64_t comp_bytes = 0;
      if (!index_bam_on_host(o.bam, bam_ix, comp_bytes, err)) die("error reading " + o.bam + ": " + err);
    }
    if (bam_ix.finish(o.bam, err)) logmsg("info", "index of " + o.bam + " written to " + o.write_bam_index);
    else if (bam_ix.unsorted()) logmsg("warning", "--write-bam-index: " + err);
    else die(err);
  }

  // the host reader, its chunks inflated on n_gpus GPUs in turn (where there are)
  void open_reader(RecordFeed& f, int n_gpus) {
    f.bam.reset(new BamReader(o.bam));
    svdss_enable_gpu_inflate(*f.bam, 0, n_gpus);
    if (!f.bam->ok() || !f.bam->read_header()) die("cannot read " + o.bam + ": " + f.bam->error());
  }

  // Pass 1 through the device path: the records of reads that have SFS.  --gpus N: the file's regions, one per GPU
  // (oversubscribed, effective_gpus puts the N shards on the GPUs there are -- the code path of N devices on a one-GPU box): every
  // region has its own scanner, batcher, feeding threads, record stream and filter; the slim form of every record that
  // passes the flag / mapq filters stays in that GPU's HBM for pass 2 (load_inputs took the memory; all of it or none is
  // used).  SVDSS_CALL_STORE=0: two passes over the file.
  void open_pass1_select(RecordFeed& f) {
    std::string names;
    std::vector<int64_t> name_off(1, 0);
    for (const auto& kv : C.sfs) { names += kv.first; name_off.push_back((int64_t)names.size()); }
    auto names_filter = [&](int32_t dev) {
      svdss_bam_filter_t* flt = nullptr;
      check(svdss_bam_filter_create(dev, (int32_t)std::min<unsigned>(o.min_mapq, 256u), n_ref_hdr, names.data(), name_off.data(),
                                    (int64_t)name_off.size() - 1, nullptr, nullptr, nullptr, 0, &flt), "svdss_bam_filter_create");
      return flt;
    };
    if (from_store()) {   // the stored batches, in batch order, through the names filter: no file is opened
      f.filters.push_back(names_filter(0));
      f.store = preset->store;
      f.store_batches = preset->store_batches;
      return;
    }
    if (store_alloc.joinable()) store_alloc.join();
    bool all_stores = !stores.empty();
    for (svdss_bam_store_t* st : stores) all_stores = all_stores && st != nullptr;
    for (size_t g = 1; g < seam_stores.size(); ++g) all_stores = all_stores && seam_stores[g] != nullptr;
    if (!all_stores) {
      for (svdss_bam_store_t* st : stores) svdss_bam_store_free(st);
      for (svdss_bam_store_t* st : seam_stores) svdss_bam_store_free(st);
      stores.clear(); seam_stores.clear();
    }
    open_select(f, n_ref_hdr, true, names_filter, bam_ix.on());
  }

  // Clusterer::align_and_extend (clusterer.cpp:56-156): pass 1 over the BAM, placement of every SFS
  void align_and_extend() {
    logmsg("info", "Placing SFSs on reference genome");
    // The inflated records of pass 1 are kept for pass 2 when they fit in memory (a second inflate of the whole file
    // otherwise): SVDSS_CALL_CACHE_GB, default 40 % of MemAvailable, at most 64 GiB.  Not on the device path.
    {
      double gb = knobs.cache_gb;
      if (!knobs.cache_gb_set) {
        if (FILE* f = fopen("/proc/meminfo", "r")) {
          char line[256];
          while (fgets(line, sizeof line, f)) {
            long long kb;
            if (sscanf(line, "MemAvailable: %lld kB", &kb) == 1) { gb = 0.4 * (double)kb / (1024.0 * 1024.0); break; }
          }
          fclose(f);
        }
        if (gb > 64) gb = 64;
      }
      cache_limit = gb > 0 ? (size_t)(gb * 1024.0 * 1024.0 * 1024.0) : 0;
      if (cache_limit == 0 || dev_pass) cache_ok = false;
    }
    {
      RecordFeed feed;
      open_bam_index();
      if (dev_pass) open_pass1_select(feed);
      else {
        // (--gpus N: the chunks of pass 1 are inflated on all N GPUs in turn, as `search` does -- on GPUs that are there,
        // whatever the oversubscribe knob says)
        open_reader(feed, std::max(1, std::min(o.gpus, n_dev)));
        ref_names = feed.bam->ref_names();
        feed.on_chunk = [this](const std::shared_ptr<BamReader::Bytes>& chunk) {
          if (!cache_ok) return;
          cache_bytes += chunk->size();
          if (cache_bytes > cache_limit) {   // too big to keep: pass 2 reads the file again
            cache_ok = false;
            cache_views.clear(); cache_views.shrink_to_fit();
            cache_chunks.clear(); cache_chunks.shrink_to_fit();
          } else cache_chunks.push_back(chunk);
        };
      }
      double pass1_join_s = 0;
      const auto pass1_t0 = std::chrono::steady_clock::now();
      const int bsize = std::max(T, (10000 / T) * T);   // config.hpp:69, config.cpp:106
      std::vector<std::vector<ESFS>> per_thread((size_t)T);
      std::vector<std::vector<Clip>> per_thread_clips((size_t)T);
      // the chromosomes in BAM header order on the GPU, for the placement kernel (SVDSS_PLACE_HOST=1: host code instead;
      // --clipped: host code as well -- the kernel reports how many SFS stay unplaced, not next to which soft clip).
      // Waiting for the FASTA's thread and the upload happen where the first batch is placed (the worker below, one at a
      // time): until then this thread goes on taking the records the device path selects -- a pass over a million reads
      // keeps a dozen thousand of them, and its feeders used to stand still behind a full queue while the reference
      // was read (0.7 s of a 1.2 s pass at GRCh38 lengths).
      svdss_ref_t* dref = nullptr;
      std::vector<int32_t> tid_map(ref_names.size(), -1);
      svdss_ref_t* session_dref = nullptr;   // (`run --samples`: the smoothing stage's upload, handed back below)
      const bool place_on_gpu = !knobs.place_host && !o.clipped;
      bool ref_set_up = false;
      auto set_up_reference = [this, &dref, &tid_map, &ref_set_up, &session_dref, place_on_gpu]() {
        if (ref_set_up) return;
        ref_set_up = true;
        reference_ready();
        SmoothHooks* const sm = preset ? preset->from_smooth : nullptr;
        if (sm && sm->dref) {   // (the smoothing stage's upload: the same chromosomes in the same order)
          if (place_on_gpu) { dref = sm->dref; tid_map = sm->tid_map; }
          if (sm->session) session_dref = sm->dref;
          else if (!place_on_gpu) svdss_ref_free(sm->dref);
          sm->dref = nullptr;
        } else if (place_on_gpu) check(resident_chromosomes(&ref_dev, ref_names, C.chrom_seqs, tid_map, &dref), "svdss_ref_upload_parts");
        ref_dev.drop();
      };
      // two batches: the next one is read (inflate + slicing, this thread) while the T slices of the previous one run
      std::vector<BamRecord> batches[2];
      std::thread worker;
      int cur = 0;
      std::string qname;
      bool eof = false;
      while (!eof) {
        std::vector<BamRecord>& batch = batches[cur];
        batch.clear();
        while ((int)batch.size() < bsize) {
          // records are located in the inflated chunks and only decoded if the read has SFS at all
          BamReader::RawView rr;
          const int rc = feed.next(rr);
          if (rc == 0) { eof = true; break; }
          if (rc < 0) { if (worker.joinable()) worker.join(); die("error reading " + o.bam + ": " + feed.err); }
          if (rr.flag & (4 | 2048 | 256)) continue;   // clusterer.cpp:118-122
          if ((unsigned)rr.mapq < o.min_mapq) continue;
          if (cache_ok) cache_views.push_back(rr);    // every record pass 2 looks at (same filters, clusterer.cpp:535-540)
          qname.assign((const char*)rr.name(), rr.l_name ? rr.l_name - 1 : 0);
          if (C.sfs.find(qname) == C.sfs.end()) continue;
          BamRecord r;
          BamReader::materialize(rr, r, false);   // (placement reads position, CIGAR and name: not the bases)
          batch.push_back(std::move(r));
        }
        {
          const auto tj0 = std::chrono::steady_clock::now();
          if (worker.joinable()) worker.join();   // batches are extended in order (per-thread output order, clusterer.cpp:129-141)
          pass1_join_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tj0).count();
        }
        // the T slices of the reference's OpenMP loop (clusterer.cpp:129-141), one worker each: the same records in
        // the same order per slice
        worker = std::thread([this, &per_thread, &per_thread_clips, &batch, &dref, &tid_map, &set_up_reference]() {
          set_up_reference();
          if (dref && !batch.empty()) {   // (the batch behind the last record may be empty: nothing to place, nothing to hand the kernel)
            // placement on the GPU (csrc/place.hip: one lane per alignment); the results go to the T per-thread lists in
            // the order the reference's slices would have produced them (record n belongs to slice n % T)
            std::vector<int32_t> tid, pos, sq, sl, cnt;
            std::vector<uint32_t> cig;
            std::vector<int64_t> cig_off(1, 0), sfs_off(1, 0);
            std::vector<const std::vector<RawSFS>*> lists;
            for (const BamRecord& r : batch) {
              // (a negative position on a record that claims to be mapped: not placed -- the walk indexes the chromosome with it)
              const bool known = r.tid >= 0 && r.tid < (int)ref_names.size() && tid_map[(size_t)r.tid] >= 0 && r.pos >= 0;
              tid.push_back(known ? tid_map[(size_t)r.tid] : -1);
              pos.push_back(r.pos);
              cig.insert(cig.end(), r.cigar.begin(), r.cigar.end());
              cig_off.push_back((int64_t)cig.size());
              const std::vector<RawSFS>& v = C.sfs.at(r.qname);
              lists.push_back(&v);
              if (known) for (const RawSFS& x : v) { sq.push_back(x.qs); sl.push_back(x.l); }
              sfs_off.push_back((int64_t)sq.size());
            }
            cnt.resize(batch.size());
            std::vector<int32_t> out(5 * std::max<size_t>(1, sq.size()));
            int64_t st[4];
            check(svdss_place_sfs_batch(dref, tid.data(), pos.data(), cig.data(), cig_off.data(), sq.data(), sl.data(),
                                        sfs_off.data(), (int64_t)batch.size(), cnt.data(), out.data(), st),
                  "svdss_place_sfs_batch");
            C.unplaced += st[0]; C.s_unplaced += st[1]; C.e_unplaced += st[2]; C.unknown += st[3];
            for (int t = 0; t < T; ++t)
              for (size_t n = (size_t)t; n < batch.size(); n += (size_t)T) {
                const BamRecord& r = batch[n];
                if (tid[n] < 0) continue;
                const int32_t* o = out.data() + 5 * sfs_off[n];
                for (int32_t j = 0; j < cnt[n]; ++j, o += 5)
                  per_thread[(size_t)t].push_back(ESFS{ref_names[(size_t)r.tid], r.qname, o[0], o[1], o[2], o[3],
                                                       (*lists[n])[(size_t)o[4]].htag});
              }
            return;
          }
          auto slice = [&](int t) {
            for (size_t n = (size_t)t; n < batch.size(); n += (size_t)T) {
              const BamRecord& r = batch[n];
              if (r.tid < 0 || r.tid >= (int)ref_names.size() || r.pos < 0) continue;
              extend_alignment(C, r, ref_names[(size_t)r.tid], per_thread[(size_t)t],
                               C.o.clipped ? &per_thread_clips[(size_t)t] : nullptr);
            }
          };
          if (T == 1 || batch.size() < 64) { for (int t = 0; t < T; ++t) slice(t); }
          else {
            std::vector<std::thread> pool;
            for (int t = 1; t < T; ++t) pool.emplace_back(slice, t);
            slice(0);
            for (std::thread& th : pool) th.join();
          }
        });
        cur ^= 1;
      }
      if (worker.joinable()) worker.join();
      write_bam_index();
      set_up_reference();   // (an input without a single batch: the later stages still want the chromosomes)
      if (feed.store) {
        region_batches.assign(1, feed.store_batches); region_seam.assign(1, 0);
        char buf[240];
        snprintf(buf, sizeof buf, "pass 1 from the records kept in HBM: %llu batches, %llu records looked at; select + records down %.3f s",
                 (unsigned long long)feed.n_batches, (unsigned long long)feed.n_records, feed.stage_s[3]);
        logmsg("debug", buf);
      }
      if (const ShardedBamSelect<SelectedBatch>* sel = feed.sel.get()) {
        region_batches.clear(); region_seam.clear();
        for (size_t g = 0; g < sel->n_regions(); ++g) { region_batches.push_back(sel->region_batches(g)); region_seam.push_back(sel->region_has_seam(g) ? 1 : 0); }
        if (sel->n_regions() > 1)
          logmsg("debug", std::to_string(sel->n_regions()) + " regions of the file, one per GPU: " + std::to_string(sel->seams_run()) + " seam(s) run, " +
                              std::to_string(sel->regions_run_again()) + " region(s) run again");
        if (feed.n_batches) {
          const double* st = feed.stage_s;
          char buf[480];
          snprintf(buf, sizeof buf, "pass 1 on the device: %llu batches, %llu records; feeder seconds summed: upload+inflate+crc+walk %.3f, turn wait %.3f, turn %.3f, "
                   "select+scans%s %.3f, records down %.3f (inflate kernels %.3f)", (unsigned long long)feed.n_batches, (unsigned long long)feed.n_records, st[0],
                   st[1], st[2], !stores.empty() ? "+store" : "", st[3], st[6], st[7]);
          logmsg("debug", buf);
          snprintf(buf, sizeof buf, "pass 1, this thread: %.3f s in all, %.3f s waiting for the device's batches, %.3f s waiting for the placement of the batch before; "
                   "the record store's memory took %.3f s; the batcher waited %.3f s for the file's loaders, %.3f s for the feeding threads",
                   std::chrono::duration<double>(std::chrono::steady_clock::now() - pass1_t0).count(), feed.wait_s, pass1_join_s, store_alloc_s, sel->waited_for_file(), sel->waited_for_feeders());
          logmsg("debug", buf);
        }
      }
      if (session_dref) session()->dref = session_dref;
      else svdss_ref_free(dref);
      for (int t = 0; t < T; ++t) extended.insert(extended.end(), per_thread[(size_t)t].begin(), per_thread[(size_t)t].end());
      for (int t = T; t-- > 0;)   // each thread's list goes in front of the others' (clusterer.cpp:24)
        clips.insert(clips.end(), per_thread_clips[(size_t)t].begin(), per_thread_clips[(size_t)t].end());
    }
    logmsg("info", std::to_string(C.unplaced.load()) + "/" + std::to_string(C.s_unplaced.load()) + "/" + std::to_string(C.e_unplaced.load()) +
                       " unplaced SFSs. " + std::to_string(C.unknown.load()) + " erroneus SFSs. " + std::to_string(clips.size()) +
                       " clipped SFSs.");   // clusterer.cpp:26-27
    stage("pass 1: placement");
  }

  // Clusterer::cluster_by_proximity (clusterer.cpp:407-474)
  void cluster_by_proximity() {
    // ---- cluster_by_proximity (clusterer.cpp:407-474)
    if (!extended.empty()) {
      std::sort(extended.begin(), extended.end());
      int maxlen = 0;
      for (const ESFS& s : extended) maxlen = std::max(maxlen, s.re - s.rs);
      const int dist = (int)(maxlen * 1.1);
      std::vector<std::pair<int, int>> intervals;
      int prev_i = 0, prev_e = extended[0].re;
      std::string prev_chrom = extended[0].chrom;
      for (size_t i = 1; i < extended.size(); ++i) {
        const ESFS& s = extended[i];
        if (s.chrom != prev_chrom) {
          prev_chrom = s.chrom; intervals.emplace_back(prev_i, (int)i - 1); prev_i = (int)i; prev_e = s.re; continue;
        }
        if (s.rs - prev_e > dist) { intervals.emplace_back(prev_i, (int)i - 1); prev_e = s.re; prev_i = (int)i; }
      }
      intervals.emplace_back(prev_i, (int)extended.size() - 1);
      std::vector<std::map<std::pair<int, int>, std::vector<ESFS>>> per_thread((size_t)T);
      for (size_t i = 0; i < intervals.size(); ++i) {
        auto& mp = per_thread[i % (size_t)T];   // schedule(static, 1)
        int j = intervals[i].first, low = extended[(size_t)j].rs, high = extended[(size_t)j].re, last_j = j;
        ++j;
        for (; j <= intervals[i].second; ++j) {
          const ESFS& s = extended[(size_t)j];
          if (s.rs <= high) { low = std::min(low, s.rs); high = std::max(high, s.re); }
          else {
            for (int k = last_j; k < j; ++k) mp[{low, high}].push_back(extended[(size_t)k]);
            low = s.rs; high = s.re; last_j = j;
          }
        }
        for (int k = last_j; k <= intervals[i].second; ++k) mp[{low, high}].push_back(extended[(size_t)k]);
      }
      for (int t = 0; t < T; ++t)
        for (auto& kv : per_thread[(size_t)t]) {
          Cluster c;
          c.sfss = kv.second;
          c.chrom = c.sfss[0].chrom;
          clusters.push_back(std::move(c));
        }
    }
    stage("cluster_by_proximity");
  }

  // the compressed bytes of a file chunk, at most (it ends somewhere in the block its end names)
  static uint64_t chunk_span(const std::pair<uint64_t, uint64_t>& ch) { return (ch.second >> 16) - (ch.first >> 16) + 65536; }

  // Where pass 2 takes the records from, in the order the sources are tried: the records pass 1 left in HBM, the record
  // cache of the host reader, the file chunks a BAI / CSI index names around the clusters, the whole file again (through
  // the device path, or the host reader)
  enum class Pass2 { store, cache, index, device, host };
  struct StoreItem { svdss_bam_store_t* st; int64_t key; size_t dev; };
  struct Pass2Plan {
    Pass2 src = Pass2::host;
    std::vector<StoreItem> items;                         // store: its batches, in file order
    int64_t st_records = 0, st_bytes = 0;
    std::vector<std::pair<uint64_t, uint64_t>> chunks;   // index: the file chunks around the clusters, merged
  };

  Pass2Plan plan_pass2(const ClusterRegions& R) {
    Pass2Plan p;
    if (!stores.empty()) {
      bool complete_all = true;
      for (size_t g = 0; g < stores.size(); ++g) {
        int32_t complete = 0;
        int64_t nr = 0, nb = 0;
        if (g > 0 && g < region_seam.size() && region_seam[g]) {
          (void)svdss_bam_store_batches(seam_stores[g], &complete, &nr, &nb);
          complete_all = complete_all && complete;
          p.st_records += nr; p.st_bytes += nb;
          p.items.push_back(StoreItem{seam_stores[g], 0, g % (size_t)n_dev});
        }
        const int64_t n_b = svdss_bam_store_batches(stores[g], &complete, &nr, &nb);
        complete_all = complete_all && complete && n_b == (g < region_batches.size() ? region_batches[g] : -1);
        p.st_records += nr; p.st_bytes += nb;
        for (int64_t k = 0; k < n_b; ++k) p.items.push_back(StoreItem{stores[g], k, g % (size_t)n_dev});
      }
      if (complete_all) { p.src = Pass2::store; return p; }
      logmsg("debug", "the record store is incomplete (" + std::to_string(p.st_bytes >> 20) + " MB kept): pass 2 reads the file again");
    }
    if (cache_ok) { p.src = Pass2::cache; return p; }
    // The records of pass 1 are not at hand.  With a BAI index beside the file (what the reference requires:
    // sam_index_load + one sam_itr_querys per cluster, clusterer.cpp:495-527) only the file chunks around the clusters are
    // read -- all regions turned into one sorted, merged chunk list, read once in file order, which visits the same records
    // in the same order as the full scan does among those that touch a cluster
    BaiIndex bai;
    bool have_bai = false;
    if (!knobs.no_bai) {
      // (x.bam.bai, x.bai, x.bam.csi, x.csi: the names htslib's sam_index_load looks for)
      const std::string stem = o.bam.size() > 4 && o.bam.compare(o.bam.size() - 4, 4, ".bam") == 0 ? o.bam.substr(0, o.bam.size() - 4) : std::string();
      have_bai = bai.load(o.bam + ".bai") || (!stem.empty() && bai.load(stem + ".bai")) || bai.load(o.bam + ".csi") ||
                 (!stem.empty() && bai.load(stem + ".csi"));
      if (have_bai && bai.refs.size() != ref_names.size()) have_bai = false;
    }
    if (have_bai) {
      for (size_t i = 0; i < R.rt.size(); ++i) bai.query(R.rt[i], R.rb[i], R.re[i], p.chunks);
      BaiIndex::merge(p.chunks);
      // The index names the file chunks around the clusters; host threads inflate them (~0.3 GB/s each; second session
      // of round 5: all of them, until then one).  When the chunks are a large part of the file, reading ALL of it
      // through the device path (tens of GB/s, only the overlapping records come back) is quicker: beyond 8 % of the
      // file per thread that scans.  SVDSS_CALL_PASS2 = bai | device overrides the estimate.
      if (dev_pass) {
        uint64_t bytes = 0;
        for (const auto& ch : p.chunks) bytes += chunk_span(ch);
        struct stat st;
        const uint64_t file_bytes = stat(o.bam.c_str(), &st) == 0 ? (uint64_t)st.st_size : 0;
        const double share = std::min(0.6, 0.08 * (double)pass2_threads(p.chunks.size()));
        if (knobs.pass2 == "device") have_bai = false;
        else if (knobs.pass2 != "bai" && file_bytes && (double)bytes > share * (double)file_bytes) have_bai = false;
      }
    }
    if (have_bai) {
      logmsg("debug", std::string("pass 2 through the ") + (bai.csi ? "CSI" : "BAI") + " index: " + std::to_string(R.rt.size()) + " regions, " +
                          std::to_string(p.chunks.size()) + " file chunks");
      p.src = Pass2::index;
    } else p.src = dev_pass ? Pass2::device : Pass2::host;
    return p;
  }

  // Round 6: the records are in HBM since pass 1 (svdss_bam_store_t; --gpus N: the store of every region in its GPU's).
  // Per stored batch a kernel keeps those that overlap a merged cluster region; they come down slim, in file order, and
  // go through `process` on a few threads, a stored batch per unit.
  std::vector<std::vector<Ev>> pass2_store(const ClusterRegions& R, const Pass2Plan& p) {
    std::vector<std::vector<Ev>> evs;
    uint64_t n_down = 0, bytes_down = 0;
    if (!R.rt.empty() && !p.items.empty()) {
      std::vector<svdss_bam_filter_t*> rf(std::min<size_t>((size_t)n_dev, stores.size()));   // the regions, on every GPU that holds a store
      for (size_t d = 0; d < rf.size(); ++d) rf[d] = R.filter((int32_t)d);
      const size_t Wt = std::max<size_t>(1, std::min<size_t>({(size_t)effective_cpus(), (size_t)8, p.items.size()}));
      // a thread's batch objects, one per device (a batch object belongs to one device); freed by that thread, beside the
      // others' frees (device and page-locked memory: milliseconds each)
      struct Selections {
        std::map<size_t, svdss_bam_batch_t*> on;
        std::string nm;
        ~Selections() { for (auto& kv : on) svdss_bam_batch_free(kv.second); }
      };
      std::atomic<uint64_t> a_down(0), a_bytes(0);
      evs = scan_units<Selections>(p.items.size(), Wt, "pass 2 from the record store: ", [&](Selections& sl, size_t k, auto& sink) -> std::string {
        const StoreItem& it = p.items[k];
        svdss_bam_batch_t*& b = sl.on[it.dev];
        const int rc = svdss_bam_store_select(it.st, it.key, rf[it.dev], &b);
        if (rc != SVDSS_OK) return std::string(svdss_strerror(rc)) + " " + svdss_last_hip_error();
        svdss_bam_selection_t r;
        (void)svdss_bam_batch_selection(b, &r);
        BamReader::RawView rr;
        for (int64_t i = 0; i < r.n_selected; ++i) {
          if (!view_of_record(r.bytes + r.rec_off[i], (size_t)(r.rec_off[i + 1] - r.rec_off[i]), rr, true)) return "corrupt record in the store";
          R.process(rr, sl.nm, sink);
        }
        a_down += (uint64_t)r.n_selected; a_bytes += (uint64_t)r.n_bytes;
        return std::string();
      });
      for (svdss_bam_filter_t* f : rf) svdss_bam_filter_free(f);
      n_down = a_down.load(); bytes_down = a_bytes.load();
    }
    logmsg("debug", "pass 2 from the records kept in HBM: " + std::to_string(p.st_records) + " records (" + std::to_string(p.st_bytes >> 20) + " MB) in " +
                        std::to_string(p.items.size()) + " batches" + (stores.size() > 1 ? " of " + std::to_string(stores.size()) + " stores" : "") + ", " +
                        std::to_string(R.rt.size()) + " regions, " + std::to_string(n_down) + " records (" + std::to_string(bytes_down >> 20) + " MB) came down");
    // (tens of GB of HBM stay allocated until the run ends: memory handed back is cleared by the driver beside whatever
    // runs next -- here the POA batches -- and `call` has room to spare: it holds no index)
    return evs;
  }

  // The chunks the index names, in runs of consecutive chunks of about the same size in the file, a few per thread:
  // every run is scanned by one thread with a file handle and an inflater of its own (bam_scan_chunks).
  std::vector<std::vector<Ev>> pass2_index(const ClusterRegions& R, const std::vector<std::pair<uint64_t, uint64_t>>& chunks) {
    const size_t Wt = pass2_threads(chunks.size());
    uint64_t total = 0, acc = 0;
    for (const auto& ch : chunks) total += chunk_span(ch);
    const uint64_t per = std::max<uint64_t>(1, total / (4 * Wt));
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> runs;
    for (const auto& ch : chunks) {
      if (runs.empty() || acc >= per) { runs.emplace_back(); acc = 0; }
      runs.back().push_back(ch);
      acc += chunk_span(ch);
    }
    return scan_units<std::string>(runs.size(), Wt, "error reading " + o.bam + ": ", [&](std::string& nm, size_t g, auto& sink) {
      return bam_scan_chunks(o.bam, runs[g], [&](const BamReader::RawView& rr) { R.process(rr, nm, sink); });
    });
  }

  // Clusterer::fill_clusters (clusterer.cpp:477-610): pass 2 over the BAM
  void fill_clusters() {
    const ClusterRegions R(clusters, ref_names, o.min_cluster_weight, o.min_mapq);
    C.small += R.n_small;
    std::vector<std::vector<int>> cov(clusters.size(), std::vector<int>(3, 0));
    // what the records do to the clusters, in BAM order
    auto apply = [&](Ev& e) {
      if (e.hp >= 0 && e.hp < 3) ++cov[e.ci][(size_t)e.hp];
      clusters[e.ci].reads.emplace_back(e.in_reads ? 1 : 0, e.hp == 0 ? 3 : e.hp);
      if (!e.in_reads) return;
      if (e.unext) ++C.unextended;
      else clusters[e.ci].subreads.push_back(SubRead{std::move(e.name), std::move(e.sub), e.hp});
    };
    auto apply_units = [&](std::vector<std::vector<Ev>> evs) {
      for (std::vector<Ev>& unit : evs)
        for (Ev& e : unit) apply(e);
    };
    const Pass2Plan p = plan_pass2(R);
    switch (p.src) {
      case Pass2::store: apply_units(pass2_store(R, p)); break;
      case Pass2::cache: {   // contiguous ranges of records, one per thread
        stage("pass 2: setup");
        const size_t n = cache_views.size();
        const size_t W = std::max<size_t>(1, std::min<size_t>({(size_t)effective_cpus(), (size_t)32, n / 4096 + 1}));
        std::vector<std::vector<Ev>> evs = scan_units<std::string>(W, W, "", [&](std::string& nm, size_t w, auto& sink) {
          for (size_t i = n * w / W; i < n * (w + 1) / W; ++i) R.process(cache_views[i], nm, sink);
          return std::string();
        });
        stage("pass 2: scan");
        apply_units(std::move(evs));
        stage("pass 2: apply");
        // (gigabytes of inflated records: released while the DP batches run)
        cache_release = std::thread([v = std::move(cache_views), c = std::move(cache_chunks)]() mutable { v.clear(); c.clear(); });
        break;
      }
      case Pass2::index: apply_units(pass2_index(R, p.chunks)); break;
      case Pass2::device: case Pass2::host: {
        // the whole file again, records applied as they come: through the device path with the merged cluster regions as
        // the filter (the records that overlap a cluster come back, in file order), or through the host reader
        if (p.src == Pass2::device && R.rt.empty()) break;
        RecordFeed feed;
        if (p.src == Pass2::host) open_reader(feed, 1);
        else open_select(feed, (int32_t)ref_names.size(), false, [&](int32_t dev) { return R.filter(dev); });
        std::string qname;
        BamReader::RawView rr;   // zero-copy: the record is used where it was inflated, within this iteration only
        int rc;
        while ((rc = feed.next(rr)) > 0) R.process(rr, qname, apply);
        if (rc < 0) die("error reading " + o.bam + ": " + feed.err);
      }
    }
    for (size_t i = 0; i < clusters.size(); ++i) {
      if (!R.live[i]) { clusters[i].reads.clear(); clusters[i].subreads.clear(); continue; }
      if (clusters[i].size() >= (size_t)o.min_cluster_weight) {
        clusters[i].cov0 = cov[i][0]; clusters[i].cov1 = cov[i][1]; clusters[i].cov2 = cov[i][2];
        clusters[i].cov = cov[i][0] + cov[i][1] + cov[i][2];
      } else ++C.small2;
    }
    stage("pass 2: fill_clusters");
  }

  // Clusterer::store_clusters (clusterer.cpp:613-626), then Caller::split_cluster (caller.cpp:100-255)
  void store_and_split() {
    // ---- store_clusters (clusterer.cpp:613-626): every cluster, also the filtered ones (their coordinates are
    // uninitialised in the reference; 0 here)
    if (!o.clusters.empty()) {
      logmsg("info", "Storing clusters to " + o.clusters);
      FILE* f = fopen(o.clusters.c_str(), "w");
      if (!f) die("cannot write " + o.clusters);
      std::string line;
      for (const Cluster& c : clusters) {
        line = c.chrom + ":" + std::to_string(c.s + 1) + "-" + std::to_string(c.e + 1) + "\t" + std::to_string(c.size());
        for (const SubRead& sr : c.subreads) { line += "\t"; line += sr.name; line += ":"; line += sr.seq; }
        line += "\n";
        fwrite(line.data(), 1, line.size(), f);
      }
      fclose(f);
    }
    logmsg("info", "Calling SVs from " + std::to_string(clusters.size()) + " clusters..");
    // ---- pcall (caller.cpp:311-406): split, then the three GPU batches
    for (size_t i = 0; i < clusters.size(); ++i) {
      if (clusters[i].size() < (size_t)o.min_cluster_weight) continue;
      for (Cluster& cl : split_cluster(clusters[i], o.useht, o.min_ratio)) subs.push_back(Sub{i, std::move(cl)});
    }
    stage("split_cluster");
  }

  // Caller::run_poa for every sub-cluster (caller.cpp:257-308), one GPU batch per device
  void run_poa() {
    consensus.assign(subs.size(), std::string());
    if (!subs.empty()) {
      // the sub-reads of every sub-cluster back to back in abPOA's alphabet: offsets first, then the bytes by T
      // threads (a 30x human sample is ~1 GB of sub-reads: one byte at a time on one thread took seconds)
      std::vector<int64_t> seq_off(1, 0), cl_off(1, 0);
      std::vector<const std::string*> srcs;
      for (const Sub& s : subs) {
        for (const SubRead& sr : s.cl.subreads) {
          srcs.push_back(&sr.seq);
          seq_off.push_back(seq_off.back() + (int64_t)sr.seq.size());
        }
        cl_off.push_back((int64_t)seq_off.size() - 1);
      }
      // (not a vector: its zero-fill of ~1 GB on one thread was a fifth of this stage at 30x; the threads below write every byte)
      struct Flat { std::unique_ptr<uint8_t[]> p; uint8_t* data() const { return p.get(); } uint8_t* begin() const { return p.get(); } } flat{std::unique_ptr<uint8_t[]>(new uint8_t[(size_t)seq_off.back() + 1])};
      {
        uint8_t lut[256];
        for (int c = 0; c < 256; ++c) lut[c] = enc26((char)c);
        const size_t ns = srcs.size(), nt = std::min<size_t>((size_t)T, std::max<size_t>(1, ns / 256));
        auto enc = [&](size_t t) {
          for (size_t k = ns * t / nt; k < ns * (t + 1) / nt; ++k) {
            uint8_t* d = flat.data() + seq_off[k];
            const std::string& q = *srcs[k];
            for (size_t x = 0; x < q.size(); ++x) d[x] = lut[(uint8_t)q[x]];
          }
        };
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nt; ++t) pool.emplace_back(enc, t);
        enc(0);
        for (std::thread& th : pool) th.join();
      }
      // --gpus G: sub-cluster k goes to GPU k % G (no exchange between the GPUs: a sub-cluster is self-contained), the
      // consensus sequences come back in sub-cluster order -- the same bytes as with one GPU
      std::vector<int64_t> lens(subs.size());
      std::vector<uint8_t> cons;
      {
        const size_t nsub = subs.size();
        std::vector<std::vector<uint8_t>> part_cons((size_t)G);
        std::vector<std::vector<int64_t>> part_lens((size_t)G);
        std::vector<std::thread> pool;
        auto run = [&](int g) {
          std::vector<uint8_t> f;
          std::vector<int64_t> so(1, 0), co(1, 0);
          for (size_t k = (size_t)g; k < nsub; k += (size_t)G) {
            for (int64_t sq = cl_off[k]; sq < cl_off[k + 1]; ++sq) {
              f.insert(f.end(), flat.begin() + seq_off[(size_t)sq], flat.begin() + seq_off[(size_t)sq + 1]);
              so.push_back((int64_t)f.size());
            }
            co.push_back((int64_t)so.size() - 1);
          }
          svdss_poa_batch_t* pb = nullptr;
          const auto tp0 = std::chrono::steady_clock::now();
          check(svdss_poa_consensus_batch(G == 1 ? flat.data() : f.data(), G == 1 ? seq_off.data() : so.data(),
                                          G == 1 ? cl_off.data() : co.data(), (int64_t)co.size() - 1, g % n_dev, &pb),
                "svdss_poa_consensus_batch");
          const auto tp1 = std::chrono::steady_clock::now();
          part_lens[(size_t)g].resize(co.size() - 1);
          part_cons[(size_t)g].resize((size_t)svdss_poa_batch_total(pb));
          check(svdss_poa_batch_fetch(pb, part_lens[(size_t)g].data(), part_cons[(size_t)g].data()), "svdss_poa_batch_fetch");
          const auto tp2 = std::chrono::steady_clock::now();
          svdss_poa_batch_free(pb);
          if (o.verbose && knobs.debug)
            fprintf(stderr, "[call] [debug] POA shard %d: batch %.3f s, fetch %.3f s, free %.3f s\n", g, std::chrono::duration<double>(tp1 - tp0).count(),
                    std::chrono::duration<double>(tp2 - tp1).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - tp2).count());
        };
        for (int g = 1; g < G; ++g) pool.emplace_back(run, g);
        run(0);
        for (std::thread& th : pool) th.join();
        std::vector<size_t> at((size_t)G, 0), idx((size_t)G, 0);
        for (size_t k = 0; k < nsub; ++k) {
          const size_t g = k % (size_t)G;
          lens[k] = part_lens[g][idx[g]++];
          cons.insert(cons.end(), part_cons[g].begin() + (long)at[g], part_cons[g].begin() + (long)(at[g] + (size_t)lens[k]));
          at[g] += (size_t)lens[k];
        }
      }
      size_t p = 0;
      for (size_t i = 0; i < subs.size(); ++i) {
        consensus[i].resize((size_t)lens[i]);
        for (int64_t k = 0; k < lens[i]; ++k) consensus[i][(size_t)k] = "ACGTN"[cons[p++]];   // caller.cpp:297
      }
    }
    stage("POA");
  }

  // ksw_extd2 of every consensus against its window, SV extraction (caller.cpp:326-406)
  void realign_and_extract() {
    if (!subs.empty()) {
      const int8_t a = 1, b = -9;   // caller.cpp:333-337
      const int8_t mat[25] = {a, b, b, b, 0, b, a, b, b, 0, b, b, a, b, 0, b, b, b, a, 0, 0, 0, 0, 0, 0};
      std::vector<uint8_t> q, t;
      std::vector<int64_t> qo(1, 0), to(1, 0);
      for (size_t i = 0; i < subs.size(); ++i) {
        const Cluster& cl = subs[i].cl;
        const std::string& cs = C.chrom_seqs[cl.chrom];
        for (char ch : consensus[i]) q.push_back(enc26(ch));
        qo.push_back((int64_t)q.size());
        for (int p = cl.s; p <= cl.e && p < (int)cs.size(); ++p) t.push_back(enc26(cs[(size_t)p]));   // caller.cpp:329
        to.push_back((int64_t)t.size());
      }
      std::vector<int32_t> scores(subs.size());
      std::vector<int64_t> ncig(subs.size());
      std::vector<uint32_t> cig;
      {
        const size_t nsub = subs.size();
        std::vector<std::vector<int32_t>> p_sc((size_t)G);
        std::vector<std::vector<int64_t>> p_nc((size_t)G);
        std::vector<std::vector<uint32_t>> p_cg((size_t)G);
        std::vector<std::thread> pool;
        auto run = [&](int g) {
          std::vector<uint8_t> q2, t2;
          std::vector<int64_t> qo2(1, 0), to2(1, 0);
          if (G > 1)
            for (size_t k = (size_t)g; k < nsub; k += (size_t)G) {
              q2.insert(q2.end(), q.begin() + qo[k], q.begin() + qo[k + 1]);
              qo2.push_back((int64_t)q2.size());
              t2.insert(t2.end(), t.begin() + to[k], t.begin() + to[k + 1]);
              to2.push_back((int64_t)t2.size());
            }
          const int64_t np = G == 1 ? (int64_t)nsub : (int64_t)qo2.size() - 1;
          svdss_aln_batch_t* ab = nullptr;
          check(svdss_align_global_batch(G == 1 ? q.data() : q2.data(), G == 1 ? qo.data() : qo2.data(),
                                         G == 1 ? t.data() : t2.data(), G == 1 ? to.data() : to2.data(), np, 5, mat, 16, 2, 41,
                                         1, g % n_dev, &ab), "svdss_align_global_batch");
          p_sc[(size_t)g].resize((size_t)np);
          p_nc[(size_t)g].resize((size_t)np);
          p_cg[(size_t)g].resize((size_t)svdss_aln_batch_total_cigar(ab));
          check(svdss_aln_batch_fetch(ab, p_sc[(size_t)g].data(), p_nc[(size_t)g].data(), p_cg[(size_t)g].data()),
                "svdss_aln_batch_fetch");
          svdss_aln_batch_free(ab);
        };
        for (int g = 1; g < G; ++g) pool.emplace_back(run, g);
        run(0);
        for (std::thread& th : pool) th.join();
        std::vector<size_t> at((size_t)G, 0), idx((size_t)G, 0);
        for (size_t k = 0; k < nsub; ++k) {
          const size_t g = k % (size_t)G;
          scores[k] = p_sc[g][idx[g]];
          ncig[k] = p_nc[g][idx[g]++];
          cig.insert(cig.end(), p_cg[g].begin() + (long)at[g], p_cg[g].begin() + (long)(at[g] + (size_t)ncig[k]));
          at[g] += (size_t)ncig[k];
        }
      }
      std::vector<std::vector<SV>> per_thread((size_t)T);
      sam_rows.resize((size_t)T);
      size_t cp = 0;
      for (size_t i = 0; i < subs.size(); ++i) {
        const Cluster& cl = subs[i].cl;
        const Cluster& parent = clusters[subs[i].parent];
        const std::string& cs = C.chrom_seqs[cl.chrom];
        std::string cigar_str;
        for (int64_t k = 0; k < ncig[i]; ++k) cigar_str += std::to_string(cig[cp + (size_t)k] >> 4) + "MID"[cig[cp + (size_t)k] & 0xf];
        if (!o.poa.empty()) {   // Consensus, caller.hpp:56-69 / caller.cpp:356-357
          const std::string p1 = std::to_string(cl.s + 1);
          sam_rows[subs[i].parent % (size_t)T].push_back(cl.chrom + ":" + p1 + "-" + std::to_string(cl.e + 1) + "\t0\t" + cl.chrom +
                                                         "\t" + p1 + "\t60\t" + cigar_str + "\t*\t0\t0\t" + consensus[i] + "\t*");
        }
        std::string names;
        for (const SubRead& sr : cl.subreads) names += sr.name + ",";
        if (!names.empty()) names.pop_back();
        std::string rvec;
        for (const auto& rd : parent.reads) rvec += std::to_string(rd.first) + ":" + std::to_string(rd.second) + "-";
        if (!rvec.empty()) rvec.pop_back();
        std::vector<SV> local;
        unsigned rpos = (unsigned)cl.s, cpos = 0;
        int nv = 0;
        for (int64_t k = 0; k < ncig[i]; ++k) {
          const unsigned l = cig[cp + (size_t)k] >> 4;
          const char op = "MID"[cig[cp + (size_t)k] & 0xf];
          if (op == 'M') { rpos += l; cpos += l; }
          else if (op == 'I') {
            if (l >= o.min_sv_length) {
              const std::string anchor(1, cs[rpos - 1]);
              SV v = make_sv("INS", cl.chrom, (int)rpos, anchor, anchor + consensus[i].substr(cpos, l), (unsigned)cl.size(),
                             cl.cov, nv, scores[i], (int)l, cigar_str);
              v.reads = names;
              local.push_back(v);
              ++nv;
            }
            cpos += l;
          } else {
            if (l >= o.min_sv_length) {
              SV v = make_sv("DEL", cl.chrom, (int)rpos, cs.substr(rpos - 1, l + 1), std::string(1, cs[rpos - 1]),
                             (unsigned)cl.size(), cl.cov, nv, scores[i], (int)l, cigar_str);
              v.reads = names;
              local.push_back(v);
              ++nv;
            }
            rpos += l;
          }
        }
        cp += (size_t)ncig[i];
        for (SV& v : local) {
          v.ngaps = nv; v.gt = "0/1"; v.gtq = 100;
          v.cov = cl.cov; v.cov0 = cl.cov0; v.cov1 = cl.cov1; v.cov2 = cl.cov2;
          v.rvec = rvec;
          per_thread[subs[i].parent % (size_t)T].push_back(v);
        }
      }
      for (int t = 0; t < T; ++t) svs.insert(svs.begin(), per_thread[(size_t)t].begin(), per_thread[(size_t)t].end());   // caller.cpp:18-22
    }
    stage("realign + SV extraction");
  }

  // sort, clean_dups, filter_sv_chains, sort (caller.cpp:23-28, 409-475)
  void dedup_and_filter() {
    std::sort(svs.begin(), svs.end());   // same libstdc++ std::sort as the reference (caller.cpp:23)
    {   // clean_dups (caller.cpp:409-426)
      std::vector<SV> kept;
      std::string lc, lr, la; int lp = -1;
      for (const SV& v : svs) {
        if (lc != v.chrom || lp != v.s || lr != v.refall || la != v.altall) kept.push_back(v);
        lc = v.chrom; lp = v.s; lr = v.refall; la = v.altall;
      }
      svs.swap(kept);
    }
    if (svs.size() >= 2) {   // filter_sv_chains (caller.cpp:429-475): ratios of adjacent candidates in one batch
      std::vector<size_t> cand;
      std::vector<uint8_t> A, B;
      std::vector<int64_t> ao(1, 0), bo(1, 0);
      for (size_t i = 1; i < svs.size(); ++i) {
        const SV &prev = svs[i - 1], &sv = svs[i];
        if (sv.chrom == prev.chrom && sv.s - prev.e < 2 * sv.l && prev.type == sv.type) {
          const double w_r = std::min((double)sv.w, (double)prev.w) / std::max((double)sv.w, (double)prev.w);
          const double l_r = std::min((double)sv.l, (double)prev.l) / std::max((double)sv.l, (double)prev.l);
          const int d = sv.s - prev.s;
          if (d < 100 && w_r >= 0.9 && l_r >= o.min_ratio) {
            const std::string& x = sv.type == "DEL" ? sv.refall : sv.altall;
            const std::string& y = sv.type == "DEL" ? prev.refall : prev.altall;
            A.insert(A.end(), x.begin(), x.end()); ao.push_back((int64_t)A.size());
            B.insert(B.end(), y.begin(), y.end()); bo.push_back((int64_t)B.size());
            cand.push_back(i);
          }
        }
      }
      std::map<size_t, double> sim;
      if (!cand.empty()) {
        std::vector<double> ratio(cand.size());
        uint8_t dummy = 0;
        check(svdss_indel_ratio_batch(A.empty() ? &dummy : A.data(), ao.data(), B.empty() ? &dummy : B.data(), bo.data(),
                                      (int64_t)cand.size(), 0, ratio.data(), nullptr), "svdss_indel_ratio_batch");
        for (size_t k = 0; k < cand.size(); ++k) sim[cand[k]] = ratio[k];
      }
      std::vector<SV> kept;
      SV prev = svs[0];
      bool reset = false;
      for (size_t i = 1; i < svs.size(); ++i) {
        if (reset) { reset = false; prev = svs[i]; continue; }
        const SV& sv = svs[i];
        auto it = sim.find(i);
        if (it != sim.end() && it->second > 70) { kept.push_back(sv.w > prev.w ? sv : prev); reset = true; continue; }
        kept.push_back(prev);
        prev = sv;
      }
      kept.push_back(prev);
      svs.swap(kept);
    }
    std::sort(svs.begin(), svs.end());
    stage("dups + chain filter");
    // ---- write_vcf (caller.cpp:59-63, 477-550)
  }

  // write_vcf / write_sam / --clipped rows (caller.cpp:36-75, 477-550)
  void write_outputs() {
    std::string out = "##fileformat=VCFv4.2\n##reference=ftp://ftp.1000genomes.ebi.ac.uk/vol1/ftp/data_collections/HGSVC2/"
                      "technical/reference/20200513_hg38_NoALT/hg38.no_alt.fa.gz\n";
    for (const std::string& n : C.chrom_names) out += "##contig=<ID=" + n + ",length=" + std::to_string(C.chrom_seqs[n].size()) + ">\n";
    out += "##FILTER=<ID=PASS,Description=\"All filters passed\">\n";
    for (const auto& f : VCF_INFO) out += std::string("##INFO=<ID=") + f[0] + ",Number=" + f[1] + ",Type=" + f[2] + ",Description=\"" + f[3] + "\">\n";
    out += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
    out += "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality\">\n";
    out += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tDEFAULT\n";
    for (const SV& v : svs) out += v.line() + "\n";
    fwrite(out.data(), 1, out.size(), stdout);
    fflush(stdout);
    logmsg("info", "Writing " + std::to_string(svs.size()) + " SVs.");
    stage("vcf");
    if (cache_release.joinable()) cache_release.join();
    if (knobs.clean_exit || session()) {   // (otherwise the process ends with _exit)
      for (svdss_bam_store_t* st : stores) svdss_bam_store_free(st);
      for (svdss_bam_store_t* st : seam_stores) svdss_bam_store_free(st);
      stores.clear(); seam_stores.clear();
    }
    // ---- write_sam (caller.cpp:65-75): rows in the order of the reference's per-thread lists, each inserted at the
    // front of the global one (caller.cpp:18-22)
    if (!o.poa.empty()) {
      logmsg("info", "Writing POA alignments to " + o.poa + "..");
      FILE* f = fopen(o.poa.c_str(), "w");
      if (!f) die("cannot write " + o.poa);
      std::string hdr = "@HD\tVN:1.4\n";
      for (const std::string& n : C.chrom_names) hdr += "@SQ\tSN:" + n + "\tLN:" + std::to_string(C.chrom_seqs[n].size()) + "\n";
      fwrite(hdr.data(), 1, hdr.size(), f);
      for (size_t t = sam_rows.size(); t-- > 0;)
        for (const std::string& row : sam_rows[t]) { fwrite(row.data(), 1, row.size(), f); fputc('\n', f); }
      fclose(f);
    }
    if (o.clipped) {   // caller.cpp:36-53: imprecise rows after the VCF, in the Clipper's own order (not sorted)
      logmsg("warning", "Calling imprecise SVs from clipped alignments is experimental");
      std::vector<std::pair<int, int>> called;
      for (const SV& v : svs) called.emplace_back(v.s - 1000, v.e + 1000);
      const std::vector<SV> rows = call_clipped(clips, C.chrom_names, C.chrom_seqs, T, called);
      logmsg("info", "Predicted " + std::to_string(rows.size()) + " SVs from clipped alignments");
      std::string text;
      for (const SV& v : rows) text += v.line() + "\n";
      fwrite(text.data(), 1, text.size(), stdout);
      fflush(stdout);
    }
  }

  int run() {
    load_inputs();
    align_and_extend();
    cluster_by_proximity();
    fill_clusters();
    store_and_split();
    run_poa();
    realign_and_extract();
    dedup_and_filter();
    write_outputs();
    if (SmoothHooks* sm = session()) {
      sm->chrom_names = std::move(C.chrom_names);
      sm->chrom_seqs = std::move(C.chrom_seqs);
    }
    return 0;
  }
};

}  // namespace

int main_call(const CallOptions& o, CallPreset* preset) {
  CallRun run(o, preset);
  return run.run();
}
