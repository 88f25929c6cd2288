// bam_device.hip -- BAM records walked, filtered and unpacked where they are inflated: compressed BGZF blocks in, SFS out
// (svdss_bam_batch_run).
//
// Stands where PingPong::load_batch_bam and the head of PingPong::process_batch stand (/root/reference/ping_pong.cpp:
// 53-128, 176-209): sam_read1 (bgzf inflate + the block_size chain of the records, :58), the flag / length / tid filters
// (:66-79), the 4-bit -> nt6 expansion (:90-94), the XF / HP aux lookup and the putative filter (:196-203).  Until round 3
// the inflated bytes went down to the host, one thread sliced the records there and the packed bases came up again
// (0.55-0.69 M reads/s against 8 M for the kernels).  Here only the compressed bytes go up and ~40 bytes per
// read (name, tags) plus the SFS come down.
//
// One batch = a run of consecutive BGZF blocks (a few hundred MB inflated), inflated into ONE device buffer so that a
// record that straddles two blocks is contiguous.  The record that straddles two BATCHES is carried: the bytes behind the
// last complete record of batch b are copied in front of batch b + 1's data (head room).  Per batch:
//   inflate     csrc/inflate.hip, one wavefront per block; crc32_kernel checks the BGZF footers (one wavefront per block:
//               lane l takes the words l, l + 64, ... with a <- a x^2048 + w through 4 x 256-entry tables in LDS, the lanes'
//               sums combined with x^(32 (64 - l)) -- the arithmetic of zlib's crc32_combine);
//   walk        the records form a chain (offset += 4 + block_size): ~23,000 dependent loads per batch if one lane
//               follows it.  walk_kernel cuts the batch into segments, one wavefront each: the 64 lanes look for the
//               first plausible record start in the segment (64 candidates per step; plausible = every field in range
//               and the record behind it plausible too), lane 0 follows the chain from there to the segment's end.
//               link_kernel then proves the guesses: starting from the TRUE first record (the carry, or the end of the
//               BAM header) the chain must arrive exactly at every segment's guessed start; a segment it does not arrive
//               at is walked again from where it did arrive.  The result never depends on the guess, only the speed does
//               (the same contract as the segmented search);
//   meta        one lane per record: core fields, the filters, XF / HP from the aux block (bam_aux_get + bam_aux2i);
//   scatter     exclusive scans (hipcub) place the names, the tags and the reads that are searched;
//   unpack      4-bit bases -> nt6, 16 output bytes per lane, straight from the inflated records;
//   search      svdss_sfs_search_batch_device on the batch's stream.
// Batches of one file run concurrently on their own streams (several feeding threads); only the link step is ordered
// (it needs the carry of the previous batch): svdss_bam_stream holds the carry and the turn.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <thread>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bam_device_internal.h"
#include "bam_index_writer.h"
#include "hip_check.h"
#include "index_host.h"
#include "inflate_dev.h"
#include "deflate_dev.h"
#include "ref_dev.h"

namespace {

constexpr int64_t kHeadDefault = (int64_t)16 << 20;   // room in front of a batch's data for the carried bytes
constexpr int kMaxSeg = 2048;
constexpr int64_t kMinRec = 36;                        // block_size field + the 32 core bytes

// ------------------------------------------------------------------ the chain of records
// (SegWalk under the name and in the unnamed namespace the kernels have always taken it by: their symbols stay what they were)
struct WalkP : SegWalk {};

// necessary conditions on the 36 bytes at p (and the name's terminator) for a record of a file htslib reads
__device__ __forceinline__ bool plausible(const uint8_t* buf, int64_t p, int64_t hi, int32_t n_ref) {
  if (p + kMinRec > hi) return false;
  const uint32_t bs = ld32(buf, p);
  if (bs < 32u || bs > (1u << 28)) return false;
  const int32_t tid = (int32_t)ld32(buf, p + 4), pos = (int32_t)ld32(buf, p + 8);
  if (tid < -1 || tid >= n_ref || pos < -1) return false;
  const uint32_t w3 = ld32(buf, p + 12), w4 = ld32(buf, p + 16);
  const int32_t l_seq = (int32_t)ld32(buf, p + 20), mtid = (int32_t)ld32(buf, p + 24), mpos = (int32_t)ld32(buf, p + 28);
  if (l_seq < 0 || mtid < -1 || mtid >= n_ref || mpos < -1) return false;
  const uint32_t l_name = w3 & 0xffu, n_cig = w4 & 0xffffu;
  if (l_name == 0) return false;
  const int64_t head = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)l_seq + 1) / 2 + l_seq;
  if (head > (int64_t)bs) return false;
  const int64_t nul = p + 36 + l_name - 1;
  if (nul < hi && buf[nul] != 0) return false;
  return true;
}

__global__ void __launch_bounds__(64) walk_kernel(WalkP P) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int64_t s_lo = P.lo + (int64_t)s * P.seg_bytes;
  int64_t s_hi = s_lo + P.seg_bytes;
  if (s_hi > P.hi || s == P.n_seg - 1) s_hi = P.hi;
  int64_t found = -1;
  for (int64_t p0 = s_lo; p0 < s_hi; p0 += 64) {
    const int64_t p = p0 + lane;
    bool ok = p < s_hi && plausible(P.buf, p, P.hi, P.n_ref);
    if (ok) {   // the record behind it: plausible too, or not visible any more
      const int64_t p2 = p + 4 + (int64_t)ld32(P.buf, p);
      ok = p2 + kMinRec > P.hi ? p2 <= P.hi + ((int64_t)1 << 28) : plausible(P.buf, p2, P.hi, P.n_ref);
    }
    const unsigned long long m = __ballot(ok);
    if (m) { found = p0 + __builtin_ctzll(m); break; }
  }
  found = ((int64_t)__builtin_amdgcn_readfirstlane((int)(found >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)found);
  uint32_t* list = P.lists + (int64_t)s * P.list_cap;
  int64_t p = found;
  int cnt = 0;
  if (found >= 0) {
    while (p < s_hi) {
      if (p + 4 > P.hi) break;
      const uint32_t bs = ld32(P.buf, p);
      if (bs < 32u) break;                                   // not a chain of records (or a damaged file: link_kernel says which)
      if (p + 4 + (int64_t)bs > P.hi) break;
      if (lane == 0) list[cnt] = (uint32_t)p;
      ++cnt;
      p += 4 + (int64_t)bs;
    }
  }
  if (lane == 0) {
    P.seg_start[s] = found >= 0 ? (uint32_t)found : 0xffffffffu;
    P.seg_end[s] = (uint32_t)(found >= 0 ? p : 0);
    P.seg_cnt[s] = cnt;
  }
}

// From the true first record through every segment: hdr[H_NREC] records, their offsets in lists / pre, hdr[H_TAIL] = the
// first byte that belongs to no complete record.  One wavefront; the segment table sits in LDS.
// start < 0 (the first batch of a file region whose first record nobody knows yet, svdss_bam_stream_region): the chain
// starts at the first guess of the segments, hdr[H_START] says where (-1: no segment found one); the caller of the region
// proves that guess when the region in front has ended (the bytes before it complete that region's last record).
__global__ void __launch_bounds__(64) link_kernel(WalkP P, int64_t start, uint32_t* pre, int32_t* seg_base, int64_t* hdr) {
  __shared__ uint32_t sst[kMaxSeg], sen[kMaxSeg];
  __shared__ int32_t scn[kMaxSeg];
  const int lane = threadIdx.x;
  for (int i = lane; i < P.n_seg; i += 64) { sst[i] = P.seg_start[i]; sen[i] = P.seg_end[i]; scn[i] = P.seg_cnt[i]; }
  __syncthreads();
  if (lane != 0) return;
  int64_t err = 0, n_rewalk = 0;
  int64_t cur = start;
  if (start < 0) {
    cur = -1;
    // (a guess counts when a chain of eight plausible records hangs on it, or one that reaches the end of the data: bytes
    // that imitate a record or two -- the tests plant such chains of three in the qualities -- are passed over)
    for (int s = 0; s < P.n_seg && cur < 0; ++s) {
      if (sst[s] == 0xffffffffu) continue;
      int64_t c = (int64_t)sst[s];
      bool good = true;
      for (int k = 0; k < 8 && c + kMinRec <= P.hi; ++k) {
        if (!plausible(P.buf, c, P.hi, P.n_ref)) { good = false; break; }
        c += 4 + (int64_t)ld32(P.buf, c);
      }
      if (good) cur = (int64_t)sst[s];
    }
    if (cur >= 0 && start == -2) cur += 4;   // (SVDSS_REGION_TEST=1: a guess that is no record -- the caller's second run is tested)
    hdr[H_START] = cur;
    if (cur < 0) { hdr[H_NREC] = 0; hdr[H_TAIL] = P.hi; hdr[H_ERR] = 0; hdr[H_REWALK] = 0; hdr[H_PRE] = 0; return; }
  } else hdr[H_START] = start;
  int n_pre = 0;
  bool stop = false;    // the chain reached the tail (or nonsense)
  auto step = [&](int64_t p, int64_t& next) -> bool {   // is there a complete record at p?
    if (p + 4 > P.hi) return false;
    const uint32_t bs = ld32(P.buf, p);
    if (bs < 32u) { err |= E_CORRUPT; return false; }
    if (p + 4 + (int64_t)bs > P.hi) return false;
    next = p + 4 + (int64_t)bs;
    return true;
  };
  // records that begin in the carried bytes
  while (!stop && cur < P.lo) {
    int64_t nx;
    if (!step(cur, nx)) { stop = true; break; }
    if (n_pre < 4) pre[n_pre] = (uint32_t)cur;
    else err |= E_CORRUPT;     // (cannot happen: the carry is one incomplete record)
    ++n_pre;
    cur = nx;
  }
  int total = n_pre;
  for (int s = 0; s < P.n_seg; ++s) {
    const int64_t s_lo = P.lo + (int64_t)s * P.seg_bytes;
    int64_t s_hi = s_lo + P.seg_bytes;
    if (s_hi > P.hi || s == P.n_seg - 1) s_hi = P.hi;
    seg_base[s] = total;
    if (stop || cur >= s_hi) { scn[s] = 0; P.seg_cnt[s] = 0; continue; }   // nothing begins here
    if ((int64_t)sst[s] == cur) {
      total += scn[s];
      cur = sen[s];
      if (cur < s_hi) { int64_t nx; (void)step(cur, nx); stop = true; }   // the tail -- or a block_size below 32 (step says which)
      continue;
    }
    // the guess was wrong (or there was none): walk the segment from where the chain really arrives
    ++n_rewalk;
    uint32_t* list = P.lists + (int64_t)s * P.list_cap;
    int cnt = 0;
    while (cur < s_hi) {
      int64_t nx;
      if (!step(cur, nx)) { stop = true; break; }
      list[cnt++] = (uint32_t)cur;
      cur = nx;
    }
    P.seg_cnt[s] = cnt;
    total += cnt;
  }
  hdr[H_NREC] = total;
  hdr[H_TAIL] = cur < P.hi ? cur : P.hi;
  hdr[H_ERR] = err;
  hdr[H_REWALK] = n_rewalk;
  hdr[H_PRE] = n_pre;
}

// ------------------------------------------------------------------ the record gate (svdss_bam_stream_set_regions)
// `--region` / `--regions-file`: a record is IN if tid >= 0 and [pos, bam_endpos) overlaps one of the stream's intervals on
// its reference (bam_endpos as in select_kernel: pos + the CIGAR's reference length, pos + 1 where that is 0).  The records
// that are out leave the chain here, right behind link_kernel: the segments' lists are compacted in place, in order, and the
// counts, bases and totals follow -- so meta_kernel, select_kernel and smooth_meta_kernel (and everything behind them) see
// the batch of a file that holds the records that are in alone.  hdr[H_GATED] counts those that left.
struct GateP {
  const uint8_t* buf;
  uint32_t* lists; int64_t list_cap;
  int32_t* seg_cnt; int32_t* seg_base; uint32_t* pre;
  int32_t n_seg, n_ref;
  const int64_t* reg_off; const int32_t* reg_beg; const int32_t* reg_end;   // per tid: [reg_off[t], reg_off[t + 1]), sorted, disjoint
  int64_t* hdr;
};
constexpr uint32_t kGateLaneCigar = 256;   // CIGARs up to here are summed by the record's own lane, longer ones by the wavefront

__device__ __forceinline__ int64_t cigar_ref_len(uint32_t c) {
  const uint32_t op = c & 15u;
  return (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? (int64_t)(c >> 4) : 0;
}

// block s < n_seg: the records of segment s; block n_seg: those that begin in the carried bytes.  One wavefront: 64 records
// at a time, a lane each; a record whose CIGAR is long is summed by all 64 lanes (coalesced loads, a shuffle reduction), so
// that a CIGAR of tens of thousands of operations does not hold 63 lanes up behind one.
__global__ void __launch_bounds__(64) gate_kernel(GateP G) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int cnt = s < G.n_seg ? G.seg_cnt[s] : (int)(G.hdr[H_PRE] < 4 ? G.hdr[H_PRE] : 4);
  uint32_t* list = s < G.n_seg ? G.lists + (int64_t)s * G.list_cap : G.pre;
  int kept = 0;
  for (int i0 = 0; i0 < cnt; i0 += 64) {
    const bool have = i0 + lane < cnt;
    const uint32_t p32 = have ? list[i0 + lane] : 0u;
    const int64_t p = p32;
    bool in = false, cand = false, longc = false;
    int32_t tid = -1, pos = 0;
    uint32_t n_cig = 0;
    int64_t cg = 0, ref_len = 0;
    if (have) {
      const uint32_t bs = ld32(G.buf, p);
      tid = (int32_t)ld32(G.buf, p + 4); pos = (int32_t)ld32(G.buf, p + 8);
      const uint32_t w3 = ld32(G.buf, p + 12), w4 = ld32(G.buf, p + 16);
      const int32_t l_seq = (int32_t)ld32(G.buf, p + 20);
      const uint32_t l_name = w3 & 0xffu;
      n_cig = w4 & 0xffffu;
      cg = p + 36 + l_name;
      const int64_t head = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)(l_seq < 0 ? 0 : l_seq) + 1) / 2 + (l_seq < 0 ? 0 : l_seq);
      // (a record whose fields do not fit its block_size stays: the kernel behind raises "corrupt record" as it always has,
      // and its CIGAR is not walked)
      if (l_seq < 0 || head > (int64_t)bs) in = true;
      else cand = tid >= 0 && tid < G.n_ref && G.reg_off[tid + 1] > G.reg_off[tid];
      longc = cand && n_cig > kGateLaneCigar;
      if (cand && !longc)
        for (uint32_t k = 0; k < n_cig; ++k) ref_len += cigar_ref_len(ld32(G.buf, cg + 4 * (int64_t)k));
    }
    unsigned long long lm = __ballot(longc);
    while (lm) {
      const int src = __builtin_ctzll(lm);
      lm &= lm - 1;
      const int64_t cg_s = __shfl(cg, src, 64);
      const uint32_t n_s = (uint32_t)__shfl((int)n_cig, src, 64);
      int64_t part = 0;
      for (uint32_t k = lane; k < n_s; k += 64) part += cigar_ref_len(ld32(G.buf, cg_s + 4 * (int64_t)k));
      for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
      if (lane == src) ref_len = part;
    }
    if (cand) {
      const int64_t a_beg = pos, a_end = (int64_t)pos + (ref_len ? ref_len : 1);
      // the first interval that ends behind a_beg overlaps iff it begins before a_end
      const int64_t lo = G.reg_off[tid], hi = G.reg_off[tid + 1];
      int64_t a = lo, b = hi;
      while (a < b) { const int64_t m = (a + b) >> 1; if ((int64_t)G.reg_end[m] > a_beg) b = m; else a = m + 1; }
      in = a < hi && (int64_t)G.reg_beg[a] < a_end;
    }
    // in order, in place: the slot written is never behind the one read (and this pass has read its 64 already)
    const unsigned long long km = __ballot(in);
    if (in) list[kept + __popcll(km & ((1ull << lane) - 1ull))] = p32;
    kept += __popcll(km);
  }
  if (lane == 0) {
    if (s < G.n_seg) G.seg_cnt[s] = kept; else G.hdr[H_PRE] = kept;
    if (cnt > kept) atomicAdd((unsigned long long*)&G.hdr[H_GATED], (unsigned long long)(cnt - kept));
  }
}
// the segments' bases and the batch's total, from the counts gate_kernel left (one wavefront, 64 segments per step)
__global__ void __launch_bounds__(64) gate_base_kernel(GateP G) {
  const int lane = threadIdx.x;
  int run = (int)G.hdr[H_PRE];
  for (int s0 = 0; s0 < G.n_seg; s0 += 64) {
    const int s = s0 + lane;
    const int c = s < G.n_seg ? G.seg_cnt[s] : 0;
    int inc = c;
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(inc, d, 64); if (lane >= d) inc += v; }
    if (s < G.n_seg) G.seg_base[s] = run + inc - c;
    run += __shfl(inc, 63, 64);
  }
  if (lane == 0) G.hdr[H_NREC] = run;
}

// ------------------------------------------------------------------ the index of the input (svdss_bam_stream_set_input_index)
// `SVDSS bamindex`, `call / run --write-bam-index`: the BAI / CSI fragments of the records AS THEY STAND IN THE FILE -- every
// record that starts in this batch's turn, in front of the gate and of every filter -- in the style of the output side's
// sm_ix_* kernels (bam_smooth.hip): a thread per record, hipcub scans for the placements, only chunks and windows come down.
struct InIxP {
  const uint8_t* buf;
  const uint32_t* lists; int64_t list_cap;
  const int32_t* seg_cnt; const int32_t* seg_base; const uint32_t* pre;
  int32_t n_seg;
  int64_t n_rec, n_pre;
  int64_t head, hi;                   // the batch's fresh bytes are buf[head, hi)
  const svdss_bgzf_block_t* blks;     // n_blk members, uoff = where each inflates to in buf
  const int64_t* mstart;              // n_blk + 1: where each begins in the file, from the batch's first; [n_blk]: right behind them
  int64_t n_blk;
  uint64_t pre_v;                     // the virtual offset of the carried bytes' first byte (below the batch's base: wraps)
  int32_t min_shift, depth;
  // per record (n_rec + 1)
  int32_t* tid; uint32_t* bin; int64_t* beg; int64_t* end; uint64_t* vb; uint64_t* ve;
  uint64_t* key;                      // (tid << 32) | (last window + 1): a running maximum of it is the last window reached so far
  const uint64_t* kmax;               // ... exclusive running maximum
  int64_t *head_f, *own, *unm, *idx;  // starts a chunk; windows it reaches into first; flag 4 set; tid >= 0 -- consecutive rows
  const int64_t *s_head, *s_own, *s_unm;
  svdss_bam_input_chunk_t* chunks; svdss_bam_input_window_t* windows;
  unsigned long long* err;            // bit 0: records out of coordinate order, bit 1: a record whose fields do not fit its block_size
};

// the virtual offset of buffer position q, relative to the batch's first member: the member that holds the byte (an empty
// member holds none: it shares its place with the member behind it, which the search below arrives at); a position in the
// carried bytes is the carry's first byte; the end of the batch's last byte is the offset right behind its members
__device__ __forceinline__ uint64_t in_ix_voff(const InIxP& P, int64_t q) {
  if (q < P.head) return P.pre_v;
  if (q >= P.hi || P.n_blk == 0) return (uint64_t)P.mstart[P.n_blk] << 16;
  int64_t a = 0, b = P.n_blk;         // the last member with uoff <= q
  while (b - a > 1) { const int64_t m = (a + b) >> 1; if (P.blks[m].uoff <= q) a = m; else b = m; }
  return ((uint64_t)P.mstart[a] << 16) | (uint64_t)(q - P.blks[a].uoff);
}

// block s < n_seg: the records of segment s; block n_seg: those that begin in the carried bytes.  A thread per record:
// tid, [beg, end) (bam_endpos as gate_kernel has it; a CIGAR kept in a CG tag is read through its <l_seq>S<ref>N stand-in),
// bin, virtual offsets of start and end
__global__ void __launch_bounds__(64) in_ix_rec_kernel(InIxP P) {
  const int s = blockIdx.x;
  const int cnt = s < P.n_seg ? P.seg_cnt[s] : (int)(P.n_pre < 4 ? P.n_pre : 4);
  const int base = s < P.n_seg ? P.seg_base[s] : 0;
  const uint32_t* list = s < P.n_seg ? P.lists + (int64_t)s * P.list_cap : P.pre;
  for (int i = threadIdx.x; i < cnt; i += 64) {
    const int64_t k = base + i;
    if (k >= P.n_rec) continue;
    const int64_t p = list[i];
    const uint32_t bs = ld32(P.buf, p);
    const int32_t tid = (int32_t)ld32(P.buf, p + 4), pos = (int32_t)ld32(P.buf, p + 8);
    const uint32_t w3 = ld32(P.buf, p + 12), w4 = ld32(P.buf, p + 16);
    const int32_t l_seq = (int32_t)ld32(P.buf, p + 20);
    const uint32_t l_name = w3 & 0xffu, n_cig = w4 & 0xffffu, flag = w4 >> 16;
    const int64_t hd = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)(l_seq < 0 ? 0 : l_seq) + 1) / 2 + (l_seq < 0 ? 0 : l_seq);
    int64_t span = 0;
    // (a record whose fields do not fit its block_size is refused by the kernel behind, as always -- svdss_bam_index_run, which
    // has none behind, looks at bit 1 --: its CIGAR is not walked)
    if (l_seq < 0 || hd > (int64_t)bs) atomicOr(P.err, 2ull);
    else {
      const int64_t cg = p + 36 + l_name;
      for (uint32_t j = 0; j < n_cig; ++j) span += cigar_ref_len(ld32(P.buf, cg + 4 * (int64_t)j));
    }
    const bool ix = tid >= 0;
    int64_t beg = 0, end = 1;
    if (ix) ix_extent(pos, span, P.min_shift, P.depth, beg, end);
    P.tid[k] = tid; P.beg[k] = beg; P.end[k] = end;
    P.bin[k] = ix ? ix_reg2bin(beg, end, P.min_shift, P.depth) : 0u;
    P.vb[k] = in_ix_voff(P, p);
    P.ve[k] = in_ix_voff(P, p + 4 + (int64_t)bs);
    P.key[k] = ix ? ((uint64_t)(uint32_t)tid << 32) | (uint64_t)(((end - 1) >> P.min_shift) + 1) : 0ull;
    P.idx[k] = ix ? 1 : 0;
    P.unm[k] = ix && (flag & 4u) ? 1 : 0;
  }
}

// a thread per record (+ the scans' total): its place in the order, does it start a chunk, which windows it reaches into first
__global__ void __launch_bounds__(256) in_ix_own_kernel(InIxP P) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > P.n_rec) return;
  if (k == P.n_rec) { P.head_f[k] = 0; P.own[k] = 0; P.unm[k] = 0; P.idx[k] = 0; return; }
  const int32_t tid = P.tid[k];
  if (k > 0) {   // by tid, then position; a record without a reference sorts behind every reference
    const int32_t pt = P.tid[k - 1];
    const int64_t a = tid < 0 ? 0x7fffffff : tid, b = pt < 0 ? 0x7fffffff : pt;
    if (a < b || (a == b && P.beg[k] < P.beg[k - 1])) atomicOr(P.err, 1ull);
  }
  if (!P.idx[k]) { P.head_f[k] = 0; P.own[k] = 0; return; }
  const uint64_t m = P.kmax[k];
  const int64_t seen = (m >> 32) == (uint64_t)(uint32_t)tid ? (int64_t)(m & 0xffffffffu) - 1 : -1;   // last window reached before
  const int64_t w0 = P.beg[k] >> P.min_shift, w1 = (P.end[k] - 1) >> P.min_shift;
  const int64_t first = w0 > seen + 1 ? w0 : seen + 1;
  P.own[k] = w1 >= first ? w1 - first + 1 : 0;
  P.head_f[k] = (k == 0 || !P.idx[k - 1] || tid != P.tid[k - 1] || P.bin[k] != P.bin[k - 1]) ? 1 : 0;
}

// a thread per record: its chunk's start / end (the counts by two atomics each on zeroed fields of its own chunk) and its windows
__global__ void __launch_bounds__(256) in_ix_emit_kernel(InIxP P) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= P.n_rec || !P.idx[k]) return;
  const int64_t c = P.s_head[k] + P.head_f[k] - 1;
  svdss_bam_input_chunk_t* ch = P.chunks + c;
  if (P.head_f[k]) {
    ch->tid = P.tid[k]; ch->bin = P.bin[k]; ch->v_beg = P.vb[k];
    atomicAdd((unsigned long long*)&ch->n_rec, (unsigned long long)(-k));
    atomicAdd((unsigned long long*)&ch->n_unmapped, (unsigned long long)(-P.s_unm[k]));
  }
  if (k + 1 == P.n_rec || P.head_f[k + 1] || !P.idx[k + 1]) {
    ch->v_end = P.ve[k];
    atomicAdd((unsigned long long*)&ch->n_rec, (unsigned long long)(k + 1));
    atomicAdd((unsigned long long*)&ch->n_unmapped, (unsigned long long)P.s_unm[k + 1]);
  }
  const int64_t n = P.own[k];
  if (n > 0) {
    const int64_t w1 = (P.end[k] - 1) >> P.min_shift;
    svdss_bam_input_window_t* w = P.windows + P.s_own[k];
    for (int64_t j = 0; j < n; ++j) { w[j].tid = P.tid[k]; w[j].window = (int32_t)(w1 - n + 1 + j); w[j].v_beg = P.vb[k]; }
  }
}

// ------------------------------------------------------------------ per record: fields, filters, tags
struct MetaP {
  const uint8_t* buf;
  const uint32_t* lists; int64_t list_cap;
  const int32_t* seg_cnt; const int32_t* seg_base; const uint32_t* pre;
  int32_t n_seg, putative;
  int64_t n_rec;
  uint32_t* rpos;                 // record offsets, in file order
  int64_t *f_pass, *f_srch, *f_name, *f_sym;   // n_rec + 1 each: inputs of the four scans
  int32_t* hp;
  int64_t* hdr;
};

// block s < n_seg: the records of segment s; block n_seg: those that begin in the carried bytes
__global__ void __launch_bounds__(64) meta_kernel(MetaP M) {
  const int s = blockIdx.x;
  const int cnt = s < M.n_seg ? M.seg_cnt[s] : (int)(M.hdr[H_PRE] < 4 ? M.hdr[H_PRE] : 4);
  const int base = s < M.n_seg ? M.seg_base[s] : 0;
  const uint32_t* list = s < M.n_seg ? M.lists + (int64_t)s * M.list_cap : M.pre;
  for (int i = threadIdx.x; i < cnt; i += 64) {
    const int64_t gi = base + i;
    const int64_t p = list[i];
    const uint32_t bs = ld32(M.buf, p);
    const int32_t tid = (int32_t)ld32(M.buf, p + 4);
    const uint32_t w3 = ld32(M.buf, p + 12), w4 = ld32(M.buf, p + 16);
    const int32_t l_seq = (int32_t)ld32(M.buf, p + 20);
    const uint32_t l_name = w3 & 0xffu, n_cig = w4 & 0xffffu, flag = w4 >> 16;
    const int64_t head = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)(l_seq < 0 ? 0 : l_seq) + 1) / 2 + (l_seq < 0 ? 0 : l_seq);
    bool keep = false, srch = false;
    int64_t hp = 0;
    if (l_seq < 0 || head > (int64_t)bs) atomicOr((unsigned long long*)&M.hdr[H_ERR], (unsigned long long)E_CORRUPT);   // BamReader::next_view: "corrupt record"
    else {
      keep = !(flag & (4u | 2048u | 256u));                  // ping_pong.cpp:66-69
      if (keep && l_seq < 100) {                             // :70-75 (the host prints the warnings)
        atomicAdd((unsigned long long*)&M.hdr[H_SHORT], 1ull);
        keep = false;
      }
      if (keep && tid < 0) atomicOr((unsigned long long*)&M.hdr[H_ERR], (unsigned long long)E_TID);   // :76-79
      if (keep) {
        const uint8_t* aux = M.buf + p + 4 + head;
        const uint8_t* end = M.buf + p + 4 + (int64_t)bs;
        int64_t xf = 0;
        (void)aux_int(aux, end, 'X', 'F', xf);               // :196-201, missing => 0
        (void)aux_int(aux, end, 'H', 'P', hp);
        srch = !(M.putative && xf != 0);                     // :202-203
      }
    }
    M.rpos[gi] = (uint32_t)p;
    M.f_pass[gi] = keep ? 1 : 0;
    M.f_srch[gi] = srch ? 1 : 0;
    M.f_name[gi] = keep ? (int64_t)(l_name ? l_name - 1 : 0) : 0;
    M.f_sym[gi] = srch ? (int64_t)l_seq : 0;
    M.hp[gi] = (int32_t)hp;
  }
  if (s == 0 && threadIdx.x == 0) { M.f_pass[M.n_rec] = 0; M.f_srch[M.n_rec] = 0; M.f_name[M.n_rec] = 0; M.f_sym[M.n_rec] = 0; }
}

struct ScatP {
  const uint8_t* buf;
  int64_t n_rec;
  const uint32_t* rpos;
  const int64_t *f_pass, *f_srch;            // the flags
  const int64_t *s_pass, *s_srch, *s_name, *s_sym;   // their exclusive scans (n_rec + 1: the last entry is the total)
  const int32_t* hp;
  int32_t* o_name_off;   // slots + 1
  char* o_names;
  int32_t* o_hp;         // slots
  int32_t* o_sidx;       // slots: index among the searched reads, -1 = not searched (putative filter)
  int64_t* sym_off;      // searched + 1
  int64_t* seq_src;      // searched: where the packed bases sit in buf
  int64_t* totals;       // slots, searched, name bytes, symbols
};

__global__ void __launch_bounds__(256) scatter_kernel(ScatP S) {
  const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi > S.n_rec) return;
  if (gi == S.n_rec) {
    S.o_name_off[S.s_pass[gi]] = (int32_t)S.s_name[gi];
    S.sym_off[S.s_srch[gi]] = S.s_sym[gi];
    S.totals[0] = S.s_pass[gi]; S.totals[1] = S.s_srch[gi]; S.totals[2] = S.s_name[gi]; S.totals[3] = S.s_sym[gi];
    return;
  }
  if (!S.f_pass[gi]) return;
  const int64_t p = S.rpos[gi];
  const uint32_t w3 = ld32(S.buf, p + 12), w4 = ld32(S.buf, p + 16);
  const uint32_t l_name = w3 & 0xffu, n_cig = w4 & 0xffffu;
  const int64_t slot = S.s_pass[gi];
  S.o_name_off[slot] = (int32_t)S.s_name[gi];
  S.o_hp[slot] = S.hp[gi];
  const uint8_t* nm = S.buf + p + 36;
  char* dst = S.o_names + S.s_name[gi];
  for (uint32_t k = 0; k + 1 < l_name; ++k) dst[k] = (char)nm[k];
  if (S.f_srch[gi]) {
    const int64_t k = S.s_srch[gi];
    S.o_sidx[slot] = (int32_t)k;
    S.sym_off[k] = S.s_sym[gi];
    S.seq_src[k] = p + 36 + (int64_t)l_name + 4 * (int64_t)n_cig;
  } else S.o_sidx[slot] = -1;
}

// 4-bit bases -> nt6 (ping_pong.cpp:90-94: seq_nt16_str, then seq_nt6_table): read r = y0 + blockIdx.y, one lane per 16
// ALIGNED output bytes (whole chunks leave as one 16-byte store; the two ends of a read byte by byte)
__global__ void __launch_bounds__(256) unpack_kernel(const uint8_t* __restrict__ buf, const int64_t* __restrict__ seq_src,
                                                     const int64_t* __restrict__ sym_off, int64_t y0, int64_t n_reads, uint8_t* out) {
  const int64_t r = y0 + blockIdx.y;
  if (r >= n_reads) return;
  const int64_t s = sym_off[r], e = sym_off[r + 1];
  const int64_t c = (s >> 4) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t o0 = c << 4;
  if (o0 >= e) return;
  nt6_chunk16(buf, seq_src[r], s, e, o0, out);
}

// ------------------------------------------------------------------ records selected for `call` (svdss_bam_select_run)
struct SelP {
  const uint8_t* buf;
  const uint32_t* lists; int64_t list_cap;
  const int32_t* seg_cnt; const int32_t* seg_base; const uint32_t* pre;
  int32_t n_seg, min_mapq, n_ref;
  int64_t n_rec;
  const uint64_t* hash; uint64_t hash_mask;              // read names wanted (hash == nullptr: no such test)
  const int64_t* reg_off; const int32_t* reg_beg; const int32_t* reg_runmax;   // regions per tid (reg_off == nullptr: none)
  uint32_t* rpos;
  int64_t *f_sel, *f_bytes;       // n_rec + 1 each
  int64_t* hdr;
  // the record store of `SVDSS call` (svdss_bam_store_t): every record that passes the flag / mapq filters, named or not, in
  // its slim form -- f_keep / f_kbytes (n_rec + 1 each; nullptr: no store), hpv: its HP tag (kNoHp: none)
  int64_t *f_keep, *f_kbytes, *hpv;
};

// block s < n_seg: the records of segment s; block n_seg: those that begin in the carried bytes.  A record is kept if it
// passes the flag / mapq filters of clusterer.cpp:118-122 (= :535-540) and, when names and / or regions are given, is
// named in the set or overlaps a region (either is enough: the host looks again, exactly)
__global__ void __launch_bounds__(64) select_kernel(SelP M) {
  const int s = blockIdx.x;
  const int cnt = s < M.n_seg ? M.seg_cnt[s] : (int)(M.hdr[H_PRE] < 4 ? M.hdr[H_PRE] : 4);
  const int base = s < M.n_seg ? M.seg_base[s] : 0;
  const uint32_t* list = s < M.n_seg ? M.lists + (int64_t)s * M.list_cap : M.pre;
  for (int i = threadIdx.x; i < cnt; i += 64) {
    const int64_t gi = base + i;
    const int64_t p = list[i];
    const uint32_t bs = ld32(M.buf, p);
    const int32_t tid = (int32_t)ld32(M.buf, p + 4), pos = (int32_t)ld32(M.buf, p + 8);
    const uint32_t w3 = ld32(M.buf, p + 12), w4 = ld32(M.buf, p + 16);
    const int32_t l_seq = (int32_t)ld32(M.buf, p + 20);
    const uint32_t l_name = w3 & 0xffu, mapq = (w3 >> 8) & 0xffu, n_cig = w4 & 0xffffu, flag = w4 >> 16;
    const int64_t head = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)(l_seq < 0 ? 0 : l_seq) + 1) / 2 + (l_seq < 0 ? 0 : l_seq);
    bool keep = false;
    if (M.f_keep) { M.f_keep[gi] = 0; M.f_kbytes[gi] = 0; }
    if (l_seq < 0 || head > (int64_t)bs) atomicOr((unsigned long long*)&M.hdr[H_ERR], (unsigned long long)E_CORRUPT);
    else {
      keep = call_keeps(flag, mapq, M.min_mapq);
      if (keep && M.f_keep) {
        M.f_keep[gi] = 1;
        M.f_kbytes[gi] = slim_measure(M.buf, p, bs, head, l_seq, M.hpv[gi]);
      }
      if (keep && (M.hash || M.reg_off)) {
        bool hit = M.hash && name_in_set(M.hash, M.hash_mask, M.buf + p + 36, l_name ? l_name - 1 : 0);
        if (!hit && M.reg_off && tid >= 0 && tid < M.n_ref) {
          const int64_t lo = M.reg_off[tid], hi = M.reg_off[tid + 1];
          if (hi > lo) {
            int64_t ref_len = 0;
            const int64_t cg = p + 36 + l_name;
            for (uint32_t k = 0; k < n_cig; ++k) {
              const uint32_t c = ld32(M.buf, cg + 4 * (int64_t)k), op = c & 15u;
              if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += c >> 4;
            }
            const int64_t a_beg = pos, a_end = (int64_t)pos + (ref_len ? ref_len : 1);      // bam_endpos
            // regions sorted by start; runmax = running maximum of their ends: the first one whose running maximum
            // passes a_beg overlaps iff it starts before a_end (csrc/call_host.cpp, fill_clusters)
            int64_t a = lo, b = hi;
            while (a < b) { const int64_t m = (a + b) >> 1; if ((int64_t)M.reg_runmax[m] > a_beg) b = m; else a = m + 1; }
            hit = a < hi && (int64_t)M.reg_beg[a] < a_end;
          }
        }
        keep = hit;
      }
    }
    M.rpos[gi] = (uint32_t)p;
    M.f_sel[gi] = keep ? 1 : 0;
    M.f_bytes[gi] = !keep ? 0 : M.f_keep ? M.f_kbytes[gi] : (((int64_t)bs + 4 + 3) & ~(int64_t)3);   // (with a store: slim, like the stored ones)
  }
  if (s == 0 && threadIdx.x == 0) { M.f_sel[M.n_rec] = 0; M.f_bytes[M.n_rec] = 0; if (M.f_keep) { M.f_keep[M.n_rec] = 0; M.f_kbytes[M.n_rec] = 0; } }
}

// a pass of `SVDSS call` over a stored batch: one lane per slim record, kept if it is named in the filter's set or its
// alignment overlaps a region (either is enough, as in select_kernel: the host looks again, exactly)
struct StoreSelP {
  const uint8_t* recs; const int64_t* off; int64_t n;
  int32_t n_ref;
  const uint64_t* hash; uint64_t hash_mask;              // read names wanted (hash == nullptr: no such test)
  const int64_t* reg_off; const int32_t* reg_beg; const int32_t* reg_runmax;
  int64_t *f_sel, *f_bytes;
};
__global__ void __launch_bounds__(256) store_select_kernel(StoreSelP M) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > M.n) return;
  if (k == M.n) { M.f_sel[k] = 0; M.f_bytes[k] = 0; return; }
  const int64_t p = M.off[k];
  const int32_t tid = (int32_t)ld32(M.recs, p + 4), pos = (int32_t)ld32(M.recs, p + 8);
  const uint32_t w3 = ld32(M.recs, p + 12), w4 = ld32(M.recs, p + 16);
  const uint32_t l_name = w3 & 0xffu, n_cig = w4 & 0xffffu;
  bool hit = M.hash && name_in_set(M.hash, M.hash_mask, M.recs + p + 36, l_name ? l_name - 1 : 0);
  if (!hit && M.reg_off && tid >= 0 && tid < M.n_ref) {
    const int64_t lo = M.reg_off[tid], hi = M.reg_off[tid + 1];
    if (hi > lo) {
      int64_t ref_len = 0;
      const int64_t cg = p + 36 + l_name;
      for (uint32_t i = 0; i < n_cig; ++i) {
        const uint32_t c = ld32(M.recs, cg + 4 * (int64_t)i), op = c & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += c >> 4;
      }
      const int64_t a_beg = pos, a_end = (int64_t)pos + (ref_len ? ref_len : 1);      // bam_endpos
      int64_t a = lo, b = hi;
      while (a < b) { const int64_t m = (a + b) >> 1; if ((int64_t)M.reg_runmax[m] > a_beg) b = m; else a = m + 1; }
      hit = a < hi && (int64_t)M.reg_beg[a] < a_end;
    }
  }
  M.f_sel[k] = hit ? 1 : 0;
  M.f_bytes[k] = hit ? M.off[k + 1] - p : 0;
}
__global__ void __launch_bounds__(64) store_export_kernel(const uint8_t* __restrict__ recs, const int64_t* __restrict__ off, int64_t n,
                                                          const int64_t* __restrict__ f_sel, const int64_t* __restrict__ s_sel,
                                                          const int64_t* __restrict__ s_bytes, uint8_t* out, int64_t* out_off, int64_t* totals) {
  const int64_t k = blockIdx.x;
  if (k == n) {
    if (threadIdx.x == 0) { out_off[s_sel[k]] = s_bytes[k]; totals[0] = s_sel[k]; totals[1] = s_bytes[k]; }
    return;
  }
  if (!f_sel[k]) return;
  const int64_t p = off[k], o = s_bytes[k];
  const uint32_t n4 = (uint32_t)((off[k + 1] - p) / 4);
  if (threadIdx.x == 0) out_off[s_sel[k]] = o;
  const uint32_t* src = (const uint32_t*)(recs + p);
  uint32_t* dst = (uint32_t*)(out + o);
  for (uint32_t i = threadIdx.x; i < n4; i += 64) dst[i] = src[i];
}

// one wavefront per kept record: its bytes (block_size field included) to a 4-aligned place of the output
__global__ void __launch_bounds__(64) export_kernel(const uint8_t* __restrict__ buf, int64_t n_rec, const uint32_t* __restrict__ rpos,
                                                    const int64_t* __restrict__ f_sel, const int64_t* __restrict__ s_sel,
                                                    const int64_t* __restrict__ s_bytes, uint8_t* out, int64_t* out_off, int64_t* totals) {
  const int64_t gi = blockIdx.x;
  if (gi == n_rec) {
    if (threadIdx.x == 0) { out_off[s_sel[gi]] = s_bytes[gi]; totals[0] = s_sel[gi]; totals[1] = s_bytes[gi]; }
    return;
  }
  if (!f_sel[gi]) return;
  const int64_t p = rpos[gi], o = s_bytes[gi];
  const uint32_t n = ld32(buf, p) + 4u;
  if (threadIdx.x == 0) out_off[s_sel[gi]] = o;
  uint32_t* dst = (uint32_t*)(out + o);
  for (uint32_t k = threadIdx.x; k < (n + 3) / 4; k += 64) dst[k] = ld32(buf, p + 4 * (int64_t)k);
}

struct OffDiff {   // length of searched read k
  const int64_t* o;
  __host__ __device__ int64_t operator()(int64_t k) const { return o[k + 1] - o[k]; }
};

}  // namespace

static std::atomic<int64_t> g_gated_total{0};   // records the gate took out, every stream of the process (svdss_bam_gated_total)

struct svdss_bam_filter {
  int device = -1;
  int32_t min_mapq = 0, n_ref = 0;
  uint64_t* d_hash = nullptr;
  uint64_t hash_mask = 0;
  int64_t* d_reg_off = nullptr;
  int32_t *d_reg_beg = nullptr, *d_reg_runmax = nullptr;
};

extern "C" int svdss_bam_stream_create(int32_t n_ref, svdss_bam_stream_t** out) {
  if (!out || n_ref < 0) return SVDSS_EINVAL;
  svdss_bam_stream* s = new (std::nothrow) svdss_bam_stream();
  if (!s) return SVDSS_ENOMEM;
  s->n_ref = n_ref;
  *out = s;
  return SVDSS_OK;
}

extern "C" void svdss_bam_stream_free(svdss_bam_stream_t* s) { delete s; }

extern "C" int svdss_bam_stream_region(svdss_bam_stream_t* s, int32_t open_start, int32_t open_end, const uint8_t* carry, int64_t n_carry) {
  if (!s || n_carry < 0 || (n_carry > 0 && !carry) || (open_start && n_carry > 0)) return SVDSS_EINVAL;
  std::lock_guard<std::mutex> lk(s->m);
  if (s->next_seq != 0) return SVDSS_EINVAL;   // (before the first batch)
  s->open_start = open_start != 0;
  s->open_end = open_end != 0;
  try { s->carry.assign(carry, carry + n_carry); } catch (...) { return SVDSS_ENOMEM; }
  return SVDSS_OK;
}
extern "C" int svdss_bam_stream_set_regions(svdss_bam_stream_t* s, int64_t n, const int32_t* tid, const int32_t* beg, const int32_t* end) {
  if (!s || n < 0 || (n > 0 && (!tid || !beg || !end))) return SVDSS_EINVAL;
  std::lock_guard<std::mutex> lk(s->m);
  if (s->next_seq != 0) return SVDSS_EINVAL;   // (before the first batch)
  try {
    std::vector<int64_t> off((size_t)s->n_ref + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
      if (tid[i] < 0 || tid[i] >= s->n_ref || beg[i] < 0 || end[i] <= beg[i]) return SVDSS_EINVAL;
      // sorted and merged: by reference, then ascending and apart
      if (i > 0 && (tid[i] < tid[i - 1] || (tid[i] == tid[i - 1] && beg[i] < end[i - 1]))) return SVDSS_EINVAL;
      ++off[(size_t)tid[i] + 1];
    }
    for (int32_t t = 0; t < s->n_ref; ++t) off[(size_t)t + 1] += off[(size_t)t];
    s->gate_tab.resize(off.size() * 8 + (size_t)n * 8);
    memcpy(s->gate_tab.data(), off.data(), off.size() * 8);
    if (n > 0) {
      memcpy(s->gate_tab.data() + off.size() * 8, beg, (size_t)n * 4);
      memcpy(s->gate_tab.data() + off.size() * 8 + (size_t)n * 4, end, (size_t)n * 4);
    }
  } catch (...) { return SVDSS_ENOMEM; }
  s->gate_n = n;
  s->gate_on = true;
  return SVDSS_OK;
}
extern "C" int svdss_bam_gated_total(int64_t* out) {
  if (!out) return SVDSS_EINVAL;
  *out = g_gated_total.load();
  return SVDSS_OK;
}
extern "C" int64_t svdss_bam_stream_gated(const svdss_bam_stream_t* s) {
  if (!s) return -1;
  std::lock_guard<std::mutex> lk(const_cast<svdss_bam_stream*>(s)->m);
  return s->n_gated;
}
extern "C" int64_t svdss_bam_stream_head(const svdss_bam_stream_t* s, const uint8_t** bytes) {
  if (!s) return -1;
  if (bytes) *bytes = s->head.data();
  return (int64_t)s->head.size();
}
extern "C" int64_t svdss_bam_stream_tail(const svdss_bam_stream_t* s, const uint8_t** bytes) {
  if (!s) return -1;
  if (bytes) *bytes = s->carry.data();
  return (int64_t)s->carry.size();
}

extern "C" int svdss_bam_stream_set_input_index(svdss_bam_stream_t* s, int32_t min_shift, int32_t depth) {
  if (!s || min_shift < 0 || min_shift > 30 || depth < 0 || (min_shift > 0 && (depth < 1 || min_shift + 3 * depth > 62))) return SVDSS_EINVAL;
  std::lock_guard<std::mutex> lk(s->m);
  if (s->next_seq != 0) return SVDSS_EINVAL;   // (before the first batch)
  s->in_ix_shift = min_shift; s->in_ix_depth = min_shift > 0 ? depth : 0;
  return SVDSS_OK;
}
extern "C" int svdss_bam_stream_set_input_carry(svdss_bam_stream_t* s, int64_t carry_v) {
  if (!s) return SVDSS_EINVAL;
  std::lock_guard<std::mutex> lk(s->m);
  if (s->next_seq != 0) return SVDSS_EINVAL;   // (before the first batch)
  s->carry_coff = carry_v >> 16;               // (below the region's first member: arithmetic shift)
  s->carry_uoff = (int32_t)(carry_v & 0xffff);
  return SVDSS_OK;
}
extern "C" int svdss_bam_stream_input_seam(const svdss_bam_stream_t* s, int32_t* has_carry, int64_t* carry_v, int64_t* head_v) {
  if (!s || !has_carry || !carry_v || !head_v) return SVDSS_EINVAL;
  *has_carry = s->carry.empty() ? 0 : 1;
  *carry_v = (int64_t)(((uint64_t)s->carry_coff << 16) + (uint64_t)s->carry_uoff);
  *head_v = s->head_v;
  return SVDSS_OK;
}
extern "C" int svdss_bam_batch_input_index(const svdss_bam_batch_t* b, svdss_bam_input_frag_t* f) {
  if (!b || !f) return SVDSS_EINVAL;
  *f = b->in_ix.f;
  return SVDSS_OK;
}

extern "C" int svdss_bam_index_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, int32_t device,
                                   int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                   const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                   svdss_bam_batch_t** out) {
  if (!s || !out || seq < 0 || skip < 0 || n_chunks < 0 || device < 0) return SVDSS_EINVAL;
  Front F;
  const int rc = batch_front(s, seq, is_last, skip, device, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, out, F);
  if (rc != SVDSS_OK) return rc;
  svdss_bam_batch* b = *out;
  b->n_records = F.hdr[H_NREC] + F.hdr[H_GATED];
  if (b->in_ix.corrupt) { b->err = "corrupt record"; return SVDSS_EIO; }
  return SVDSS_OK;
}

// ---- the fold of the input index for callers without C++ (BamIndexBuilder, bam_index_writer.h)
struct svdss_bam_input_indexer {
  std::unique_ptr<BamIndexBuilder> b;
  std::vector<uint8_t> bytes;
};
extern "C" int svdss_bam_input_indexer_create(int32_t n_ref, const int32_t* ref_len, int32_t csi, int32_t* min_shift, int32_t* depth,
                                              svdss_bam_input_indexer_t** out) {
  if (!out || n_ref < 0 || (n_ref > 0 && !ref_len) || !min_shift || !depth) return SVDSS_EINVAL;
  try {
    const std::vector<int32_t> lens(ref_len, ref_len + n_ref);
    bool is_csi = false;
    int sh = 0, dp = 0;
    std::string err;
    if (!bam_index_scheme(csi ? "x.csi" : "x.bai", lens, is_csi, sh, dp, err)) { g_svdss_hip_err = err; return SVDSS_ERANGE; }
    svdss_bam_input_indexer* ix = new svdss_bam_input_indexer();
    ix->b.reset(new BamIndexBuilder(n_ref, is_csi, sh, dp));
    *min_shift = sh; *depth = dp;
    *out = ix;
  } catch (...) { return SVDSS_ENOMEM; }
  return SVDSS_OK;
}
extern "C" int svdss_bam_input_indexer_add(svdss_bam_input_indexer_t* ix, const svdss_bam_input_frag_t* f, int64_t base) {
  if (!ix || !f || base < 0 || !f->on) return SVDSS_EINVAL;
  try { ix->b->add_input_fragment(*f, (uint64_t)base); } catch (...) { return SVDSS_ENOMEM; }
  return SVDSS_OK;
}
extern "C" int svdss_bam_input_indexer_finish(svdss_bam_input_indexer_t* ix, int64_t end_offset, const uint8_t** bytes, int64_t* n_bytes) {
  if (!ix || !bytes || !n_bytes || end_offset < 0) return SVDSS_EINVAL;
  ix->b->finish_input((uint64_t)end_offset);
  if (ix->b->unsorted()) { g_svdss_hip_err = "the records are not sorted by coordinate"; return SVDSS_EIO; }
  char* mem = nullptr;
  size_t n = 0;
  FILE* f = open_memstream(&mem, &n);
  if (!f) return SVDSS_ENOMEM;
  const bool ok = ix->b->encode(f);
  if (fclose(f) != 0 || !ok) { free(mem); return SVDSS_EIO; }
  try { ix->bytes.assign((const uint8_t*)mem, (const uint8_t*)mem + n); } catch (...) { free(mem); return SVDSS_ENOMEM; }
  free(mem);
  *bytes = ix->bytes.data(); *n_bytes = (int64_t)ix->bytes.size();
  return SVDSS_OK;
}
extern "C" void svdss_bam_input_indexer_free(svdss_bam_input_indexer_t* ix) { delete ix; }

extern "C" const char* svdss_bam_stream_error(const svdss_bam_stream_t* s) { return s ? s->err.c_str() : ""; }

extern "C" int64_t svdss_bam_stream_rewalked(const svdss_bam_stream_t* s, int64_t* n_segments) {
  if (!s) return -1;
  if (n_segments) *n_segments = s->n_segments;
  return s->n_rewalked;
}

extern "C" void svdss_bam_batch_free(svdss_bam_batch_t* b) {
  if (!b) return;
  if (b->device >= 0) (void)hipSetDevice(b->device);
  if (b->e0) (void)hipEventDestroy(b->e0);
  if (b->e1) (void)hipEventDestroy(b->e1);
  if (b->st) (void)hipStreamDestroy(b->st);
  if (b->search.sfs) svdss_sfs_batch_free(b->search.sfs);
  delete b;   // (its buffers: ~DevBuf / ~PinBuf, on the device made current above)
}

// the gzip header in front of a member's deflate stream at data + coff: 12 + XLEN bytes that begin with 1f 8b 08 and
// FLG.FEXTRA, 18 in every BGZF file anybody writes (0: none found -- the stored blocks of a seam have none)
static inline int64_t member_header_len(const uint8_t* data, int64_t coff) {
  for (int64_t h = 18; h <= coff && h <= 12 + 0xffff; ++h) {
    const uint8_t* q = data + coff - h;
    if (q[0] == 31 && q[1] == 139 && q[2] == 8 && (q[3] & 4) && (int64_t)(q[10] | (q[11] << 8)) == h - 12) return h;
  }
  return 0;
}

int batch_front(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, int device,
                int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                svdss_bam_batch_t** out, Front& F) {
  BatchRun run(*out);
  run.release = [&](int code, const std::string& msg) { pass_turn(s, &svdss_bam_stream::next_seq, seq, code, msg); };
  // SVDSS_BAM_SKIP_RESTART: this batch begins a range of the file of its own -- at a known record start, `skip` bytes into
  // its first member -- behind a gap: what the batch in front carried (the cut record at its range's end) is dropped
  const bool restart = (skip & SVDSS_BAM_SKIP_RESTART) != 0;
  skip &= ~SVDSS_BAM_SKIP_RESTART;
  if (const char* m = bgzf_check_args(n_chunks, comp, comp_bytes, blocks, crc, n_blocks)) return run.fail(SVDSS_EINVAL, m);
  BCHK(hipSetDevice(device));
  RCHK(run.batch_object(out, device));
  svdss_bam_batch* b = run.b;
  const hipStream_t st = run.st;
  b->n_records = b->search.n_slots = b->search.n_searched = b->search.n_short = b->search.total_sfs = 0;
  static const int64_t HEAD = [] {
    const char* e = getenv("SVDSS_BAM_HEADROOM_MB");
    const int64_t mb = e && *e ? atoll(e) : 0;
    return mb > 0 ? mb << 20 : kHeadDefault;
  }();

  // ---- the batch's blocks: compressed bytes back to back, inflated bytes back to back behind the head room
  BgzfIntake& in = b->front.in;
  RCHK(in.plan(n_chunks, comp, comp_bytes, blocks, crc, n_blocks));
  const int64_t total_blocks = in.P.n_blocks, total_inf = in.P.inflated;
  if (HEAD + total_inf + skip >= ((int64_t)1 << 32) - 65536) return run.fail(SVDSS_ERANGE, "batch too large");
  if (skip > total_inf) return run.fail(SVDSS_EIO, "truncated header");
  RCHK(b->front.buf.ensure((size_t)(HEAD + total_inf) + 4096));
  RCHK(b->front.hdr.ensure(sizeof(int64_t) * H_N));
  RCHK(b->front.pre.ensure(64));
  RCHK(b->totals.ensure(64));
  // (the input index's scheme: set before batch 0 and not changed after it, so read without the stream's lock)
  const bool ix_on = s->in_ix_shift > 0;
  b->in_ix.f = svdss_bam_input_frag_t{};
  b->in_ix.corrupt = false;
  if (ix_on) {   // where every member begins in the file, from the batch's first (consecutive members: header, stream, footer)
    b->in_ix.chunks.clear(); b->in_ix.windows.clear();
    try { b->in_ix.h_mstart.assign((size_t)total_blocks + 1, 0); } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
    b->in_ix.f.on = 1; b->in_ix.f.first_data = -1;
    int64_t k = 0, fpos = 0;
    for (int32_t c = 0; c < n_chunks; ++c)
      for (int64_t i = 0; i < n_blocks[c]; ++i, ++k) {
        b->in_ix.h_mstart[(size_t)k] = fpos;
        if (blocks[c][i].isize > 0 && b->in_ix.f.first_data < 0) b->in_ix.f.first_data = fpos;
        fpos += member_header_len(comp[c], blocks[c][i].coff) + blocks[c][i].clen + 8;
      }
    b->in_ix.h_mstart[(size_t)total_blocks] = fpos; b->in_ix.f.comp_bytes = fpos;
    RCHK(b->in_ix.mstart.ensure(sizeof(int64_t) * (size_t)(total_blocks + 1)));
    BCHK(hipMemcpyAsync(b->in_ix.mstart.p, b->in_ix.h_mstart.data(), sizeof(int64_t) * (size_t)(total_blocks + 1), hipMemcpyHostToDevice, st));
  }
  BCHK(hipMemsetAsync(b->front.hdr.p, 0, sizeof(int64_t) * H_N, st));
  // (the gate's intervals: set before batch 0 and not changed after it, so read without the stream's lock)
  const bool gate_on = s->gate_on;
  if (gate_on) {
    RCHK(b->front.gate.ensure(s->gate_tab.size() + 64));
    BCHK(hipMemcpyAsync(b->front.gate.p, s->gate_tab.data(), s->gate_tab.size(), hipMemcpyHostToDevice, st));
  }
  RCHK(in.enqueue(st, b->e0, b->e1, (uint8_t*)b->front.buf.p, HEAD));
  const svdss_bgzf_block_t* const h_blk = in.h_blk();
  // ---- the chain of records, guessed per segment (does not need the carry)
  SegWalk W;
  W.buf = (const uint8_t*)b->front.buf.p;
  W.lo = HEAD + (seq == 0 || restart ? skip : 0);
  W.hi = HEAD + total_inf;
  W.n_ref = s->n_ref;
  {
    int64_t seg_target = (int64_t)256 << 10;
    if (const char* e = getenv("SVDSS_BAM_SEG_KB")) if (atoll(e) > 0) seg_target = atoll(e) << 10;
    const int64_t fresh = W.hi - W.lo;
    int64_t n_seg = (fresh + seg_target - 1) / seg_target;
    n_seg = std::max<int64_t>(1, std::min<int64_t>(kMaxSeg, n_seg));
    W.n_seg = (int32_t)n_seg;
    W.seg_bytes = std::max<int64_t>(64, ((fresh + n_seg - 1) / n_seg + 63) & ~(int64_t)63);
    W.list_cap = W.seg_bytes / kMinRec + 4;
  }
  RCHK(b->front.seg.ensure((size_t)W.n_seg * 16 + 64));
  RCHK(b->front.lists.ensure((size_t)W.n_seg * (size_t)W.list_cap * sizeof(uint32_t)));
  W.seg_start = (uint32_t*)b->front.seg.p;
  W.seg_end = W.seg_start + W.n_seg;
  W.seg_cnt = (int32_t*)(W.seg_end + W.n_seg);
  int32_t* seg_base = W.seg_cnt + W.n_seg;
  W.lists = (uint32_t*)b->front.lists.p;
  hipLaunchKernelGGL(walk_kernel, dim3((unsigned)W.n_seg), dim3(64), 0, st, WalkP{W});
  BCHK(hipGetLastError());
  RCHK(in.enqueue_status_download(st));
  BCHK(hipStreamSynchronize(st));
  const int verdict = in.verdict(b->e0, b->e1, b->inflate_ms);
  run.lap(0);   // buffers, upload, inflate, CRC, segment walk
  RCHK(verdict);

  // ---- this batch's turn: carry in, the chain proved and completed, carry out
  const bool my_turn = wait_turn(s, &svdss_bam_stream::next_seq, seq);
  run.release = nullptr;   // (taken, or let through by a stream that failed: nothing to pass on any more)
  if (!my_turn) return run.fail(s->failed, s->err);
  run.lap(1);   // waiting for the turn
  int turn_code = SVDSS_OK;
  std::string turn_msg;
  int64_t hdr[H_N] = {0};
  uint64_t ix_pre_v = 0;     // (input index) where the carry that goes in begins in the file, relative to this batch's first member
  // (input index) the virtual offset of buffer position q >= HEAD as in_ix_voff has it, in its two parts
  auto host_voff = [&](int64_t q, int64_t& c_off, int32_t& u_off) {
    const std::vector<int64_t>& ms = b->in_ix.h_mstart;
    if (q >= W.hi || total_blocks == 0) { c_off = ms[(size_t)total_blocks]; u_off = 0; return; }
    int64_t lo = 0, hi2 = total_blocks;
    while (hi2 - lo > 1) { const int64_t m = (lo + hi2) >> 1; if (h_blk[m].uoff <= q) lo = m; else hi2 = m; }
    c_off = ms[(size_t)lo]; u_off = (int32_t)(q - h_blk[lo].uoff);
  };
  {
    const int64_t carry_len = restart && seq > 0 ? 0 : (int64_t)s->carry.size();
    auto turn_fail = [&](int code, const std::string& msg) { turn_code = code; turn_msg = msg; };
    hipError_t e = hipSuccess;
    if (carry_len > HEAD) turn_fail(SVDSS_ERANGE, "a record larger than the head room (SVDSS_BAM_HEADROOM_MB)");
    if (!turn_code && carry_len > 0)
      e = hipMemcpyAsync((uint8_t*)b->front.buf.p + (HEAD - carry_len), s->carry.data(), (size_t)carry_len, hipMemcpyHostToDevice, st);
    if (!turn_code && e == hipSuccess) {
      // (SVDSS_REGION_TEST, for the tests of the caller's second run: 1 = start at a guess that is no record, 2 = a head one byte short)
      static const int region_test = getenv("SVDSS_REGION_TEST") ? atoi(getenv("SVDSS_REGION_TEST")) : 0;
      const int64_t start = seq == 0 && s->open_start ? (region_test == 1 ? -2 : -1) : (seq == 0 || restart) && carry_len == 0 ? W.lo : HEAD - carry_len;
      hipLaunchKernelGGL(link_kernel, dim3(1), dim3(64), 0, st, WalkP{W}, start, (uint32_t*)b->front.pre.p, seg_base, (int64_t*)b->front.hdr.p);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(hdr, b->front.hdr.p, sizeof hdr, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e == hipSuccess) {
        if (hdr[H_ERR] & E_CORRUPT) turn_fail(SVDSS_EIO, "truncated record");   // (a block_size below 32: BamReader says the same)
        else if (start < 0 && hdr[H_START] < 0) turn_fail(SVDSS_EIO, "no record found at the start of the region");
        else {
          if (start < 0) {   // the region's bytes in front of its first record: the end of the previous region's last one
            const int64_t head_len = std::max<int64_t>(0, hdr[H_START] - W.lo - (region_test == 2 ? 1 : 0));
            try { s->head.resize((size_t)head_len); } catch (...) { turn_fail(SVDSS_ENOMEM, "out of memory"); }
            if (!turn_code && head_len > 0) {
              e = hipMemcpyAsync(s->head.data(), (const uint8_t*)b->front.buf.p + W.lo, (size_t)head_len, hipMemcpyDeviceToHost, st);
              if (e == hipSuccess) e = hipStreamSynchronize(st);
            }
          }
          const int64_t tail = hdr[H_TAIL], tail_len = W.hi - tail;
          if (ix_on) {
            // the carry that goes in began where the stream remembers; the one that goes out begins in this batch's members, or
            // is the same record still (one longer than the batch): either way relative to the NEXT batch's first member
            ix_pre_v = ((uint64_t)s->carry_coff << 16) + (uint64_t)s->carry_uoff;
            const int64_t span = b->in_ix.f.comp_bytes;
            if (tail_len > 0 && tail >= HEAD) { host_voff(tail, s->carry_coff, s->carry_uoff); s->carry_coff -= span; }
            else if (tail_len > 0) s->carry_coff -= span;
            else { s->carry_coff = 0; s->carry_uoff = 0; }
            if (start < 0) { int64_t c0 = 0; int32_t u0 = 0; host_voff(hdr[H_START], c0, u0); s->head_v = (int64_t)(((uint64_t)c0 << 16) | (uint64_t)u0); }
            b->in_ix.f.ends_at_boundary = tail_len == 0 ? 1 : 0;      // (of the last record, if there is one: below)
          }
          try { s->carry.resize((size_t)tail_len); } catch (...) { turn_fail(SVDSS_ENOMEM, "out of memory"); }
          if (!turn_code && tail_len > 0) {
            e = hipMemcpyAsync(s->carry.data(), (const uint8_t*)b->front.buf.p + tail, (size_t)tail_len, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
          }
          if (!turn_code && is_last && tail_len > 0 && !s->open_end) turn_fail(SVDSS_EIO, "truncated record");
          s->n_rewalked += hdr[H_REWALK];
          s->n_segments += W.n_seg;
        }
      }
    }
    if (e != hipSuccess && !turn_code) {
      g_svdss_hip_err = std::string("bam batch turn: ") + hipGetErrorString(e);
      turn_fail(e == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP, g_svdss_hip_err);
    }
  }
  done_turn(s, &svdss_bam_stream::next_seq, turn_code, turn_msg);
  if (turn_code) { b->err = turn_msg; return turn_code; }
  // ---- the index of the input, outside the turn and in front of the gate: every record of the chain as link_kernel left it
  if (ix_on) {
    svdss_bam_input_frag_t& f = b->in_ix.f;
    const int64_t n = hdr[H_NREC];
    f.n_records = n;
    if (n == 0) f.ends_at_boundary = 0;
    else {
      const size_t n1 = (size_t)n + 1;
      RCHK(b->in_ix.rec.ensure(8 + 8 * 14 * n1 + 8 * n1 + 256));
      InIxP P;
      P.buf = W.buf; P.lists = W.lists; P.list_cap = W.list_cap; P.seg_cnt = W.seg_cnt; P.seg_base = seg_base; P.pre = (const uint32_t*)b->front.pre.p;
      P.n_seg = W.n_seg; P.n_rec = n; P.n_pre = hdr[H_PRE];
      P.head = HEAD; P.hi = W.hi;
      P.blks = (const svdss_bgzf_block_t*)in.blks.p; P.mstart = (const int64_t*)b->in_ix.mstart.p; P.n_blk = total_blocks;
      P.pre_v = ix_pre_v; P.min_shift = s->in_ix_shift; P.depth = s->in_ix_depth;
      int64_t* i64 = (int64_t*)b->in_ix.rec.p;
      unsigned long long* d_err = (unsigned long long*)i64;    // 8 bytes, then the per-record arrays
      P.err = d_err;
      P.beg = i64 + 1; P.end = P.beg + n1;
      P.head_f = P.end + n1; P.own = P.head_f + n1; P.unm = P.own + n1; P.idx = P.unm + n1;       // four rows in, four rows out
      int64_t* s_head = P.idx + n1; int64_t* s_own = s_head + n1; int64_t* s_unm = s_own + n1; int64_t* s_idx = s_unm + n1;
      P.s_head = s_head; P.s_own = s_own; P.s_unm = s_unm;
      P.vb = (uint64_t*)(s_idx + n1); P.ve = P.vb + n1; P.key = P.ve + n1;
      uint64_t* kmax = P.key + n1;
      P.kmax = kmax;
      P.tid = (int32_t*)(kmax + n1); P.bin = (uint32_t*)(P.tid + n1);
      P.chunks = nullptr; P.windows = nullptr;
      const unsigned g = (unsigned)((n + 1 + 255) / 256);
      BCHK(hipMemsetAsync(d_err, 0, 8, st));
      hipLaunchKernelGGL(in_ix_rec_kernel, dim3((unsigned)W.n_seg + 1), dim3(64), 0, st, P);
      BCHK(hipGetLastError());
      {
        size_t t0 = 0, t1 = 0;
        BCHK(hipcub::DeviceScan::ExclusiveScan(nullptr, t0, P.key, kmax, hipcub::Max(), (uint64_t)0, (int)n, st));
        BCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, P.head_f, s_head, (int)n1, st));
        RCHK(run.scan_tmp(std::max(t0, t1)));   // (room for the sums below as well: nothing is allocated between the kernels)
        t0 = b->tmp.cap;
        BCHK(hipcub::DeviceScan::ExclusiveScan(b->tmp.p, t0, P.key, kmax, hipcub::Max(), (uint64_t)0, (int)n, st));
        hipLaunchKernelGGL(in_ix_own_kernel, dim3(g), dim3(256), 0, st, P);
        BCHK(hipGetLastError());
        RCHK(run.scan_rows(P.head_f, s_head, (int64_t)n1, 4));
      }
      // counts, order flag, the first and last record's (tid, beg)
      int64_t cnt[3] = {0, 0, 0}, be[2] = {0, 0};
      int32_t td[2] = {0, 0};
      unsigned long long h_err = 0;
      BCHK(hipMemcpyAsync(&cnt[0], s_head + n, 8, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(&cnt[1], s_own + n, 8, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(&cnt[2], s_idx + n, 8, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(&h_err, d_err, 8, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(&td[0], P.tid, 4, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(&td[1], P.tid + (n - 1), 4, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(&be[0], P.beg, 8, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(&be[1], P.beg + (n - 1), 8, hipMemcpyDeviceToHost, st));
      BCHK(hipStreamSynchronize(st));
      f.first_tid = td[0]; f.last_tid = td[1]; f.first_beg = be[0]; f.last_beg = be[1];
      f.n_no_coor = n - cnt[2];
      if (td[1] < 0) f.ends_at_boundary = 0;       // (a record without a reference has no chunk whose end could wait)
      b->in_ix.corrupt = (h_err & 2) != 0;
      if (h_err & 1) f.unsorted = 1;               // out of order: the builder refuses; nothing else comes down
      else {
        const int64_t n_ch = cnt[0], n_win = cnt[1];
        const size_t ch_bytes = sizeof(svdss_bam_input_chunk_t) * (size_t)n_ch;
        RCHK(b->in_ix.frag.ensure(ch_bytes + sizeof(svdss_bam_input_window_t) * (size_t)n_win + 512));
        P.chunks = (svdss_bam_input_chunk_t*)b->in_ix.frag.p;
        P.windows = (svdss_bam_input_window_t*)((uint8_t*)b->in_ix.frag.p + ((ch_bytes + 255) & ~(size_t)255));
        try { b->in_ix.chunks.resize((size_t)n_ch); b->in_ix.windows.resize((size_t)n_win); } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
        if (n_ch) BCHK(hipMemsetAsync(P.chunks, 0, ch_bytes, st));
        hipLaunchKernelGGL(in_ix_emit_kernel, dim3(g), dim3(256), 0, st, P);
        BCHK(hipGetLastError());
        if (n_ch) BCHK(hipMemcpyAsync(b->in_ix.chunks.data(), P.chunks, ch_bytes, hipMemcpyDeviceToHost, st));
        if (n_win) BCHK(hipMemcpyAsync(b->in_ix.windows.data(), P.windows, sizeof(svdss_bam_input_window_t) * (size_t)n_win, hipMemcpyDeviceToHost, st));
        BCHK(hipStreamSynchronize(st));
        f.n_chunks = n_ch; f.chunks = b->in_ix.chunks.data();
        f.n_windows = n_win; f.windows = b->in_ix.windows.data();
      }
    }
  }
  // ---- the record gate, outside the turn (it needs nothing of the batches in front): the chain loses the records outside
  // the stream's regions before any front end looks at it
  if (gate_on && hdr[H_NREC] > 0) {
    GateP G;
    G.buf = W.buf; G.lists = W.lists; G.list_cap = W.list_cap; G.seg_cnt = W.seg_cnt; G.seg_base = seg_base; G.pre = (uint32_t*)b->front.pre.p;
    G.n_seg = W.n_seg; G.n_ref = s->n_ref;
    G.reg_off = (const int64_t*)b->front.gate.p;
    G.reg_beg = (const int32_t*)(G.reg_off + (s->n_ref + 1)); G.reg_end = G.reg_beg + s->gate_n;
    G.hdr = (int64_t*)b->front.hdr.p;
    hipLaunchKernelGGL(gate_kernel, dim3((unsigned)W.n_seg + 1), dim3(64), 0, st, G);
    BCHK(hipGetLastError());
    hipLaunchKernelGGL(gate_base_kernel, dim3(1), dim3(64), 0, st, G);
    BCHK(hipGetLastError());
    BCHK(hipMemcpyAsync(hdr, b->front.hdr.p, sizeof hdr, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    std::lock_guard<std::mutex> lk(s->m);
    s->n_gated += hdr[H_GATED];
    g_gated_total.fetch_add(hdr[H_GATED], std::memory_order_relaxed);
  }
  run.lap(2);   // the turn: carry in, link, carry out (and the gate)
  F.W = W; F.seg_base = seg_base; F.total_inf = total_inf; F.HEAD = HEAD;
  memcpy(F.hdr, hdr, sizeof hdr);
  return SVDSS_OK;
}

__global__ void __launch_bounds__(256) rebase_offsets_kernel(const int64_t* __restrict__ in, int64_t n, int64_t base, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i] + base;
}

// ---- the park (see struct svdss_bam_park)
extern "C" int svdss_bam_park_create(int32_t device, int64_t read_bytes, int64_t max_reads, svdss_bam_park_t** out) {
  if (!out || device < 0 || read_bytes < 4096 || max_reads < 1) return SVDSS_EINVAL;
  HIPCHK(hipSetDevice(device));
  svdss_bam_park* p = new (std::nothrow) svdss_bam_park();
  if (!p) return SVDSS_ENOMEM;
  p->device = device;
  if (const char* e = getenv("SVDSS_PARK_GROUP_READS")) if (atoll(e) > 0) p->group_reads = atoll(e);
  if (const char* e = getenv("SVDSS_PARK_GROUP_MB")) if (atoll(e) > 0) p->group_bytes = atoll(e) << 20;
  if (const char* e = getenv("SVDSS_PARK_ARENA_MB")) if (atoll(e) > 0) p->arena_bytes = atoll(e) << 20;
  p->max_bytes = read_bytes;
  p->arena_bytes = std::min(p->arena_bytes, read_bytes);
  p->group_bytes = std::min(p->group_bytes, p->arena_bytes / 2);
  p->reads_per_arena = std::max<int64_t>(1024, (int64_t)((double)max_reads * (double)p->arena_bytes / (double)read_bytes) + 1);
  hipError_t e = park_new_arena(p);
  if (e == hipSuccess) e = svdss_make_stream(&p->st, "SVDSS_SEARCH_CUS");
  if (e != hipSuccess) {
    g_svdss_hip_err = std::string("svdss_bam_park_create: ") + hipGetErrorString(e);
    svdss_bam_park_free(p);
    return e == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP;
  }
  *out = p;
  return SVDSS_OK;
}

extern "C" void svdss_bam_park_free(svdss_bam_park_t* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->st) (void)hipStreamDestroy(p->st);
  for (ParkArena& A : p->arenas) { if (A.d_reads) (void)hipFree(A.d_reads); if (A.d_off) (void)hipFree(A.d_off); }
  delete p;
}

// no more reservations: the open group is closed (the index is resident; batches go straight to the search from here on)
extern "C" int svdss_bam_park_close(svdss_bam_park_t* p) {
  if (!p) return SVDSS_EINVAL;
  { std::lock_guard<std::mutex> lk(p->m); p->closed = true; if (!p->groups.empty()) p->groups.back().closed = true; }
  p->cv.notify_all();
  return SVDSS_OK;
}

extern "C" int64_t svdss_bam_park_groups(svdss_bam_park_t* p) {
  if (!p) return -1;
  std::lock_guard<std::mutex> lk(p->m);
  return (int64_t)p->groups.size();
}

// 1: group g is closed and all its batches have unpacked (svdss_bam_park_search would not wait); 0: not yet, or no such group
extern "C" int32_t svdss_bam_park_group_ready(svdss_bam_park_t* p, int64_t g) {
  if (!p || g < 0) return 0;
  std::lock_guard<std::mutex> lk(p->m);
  return g < (int64_t)p->groups.size() && p->groups[(size_t)g].closed && p->groups[(size_t)g].pending == 0 ? 1 : 0;
}

extern "C" int svdss_bam_park_group(svdss_bam_park_t* p, int64_t g, int64_t* n_batches, int64_t* n_reads, int64_t* n_syms) {
  if (!p || g < 0) return SVDSS_EINVAL;
  std::lock_guard<std::mutex> lk(p->m);
  if (g >= (int64_t)p->groups.size()) return SVDSS_EINVAL;
  const ParkGroup& G = p->groups[(size_t)g];
  if (n_batches) *n_batches = G.n_batches;
  if (n_reads) *n_reads = G.n_reads;
  if (n_syms) *n_syms = G.n_syms;
  return SVDSS_OK;
}

// One group searched as ONE launch (one lane per read: the large-batch regime).  Waits until the group is closed and all
// its batches have unpacked; results with svdss_sfs_batch_fetch (reads in reservation order).
extern "C" int svdss_bam_park_search(svdss_bam_park_t* p, int64_t g, const svdss_index_t* ix, int32_t flags, svdss_sfs_batch_t** sfs) {
  if (!p || !ix || !sfs || g < 0) return SVDSS_EINVAL;
  if (ix->device != p->device || !ix->d_blocks) return SVDSS_ENODEV;
  ParkGroup G;
  {
    std::unique_lock<std::mutex> lk(p->m);
    if (g >= (int64_t)p->groups.size()) return SVDSS_EINVAL;
    p->cv.wait(lk, [&] { return p->groups[(size_t)g].closed && p->groups[(size_t)g].pending == 0; });
    G = p->groups[(size_t)g];
  }
  HIPCHK(hipSetDevice(p->device));
  // (the bytes behind the last read up to the end of its 16-byte chunk and one chunk more: what a batch's own buffer has zeroed)
  const ParkArena A = [&] { std::lock_guard<std::mutex> lk(p->m); return p->arenas[(size_t)G.arena]; }();
  HIPCHK(hipMemsetAsync(A.d_reads + G.sym0 + G.n_syms, 0, (size_t)((((G.n_syms + 15) & ~(int64_t)15) + 16) - G.n_syms), p->st));
  const int rc = svdss_sfs_search_batch_device(ix, A.d_reads + G.sym0, A.d_off + G.off0, G.n_reads, G.n_syms, flags & SVDSS_SFS_ASSEMBLE, (void*)p->st, sfs);
  if (rc != SVDSS_OK) return rc;
  HIPCHK(hipStreamSynchronize(p->st));
  return SVDSS_OK;
}

// The front half of svdss_bam_batch_run: inflate, CRC, record chain, the turn, fields / filters / tags, bases unpacked --
// into `park` when one is given and has room (svdss_bam_batch_parked says where), else into the batch object.  Names, tags
// and slots of the batch are on the host when it returns (svdss_bam_batch_result; counts / SFS after the search).
extern "C" int svdss_bam_batch_front(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, int32_t device, svdss_bam_park_t* park,
                                     int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                     const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                     int32_t flags, svdss_bam_batch_t** out) {
  if (!s || !out || seq < 0 || skip < 0 || n_chunks < 0 || device < 0) return SVDSS_EINVAL;
  if (park && park->device != device) return SVDSS_EINVAL;
  if (*out) (*out)->search.front_done = false;
  Front F;
  {
    const int rc = batch_front(s, seq, is_last, skip, device, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, out, F);
    if (rc != SVDSS_OK) return rc;
  }
  svdss_bam_batch* b = *out;
  BatchRun run(b);
  const hipStream_t st = run.st;
  const SegWalk& W = F.W;
  int32_t* seg_base = F.seg_base;
  const int64_t* hdr = F.hdr;
  const int64_t total_inf = F.total_inf, HEAD = F.HEAD;
  int64_t pg = -1, pfirst = 0, psym = 0;      // the park's group this batch reserved room in (-1: none)
  auto unpark = [&]() { if (pg >= 0) { park_done(park, pg); pg = -1; } };
  run.release = [&](int, const std::string&) { unpark(); };   // (a failure must not leave the group waiting for this batch)

  // ---- fields, filters, tags; where everything goes
  const int64_t n_rec = hdr[H_NREC];
  b->n_records = n_rec + hdr[H_GATED];   // (the records the gate took out of the chain are records of the batch)
  RCHK(b->rpos.ensure(sizeof(uint32_t) * (size_t)(n_rec + 1)));
  RCHK(b->flags.ensure(sizeof(int64_t) * 4 * (size_t)(n_rec + 1)));
  RCHK(b->scans.ensure(sizeof(int64_t) * 4 * (size_t)(n_rec + 1)));
  RCHK(b->search.d_hp.ensure(sizeof(int32_t) * (size_t)(n_rec + 1)));
  MetaP M;
  M.buf = W.buf; M.lists = W.lists; M.list_cap = W.list_cap; M.seg_cnt = W.seg_cnt; M.seg_base = seg_base; M.pre = (const uint32_t*)b->front.pre.p;
  M.n_seg = W.n_seg; M.putative = (flags & SVDSS_BAM_PUTATIVE) ? 1 : 0; M.n_rec = n_rec;
  M.rpos = (uint32_t*)b->rpos.p;
  M.f_pass = (int64_t*)b->flags.p; M.f_srch = M.f_pass + (n_rec + 1); M.f_name = M.f_srch + (n_rec + 1); M.f_sym = M.f_name + (n_rec + 1);
  M.hp = (int32_t*)b->search.d_hp.p; M.hdr = (int64_t*)b->front.hdr.p;
  hipLaunchKernelGGL(meta_kernel, dim3((unsigned)W.n_seg + 1), dim3(64), 0, st, M);
  BCHK(hipGetLastError());
  int64_t* sc = (int64_t*)b->scans.p;
  RCHK(run.scan_rows(M.f_pass, sc, n_rec + 1, 4));
  // (sizes of the outputs are not known yet: bounded by the records / the inflated bytes)
  RCHK(b->search.o_small.ensure(sizeof(int32_t) * 3 * (size_t)(n_rec + 2)));
  RCHK(b->search.d_names.ensure((size_t)n_rec * 255 + 64 < (size_t)total_inf + (size_t)HEAD ? (size_t)n_rec * 255 + 64 : (size_t)total_inf + (size_t)HEAD + 64));
  RCHK(b->search.sym_off.ensure(sizeof(int64_t) * (size_t)(n_rec + 2)));
  RCHK(b->search.seq_src.ensure(sizeof(int64_t) * (size_t)(n_rec + 2)));
  ScatP S;
  S.buf = W.buf; S.n_rec = n_rec; S.rpos = M.rpos; S.f_pass = M.f_pass; S.f_srch = M.f_srch;
  S.s_pass = sc; S.s_srch = sc + (n_rec + 1); S.s_name = sc + 2 * (n_rec + 1); S.s_sym = sc + 3 * (n_rec + 1);
  S.hp = M.hp;
  S.o_name_off = (int32_t*)b->search.o_small.p; S.o_hp = S.o_name_off + (n_rec + 2); S.o_sidx = S.o_hp + (n_rec + 2);
  S.o_names = (char*)b->search.d_names.p; S.sym_off = (int64_t*)b->search.sym_off.p; S.seq_src = (int64_t*)b->search.seq_src.p;
  S.totals = (int64_t*)b->totals.p;
  hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((n_rec + 1 + 255) / 256)), dim3(256), 0, st, S);
  BCHK(hipGetLastError());
  int64_t totals[4] = {0, 0, 0, 0}, hdr2[H_N] = {0};
  BCHK(hipMemcpyAsync(totals, b->totals.p, sizeof totals, hipMemcpyDeviceToHost, st));
  BCHK(hipMemcpyAsync(hdr2, b->front.hdr.p, sizeof hdr2, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  run.lap(3);   // fields / filters / tags, scans, scatter
  if (const char* bad = record_error(hdr2[H_ERR])) return run.fail(SVDSS_EIO, bad);
  const int64_t n_slots = totals[0], n_srch = totals[1], name_bytes = totals[2], total_syms = totals[3];
  b->search.n_slots = n_slots; b->search.n_searched = n_srch; b->search.n_short = hdr2[H_SHORT];
  if (total_syms >= ((int64_t)1 << 40)) return run.fail(SVDSS_ERANGE, "batch too large");

  // ---- bases, search
  const size_t padded = (size_t)((total_syms + 15) & ~(int64_t)15) + 16;
  b->search.park_group = n_srch > 0 ? -1 : -2;
  b->search.park_first = 0;
  uint8_t* reads_out = nullptr;
  const int64_t* off_out = (const int64_t*)S.sym_off;
  if (n_srch > 0 && park && park_reserve(park, n_srch, total_syms, pg, pfirst, psym)) {
    // the reads go behind those of the batches that reserved before this one; the offsets are the group's
    ParkArena A;
    const ParkGroup G = [&] { std::lock_guard<std::mutex> lk(park->m); A = park->arenas[(size_t)park->groups[(size_t)pg].arena]; return park->groups[(size_t)pg]; }();
    reads_out = A.d_reads + G.sym0;
    int64_t* po = A.d_off + G.off0 + pfirst;
    hipLaunchKernelGGL(rebase_offsets_kernel, dim3((unsigned)((n_srch + 1 + 255) / 256)), dim3(256), 0, st, (const int64_t*)S.sym_off, n_srch + 1, psym, po);
    off_out = po;
    b->search.park_group = pg; b->search.park_first = pfirst;
    BCHK(hipGetLastError());
  } else {
    RCHK(b->search.reads.ensure(padded + 16));
    reads_out = (uint8_t*)b->search.reads.p;
  }
  if (n_srch > 0) {
    if (b->search.park_group < 0) BCHK(hipMemsetAsync((uint8_t*)b->search.reads.p + (padded >= 32 ? padded - 32 : 0), 0, padded >= 32 ? 32 : padded, st));
    // (the longest read decides the grid's width: the scan's inputs hold the lengths, the host does not -- bounded by
    // the largest record of the batch, i.e. by the batch itself; a second pass over the symbol offsets would cost more)
    int64_t max_len = 0;
    {
      // longest searched read = max over k of sym_off[k + 1] - sym_off[k]: one small reduction
      size_t tb = 0;
      hipcub::CountingInputIterator<int64_t> cnt(0);
      hipcub::TransformInputIterator<int64_t, OffDiff, hipcub::CountingInputIterator<int64_t>> it(cnt, OffDiff{S.sym_off});
      int64_t* d_max = (int64_t*)b->totals.p + 4;
      BCHK(hipcub::DeviceReduce::Max(nullptr, tb, it, d_max, (int)n_srch, st));
      RCHK(run.scan_tmp(tb));
      tb = b->tmp.cap;
      BCHK(hipcub::DeviceReduce::Max(b->tmp.p, tb, it, d_max, (int)n_srch, st));
      BCHK(hipMemcpyAsync(&max_len, d_max, sizeof max_len, hipMemcpyDeviceToHost, st));
      BCHK(hipStreamSynchronize(st));
    }
    if (max_len >= (int64_t)0x7fffffff) return run.fail(SVDSS_ERANGE, "read too long");
    if (max_len > 0) {
      const unsigned gx = (unsigned)((max_len + 15 + 256 * 16 - 1) / (256 * 16) + 1);
      for (int64_t y0 = 0; y0 < n_srch; y0 += 65535) {
        const unsigned gy = (unsigned)std::min<int64_t>(65535, n_srch - y0);
        hipLaunchKernelGGL(unpack_kernel, dim3(gx, gy), dim3(256), 0, st, W.buf, (const int64_t*)S.seq_src, off_out, y0, n_srch, reads_out);
      }
      BCHK(hipGetLastError());
    }
  }
  // ---- what the host needs of the slots: names and tags
  b->search.name_bytes = name_bytes;
  try {
    b->search.name_off.resize((size_t)n_slots + 1); b->search.hp.resize((size_t)n_slots); b->search.sidx.resize((size_t)n_slots);
    b->search.names.resize((size_t)name_bytes + 1); b->search.counts.clear(); b->search.qs.clear(); b->search.len.clear();
  } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
  {
    hipError_t e = hipMemcpyAsync(b->search.name_off.data(), S.o_name_off, sizeof(int32_t) * (size_t)(n_slots + 1), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && n_slots > 0) e = hipMemcpyAsync(b->search.hp.data(), S.o_hp, sizeof(int32_t) * (size_t)n_slots, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && n_slots > 0) e = hipMemcpyAsync(b->search.sidx.data(), S.o_sidx, sizeof(int32_t) * (size_t)n_slots, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && name_bytes > 0) e = hipMemcpyAsync(b->search.names.data(), S.o_names, (size_t)name_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    unpark();     // (the unpack has run: the group may be searched)
    if (e != hipSuccess) { g_svdss_hip_err = std::string("bam batch front: ") + hipGetErrorString(e); return run.fail(e == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP, g_svdss_hip_err); }
  }
  run.lap(4);   // unpack; names and tags down
  b->search.cur_reads = reads_out; b->search.cur_off = off_out; b->search.cur_syms = total_syms; b->search.cur_flags = flags;
  b->stage_ms[5] = b->stage_ms[6] = 0;
  b->search.front_done = true;
  return SVDSS_OK;
}

extern "C" int svdss_bam_batch_parked(const svdss_bam_batch_t* b, int64_t* group, int64_t* first, int64_t* n_reads) {
  if (!b || !b->search.front_done) return SVDSS_EINVAL;
  if (group) *group = b->search.park_group;
  if (first) *first = b->search.park_first;
  if (n_reads) *n_reads = b->search.n_searched;
  return SVDSS_OK;
}

// The search half, for a batch whose front half left the reads in the batch object (not parked): search, counts and SFS down.
extern "C" int svdss_bam_batch_search(svdss_bam_batch_t* b, const svdss_index_t* ix) {
  if (!b || !ix || !b->search.front_done || b->search.park_group >= 0) return SVDSS_EINVAL;
  if (ix->device != b->device || !ix->d_blocks) return SVDSS_ENODEV;
  BatchRun run(b);
  const hipStream_t st = run.st;
  const int32_t flags = b->search.cur_flags;
  const int64_t n_srch = b->search.n_searched, total_syms = b->search.cur_syms;
  BCHK(hipSetDevice(b->device));
  b->search.front_done = false;
  {
    const int rc = svdss_sfs_search_batch_device(ix, b->search.cur_reads, b->search.cur_off, n_srch, total_syms,
                                                 (flags & SVDSS_SFS_ASSEMBLE), (void*)st, &b->search.sfs);
    if (rc != SVDSS_OK) return run.fail(rc, std::string("search: ") + svdss_last_hip_error());
  }
  run.lap(5);   // search
  b->search.total_sfs = svdss_sfs_batch_total(b->search.sfs);
  try {
    b->search.counts.resize((size_t)n_srch); b->search.qs.resize((size_t)b->search.total_sfs); b->search.len.resize((size_t)b->search.total_sfs);
  } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
  if (n_srch > 0) {
    void *d_counts = nullptr, *d_qs = nullptr, *d_len = nullptr;
    RCHK(svdss_sfs_batch_device_ptrs(b->search.sfs, &d_counts, &d_qs, &d_len, nullptr));
    BCHK(hipMemcpyAsync(b->search.counts.data(), d_counts, sizeof(int64_t) * (size_t)n_srch, hipMemcpyDeviceToHost, st));
    if (b->search.total_sfs > 0) {
      BCHK(hipMemcpyAsync(b->search.qs.data(), d_qs, sizeof(int32_t) * (size_t)b->search.total_sfs, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(b->search.len.data(), d_len, sizeof(int32_t) * (size_t)b->search.total_sfs, hipMemcpyDeviceToHost, st));
    }
  }
  BCHK(hipStreamSynchronize(st));
  run.lap(6);   // results down
  return SVDSS_OK;
}

extern "C" int svdss_bam_batch_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_index_t* ix,
                                   int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                   const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                   int32_t flags, svdss_bam_batch_t** out) {
  if (!s || !ix || !out || seq < 0 || skip < 0 || n_chunks < 0) return SVDSS_EINVAL;
  if (ix->device < 0 || !ix->d_blocks) return SVDSS_ENODEV;   // (the caller's mistake: the stream's turn is not taken)
  const int rc = svdss_bam_batch_front(s, seq, is_last, skip, ix->device, nullptr, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, flags, out);
  if (rc != SVDSS_OK) return rc;
  return svdss_bam_batch_search(*out, ix);
}

extern "C" int svdss_bam_filter_create(int32_t device, int32_t min_mapq, int32_t n_ref, const char* names, const int64_t* name_off,
                                       int64_t n_names, const int32_t* reg_tid, const int32_t* reg_beg, const int32_t* reg_end,
                                       int64_t n_regions, svdss_bam_filter_t** out) {
  if (!out || device < 0 || n_ref < 0 || n_names < 0 || n_regions < 0) return SVDSS_EINVAL;
  if ((n_names > 0 && (!names || !name_off)) || (n_regions > 0 && (!reg_tid || !reg_beg || !reg_end))) return SVDSS_EINVAL;
  HIPCHK(hipSetDevice(device));
  svdss_bam_filter* f = new (std::nothrow) svdss_bam_filter();
  if (!f) return SVDSS_ENOMEM;
  f->device = device; f->min_mapq = min_mapq; f->n_ref = n_ref;
  auto bail = [&](int code) { svdss_bam_filter_free(f); return code; };
  try {
    // (a name array that is given but EMPTY is the empty set: nothing is named, so nothing passes by name -- `call` on an
    // empty SFS file does not have every record of the BAM exported to look at; no array at all: no name test)
    if (n_names > 0 || (names && name_off)) {
      uint64_t size = 64;
      while (size < 2 * (uint64_t)n_names) size <<= 1;
      std::vector<uint64_t> tab((size_t)size, 0);
      for (int64_t i = 0; i < n_names; ++i) {
        if (name_off[i + 1] < name_off[i]) return bail(SVDSS_EINVAL);
        const uint64_t h = name_hash((const uint8_t*)names + name_off[i], (uint32_t)(name_off[i + 1] - name_off[i]));
        for (uint64_t k = h & (size - 1);; k = (k + 1) & (size - 1)) {
          if (tab[(size_t)k] == h) break;
          if (tab[(size_t)k] == 0) { tab[(size_t)k] = h; break; }
        }
      }
      if (hipMalloc((void**)&f->d_hash, size * 8) != hipSuccess) return bail(SVDSS_ENOMEM);
      if (hipMemcpy(f->d_hash, tab.data(), size * 8, hipMemcpyHostToDevice) != hipSuccess) return bail(SVDSS_EHIP);
      f->hash_mask = size - 1;
    }
    if (n_regions > 0) {
      std::vector<int64_t> off((size_t)n_ref + 1, 0);
      std::vector<int32_t> runmax((size_t)n_regions);
      for (int64_t i = 0; i < n_regions; ++i) {
        if (reg_tid[i] < 0 || reg_tid[i] >= n_ref) return bail(SVDSS_EINVAL);
        if (i > 0 && (reg_tid[i] < reg_tid[i - 1] || (reg_tid[i] == reg_tid[i - 1] && reg_beg[i] < reg_beg[i - 1]))) return bail(SVDSS_EINVAL);
        ++off[(size_t)reg_tid[i] + 1];
        runmax[(size_t)i] = (i > 0 && reg_tid[i] == reg_tid[i - 1]) ? std::max(runmax[(size_t)i - 1], reg_end[i]) : reg_end[i];
      }
      for (int32_t t = 0; t < n_ref; ++t) off[(size_t)t + 1] += off[(size_t)t];
      if (hipMalloc((void**)&f->d_reg_off, off.size() * 8) != hipSuccess || hipMalloc((void**)&f->d_reg_beg, (size_t)n_regions * 4) != hipSuccess ||
          hipMalloc((void**)&f->d_reg_runmax, (size_t)n_regions * 4) != hipSuccess)
        return bail(SVDSS_ENOMEM);
      if (hipMemcpy(f->d_reg_off, off.data(), off.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(f->d_reg_beg, reg_beg, (size_t)n_regions * 4, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(f->d_reg_runmax, runmax.data(), (size_t)n_regions * 4, hipMemcpyHostToDevice) != hipSuccess)
        return bail(SVDSS_EHIP);
    }
  } catch (...) { return bail(SVDSS_ENOMEM); }
  *out = f;
  return SVDSS_OK;
}

extern "C" void svdss_bam_filter_free(svdss_bam_filter_t* f) {
  if (!f) return;
  if (f->device >= 0) (void)hipSetDevice(f->device);
  if (f->d_hash) (void)hipFree(f->d_hash);
  if (f->d_reg_off) (void)hipFree(f->d_reg_off);
  if (f->d_reg_beg) (void)hipFree(f->d_reg_beg);
  if (f->d_reg_runmax) (void)hipFree(f->d_reg_runmax);
  delete f;
}

extern "C" int svdss_bam_store_create(int32_t device, int64_t max_bytes, int64_t initial_bytes, svdss_bam_store_t** out) {
  if (!out || device < 0 || max_bytes < 0 || initial_bytes < 0) return SVDSS_EINVAL;
  svdss_bam_store* t = new (std::nothrow) svdss_bam_store();
  if (!t) return SVDSS_ENOMEM;
  t->device = device;
  t->max_bytes = max_bytes;
  if (const char* e = getenv("SVDSS_STORE_ARENA_MB")) if (atoll(e) > 0) t->arena_bytes = atoll(e) << 20;
  // initial_bytes of arenas are taken by a thread of the store, one after the other, AHEAD of the batches: a hipMalloc by a
  // feeding thread in the middle of the stream waits for the device (24 arenas of 2 GB on demand cost `SVDSS call` 2.5 s of a
  // 3.3 s pass at 30x), and memory that another process has just handed back is cleared by the driver before it is handed
  // out again -- 4 s for 50 GB right behind a `SVDSS search` that held 190 GB, taken in one piece before the stream began.
  // Taken ahead, piece by piece, the clearing runs beside the stream; a batch only waits when it has caught up with it.
  initial_bytes = std::min(initial_bytes, max_bytes);
  if (initial_bytes > 0) {
    t->ahead_running = true;
    t->ahead = std::thread([t, initial_bytes] {
      (void)hipSetDevice(t->device);
      int64_t left = initial_bytes;
      while (left > 0) {
        { std::lock_guard<std::mutex> lk(t->m); if (t->stop) break; }
        StoreArena A;
        A.cap = std::min(left, t->arena_bytes);
        if (A.cap < ((int64_t)1 << 20) && left != initial_bytes) break;
        if (hipMalloc((void**)&A.p, (size_t)A.cap) != hipSuccess) { (void)hipGetLastError(); break; }
        { std::lock_guard<std::mutex> lk(t->m); t->allocated += A.cap; t->arenas.push_back(A); }
        t->cv.notify_all();
        left -= A.cap;
      }
      { std::lock_guard<std::mutex> lk(t->m); t->ahead_running = false; }
      t->cv.notify_all();
    });
  }
  *out = t;
  return SVDSS_OK;
}
extern "C" void svdss_bam_store_free(svdss_bam_store_t* t) {
  if (!t) return;
  { std::lock_guard<std::mutex> lk(t->m); t->stop = true; }
  if (t->ahead.joinable()) t->ahead.join();
  (void)hipSetDevice(t->device);
  for (StoreArena& A : t->arenas) if (A.p) (void)hipFree(A.p);
  delete t;
}
// forget what is stored (the arenas stay): a region of the file that runs again (ShardedBamSelect, bam_device_select.h)
extern "C" int svdss_bam_store_reset(svdss_bam_store_t* t) {
  if (!t) return SVDSS_EINVAL;
  std::lock_guard<std::mutex> lk(t->m);
  t->batches.clear();
  for (StoreArena& A : t->arenas) A.used = 0;
  t->cur = 0;
  t->n_records = 0; t->n_bytes = 0;
  t->complete = true;
  return SVDSS_OK;
}
extern "C" int64_t svdss_bam_store_batches(svdss_bam_store_t* t, int32_t* complete, int64_t* n_records, int64_t* n_bytes) {
  if (!t) return -1;
  std::lock_guard<std::mutex> lk(t->m);
  if (complete) *complete = t->complete ? 1 : 0;
  if (n_records) *n_records = t->n_records;
  if (n_bytes) *n_bytes = t->n_bytes;
  return (int64_t)t->batches.size();
}
// room for a batch's slim records (+ their n + 1 offsets); false: the store is over its limit (and stays incomplete)
bool store_reserve(svdss_bam_store* t, int64_t seq, int64_t bytes, int64_t n, StoreBatch& B, uint8_t*& base) {
  const int64_t need = ((bytes + 255) & ~(int64_t)255) + (((n + 1) * 8 + 255) & ~(int64_t)255);
  std::unique_lock<std::mutex> lk(t->m);
  if (!t->complete) return false;
  for (;;) {
    // the arena in use, then those taken ahead that nothing has been placed in yet
    while (t->cur < t->arenas.size() && t->arenas[t->cur].used + need > t->arenas[t->cur].cap) ++t->cur;
    if (t->cur < t->arenas.size()) break;
    if (t->ahead_running) { t->cv.wait(lk); continue; }      // (the thread that takes arenas ahead has not got this far yet)
    StoreArena A;
    A.cap = std::max(std::min(t->arena_bytes, t->max_bytes - t->allocated), need);     // (a small store -- a seam's -- takes small arenas)
    if (t->allocated + A.cap > t->max_bytes || hipMalloc((void**)&A.p, (size_t)A.cap) != hipSuccess) { (void)hipGetLastError(); t->complete = false; return false; }
    t->allocated += A.cap;
    t->arenas.push_back(A);
  }
  StoreArena& A = t->arenas[t->cur];
  B.arena = (int)t->cur; B.at = A.used; B.bytes = bytes; B.n = n;
  B.off_at = A.used + ((bytes + 255) & ~(int64_t)255);
  A.used += need;
  base = A.p;
  t->batches[seq] = B;
  t->n_records += n; t->n_bytes += bytes;
  return true;
}

extern "C" int svdss_bam_select_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_filter_t* f,
                                    int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                    const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                    svdss_bam_batch_t** out) {
  return svdss_bam_select_store_run(s, seq, is_last, skip, f, nullptr, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, out);
}

extern "C" int svdss_bam_select_store_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_filter_t* f,
                                          svdss_bam_store_t* store, int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                          const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                          svdss_bam_batch_t** out) {
  if (!s || !f || !out || seq < 0 || skip < 0 || n_chunks < 0) return SVDSS_EINVAL;
  if (store && store->device != f->device) return SVDSS_EINVAL;
  if (store) { std::lock_guard<std::mutex> lk(store->m); if (!store->complete) store = nullptr; }
  Front F;
  {
    const int rc = batch_front(s, seq, is_last, skip, f->device, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, out, F);
    if (rc != SVDSS_OK) return rc;
  }
  svdss_bam_batch* b = *out;
  BatchRun run(b);
  const hipStream_t st = run.st;
  const SegWalk& W = F.W;
  const int64_t n_rec = F.hdr[H_NREC];
  b->n_records = n_rec + F.hdr[H_GATED];
  b->sel.n = 0; b->sel.bytes = 0; b->sel.slim = false;
  RCHK(b->rpos.ensure(sizeof(uint32_t) * (size_t)(n_rec + 1)));
  RCHK(b->flags.ensure(sizeof(int64_t) * 5 * (size_t)(n_rec + 1)));
  RCHK(b->scans.ensure(sizeof(int64_t) * 4 * (size_t)(n_rec + 1)));
  SelP M;
  M.buf = W.buf; M.lists = W.lists; M.list_cap = W.list_cap; M.seg_cnt = W.seg_cnt; M.seg_base = F.seg_base; M.pre = (const uint32_t*)b->front.pre.p;
  M.n_seg = W.n_seg; M.min_mapq = f->min_mapq; M.n_ref = f->n_ref; M.n_rec = n_rec;
  M.hash = f->d_hash; M.hash_mask = f->hash_mask; M.reg_off = f->d_reg_off; M.reg_beg = f->d_reg_beg; M.reg_runmax = f->d_reg_runmax;
  M.rpos = (uint32_t*)b->rpos.p;
  M.f_sel = (int64_t*)b->flags.p; M.f_bytes = M.f_sel + (n_rec + 1);
  M.f_keep = store ? M.f_bytes + (n_rec + 1) : nullptr; M.f_kbytes = store ? M.f_keep + (n_rec + 1) : nullptr; M.hpv = store ? M.f_kbytes + (n_rec + 1) : nullptr;
  M.hdr = (int64_t*)b->front.hdr.p;
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)W.n_seg + 1), dim3(64), 0, st, M);
  BCHK(hipGetLastError());
  int64_t* sc = (int64_t*)b->scans.p;
  RCHK(run.scan_rows(M.f_sel, sc, n_rec + 1, store ? 4 : 2));
  // (how much is kept is only known on the device: bounded by the batch itself)
  RCHK(b->sel.out.ensure((size_t)(F.total_inf + F.HEAD) + 4 * (size_t)(n_rec + 1) + 64));
  RCHK(b->sel.off.ensure(sizeof(int64_t) * (size_t)(n_rec + 2)));
  if (store)
    hipLaunchKernelGGL(slim_export_kernel, dim3((unsigned)(n_rec + 1)), dim3(64), 0, st, W.buf, n_rec, (const uint32_t*)M.rpos, (const int64_t*)M.f_sel,
                       (const int64_t*)sc, (const int64_t*)(sc + (n_rec + 1)), (const int64_t*)M.hpv, (uint8_t*)b->sel.out.p, (int64_t*)b->sel.off.p,
                       (int64_t*)b->totals.p);
  else
    hipLaunchKernelGGL(export_kernel, dim3((unsigned)(n_rec + 1)), dim3(64), 0, st, W.buf, n_rec, (const uint32_t*)M.rpos, (const int64_t*)M.f_sel,
                       (const int64_t*)sc, (const int64_t*)(sc + (n_rec + 1)), (uint8_t*)b->sel.out.p, (int64_t*)b->sel.off.p, (int64_t*)b->totals.p);
  BCHK(hipGetLastError());
  b->sel.slim = store != nullptr;
  int64_t totals[2] = {0, 0}, hdr2[H_N] = {0};
  BCHK(hipMemcpyAsync(totals, b->totals.p, sizeof totals, hipMemcpyDeviceToHost, st));
  BCHK(hipMemcpyAsync(hdr2, b->front.hdr.p, sizeof hdr2, hipMemcpyDeviceToHost, st));
  int64_t kept[2] = {0, 0};       // the store's share: records, bytes (the last entries of the third and fourth scan)
  if (store) {
    BCHK(hipMemcpyAsync(&kept[0], sc + 2 * (n_rec + 1) + n_rec, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&kept[1], sc + 3 * (n_rec + 1) + n_rec, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  }
  BCHK(hipStreamSynchronize(st));
  run.lap(3);
  if (const char* bad = record_error(hdr2[H_ERR])) return run.fail(SVDSS_EIO, bad);   // (select_kernel raises E_CORRUPT only)
  if (store) {
    StoreBatch B;
    uint8_t* base = nullptr;
    if (store_reserve(store, seq, kept[1], kept[0], B, base)) {
      hipLaunchKernelGGL(slim_export_kernel, dim3((unsigned)(n_rec + 1)), dim3(64), 0, st, W.buf, n_rec, (const uint32_t*)M.rpos, (const int64_t*)M.f_keep,
                         (const int64_t*)(sc + 2 * (n_rec + 1)), (const int64_t*)(sc + 3 * (n_rec + 1)), (const int64_t*)M.hpv, base + B.at,
                         (int64_t*)(base + B.off_at), (int64_t*)b->totals.p + 2);
      BCHK(hipGetLastError());
    }
  }
  b->sel.n = totals[0];
  b->sel.bytes = totals[1];
  RCHK(b->sel.host.ensure((size_t)totals[1]));
  try { b->sel.host_off.resize((size_t)totals[0] + 1); } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
  BCHK(hipMemcpyAsync(b->sel.host_off.data(), b->sel.off.p, sizeof(int64_t) * (size_t)(totals[0] + 1), hipMemcpyDeviceToHost, st));
  if (totals[1] > 0) BCHK(hipMemcpyAsync(b->sel.host.p, b->sel.out.p, (size_t)totals[1], hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  run.lap(6);
  return SVDSS_OK;
}

// A pass over ONE stored batch: its slim records that `f` names or whose alignment overlaps a region of `f`, in file order, on the host
// (svdss_bam_batch_selection, slim = 1).  Any batch object of the store's device (or none yet) may be used; calls on different
// batch objects overlap.
extern "C" int svdss_bam_store_select(svdss_bam_store_t* t, int64_t seq, const svdss_bam_filter_t* f, svdss_bam_batch_t** out) {
  if (!t || !f || !out || seq < 0 || f->device != t->device) return SVDSS_EINVAL;
  StoreBatch B;
  const uint8_t* base = nullptr;
  {
    std::lock_guard<std::mutex> lk(t->m);
    auto it = t->batches.find(seq);
    if (it == t->batches.end()) return SVDSS_EINVAL;
    B = it->second;
    base = t->arenas[(size_t)B.arena].p;
  }
  HIPCHK(hipSetDevice(t->device));
  BatchRun run;
  RCHK(run.batch_object(out, t->device));
  svdss_bam_batch* b = run.b;
  const hipStream_t st = run.st;
  const int64_t n = B.n;
  b->n_records = n; b->sel.n = 0; b->sel.bytes = 0; b->sel.slim = true; b->inflate_ms = 0;
  for (int k = 0; k < 8; ++k) b->stage_ms[k] = 0;
  const auto t0 = std::chrono::steady_clock::now();
  RCHK(b->flags.ensure(sizeof(int64_t) * 2 * (size_t)(n + 1)));
  RCHK(b->scans.ensure(sizeof(int64_t) * 2 * (size_t)(n + 1)));
  RCHK(b->totals.ensure(64));
  StoreSelP M;
  M.recs = base + B.at; M.off = (const int64_t*)(base + B.off_at); M.n = n; M.n_ref = f->n_ref;
  M.hash = f->d_hash; M.hash_mask = f->hash_mask; M.reg_off = f->d_reg_off; M.reg_beg = f->d_reg_beg; M.reg_runmax = f->d_reg_runmax;
  M.f_sel = (int64_t*)b->flags.p; M.f_bytes = M.f_sel + (n + 1);
  hipLaunchKernelGGL(store_select_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, M);
  BCHK(hipGetLastError());
  int64_t* sc = (int64_t*)b->scans.p;
  RCHK(run.scan_rows(M.f_sel, sc, n + 1, 2));
  RCHK(b->sel.out.ensure((size_t)B.bytes + 64));
  RCHK(b->sel.off.ensure(sizeof(int64_t) * (size_t)(n + 2)));
  hipLaunchKernelGGL(store_export_kernel, dim3((unsigned)(n + 1)), dim3(64), 0, st, M.recs, M.off, n, (const int64_t*)M.f_sel, (const int64_t*)sc,
                     (const int64_t*)(sc + (n + 1)), (uint8_t*)b->sel.out.p, (int64_t*)b->sel.off.p, (int64_t*)b->totals.p);
  BCHK(hipGetLastError());
  int64_t totals[2] = {0, 0};
  BCHK(hipMemcpyAsync(totals, b->totals.p, sizeof totals, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  b->sel.n = totals[0];
  b->sel.bytes = totals[1];
  RCHK(b->sel.host.ensure((size_t)totals[1]));
  try { b->sel.host_off.resize((size_t)totals[0] + 1); } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
  BCHK(hipMemcpyAsync(b->sel.host_off.data(), b->sel.off.p, sizeof(int64_t) * (size_t)(totals[0] + 1), hipMemcpyDeviceToHost, st));
  if (totals[1] > 0) BCHK(hipMemcpyAsync(b->sel.host.p, b->sel.out.p, (size_t)totals[1], hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  b->stage_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SVDSS_OK;
}

extern "C" int svdss_bam_batch_selection(const svdss_bam_batch_t* b, svdss_bam_selection_t* r) {
  if (!b || !r) return SVDSS_EINVAL;
  r->n_records = b->n_records; r->n_selected = b->sel.n; r->n_bytes = b->sel.bytes;
  r->rec_off = b->sel.host_off.data(); r->bytes = (const uint8_t*)b->sel.host.p;
  r->slim = b->sel.slim ? 1 : 0;
  r->inflate_kernel_ms = b->inflate_ms;
  for (int k = 0; k < 8; ++k) r->stage_ms[k] = b->stage_ms[k];
  return SVDSS_OK;
}

extern "C" int svdss_bam_batch_result(const svdss_bam_batch_t* b, svdss_bam_result_t* r) {
  if (!b || !r) return SVDSS_EINVAL;
  r->n_records = b->n_records; r->n_slots = b->search.n_slots; r->n_searched = b->search.n_searched; r->n_short = b->search.n_short;
  r->total_sfs = b->search.total_sfs;
  r->name_off = b->search.name_off.data(); r->names = b->search.names.data(); r->hp = b->search.hp.data(); r->sidx = b->search.sidx.data();
  r->counts = b->search.counts.data(); r->qs = b->search.qs.data(); r->len = b->search.len.data();
  r->inflate_kernel_ms = b->inflate_ms;
  for (int k = 0; k < 8; ++k) r->stage_ms[k] = b->stage_ms[k];
  return SVDSS_OK;
}

extern "C" const char* svdss_bam_batch_error(const svdss_bam_batch_t* b) { return b ? b->err.c_str() : ""; }

