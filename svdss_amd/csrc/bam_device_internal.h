// bam_device_internal.h -- what the units of the BAM device path share (bam_device.hip: front end, search, select, store;
// bam_smooth.hip: `SVDSS smooth`): the stream and batch objects, the front end's result, the scope an entry point runs a
// batch in (BatchRun), the record store and the few device helpers the kernels of both units use.  Kernels stay in the unit
// that launches them, but for slim_export_kernel, which both launch.  How a batch's BGZF members get into HBM (BgzfIntake,
// crc32_kernel), the turn in file order, BCHK / RCHK and the hipcub helper are bgzf_intake.h's: the text units share them.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <algorithm>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bam_aux_walk.h"
#include "bgzf_intake.h"

// error bits a batch's kernels raise (hdr[H_ERR]; bam_smooth.hip adds one of its own)
enum { E_CORRUPT = 1, E_TID = 2 };
enum { H_NREC = 0, H_TAIL = 1, H_ERR = 2, H_REWALK = 3, H_PRE = 4, H_SHORT = 5, H_START = 6, H_GATED = 7, H_N = 8 };

// what the host says about them: the words of the host path (BamReader::next_view, ping_pong.cpp:76-79)
static inline const char* record_error(int64_t bits) {
  return (bits & E_CORRUPT) ? "corrupt record" : (bits & E_TID) ? "core.tid < 0. Why are we here? Please check" : nullptr;
}

namespace {   // (every unit its own copy: no device-side linking)

// bam_aux_get + bam_aux2i for one two-letter tag, as BamReader::aux_int reads it (csrc/bam_reader.h): integer types
// only, anything unexpected ends the scan with "absent"
__device__ bool aux_int(const uint8_t* p, const uint8_t* e, char a, char b, int64_t& out) {
  while (p < e) {
    const int64_t sz = svdss_aux_value_size(p, e);   // (bam_aux_walk.h: the value lies inside the block, or the walk gives up)
    if (sz < 0) return false;
    const char t0 = (char)p[0], t1 = (char)p[1], ty = (char)p[2];
    p += 3;
    if (t0 == a && t1 == b) {
      switch (ty) {
        case 'c': out = (int8_t)p[0]; return true;
        case 'C': out = p[0]; return true;
        case 's': out = (int16_t)((uint16_t)p[0] | ((uint16_t)p[1] << 8)); return true;
        case 'S': out = (uint16_t)((uint16_t)p[0] | ((uint16_t)p[1] << 8)); return true;
        case 'i': out = (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); return true;
        case 'I': out = (uint32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); return true;
        default: return false;
      }
    }
    p += sz;
  }
  return false;
}

// ------------------------------------------------------------------ read names wanted (svdss_bam_filter_t), slim records (svdss_bam_store_t)
__host__ __device__ inline uint64_t name_hash(const uint8_t* p, uint32_t n) {   // FNV-1a, 0 kept for "empty slot"
  uint64_t h = 1469598103934665603ull;
  for (uint32_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h ? h : 1;
}
// is the name's hash in the filter's open-addressed table?  (a hit may be another name with the same hash: the host looks again)
__device__ __forceinline__ bool name_in_set(const uint64_t* __restrict__ hash, uint64_t mask, const uint8_t* name, uint32_t n) {
  const uint64_t h = name_hash(name, n);
  for (uint64_t k = h & mask;; k = (k + 1) & mask) {
    const uint64_t e = hash[k];
    if (e == h) return true;
    if (e == 0) return false;
  }
}

constexpr int64_t kNoHp = (int64_t)1 << 40;   // "the record has no integer HP tag"

// the flag / mapq filters of `SVDSS call` (clusterer.cpp:118-122 = :535-540): what a record store keeps
__device__ __forceinline__ bool call_keeps(uint32_t flag, uint32_t mapq, int32_t min_mapq) {
  return !(flag & (4u | 2048u | 256u)) && (int32_t)mapq >= min_mapq;
}
// the size of a record's slim form, 4-aligned (block_size + core .. bases + "HPi" + value), and its HP tag (kNoHp: none);
// the record begins at buf + p, bs = its block_size, head = core .. qualities
__device__ __forceinline__ int64_t slim_measure(const uint8_t* buf, int64_t p, uint32_t bs, int64_t head, int32_t l_seq, int64_t& hpv) {
  int64_t hp = 0;
  const bool have = aux_int(buf + p + 4 + head, buf + p + 4 + bs, 'H', 'P', hp);
  hpv = have ? hp : kNoHp;
  return (4 + head - l_seq + (have ? 7 : 0) + 3) & ~(int64_t)3;
}

// one wavefront per stored record: block_size' | core | name | CIGAR | packed bases | HP as an int32 tag if the record had
// an integer one -- no qualities, no other tags (`call` reads neither: clusterer.cpp:56-156, 477-610).  f_keep: which
// records, s_keep / s_bytes: its exclusive sums (entry n_rec: the totals), hpv: what slim_measure left
__global__ void __launch_bounds__(64) slim_export_kernel(const uint8_t* __restrict__ buf, int64_t n_rec, const uint32_t* __restrict__ rpos,
                                                         const int64_t* __restrict__ f_keep, const int64_t* __restrict__ s_keep,
                                                         const int64_t* __restrict__ s_bytes, const int64_t* __restrict__ hpv,
                                                         uint8_t* out, int64_t* out_off, int64_t* totals) {
  const int64_t gi = blockIdx.x;
  if (gi == n_rec) {
    if (threadIdx.x == 0) { out_off[s_keep[gi]] = s_bytes[gi]; totals[0] = s_keep[gi]; totals[1] = s_bytes[gi]; }
    return;
  }
  if (!f_keep[gi]) return;
  const int64_t p = rpos[gi], o = s_bytes[gi];
  const uint32_t w3 = ld32(buf, p + 12), w4 = ld32(buf, p + 16);
  const int32_t l_seq = (int32_t)ld32(buf, p + 20);
  const uint32_t l_name = w3 & 0xffu, n_cig = w4 & 0xffffu;
  const uint32_t n1 = 36u + l_name + 4u * n_cig + ((uint32_t)l_seq + 1u) / 2u;       // bytes taken over (block_size field included)
  const int64_t hp = hpv[gi];
  const uint32_t total = n1 + (hp != kNoHp ? 7u : 0u);
  if (threadIdx.x == 0) out_off[s_keep[gi]] = o;
  uint32_t* dst = (uint32_t*)(out + o);
  for (uint32_t k = threadIdx.x; k < n1 / 4; k += 64) {
    uint32_t w = ld32(buf, p + 4 * (int64_t)k);
    if (k == 0) w = total - 4u;                       // the slim record's block_size
    dst[k] = w;
  }
  if (threadIdx.x == 0) {
    uint8_t* q = out + o;
    for (uint32_t k = n1 & ~3u; k < n1; ++k) q[k] = buf[p + k];
    if (hp != kNoHp) {
      const bool neg_ok = hp >= -2147483648ll && hp <= 2147483647ll;
      q[n1] = 'H'; q[n1 + 1] = 'P'; q[n1 + 2] = neg_ok ? 'i' : 'I';
      const uint32_t v = (uint32_t)hp;
      q[n1 + 3] = (uint8_t)v; q[n1 + 4] = (uint8_t)(v >> 8); q[n1 + 5] = (uint8_t)(v >> 16); q[n1 + 6] = (uint8_t)(v >> 24);
    }
    // the bytes up to the 4-aligned end are part of what a selection brings down: zero, not what the arena held before
    for (uint32_t k = total; k < ((total + 3u) & ~3u); ++k) q[k] = 0;
  }
}

// 16 ALIGNED output bytes [o0, o0 + 16) of a read's nt6 symbols (ping_pong.cpp:90-94: seq_nt16_str, then seq_nt6_table), clipped
// to the read [s, e); its packed 4-bit bases begin at buf + src: three dword loads, a 16-entry nibble table in a register,
// whole chunks leave as one 16-byte store, the two ends of a read byte by byte (unpack_kernel, sm_sfs_nt6_kernel)
__device__ __forceinline__ void nt6_chunk16(const uint8_t* __restrict__ buf, int64_t src, int64_t s, int64_t e, int64_t o0, uint8_t* out) {
  const int64_t a = o0 < s ? s : o0, b = o0 + 16 < e ? o0 + 16 : e;    // output bytes [a, b)
  const int64_t i0 = a - s;                                            // first symbol of the read this lane writes
  const int64_t sb = src + (i0 >> 1);
  const uint64_t lo = (uint64_t)ld32(buf, sb) | ((uint64_t)ld32(buf, sb + 4) << 32);
  const uint32_t hi = ld32(buf, sb + 8);
  // "=ACMGRSVTWYHKDBN": A=1 C=2 G=4 T=8 -> nt6 1..4, every other code (IUPAC, '=') -> 5 like seq_nt6_table
  const uint64_t lut = 0x5555555455535215ull;
  uint32_t w[4] = {0, 0, 0, 0};
  const int n = (int)(b - a);
  const int odd = (int)(i0 & 1);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int ni = k + odd;                        // nibble index from the first loaded byte
    const int by = ni >> 1;
    const uint32_t byte = by < 8 ? (uint32_t)(lo >> (8 * by)) & 0xffu : (hi >> (8 * (by - 8))) & 0xffu;
    const uint32_t v = (ni & 1) ? (byte & 15u) : (byte >> 4);
    const uint32_t sym = (uint32_t)(lut >> (4 * v)) & 15u;
    w[k >> 2] |= sym << (8 * (k & 3));
  }
  if (n == 16) {
    *(uint4*)(out + a) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    for (int k = 0; k < n; ++k) out[a + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
}

}  // namespace

// ------------------------------------------------------------------ the stream of a file's batches
struct svdss_bam_stream {
  int32_t n_ref = 0;
  std::mutex m;
  std::condition_variable cv;
  int64_t next_seq = 0;
  int failed = 0;
  std::string err;
  std::vector<uint8_t> carry;      // the bytes behind the last complete record of the batch that had its turn last
  // a region of a file (svdss_bam_stream_region): open_start = batch 0 begins somewhere inside a record, `head` = its bytes
  // in front of the first record the chain was started at; open_end = the last batch may end inside a record (carry stays)
  bool open_start = false, open_end = false;
  std::vector<uint8_t> head;
  int64_t n_rewalked = 0, n_segments = 0;
  // smoothing (bam_smooth.hip): the output stream's turn, and the bytes behind its last full BGZF block (at first: the
  // BAM header of the output)
  int64_t next_out = 0;
  std::vector<uint8_t> out_tail;
  // the record gate (svdss_bam_stream_set_regions): the intervals as gate_kernel reads them -- n_ref + 1 offsets (int64), the
  // begins, the ends (int32 each) -- and the records of the batches so far that were outside them
  bool gate_on = false;
  std::vector<uint8_t> gate_tab;
  int64_t gate_n = 0, n_gated = 0;
  // the index of the input (svdss_bam_stream_set_input_index; in_ix_shift 0: off).  Next to the carry, where its first byte
  // is in the file: the compressed offset of the member that holds it, RELATIVE to the first member of the batch that has
  // its turn next (so below 0), and the offset in that member.  head_v: the virtual offset of the record an open_start
  // region's chain was started at, relative to the region's first member.
  int32_t in_ix_shift = 0, in_ix_depth = 0;
  int64_t carry_coff = 0, head_v = 0;
  int32_t carry_uoff = 0;
};

// Batches take turns in file order (wait_turn / done_turn / pass_turn, bgzf_intake.h): at the carry (`turn` =
// &svdss_bam_stream::next_seq) and, when smoothing, at the output stream (next_out).

// ------------------------------------------------------------------ the batch object
// One object for every job (callers reuse it across jobs); the members are grouped by the job that owns them.
using BamBuf = DevBuf<3, 4096>;   // grows to n + n / 8 + 4096

struct svdss_bam_batch {
  int device = -1;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::string err;
  int64_t n_records = 0;
  double inflate_ms = 0;
  double stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // host clock between the waits of the last run (svdss_bam_result_t::stage_ms)
  // shared on purpose: record offsets, the flags and their scans, hipcub's temporary storage, small totals
  BamBuf rpos, flags, scans, tmp, totals;
  // batch_front: the blocks, the inflated bytes, the record chain (pre and hdr are read by the job that follows)
  struct {
    BgzfIntake in;
    BamBuf buf, seg, lists, pre, hdr, gate;
  } front;
  // svdss_bam_batch_front / _search: what the front half left for the search half, and the results on the host
  struct {
    const uint8_t* cur_reads = nullptr;
    const int64_t* cur_off = nullptr;
    int64_t cur_syms = 0, name_bytes = 0;
    int32_t cur_flags = 0;
    bool front_done = false;
    int64_t park_group = -1, park_first = 0;   // -1: not parked (reads in this object), -2: nothing to search, >= 0: group
    BamBuf d_hp, o_small, d_names, sym_off, seq_src, reads;
    svdss_sfs_batch_t* sfs = nullptr;
    std::vector<int32_t> name_off, hp, sidx, qs, len;
    std::vector<char> names;
    std::vector<int64_t> counts;
    int64_t n_slots = 0, n_searched = 0, n_short = 0, total_sfs = 0;
  } search;
  // svdss_bam_select_run / _select_store_run / svdss_bam_store_select: the kept records and their offsets, device and host
  struct {
    BamBuf out, off;
    PinBuf<2, (size_t)1 << 20, 64> host;   // page-locked (grows to n + n / 4 + 1 MB); smoothing's BGZF members land here too
    std::vector<int64_t> host_off;
    int64_t n = 0, bytes = 0;
    bool slim = false;               // the kept records are slim ones (svdss_bam_store_select)
  } sel;
  // svdss_bam_smooth_run / _measure (bam_smooth.hip)
  struct {
    BamBuf rec, out, scratch, members, dense, len;
    BamBuf lz;   // the match finder's candidates (svdss_bam_smooth_set_deflate: lz mode only)
    BamBuf store_flags, store_scans;   // svdss_bam_smooth_set_store: which records the store keeps, their sizes and HP; the sums
    int64_t kept = 0, out_bytes = 0, bgzf_bytes = 0, in0 = 0, xf[4] = {0, 0, 0, 0};
    const uint8_t* bgzf = nullptr;   // where the last run's BGZF members are (the caller's buffer or sel.host)
    std::vector<int64_t> nmx;
    std::vector<uint8_t> fits;
  } sm;
  // ... with an index asked for (svdss_bam_smooth_set_index): the batch's fragments (svdss_bam_batch_index)
  struct {
    BamBuf rec, frag;                // per kept record; the chunks and windows
    bool on = false;
    std::vector<svdss_bam_index_chunk_t> chunks;
    std::vector<svdss_bam_index_window_t> windows;
    int64_t hdr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  } sm_ix;
  // batch_front with the stream's input index on (svdss_bam_stream_set_input_index): the fragments of the batch's records
  // as they stand in the file (svdss_bam_batch_input_index)
  struct {
    BamBuf rec, frag, mstart;        // per record; the chunks and windows; where every member starts in the file
    std::vector<int64_t> h_mstart;
    std::vector<svdss_bam_input_chunk_t> chunks;
    std::vector<svdss_bam_input_window_t> windows;
    svdss_bam_input_frag_t f{};
    bool corrupt = false;            // a record whose fields do not fit its block_size (svdss_bam_index_run refuses the batch)
  } in_ix;
};

// ------------------------------------------------------------------ the park (bam_device.hip owns it; bam_smooth.hip parks the
// reads of smoothed batches in it as well)
// Reads unpacked while no index is resident yet (`SVDSS search` restores its index for seconds; the BAM front end runs
// meanwhile): an arena of nt6 bytes + one of offsets, cut into GROUPS of consecutive reservations that are searched as one
// large launch each (one lane per read) once the index is there.  A group's reads are contiguous from a 16-byte aligned
// start, its offsets relative to that start.
struct ParkGroup {
  int32_t arena = 0;
  int64_t sym0 = 0, n_syms = 0;      // where its reads begin in its arena (16-aligned), symbols so far
  int64_t off0 = 0, n_reads = 0;     // where its offsets begin, reads so far (offsets: n_reads + 1 entries)
  int32_t n_batches = 0, pending = 0;
  bool closed = false;
};
// (arenas are allocated one at a time, the first before the index restore starts: a process that searches 1 % of its reads --
// `SVDSS search` on a smoothed BAM -- never needs a second one, and memory the driver hands out is cleared first, 30-50 GB/s)
struct ParkArena {
  uint8_t* d_reads = nullptr;
  int64_t* d_off = nullptr;
  int64_t cap_bytes = 0, cap_off = 0;
};
struct svdss_bam_park {
  int device = -1;
  std::vector<ParkArena> arenas;
  int64_t arena_bytes = (int64_t)8 << 30, max_bytes = 0, reads_per_arena = 0;
  int64_t group_reads = 262144, group_bytes = (int64_t)4 << 30;
  hipStream_t st = nullptr;
  std::mutex m;
  std::condition_variable cv;
  std::vector<ParkGroup> groups;
  bool closed = false;
};

static inline hipError_t park_new_arena(svdss_bam_park* p) {
  ParkArena A;
  A.cap_bytes = std::min(p->arena_bytes, p->max_bytes - (int64_t)p->arenas.size() * p->arena_bytes);
  if (A.cap_bytes < 4096) return hipErrorOutOfMemory;
  A.cap_off = p->reads_per_arena + 64;
  hipError_t e = hipMalloc((void**)&A.d_reads, (size_t)A.cap_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&A.d_off, sizeof(int64_t) * (size_t)A.cap_off);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (A.d_reads) (void)hipFree(A.d_reads);
    return e;
  }
  p->arenas.push_back(A);
  return hipSuccess;
}

// room for n reads / syms symbols: group, index of the first read and symbol offset inside it; false = not parked
static inline bool park_reserve(svdss_bam_park* p, int64_t n, int64_t syms, int64_t& g, int64_t& first, int64_t& sym_first) {
  std::lock_guard<std::mutex> lk(p->m);
  if (p->closed) return false;
  auto fits = [&](const ParkGroup& G) {
    const ParkArena& A = p->arenas[(size_t)G.arena];
    return G.sym0 + G.n_syms + syms + 64 <= A.cap_bytes && G.off0 + G.n_reads + n + 2 <= A.cap_off;
  };
  if (!p->groups.empty() && !p->groups.back().closed && !fits(p->groups.back())) p->groups.back().closed = true;
  if (p->groups.empty() || p->groups.back().closed) {
    ParkGroup G;
    if (!p->groups.empty()) {
      const ParkGroup& L = p->groups.back();
      G.arena = L.arena;
      G.sym0 = ((L.sym0 + L.n_syms + 15) & ~(int64_t)15) + 32;
      G.off0 = L.off0 + L.n_reads + 1;
    }
    if (!fits(G)) {
      // the next arena (what is parked stays where it is); none to be had: the rest of the file waits for the index
      if (syms + 64 > p->arena_bytes || n + 2 > p->reads_per_arena || park_new_arena(p) != hipSuccess) { p->closed = true; return false; }
      G.arena = (int32_t)p->arenas.size() - 1; G.sym0 = 0; G.off0 = 0;
      if (!fits(G)) { p->closed = true; return false; }
    }
    p->groups.push_back(G);
  }
  ParkGroup& G = p->groups.back();
  g = (int64_t)p->groups.size() - 1;
  first = G.n_reads; sym_first = G.n_syms;
  G.n_reads += n; G.n_syms += syms; ++G.n_batches; ++G.pending;
  if (G.n_reads >= p->group_reads || G.n_syms >= p->group_bytes) G.closed = true;
  return true;
}
static inline void park_done(svdss_bam_park* p, int64_t g) {
  { std::lock_guard<std::mutex> lk(p->m); --p->groups[(size_t)g].pending; }
  p->cv.notify_all();
}

// ------------------------------------------------------------------ the record store (bam_device.hip owns it; bam_smooth.hip
// deposits the batches of a smoothing run in it as well: svdss_bam_smooth_set_store)
// What `SVDSS call` keeps of a pass over the BAM (svdss_bam_store_t): the slim records of every batch, in HBM, batch by
// batch in arenas allocated as they are needed.
struct StoreBatch { int arena = -1; int64_t at = 0, bytes = 0, n = 0, off_at = 0; };
struct StoreArena { uint8_t* p = nullptr; int64_t cap = 0, used = 0; };
struct svdss_bam_store {
  int device = -1;
  int64_t max_bytes = 0, arena_bytes = (int64_t)2 << 30, allocated = 0;
  // arenas taken AHEAD of the batches by a thread of the store (see svdss_bam_store_create): next_use = the first arena no
  // batch has been placed in yet
  std::thread ahead;
  std::condition_variable cv;
  bool ahead_running = false, stop = false;
  size_t cur = 0;                // the arena batches are being placed in
  std::mutex m;
  std::vector<StoreArena> arenas;
  std::map<int64_t, StoreBatch> batches;
  bool complete = true;          // false: a batch did not fit (the caller reads the file again)
  int64_t n_records = 0, n_bytes = 0;
};
// room for batch `seq`'s slim records (+ their n + 1 offsets) at base + B.at / base + B.off_at; false: the store is over its
// limit (and stays incomplete).  (bam_device.hip)
__attribute__((visibility("hidden")))
bool store_reserve(svdss_bam_store* t, int64_t seq, int64_t bytes, int64_t n, StoreBatch& B, uint8_t*& base);

// ------------------------------------------------------------------ the front end's result
// the chain of records of a batch, per segment (the argument of walk_kernel / link_kernel)
struct SegWalk {
  const uint8_t* buf;
  int64_t lo, hi;          // fresh data of this batch: [lo, hi) (lo = head room [+ BAM header in the first batch])
  int64_t seg_bytes;
  int32_t n_seg, n_ref;
  uint32_t* seg_start;     // guessed first record of the segment (0xffffffff: none found)
  uint32_t* seg_end;       // where the chain from there left the segment (or stopped: tail / nonsense)
  int32_t* seg_cnt;
  uint32_t* lists;         // n_seg lists of list_cap offsets
  int64_t list_cap;
};

struct Front {
  SegWalk W;
  int32_t* seg_base = nullptr;
  int64_t hdr[H_N];
  int64_t total_inf = 0, HEAD = 0;
};

// ------------------------------------------------------------------ the scope an entry point runs a batch in
// The batch, its stream, the stage clock and the one way out on failure.  Entry points differ in a single thing: what else
// a failure must let go of (the input turn, the park group, the output turn) -- `release`, set where it is owed and
// cleared where it has been settled.  BCHK / RCHK (bgzf_intake.h) return through fail() of the BatchRun named `run`.
struct BatchRun {
  svdss_bam_batch* b = nullptr;
  hipStream_t st = nullptr;
  std::function<void(int, const std::string&)> release;
  std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();

  explicit BatchRun(svdss_bam_batch* b_ = nullptr) : b(b_), st(b_ ? b_->st : nullptr) {}

  void lap(int k) {
    const auto t = std::chrono::steady_clock::now();
    b->stage_ms[k] = std::chrono::duration<double, std::milli>(t - t_prev).count();
    t_prev = t;
  }
  int fail(int code, const std::string& msg) {
    if (b) {
      b->err = msg;
      // the caller recycles its page-locked slabs as soon as this returns: no copy out of them may still be under way
      if (b->st) (void)hipStreamSynchronize(b->st);
    }
    if (release) { release(code, msg); release = nullptr; }
    return code;
  }
  // The helpers below return a code and leave the message in the thread's error string (RCHK passes both to fail()).
  // the batch object, created on first use: of this device, with its stream and events
  int batch_object(svdss_bam_batch_t** out, int device) {
    if (!*out) {
      *out = new (std::nothrow) svdss_bam_batch();
      if (!*out) { g_svdss_hip_err = "out of memory"; return SVDSS_ENOMEM; }
      (*out)->device = device;
    }
    b = *out;
    if (b->device != device) { g_svdss_hip_err = "batch object of another device"; return SVDSS_EINVAL; }
    if (!b->st) HIPCHK(svdss_make_stream(&b->st, "SVDSS_SEARCH_CUS"));
    if (!b->e0) { HIPCHK(hipEventCreate(&b->e0)); HIPCHK(hipEventCreate(&b->e1)); }
    st = b->st;
    b->err.clear();
    t_prev = std::chrono::steady_clock::now();   // (the stage clock runs from here)
    return SVDSS_OK;
  }
  // room for a hipcub call that asked for `bytes` of temporary storage (b->tmp.cap is what the call may then be told)
  int scan_tmp(size_t bytes) { return b->tmp.ensure(bytes + 256); }
  // exclusive sums of `rows` consecutive rows of n entries (the last entry of a row: its total)
  int scan_rows(int64_t* in, int64_t* out, int64_t n, int rows) {
    return cub_twice(b->tmp, st, [&](void* t, size_t& tb, hipStream_t q, int k) {
      return hipcub::DeviceScan::ExclusiveSum(t, tb, in + (int64_t)k * n, out + (int64_t)k * n, (int)n, q);
    }, rows);
  }
};

// What every entry point that reads BGZF blocks does first: the batch's blocks up, inflated, checked; the record chain of
// its segments; the batch's turn at the carry.  On success the records of the batch are listed (F.W / F.seg_base /
// front.pre, F.hdr) and the turn is over.  (bam_device.hip)
__attribute__((visibility("hidden")))
int batch_front(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, int device,
                int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                svdss_bam_batch_t** out, Front& F);
