// ref_stream.hip -- the reference FASTA inflated and parsed where placement and smoothing read it (gfx950).
//
// Stands where load_chromosomes stands on the host (csrc/fastx_reader.h: FastxReader::next per record, then toupper;
// the reference's chromosomes.cpp:9-27).  A batch is a run of text bytes in HBM: BGZF members inflated by csrc/inflate.hip
// and checked against their CRC32, or a slab of a plain file.  A chromosome is one record of 250 Mb: it streams through
// the batches, no sequence byte is carried from one to the next.  What a batch hands to the one behind it:
//   the in-header bit       the text ended inside a header line
//   the at-line-start bit   the text ended behind a '\n' (or nothing has been read yet)
//   the partial header line (on the host, at most header_cap bytes) and where its record's bases begin
//   the running output offset (64 bit; a batch's own offsets are 32 bit, a batch is smaller than 1 GiB)
//
// The shape: first byte '>', no '\r', no NUL, no line that begins with '@', no header line longer than
// header_cap, no name twice.  Within it a record begins at every line that begins with '>', its name is the bytes behind
// '>' up to the first blank or tab, its sequence every other line up to the next header, joined, a-z raised.  Anything
// else DECLINES the stream as a whole: nothing is delivered and the caller reads the file with the host reader.
//
// Launches per batch (T = 4096 bytes per workgroup, 16 bytes per lane), all in the batch's turn in file order:
//   rs_tile_kernel     per tile: what it does to the in-header bit (sets it, clears it, passes it on), the bytes it keeps
//                      whatever the bit is and those it keeps only if the bit comes in clear, its header lines; the first
//                      byte that breaks the shape
//   (max-scan)         tile -> the bit it begins with, seeded by the batch in front
//   rs_tiles_kernel    tile -> bytes kept;  (scans) tile -> output offset, tile -> index of its first header
//   rs_gather_kernel   the kept bytes of a tile compacted in LDS, upper-cased, stored as one run; where every header
//                      line begins in the text and in the output
//   rs_hdr_len_kernel, (scan), rs_hdr_copy_kernel   the header lines' text into a side buffer for the host
// Upload, inflate and CRC of different batches overlap; so does bringing a batch's output down to the host copy.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bgzf_intake.h"
#include "ref_dev.h"
#include "ref_pieces.h"

namespace {

constexpr int RS_T = 4096;      // bytes per tile
constexpr int RS_TPB = 256;     // 16 bytes per lane
constexpr unsigned long long RS_NONE = 0x7fffffffffffffffull;
enum { RH_BAD = 0, RH_LASTNL = 1, RH_N = 2 };

__device__ __forceinline__ uint32_t rs_byte(const uint4& v, int k) {
  const uint32_t w = k < 8 ? (k < 4 ? v.x : v.y) : (k < 12 ? v.z : v.w);
  return (w >> (8 * (k & 3))) & 0xffu;
}

// A lane's 16 bytes, walked once: state 0 = in a sequence line, 1 = in a header line, 2 = whatever the lane came in with
// (no line has begun in front of this byte inside the lane).  `rest` counts the bytes kept whatever came in, `seg` those in
// front of the lane's first line start, `nh` the lines that begin with '>'.
struct RsLane { int s, rest, seg, nh; };
__device__ __forceinline__ RsLane rs_walk(const uint4& v, int64_t p0, int64_t N, uint32_t prev) {
  RsLane L{2, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (p0 + k >= N) continue;
    const uint32_t c = rs_byte(v, k);
    if (prev == '\n') { L.s = c == '>'; L.nh += L.s; }
    if (c != '\n') { L.rest += L.s == 0; L.seg += L.s == 2; }
    else L.s = 0;
    prev = c;
  }
  return L;
}

// the byte in front of a lane's first: the text's own, or what the batch in front says about its last byte
__device__ __forceinline__ uint32_t rs_prev(const uint8_t* buf, int64_t p0, int als0) { return p0 > 0 ? buf[p0 - 1] : (als0 ? '\n' : 'x'); }

// the state every lane begins with, from the states the lanes in front leave: the last one that is not 2 wins (-1: none)
template <class Scan>
__device__ __forceinline__ int rs_lane_in(typename Scan::TempStorage& tmp, int s, int* incl_last) {
  const int v = s == 2 ? -1 : (int)threadIdx.x * 2 + s;
  int e = -1, all = -1;
  Scan(tmp).ExclusiveScan(v, e, -1, hipcub::Max(), all);
  if (incl_last) *incl_last = all;
  return e < 0 ? 2 : (e & 1);
}

__global__ void __launch_bounds__(RS_TPB) rs_tile_kernel(const uint8_t* __restrict__ buf, int64_t N, int als0, int first,
                                                         int32_t* __restrict__ tile_kind, int32_t* __restrict__ tile_rest,
                                                         int32_t* __restrict__ tile_seg, int32_t* __restrict__ tile_hdrs,
                                                         unsigned long long* hdr) {
  typedef hipcub::BlockScan<int, RS_TPB> Scan;
  typedef hipcub::BlockReduce<int, RS_TPB> Red;
  __shared__ union { typename Scan::TempStorage scan; typename Red::TempStorage red; } tmp;
  const int64_t p0 = (int64_t)blockIdx.x * RS_T + (int64_t)threadIdx.x * 16;
  RsLane L{2, 0, 0, 0};
  if (p0 < N) {
    const uint4 v = *(const uint4*)(buf + p0);
    uint32_t prev = rs_prev(buf, p0, als0);
    L = rs_walk(v, p0, N, prev);
    unsigned long long bad = RS_NONE;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int64_t p = p0 + k;
      if (p >= N) continue;
      const uint32_t c = rs_byte(v, k);
      int why = 0;
      if (p == 0 && first && c != '>') why = SVDSS_REF_NOT_FASTA;
      else if (c == '\r') why = SVDSS_REF_CR;
      else if (c == 0) why = SVDSS_REF_NUL;
      else if (prev == '\n' && c == '@') why = SVDSS_REF_AT;
      if (why && bad == RS_NONE) bad = ((unsigned long long)p << 4) | (unsigned)why;
      if (p == N - 1) hdr[RH_LASTNL] = c == '\n';
      prev = c;
    }
    if (bad != RS_NONE) atomicMin(&hdr[RH_BAD], bad);
  }
  int last = -1;
  const int in = rs_lane_in<Scan>(tmp.scan, L.s, &last);
  __syncthreads();
  const int rest = Red(tmp.red).Sum(L.rest + (in == 0 ? L.seg : 0));
  __syncthreads();
  const int seg = Red(tmp.red).Sum(in == 2 ? L.seg : 0);
  __syncthreads();
  const int nh = Red(tmp.red).Sum(L.nh);
  if (threadIdx.x == 0) {
    tile_kind[blockIdx.x] = last < 0 ? -1 : (int)blockIdx.x * 2 + (last & 1);
    tile_rest[blockIdx.x] = rest;
    tile_seg[blockIdx.x] = seg;
    tile_hdrs[blockIdx.x] = nh;
  }
}

// tile_m: the inclusive max-scan of tile_kind.  Entry n_tiles closes the sums.
__global__ void __launch_bounds__(256) rs_tiles_kernel(const int32_t* __restrict__ tile_m, const int32_t* __restrict__ tile_rest,
                                                       const int32_t* __restrict__ tile_seg, int32_t n_tiles, int seed,
                                                       int32_t* __restrict__ tile_in, int32_t* __restrict__ tile_kept) {
  const int32_t i = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (i > n_tiles) return;
  if (i == n_tiles) { tile_kept[i] = 0; return; }
  const int32_t m = i ? tile_m[i - 1] : -1;
  const int in = m < 0 ? seed : (m & 1);
  tile_in[i] = in;
  tile_kept[i] = tile_rest[i] + (in ? 0 : tile_seg[i]);
}

// The kept bytes of a tile, in text order, are one run of the output.  They are compacted in LDS at the run's own
// alignment (the run begins at byte `dst & 15` of the LDS image), so the image leaves in aligned 16-byte stores; the
// ragged first and last 16 bytes, which neighbouring tiles share, leave byte by byte.
__global__ void __launch_bounds__(RS_TPB) rs_gather_kernel(const uint8_t* __restrict__ buf, int64_t N, int als0,
                                                           const int32_t* __restrict__ tile_in, const int32_t* __restrict__ tile_off,
                                                           const int32_t* __restrict__ tile_hb, uint8_t* __restrict__ out,
                                                           int32_t* __restrict__ hdr_pos, int32_t* __restrict__ hdr_out) {
  typedef hipcub::BlockScan<int, RS_TPB> Scan;
  __shared__ typename Scan::TempStorage tmp;
  __shared__ __align__(16) uint8_t sym[RS_T + 16];
  const int64_t p0 = (int64_t)blockIdx.x * RS_T + (int64_t)threadIdx.x * 16;
  const bool mine = p0 < N;
  uint4 v = make_uint4(0, 0, 0, 0);
  uint32_t prev = 'x';
  RsLane L{2, 0, 0, 0};
  if (mine) {
    v = *(const uint4*)(buf + p0);
    prev = rs_prev(buf, p0, als0);
    L = rs_walk(v, p0, N, prev);
  }
  int in = rs_lane_in<Scan>(tmp, L.s, nullptr);
  if (in == 2) in = tile_in[blockIdx.x];
  __syncthreads();
  const int cnt = L.rest + (in == 0 ? L.seg : 0);
  int before = 0;
  Scan(tmp).ExclusiveSum(cnt | (L.nh << 16), before);
  const int32_t dst = tile_off[blockIdx.x], n = tile_off[blockIdx.x + 1] - dst;
  const int a = dst & 15;
  if (mine && (cnt || L.nh)) {
    int kb = before & 0xffff, hb = tile_hb[blockIdx.x] + (before >> 16), s = in;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (p0 + k >= N) continue;
      const uint32_t c = rs_byte(v, k);
      if (prev == '\n') {
        s = c == '>';
        if (s) { hdr_pos[hb] = (int32_t)(p0 + k); hdr_out[hb] = dst + kb; ++hb; }
      }
      if (c == '\n') s = 0;
      else if (s == 0) sym[a + kb++] = (uint8_t)(c - ((c >= 'a' && c <= 'z') ? 32u : 0u));
      prev = c;
    }
  }
  __syncthreads();
  if (n <= 0) return;
  uint8_t* const g = out + (dst - a);
  const int total = a + n;
  for (int lo = (int)threadIdx.x * 16; lo < total; lo += RS_TPB * 16) {
    if (lo >= a && lo + 16 <= total) {
      *(uint4*)(g + lo) = *(const uint4*)(sym + lo);
    } else {
      const int e = lo + 16 < total ? lo + 16 : total;
      for (int j = lo > a ? lo : a; j < e; ++j) g[j] = sym[j];
    }
  }
}

// entry e: a header line's text from pos[e] up to its '\n' -- or to the end of the text (term 0: it goes on in the next
// batch), or to `limit` bytes (longer than any header may be).  cont = 1: entry 0 is the text's head, which goes on with the
// header line the batch in front ended in.
__global__ void __launch_bounds__(64) rs_hdr_len_kernel(const uint8_t* __restrict__ buf, int64_t N, const int32_t* __restrict__ hdr_pos,
                                                        int cont, int32_t n_ent, int32_t limit, int32_t* __restrict__ ent_pos,
                                                        int32_t* __restrict__ ent_len, int32_t* __restrict__ ent_term) {
  const int32_t e = (int32_t)blockIdx.x;
  if (e > n_ent) return;
  if (e == n_ent) { if (threadIdx.x == 0) ent_len[e] = 0; return; }
  const int64_t pos = (cont && e == 0) ? 0 : hdr_pos[e - cont];
  const int64_t end = pos + limit < N ? pos + limit : N;
  int64_t found = -1;
  for (int64_t q = pos; q < end && found < 0; q += 64) {
    const int64_t p = q + threadIdx.x;
    const unsigned long long hit = __ballot(p < end && buf[p] == '\n');
    if (hit) found = q + (__ffsll((long long)hit) - 1);
  }
  if (threadIdx.x == 0) {
    ent_pos[e] = (int32_t)pos;
    ent_len[e] = (int32_t)((found >= 0 ? found : end) - pos);
    ent_term[e] = found >= 0;
  }
}
__global__ void __launch_bounds__(64) rs_hdr_copy_kernel(const uint8_t* __restrict__ buf, const int32_t* __restrict__ ent_pos,
                                                         const int32_t* __restrict__ ent_off, uint8_t* __restrict__ side) {
  const int32_t e = (int32_t)blockIdx.x;
  const int32_t o = ent_off[e], n = ent_off[e + 1] - o;
  const uint8_t* src = buf + ent_pos[e];
  for (int32_t k = (int32_t)threadIdx.x; k < n; k += 64) side[o + k] = src[k];
}

using RsBuf = DevBuf<3, 4096>;

// what a batch works in; as many as there are batches in flight at once, reused from batch to batch
struct RsSlot {
  hipStream_t st = nullptr;
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  BgzfIntake in;
  RsBuf text, hdr, tile_kind, tile_m, tile_rest, tile_seg, tile_hdrs, tile_in, tile_kept, tile_off, tile_hb, tmp;
  RsBuf hdr_pos, hdr_out, ent_pos, ent_len, ent_term, ent_off, side;
  std::vector<int32_t> h_ent_len, h_ent_term, h_ent_pos, h_hdr_out;
  std::vector<uint8_t> h_side;
  ~RsSlot() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }
};

// a batch's output: out[start, start + n) of the whole, in HBM until svdss_ref_stream_finish and on the host
struct RsSegment {
  int64_t start = 0, n = 0;
  void* d = nullptr;
  std::unique_ptr<uint8_t[]> h;
};

}  // namespace

struct svdss_ref_stream {
  int device = 0;
  int64_t cap = 0;
  std::mutex m;
  std::condition_variable cv;
  int64_t next_seq = 0;
  int failed = 0;                  // SVDSS_E*: every later batch returns it
  int32_t declined = 0;            // SVDSS_REF_*: every later batch returns at once
  int64_t declined_at = 0;
  std::string err;
  bool done = false;               // the last batch had its turn
  // what a batch hands to the one behind it
  bool in_header = false, als = true;
  std::string carry;               // the header line the text ended in
  int64_t carry_out = 0, carry_at = 0;
  int64_t out_off = 0, text_off = 0;
  // the records so far
  std::vector<std::string> names;
  std::unordered_set<std::string> seen;
  std::vector<int64_t> seq_off, name_off;
  std::string names_flat;
  std::vector<RsSegment> segs;     // in file order
  bool finished = false;           // svdss_ref_stream_finish took the segments' device memory
  bool host_dropped = false;
  int64_t n_batches = 0;
  double inflate_ms = 0, parse_ms = 0;
  std::vector<std::unique_ptr<RsSlot>> idle;
};

namespace {

void rs_free_device(svdss_ref_stream* s) {
  for (RsSegment& g : s->segs) if (g.d) { (void)hipFree(g.d); g.d = nullptr; }
}
// (with the stream's lock held) nothing is delivered: the caller reads the file as it did before
void rs_decline(svdss_ref_stream* s, int32_t why, int64_t at, const std::string& msg) {
  if (s->declined) return;
  s->declined = why;
  s->declined_at = at;
  s->err = msg;
  rs_free_device(s);
  s->segs.clear();
  s->names.clear(); s->seen.clear(); s->seq_off.clear(); s->carry.clear();
}

// the scope of one batch: its slot goes back, and its turn is passed on, on every way out
struct RsRun {
  svdss_ref_stream* s;
  std::unique_ptr<RsSlot> slot;
  int64_t seq;
  int turn = 0;                    // 0 not taken yet, 1 held, 2 over
  RsRun(svdss_ref_stream* s_, int64_t seq_) : s(s_), seq(seq_) {}
  ~RsRun() {
    if (slot && slot->st) (void)hipStreamSynchronize(slot->st);
    std::lock_guard<std::mutex> lk(s->m);
    if (slot) s->idle.push_back(std::move(slot));
  }
  bool wait_turn() {
    std::unique_lock<std::mutex> lk(s->m);
    s->cv.wait(lk, [&] { return s->next_seq == seq || s->failed || s->declined; });
    if (s->failed || s->declined) { turn = 2; return false; }
    turn = 1;
    return true;
  }
  void end_turn() {
    { std::lock_guard<std::mutex> lk(s->m); ++s->next_seq; }
    turn = 2;
    s->cv.notify_all();
  }
  int fail(int code, const std::string& msg, int32_t why = 0) {
    {
      std::lock_guard<std::mutex> lk(s->m);
      if (!s->failed && !s->declined) { s->failed = code; rs_decline(s, why ? why : SVDSS_REF_ERROR, s->text_off, msg); }
      if (turn == 1) ++s->next_seq;
    }
    turn = 2;
    s->cv.notify_all();
    return code;
  }
  int scan_sum(const int32_t* in, int32_t* out, int64_t n) {
    return cub_twice(slot->tmp, slot->st, [&](void* t, size_t& tb, hipStream_t q, int) { return hipcub::DeviceScan::ExclusiveSum(t, tb, in, out, (int)n, q); });
  }
  int scan_max(const int32_t* in, int32_t* out, int64_t n) {
    return cub_twice(slot->tmp, slot->st, [&](void* t, size_t& tb, hipStream_t q, int) {
      return hipcub::DeviceScan::InclusiveScan(t, tb, in, out, hipcub::Max(), (int)n, q);
    });
  }
};

// (with the stream's lock held) a complete header line: one more record whose bases begin at `out`; false: declined
bool rs_record(svdss_ref_stream* s, const char* line, size_t len, int64_t out, int64_t at) {
  if ((int64_t)len > s->cap) { rs_decline(s, SVDSS_REF_LONG_HEADER, at, "a header line longer than the cap"); return false; }
  size_t e = 1;
  while (e < len && line[e] != ' ' && line[e] != '\t') ++e;
  std::string name(line + (len ? 1 : 0), len ? e - 1 : 0);
  if (!s->seen.insert(name).second) { rs_decline(s, SVDSS_REF_DUPLICATE, at, "the name " + name + " occurs twice"); return false; }
  s->names.push_back(std::move(name));
  s->seq_off.push_back(out);
  return true;
}

}  // namespace

extern "C" int32_t svdss_ref_stream_tile_bytes(void) { return RS_T; }

extern "C" int svdss_ref_stream_create(int32_t device, int64_t header_cap, svdss_ref_stream_t** out) {
  if (!out || device < 0 || header_cap < 1 || header_cap > ((int64_t)1 << 28)) return SVDSS_EINVAL;
  svdss_ref_stream* s = new (std::nothrow) svdss_ref_stream();
  if (!s) return SVDSS_ENOMEM;
  s->device = device;
  s->cap = header_cap;
  *out = s;
  return SVDSS_OK;
}

extern "C" void svdss_ref_stream_free(svdss_ref_stream_t* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  rs_free_device(s);
  s->idle.clear();
  delete s;
}

extern "C" const char* svdss_ref_stream_error(const svdss_ref_stream_t* s) { return s ? s->err.c_str() : ""; }

extern "C" int svdss_ref_stream_batch(svdss_ref_stream_t* s, int64_t seq, int32_t is_last, int32_t n_chunks,
                                      const uint8_t* const* comp, const int64_t* comp_bytes, const svdss_bgzf_block_t* const* blocks,
                                      const uint32_t* const* crc, const int64_t* n_blocks, const uint8_t* plain, int64_t plain_bytes) {
  if (!s || seq < 0 || n_chunks < 0 || plain_bytes < 0) return SVDSS_EINVAL;
  RsRun run(s, seq);
  {
    std::lock_guard<std::mutex> lk(s->m);
    if (s->failed) return s->failed;
    if (s->declined) return SVDSS_OK;
    if (!s->idle.empty()) { run.slot = std::move(s->idle.back()); s->idle.pop_back(); }
  }
  if (const char* m = bgzf_check_args(n_chunks, comp, comp_bytes, blocks, crc, n_blocks)) return run.fail(SVDSS_EINVAL, m);
  if (plain_bytes > 0 && (!plain || n_chunks > 0)) return run.fail(SVDSS_EINVAL, "bad argument");
  BCHK(hipSetDevice(s->device));
  if (!run.slot) {
    run.slot.reset(new (std::nothrow) RsSlot());
    if (!run.slot) return run.fail(SVDSS_ENOMEM, "out of memory");
  }
  RsSlot* b = run.slot.get();
  if (!b->st) BCHK(svdss_make_stream(&b->st, nullptr));
  for (hipEvent_t& e : b->ev) if (!e) BCHK(hipEventCreate(&e));
  const hipStream_t st = b->st;

  // ---- this batch's bytes into HBM: BGZF members inflated and checked, or plain bytes
  BgzfIntake& in = b->in;
  RCHK(in.plan(n_chunks, comp, comp_bytes, blocks, crc, n_blocks));
  const int64_t N = plain_bytes + in.P.inflated;
  if (N >= ((int64_t)1 << 30)) return run.fail(SVDSS_ERANGE, "batch too large");
  RCHK(b->text.ensure((size_t)N + 2 * RS_T));
  RCHK(b->hdr.ensure(sizeof(unsigned long long) * RH_N));
  uint8_t* const buf = (uint8_t*)b->text.p;
  double inflate_ms = 0, parse_ms = 0;
  if (plain_bytes > 0) {
    BCHK(hipMemcpyAsync(buf, plain, (size_t)plain_bytes, hipMemcpyHostToDevice, st));
    BCHK(hipStreamSynchronize(st));
  } else {
    RCHK(in.enqueue(st, b->ev[0], b->ev[1], buf, 0));
    RCHK(in.enqueue_status_download(st));
    BCHK(hipStreamSynchronize(st));
    if (const int rc = in.verdict(b->ev[0], b->ev[1], inflate_ms)) return run.fail(rc, g_svdss_hip_err, SVDSS_REF_IO);
  }
  // the segment the batch's output goes to: never more bytes than its text
  RsSegment seg;
  if (N > 0) {
    BCHK(hipMalloc(&seg.d, (size_t)N + 32));
    seg.h.reset(new (std::nothrow) uint8_t[(size_t)N]);
  }
  struct SegGuard { RsSegment& g; ~SegGuard() { if (g.d) (void)hipFree(g.d); } } guard{seg};
  if (N > 0 && !seg.h) return run.fail(SVDSS_ENOMEM, "out of memory");

  // ---- this batch's turn in file order
  if (!run.wait_turn()) return s->failed;
  const int seed = s->in_header ? 1 : 0, als0 = s->als ? 1 : 0, first = s->text_off == 0 ? 1 : 0;
  const int64_t n_tiles = (N + RS_T - 1) / RS_T;
  int32_t kept = 0, n_hdr = 0;
  bool in_header = s->in_header, als = s->als;
  if (N > 0) {
    for (RsBuf* q : {&b->tile_kind, &b->tile_m, &b->tile_rest, &b->tile_seg, &b->tile_hdrs, &b->tile_in, &b->tile_kept, &b->tile_off, &b->tile_hb})
      RCHK(q->ensure(sizeof(int32_t) * (size_t)(n_tiles + 2)));
    unsigned long long h0[RH_N] = {RS_NONE, 0};
    BCHK(hipMemcpyAsync(b->hdr.p, h0, sizeof h0, hipMemcpyHostToDevice, st));
    BCHK(hipMemsetAsync((int32_t*)b->tile_hdrs.p + n_tiles, 0, sizeof(int32_t), st));
    BCHK(hipEventRecord(b->ev[2], st));
    hipLaunchKernelGGL(rs_tile_kernel, dim3((unsigned)n_tiles), dim3(RS_TPB), 0, st, (const uint8_t*)buf, N, als0, first, (int32_t*)b->tile_kind.p,
                       (int32_t*)b->tile_rest.p, (int32_t*)b->tile_seg.p, (int32_t*)b->tile_hdrs.p, (unsigned long long*)b->hdr.p);
    BCHK(hipGetLastError());
    RCHK(run.scan_max((const int32_t*)b->tile_kind.p, (int32_t*)b->tile_m.p, n_tiles));
    hipLaunchKernelGGL(rs_tiles_kernel, dim3((unsigned)((n_tiles + 256) / 256)), dim3(256), 0, st, (const int32_t*)b->tile_m.p, (const int32_t*)b->tile_rest.p,
                       (const int32_t*)b->tile_seg.p, (int32_t)n_tiles, seed, (int32_t*)b->tile_in.p, (int32_t*)b->tile_kept.p);
    BCHK(hipGetLastError());
    RCHK(run.scan_sum((const int32_t*)b->tile_kept.p, (int32_t*)b->tile_off.p, n_tiles + 1));
    RCHK(run.scan_sum((const int32_t*)b->tile_hdrs.p, (int32_t*)b->tile_hb.p, n_tiles + 1));
    BCHK(hipEventRecord(b->ev[3], st));
    int32_t m_last = -1;
    unsigned long long h1[RH_N];
    BCHK(hipMemcpyAsync(&kept, (int32_t*)b->tile_off.p + n_tiles, sizeof kept, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&n_hdr, (int32_t*)b->tile_hb.p + n_tiles, sizeof n_hdr, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&m_last, (int32_t*)b->tile_m.p + (n_tiles - 1), sizeof m_last, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(h1, b->hdr.p, sizeof h1, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev[2], b->ev[3]) == hipSuccess) parse_ms += ms;
    if (h1[RH_BAD] != RS_NONE) {
      static const char* const what[] = {"", "a carriage return", "a NUL byte", "a line that begins with '@'", "the first byte is not '>'"};
      const int32_t why = (int32_t)(h1[RH_BAD] & 15);
      {
        std::lock_guard<std::mutex> lk(s->m);
        rs_decline(s, why, s->text_off + (int64_t)(h1[RH_BAD] >> 4), what[why < 5 ? why : 0]);
      }
      run.end_turn();
      return SVDSS_OK;
    }
    in_header = m_last < 0 ? s->in_header : (m_last & 1) != 0;
    als = h1[RH_LASTNL] != 0;
    const int32_t n_ent = seed + n_hdr;
    RCHK(b->hdr_pos.ensure(sizeof(int32_t) * (size_t)(n_hdr + 1)));
    RCHK(b->hdr_out.ensure(sizeof(int32_t) * (size_t)(n_hdr + 1)));
    BCHK(hipEventRecord(b->ev[4], st));
    hipLaunchKernelGGL(rs_gather_kernel, dim3((unsigned)n_tiles), dim3(RS_TPB), 0, st, (const uint8_t*)buf, N, als0, (const int32_t*)b->tile_in.p,
                       (const int32_t*)b->tile_off.p, (const int32_t*)b->tile_hb.p, (uint8_t*)seg.d, (int32_t*)b->hdr_pos.p, (int32_t*)b->hdr_out.p);
    BCHK(hipGetLastError());
    int32_t side_bytes = 0;
    if (n_ent > 0) {
      for (RsBuf* q : {&b->ent_pos, &b->ent_len, &b->ent_term, &b->ent_off}) RCHK(q->ensure(sizeof(int32_t) * (size_t)(n_ent + 2)));
      const int32_t limit = (int32_t)std::min<int64_t>(s->cap + 1, N);
      hipLaunchKernelGGL(rs_hdr_len_kernel, dim3((unsigned)(n_ent + 1)), dim3(64), 0, st, (const uint8_t*)buf, N, (const int32_t*)b->hdr_pos.p, seed, n_ent,
                         limit, (int32_t*)b->ent_pos.p, (int32_t*)b->ent_len.p, (int32_t*)b->ent_term.p);
      BCHK(hipGetLastError());
      RCHK(run.scan_sum((const int32_t*)b->ent_len.p, (int32_t*)b->ent_off.p, (int64_t)n_ent + 1));
      BCHK(hipEventRecord(b->ev[5], st));
      BCHK(hipMemcpyAsync(&side_bytes, (int32_t*)b->ent_off.p + n_ent, sizeof side_bytes, hipMemcpyDeviceToHost, st));
      BCHK(hipStreamSynchronize(st));
      if (hipEventElapsedTime(&ms, b->ev[4], b->ev[5]) == hipSuccess) parse_ms += ms;
      RCHK(b->side.ensure((size_t)side_bytes + 16));
      BCHK(hipEventRecord(b->ev[6], st));
      hipLaunchKernelGGL(rs_hdr_copy_kernel, dim3((unsigned)n_ent), dim3(64), 0, st, (const uint8_t*)buf, (const int32_t*)b->ent_pos.p,
                         (const int32_t*)b->ent_off.p, (uint8_t*)b->side.p);
      BCHK(hipGetLastError());
      BCHK(hipEventRecord(b->ev[7], st));
      try {
        b->h_ent_len.resize((size_t)n_ent); b->h_ent_term.resize((size_t)n_ent); b->h_ent_pos.resize((size_t)n_ent);
        b->h_hdr_out.resize((size_t)n_hdr + 1); b->h_side.resize((size_t)side_bytes + 1);
      } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
      BCHK(hipMemcpyAsync(b->h_ent_len.data(), b->ent_len.p, sizeof(int32_t) * (size_t)n_ent, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(b->h_ent_term.data(), b->ent_term.p, sizeof(int32_t) * (size_t)n_ent, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(b->h_ent_pos.data(), b->ent_pos.p, sizeof(int32_t) * (size_t)n_ent, hipMemcpyDeviceToHost, st));
      if (n_hdr > 0) BCHK(hipMemcpyAsync(b->h_hdr_out.data(), b->hdr_out.p, sizeof(int32_t) * (size_t)n_hdr, hipMemcpyDeviceToHost, st));
      if (side_bytes > 0) BCHK(hipMemcpyAsync(b->h_side.data(), b->side.p, (size_t)side_bytes, hipMemcpyDeviceToHost, st));
      BCHK(hipStreamSynchronize(st));
      if (hipEventElapsedTime(&ms, b->ev[6], b->ev[7]) == hipSuccess) parse_ms += ms;
    } else {
      BCHK(hipEventRecord(b->ev[5], st));
      BCHK(hipStreamSynchronize(st));
      if (hipEventElapsedTime(&ms, b->ev[4], b->ev[5]) == hipSuccess) parse_ms += ms;
    }
    // the header lines, in text order: the one that goes on from the batch in front, the complete ones, the one that goes on
    std::lock_guard<std::mutex> lk(s->m);
    bool ok = true;
    int64_t side_at = 0;
    for (int32_t e = 0; e < n_ent && ok; ++e) {
      const char* text = (const char*)b->h_side.data() + side_at;
      const int32_t len = b->h_ent_len[(size_t)e];
      side_at += len;
      const bool term = b->h_ent_term[(size_t)e] != 0;
      const int64_t at = s->text_off + b->h_ent_pos[(size_t)e];
      if (seed && e == 0) {
        s->carry.append(text, (size_t)len);
        if ((int64_t)s->carry.size() > s->cap) { rs_decline(s, SVDSS_REF_LONG_HEADER, s->carry_at, "a header line longer than the cap"); ok = false; }
        else if (term) { ok = rs_record(s, s->carry.data(), s->carry.size(), s->carry_out, s->carry_at); s->carry.clear(); }
        continue;
      }
      const int64_t out = s->out_off + b->h_hdr_out[(size_t)(e - seed)];
      if (term) ok = rs_record(s, text, (size_t)len, out, at);
      else if ((int64_t)len > s->cap) { rs_decline(s, SVDSS_REF_LONG_HEADER, at, "a header line longer than the cap"); ok = false; }
      else { s->carry.assign(text, (size_t)len); s->carry_out = out; s->carry_at = at; }
    }
    if (!ok) {
      ++s->next_seq;
      run.turn = 2;
      s->cv.notify_all();
      return SVDSS_OK;
    }
  }
  {
    std::lock_guard<std::mutex> lk(s->m);
    seg.start = s->out_off;
    seg.n = kept;
    s->in_header = in_header;
    s->als = als;
    s->out_off += kept;
    s->text_off += N;
    ++s->n_batches;
    s->inflate_ms += inflate_ms;
    s->parse_ms += parse_ms;
    bool ok = true;
    if (is_last) {
      if (s->text_off == 0) { rs_decline(s, SVDSS_REF_EMPTY, 0, "the file is empty"); ok = false; }
      else if (s->in_header) { ok = rs_record(s, s->carry.data(), s->carry.size(), s->carry_out, s->carry_at); s->carry.clear(); }   // a last header line without '\n'
      if (ok) {
        s->seq_off.push_back(s->out_off);
        s->name_off.assign(1, 0);
        for (const std::string& nm : s->names) { s->names_flat += nm; s->name_off.push_back((int64_t)s->names_flat.size()); }
        s->done = true;
      }
    }
    if (!ok) {
      ++s->next_seq;
      run.turn = 2;
      s->cv.notify_all();
      return SVDSS_OK;
    }
  }
  // ---- the output down to the host copy, beside the batches behind this one (the segment's memory is the stream's from
  // here on: it is entered when the bytes are down, under the lock)
  uint8_t* const h = seg.h.get();
  void* const d = seg.d;
  const int64_t n_out = kept;
  run.end_turn();
  if (n_out > 0) {
    BCHK(hipMemcpyAsync(h, d, (size_t)n_out, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
  }
  {
    std::lock_guard<std::mutex> lk(s->m);
    if (s->declined || s->failed) return s->failed;      // (declined meanwhile: the guard frees the segment)
    if (n_out > 0) {
      auto it = std::lower_bound(s->segs.begin(), s->segs.end(), seg.start, [](const RsSegment& g, int64_t v) { return g.start < v; });
      s->segs.insert(it, std::move(seg));
      seg.d = nullptr;
    }
  }
  return SVDSS_OK;
}

extern "C" int svdss_ref_stream_result(const svdss_ref_stream_t* s, svdss_ref_stream_result_t* r) {
  if (!s || !r) return SVDSS_EINVAL;
  memset(r, 0, sizeof *r);
  r->declined = s->declined;
  r->declined_at = s->declined_at;
  r->n_batches = s->n_batches;
  r->text_bytes = s->text_off;
  r->inflate_kernel_ms = s->inflate_ms;
  r->parse_kernel_ms = s->parse_ms;
  if (s->declined || !s->done) return s->declined ? SVDSS_OK : SVDSS_EINVAL;
  r->n_records = (int64_t)s->names.size();
  r->name_off = s->name_off.data();
  r->names = s->names_flat.data();
  r->seq_off = s->seq_off.data();
  return SVDSS_OK;
}

extern "C" int svdss_ref_stream_download(const svdss_ref_stream_t* s, int64_t rec, uint8_t* dst) {
  if (!s || !s->done || s->declined || s->host_dropped || rec < 0 || rec >= (int64_t)s->names.size()) return SVDSS_EINVAL;
  const int64_t a = s->seq_off[(size_t)rec], b = s->seq_off[(size_t)rec + 1];
  if (b > a && !dst) return SVDSS_EINVAL;
  const bool ok = ref_pieces(s->segs, a, b, [&](const RsSegment& g, int64_t from, int64_t n, int64_t to) { memcpy(dst + to, g.h.get() + from, (size_t)n); return true; });
  return ok ? SVDSS_OK : SVDSS_EINVAL;
}

extern "C" void svdss_ref_stream_drop_host(svdss_ref_stream_t* s) {
  if (!s) return;
  for (RsSegment& g : s->segs) g.h.reset();
  s->host_dropped = true;
}

extern "C" int svdss_ref_stream_finish(svdss_ref_stream_t* s, const int32_t* order, int32_t n, int32_t device, svdss_ref_t** out) {
  if (!s || !out || n < 0 || (n > 0 && !order) || !s->done || s->declined || s->finished || device != s->device) return SVDSS_EINVAL;
  std::vector<int64_t> off((size_t)n + 1, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (order[i] < 0 || order[i] >= (int32_t)s->names.size()) return SVDSS_EINVAL;
    off[(size_t)i + 1] = off[(size_t)i] + (s->seq_off[(size_t)order[i] + 1] - s->seq_off[(size_t)order[i]]);
  }
  HIPCHK(hipSetDevice(device));
  void *d_seq = nullptr, *d_off = nullptr;
  auto fail = [&](int code) { if (d_seq) (void)hipFree(d_seq); if (d_off) (void)hipFree(d_off); return code; };
  if (hipMalloc(&d_seq, (size_t)off[(size_t)n] + 16) != hipSuccess || hipMalloc(&d_off, sizeof(int64_t) * (size_t)(n + 1)) != hipSuccess) return fail(SVDSS_ENOMEM);
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(SVDSS_EHIP);
  bool ok = hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st) == hipSuccess;
  for (int32_t i = 0; i < n && ok; ++i) {
    const int64_t a = s->seq_off[(size_t)order[i]], b = s->seq_off[(size_t)order[i] + 1];
    ok = ref_pieces(s->segs, a, b, [&](const RsSegment& g, int64_t from, int64_t cnt, int64_t to) {
      return hipMemcpyAsync((uint8_t*)d_seq + off[(size_t)i] + to, (const uint8_t*)g.d + from, (size_t)cnt, hipMemcpyDeviceToDevice, st) == hipSuccess;
    });
  }
  ok = hipStreamSynchronize(st) == hipSuccess && ok;
  (void)hipStreamDestroy(st);
  if (!ok) return fail(SVDSS_EHIP);
  const int rc = svdss_ref_adopt(device, d_seq, d_off, n, out);
  if (rc != SVDSS_OK) return fail(rc);
  rs_free_device(s);
  s->finished = true;
  return SVDSS_OK;
}
