// fastx_device.hip -- `SVDSS search --fastx` with the records found where the text is inflated (gfx950).
//
// Stands where the kseq loop of the reference stands (/root/reference/ping_pong.cpp:130-173: kseq_read per record, then
// rb3_char2nt6 per base :158; fastq.hpp:17-35) and where csrc/fastx_reader.h stands on the host path.  A batch is a run of
// text bytes in HBM -- the bytes the previous batch left behind its last complete record (the carry), then this batch's
// bytes: BGZF members inflated by csrc/inflate.hip and checked against their CRC32, or plain bytes uploaded.  The run
// starts at a record start by construction.  Out come a record table (name, sequence length) and the reads as
// svdss_sfs_search_batch_device takes them: nt6 symbols back to back with int64 offsets.
//
// The parser does not guess.  It knows two shapes and proves, in the same pass, that FastxReader::next returns the same
// records (tests/mirror/fastx.py restates both and holds them against the reader):
//   FASTA ('>' first): no '\r', no NUL, no line that begins with '@'; a record begins at every line that begins with
//          '>', its sequence is every other line up to the next such line; empty lines add nothing.
//   FASTQ ('@' first): no '\r', no NUL; lines in groups of four from the start of the stream: '@' line, a line that
//          begins with neither '>' nor '+', a '+' line, a line as long as the second; empty lines only behind the last
//          group at the end of the stream.
// Anything else is DECLINED: the batch delivers the records it proved in front of that point, says where the first
// unparsed byte is and hands the text from there to the caller, who reads on with FastxReader; every later batch of the
// stream only inflates and hands its text down.
//
// Launches per batch (T = 4096 bytes per workgroup, 16 bytes per lane):
//   fx_tile_kernel      newlines per tile; the first '\r' / NUL of the text
//   (scan)              tile -> index of its first line
//   fx_lines_kernel     where every line starts
//   fx_classify_kernel  per line (FASTA) or group of four (FASTQ): header flag, sequence length, the first line that
//                       breaks the shape
//   fx_limit_kernel / fx_mask_kernel   the line the proved records end at; what lies behind it counts for nothing
//   (scans)             line -> record index, line -> position of its bases in the output
//   -- the carry is known here: the batch's turn in file order ends, the rest overlaps with the other batches --
//   fx_records_kernel, (scan), fx_names_kernel   header line, offsets and name of every record
//   fx_gather_kernel    nt6 of every sequence byte at its output position (a tile's bases are contiguous in the
//                       output: compacted in LDS, stored coalesced)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bgzf_intake.h"
#include "index_host.h"

namespace {

constexpr int FX_T = 4096;      // bytes per tile
constexpr int FX_TPB = 256;     // 16 bytes per lane
enum { X_BADPOS = 0, X_LASTNL = 1, X_BADLINE = 2, X_HMAX = 3, X_LIMIT = 4, X_CARRY = 5, X_N = 8 };
constexpr unsigned long long X_NONE = 0x7fffffffffffffffull;

__device__ __forceinline__ uint32_t byte_of(const uint4& v, int k) {
  const uint32_t w = k < 8 ? (k < 4 ? v.x : v.y) : (k < 12 ? v.z : v.w);
  return (w >> (8 * (k & 3))) & 0xffu;
}
// the mapping of svdss_nt6_encode: A/a 1, C/c 2, G/g 3, T/t 4, everything else 5
__device__ __forceinline__ uint8_t nt6_of(uint32_t c) {
  const uint32_t l = c | 0x20u;
  return l == 'a' ? 1 : l == 'c' ? 2 : l == 'g' ? 3 : l == 't' ? 4 : 5;
}

// the text is buf[lo, hi); tiles are cut at multiples of FX_T from `base` (lo rounded down): every load is 16 aligned bytes
__global__ void __launch_bounds__(FX_TPB) fx_tile_kernel(const uint8_t* __restrict__ buf, int64_t base, int64_t lo, int64_t hi,
                                                         int32_t* __restrict__ tile_nl, unsigned long long* hdr) {
  typedef hipcub::BlockReduce<int, FX_TPB> Red;
  __shared__ typename Red::TempStorage tmp;
  const int64_t p0 = base + (int64_t)blockIdx.x * FX_T + (int64_t)threadIdx.x * 16;
  int nl = 0;
  int64_t bad = -1;
  if (p0 < hi && p0 + 16 > lo) {
    const uint4 v = *(const uint4*)(buf + p0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int64_t p = p0 + k;
      if (p < lo || p >= hi) continue;
      const uint32_t c = byte_of(v, k);
      nl += c == '\n';
      if ((c == '\r' || c == 0) && bad < 0) bad = p - lo;
      if (p == hi - 1) hdr[X_LASTNL] = c == '\n';
    }
  }
  const int tot = Red(tmp).Sum(nl);
  if (threadIdx.x == 0) tile_nl[blockIdx.x] = tot;
  if (bad >= 0) atomicMin(&hdr[X_BADPOS], (unsigned long long)bad);
}

// ls[i] = where line i starts, relative to lo (ls[0] = 0; the entry behind the last line is the host's)
__global__ void __launch_bounds__(FX_TPB) fx_lines_kernel(const uint8_t* __restrict__ buf, int64_t base, int64_t lo, int64_t hi,
                                                          const int32_t* __restrict__ tile_base, int32_t* __restrict__ ls) {
  typedef hipcub::BlockScan<int, FX_TPB> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const int64_t p0 = base + (int64_t)blockIdx.x * FX_T + (int64_t)threadIdx.x * 16;
  int nl = 0;
  uint4 v = make_uint4(0, 0, 0, 0);
  const bool mine = p0 < hi && p0 + 16 > lo;
  if (mine) {
    v = *(const uint4*)(buf + p0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int64_t p = p0 + k;
      nl += (p >= lo && p < hi && byte_of(v, k) == '\n');
    }
  }
  int before = 0;
  Scan(tmp).ExclusiveSum(nl, before);
  if (blockIdx.x == 0 && threadIdx.x == 0) ls[0] = 0;
  if (!mine || nl == 0) return;
  int idx = tile_base[blockIdx.x] + before;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t p = p0 + k;
    if (p >= lo && p < hi && byte_of(v, k) == '\n') ls[++idx] = (int32_t)(p + 1 - lo);
  }
}

struct FxP {
  const uint8_t* text;      // buf + lo
  const int32_t* ls;        // L + 1 line starts: line i is text[ls[i], ls[i + 1] - 1)
  int32_t L, Lc, N;         // lines, complete lines (a last line without '\n' counts at the end of the stream only), bytes
  int32_t fastq, is_last;
  int32_t* hflag;           // L + 1: the line begins a record
  int32_t* slen;            // L + 1: bases the line adds to its record
  unsigned long long* hdr;
};

__global__ void __launch_bounds__(256) fx_classify_kernel(FxP P) {
  const int32_t i = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (i > P.L) return;
  if (i == P.L) { P.hflag[i] = 0; P.slen[i] = 0; return; }
  const unsigned long long badpos = P.hdr[X_BADPOS];
  const int32_t s = P.ls[i], len = P.ls[i + 1] - 1 - s;
  if (!P.fastq) {
    const uint32_t c = len > 0 ? P.text[s] : '\n';
    const int h = c == '>';
    P.hflag[i] = h;
    P.slen[i] = h ? 0 : len;
    if (c == '@' || (badpos >= (unsigned long long)s && badpos < (unsigned long long)P.ls[i + 1]))
      atomicMin(&P.hdr[X_BADLINE], (unsigned long long)i);
    return;
  }
  const int32_t G4 = P.Lc / 4 * 4;
  if (i >= G4) {
    // behind the last complete group: the next batch's, or -- at the end of the stream -- empty lines
    P.hflag[i] = 0; P.slen[i] = 0;
    if ((P.is_last && len > 0) || (badpos >= (unsigned long long)s && badpos < (unsigned long long)P.ls[i + 1]))
      atomicMin(&P.hdr[X_BADLINE], (unsigned long long)G4);
    return;
  }
  if (i & 3) return;
  const int32_t s1 = P.ls[i + 1], s2 = P.ls[i + 2], s3 = P.ls[i + 3], e = P.ls[i + 4];
  const int32_t len1 = s2 - 1 - s1, len2 = s3 - 1 - s2, len3 = e - 1 - s3;
  const bool ok = len >= 1 && P.text[s] == '@' && !(len1 > 0 && (P.text[s1] == '>' || P.text[s1] == '+')) &&
                  len2 >= 1 && P.text[s2] == '+' && len3 == len1;
  P.hflag[i] = 1; P.hflag[i + 1] = 0; P.hflag[i + 2] = 0; P.hflag[i + 3] = 0;
  P.slen[i] = 0; P.slen[i + 1] = len1; P.slen[i + 2] = 0; P.slen[i + 3] = 0;
  if (!ok || (badpos >= (unsigned long long)s && badpos < (unsigned long long)e)) atomicMin(&P.hdr[X_BADLINE], (unsigned long long)i);
}
// FASTA: the last header line at or in front of the first line that breaks the shape -- the record it opens is not proved
__global__ void __launch_bounds__(256) fx_limit_kernel(FxP P) {
  const int32_t i = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (i >= P.L || !P.hflag[i]) return;
  if ((unsigned long long)i <= P.hdr[X_BADLINE]) atomicMax(&P.hdr[X_HMAX], (unsigned long long)i);
}
// the proved records end in front of line `limit`: the lines from there on count for nothing
__global__ void __launch_bounds__(256) fx_mask_kernel(FxP P) {
  const int32_t i = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (i > P.L) return;
  const unsigned long long badline = P.hdr[X_BADLINE];
  int32_t limit;
  if (P.fastq) limit = badline < (unsigned long long)(P.Lc / 4 * 4) ? (int32_t)badline : P.Lc / 4 * 4;
  else limit = (badline == X_NONE && P.is_last) ? P.L : (int32_t)P.hdr[X_HMAX];
  if (i >= limit) { P.hflag[i] = 0; P.slen[i] = 0; }
  if (i == 0) {
    P.hdr[X_LIMIT] = (unsigned long long)limit;
    P.hdr[X_CARRY] = (unsigned long long)(limit < P.L ? P.ls[limit] : P.N);
  }
}

struct FxR {
  const uint8_t* text;
  const int32_t* ls;
  const int32_t* hflag;
  const int32_t* ridx;      // exclusive sums of hflag
  const int32_t* spos;      // exclusive sums of slen
  int32_t L, n_rec;
  int32_t* hline;           // n_rec
  int32_t* name_len;        // n_rec + 1
  int64_t* off;             // n_rec + 1
};
__global__ void __launch_bounds__(256) fx_records_kernel(FxR R) {
  const int32_t i = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (i > R.L) return;
  if (i == R.L) { R.off[R.n_rec] = R.spos[R.L]; R.name_len[R.n_rec] = 0; return; }
  if (!R.hflag[i]) return;
  const int32_t r = R.ridx[i];
  R.hline[r] = i;
  R.off[r] = R.spos[i];
  // the name: the header without its first byte, up to the first blank, tab or end of line
  const int32_t s = R.ls[i] + 1, e = R.ls[i + 1] - 1;
  int32_t q = s;
  while (q < e && R.text[q] != ' ' && R.text[q] != '\t') ++q;
  R.name_len[r] = q - s;
}
__global__ void __launch_bounds__(256) fx_names_kernel(FxR R, const int32_t* __restrict__ name_off, char* __restrict__ names, int32_t* __restrict__ seq_len) {
  const int32_t r = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (r >= R.n_rec) return;
  seq_len[r] = (int32_t)(R.off[r + 1] - R.off[r]);
  const uint8_t* src = R.text + R.ls[R.hline[r]] + 1;
  char* dst = names + name_off[r];
  const int32_t n = name_off[r + 1] - name_off[r];
  for (int32_t k = 0; k < n; ++k) dst[k] = (char)src[k];
}

// The bases of a tile, in the order they stand in the text, are consecutive in the output (the output IS the text without
// its headers, separators, qualities and newlines): every lane finds the output position of its bytes from its line's
// (spos - ls), the tile's symbols are compacted in LDS and leave as one contiguous run.
__global__ void __launch_bounds__(FX_TPB) fx_gather_kernel(const uint8_t* __restrict__ buf, int64_t base, int64_t lo, int64_t hi,
                                                           const int32_t* __restrict__ tile_base, const int32_t* __restrict__ ls,
                                                           const int32_t* __restrict__ slen, const int32_t* __restrict__ spos,
                                                           const unsigned long long* __restrict__ hdr, uint8_t* __restrict__ out) {
  typedef hipcub::BlockScan<int, FX_TPB> Scan;
  typedef hipcub::BlockReduce<int, FX_TPB> Red;
  __shared__ union { typename Scan::TempStorage scan; typename Red::TempStorage red; } tmp;
  __shared__ uint8_t sym[FX_T];
  __shared__ int s_first, s_count;
  const int32_t limit = (int32_t)hdr[X_LIMIT];
  const int64_t p0 = base + (int64_t)blockIdx.x * FX_T + (int64_t)threadIdx.x * 16;
  const bool mine = p0 < hi && p0 + 16 > lo;
  uint4 v = make_uint4(0, 0, 0, 0);
  int nl = 0;
  if (mine) {
    v = *(const uint4*)(buf + p0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int64_t p = p0 + k;
      nl += (p >= lo && p < hi && byte_of(v, k) == '\n');
    }
  }
  int before = 0;
  Scan(tmp.scan).ExclusiveSum(nl, before);
  __syncthreads();
  int op[16];
  int first = INT_MAX, cnt = 0;
  if (mine) {
    int line = tile_base[blockIdx.x] + before;
    bool isseq = line < limit && slen[line] > 0;
    int delta = isseq ? spos[line] - ls[line] : 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int64_t p = p0 + k;
      op[k] = -1;
      if (p < lo || p >= hi) continue;
      if (byte_of(v, k) == '\n') {
        ++line;
        isseq = line < limit && slen[line] > 0;
        delta = isseq ? spos[line] - ls[line] : 0;
      } else if (isseq) {
        op[k] = delta + (int)(p - lo);
        if (first == INT_MAX) first = op[k];
        ++cnt;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) op[k] = -1;
  }
  const int bfirst = Red(tmp.red).Reduce(first, hipcub::Min());
  __syncthreads();
  const int bcnt = Red(tmp.red).Sum(cnt);
  if (threadIdx.x == 0) { s_first = bfirst; s_count = bcnt; }
  __syncthreads();
  const int tb = s_first, n = s_count;
  if (n == 0) return;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (op[k] >= 0) sym[op[k] - tb] = nt6_of(byte_of(v, k));
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += FX_TPB) out[(int64_t)tb + j] = sym[j];
}

using FxBuf = DevBuf<3, 4096>;

}  // namespace

struct svdss_fastx_stream {
  int device = 0;
  int64_t cap = 0;                 // a carry longer than this declines
  std::mutex m;
  std::condition_variable cv;
  int64_t next_seq = 0;
  int failed = 0;
  std::string err;
  int shape = 0;                   // 0 not known yet, '>' FASTA, '@' FASTQ
  bool fallen = false;             // a batch declined: the batches behind it only hand their text down
  std::vector<uint8_t> carry;      // the bytes behind the last proved record of the batch that had its turn last
};

struct svdss_fastx_batch {
  int device = -1;
  hipStream_t st = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::string err;
  BgzfIntake in;
  FxBuf buf, hdr, tile_nl, tile_base, ls, hflag, slen, ridx, spos, tmp, hline, name_len, name_off, off, seq_len, names, reads;
  svdss_sfs_batch_t* sfs = nullptr;
  // the last run's results on the host
  int64_t n_records = 0, total_sfs = 0, n_text = 0;
  int32_t declined = 0;
  bool parse_only = false;
  std::vector<int32_t> h_name_off, h_seq_len, h_qs, h_len;
  std::vector<char> h_names;
  std::vector<int64_t> h_counts, h_off;
  std::vector<uint8_t> h_reads, h_text;
  double inflate_ms = 0, parse_ms = 0, stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int32_t sentinel = 0;
};

namespace {

// the scope of one run: the one way out on failure passes the turn on (or gives it up) with the failure
struct FxRun {
  svdss_fastx_stream* s;
  svdss_fastx_batch* b = nullptr;
  int64_t seq;
  int turn = 0;                    // 0 not taken yet, 1 held, 2 over
  std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
  FxRun(svdss_fastx_stream* s_, int64_t seq_) : s(s_), seq(seq_) {}
  void lap(int k) {
    const auto t = std::chrono::steady_clock::now();
    b->stage_ms[k] = std::chrono::duration<double, std::milli>(t - t_prev).count();
    t_prev = t;
  }
  int fail(int code, const std::string& msg) {
    if (b) {
      b->err = msg;
      if (b->st) (void)hipStreamSynchronize(b->st);   // (the caller recycles its buffers as soon as this returns)
    }
    if (turn == 0) pass_turn(s, &svdss_fastx_stream::next_seq, seq, code, msg);
    else if (turn == 1) done_turn(s, &svdss_fastx_stream::next_seq, code, msg);
    turn = 2;
    return code;
  }
  int scan(const int32_t* in, int32_t* out, int64_t n) {
    return cub_twice(b->tmp, b->st, [&](void* t, size_t& tb, hipStream_t q, int) { return hipcub::DeviceScan::ExclusiveSum(t, tb, in, out, (int)n, q); });
  }
};

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int32_t svdss_fastx_tile_bytes(void) { return FX_T; }

extern "C" int svdss_fastx_stream_create(int32_t device, int64_t carry_cap, svdss_fastx_stream_t** out) {
  if (!out || device < 0 || carry_cap < 0) return SVDSS_EINVAL;
  svdss_fastx_stream* s = new (std::nothrow) svdss_fastx_stream();
  if (!s) return SVDSS_ENOMEM;
  s->device = device;
  s->cap = carry_cap;
  *out = s;
  return SVDSS_OK;
}
extern "C" void svdss_fastx_stream_free(svdss_fastx_stream_t* s) { delete s; }
extern "C" const char* svdss_fastx_stream_error(const svdss_fastx_stream_t* s) { return s ? s->err.c_str() : ""; }
extern "C" const char* svdss_fastx_batch_error(const svdss_fastx_batch_t* b) { return b ? b->err.c_str() : ""; }

extern "C" void svdss_fastx_batch_free(svdss_fastx_batch_t* b) {
  if (!b) return;
  if (b->device >= 0) (void)hipSetDevice(b->device);
  for (hipEvent_t e : b->ev) if (e) (void)hipEventDestroy(e);
  if (b->st) (void)hipStreamDestroy(b->st);
  if (b->sfs) svdss_sfs_batch_free(b->sfs);
  delete b;
}

extern "C" int svdss_fastx_batch_run(svdss_fastx_stream_t* s, int64_t seq, int32_t is_last, const svdss_index_t* ix,
                                     int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                     const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                     const uint8_t* plain, int64_t plain_bytes, int32_t flags, svdss_fastx_batch_t** out) {
  if (!s || !out || seq < 0 || n_chunks < 0 || plain_bytes < 0) return SVDSS_EINVAL;
  if (ix && (ix->device < 0 || !ix->d_blocks)) return SVDSS_ENODEV;   // (the caller's mistake: the stream's turn is not taken)
  FxRun run(s, seq);
  if (const char* m = bgzf_check_args(n_chunks, comp, comp_bytes, blocks, crc, n_blocks)) return run.fail(SVDSS_EINVAL, m);
  if (plain_bytes > 0 && (!plain || n_chunks > 0)) return run.fail(SVDSS_EINVAL, "bad argument");
  const int device = ix ? ix->device : s->device;
  BCHK(hipSetDevice(device));
  if (!*out) {
    *out = new (std::nothrow) svdss_fastx_batch();
    if (!*out) return run.fail(SVDSS_ENOMEM, "out of memory");
    (*out)->device = device;
  }
  svdss_fastx_batch* b = run.b = *out;
  if (b->device != device) return run.fail(SVDSS_EINVAL, "batch object of another device");
  if (!b->st) BCHK(svdss_make_stream(&b->st, "SVDSS_SEARCH_CUS"));
  for (hipEvent_t& e : b->ev) if (!e) BCHK(hipEventCreate(&e));
  const hipStream_t st = b->st;
  b->err.clear();
  b->n_records = b->total_sfs = b->n_text = 0;
  b->declined = 0;
  b->parse_only = ix == nullptr;
  b->inflate_ms = b->parse_ms = 0;
  for (double& x : b->stage_ms) x = 0;
  b->h_text.clear();
  run.t_prev = std::chrono::steady_clock::now();

  // ---- this batch's bytes into HBM, behind the room for the carry: BGZF members inflated and checked, or plain bytes
  BgzfIntake& in = b->in;
  RCHK(in.plan(n_chunks, comp, comp_bytes, blocks, crc, n_blocks));
  const int64_t fresh = plain_bytes + in.P.inflated;
  const int64_t HEAD = (s->cap + FX_T - 1) / FX_T * FX_T + FX_T;
  if (HEAD + fresh >= ((int64_t)1 << 31) - 4 * FX_T) return run.fail(SVDSS_ERANGE, "batch too large");
  RCHK(b->buf.ensure((size_t)(HEAD + fresh) + 2 * FX_T));
  RCHK(b->hdr.ensure(sizeof(int64_t) * X_N));
  uint8_t* const buf = (uint8_t*)b->buf.p;
  if (plain_bytes > 0) {
    BCHK(hipMemcpyAsync(buf + HEAD, plain, (size_t)plain_bytes, hipMemcpyHostToDevice, st));
    BCHK(hipStreamSynchronize(st));
  } else {
    RCHK(in.enqueue(st, b->ev[0], b->ev[1], buf, HEAD));
    RCHK(in.enqueue_status_download(st));
    BCHK(hipStreamSynchronize(st));
    RCHK(in.verdict(b->ev[0], b->ev[1], b->inflate_ms));
  }
  run.lap(0);   // buffers, upload, inflate, CRC

  // ---- this batch's turn in file order: carry in, the lines, the shape, the line the proved records end at, carry out
  if (!wait_turn(s, &svdss_fastx_stream::next_seq, seq)) { run.turn = 2; return run.fail(s->failed, s->err); }
  run.turn = 1;
  run.lap(1);
  auto text_down = [&](int64_t from, int64_t to) -> hipError_t {   // buf[from, to) -> h_text
    try { b->h_text.resize((size_t)(to - from)); } catch (...) { return hipErrorOutOfMemory; }
    if (to <= from) return hipSuccess;
    hipError_t e = hipMemcpyAsync(b->h_text.data(), buf + from, (size_t)(to - from), hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
  };
  const int64_t hi = HEAD + fresh;
  if (s->fallen) {
    BCHK(text_down(HEAD, hi));
    b->declined = 1;
    b->n_text = fresh;
    done_turn(s, &svdss_fastx_stream::next_seq, SVDSS_OK, "");
    run.turn = 2;
    run.lap(2);
    return SVDSS_OK;
  }
  const int64_t carry_len = (int64_t)s->carry.size();   // (<= cap: a longer one declined)
  const int64_t lo = HEAD - carry_len, base = lo & ~(int64_t)(FX_T - 1);
  const int64_t N = hi - lo;
  b->n_text = N;
  if (carry_len > 0) BCHK(hipMemcpyAsync(buf + lo, s->carry.data(), (size_t)carry_len, hipMemcpyHostToDevice, st));
  if (s->shape == 0 && N > 0) {
    uint8_t c0 = 0;
    BCHK(hipMemcpyAsync(&c0, buf + lo, 1, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    s->shape = c0 == '>' || c0 == '@' ? (int)c0 : -1;
  }
  int64_t L = 0, carry_at = 0, n_rec = 0, total_syms = 0;
  const int64_t n_tiles = N > 0 ? (hi - base + FX_T - 1) / FX_T : 0;
  bool declined = s->shape < 0;
  const bool parsed = N > 0 && !declined;
  if (parsed) {
    RCHK(b->tile_nl.ensure(sizeof(int32_t) * (size_t)(n_tiles + 1)));
    RCHK(b->tile_base.ensure(sizeof(int32_t) * (size_t)(n_tiles + 1)));
    unsigned long long h0[X_N] = {X_NONE, 0, X_NONE, 0, 0, 0, 0, 0};
    BCHK(hipMemcpyAsync(b->hdr.p, h0, sizeof h0, hipMemcpyHostToDevice, st));
    BCHK(hipMemsetAsync((int32_t*)b->tile_nl.p + n_tiles, 0, sizeof(int32_t), st));
    BCHK(hipEventRecord(b->ev[2], st));
    hipLaunchKernelGGL(fx_tile_kernel, dim3((unsigned)n_tiles), dim3(FX_TPB), 0, st, (const uint8_t*)buf, base, lo, hi, (int32_t*)b->tile_nl.p,
                       (unsigned long long*)b->hdr.p);
    BCHK(hipGetLastError());
    RCHK(run.scan((const int32_t*)b->tile_nl.p, (int32_t*)b->tile_base.p, n_tiles + 1));
    int32_t n_nl = 0;
    unsigned long long h1[X_N];
    BCHK(hipMemcpyAsync(&n_nl, (int32_t*)b->tile_base.p + n_tiles, sizeof n_nl, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(h1, b->hdr.p, sizeof h1, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    const bool open_line = h1[X_LASTNL] == 0;     // the text ends inside a line
    L = (int64_t)n_nl + (open_line ? 1 : 0);
    const int64_t Lc = is_last ? L : n_nl;
    for (FxBuf* q : {&b->ls, &b->hflag, &b->slen, &b->ridx, &b->spos}) RCHK(q->ensure(sizeof(int32_t) * (size_t)(L + 2)));
    int32_t* ls = (int32_t*)b->ls.p;
    hipLaunchKernelGGL(fx_lines_kernel, dim3((unsigned)n_tiles), dim3(FX_TPB), 0, st, (const uint8_t*)buf, base, lo, hi, (const int32_t*)b->tile_base.p, ls);
    BCHK(hipGetLastError());
    if (open_line) {   // (so that every line i is text[ls[i], ls[i + 1] - 1))
      b->sentinel = (int32_t)(N + 1);
      BCHK(hipMemcpyAsync(ls + L, &b->sentinel, sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    FxP P;
    P.text = buf + lo; P.ls = ls; P.L = (int32_t)L; P.Lc = (int32_t)Lc; P.N = (int32_t)N;
    P.fastq = s->shape == '@'; P.is_last = is_last ? 1 : 0;
    P.hflag = (int32_t*)b->hflag.p; P.slen = (int32_t*)b->slen.p; P.hdr = (unsigned long long*)b->hdr.p;
    hipLaunchKernelGGL(fx_classify_kernel, dim3(blocks_for(L + 1)), dim3(256), 0, st, P);
    BCHK(hipGetLastError());
    if (!P.fastq) {
      hipLaunchKernelGGL(fx_limit_kernel, dim3(blocks_for(L + 1)), dim3(256), 0, st, P);
      BCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(fx_mask_kernel, dim3(blocks_for(L + 1)), dim3(256), 0, st, P);
    BCHK(hipGetLastError());
    RCHK(run.scan(P.hflag, (int32_t*)b->ridx.p, L + 1));
    RCHK(run.scan(P.slen, (int32_t*)b->spos.p, L + 1));
    BCHK(hipEventRecord(b->ev[3], st));
    int32_t tot[2] = {0, 0};
    BCHK(hipMemcpyAsync(&tot[0], (int32_t*)b->ridx.p + L, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&tot[1], (int32_t*)b->spos.p + L, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(h1, b->hdr.p, sizeof h1, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    n_rec = tot[0]; total_syms = tot[1];
    carry_at = (int64_t)h1[X_CARRY];
    declined = h1[X_BADLINE] != X_NONE;
    // a record that does not end within the cap (at the end of the stream nothing is carried: a FASTQ's empty lines)
    if (!declined && !is_last && N - carry_at > s->cap) declined = true;
  }
  {
    hipError_t e = hipSuccess;
    if (declined) {
      e = text_down(lo + carry_at, hi);
      s->fallen = true;
      s->carry.clear();
    } else if (!is_last) {
      try { s->carry.resize((size_t)(N - carry_at)); } catch (...) { e = hipErrorOutOfMemory; }
      if (e == hipSuccess && N > carry_at) {
        e = hipMemcpyAsync(s->carry.data(), buf + lo + carry_at, (size_t)(N - carry_at), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
      }
    } else {
      s->carry.clear();
    }
    BCHK(e);
  }
  b->declined = declined ? 1 : 0;
  done_turn(s, &svdss_fastx_stream::next_seq, SVDSS_OK, "");
  run.turn = 2;
  run.lap(2);   // the turn

  // ---- the proved records: header line, offsets, name; the bases as nt6 at their output positions
  b->n_records = n_rec;
  try {
    b->h_name_off.assign((size_t)n_rec + 1, 0); b->h_seq_len.resize((size_t)n_rec); b->h_names.clear();
    b->h_counts.clear(); b->h_qs.clear(); b->h_len.clear(); b->h_off.clear(); b->h_reads.clear();
  } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
  if (n_rec > 0) {
    RCHK(b->hline.ensure(sizeof(int32_t) * (size_t)n_rec));
    RCHK(b->name_len.ensure(sizeof(int32_t) * (size_t)(n_rec + 1)));
    RCHK(b->name_off.ensure(sizeof(int32_t) * (size_t)(n_rec + 1)));
    RCHK(b->seq_len.ensure(sizeof(int32_t) * (size_t)n_rec));
    RCHK(b->off.ensure(sizeof(int64_t) * (size_t)(n_rec + 1)));
    RCHK(b->reads.ensure((size_t)total_syms + 4096));
    FxR R;
    R.text = buf + lo; R.ls = (const int32_t*)b->ls.p; R.hflag = (const int32_t*)b->hflag.p; R.ridx = (const int32_t*)b->ridx.p;
    R.spos = (const int32_t*)b->spos.p; R.L = (int32_t)L; R.n_rec = (int32_t)n_rec;
    R.hline = (int32_t*)b->hline.p; R.name_len = (int32_t*)b->name_len.p; R.off = (int64_t*)b->off.p;
    BCHK(hipEventRecord(b->ev[4], st));
    hipLaunchKernelGGL(fx_records_kernel, dim3(blocks_for(L + 1)), dim3(256), 0, st, R);
    BCHK(hipGetLastError());
    RCHK(run.scan(R.name_len, (int32_t*)b->name_off.p, n_rec + 1));
    BCHK(hipMemcpyAsync(b->h_name_off.data(), b->name_off.p, sizeof(int32_t) * (size_t)(n_rec + 1), hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    const int64_t name_bytes = b->h_name_off[(size_t)n_rec];
    RCHK(b->names.ensure((size_t)name_bytes + 16));
    hipLaunchKernelGGL(fx_names_kernel, dim3(blocks_for(n_rec)), dim3(256), 0, st, R, (const int32_t*)b->name_off.p, (char*)b->names.p, (int32_t*)b->seq_len.p);
    BCHK(hipGetLastError());
    if (total_syms > 0) {
      hipLaunchKernelGGL(fx_gather_kernel, dim3((unsigned)n_tiles), dim3(FX_TPB), 0, st, (const uint8_t*)buf, base, lo, hi, (const int32_t*)b->tile_base.p,
                         (const int32_t*)b->ls.p, (const int32_t*)b->slen.p, (const int32_t*)b->spos.p, (const unsigned long long*)b->hdr.p, (uint8_t*)b->reads.p);
      BCHK(hipGetLastError());
    }
    BCHK(hipEventRecord(b->ev[5], st));
    try {
      b->h_names.resize((size_t)name_bytes);
      if (b->parse_only) { b->h_off.resize((size_t)n_rec + 1); b->h_reads.resize((size_t)total_syms); }
    } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
    if (name_bytes > 0) BCHK(hipMemcpyAsync(b->h_names.data(), b->names.p, (size_t)name_bytes, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(b->h_seq_len.data(), b->seq_len.p, sizeof(int32_t) * (size_t)n_rec, hipMemcpyDeviceToHost, st));
    if (b->parse_only) {
      BCHK(hipMemcpyAsync(b->h_off.data(), b->off.p, sizeof(int64_t) * (size_t)(n_rec + 1), hipMemcpyDeviceToHost, st));
      if (total_syms > 0) BCHK(hipMemcpyAsync(b->h_reads.data(), b->reads.p, (size_t)total_syms, hipMemcpyDeviceToHost, st));
    }
    BCHK(hipStreamSynchronize(st));
  }
  if (parsed) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev[2], b->ev[3]) == hipSuccess) b->parse_ms += ms;
    if (n_rec > 0 && hipEventElapsedTime(&ms, b->ev[4], b->ev[5]) == hipSuccess) b->parse_ms += ms;
  }
  run.lap(3);   // records, names, bases
  if (b->parse_only && n_rec == 0) b->h_off.assign(1, 0);

  // ---- the search
  if (ix && n_rec > 0) {
    const int rc = svdss_sfs_search_batch_device(ix, (const uint8_t*)b->reads.p, (const int64_t*)b->off.p, n_rec, total_syms,
                                                 (flags & SVDSS_SFS_ASSEMBLE), (void*)st, &b->sfs);
    if (rc != SVDSS_OK) return run.fail(rc, std::string("search: ") + svdss_last_hip_error());
    run.lap(5);
    b->total_sfs = svdss_sfs_batch_total(b->sfs);
    try {
      b->h_counts.resize((size_t)n_rec); b->h_qs.resize((size_t)b->total_sfs); b->h_len.resize((size_t)b->total_sfs);
    } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
    void *d_counts = nullptr, *d_qs = nullptr, *d_len = nullptr;
    RCHK(svdss_sfs_batch_device_ptrs(b->sfs, &d_counts, &d_qs, &d_len, nullptr));
    BCHK(hipMemcpyAsync(b->h_counts.data(), d_counts, sizeof(int64_t) * (size_t)n_rec, hipMemcpyDeviceToHost, st));
    if (b->total_sfs > 0) {
      BCHK(hipMemcpyAsync(b->h_qs.data(), d_qs, sizeof(int32_t) * (size_t)b->total_sfs, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(b->h_len.data(), d_len, sizeof(int32_t) * (size_t)b->total_sfs, hipMemcpyDeviceToHost, st));
    }
    BCHK(hipStreamSynchronize(st));
    run.lap(6);   // results down
  }
  return SVDSS_OK;
}

extern "C" int svdss_fastx_batch_result(const svdss_fastx_batch_t* b, svdss_fastx_result_t* r) {
  if (!b || !r) return SVDSS_EINVAL;
  memset(r, 0, sizeof *r);
  r->n_records = b->n_records;
  r->name_off = b->h_name_off.data();
  r->names = b->h_names.data();
  r->seq_len = b->h_seq_len.data();
  r->counts = b->h_counts.data();
  r->qs = b->h_qs.data();
  r->len = b->h_len.data();
  r->total_sfs = b->total_sfs;
  r->reads = b->h_reads.data();
  r->offsets = b->h_off.data();
  r->declined = b->declined;
  r->n_text_bytes = b->n_text;
  r->text = b->h_text.data();
  r->text_bytes = (int64_t)b->h_text.size();
  r->inflate_kernel_ms = b->inflate_ms;
  r->parse_kernel_ms = b->parse_ms;
  for (int k = 0; k < 8; ++k) r->stage_ms[k] = b->stage_ms[k];
  return SVDSS_OK;
}
