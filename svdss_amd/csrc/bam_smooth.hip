// bam_smooth.hip -- `SVDSS smooth` on the device path (beside bam_device.hip: same front end, same batch objects).
//
// Stands where smoother.cpp's batch loop stands (:349-494 driver, :498-571 loader, :84-232 smooth_read, :50-82
// rebuild_bam_entry, :441-494 writer): BGZF blocks in, BGZF blocks out.  The inflated records never leave HBM: the front end
// of `search` (inflate, CRC32, record chain, the turn) lists them; a thread per record applies the filters of :509-537; a
// wavefront per kept record walks its CIGAR against the reference (fits? matches / mismatches, new length, new CIGAR
// length, "nothing interesting", where XF sits in the aux block); a thread per record decides XF (0 smoothed, 1 too many
// mismatches, 2 nothing interesting, 3 inconsistent) and the record's new size; a wavefront per record writes the new record
// behind the previous one; and the batch's bytes -- with the bytes the batch before it left over, see the output turn --
// are cut into BGZF blocks of 0xff00 bytes, deflated (csrc/deflate.hip), given their CRC32 / ISIZE and copied down.
// Output bytes = those of the host path (csrc/smooth_host.cpp with BgzfWriter + the GPU encoder): the same records in the
// same order, cut at the same stream offsets, through the same encoder.
//
// The output turn: a BGZF block holds 0xff00 bytes of the output STREAM, whatever batch they come from, so a batch has to
// know how many bytes the batches before it leave over.  Batches take a second turn in file order (svdss_bam_stream::
// next_out): batch k receives the unfinished block of batch k - 1 (at most 0xff00 - 1 bytes, through host memory like the
// record carry; for batch 0: the BAM header of the output), puts it in front of its own records, hands the bytes behind its
// last full block on, and only then deflates -- so the deflate kernels of different batches overlap.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "bam_device_internal.h"
#include "bam_index_writer.h"
#include "deflate_dev.h"
#include "ref_dev.h"

namespace {

enum { E_NCIG = 4 };   // more than 65535 CIGAR operations after smoothing (further bits of hdr[H_ERR])
constexpr int kSmMinIndel = 20;          // config.hpp:95
constexpr int64_t kBgzfBlock = 0xff00;

struct SmMetaP {
  const uint8_t* buf;
  const uint32_t* lists; int64_t list_cap;
  const int32_t* seg_cnt; const int32_t* seg_base; const uint32_t* pre;
  int32_t n_seg, min_mapq, n_ref;
  int64_t n_rec;
  const int32_t* tidmap;
  uint32_t* rpos;
  int64_t* f_keep;       // n_rec + 1
  int64_t* hdr;
};

// a thread per record: the filters of smoother.cpp:509-537 (= eligible() of smooth_host.cpp)
__global__ void __launch_bounds__(64) smooth_meta_kernel(SmMetaP M) {
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
    const uint32_t l_name = w3 & 0xffu, mapq = (w3 >> 8) & 0xffu, n_cig = w4 & 0xffffu, flag = w4 >> 16;
    const int64_t head = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)(l_seq < 0 ? 0 : l_seq) + 1) / 2 + (l_seq < 0 ? 0 : l_seq);
    bool keep = false;
    if (l_seq < 0 || head > (int64_t)bs) atomicOr((unsigned long long*)&M.hdr[H_ERR], (unsigned long long)E_CORRUPT);
    else {
      keep = !(flag & (4u | 2048u | 256u)) && (int32_t)mapq >= M.min_mapq && l_seq >= 2;
      if (keep && tid < 0) atomicOr((unsigned long long*)&M.hdr[H_ERR], (unsigned long long)E_TID);
      keep = keep && tid >= 0 && tid < M.n_ref && M.tidmap[tid] >= 0;
    }
    M.rpos[gi] = (uint32_t)p;
    M.f_keep[gi] = keep ? 1 : 0;
  }
  if (s == 0 && threadIdx.x == 0) M.f_keep[M.n_rec] = 0;
}

// svdss_bam_smooth_set_store: a thread per record of the batch, kept or dropped by the smoothing (rpos lists them all, and
// smooth_meta_kernel has checked their sizes) -- does `SVDSS call` keep it, and how long is its slim form?  Rows of n_rec + 1.
__global__ void __launch_bounds__(256) smooth_store_flag_kernel(const uint8_t* __restrict__ buf, const uint32_t* __restrict__ rpos, int64_t n_rec,
                                                                int32_t min_mapq, int64_t* f_keep, int64_t* f_kbytes, int64_t* hpv) {
  const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi > n_rec) return;
  int64_t keep = 0, kbytes = 0, hp = kNoHp;
  if (gi < n_rec) {
    const int64_t p = rpos[gi];
    const uint32_t bs = ld32(buf, p);
    const uint32_t w3 = ld32(buf, p + 12), w4 = ld32(buf, p + 16);
    const int32_t l_seq = (int32_t)ld32(buf, p + 20);
    const uint32_t l_name = w3 & 0xffu, mapq = (w3 >> 8) & 0xffu, n_cig = w4 & 0xffffu, flag = w4 >> 16;
    const int64_t head = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)l_seq + 1) / 2 + l_seq;
    if (call_keeps(flag, mapq, min_mapq)) { keep = 1; kbytes = slim_measure(buf, p, bs, head, l_seq, hp); }
  }
  f_keep[gi] = keep; f_kbytes[gi] = kbytes; hpv[gi] = hp;
}

struct SmWalkP {
  const uint8_t* buf;
  const uint32_t* rpos; const int64_t* f_keep; const int64_t* s_keep;
  int64_t n_rec;
  const uint8_t* ref; const int64_t* ref_off; const int32_t* tidmap;
  // per kept record
  uint32_t* kpos;
  int64_t* nmx;          // matches, mismatches
  int32_t* nlen;         // bases of the smoothed read
  int32_t* ncig;         // CIGAR operations of the smoothed read
  uint8_t* kflags;       // bit 0: the CIGAR fits read and contig, bit 1: nothing interesting
  int32_t* xf_at;        // where the value byte(s) of an integer XF sit (offset from the record's block_size field); -1: no XF,
  int32_t* xf_sz;        // append one; -2: aux block the host's walk gives up on, left alone.  xf_sz: bytes of the value
};

// the CIGAR of a record, 64 operations at a time: one load per lane, operations handed round with shuffles
struct CigIter {
  const uint8_t* buf; int64_t at; int n, done, have; uint32_t mine;
  __device__ CigIter(const uint8_t* b, int64_t cg, int n_cig) : buf(b), at(cg), n(n_cig), done(0), have(0), mine(0) {}
  __device__ bool next(uint32_t& w) {
    if (done >= n) return false;
    const int k = done & 63;
    if (k == 0) {
      const int lane = threadIdx.x & 63;
      mine = done + lane < n ? ld32(buf, at + 4 * (int64_t)(done + lane)) : 0u;
    }
    w = (uint32_t)__shfl((int)mine, k, 64);
    ++done;
    return true;
  }
};

__device__ __forceinline__ char sm4_base(const uint8_t* buf, int64_t sq, int64_t i) {
  const uint8_t b = buf[sq + (i >> 1)];
  return "=ACMGRSVTWYHKDBN"[(i & 1) ? (b & 15) : (b >> 4)];
}
__device__ __forceinline__ uint32_t sm_code_of(char c) {   // the table write_record (smooth_host.cpp) packs with
  switch (c) {
    case '=': return 0; case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'M': case 'm': return 3;
    case 'G': case 'g': return 4; case 'R': case 'r': return 5; case 'S': case 's': return 6; case 'V': case 'v': return 7;
    case 'T': case 't': return 8; case 'W': case 'w': return 9; case 'Y': case 'y': return 10; case 'H': case 'h': return 11;
    case 'K': case 'k': return 12; case 'D': case 'd': return 13; case 'B': case 'b': return 14; default: return 15;
  }
}

// a wavefront per record: what smooth_read (smoother.cpp:84-232) learns about it without writing anything
__global__ void __launch_bounds__(64) smooth_walk_kernel(SmWalkP A) {
  const int64_t gi = blockIdx.x;
  if (!A.f_keep[gi]) return;
  const int lane = threadIdx.x;
  const int64_t k = A.s_keep[gi];
  const int64_t p = A.rpos[gi];
  const uint32_t bs = ld32(A.buf, p);
  const int32_t tid = (int32_t)ld32(A.buf, p + 4), pos = (int32_t)ld32(A.buf, p + 8);
  const uint32_t w3 = ld32(A.buf, p + 12), w4 = ld32(A.buf, p + 16);
  const int64_t l_seq = (int32_t)ld32(A.buf, p + 20);
  const int64_t l_name = w3 & 0xffu;
  const int n_cig = (int)(w4 & 0xffffu);
  const int64_t cg = p + 36 + l_name, sq = cg + 4 * (int64_t)n_cig, ax = sq + (l_seq + 1) / 2 + l_seq, rec_end = p + 4 + (int64_t)bs;
  const int32_t ct = A.tidmap[tid];
  const int64_t ref_len = A.ref_off[ct + 1] - A.ref_off[ct];
  const uint8_t* cseq = A.ref + A.ref_off[ct];
  // cigar_fits (smooth_host.cpp): the alignment stays inside its contig and the CIGAR adds up to the read
  int64_t rl = 0, qlen = 0;
  {
    CigIter it(A.buf, cg, n_cig);
    uint32_t w;
    while (it.next(w)) {
      const uint32_t l = w >> 4, op = w & 0xf;
      if (op == 0 || op == 7 || op == 8) { rl += l; qlen += l; }
      else if (op == 1 || op == 4) qlen += l;
      else if (op == 2) rl += l;
      else break;
    }
  }
  const bool fits = pos >= 0 && (int64_t)pos + rl <= ref_len && qlen == l_seq;
  unsigned long long nm = 0, nx = 0;
  int64_t no = 0;
  int n_nc = 0;
  bool ignore = true;
  if (fits) {
    int64_t ref_off = pos, q_off = 0;
    bool last_is_m = false;
    CigIter it(A.buf, cg, n_cig);
    uint32_t w;
    while (it.next(w)) {
      const uint32_t l = w >> 4, op = w & 0xf;
      if (op == 0 || op == 7 || op == 8) {
        for (uint32_t j = lane; j < l; j += 64) {
          if ((char)cseq[ref_off + j] == sm4_base(A.buf, sq, q_off + j)) ++nm; else ++nx;
        }
        no += l; ref_off += l; q_off += l;
        if (!(n_nc && last_is_m)) ++n_nc;
        last_is_m = true;
      } else if (op == 1) {
        if ((int)l > kSmMinIndel) { ignore = false; no += l; ++n_nc; last_is_m = false; }
        q_off += l;
      } else if (op == 2) {
        if ((int)l <= kSmMinIndel) no += l;
        else { ignore = false; ++n_nc; last_is_m = false; }
        ref_off += l;
      } else if (op == 4) {
        ignore = false;
        no += l; q_off += l;
        ++n_nc; last_is_m = false;
      } else break;
    }
    for (int d = 32; d >= 1; d >>= 1) { nm += __shfl_xor(nm, d, 64); nx += __shfl_xor(nx, d, 64); }
  }
  // set_xf (smooth_host.cpp; bam_aux_update_int): an integer XF is overwritten, else XF:C is appended; an aux block the
  // walk gives up on (bam_aux_walk.h) is left alone.  (ax <= rec_end here: smooth_meta_kernel keeps no record whose core,
  // name, CIGAR, bases and qualities do not fit in its block_size -- it raises E_CORRUPT, the batch fails as the host
  // reader's "corrupt record" does -- so an empty aux block is [ax, ax): absent, XF:C appended)
  int32_t xat = -1, xsz = 0;
  {
    const int64_t at = svdss_aux_find_int(A.buf + ax, A.buf + rec_end, 'X', 'F', xsz);
    if (at == SVDSS_AUX_BAD) xat = -2;
    else if (at >= 0) xat = (int32_t)(ax + at - p);
  }
  if (lane == 0) {
    A.kpos[k] = (uint32_t)p;
    A.nmx[2 * k] = (int64_t)nm; A.nmx[2 * k + 1] = (int64_t)nx;
    A.nlen[k] = (int32_t)no;
    A.ncig[k] = n_nc;
    A.kflags[k] = (uint8_t)((fits ? 1 : 0) | (ignore ? 2 : 0));
    A.xf_at[k] = xat; A.xf_sz[k] = xsz;
  }
}

struct SmSizeP {
  const uint8_t* buf;
  int64_t n_keep;
  const uint32_t* kpos; const int64_t* nmx; const int32_t* nlen; const int32_t* ncig; const uint8_t* kflags; const int32_t* xf_at;
  double acc;
  uint8_t* xfv;          // the XF value of the record
  int64_t* osize;        // n_keep + 1: bytes of the output record (block_size field included)
  int64_t* ssize;        // n_keep + 1: bytes of scratch (one per base of a smoothed read)
  int64_t* hdr;
};

__global__ void __launch_bounds__(256) smooth_size_kernel(SmSizeP S) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > S.n_keep) return;
  if (k == S.n_keep) { S.osize[k] = 0; S.ssize[k] = 0; return; }
  const int64_t p = S.kpos[k];
  const uint32_t bs = ld32(S.buf, p);
  const uint32_t w3 = ld32(S.buf, p + 12), w4 = ld32(S.buf, p + 16);
  const int64_t l_seq = (int32_t)ld32(S.buf, p + 20), l_name = w3 & 0xffu, n_cig = w4 & 0xffffu;
  const int64_t aux_len = (int64_t)bs - (32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq);
  const uint8_t fl = S.kflags[k];
  const double nm = (double)S.nmx[2 * k], nx = (double)S.nmx[2 * k + 1];
  int v;
  if (!(fl & 1)) v = 3;
  else if (nx / nm > S.acc) v = 1;
  else if (fl & 2) v = 2;
  else v = 0;
  const int64_t extra = S.xf_at[k] == -1 ? 4 : 0;
  int64_t sz, sc = 0;
  if (v != 0) sz = 4 + (int64_t)bs + extra;
  else {
    const int64_t nl = S.nlen[k], nc = S.ncig[k];
    if (nc > 65535) atomicOr((unsigned long long*)&S.hdr[H_ERR], (unsigned long long)E_NCIG);
    sz = 4 + 32 + l_name + 4 * nc + (nl + 1) / 2 + nl + aux_len + extra;
    sc = nl;
  }
  S.xfv[k] = (uint8_t)v;
  S.osize[k] = sz;
  S.ssize[k] = sc;
}

struct SmWriteP {
  const uint8_t* buf;
  int64_t n_keep;
  const uint32_t* kpos; const int32_t* nlen; const int32_t* ncig; const int32_t* xf_at; const int32_t* xf_sz; const uint8_t* xfv;
  const int64_t* ooff; const int64_t* soff;
  const uint8_t* ref; const int64_t* ref_off; const int32_t* tidmap;
  uint8_t* out; uint8_t* scratch;
};

__device__ __forceinline__ void sm_st32(uint8_t* o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24); }

// a wavefront per kept record: the record as smooth_read + rebuild_bam_entry (smoother.cpp:50-82) leave it
__global__ void __launch_bounds__(64) smooth_write_kernel(SmWriteP A) {
  const int64_t k = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t p = A.kpos[k];
  const uint8_t* src = A.buf + p;
  uint8_t* o = A.out + A.ooff[k];
  const uint32_t bs = ld32(A.buf, p);
  const int32_t tid = (int32_t)ld32(A.buf, p + 4), pos = (int32_t)ld32(A.buf, p + 8);
  const uint32_t w3 = ld32(A.buf, p + 12), w4 = ld32(A.buf, p + 16);
  const int64_t l_seq = (int32_t)ld32(A.buf, p + 20), l_name = w3 & 0xffu;
  const int n_cig = (int)(w4 & 0xffffu);
  const int64_t cg = 36 + l_name, sq = cg + 4 * (int64_t)n_cig, ql = sq + (l_seq + 1) / 2, ax = ql + l_seq, rec_len = 4 + (int64_t)bs;
  const int64_t aux_len = rec_len - ax;
  const int v = A.xfv[k];
  const int32_t xat = A.xf_at[k], xsz = A.xf_sz[k];
  int64_t o_ax;          // where the aux block starts in the output record
  if (v != 0) {
    // the record as it is (nine records in ten of a HiFi sample: "nothing interesting"): a dword per lane and step -- bytes up
    // to the output's dword boundary, dwords (the input read unaligned: two aligned loads and an alignbyte), bytes
    int64_t head = (int64_t)((4u - (uint32_t)((uintptr_t)o & 3u)) & 3u);
    if (head > rec_len) head = rec_len;
    if (lane < head) o[lane] = src[lane];
    const int64_t nw = (rec_len - head) >> 2;
    uint32_t* const d32 = (uint32_t*)(o + head);
    for (int64_t i = lane; i < nw; i += 64) d32[i] = ld32(A.buf, p + head + 4 * i);
    const int64_t done = head + 4 * nw;
    if (lane < rec_len - done) o[done + lane] = src[done + lane];
    o_ax = ax;
  } else {
    const int64_t nl = A.nlen[k];
    const int nc = A.ncig[k];
    const int64_t o_cg = 36 + l_name, o_sq = o_cg + 4 * (int64_t)nc, o_ql = o_sq + (nl + 1) / 2;
    o_ax = o_ql + nl;
    // core (the fields that change are written behind the copy) and name
    for (int64_t i = lane; i < 36 + l_name; i += 64) o[i] = src[i];
    const int32_t ct = A.tidmap[tid];
    const uint8_t* cseq = A.ref + A.ref_off[ct];
    uint8_t* ns = A.scratch + A.soff[k];       // 4-bit codes of the new read, one per byte
    uint8_t* nq = o + o_ql;
    int64_t ref_off = pos, q_off = 0, no = 0;
    uint32_t m_diff = 0, last_word = 0;
    int n_nc = 0;
    CigIter it(A.buf, p + cg, n_cig);
    uint32_t w;
    while (it.next(w)) {
      const uint32_t l = w >> 4, op = w & 0xf;
      if (op == 0 || op == 7 || op == 8) {
        for (uint32_t j = lane; j < l; j += 64) {
          ns[no + j] = (uint8_t)sm_code_of((char)cseq[ref_off + j]);
          nq[no + j] = q_off + j < l_seq ? src[ql + q_off + j] : (uint8_t)255;
        }
        no += l; ref_off += l; q_off += l;
        if (n_nc && (last_word & 0xf) == 0) last_word += (l + m_diff) << 4;
        else { last_word = ((l + m_diff) << 4) | 0; ++n_nc; }
        if (lane == 0) sm_st32(o + o_cg + 4 * (int64_t)(n_nc - 1), last_word);
        m_diff = 0;
      } else if (op == 1) {
        if ((int)l > kSmMinIndel) {
          for (uint32_t j = lane; j < l; j += 64) {
            ns[no + j] = (uint8_t)sm_code_of(sm4_base(A.buf, p + sq, q_off + j));
            nq[no + j] = q_off + j < l_seq ? src[ql + q_off + j] : (uint8_t)255;
          }
          no += l;
          last_word = w; ++n_nc;
          if (lane == 0) sm_st32(o + o_cg + 4 * (int64_t)(n_nc - 1), w);
        }
        q_off += l;
      } else if (op == 2) {
        if ((int)l <= kSmMinIndel) {
          for (uint32_t j = lane; j < l; j += 64) {
            ns[no + j] = (uint8_t)sm_code_of((char)cseq[ref_off + j]);
            nq[no + j] = q_off + j < l_seq ? src[ql + q_off + j] : (uint8_t)255;     // qualities of the NEXT read bases (smoother.cpp:164-166)
          }
          no += l;
          m_diff += l;
        } else {
          last_word = w; ++n_nc;
          if (lane == 0) sm_st32(o + o_cg + 4 * (int64_t)(n_nc - 1), w);
        }
        ref_off += l;
      } else if (op == 4) {
        for (uint32_t j = lane; j < l; j += 64) {
          ns[no + j] = (uint8_t)sm_code_of(sm4_base(A.buf, p + sq, q_off + j));
          nq[no + j] = q_off + j < l_seq ? src[ql + q_off + j] : (uint8_t)255;
        }
        no += l; q_off += l;
        last_word = w; ++n_nc;
        if (lane == 0) sm_st32(o + o_cg + 4 * (int64_t)(n_nc - 1), w);
      } else break;
    }
    __syncthreads();   // the codes are complete
    for (int64_t b = lane; b < (nl + 1) / 2; b += 64) {
      const uint32_t hi = ns[2 * b], lo = 2 * b + 1 < nl ? (uint32_t)ns[2 * b + 1] : 0u;
      o[o_sq + b] = (uint8_t)((hi << 4) | lo);
    }
    for (int64_t i = lane; i < aux_len; i += 64) o[o_ax + i] = src[ax + i];
    __syncthreads();
    if (lane == 0) {
      const uint32_t nbs = (uint32_t)(o_ax + aux_len - 4);
      sm_st32(o, nbs);
      o[16] = (uint8_t)(nc & 0xff); o[17] = (uint8_t)(nc >> 8);       // n_cigar_op
      sm_st32(o + 20, (uint32_t)nl);                                  // l_seq
    }
  }
  __syncthreads();
  // XF
  if (xat >= 0) {
    uint8_t* x = o + o_ax + (xat - ax);
    if (lane < xsz) x[lane] = lane == 0 ? (uint8_t)v : (uint8_t)0;
  } else if (xat == -1) {
    if (lane == 0) {
      uint8_t* x = o + o_ax + aux_len;
      x[0] = 'X'; x[1] = 'F'; x[2] = 'C'; x[3] = (uint8_t)v;
      const uint32_t nbs = (uint32_t)(o_ax + aux_len + 4 - 4);
      sm_st32(o, nbs);
    }
  }
}

// ---- `smooth --write-index` (bam_index_writer.h): the batch's index fragments, reduced before anything comes down
struct SmIxP {
  const uint8_t* out;        // the batch's rebuilt records (sm_out + room); record k at ooff[k]
  const int64_t* ooff;       // n_keep + 1
  int64_t n_keep;
  int64_t tail_in, in_len, n_blk;   // the output turn: bytes in front of the records, bytes in full members, members
  const int64_t* d_off;      // n_blk + 1 compressed offsets of the members (nullptr: n_blk == 0)
  int32_t min_shift, depth;
  // per kept record (n_keep + 1)
  int32_t* tid; uint32_t* bin; int64_t* beg; int64_t* end; uint64_t* vb; uint64_t* ve;
  uint64_t* key;             // (tid << 32) | (last window + 1): a running maximum of it is the last window reached so far
  const uint64_t* kmax;      // ... exclusive running maximum
  int64_t* head; int64_t* own;           // starts a chunk; windows it reaches into first
  const int64_t* s_head; const int64_t* s_own;
  svdss_bam_index_chunk_t* chunks; svdss_bam_index_window_t* windows;
  unsigned long long* err;   // bit 0: records out of coordinate order
};

// the virtual offset (relative to the batch's first member) of position q of the batch's stream: the member that holds the
// byte; behind the batch's full members (the carried block, which is the next batch's first member, or the end of the
// output) the offset right after them
__device__ __forceinline__ uint64_t sm_ix_voff(const SmIxP& P, int64_t q) {
  if (q < P.in_len) return ((uint64_t)P.d_off[q / kBgzfBlock] << 16) | (uint64_t)(q % kBgzfBlock);
  const int64_t after = P.n_blk > 0 ? P.d_off[P.n_blk] : 0;
  return ((uint64_t)after << 16) | (uint64_t)(q - P.in_len);
}

__device__ __forceinline__ void sm_ix_core(const SmIxP& P, int64_t k, int32_t& tid, int32_t& pos, int64_t& span) {
  const int64_t r = P.ooff[k];
  tid = (int32_t)ld32(P.out, r + 4);
  pos = (int32_t)ld32(P.out, r + 8);
  const int64_t l_name = ld32(P.out, r + 12) & 0xffu;
  const int n_cig = (int)(ld32(P.out, r + 16) & 0xffffu);
  span = 0;
  for (int j = 0; j < n_cig; ++j) {
    const uint32_t c = ld32(P.out, r + 36 + l_name + 4 * (int64_t)j);
    if (ix_ref_op(c & 0xfu)) span += c >> 4;
  }
}

// a thread per kept record: tid, [beg, end) (the span of the CIGAR as written), bin, virtual offsets of start and end
__global__ void __launch_bounds__(256) sm_ix_rec_kernel(SmIxP P) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= P.n_keep) return;
  int32_t tid, pos;
  int64_t span, beg, end;
  sm_ix_core(P, k, tid, pos, span);
  ix_extent(pos, span, P.min_shift, P.depth, beg, end);
  P.tid[k] = tid; P.beg[k] = beg; P.end[k] = end;
  P.bin[k] = ix_reg2bin(beg, end, P.min_shift, P.depth);
  P.vb[k] = sm_ix_voff(P, P.tail_in + P.ooff[k]);
  P.ve[k] = sm_ix_voff(P, P.tail_in + P.ooff[k + 1]);
  P.key[k] = ((uint64_t)(uint32_t)tid << 32) | (uint64_t)(((end - 1) >> P.min_shift) + 1);
  if (k > 0) {
    const int64_t r = P.ooff[k - 1];
    const int32_t ptid = (int32_t)ld32(P.out, r + 4);
    int64_t pbeg, pend;
    ix_extent((int32_t)ld32(P.out, r + 8), 1, P.min_shift, P.depth, pbeg, pend);
    if (tid < ptid || (tid == ptid && beg < pbeg)) atomicOr(P.err, 1ull);
  }
}

// a thread per kept record (+ the scans' total): does it start a chunk, which windows does it reach into first
__global__ void __launch_bounds__(256) sm_ix_own_kernel(SmIxP P) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > P.n_keep) return;
  if (k == P.n_keep) { P.head[k] = 0; P.own[k] = 0; return; }
  const uint64_t m = P.kmax[k];
  const int32_t tid = P.tid[k];
  const int64_t seen = (m >> 32) == (uint64_t)(uint32_t)tid ? (int64_t)(m & 0xffffffffu) - 1 : -1;   // last window reached before
  const int64_t w0 = P.beg[k] >> P.min_shift, w1 = (P.end[k] - 1) >> P.min_shift;
  const int64_t first = w0 > seen + 1 ? w0 : seen + 1;
  P.own[k] = w1 >= first ? w1 - first + 1 : 0;
  P.head[k] = (k == 0 || tid != P.tid[k - 1] || P.bin[k] != P.bin[k - 1]) ? 1 : 0;
}

// a thread per kept record: its chunk's start / end (the record count by two atomics on a zeroed field) and its windows
__global__ void __launch_bounds__(256) sm_ix_emit_kernel(SmIxP P) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= P.n_keep) return;
  const int64_t c = P.s_head[k] + P.head[k] - 1;
  svdss_bam_index_chunk_t* ch = P.chunks + c;
  if (P.head[k]) {
    ch->tid = P.tid[k]; ch->bin = P.bin[k]; ch->v_beg = P.vb[k];
    atomicAdd((unsigned long long*)&ch->n_rec, (unsigned long long)(-k));
  }
  if (k + 1 == P.n_keep || P.head[k + 1]) {
    ch->v_end = P.ve[k];
    atomicAdd((unsigned long long*)&ch->n_rec, (unsigned long long)(k + 1));
  }
  const int64_t n = P.own[k];
  if (n > 0) {
    const int64_t w1 = (P.end[k] - 1) >> P.min_shift;
    svdss_bam_index_window_t* w = P.windows + P.s_own[k];
    for (int64_t j = 0; j < n; ++j) { w[j].tid = P.tid[k]; w[j].window = (int32_t)(w1 - n + 1 + j); w[j].v_beg = P.vb[k]; }
  }
}

// ---- `smooth --index --sfs`: what `SVDSS search` would read from the smoothed BAM, taken from the rebuilt records while
// they are in HBM (the fields, filters and tags of bam_device.hip's meta_kernel / scatter_kernel / unpack_kernel, on the
// OUTPUT records: names, HP and XF as search's aux walk finds them, l_seq as rebuilt)
struct SmSfsP {
  const uint8_t* out;        // the batch's rebuilt records (sm_out + room); record k at ooff[k]
  const int64_t* ooff;       // n_keep + 1
  int64_t n_keep;
  int32_t putative;
  int64_t *f_pass, *f_srch, *f_name, *f_sym, *f_short;   // n_keep + 1 each, consecutive rows: inputs of the scans
  const int64_t *s_pass, *s_srch, *s_name, *s_sym;       // their exclusive sums (the last entry of a row: its total)
  int32_t* hp;               // n_keep
  // host-bound block, per read of the sequence ("slot": kept, l_seq >= 100)
  int32_t* o_name_off;       // slots + 1
  char* o_names;
  int32_t* o_hp;
  int32_t* o_sidx;           // index among the searched reads, -1: keeps its place but is not searched (XF != 0, putative)
  // per searched read
  int64_t* sym_off;          // searched + 1: where its symbols go, from the destination's start (sym_base: the park group's fill)
  int64_t sym_base;
  int64_t* seq_src;          // where its packed bases sit in `out`
};

__device__ __forceinline__ void sm_sfs_fields(const SmSfsP& P, int64_t k, int64_t& r, uint32_t& bs, uint32_t& l_name, uint32_t& n_cig, uint32_t& flag, int32_t& l_seq) {
  r = P.ooff[k];
  bs = ld32(P.out, r);
  const uint32_t w3 = ld32(P.out, r + 12), w4 = ld32(P.out, r + 16);
  l_seq = (int32_t)ld32(P.out, r + 20);
  l_name = w3 & 0xffu; n_cig = w4 & 0xffffu; flag = w4 >> 16;
}

// a thread per kept record: in the sequence (ping_pong.cpp:66-75)?  searched (:196-203)?  name bytes, symbols, HP
__global__ void __launch_bounds__(256) sm_sfs_flag_kernel(SmSfsP P) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > P.n_keep) return;
  if (k == P.n_keep) { P.f_pass[k] = 0; P.f_srch[k] = 0; P.f_name[k] = 0; P.f_sym[k] = 0; P.f_short[k] = 0; return; }
  int64_t r; uint32_t bs, l_name, n_cig, flag; int32_t l_seq;
  sm_sfs_fields(P, k, r, bs, l_name, n_cig, flag, l_seq);
  const int64_t head = 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)l_seq + 1) / 2 + l_seq;
  bool keep = !(flag & (4u | 2048u | 256u)) && l_seq >= 0 && head <= (int64_t)bs;
  const bool is_short = keep && l_seq < 100;
  keep = keep && !is_short;
  bool srch = false;
  int64_t hp = 0;
  if (keep) {
    const uint8_t* aux = P.out + r + 4 + head;
    const uint8_t* end = P.out + r + 4 + (int64_t)bs;
    int64_t xf = 0;
    (void)aux_int(aux, end, 'X', 'F', xf);
    (void)aux_int(aux, end, 'H', 'P', hp);
    srch = !(P.putative && xf != 0);
  }
  P.f_pass[k] = keep ? 1 : 0;
  P.f_srch[k] = srch ? 1 : 0;
  P.f_name[k] = keep ? (int64_t)(l_name ? l_name - 1 : 0) : 0;
  P.f_sym[k] = srch ? (int64_t)l_seq : 0;
  P.f_short[k] = is_short ? 1 : 0;
  P.hp[k] = (int32_t)hp;
}

// a thread per kept record (+ the totals' entry): the host-bound block and where the searched reads' symbols go
__global__ void __launch_bounds__(256) sm_sfs_scatter_kernel(SmSfsP P) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > P.n_keep) return;
  if (k == P.n_keep) {
    P.o_name_off[P.s_pass[k]] = (int32_t)P.s_name[k];
    P.sym_off[P.s_srch[k]] = P.sym_base + P.s_sym[k];
    return;
  }
  if (!P.f_pass[k]) return;
  int64_t r; uint32_t bs, l_name, n_cig, flag; int32_t l_seq;
  sm_sfs_fields(P, k, r, bs, l_name, n_cig, flag, l_seq);
  const int64_t slot = P.s_pass[k];
  P.o_name_off[slot] = (int32_t)P.s_name[k];
  P.o_hp[slot] = P.hp[k];
  const uint8_t* nm = P.out + r + 36;
  char* dst = P.o_names + P.s_name[k];
  for (uint32_t i = 0; i + 1 < l_name; ++i) dst[i] = (char)nm[i];
  if (P.f_srch[k]) {
    const int64_t j = P.s_srch[k];
    P.o_sidx[slot] = (int32_t)j;
    P.sym_off[j] = P.sym_base + P.s_sym[k];
    P.seq_src[j] = r + 36 + (int64_t)l_name + 4 * (int64_t)n_cig;
  } else P.o_sidx[slot] = -1;
}

// a workgroup per searched read: its packed bases -> nt6 at its place in the park's arena or the batch's buffer, a lane per
// 16 aligned output bytes (nt6_chunk16: dword loads of the packed bases, one 16-byte store)
__global__ void __launch_bounds__(256) sm_sfs_nt6_kernel(const uint8_t* __restrict__ recs, const int64_t* __restrict__ seq_src,
                                                         const int64_t* __restrict__ sym_off, uint8_t* out) {
  const int64_t j = blockIdx.x;
  const int64_t s = sym_off[j], e = sym_off[j + 1];
  const int64_t src = seq_src[j];
  for (int64_t c = (s >> 4) + threadIdx.x; (c << 4) < e; c += 256) nt6_chunk16(recs, src, s, e, c << 4, out);
}

struct FootP { const uint8_t* in; int64_t in_bytes; int32_t block_bytes; uint8_t* members; int64_t stride; const int32_t* len; };

// a wavefront per BGZF block of the output: CRC32 of its bytes and their number into the member's last 8 bytes
__global__ void __launch_bounds__(64) bgzf_footer_kernel(FootP F) {
  __shared__ uint32_t T[5][256];
  const int lane = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) T[k][lane + 64 * i] = g_crc_tab[k][lane + 64 * i];
  const uint32_t weight = g_crc_tab[5][lane];
  __syncthreads();
  const int64_t b = blockIdx.x;
  const int64_t start = b * (int64_t)F.block_bytes;
  const int n = (int)(F.in_bytes - start < F.block_bytes ? F.in_bytes - start : F.block_bytes);
  const uint8_t* p = F.in + start;
  const int J = n >> 8;
  uint32_t state = 0xFFFFFFFFu;
  if (J > 0) {
    uint32_t a = 0;
    for (int j = 0; j < J; ++j) {
      uint32_t w;
      __builtin_memcpy(&w, p + (int64_t)(j * 64 + lane) * 4, 4);
      if (j == 0 && lane == 0) w ^= 0xFFFFFFFFu;
      a = T[1][a & 0xff] ^ T[2][(a >> 8) & 0xff] ^ T[3][(a >> 16) & 0xff] ^ T[4][a >> 24] ^ w;
    }
    uint32_t c = gf_mul(a, weight);
    for (int d = 32; d >= 1; d >>= 1) c ^= (uint32_t)__shfl_xor((int)c, d, 64);
    state = c;
  }
  if (lane == 0) {
    for (int i = J << 8; i < n; ++i) state = T[0][(state ^ p[i]) & 0xff] ^ (state >> 8);
    uint8_t* f = F.members + b * F.stride + F.len[b] - 8;
    sm_st32(f, ~state);
    sm_st32(f + 4, (uint32_t)n);
  }
}

}  // namespace

struct svdss_bam_smooth {
  int device = -1;
  int32_t min_mapq = 0, n_ref = 0;
  int32_t ix_shift = 0, ix_depth = 0;   // svdss_bam_smooth_set_index (0: no index fragments)
  int32_t deflate_mode = SVDSS_DEFLATE_RUNS;   // svdss_bam_smooth_set_deflate
  int32_t search_flags = -1;            // svdss_bam_smooth_set_search (-1: the reads are not exported for a search)
  svdss_bam_park* park = nullptr;       // ... where they wait for the index (nullptr: in the batch object)
  bool write_bam = true;                // svdss_bam_smooth_set_output (false: no BGZF members)
  svdss_bam_store* store = nullptr;     // svdss_bam_smooth_set_store (nullptr: nothing is kept for `call`)
  int32_t store_min_mapq = 0;           // ... `call`'s own --min-mapq
  SvdssRefView ref;
  int32_t* d_tidmap = nullptr;
};

extern "C" int svdss_bam_smooth_create(const svdss_ref_t* ref, const int32_t* tid_map, int32_t n_ref, int32_t min_mapq,
                                       svdss_bam_smooth_t** out) {
  if (!ref || !out || n_ref < 0 || (n_ref > 0 && !tid_map)) return SVDSS_EINVAL;
  const SvdssRefView v = svdss_ref_view(ref);
  for (int32_t i = 0; i < n_ref; ++i)
    if (tid_map[i] < -1 || tid_map[i] >= v.n_chrom) return SVDSS_EINVAL;
  HIPCHK(hipSetDevice(v.device));
  svdss_bam_smooth* s = new (std::nothrow) svdss_bam_smooth();
  if (!s) return SVDSS_ENOMEM;
  s->device = v.device; s->min_mapq = min_mapq; s->n_ref = n_ref; s->ref = v;
  hipError_t e = hipMalloc((void**)&s->d_tidmap, sizeof(int32_t) * (size_t)(n_ref + 1));
  if (e == hipSuccess && n_ref > 0) e = hipMemcpy(s->d_tidmap, tid_map, sizeof(int32_t) * (size_t)n_ref, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    g_svdss_hip_err = std::string("svdss_bam_smooth_create: ") + hipGetErrorString(e);
    if (s->d_tidmap) (void)hipFree(s->d_tidmap);
    delete s;
    return e == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP;
  }
  *out = s;
  return SVDSS_OK;
}

extern "C" void svdss_bam_smooth_free(svdss_bam_smooth_t* s) {
  if (!s) return;
  if (s->device >= 0) (void)hipSetDevice(s->device);
  if (s->d_tidmap) (void)hipFree(s->d_tidmap);
  delete s;
}

extern "C" int svdss_bam_smooth_set_index(svdss_bam_smooth_t* sm, int32_t min_shift, int32_t depth) {
  if (!sm || min_shift < 0 || (min_shift > 0 && (depth < 1 || depth > 10 || min_shift + 3 * depth > 48))) return SVDSS_EINVAL;
  sm->ix_shift = min_shift;
  sm->ix_depth = min_shift > 0 ? depth : 0;
  return SVDSS_OK;
}

extern "C" int svdss_bam_smooth_set_deflate(svdss_bam_smooth_t* sm, int32_t mode) {
  if (!sm || (mode != SVDSS_DEFLATE_RUNS && mode != SVDSS_DEFLATE_LZ)) return SVDSS_EINVAL;
  sm->deflate_mode = mode;
  return SVDSS_OK;
}

extern "C" int svdss_bam_smooth_set_search(svdss_bam_smooth_t* sm, int32_t flags, svdss_bam_park_t* park) {
  if (!sm || flags < -1 || (flags >= 0 && (flags & ~(SVDSS_SFS_ASSEMBLE | SVDSS_BAM_PUTATIVE))) || (flags < 0 && park)) return SVDSS_EINVAL;
  if (park && park->device != sm->device) return SVDSS_EINVAL;
  sm->search_flags = flags;
  sm->park = park;
  return SVDSS_OK;
}

extern "C" int svdss_bam_smooth_set_output(svdss_bam_smooth_t* sm, int32_t write_bam) {
  if (!sm || (write_bam != 0 && write_bam != 1)) return SVDSS_EINVAL;
  sm->write_bam = write_bam != 0;
  return SVDSS_OK;
}

extern "C" int svdss_bam_smooth_set_store(svdss_bam_smooth_t* sm, svdss_bam_store_t* store, int32_t min_mapq) {
  if (!sm || (store && store->device != sm->device)) return SVDSS_EINVAL;
  sm->store = store;
  sm->store_min_mapq = min_mapq;
  return SVDSS_OK;
}

extern "C" int svdss_bam_stream_set_output_prefix(svdss_bam_stream_t* s, const uint8_t* bytes, int64_t n) {
  if (!s || n < 0 || (n > 0 && !bytes)) return SVDSS_EINVAL;
  std::lock_guard<std::mutex> lk(s->m);
  try { s->out_tail.assign(bytes, bytes + n); } catch (...) { return SVDSS_ENOMEM; }
  return SVDSS_OK;
}

// mode 0: measure (smoother.cpp:259-346 on the batch: matches / mismatches of the kept records come down);
// mode 1: smooth, rebuild, deflate
static int smooth_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_smooth_t* sm, int mode, double acc,
                      uint8_t* host_out, int64_t host_cap, int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes, const svdss_bgzf_block_t* const* blocks,
                      const uint32_t* const* crc, const int64_t* n_blocks, svdss_bam_batch_t** out) {
  if (!s || !sm || !out || seq < 0 || skip < 0 || n_chunks < 0) return SVDSS_EINVAL;
  constexpr auto out_turn = &svdss_bam_stream::next_out;
  const bool owes_out_turn = mode != 0;   // (a batch that fails before its output turn still has to pass that turn on)
  Front F;
  {
    const int rc = batch_front(s, seq, is_last, skip, sm->device, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, out, F);
    if (rc != SVDSS_OK) {
      if (owes_out_turn) pass_turn(s, out_turn, seq, rc, *out ? (*out)->err : std::string("batch failed"));
      return rc;
    }
  }
  svdss_bam_batch* b = *out;
  BatchRun run(b);
  if (owes_out_turn) run.release = [&](int code, const std::string& msg) { pass_turn(s, out_turn, seq, code, msg); };
  const hipStream_t st = run.st;
  const SegWalk& W = F.W;
  const int64_t n_rec = F.hdr[H_NREC];
  b->n_records = n_rec + F.hdr[H_GATED];
  b->sm.kept = 0; b->sm.out_bytes = 0; b->sm.bgzf_bytes = 0; b->sm.bgzf = nullptr;
  for (int k = 0; k < 4; ++k) b->sm.xf[k] = 0;
  RCHK(b->rpos.ensure(sizeof(uint32_t) * (size_t)(n_rec + 1)));
  const bool sfs_on = mode != 0 && sm->search_flags >= 0;
  b->search.front_done = false;
  // (with the reads exported for a search, five rows of flags over the kept records follow the two over all records)
  RCHK(b->flags.ensure(sizeof(int64_t) * (sfs_on ? 5 : 2) * (size_t)(n_rec + 1)));
  RCHK(b->scans.ensure(sizeof(int64_t) * (sfs_on ? 5 : 2) * (size_t)(n_rec + 1)));
  SmMetaP M;
  M.buf = W.buf; M.lists = W.lists; M.list_cap = W.list_cap; M.seg_cnt = W.seg_cnt; M.seg_base = F.seg_base; M.pre = (const uint32_t*)b->front.pre.p;
  M.n_seg = W.n_seg; M.min_mapq = sm->min_mapq; M.n_ref = sm->n_ref; M.n_rec = n_rec; M.tidmap = sm->d_tidmap;
  M.rpos = (uint32_t*)b->rpos.p; M.f_keep = (int64_t*)b->flags.p; M.hdr = (int64_t*)b->front.hdr.p;
  hipLaunchKernelGGL(smooth_meta_kernel, dim3((unsigned)W.n_seg + 1), dim3(64), 0, st, M);
  BCHK(hipGetLastError());
  int64_t* s_keep = (int64_t*)b->scans.p;
  RCHK(run.scan_rows(M.f_keep, s_keep, n_rec + 1, 1));
  int64_t n_keep = 0, hdr2[H_N] = {0};
  BCHK(hipMemcpyAsync(&n_keep, s_keep + n_rec, sizeof n_keep, hipMemcpyDeviceToHost, st));
  BCHK(hipMemcpyAsync(hdr2, b->front.hdr.p, sizeof hdr2, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  if (const char* bad = record_error(hdr2[H_ERR])) return run.fail(SVDSS_EIO, bad);
  b->sm.kept = n_keep;
  // per kept record: kpos u32 | nlen i32 | ncig i32 | xf_at i32 | xf_sz i32 | nmx 2 x i64 | osize, ssize, ooff, soff (n + 1) x i64 | kflags u8 | xfv u8
  const size_t nk = (size_t)n_keep + 1;
  RCHK(b->sm.rec.ensure(20 * nk + 16 * nk + 32 * nk + 2 * nk + 256));
  uint8_t* base = (uint8_t*)b->sm.rec.p;
  int64_t* d_nmx = (int64_t*)base;                    // 16 nk
  int64_t* d_osize = d_nmx + 2 * nk;                  // 8 nk each
  int64_t* d_ssize = d_osize + nk;
  int64_t* d_ooff = d_ssize + nk;
  int64_t* d_soff = d_ooff + nk;
  uint32_t* d_kpos = (uint32_t*)(d_soff + nk);        // 4 nk each
  int32_t* d_nlen = (int32_t*)(d_kpos + nk);
  int32_t* d_ncig = d_nlen + nk;
  int32_t* d_xat = d_ncig + nk;
  int32_t* d_xsz = d_xat + nk;
  uint8_t* d_kfl = (uint8_t*)(d_xsz + nk);
  uint8_t* d_xfv = d_kfl + nk;
  if (n_keep > 0) {
    SmWalkP A;
    A.buf = W.buf; A.rpos = M.rpos; A.f_keep = M.f_keep; A.s_keep = s_keep; A.n_rec = n_rec;
    A.ref = sm->ref.d_seq; A.ref_off = sm->ref.d_off; A.tidmap = sm->d_tidmap;
    A.kpos = d_kpos; A.nmx = d_nmx; A.nlen = d_nlen; A.ncig = d_ncig; A.kflags = d_kfl; A.xf_at = d_xat; A.xf_sz = d_xsz;
    hipLaunchKernelGGL(smooth_walk_kernel, dim3((unsigned)n_rec), dim3(64), 0, st, A);
    BCHK(hipGetLastError());
  }
  run.lap(3);
  if (mode == 0) {
    try { b->sm.nmx.resize(2 * (size_t)n_keep); b->sm.fits.resize((size_t)n_keep); } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
    if (n_keep > 0) {
      BCHK(hipMemcpyAsync(b->sm.nmx.data(), d_nmx, 16 * (size_t)n_keep, hipMemcpyDeviceToHost, st));
      BCHK(hipMemcpyAsync(b->sm.fits.data(), d_kfl, (size_t)n_keep, hipMemcpyDeviceToHost, st));
      BCHK(hipStreamSynchronize(st));
      for (uint8_t& f : b->sm.fits) f &= 1;
    }
    run.lap(6);
    return SVDSS_OK;
  }
  // ---- svdss_bam_smooth_set_store: what `SVDSS call` keeps of the batch's ORIGINAL records (W.buf), whatever the smoothing
  // thinks of them -- flags, sizes and their sums now; the totals come down with the sizes' below, the records go into the
  // store behind that wait (the bytes svdss_bam_select_store_run leaves: its predicate, its sizes, its export kernel)
  svdss_bam_store* store = sm->store;
  if (store) { std::lock_guard<std::mutex> lk(store->m); if (!store->complete) store = nullptr; }
  int64_t st_kept[2] = {0, 0};
  int64_t *st_flags = nullptr, *st_sums = nullptr;
  if (store) {
    const int64_t row = n_rec + 1;
    RCHK(b->sm.store_flags.ensure(sizeof(int64_t) * 3 * (size_t)row));
    RCHK(b->sm.store_scans.ensure(sizeof(int64_t) * 2 * (size_t)row));
    st_flags = (int64_t*)b->sm.store_flags.p; st_sums = (int64_t*)b->sm.store_scans.p;
    hipLaunchKernelGGL(smooth_store_flag_kernel, dim3((unsigned)((row + 255) / 256)), dim3(256), 0, st, W.buf, (const uint32_t*)M.rpos, n_rec,
                       sm->store_min_mapq, st_flags, st_flags + row, st_flags + 2 * row);
    BCHK(hipGetLastError());
    RCHK(run.scan_rows(st_flags, st_sums, row, 2));
    BCHK(hipMemcpyAsync(&st_kept[0], st_sums + n_rec, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&st_kept[1], st_sums + row + n_rec, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  }
  // ---- sizes, places, the records
  {
    SmSizeP S;
    S.buf = W.buf; S.n_keep = n_keep; S.kpos = d_kpos; S.nmx = d_nmx; S.nlen = d_nlen; S.ncig = d_ncig; S.kflags = d_kfl; S.xf_at = d_xat;
    S.acc = acc; S.xfv = d_xfv; S.osize = d_osize; S.ssize = d_ssize; S.hdr = (int64_t*)b->front.hdr.p;
    hipLaunchKernelGGL(smooth_size_kernel, dim3((unsigned)((n_keep + 1 + 255) / 256)), dim3(256), 0, st, S);
    BCHK(hipGetLastError());
    RCHK(run.scan_rows(d_osize, d_ooff, n_keep + 1, 2));   // osize -> ooff, ssize -> soff
  }
  int64_t tot[2] = {0, 0};
  BCHK(hipMemcpyAsync(&tot[0], d_ooff + n_keep, 8, hipMemcpyDeviceToHost, st));
  BCHK(hipMemcpyAsync(&tot[1], d_soff + n_keep, 8, hipMemcpyDeviceToHost, st));
  BCHK(hipMemcpyAsync(hdr2, b->front.hdr.p, sizeof hdr2, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  if (hdr2[H_ERR] & E_NCIG) return run.fail(SVDSS_ERANGE, "more than 65535 CIGAR operations (CG tag records are not supported)");
  if (store) {
    StoreBatch B;
    uint8_t* sbase = nullptr;
    if (store_reserve(store, seq, st_kept[1], st_kept[0], B, sbase)) {
      const int64_t row = n_rec + 1;
      RCHK(b->totals.ensure(64));
      hipLaunchKernelGGL(slim_export_kernel, dim3((unsigned)row), dim3(64), 0, st, W.buf, n_rec, (const uint32_t*)M.rpos, (const int64_t*)st_flags,
                         (const int64_t*)st_sums, (const int64_t*)(st_sums + row), (const int64_t*)(st_flags + 2 * row), sbase + B.at,
                         (int64_t*)(sbase + B.off_at), (int64_t*)b->totals.p + 2);
      BCHK(hipGetLastError());
    }
  }
  const int64_t out_bytes = tot[0];
  b->sm.out_bytes = out_bytes;
  // the output stream of the batch sits behind room for what the batch before leaves over (batch 0: the BAM header)
  int64_t room = kBgzfBlock;
  if (seq == 0) { std::lock_guard<std::mutex> lk(s->m); room = std::max<int64_t>(room, (int64_t)s->out_tail.size()); }
  room = (room + 255) & ~(int64_t)255;
  RCHK(b->sm.out.ensure((size_t)(room + out_bytes) + 4096));
  RCHK(b->sm.scratch.ensure((size_t)tot[1] + 4096));
  if (n_keep > 0) {
    SmWriteP A;
    A.buf = W.buf; A.n_keep = n_keep; A.kpos = d_kpos; A.nlen = d_nlen; A.ncig = d_ncig; A.xf_at = d_xat; A.xf_sz = d_xsz; A.xfv = d_xfv;
    A.ooff = d_ooff; A.soff = d_soff; A.ref = sm->ref.d_seq; A.ref_off = sm->ref.d_off; A.tidmap = sm->d_tidmap;
    A.out = (uint8_t*)b->sm.out.p + room; A.scratch = (uint8_t*)b->sm.scratch.p;
    hipLaunchKernelGGL(smooth_write_kernel, dim3((unsigned)n_keep), dim3(64), 0, st, A);
    BCHK(hipGetLastError());
  }
  std::vector<uint8_t> h_xfv;
  try { h_xfv.resize((size_t)n_keep); } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
  if (n_keep > 0) BCHK(hipMemcpyAsync(h_xfv.data(), d_xfv, (size_t)n_keep, hipMemcpyDeviceToHost, st));
  run.lap(4);
  // ---- `smooth --index --sfs`: the reads `SVDSS search` would take from these records -- names, HP and slots to the host,
  // the searched reads' bases as nt6 into the park (svdss_bam_batch_parked says where) or, without room there, into the
  // batch object (svdss_bam_smooth_search finishes it).  Before the output turn: the wait for it hides this.
  b->stage_ms[7] = 0;
  if (sfs_on) {
    int64_t pg = -1, pfirst = 0, psym = 0;      // the park's group this batch reserved room in (-1: none)
    auto unpark = [&]() { if (pg >= 0) { park_done(sm->park, pg); pg = -1; } };
    // (a failure must neither leave the group waiting for this batch nor keep the output turn)
    run.release = [&](int code, const std::string& msg) { unpark(); pass_turn(s, out_turn, seq, code, msg); };
    RCHK(b->search.d_hp.ensure(sizeof(int32_t) * nk));
    RCHK(b->search.o_small.ensure(sizeof(int32_t) * 3 * (nk + 1)));
    RCHK(b->search.d_names.ensure(std::min<size_t>((size_t)n_keep * 255, (size_t)out_bytes) + 64));
    RCHK(b->search.sym_off.ensure(sizeof(int64_t) * (nk + 1)));
    RCHK(b->search.seq_src.ensure(sizeof(int64_t) * (nk + 1)));
    SmSfsP P;
    P.out = (const uint8_t*)b->sm.out.p + room; P.ooff = d_ooff; P.n_keep = n_keep; P.putative = (sm->search_flags & SVDSS_BAM_PUTATIVE) ? 1 : 0;
    P.f_pass = (int64_t*)b->flags.p; P.f_srch = P.f_pass + nk; P.f_name = P.f_srch + nk; P.f_sym = P.f_name + nk; P.f_short = P.f_sym + nk;
    int64_t* sc = (int64_t*)b->scans.p;
    P.s_pass = sc; P.s_srch = sc + nk; P.s_name = sc + 2 * nk; P.s_sym = sc + 3 * nk;
    P.hp = (int32_t*)b->search.d_hp.p;
    P.o_name_off = (int32_t*)b->search.o_small.p; P.o_hp = P.o_name_off + (nk + 1); P.o_sidx = P.o_hp + (nk + 1);
    P.o_names = (char*)b->search.d_names.p; P.sym_off = (int64_t*)b->search.sym_off.p; P.seq_src = (int64_t*)b->search.seq_src.p;
    P.sym_base = 0;
    const unsigned g = (unsigned)((nk + 255) / 256);
    hipLaunchKernelGGL(sm_sfs_flag_kernel, dim3(g), dim3(256), 0, st, P);
    BCHK(hipGetLastError());
    RCHK(run.scan_rows(P.f_pass, sc, (int64_t)nk, 5));
    int64_t totals[5] = {0, 0, 0, 0, 0};     // slots, searched, name bytes, symbols, short
    for (int k = 0; k < 5; ++k) BCHK(hipMemcpyAsync(&totals[k], sc + (size_t)k * nk + (size_t)n_keep, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    const int64_t n_slots = totals[0], n_srch = totals[1], name_bytes = totals[2], total_syms = totals[3];
    b->search.n_slots = n_slots; b->search.n_searched = n_srch; b->search.n_short = totals[4]; b->search.total_sfs = 0;
    if (total_syms >= ((int64_t)1 << 40)) return run.fail(SVDSS_ERANGE, "batch too large");
    const size_t padded = (size_t)((total_syms + 15) & ~(int64_t)15) + 16;
    b->search.park_group = n_srch > 0 ? -1 : -2;
    b->search.park_first = 0;
    uint8_t* reads_out = nullptr;
    const int64_t* off_out = P.sym_off;
    if (n_srch > 0 && sm->park && park_reserve(sm->park, n_srch, total_syms, pg, pfirst, psym)) {
      // the reads go behind those of the batches that reserved before this one; the offsets are the group's
      ParkArena A;
      const ParkGroup G = [&] { std::lock_guard<std::mutex> lk(sm->park->m); A = sm->park->arenas[(size_t)sm->park->groups[(size_t)pg].arena]; return sm->park->groups[(size_t)pg]; }();
      reads_out = A.d_reads + G.sym0;
      P.sym_off = A.d_off + G.off0 + pfirst;
      P.sym_base = psym;
      off_out = P.sym_off;
      b->search.park_group = pg; b->search.park_first = pfirst;
    } else if (n_srch > 0) {
      RCHK(b->search.reads.ensure(padded + 16));
      reads_out = (uint8_t*)b->search.reads.p;
      BCHK(hipMemsetAsync(reads_out + (padded >= 32 ? padded - 32 : 0), 0, padded >= 32 ? 32 : padded, st));
    }
    hipLaunchKernelGGL(sm_sfs_scatter_kernel, dim3(g), dim3(256), 0, st, P);
    BCHK(hipGetLastError());
    if (n_srch > 0) {
      hipLaunchKernelGGL(sm_sfs_nt6_kernel, dim3((unsigned)n_srch), dim3(256), 0, st, P.out, (const int64_t*)P.seq_src, off_out, reads_out);
      BCHK(hipGetLastError());
    }
    b->search.name_bytes = name_bytes;
    try {
      b->search.name_off.resize((size_t)n_slots + 1); b->search.hp.resize((size_t)n_slots); b->search.sidx.resize((size_t)n_slots);
      b->search.names.resize((size_t)name_bytes + 1); b->search.counts.clear(); b->search.qs.clear(); b->search.len.clear();
    } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
    {
      hipError_t e = hipMemcpyAsync(b->search.name_off.data(), P.o_name_off, sizeof(int32_t) * (size_t)(n_slots + 1), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && n_slots > 0) e = hipMemcpyAsync(b->search.hp.data(), P.o_hp, sizeof(int32_t) * (size_t)n_slots, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && n_slots > 0) e = hipMemcpyAsync(b->search.sidx.data(), P.o_sidx, sizeof(int32_t) * (size_t)n_slots, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && name_bytes > 0) e = hipMemcpyAsync(b->search.names.data(), P.o_names, (size_t)name_bytes, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      unpark();     // (the bases are in place: the group may be searched)
      if (e != hipSuccess) { g_svdss_hip_err = std::string("smooth sfs export: ") + hipGetErrorString(e); return run.fail(e == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP, g_svdss_hip_err); }
    }
    b->search.cur_reads = reads_out; b->search.cur_off = off_out; b->search.cur_syms = total_syms; b->search.cur_flags = sm->search_flags;
    b->search.front_done = true;
    run.release = [&](int code, const std::string& msg) { pass_turn(s, out_turn, seq, code, msg); };
    run.lap(7);
  }
  // ---- the output turn
  const bool my_turn = wait_turn(s, out_turn, seq);
  run.release = nullptr;   // (taken, or let through by a stream that failed: nothing to pass on any more)
  if (!my_turn) return run.fail(s->failed, s->err);
  if (!sm->write_bam) {
    // --nobam: nothing of the output stream is kept -- no tail handed on, no members; the turn itself is passed on in order
    const hipError_t e = hipStreamSynchronize(st);   // (the XF values are down)
    if (e != hipSuccess) g_svdss_hip_err = std::string("smooth output turn: ") + hipGetErrorString(e);
    done_turn(s, out_turn, e == hipSuccess ? SVDSS_OK : SVDSS_EHIP, e == hipSuccess ? std::string() : g_svdss_hip_err);
    if (e != hipSuccess) { b->err = g_svdss_hip_err; return SVDSS_EHIP; }
    for (uint8_t v : h_xfv) ++b->sm.xf[v & 3];
    b->sm_ix.on = false; b->sm_ix.chunks.clear(); b->sm_ix.windows.clear();
    run.lap(5);
    b->stage_ms[6] = 0;
    return SVDSS_OK;
  }
  int turn_code = SVDSS_OK;
  std::string turn_msg;
  int64_t in_len = 0, stream_bytes = 0, n_blk = 0;
  {
    auto turn_fail = [&](int code, const std::string& msg) { turn_code = code; turn_msg = msg; };
    const int64_t tail_in = (int64_t)s->out_tail.size();
    hipError_t e = hipSuccess;
    if (tail_in > room) turn_fail(SVDSS_ERANGE, "output tail larger than its room");
    if (!turn_code && tail_in > 0)
      e = hipMemcpyAsync((uint8_t*)b->sm.out.p + (room - tail_in), s->out_tail.data(), (size_t)tail_in, hipMemcpyHostToDevice, st);
    stream_bytes = tail_in + out_bytes;
    in_len = is_last ? stream_bytes : stream_bytes / kBgzfBlock * kBgzfBlock;     // the last batch also writes the short block
    const int64_t tail_out = stream_bytes - in_len;
    if (!turn_code && e == hipSuccess) {
      try { s->out_tail.resize((size_t)tail_out); } catch (...) { turn_fail(SVDSS_ENOMEM, "out of memory"); }
      if (!turn_code && tail_out > 0)
        e = hipMemcpyAsync(s->out_tail.data(), (const uint8_t*)b->sm.out.p + (room - tail_in) + in_len, (size_t)tail_out, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess && !turn_code) {
      g_svdss_hip_err = std::string("smooth output turn: ") + hipGetErrorString(e);
      turn_fail(e == hipErrorOutOfMemory ? SVDSS_ENOMEM : SVDSS_EHIP, g_svdss_hip_err);
    }
    b->sm.in0 = room - tail_in;
  }
  done_turn(s, out_turn, turn_code, turn_msg);
  if (turn_code) { b->err = turn_msg; return turn_code; }
  for (uint8_t v : h_xfv) ++b->sm.xf[v & 3];
  run.lap(5);
  // ---- BGZF: deflate, footers, back to back, down
  n_blk = (in_len + kBgzfBlock - 1) / kBgzfBlock;
  b->sm.bgzf_bytes = 0;
  const int64_t* d_off_out = nullptr;   // the members' compressed offsets (for the index fragments)
  if (n_blk > 0) {
    const int64_t stride = svdss_deflate_stride((int32_t)kBgzfBlock);
    RCHK(b->sm.members.ensure((size_t)(n_blk * stride) + 256));
    RCHK(b->sm.dense.ensure((size_t)(n_blk * stride) + 256));
    RCHK(b->sm.len.ensure(sizeof(int32_t) * (size_t)n_blk + sizeof(int64_t) * (size_t)(n_blk + 1) + 256));
    int32_t* d_len = (int32_t*)b->sm.len.p;
    int64_t* d_off = (int64_t*)((uint8_t*)b->sm.len.p + ((sizeof(int32_t) * (size_t)n_blk + 63) & ~(size_t)63));
    d_off_out = d_off;
    const uint8_t* d_in = (const uint8_t*)b->sm.out.p + b->sm.in0;
    BCHK(hipMemsetAsync(b->sm.members.p, 0, (size_t)(n_blk * stride), st));
    const size_t lz_bytes = (size_t)svdss_deflate_scratch_bytes(in_len, (int32_t)kBgzfBlock, sm->deflate_mode);
    if (lz_bytes) RCHK(b->sm.lz.ensure(lz_bytes));
    BCHK(svdss_deflate_enqueue_mode(st, d_in, in_len, (int32_t)kBgzfBlock, (uint8_t*)b->sm.members.p, stride, d_len, sm->deflate_mode,
                                    lz_bytes ? b->sm.lz.p : nullptr));
    BCHK(crc_tables_ready());
    FootP Fp{d_in, in_len, (int32_t)kBgzfBlock, (uint8_t*)b->sm.members.p, stride, d_len};
    hipLaunchKernelGGL(bgzf_footer_kernel, dim3((unsigned)n_blk), dim3(64), 0, st, Fp);
    BCHK(hipGetLastError());
    BCHK(svdss_deflate_compact_enqueue(st, (const uint8_t*)b->sm.members.p, stride, d_len, n_blk, d_off, (uint8_t*)b->sm.dense.p));
    int64_t total = 0;
    BCHK(hipMemcpyAsync(&total, d_off + n_blk, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    uint8_t* dst = host_out;
    if (!dst || total > host_cap) {     // (no buffer of the caller's, or too small a one: the batch object's own)
      RCHK(b->sel.host.ensure((size_t)total));
      dst = (uint8_t*)b->sel.host.p;
    }
    BCHK(hipMemcpyAsync(dst, b->sm.dense.p, (size_t)total, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    b->sm.bgzf = dst;
    b->sm.bgzf_bytes = total;
  }
  // ---- index fragments (`smooth --write-index`): chunks and first-reached windows, reduced here; only they come down
  b->sm_ix.on = sm->ix_shift > 0;
  b->sm_ix.chunks.clear(); b->sm_ix.windows.clear();
  for (int64_t& v : b->sm_ix.hdr) v = 0;
  if (b->sm_ix.on && n_keep > 0) {
    const size_t nk1 = (size_t)n_keep + 1;
    RCHK(b->sm_ix.rec.ensure(80 * nk1 + 8 * nk1 + 256));
    SmIxP P;
    P.out = (const uint8_t*)b->sm.out.p + room; P.ooff = d_ooff; P.n_keep = n_keep;
    P.tail_in = room - b->sm.in0; P.in_len = in_len; P.n_blk = n_blk; P.d_off = d_off_out;
    P.min_shift = sm->ix_shift; P.depth = sm->ix_depth;
    int64_t* i64 = (int64_t*)b->sm_ix.rec.p;
    unsigned long long* d_err = (unsigned long long*)i64;    // 8 bytes, then the per-record arrays
    P.err = d_err;
    P.beg = i64 + 1; P.end = P.beg + nk1; P.head = P.end + nk1; P.own = P.head + nk1;
    int64_t* s_head = P.own + nk1; int64_t* s_own = s_head + nk1;
    P.s_head = s_head; P.s_own = s_own;
    P.vb = (uint64_t*)(s_own + nk1); P.ve = P.vb + nk1; P.key = P.ve + nk1;
    uint64_t* kmax = P.key + nk1;
    P.kmax = kmax;
    P.tid = (int32_t*)(kmax + nk1); P.bin = (uint32_t*)(P.tid + nk1);
    P.chunks = nullptr; P.windows = nullptr;
    const unsigned g = (unsigned)((n_keep + 1 + 255) / 256);
    BCHK(hipMemsetAsync(d_err, 0, 8, st));
    hipLaunchKernelGGL(sm_ix_rec_kernel, dim3(g), dim3(256), 0, st, P);
    BCHK(hipGetLastError());
    {
      size_t t0 = 0, t1 = 0;
      BCHK(hipcub::DeviceScan::ExclusiveScan(nullptr, t0, P.key, kmax, hipcub::Max(), (uint64_t)0, (int)n_keep, st));
      BCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, P.head, s_head, (int)nk1, st));
      RCHK(run.scan_tmp(std::max(t0, t1)));   // (room for the sums below as well: nothing is allocated between the kernels)
      t0 = b->tmp.cap;
      BCHK(hipcub::DeviceScan::ExclusiveScan(b->tmp.p, t0, P.key, kmax, hipcub::Max(), (uint64_t)0, (int)n_keep, st));
      hipLaunchKernelGGL(sm_ix_own_kernel, dim3(g), dim3(256), 0, st, P);
      BCHK(hipGetLastError());
      RCHK(run.scan_rows(P.head, s_head, (int64_t)nk1, 2));   // head -> s_head, own -> s_own
    }
    // counts, order flag, the first and last record's (tid, beg)
    int64_t cnt[2] = {0, 0}, be[2] = {0, 0};
    int32_t td[2] = {0, 0};
    unsigned long long h_err = 0;
    BCHK(hipMemcpyAsync(&cnt[0], s_head + n_keep, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&cnt[1], s_own + n_keep, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&h_err, d_err, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&td[0], P.tid, 4, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&td[1], P.tid + (n_keep - 1), 4, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&be[0], P.beg, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&be[1], P.beg + (n_keep - 1), 8, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    b->sm_ix.hdr[2] = td[0]; b->sm_ix.hdr[3] = td[1]; b->sm_ix.hdr[4] = be[0]; b->sm_ix.hdr[5] = be[1];
    if (h_err & 1) b->sm_ix.hdr[6] = 1;      // out of order: the builder refuses; nothing else comes down
    else {
      const int64_t n_ch = cnt[0], n_win = cnt[1];
      const size_t ch_bytes = sizeof(svdss_bam_index_chunk_t) * (size_t)n_ch;
      RCHK(b->sm_ix.frag.ensure(ch_bytes + sizeof(svdss_bam_index_window_t) * (size_t)n_win + 256));
      P.chunks = (svdss_bam_index_chunk_t*)b->sm_ix.frag.p;
      P.windows = (svdss_bam_index_window_t*)((uint8_t*)b->sm_ix.frag.p + ((ch_bytes + 255) & ~(size_t)255));
      try { b->sm_ix.chunks.resize((size_t)n_ch); b->sm_ix.windows.resize((size_t)n_win); } catch (...) { return run.fail(SVDSS_ENOMEM, "out of memory"); }
      BCHK(hipMemsetAsync(P.chunks, 0, ch_bytes, st));
      hipLaunchKernelGGL(sm_ix_emit_kernel, dim3(g), dim3(256), 0, st, P);
      BCHK(hipGetLastError());
      if (n_ch) BCHK(hipMemcpyAsync(b->sm_ix.chunks.data(), P.chunks, ch_bytes, hipMemcpyDeviceToHost, st));
      if (n_win) BCHK(hipMemcpyAsync(b->sm_ix.windows.data(), P.windows, sizeof(svdss_bam_index_window_t) * (size_t)n_win, hipMemcpyDeviceToHost, st));
      BCHK(hipStreamSynchronize(st));
    }
  }
  run.lap(6);
  return SVDSS_OK;
}

extern "C" int svdss_bam_smooth_measure(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_smooth_t* sm,
                                        int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                        const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                        svdss_bam_batch_t** out) {
  return smooth_run(s, seq, is_last, skip, sm, 0, 0.0, nullptr, 0, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, out);
}

extern "C" int svdss_bam_smooth_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_smooth_t* sm,
                                    double max_mismatch_rate, uint8_t* host_out, int64_t host_cap, int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                                    const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                                    svdss_bam_batch_t** out) {
  return smooth_run(s, seq, is_last, skip, sm, 1, max_mismatch_rate, host_out, host_cap, n_chunks, comp, comp_bytes, blocks, crc, n_blocks, out);
}

extern "C" int svdss_bam_batch_index(const svdss_bam_batch_t* b, svdss_bam_index_frag_t* f) {
  if (!b || !f) return SVDSS_EINVAL;
  f->n_chunks = (int64_t)b->sm_ix.chunks.size(); f->chunks = b->sm_ix.chunks.data();
  f->n_windows = (int64_t)b->sm_ix.windows.size(); f->windows = b->sm_ix.windows.data();
  f->unsorted = (int32_t)b->sm_ix.hdr[6];
  f->first_tid = (int32_t)b->sm_ix.hdr[2]; f->last_tid = (int32_t)b->sm_ix.hdr[3];
  f->first_beg = b->sm_ix.hdr[4]; f->last_beg = b->sm_ix.hdr[5];
  return SVDSS_OK;
}

extern "C" int svdss_bam_batch_smoothed(const svdss_bam_batch_t* b, svdss_bam_smoothed_t* r) {
  if (!b || !r) return SVDSS_EINVAL;
  r->n_records = b->n_records; r->n_kept = b->sm.kept;
  r->match_mismatch = b->sm.nmx.data(); r->fits = b->sm.fits.data();
  r->out_bytes = b->sm.out_bytes;
  r->bgzf = b->sm.bgzf; r->bgzf_bytes = b->sm.bgzf_bytes;
  for (int k = 0; k < 4; ++k) r->n_xf[k] = b->sm.xf[k];
  r->inflate_kernel_ms = b->inflate_ms;
  for (int k = 0; k < 8; ++k) r->stage_ms[k] = b->stage_ms[k];
  return SVDSS_OK;
}

// A batch whose reads stayed in the batch object (svdss_bam_batch_parked: group -1): searched here, counts and SFS down
// (svdss_bam_batch_result).  The smoothing run's stage clock stays as it was; the search is added to its stage 7.
extern "C" int svdss_bam_smooth_search(svdss_bam_batch_t* b, const svdss_index_t* ix) {
  if (!b || !ix) return SVDSS_EINVAL;
  double keep[8];
  for (int k = 0; k < 8; ++k) keep[k] = b->stage_ms[k];
  const int rc = svdss_bam_batch_search(b, ix);
  if (rc == SVDSS_OK) keep[7] += b->stage_ms[5] + b->stage_ms[6];
  for (int k = 0; k < 8; ++k) b->stage_ms[k] = keep[k];
  return rc;
}
