// input_index_fold.cpp -- the input-side fold of csrc/bam_index_writer.h (BamIndexBuilder::add_input_fragment / add_input_seam /
// finish_input) without a GPU: the BAM is read here, cut into batches of consecutive members and into regions, every batch
// reduced to the fragments the device path leaves (svdss_bam_input_frag_t: chunks and first-reached windows relative to the
// batch's first member, a record that began in an earlier batch addressed below the batch's base, the last record's end at the
// batch's last byte left to the fold), every seam to the one record it completes -- and folded.  tests/test_bam_input_index.py
// holds the file written against the host reader's.  Stand-alone: also what a sanitizer run of the fold uses.
//   _input_index_fold BAM OUT MEMBERS_PER_BATCH [first member of region 1, of region 2, ...]
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../svdss_amd/csrc/bam_index_writer.h"

struct Member { uint64_t coff, clen; int64_t u0, n; };
struct Rec { int64_t u0, u1; int32_t tid, pos; uint32_t flag; int64_t span; };

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> d;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + k);
  fclose(f);
  return d;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s BAM OUT MEMBERS_PER_BATCH [region starts]\n", argv[0]); return 2; }
  const std::vector<uint8_t> file = slurp(argv[1]);
  const size_t per_batch = (size_t)atoll(argv[3]);
  // ---- members and the inflated stream
  std::vector<Member> mem;
  std::vector<uint8_t> raw;
  for (size_t p = 0; p + 18 <= file.size();) {
    uint16_t bsize;
    memcpy(&bsize, file.data() + p + 16, 2);
    const size_t tot = (size_t)bsize + 1;
    uint32_t isize;
    memcpy(&isize, file.data() + p + tot - 4, 4);
    const size_t at = raw.size();
    raw.resize(at + isize);
    if (isize) {
      z_stream z;
      memset(&z, 0, sizeof z);
      inflateInit2(&z, -15);
      z.next_in = const_cast<uint8_t*>(file.data() + p + 18); z.avail_in = (uInt)(tot - 26);
      z.next_out = raw.data() + at; z.avail_out = isize;
      if (inflate(&z, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "inflate failed\n"); return 2; }
      inflateEnd(&z);
    }
    mem.push_back(Member{p, tot, (int64_t)at, (int64_t)isize});
    p += tot;
  }
  const uint64_t end_off = !mem.empty() && mem.back().n == 0 && mem.back().clen == 28 ? mem.back().coff : file.size();
  // ---- header, records
  int32_t l_text, n_ref;
  memcpy(&l_text, raw.data() + 4, 4);
  memcpy(&n_ref, raw.data() + 8 + l_text, 4);
  int64_t u = 12 + (int64_t)l_text;
  std::vector<int32_t> lens;
  for (int32_t i = 0; i < n_ref; ++i) {
    int32_t l_name, len;
    memcpy(&l_name, raw.data() + u, 4);
    memcpy(&len, raw.data() + u + 4 + l_name, 4);
    lens.push_back(len);
    u += 8 + l_name;
  }
  std::vector<Rec> recs;
  while (u + 4 <= (int64_t)raw.size()) {
    const uint8_t* r = raw.data() + u;
    int32_t bs;
    memcpy(&bs, r, 4);
    Rec x;
    x.u0 = u; x.u1 = u + 4 + bs;
    memcpy(&x.tid, r + 4, 4); memcpy(&x.pos, r + 8, 4);
    uint16_t n_cig, flag;
    memcpy(&n_cig, r + 16, 2); memcpy(&flag, r + 18, 2);
    x.flag = flag; x.span = 0;
    for (uint32_t k = 0; k < n_cig; ++k) {
      uint32_t c;
      memcpy(&c, r + 36 + r[12] + 4 * (size_t)k, 4);
      if (ix_ref_op(c & 15u)) x.span += c >> 4;
    }
    recs.push_back(x);
    u = x.u1;
  }
  bool csi;
  int shift, depth;
  std::string err;
  if (!bam_index_scheme(argv[2], lens, csi, shift, depth, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  BamIndexBuilder B(n_ref, csi, shift, depth);
  // the virtual offset of stream position q relative to file offset `base`: the member that holds the byte; hi: the end of
  // the batch's bytes, addressed right behind its members
  auto voff = [&](int64_t q, uint64_t base, int64_t hi, uint64_t behind) -> uint64_t {
    if (q >= hi) return (behind - base) << 16;
    size_t a = 0, b = mem.size();
    while (b - a > 1) { const size_t m = (a + b) / 2; if (mem[m].u0 <= q) a = m; else b = m; }
    return ((mem[a].coff - base) << 16) + (uint64_t)(q - mem[a].u0);       // (below the base: wraps)
  };
  // ---- regions of members, batches of members
  std::vector<size_t> cuts{0};
  for (int i = 4; i < argc; ++i) cuts.push_back((size_t)atoll(argv[i]));
  cuts.push_back(mem.size());
  size_t next_rec = 0;
  for (size_t g = 0; g + 1 < cuts.size(); ++g) {
    const int64_t reg_u0 = cuts[g] < mem.size() ? mem[cuts[g]].u0 : (int64_t)raw.size();
    if (g > 0 && next_rec < recs.size() && recs[next_rec].u0 < reg_u0) {
      // the seam: the record the region in front could not complete -- as a batch of its own whose offsets mean nothing
      const Rec& x = recs[next_rec++];
      svdss_bam_input_frag_t f{};
      svdss_bam_input_chunk_t ch{};
      std::vector<svdss_bam_input_window_t> win;
      f.on = 1; f.n_records = 1; f.first_tid = f.last_tid = x.tid;
      int64_t beg = 0, end = 1;
      if (x.tid >= 0) {
        ix_extent(x.pos, x.span, shift, depth, beg, end);
        ch.tid = x.tid; ch.bin = ix_reg2bin(beg, end, shift, depth); ch.n_rec = 1; ch.n_unmapped = (x.flag & 4) ? 1 : 0; ch.v_beg = 77; ch.v_end = 99;
        f.n_chunks = 1; f.chunks = &ch;
        for (int64_t w = beg >> shift; w <= (end - 1) >> shift; ++w) win.push_back(svdss_bam_input_window_t{x.tid, (int32_t)w, 77});
        f.n_windows = (int64_t)win.size(); f.windows = win.data();
      } else f.n_no_coor = 1;
      f.first_beg = f.last_beg = beg;
      // its start: where the carry of the region in front begins; its end: the first record start of this region
      B.add_input_seam(f, voff(x.u0, 0, (int64_t)raw.size() + 1, 0), voff(x.u1, 0, (int64_t)raw.size() + 1, 0));
    }
    for (size_t m0 = cuts[g]; m0 < cuts[g + 1]; m0 += per_batch) {
      const size_t m1 = std::min(m0 + per_batch, cuts[g + 1]);
      const uint64_t base = mem[m0].coff, behind = mem[m1 - 1].coff + mem[m1 - 1].clen;
      const int64_t hi = mem[m1 - 1].u0 + mem[m1 - 1].n;
      svdss_bam_input_frag_t f{};
      f.on = 1; f.first_data = -1; f.comp_bytes = (int64_t)(behind - base);
      for (size_t m = m0; m < m1; ++m) if (mem[m].n > 0) { f.first_data = (int64_t)(mem[m].coff - base); break; }
      std::vector<svdss_bam_input_chunk_t> chunks;
      std::vector<svdss_bam_input_window_t> win;
      int32_t seen_tid = -1;
      int64_t seen_win = -1;         // the last window the batch's records have reached on seen_tid
      bool prev_ix = false;
      const size_t first = next_rec;
      while (next_rec < recs.size() && recs[next_rec].u1 <= hi) {       // the records that are complete in this batch
        const Rec& x = recs[next_rec];
        int64_t beg = 0, end = 1;
        if (next_rec > first) {
          const Rec& p = recs[next_rec - 1];
          int64_t pb = 0, pe = 1;
          if (p.tid >= 0) ix_extent(p.pos, p.span, shift, depth, pb, pe);
          int64_t cb = 0, ce = 1;
          if (x.tid >= 0) ix_extent(x.pos, x.span, shift, depth, cb, ce);
          const int64_t a = x.tid < 0 ? 0x7fffffff : x.tid, b = p.tid < 0 ? 0x7fffffff : p.tid;
          if (a < b || (a == b && cb < pb)) f.unsorted = 1;
        }
        if (x.tid >= 0) {
          ix_extent(x.pos, x.span, shift, depth, beg, end);
          const uint32_t bin = ix_reg2bin(beg, end, shift, depth);
          const uint64_t vb = voff(x.u0, base, hi, behind), ve = voff(x.u1, base, hi, behind);
          if (!prev_ix || chunks.back().tid != x.tid || chunks.back().bin != bin) chunks.push_back(svdss_bam_input_chunk_t{x.tid, bin, 0, 0, vb, ve});
          chunks.back().v_end = ve;
          chunks.back().n_rec += 1;
          chunks.back().n_unmapped += (x.flag & 4) ? 1 : 0;
          if (x.tid != seen_tid) { seen_tid = x.tid; seen_win = -1; }
          for (int64_t w = std::max(beg >> shift, seen_win + 1); w <= (end - 1) >> shift; ++w) win.push_back(svdss_bam_input_window_t{x.tid, (int32_t)w, vb});
          seen_win = std::max(seen_win, (end - 1) >> shift);
          prev_ix = true;
        } else { ++f.n_no_coor; prev_ix = false; }
        if (next_rec == first) { f.first_tid = x.tid; f.first_beg = beg; }
        f.last_tid = x.tid; f.last_beg = beg;
        ++f.n_records;
        ++next_rec;
      }
      f.n_chunks = (int64_t)chunks.size(); f.chunks = chunks.data();
      f.n_windows = (int64_t)win.size(); f.windows = win.data();
      f.ends_at_boundary = f.n_records > 0 && recs[next_rec - 1].u1 == hi && recs[next_rec - 1].tid >= 0 ? 1 : 0;
      B.add_input_fragment(f, base);
    }
  }
  B.finish_input(end_off);
  if (B.unsorted()) { fprintf(stderr, "not sorted\n"); return 1; }
  if (!B.write(argv[2], err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  printf("%zu records, %zu members, %llu chunks\n", recs.size(), mem.size(), (unsigned long long)B.n_chunks());
  return 0;
}
