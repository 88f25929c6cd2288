// gzip_host_harness.cpp -- csrc/gzip_stream.h on the CPU, as a program of its own (tests/test_gzip_host.py builds it with
// -fsanitize=address,undefined and runs it):
//   headers   every FLG combination of a gzip member header, whole and cut after every byte; bad magic, method, flags
//   combine   gz_crc32_combine against zlib's crc32 of the concatenation, second lengths 0, 1 and 2^20 + 3
//   resume    GzHostTail from the carried state at the end of every deflate block of a stream whose block ends fall on
//             every bit offset 0..7: the rest of the text, the trailer checked, a second member and trailing bytes behind it
// Prints one line per part and exits 0, or says what differs and exits 1.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../svdss_amd/csrc/gzip_stream.h"

static int fail(const std::string& what) {
  printf("FAIL %s\n", what.c_str());
  return 1;
}

static std::vector<uint8_t> make_text(size_t n, uint32_t seed) {
  std::vector<uint8_t> t(n);
  uint32_t x = seed;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    const bool qual = (i / 700) & 1;
    t[i] = qual ? (uint8_t)(40 + ((x >> 24) % 30)) : (uint8_t)"ACGT"[(x >> 24) & 3];
    if (i % 700 == 699) t[i] = '\n';
  }
  return t;
}

static std::vector<uint8_t> raw_deflate(const std::vector<uint8_t>& text, int level, int mem_level) {
  z_stream z;
  memset(&z, 0, sizeof z);
  deflateInit2(&z, level, Z_DEFLATED, -15, mem_level, Z_DEFAULT_STRATEGY);
  std::vector<uint8_t> out(deflateBound(&z, (uLong)text.size()) + 64);
  z.next_in = const_cast<uint8_t*>(text.data());
  z.avail_in = (uInt)text.size();
  z.next_out = out.data();
  z.avail_out = (uInt)out.size();
  deflate(&z, Z_FINISH);
  out.resize(z.total_out);
  deflateEnd(&z);
  return out;
}

static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }

static int test_headers() {
  int n_ok = 0;
  for (int flg = 0; flg < 32; ++flg) {
    std::vector<uint8_t> h = {0x1f, 0x8b, 8, (uint8_t)flg, 1, 2, 3, 4, 2, 3};
    if (flg & 4) { h.push_back(5); h.push_back(0); for (int i = 0; i < 5; ++i) h.push_back((uint8_t)(i * 50)); }
    if (flg & 8) { for (char c : std::string("reads.fastq")) h.push_back((uint8_t)c); h.push_back(0); }
    if (flg & 16) { for (char c : std::string("a comment")) h.push_back((uint8_t)c); h.push_back(0); }
    if (flg & 2) { h.push_back(0xab); h.push_back(0xcd); }
    const size_t len = h.size();
    h.push_back(0x03);      // (something behind it)
    h.push_back(0x00);
    if (gz_parse_header(h.data(), (int64_t)h.size()) != (int64_t)len) return fail("header length, FLG " + std::to_string(flg));
    if (gz_parse_header(h.data(), (int64_t)len) != (int64_t)len) return fail("header exactly, FLG " + std::to_string(flg));
    for (size_t cut = 0; cut < len; ++cut) {
      // (a copy of exactly `cut` bytes: the sanitizer sees a read past it)
      std::vector<uint8_t> c(h.begin(), h.begin() + (long)cut);
      if (gz_parse_header(c.data(), (int64_t)cut) != 0) return fail("cut header, FLG " + std::to_string(flg) + " at " + std::to_string(cut));
    }
    ++n_ok;
  }
  const uint8_t bad_magic[10] = {0x1f, 0x8c, 8, 0, 0, 0, 0, 0, 0, 3}, bad_method[10] = {0x1f, 0x8b, 7, 0, 0, 0, 0, 0, 0, 3},
                bad_flags[10] = {0x1f, 0x8b, 8, 0x20, 0, 0, 0, 0, 0, 3};
  if (gz_parse_header(bad_magic, 10) != -1 || gz_parse_header(bad_magic, 2) != -1) return fail("bad magic");
  if (gz_parse_header(bad_method, 10) != -1 || gz_parse_header(bad_method, 3) != -1) return fail("bad method");
  if (gz_parse_header(bad_flags, 10) != -1) return fail("reserved flags");
  if (gz_parse_header(bad_magic, 0) != 0 || gz_parse_header(bad_magic, 1) != 0) return fail("empty");
  printf("headers ok: %d FLG combinations\n", n_ok);
  return 0;
}

static int test_combine() {
  const std::vector<uint8_t> a = make_text(70001, 7), b = make_text((1u << 20) + 3, 9);
  const size_t lens[] = {0, 1, ((size_t)1 << 20) + 3, 4096, 65535};
  for (size_t la : {(size_t)0, (size_t)1, a.size()})
    for (size_t lb : lens) {
      std::vector<uint8_t> cat(a.begin(), a.begin() + (long)la);
      cat.insert(cat.end(), b.begin(), b.begin() + (long)lb);
      const uint32_t c1 = (uint32_t)crc32(0, a.data(), (uInt)la), c2 = (uint32_t)crc32(0, b.data(), (uInt)lb);
      const uint32_t want = (uint32_t)crc32(0, cat.data(), (uInt)cat.size());
      if (gz_crc32_combine(c1, c2, lb) != want) return fail("combine " + std::to_string(la) + " + " + std::to_string(lb));
    }
  // many pieces in a row, as the unit joins them
  uint32_t run = 0;
  size_t at = 0, step = 1;
  while (at < b.size()) {
    const size_t n = std::min(step, b.size() - at);
    run = gz_crc32_combine(run, (uint32_t)crc32(0, b.data() + at, (uInt)n), n);
    at += n;
    step = step * 3 + 1;
  }
  if (run != (uint32_t)crc32(0, b.data(), (uInt)b.size())) return fail("combine chain");
  printf("combine ok\n");
  return 0;
}

static int read_all(GzHostTail& t, std::vector<uint8_t>& out, size_t piece) {
  std::vector<uint8_t> buf(piece);
  for (;;) {
    const int64_t n = t.next(buf.data(), buf.size());
    if (n < 0) return -1;
    if (n == 0) return 0;
    out.insert(out.end(), buf.begin(), buf.begin() + n);
  }
}

static int test_resume() {
  const std::vector<uint8_t> text = make_text(400000, 3), second = make_text(5000, 4);
  // (memLevel 1: a block every few hundred symbols, so the block ends fall on every bit offset)
  const std::vector<uint8_t> body = raw_deflate(text, 6, 1);
  std::vector<uint8_t> file = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
  const size_t body_at = file.size();
  file.insert(file.end(), body.begin(), body.end());
  put32(file, (uint32_t)crc32(0, text.data(), (uInt)text.size()));
  put32(file, (uint32_t)text.size());
  const size_t one_member = file.size();
  {
    std::vector<uint8_t> b2 = raw_deflate(second, 9, 8);
    const uint8_t h[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
    file.insert(file.end(), h, h + 10);
    file.insert(file.end(), b2.begin(), b2.end());
    put32(file, (uint32_t)crc32(0, second.data(), (uInt)second.size()));
    put32(file, (uint32_t)second.size());
  }
  for (char c : std::string("trailing bytes, no header")) file.push_back((uint8_t)c);
  std::vector<uint8_t> want_rest_all(text);
  want_rest_all.insert(want_rest_all.end(), second.begin(), second.end());

  // the block ends, by zlib itself (Z_BLOCK): bit position in the body and bytes of text in front of it
  z_stream z;
  memset(&z, 0, sizeof z);
  inflateInit2(&z, -15);
  std::vector<uint8_t> sink(text.size() + 16);
  z.next_in = const_cast<uint8_t*>(body.data());
  z.avail_in = (uInt)body.size();
  z.next_out = sink.data();
  z.avail_out = (uInt)sink.size();
  struct End { uint64_t bit; size_t bytes; };
  std::vector<End> ends = {{0, 0}};
  for (;;) {
    const int rc = inflate(&z, Z_BLOCK);
    if (rc != Z_OK && rc != Z_STREAM_END) { inflateEnd(&z); return fail("zlib Z_BLOCK"); }
    if (rc == Z_STREAM_END) break;
    if ((z.data_type & 128) && !(z.data_type & 64)) ends.push_back({8ull * z.total_in - (uint64_t)(z.data_type & 63), (size_t)z.total_out});
  }
  inflateEnd(&z);
  int seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int n_run = 0;
  for (size_t e = 0; e < ends.size(); ++e) {
    const int bit = (int)(ends[e].bit & 7);
    if (seen[bit] >= 6 && e + 3 < ends.size()) continue;      // (six per bit offset, and the last few)
    ++seen[bit];
    GzCarry c;
    c.byte_pos = (int64_t)(body_at + (ends[e].bit >> 3));
    c.bit = bit;
    c.in_member = 1;
    c.crc = (uint32_t)crc32(0, text.data(), (uInt)ends[e].bytes);
    c.count = ends[e].bytes;
    c.dict_len = (uint32_t)std::min<size_t>(32768, ends[e].bytes);
    memcpy(c.dict + 32768 - c.dict_len, text.data() + ends[e].bytes - c.dict_len, c.dict_len);
    for (int variant = 0; variant < 2; ++variant) {
      // variant 0: the file ends with the first member; 1: a second member and trailing bytes follow
      const size_t file_end = variant ? file.size() : one_member;
      size_t at = (size_t)c.byte_pos;
      const size_t feed = 1 + (e * 37 + (size_t)variant) % 5000;      // (pieces of odd sizes)
      GzHostTail tail(c, [&](uint8_t* dst, size_t cap) {
        const size_t n = std::min(std::min(cap, feed), file_end - at);
        memcpy(dst, file.data() + at, n);
        at += n;
        return n;
      });
      std::vector<uint8_t> got;
      if (read_all(tail, got, 1 + (e * 101) % 70000) != 0) return fail("resume at block end " + std::to_string(e) + ": " + tail.error());
      const std::vector<uint8_t>& all = variant ? want_rest_all : text;
      if (got.size() != all.size() - ends[e].bytes || memcmp(got.data(), all.data() + ends[e].bytes, got.size()) != 0)
        return fail("resume at block end " + std::to_string(e) + " (bit " + std::to_string(bit) + "): text differs");
      ++n_run;
    }
  }
  for (int b = 0; b < 8; ++b)
    if (!seen[b]) return fail("no block end at bit offset " + std::to_string(b));
  // a wrong CRC32, a wrong ISIZE and a truncated stream are errors
  for (int kind = 0; kind < 3; ++kind) {
    std::vector<uint8_t> f(file.begin(), file.begin() + (long)one_member);
    if (kind == 0) f[one_member - 8] ^= 1;
    if (kind == 1) f[one_member - 1] ^= 1;
    if (kind == 2) f.resize(one_member - 20);
    const End& e = ends[ends.size() / 2];
    GzCarry c;
    c.byte_pos = (int64_t)(body_at + (e.bit >> 3));
    c.bit = (int)(e.bit & 7);
    c.in_member = 1;
    c.crc = (uint32_t)crc32(0, text.data(), (uInt)e.bytes);
    c.count = e.bytes;
    c.dict_len = (uint32_t)std::min<size_t>(32768, e.bytes);
    memcpy(c.dict + 32768 - c.dict_len, text.data() + e.bytes - c.dict_len, c.dict_len);
    size_t at = (size_t)c.byte_pos;
    GzHostTail tail(c, [&](uint8_t* dst, size_t cap) {
      const size_t n = std::min(cap, f.size() - at);
      memcpy(dst, f.data() + at, n);
      at += n;
      return n;
    });
    std::vector<uint8_t> got;
    if (read_all(tail, got, 65536) != -1 || tail.error().empty()) return fail("damage of kind " + std::to_string(kind) + " went unnoticed");
  }
  // from a member header (in_member 0) and from a trailer (want_trailer 1)
  {
    GzCarry c;
    size_t at = 0;
    GzHostTail tail(c, [&](uint8_t* dst, size_t cap) { const size_t n = std::min(cap, file.size() - at); memcpy(dst, file.data() + at, n); at += n; return n; });
    std::vector<uint8_t> got;
    if (read_all(tail, got, 4096) != 0 || got != want_rest_all) return fail("from the file's first byte");
    GzCarry t;
    t.byte_pos = (int64_t)one_member - 8;
    t.want_trailer = 1; t.in_member = 1;
    t.crc = (uint32_t)crc32(0, text.data(), (uInt)text.size());
    t.count = text.size();
    at = (size_t)t.byte_pos;
    GzHostTail tail2(t, [&](uint8_t* dst, size_t cap) { const size_t n = std::min(cap, file.size() - at); memcpy(dst, file.data() + at, n); at += n; return n; });
    got.clear();
    if (read_all(tail2, got, 4096) != 0 || got != second) return fail("from a trailer");
  }
  printf("resume ok: %d runs over %zu block ends, every bit offset\n", n_run, ends.size());
  return 0;
}

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "all";
  if ((what == "all" || what == "headers") && test_headers()) return 1;
  if ((what == "all" || what == "combine") && test_combine()) return 1;
  if ((what == "all" || what == "resume") && test_resume()) return 1;
  return 0;
}
