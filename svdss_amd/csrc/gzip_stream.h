// gzip_stream.h -- the host side of csrc/gzip_stream.hip (plain single-stream gzip inflated chunk-parallel on the device):
// what is decided before the kernels run and after the unit declines.  Plain C++ and zlib, no HIP:
//   * gz_parse_header       the gzip member header (RFC 1952): complete, not complete yet, or not one;
//   * gz_crc32_combine      the CRC32 of a concatenation from the CRC32s of its parts (GF(2) matrix method), which joins
//                           the CRCs the resolve kernel gives per piece of text;
//   * GzCarry               what the unit carries between windows and hands over when it declines;
//   * GzHostTail            the hand-over: zlib raw inflate from exactly that state (bit position primed, dictionary set) to
//                           the member's end, its trailer checked against the carried CRC32 and byte count, further members
//                           as gzread reads them (bytes that are no gzip header end the input silently).
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

// The gzip member header at b[0 .. n): its length; 0 = what is there fits but the header is not complete; -1 = not a header
// (wrong magic, a method other than deflate, reserved flag bits).  MTIME, XFL, OS, FEXTRA, FNAME, FCOMMENT and FHCRC are skipped.
inline int64_t gz_parse_header(const uint8_t* b, int64_t n) {
  static const uint8_t magic[3] = {0x1f, 0x8b, 8};
  for (int i = 0; i < 3; ++i)
    if (n > i && b[i] != magic[i]) return -1;
  if (n < 10) return 0;
  const uint8_t flg = b[3];
  if (flg & 0xe0) return -1;
  int64_t p = 10;
  if (flg & 4) {
    if (n < p + 2) return 0;
    p += 2 + (int64_t)b[p] + 256 * (int64_t)b[p + 1];
  }
  for (int bit = 8; bit <= 16; bit <<= 1)
    if (flg & bit) {
      for (;;) {
        if (p >= n) return 0;
        if (b[p++] == 0) break;
      }
    }
  if (flg & 2) p += 2;
  return p <= n ? p : 0;
}

// ---- crc32_combine, the GF(2) matrix method: appending len2 zero bytes to a message multiplies its CRC register by a
// 32 x 32 matrix over GF(2); the matrix for one zero bit is squared up to the bytes of len2
namespace gz_detail {
inline uint32_t gf2_times(const uint32_t* mat, uint32_t vec) {
  uint32_t sum = 0;
  for (; vec; vec >>= 1, ++mat)
    if (vec & 1u) sum ^= *mat;
  return sum;
}
inline void gf2_square(uint32_t* square, const uint32_t* mat) {
  for (int n = 0; n < 32; ++n) square[n] = gf2_times(mat, mat[n]);
}
}  // namespace gz_detail
inline uint32_t gz_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
  if (len2 == 0) return crc1;
  uint32_t even[32], odd[32];
  odd[0] = 0xedb88320u;                       // the operator for one zero bit
  for (int n = 1; n < 32; ++n) odd[n] = 1u << (n - 1);
  gz_detail::gf2_square(even, odd);           // two zero bits
  gz_detail::gf2_square(odd, even);           // four
  do {                                        // (the first squaring below gives the operator for one zero byte)
    gz_detail::gf2_square(even, odd);
    if (len2 & 1) crc1 = gz_detail::gf2_times(even, crc1);
    len2 >>= 1;
    if (!len2) break;
    gz_detail::gf2_square(odd, even);
    if (len2 & 1) crc1 = gz_detail::gf2_times(odd, crc1);
    len2 >>= 1;
  } while (len2);
  return crc1 ^ crc2;
}

// What the unit carries from window to window, and reports when it declines: where the stream stands (the byte of the file
// and the bit in it; the next thing there is a block header, a member's trailer or a member header), the text in front of
// it that matches may still reach, and the member's running CRC32 and byte count.
struct GzCarry {
  int64_t byte_pos = 0;        // of the file
  int32_t bit = 0;             // 0..7, within that byte
  int32_t in_member = 0;       // 1: inside a member's deflate stream; 0: at a member header (or the end of the file)
  int32_t want_trailer = 0;    // 1: at a member's CRC32 / ISIZE
  uint32_t crc = 0;            // of the member's text so far
  uint64_t count = 0;          // bytes of it
  uint32_t dict_len = 0;       // valid bytes at the END of dict
  uint8_t dict[32768];
  const uint8_t* dict_data() const { return dict + (32768 - dict_len); }
};

// The host's part behind a decline.  `read` hands over the file's bytes from carry.byte_pos on (any number per call, 0 =
// the end); next() gives text until it returns 0 (the end) or -1 (error() says what is wrong with the stream).
class GzHostTail {
 public:
  using Read = std::function<size_t(uint8_t*, size_t)>;
  GzHostTail(const GzCarry& c, Read read) : read_(std::move(read)), in_((size_t)1 << 20), crc_(c.crc), count_(c.count) {
    memset(&z_, 0, sizeof z_);
    if (c.want_trailer) { state_ = TRAILER; return; }
    if (!c.in_member) { state_ = BETWEEN; return; }
    if (inflateInit2(&z_, -15) != Z_OK) { fail("zlib: inflateInit2"); return; }
    live_ = true;
    state_ = RAW;
    if (c.dict_len && inflateSetDictionary(&z_, c.dict_data(), c.dict_len) != Z_OK) { fail("zlib: inflateSetDictionary"); return; }
    if (c.bit) {
      // the bits of the first byte from the carried one on go in through inflatePrime; the stream proper starts behind it
      uint8_t first;
      if (!fill() || avail_ == 0) { fail("truncated stream"); return; }
      first = in_[at_++];
      --avail_;
      if (inflatePrime(&z_, 8 - c.bit, first >> c.bit) != Z_OK) fail("zlib: inflatePrime");
    }
  }
  ~GzHostTail() { if (live_) inflateEnd(&z_); }
  GzHostTail(const GzHostTail&) = delete;
  GzHostTail& operator=(const GzHostTail&) = delete;
  const std::string& error() const { return err_; }

  int64_t next(uint8_t* out, size_t cap) {
    while (state_ != DONE && state_ != FAILED) {
      if (state_ == TRAILER) {
        uint8_t t[8];
        for (int i = 0; i < 8; ++i) {
          if (!fill() || avail_ == 0) return fail("truncated trailer");
          t[i] = in_[at_++];
          --avail_;
        }
        const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (crc != crc_) return fail("CRC32 mismatch");
        if (isize != (uint32_t)count_) return fail("ISIZE mismatch");
        state_ = BETWEEN;
        continue;
      }
      if (state_ == BETWEEN) {
        // another member, the end of the file, or bytes that are no header: gzread ignores those
        if (live_) { inflateEnd(&z_); live_ = false; }
        uint8_t m[2];
        size_t got = 0;
        while (got < 2 && fill() && avail_) { m[got++] = in_[at_]; if (got < 2) { ++at_; --avail_; } }
        if (got < 2 || m[0] != 0x1f || m[1] != 0x8b) { state_ = DONE; break; }
        // (the second magic byte is still in the buffer; zlib gets the first one back through a two-byte prefix)
        memset(&z_, 0, sizeof z_);
        if (inflateInit2(&z_, 15 + 16) != Z_OK) return fail("zlib: inflateInit2");
        live_ = true;
        prefix_[0] = 0x1f;
        use_prefix_ = true;
        state_ = WRAPPED;
        continue;
      }
      // RAW or WRAPPED: inflate
      if (use_prefix_) {
        z_.next_in = prefix_;
        z_.avail_in = 1;
      } else {
        if (avail_ == 0 && !fill()) { /* zlib decides below: no input and no progress is a truncated stream */ }
        z_.next_in = in_.data() + at_;
        z_.avail_in = (uInt)avail_;
      }
      z_.next_out = out;
      z_.avail_out = (uInt)cap;
      const bool had_input = z_.avail_in > 0;
      const int rc = inflate(&z_, Z_NO_FLUSH);
      if (use_prefix_) { if (z_.avail_in == 0) use_prefix_ = false; }
      else { at_ += avail_ - z_.avail_in; avail_ = z_.avail_in; }
      const size_t n = cap - z_.avail_out;
      if (rc != Z_OK && rc != Z_STREAM_END && rc != Z_BUF_ERROR) return fail(z_.msg ? std::string("zlib: ") + z_.msg : "zlib: damaged stream");
      if (state_ == RAW) { crc_ = (uint32_t)crc32(crc_, out, (uInt)n); count_ += n; }
      if (rc == Z_STREAM_END) state_ = state_ == RAW ? TRAILER : BETWEEN;   // (windowBits 31: zlib checked the trailer)
      else if (n == 0 && !had_input && eof_) return fail("truncated stream");
      if (n) return (int64_t)n;
    }
    return state_ == FAILED ? -1 : 0;
  }

 private:
  enum State { RAW, TRAILER, BETWEEN, WRAPPED, DONE, FAILED };
  int64_t fail(const std::string& why) { err_ = why; state_ = FAILED; return -1; }
  bool fill() {       // true: avail_ > 0, or the end was reached (avail_ == 0)
    if (avail_ > 0) return true;
    if (eof_) return true;
    at_ = 0;
    avail_ = read_(in_.data(), in_.size());
    if (avail_ == 0) eof_ = true;
    return true;
  }
  Read read_;
  std::vector<uint8_t> in_;
  size_t at_ = 0, avail_ = 0;
  bool eof_ = false, live_ = false, use_prefix_ = false;
  uint8_t prefix_[2] = {0, 0};
  z_stream z_;
  State state_ = DONE;
  uint32_t crc_;
  uint64_t count_;
  std::string err_;
};
