// rld0.h -- ropebwt3's `.fmd` (rld0, magic "RLD\3") export / import; see rld0.cpp.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

struct svdss_index;

bool rld0_is_fmd(const char* path);
// BWT symbols 0..5 -> file; SVDSS_OK / SVDSS_EINVAL / SVDSS_EIO
int rld0_write(const char* path, const uint8_t* bwt, int64_t n);
// the rank frames from the block headers of the data words, fed in slices (rld0.cpp); the file's header
struct Rld0Frames {
  std::vector<uint64_t> frame;
  uint64_t n_frames = 0, fk = 1, cnt[6] = {0, 0, 0, 0, 0, 0};
  int64_t last = 0;
  int ibits = 0;
  void begin(uint64_t total, int64_t k);
  void feed(const uint64_t* z, int64_t first_word, int64_t n_words);
  void finish();
};
bool rld0_write_header(FILE* f, int64_t k, uint64_t n_frames, const uint64_t mcnt[6]);
// rld0_dev.hip, the encoder on the device: the .fmd of the BWT behind rank blocks resident on the current device / on the
// host (uploaded to `device`).  SVDSS_OK: written there; -(SVDSS_FMD_DECLINED_*): declined, nothing written; else an error
int rld0_dev_encode(const void* d_blocks, int64_t n, const int64_t acc[7], const char* path);
int rld0_dev_encode_host_blocks(const svdss_index* ix, int device, const char* path);
// what svdss_fmd_encode_last reports after the HOST encoder wrote a file: why it did (SVDSS_FMD_HOST, SVDSS_FMD_DECLINED_*)
void rld0_encode_note(int32_t route, double total_ms);
// the header's occurrence count of every symbol (cheap: 72 bytes read)
int rld0_header_counts(const char* path, uint64_t mcnt_out[6]);
// file -> BWT symbols
int rld0_read(const char* path, std::vector<uint8_t>& bwt);
// rank blocks, acc and '$' rows of a BWT into *ix (text and suffix array stay empty)
int svdss_blocks_from_bwt(const uint8_t* bwt, int64_t n, int threads, svdss_index* ix);
// the strings of the collection (LF walks from the sentinel rows), in sentinel order
int rld0_strings_of_bwt(const uint8_t* bwt, int64_t n, int threads, std::vector<std::vector<uint8_t>>& out);
// indices of one string of every reverse-complement pair; SVDSS_EIO if the collection is not closed under it
int rld0_pick_strands(std::vector<std::vector<uint8_t>>& strings, std::vector<int64_t>& picked);
// '$' of a BWT counted; SVDSS_EINVAL for a symbol above 5
int rld0_count_sentinels(const uint8_t* bwt, int64_t n, int threads, int64_t* m);
// the strings by MARKED LF walks on the host (bwt_invert.h: the host driver of what bwt_invert.hip runs on a device), written
// back to back into out (n - m bytes), lengths into lens (m); ms[3]: milliseconds of the rank blocks' build, pass 1, pass 2
int rld0_strings_marked(const uint8_t* bwt, int64_t n, int64_t stride, int64_t max_steps, int threads, uint8_t* out, int64_t* lens, double ms[3]);
