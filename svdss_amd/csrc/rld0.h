// rld0.h -- ropebwt3's `.fmd` (rld0, magic "RLD\3") export / import; see rld0.cpp.
#pragma once
#include <stdint.h>

#include <vector>

struct svdss_index;

bool rld0_is_fmd(const char* path);
// BWT symbols 0..5 -> file; SVDSS_OK / SVDSS_EINVAL / SVDSS_EIO
int rld0_write(const char* path, const uint8_t* bwt, int64_t n);
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
