// ref_pieces.h -- the output of the reference stream (csrc/ref_stream.hip) lies in segments, one per batch, in file order:
// out[start, start + n) each, empty batches left out.  A record is a range of the output: ref_pieces walks the segments that
// hold it.  Host code alone (tests/native/ref_host.cpp runs it under the sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

// f(segment, first byte within it, bytes, offset within [a, b)) for the segments that hold out[a, b), in order; false: f
// said so, or the segments do not cover the range
template <class Seg, class F>
bool ref_pieces(const std::vector<Seg>& segs, int64_t a, int64_t b, F f) {
  auto it = std::upper_bound(segs.begin(), segs.end(), a, [](int64_t v, const Seg& g) { return v < g.start; });
  if (it != segs.begin()) --it;
  int64_t at = a;
  for (; it != segs.end() && at < b; ++it) {
    if (it->start > at) return false;
    if (it->start + it->n <= at) continue;
    const int64_t n = std::min(b, it->start + it->n) - at;
    if (!f(*it, at - it->start, n, at - a)) return false;
    at += n;
  }
  return at >= b;
}
