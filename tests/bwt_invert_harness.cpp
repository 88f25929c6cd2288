// bwt_invert_harness.cpp -- the host driver of csrc/bwt_invert.h (the walker arithmetic, the step, the store packer and
// the chaining the GPU kernels of bwt_invert.hip share) over generated string collections and strides, as a program of
// its own for AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_bwt_invert_san.py builds and runs it).
//
//   bwt_invert_harness [seed]
// For every collection: the BWT with the sentinels in ropebwt's order (naive suffix sort), the rank blocks
// (svdss_blocks_from_bwt), then bwt_invert_host at every stride into a buffer that ends exactly where the heap block
// ends and starts 0..3 bytes off a word -- the strings must be the collection's, in order.  A BWT with a cycle that
// misses every sentinel must give SVDSS_EIO, a step limit of 5 SVDSS_ERANGE.  Exit 0 and "ok: ..." on success.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../include/svdss_hip.h"
#include "../svdss_amd/csrc/bwt_invert.h"
#include "../svdss_amd/csrc/index_host.h"
#include "../svdss_amd/csrc/rld0.h"

typedef std::vector<uint8_t> Str;

static std::vector<uint8_t> collection_bwt(const std::vector<Str>& strings) {
  const int64_t m = (int64_t)strings.size();
  std::vector<int64_t> t;   // symbols above every sentinel, $_i = i
  for (int64_t i = 0; i < m; ++i) {
    for (uint8_t c : strings[(size_t)i]) t.push_back((int64_t)c + m);
    t.push_back(i);
  }
  const int64_t n = (int64_t)t.size();
  std::vector<int64_t> sa((size_t)n);
  for (int64_t i = 0; i < n; ++i) sa[(size_t)i] = i;
  std::sort(sa.begin(), sa.end(), [&](int64_t a, int64_t b) {
    while (a < n && b < n) {   // (a sentinel is unique: the comparison ends there at the latest)
      if (t[(size_t)a] != t[(size_t)b]) return t[(size_t)a] < t[(size_t)b];
      ++a; ++b;
    }
    return a > b;
  });
  std::vector<uint8_t> bwt((size_t)n);
  for (int64_t r = 0; r < n; ++r) {
    const int64_t prev = t[(size_t)((sa[(size_t)r] + n - 1) % n)];
    bwt[(size_t)r] = prev < m ? 0 : (uint8_t)(prev - m);
  }
  return bwt;
}

static SvdssDevIndex view_of(const svdss_index& ix, int64_t n) {
  SvdssDevIndex v;
  memset(&v, 0, sizeof v);
  v.blocks = ix.blocks.data();
  v.dollar = ix.dollar.data();
  v.n = n;
  v.n_dollar = (int32_t)ix.dollar.size();
  memcpy(v.acc, ix.acc, sizeof v.acc);
  return v;
}

static int fail(const char* what, size_t coll, int64_t stride) {
  fprintf(stderr, "FAILED: %s (collection %zu, stride %lld)\n", what, coll, (long long)stride);
  return 1;
}

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
  auto rnd = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
  auto random_str = [&](int64_t len, int n_per_mille) {
    Str s((size_t)len);
    for (uint8_t& c : s) c = rnd(0, 999) < n_per_mille ? 5 : (uint8_t)rnd(1, 4);
    return s;
  };
  std::vector<std::vector<Str>> colls;
  colls.push_back({random_str(0, 0), random_str(1, 0), random_str(2, 0), random_str(127, 0), random_str(128, 0), random_str(129, 0), random_str(300, 0)});
  colls.push_back({Str(700, 1), random_str(40, 0)});                       // a run: LF is sequential
  colls.push_back({random_str(500, 200), Str(130, 5), random_str(60, 0)}); // N: the slow rank path
  { const Str s = random_str(200, 0); colls.push_back({s, random_str(30, 0), s}); }
  { std::vector<Str> many; for (int i = 0; i < 300; ++i) many.push_back(random_str(rnd(0, 12), 30)); colls.push_back(many); }
  colls.push_back({random_str(900, 0)});
  for (int k = 0; k < 6; ++k) {
    std::vector<Str> c;
    const int m = (int)rnd(1, 9);
    for (int i = 0; i < m; ++i) c.push_back(random_str(rnd(0, 400), k % 2 ? 50 : 0));
    colls.push_back(c);
  }
  const int64_t strides[] = {1, 2, 3, 5, 7, 8, 64, 4096, (int64_t)1 << 20};
  int64_t runs = 0;
  for (size_t ci = 0; ci < colls.size(); ++ci) {
    const std::vector<Str>& strings = colls[ci];
    const std::vector<uint8_t> bwt = collection_bwt(strings);
    const int64_t n = (int64_t)bwt.size(), m = (int64_t)strings.size();
    svdss_index ix;
    if (svdss_blocks_from_bwt(bwt.data(), n, 2, &ix) != SVDSS_OK) return fail("svdss_blocks_from_bwt", ci, 0);
    const SvdssDevIndex v = view_of(ix, n);
    Str want;
    for (const Str& s : strings) want.insert(want.end(), s.begin(), s.end());
    for (const int64_t stride : strides) {
      for (int shift = 0; shift < 4; ++shift) {
        // the output ends where the heap block ends, and begins `shift` bytes into it: a byte too many on either side is seen
        std::vector<uint8_t> buf((size_t)(shift + n - m));
        std::vector<int64_t> lens((size_t)m);
        const int rc = bwt_invert_host(v, stride, SVDSS_INVERT_MAX_STEPS_DEFAULT, 2, buf.data() + shift, lens.data());
        if (rc != SVDSS_OK) return fail("bwt_invert_host", ci, stride);
        for (int64_t r = 0; r < m; ++r)
          if (lens[(size_t)r] != (int64_t)strings[(size_t)r].size()) return fail("a string's length", ci, stride);
        if (n - m > 0 && memcmp(buf.data() + shift, want.data(), (size_t)(n - m)) != 0) return fail("the strings", ci, stride);
        ++runs;
      }
    }
    // the step limit
    if (n - m > 50) {
      std::vector<uint8_t> buf((size_t)(n - m));
      std::vector<int64_t> lens((size_t)m);
      if (bwt_invert_host(v, (int64_t)1 << 20, 5, 2, buf.data(), lens.data()) != SVDSS_ERANGE && m == 1) return fail("the step limit", ci, 0);
    }
    // one more row that maps to itself (a symbol T behind a BWT without N: LF(n) = n): no sentinel's walk reaches it
    bool has_n = false;
    for (uint8_t c : bwt) has_n = has_n || c == 5;
    if (!has_n) {
      std::vector<uint8_t> bad = bwt;
      bad.push_back(4);
      // (rows whose suffix starts with T stay where they are only if the new T row sorts last: T is the largest symbol)
      svdss_index bx;
      if (svdss_blocks_from_bwt(bad.data(), n + 1, 2, &bx) != SVDSS_OK) return fail("svdss_blocks_from_bwt (cycle)", ci, 0);
      const SvdssDevIndex bv = view_of(bx, n + 1);
      for (const int64_t stride : strides) {
        std::vector<uint8_t> buf((size_t)(n + 1 - m));
        std::vector<int64_t> lens((size_t)m);
        if (bwt_invert_host(bv, stride, SVDSS_INVERT_MAX_STEPS_DEFAULT, 2, buf.data(), lens.data()) != SVDSS_EIO) return fail("a cycle was not refused", ci, stride);
        ++runs;
      }
    }
  }
  printf("ok: %zu collections, %lld runs\n", colls.size(), (long long)runs);
  return 0;
}
