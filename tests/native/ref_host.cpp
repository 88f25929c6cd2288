// ref_host.cpp -- the host-only parts of the device reference loader, on their own so that they run under
// -fsanitize=address,undefined: the name lookup upload_chromosomes shares with svdss_ref_stream_finish (header_order,
// csrc/host_common.h) and the walk over the stream's segments that assembles a record (ref_pieces, csrc/ref_pieces.h).
// Reads "names of the BAM header | names of the FASTA | segment lengths | record ranges a:b ..." from its arguments and
// prints what the two compute; tests/test_ref_host_native.py holds the output against Python.
#include <cstdio>
#include <cstring>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../../svdss_amd/csrc/host_common.h"
#include "../../svdss_amd/csrc/ref_pieces.h"

struct Seg { int64_t start, n; std::vector<uint8_t> h; };

static std::vector<std::string> words(const char* s) {
  std::vector<std::string> out;
  std::istringstream in(s);
  for (std::string w; in >> w;) out.push_back(w == "-" ? std::string() : w);
  return out;
}

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: ref_host '<header names>' '<fasta names>' '<segment lengths>' '<a:b ...>'\n"); return 2; }
  const std::vector<std::string> header = words(argv[1]), fasta = words(argv[2]);
  const std::set<std::string> have(fasta.begin(), fasta.end());
  std::vector<int32_t> tid_map;
  const std::vector<size_t> order = header_order(header, [&](const std::string& n) { return have.count(n) > 0; }, tid_map);
  printf("order");
  for (size_t t : order) printf(" %zu", t);
  printf("\ntid_map");
  for (int32_t t : tid_map) printf(" %d", t);
  printf("\n");
  // segments filled with the bytes of one running counter: a record's bytes are then known from its range alone
  std::vector<Seg> segs;
  int64_t at = 0;
  for (const std::string& w : words(argv[3])) {
    const int64_t n = atoll(w.c_str());
    if (n <= 0) continue;                       // (empty batches leave no segment)
    Seg g{at, n, std::vector<uint8_t>((size_t)n)};
    for (int64_t i = 0; i < n; ++i) g.h[(size_t)i] = (uint8_t)((at + i) * 7 + 3);
    at += n;
    segs.push_back(std::move(g));
  }
  for (const std::string& w : words(argv[4])) {
    long long a = 0, b = 0;
    if (sscanf(w.c_str(), "%lld:%lld", &a, &b) != 2) return 2;
    std::vector<uint8_t> dst((size_t)(b > a ? b - a : 0));
    int pieces = 0;
    const bool ok = ref_pieces(segs, a, b, [&](const Seg& g, int64_t from, int64_t n, int64_t to) {
      memcpy(dst.data() + to, g.h.data() + from, (size_t)n);
      ++pieces;
      return true;
    });
    bool same = ok;
    for (int64_t i = a; i < b && same; ++i) same = dst[(size_t)(i - a)] == (uint8_t)(i * 7 + 3);
    printf("range %lld:%lld %s pieces %d\n", a, b, !ok ? "uncovered" : same ? "ok" : "WRONG", pieces);
  }
  return 0;
}
