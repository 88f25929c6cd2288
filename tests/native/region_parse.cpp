// region_parse.cpp -- test shim over csrc/bam_regions.h: the --region texts and the BED file of the command line against a
// list of reference names, as `SVDSS` resolves them before it opens anything.
//   region_parse NAMES [--bed FILE] [REG ...]     NAMES: a file, one reference name per line
// stdout: "tid<TAB>beg<TAB>end" per merged interval (0-based, half open); a refusal: its message on stderr, exit 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../svdss_amd/csrc/bam_regions.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<std::string> names, texts;
  std::string bed, line;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  for (int c; (c = fgetc(f)) != EOF;) {
    if (c == '\n') { names.push_back(line); line.clear(); } else line.push_back((char)c);
  }
  fclose(f);
  for (int i = 2; i < argc; ++i) {
    if (!strcmp(argv[i], "--bed") && i + 1 < argc) bed = argv[++i];
    else texts.push_back(argv[i]);
  }
  BamRegionSet U;
  std::string err;
  if (!resolve_regions(texts, bed, names, U, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  for (size_t k = 0; k < U.size(); ++k) printf("%d\t%d\t%d\n", U.tid[k], U.beg[k], U.end[k]);
  // the per-reference offsets must list the intervals by reference
  for (int32_t t = 0; t < U.n_ref; ++t)
    for (int64_t k = U.off[(size_t)t]; k < U.off[(size_t)t + 1]; ++k)
      if (U.tid[(size_t)k] != t) return 3;
  return 0;
}
