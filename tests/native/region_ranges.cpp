// region_ranges.cpp -- test shim over csrc/bam_region_ranges.h: the byte ranges of a BAM that an index names for regions.
//   region_ranges BAM INDEX tid:beg-end [tid:beg-end ...]     (0-based, half open; any order, may overlap)
// stdout: "begin<TAB>end<TAB>skip" per range (file offsets of BGZF members; skip: bytes into the first member).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../svdss_amd/csrc/bam_region_ranges.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  BaiIndex ix;
  if (!ix.load(argv[2])) { fprintf(stderr, "cannot load %s\n", argv[2]); return 1; }
  std::vector<std::pair<int32_t, std::pair<int32_t, int32_t>>> iv;
  for (int i = 3; i < argc; ++i) {
    int t; long b, e;
    if (sscanf(argv[i], "%d:%ld-%ld", &t, &b, &e) != 3) return 2;
    iv.push_back({t, {(int32_t)b, (int32_t)e}});
  }
  BamRegionSet U;
  U.assign((int32_t)ix.refs.size(), iv);
  std::vector<BamFileRange> r;
  std::string err;
  if (!region_file_ranges(argv[1], ix, U, r, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  for (const BamFileRange& x : r) printf("%zu\t%zu\t%lld\n", x.begin, x.end, (long long)x.skip);
  return 0;
}
