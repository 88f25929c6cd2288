// run_samples_parse.cpp -- test shim over csrc/run_samples.h: the list of `SVDSS run --samples LIST` as the binary reads it
// before it opens anything.
//   run_samples_parse LIST [INPUT ...]     INPUT: a path the run reads beside the BAMs of the list (FASTA, index, BED)
// stdout: "line<TAB>BAM<TAB>VCF<TAB>SFS" per sample (SFS empty where the line has two columns); a refusal: its message on
// stderr, exit 1.
#include <cstdio>
#include <string>
#include <vector>

#include "../../svdss_amd/csrc/run_samples.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<std::string> inputs;
  for (int i = 2; i < argc; ++i) inputs.push_back(argv[i]);
  std::vector<RunSample> samples;
  std::string err;
  if (!load_run_samples(argv[1], inputs, samples, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  for (const RunSample& s : samples) printf("%ld\t%s\t%s\t%s\n", s.line, s.bam.c_str(), s.vcf.c_str(), s.sfs.c_str());
  return 0;
}
