// The command line's own `--compress` (csrc/cli_options.h) for tests/test_cli_compress.py: parse_options on an argv,
// "compress=<0|1> threads=<n> bam=<text>" or "error: <text>" into out.
#include <cstdio>
#include <string>

#include "../../svdss_amd/csrc/cli_options.h"

extern "C" int compress_parse(int argc, char** argv, char* out, int cap) {
  Options o;
  std::string err;
  if (!parse_options(argc, argv, 1, o, err)) return snprintf(out, (size_t)cap, "error: %s", err.c_str());
  return snprintf(out, (size_t)cap, "compress=%d threads=%d bam=%s", o.compress, o.threads, o.bam.c_str());
}
