// The command line's own `--nobam` (csrc/cli_options.h) for tests/test_smooth_sfs_cli.py: parse_options on an argv,
// "nobam=<0|1> index=<text> sfs=<text> bsize=<n> putative=<0|1> assemble=<0|1>" or "error: <text>" into out.
#include <cstdio>
#include <string>

#include "../../svdss_amd/csrc/cli_options.h"

extern "C" int nobam_parse(int argc, char** argv, char* out, int cap) {
  Options o;
  std::string err;
  if (!parse_options(argc, argv, 1, o, err)) return snprintf(out, (size_t)cap, "error: %s", err.c_str());
  return snprintf(out, (size_t)cap, "nobam=%d index=%s sfs=%s bsize=%d putative=%d assemble=%d", o.nobam ? 1 : 0, o.index.c_str(), o.sfs.c_str(), o.bsize,
                  o.putative ? 1 : 0, o.assemble ? 1 : 0);
}
