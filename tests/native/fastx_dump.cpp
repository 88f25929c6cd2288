// fastx_dump.cpp -- the records FastxReader (svdss_amd/csrc/fastx_reader.h) returns for a file, one per line: name, a tab,
// the sequence.  `fastx_dump FILE` reads the file as the binary does (gzopen); `fastx_dump FILE N` hands the reader the
// file's bytes through its memory source, cut into buffers of N bytes.  Built and run by tests/test_fastx_mirror.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>

#include "../../svdss_amd/csrc/fastx_reader.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::unique_ptr<FastxReader> fx;
  std::string bytes;
  size_t at = 0;
  if (argc > 2) {
    const size_t cut = (size_t)atoll(argv[2]);
    std::ifstream in(argv[1], std::ios::binary);
    bytes.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    fx.reset(new FastxReader([&bytes, &at, cut](std::string& buf) {
      if (at >= bytes.size()) return false;
      buf = bytes.substr(at, cut);
      at += buf.size();
      return true;
    }));
  } else {
    fx.reset(new FastxReader(argv[1]));
  }
  if (!fx->ok()) return 1;
  std::string name, seq;
  while (fx->next(name, seq)) {
    fwrite(name.data(), 1, name.size(), stdout);
    fputc('\t', stdout);
    fwrite(seq.data(), 1, seq.size(), stdout);
    fputc('\n', stdout);
  }
  return 0;
}
