// run_samples.h -- `SVDSS run --samples LIST`: the list of samples, one per line, tab-separated: BAM<TAB>VCF[<TAB>SFS].
//
// The rules, in one place: lines end at '\n', one '\r' in front of it is dropped; a line that is empty then, or starts with
// '#', is skipped; every other line is split at EVERY tab -- nothing is trimmed, so a path may hold spaces -- into two or
// three columns, none of them empty (a trailing tab makes an empty column).  Samples keep the order of their lines.
// Two lines may name the same BAM; no two outputs (VCF or SFS, of any line) may be the same path, and no output may be a
// path the run reads (a BAM of the list, and whatever else the caller names: FASTA, index, the list itself, the BED).
// Paths are compared as texts.
// No HIP, no library: tests compile this header alone (tests/native/run_samples_parse.cpp).
#pragma once
#include <cstdio>
#include <set>
#include <string>
#include <vector>

struct RunSample {
  std::string bam, vcf, sfs;   // sfs: empty where the line has two columns
  long line = 0;               // 1-based line of the list
};

// the text of a list into samples; false and a message that names the line
inline bool parse_run_samples_text(const std::string& text, const std::string& list_name, std::vector<RunSample>& out, std::string& err) {
  out.clear();
  long n_line = 0;
  for (size_t at = 0; at < text.size();) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    std::string line = text.substr(at, nl - at);
    at = nl + 1;
    ++n_line;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    const std::string where = "--samples " + list_name + " line " + std::to_string(n_line) + ": ";
    std::vector<std::string> cols;
    for (size_t c0 = 0;;) {
      const size_t tab = line.find('\t', c0);
      cols.push_back(line.substr(c0, tab == std::string::npos ? tab : tab - c0));
      if (tab == std::string::npos) break;
      c0 = tab + 1;
    }
    if (cols.size() < 2) { err = where + "fewer than two tab-separated columns (BAM<TAB>VCF[<TAB>SFS])"; return false; }
    if (cols.size() > 3) { err = where + "more than three tab-separated columns (BAM<TAB>VCF[<TAB>SFS])"; return false; }
    for (size_t k = 0; k < cols.size(); ++k)
      if (cols[k].empty()) { err = where + "column " + std::to_string(k + 1) + " is empty"; return false; }
    RunSample s;
    s.bam = cols[0]; s.vcf = cols[1]; s.sfs = cols.size() == 3 ? cols[2] : "";
    s.line = n_line;
    out.push_back(s);
  }
  if (out.empty()) { err = "--samples " + list_name + ": no sample in the list"; return false; }
  return true;
}

// the outputs against each other and against what the run reads (`inputs`: beside the BAMs of the list)
inline bool check_run_samples_paths(const std::vector<RunSample>& samples, const std::vector<std::string>& inputs, const std::string& list_name, std::string& err) {
  std::set<std::string> reads(inputs.begin(), inputs.end()), writes;
  for (const RunSample& s : samples) reads.insert(s.bam);
  for (const RunSample& s : samples)
    for (const std::string* p : {&s.vcf, &s.sfs}) {
      if (p->empty()) continue;
      const std::string where = "--samples " + list_name + " line " + std::to_string(s.line) + ": ";
      if (reads.count(*p)) { err = where + "the output " + *p + " is an input of the run"; return false; }
      if (!writes.insert(*p).second) { err = where + "the output " + *p + " is named twice"; return false; }
    }
  return true;
}

// the file at `path` through the two above; a list that cannot be read is refused like one without a sample
inline bool load_run_samples(const std::string& path, const std::vector<std::string>& inputs, std::vector<RunSample>& out, std::string& err) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { err = "--samples " + path + ": cannot read the list"; return false; }
  std::string text;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) { err = "--samples " + path + ": cannot read the list"; return false; }
  std::vector<std::string> in = inputs;
  in.push_back(path);
  return parse_run_samples_text(text, path, out, err) && check_run_samples_paths(out, in, path, err);
}
