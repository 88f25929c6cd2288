// host_common.h -- what the host files of the binary (svdss_main.cpp, search_host.cpp, call_host.cpp, smooth_host.cpp) share:
// one logmsg / die / check, how an SVDSS_* variable is read, the number of GPUs a `--gpus N` comes to, and the chromosomes
// in BAM header order on a GPU.
// A file that defines SVDSS_LOG_TAG before it includes this header writes "[tag] [level] message" (`call`, `smooth`);
// without one the lines are the reference's (spdlog's default pattern with a time stamp: main.cpp, ping_pong.cpp).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/svdss_hip.h"

[[maybe_unused]] static void logmsg(const char* lvl, const std::string& m) {
#ifdef SVDSS_LOG_TAG
  fprintf(stderr, "[" SVDSS_LOG_TAG "] [%s] %s\n", lvl, m.c_str());
#else
  time_t t = time(nullptr);
  char ts[32];
  strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S", localtime(&t));
  fprintf(stderr, "[%s] [stderr] [%s] %s\n", ts, lvl, m.c_str());
#endif
}

// `SVDSS run --samples` (run_host.cpp): while a sample runs, a fatal message is prefixed by the sample's number and BAM, and
// the outputs it has begun (<path>.tmp) go with the process.  Empty for every other command: the messages are as they were.
struct DieContext { std::string prefix; std::vector<std::string> unlink; };
inline DieContext& die_context() { static DieContext c; return c; }

[[noreturn]] [[maybe_unused]] static void die(const std::string& m) {
  const DieContext& c = die_context();
  logmsg("critical", c.prefix + m);
  for (const std::string& p : c.unlink) (void)remove(p.c_str());
  exit(EXIT_FAILURE);
}

[[maybe_unused]] static void check(int rc, const char* what) {
  if (rc != SVDSS_OK) die(std::string(what) + ": " + svdss_strerror(rc) + " " + svdss_last_hip_error());
}

// --gpus N: the GPUs there are at most, one at least.  With the variable read here set (the tests' oversubscribe knob): N as
// asked, replica / shard / region d on GPU d % count -- the code path of N devices on a one-GPU box.
inline int effective_gpus(int requested) {
  return std::max(1, getenv("SVDSS_GPUS_OVERSUBSCRIBE") ? requested : std::min(requested, std::max(1, svdss_device_count())));
}

// an SVDSS_* variable: the value if it is set and at least `least` / if it is set, raised to `least` / -1 not set, 0 off, 1 on
inline int64_t env_from(const char* name, int64_t least, int64_t dflt) { const char* e = getenv(name); return e && atoll(e) >= least ? atoll(e) : dflt; }
inline int64_t env_raised(const char* name, int64_t least, int64_t dflt) { const char* e = getenv(name); return e ? std::max<int64_t>(least, atoll(e)) : dflt; }
inline int env_switch(const char* name) { const char* e = getenv(name); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }

// the header references the FASTA has, in header order: `has(name)` says whether it does; tid_map[t]: the place of header
// reference t among them, -1 where the FASTA has no such name
template <class Has>
inline std::vector<size_t> header_order(const std::vector<std::string>& ref_names, Has has, std::vector<int32_t>& tid_map) {
  std::vector<size_t> order;
  tid_map.assign(ref_names.size(), -1);
  for (size_t t = 0; t < ref_names.size(); ++t) {
    if (!has(ref_names[t])) continue;
    tid_map[t] = (int32_t)order.size();
    order.push_back(t);
  }
  return order;
}

// the chromosomes the BAM header names, in its order, one buffer on `device` (svdss_ref_upload_parts: no concatenation on
// the host); tid_map as header_order leaves it
inline int upload_chromosomes(const std::vector<std::string>& ref_names, const std::unordered_map<std::string, std::string>& seqs, int device,
                              std::vector<int32_t>& tid_map, svdss_ref_t** dref) {
  std::vector<const uint8_t*> parts;
  std::vector<int64_t> lens;
  for (const size_t t : header_order(ref_names, [&](const std::string& n) { return seqs.count(n) > 0; }, tid_map)) {
    const std::string& s = seqs.find(ref_names[t])->second;
    parts.push_back((const uint8_t*)s.data());
    lens.push_back((int64_t)s.size());
  }
  return svdss_ref_upload_parts(parts.data(), lens.data(), (int32_t)parts.size(), device, dref);
}
