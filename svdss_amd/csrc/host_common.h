// host_common.h -- what the host files of the binary (svdss_main.cpp, search_host.cpp, call_host.cpp, smooth_host.cpp) share:
// one logmsg / die / check, and the number of GPUs a `--gpus N` comes to.
// A file that defines SVDSS_LOG_TAG before it includes this header writes "[tag] [level] message" (`call`, `smooth`);
// without one the lines are the reference's (spdlog's default pattern with a time stamp: main.cpp, ping_pong.cpp).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <string>

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

[[noreturn]] [[maybe_unused]] static void die(const std::string& m) {
  logmsg("critical", m);
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
