// aln_band_dump.cpp -- the planner of the realignment's diagonal bands (svdss_amd/csrc/aln_band.h) behind a C interface for
// tests/aln_band_lib.py.  g++ only: the header has no HIP in it.  Test infrastructure only.
#include <cstdint>
#include <vector>

#include "../../svdss_amd/csrc/aln_band.h"

// gaps: q, e, q2, e2.  out: lo, hi, c1, c2, mode, S_lb, x (where S_lb's gap run sits), provable, M, steps, full steps
extern "C" void aln_band_plan_c(const uint8_t* q, int64_t ql, const uint8_t* t, int64_t tl, int m, const int8_t* mat, const int32_t* gaps,
                                int level, int64_t* out) {
  const AlnScoring s{m, mat, gaps[0], gaps[1], gaps[2], gaps[3]};
  std::vector<int32_t> scratch;
  int64_t slb = 0, x = 0, full = 0;
  int M = 0;
  const AlnBand b = aln_band_plan(q, ql, t, tl, s, level, scratch, &slb, &x);
  const bool ok = aln_band_provable(s, &M);
  const int64_t steps = aln_band_steps(ql, tl, b, &full);
  const int64_t v[11] = {b.lo, b.hi, b.c1, b.c2, b.mode, slb, x, ok, M, steps, full};
  for (int k = 0; k < 11; ++k) out[k] = v[k];
}

extern "C" int64_t aln_band_f_c(int64_t d, int64_t ql, int64_t tl, int m, const int8_t* mat, const int32_t* gaps) {
  const AlnScoring s{m, mat, gaps[0], gaps[1], gaps[2], gaps[3]};
  int M = 0;
  aln_band_provable(s, &M);
  return aln_band_f(d, ql, tl, M, s);
}

extern "C" int aln_band_live_c(int d, const int32_t* band) {
  const AlnBand b{band[0], band[1], band[2], band[3], band[4]};
  return aln_band_live(d, b) ? 1 : 0;
}

// out: a0, e0, a1, e1
extern "C" void aln_band_stripe_c(int ql, int tl, int s, const int32_t* band, int32_t* out) {
  const AlnBand b{band[0], band[1], band[2], band[3], band[4]};
  const AlnStripeSteps r = aln_band_stripe_steps(ql, tl, s, b);
  out[0] = r.a[0]; out[1] = r.e[0]; out[2] = r.a[1]; out[3] = r.e[1];
}

// the planning of a whole batch, timed by the caller: what svdss_align_global_batch does before its upload
extern "C" int64_t aln_band_plan_batch_c(const uint8_t* q, const int64_t* q_off, const uint8_t* t, const int64_t* t_off, int64_t n, int m,
                                         const int8_t* mat, const int32_t* gaps, int level) {
  const AlnScoring s{m, mat, gaps[0], gaps[1], gaps[2], gaps[3]};
  std::vector<int32_t> scratch;
  int64_t steps = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t ql = q_off[i + 1] - q_off[i], tl = t_off[i + 1] - t_off[i];
    const AlnBand b = aln_band_plan(q + q_off[i], ql, t + t_off[i], tl, s, level, scratch);
    steps += aln_band_steps(ql, tl, b);
  }
  return steps;
}
