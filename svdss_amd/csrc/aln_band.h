// aln_band.h -- which cells of a realignment matrix an optimal alignment can cross, decided before the launch
// (align_wave_kernel, call_dp.hip).  No HIP in it: tests/native/aln_band_dump.cpp builds it with g++.
//
// Cell (i, j): i indexes the target, j the query; diagonal d = j - i.  A global alignment starts on diagonal 0 and ends
// on diagonal D = ql - tl.  g(0) = 0, g(k) = min(q + k e, q2 + k e2) is what one gap run of k costs.
//
//   S_lb   the score of an alignment that exists: the plain diagonal for D = 0, else the best single gap run of |D|
//          (prefix on diagonal 0 + suffix on diagonal D - g(|D|), the gap anywhere from the first to the last column).
//   f(d) = M min(ql, tl) - g(|d|) - g(|D - d|), M the largest matrix entry: no alignment that is in match state on
//          diagonal d, or starts or ends a gap run there, scores more.  (It has at most min(ql, tl) match columns of at
//          most M each, M > 0, and its gap runs move it from diagonal 0 to d and from d to D: with q, e, q2, e2 >= 0, g
//          does not decrease and is subadditive, g(a) + g(b) >= g(a + b), so these runs cost at least g(|d|) + g(|D - d|).)
//   live   {d : f(d) >= S_lb}.  f(0) = f(D) >= S_lb always; f falls away outside [0, D] (taking D > 0) and -f is concave
//          between: the live set is [lo, c1] + [c2, hi] with lo <= 0 <= c1, c2 <= D <= hi, or one interval.
//
// Tier 1 computes the hull [lo, hi] only.  Tier 2 also leaves out a dead interior (c1, c2) of ALN_BAND_MIN_DEAD diagonals
// or more: an optimal alignment is never in match state there and never starts or ends a gap run there, so it crosses the
// interior in ONE gap run -- horizontal (along the query) for D > 0, vertical for D < 0.  (One that crossed it the other way
// would have to come back: match state on some b >= c2, then on some a <= c1, then D; its runs cost at least
// g(b) + g(b - a) + g(D - a) >= g(c1 + 1) + g(D - c1 - 1) + g(b - a), which puts it below f(c1 + 1) < S_lb.)
//
// Why the pruned matrix gives the same score and the same CIGAR, bit for bit.  A pruned cell hands on "no path", so every
// value the kernel computes is the exact one or an under-estimate.  Take a cell on the path ksw2's backtrack follows: that
// path is optimal, so in match state and where its gap runs start and end it is on live diagonals, and inside a gap run
// within the hull or crossing the dead interior as above, where the run's value is carried in closed form (- e per cell).
// By induction along the path the candidate that wins a comparison there is exact; a losing candidate is exact or
// under-estimated and still loses, and one that ties lies on an optimal path itself and is therefore exact: no comparison
// the backtrack consults can come out differently.  Parameters outside the proof's conditions plan the full matrix.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define ALN_HD __host__ __device__
#else
#define ALN_HD
#endif

#define ALN_BAND_MIN_DEAD 128   // the lanes of one step span 127 diagonals: a narrower interior never empties a step

enum { ALN_FULL = 0, ALN_ONE_BAND = 1, ALN_CARRY = 2 };

// live diagonals of a pair: [lo, c1] and [c2, hi] within [-tl, ql]; ALN_ONE_BAND and ALN_FULL have c1 = hi, c2 = hi + 1
struct AlnBand {
  int32_t lo, hi, c1, c2;
  int32_t mode;
};

struct AlnScoring {
  int m;
  const int8_t* mat;   // m x m, row = target symbol
  int q, e, q2, e2;
};

inline int64_t aln_gap(int64_t k, const AlnScoring& s) {
  if (k <= 0) return 0;
  const int64_t a = s.q + k * s.e, b = s.q2 + k * s.e2;
  return a < b ? a : b;
}

inline AlnBand aln_band_full(int64_t ql, int64_t tl) {
  AlnBand b;
  b.lo = (int32_t)-tl;
  b.hi = (int32_t)ql;
  b.c1 = b.hi;
  b.c2 = b.hi + 1;
  b.mode = ALN_FULL;
  return b;
}

// true where the bound is proven: a positive largest entry, no negative gap cost
inline bool aln_band_provable(const AlnScoring& s, int* M_out) {
  int M = -128;
  for (int k = 0; k < s.m * s.m; ++k) M = s.mat[k] > M ? s.mat[k] : M;
  *M_out = M;
  return M > 0 && s.q >= 0 && s.e >= 0 && s.q2 >= 0 && s.e2 >= 0;
}

// f(d) of the header comment; M the largest matrix entry
inline int64_t aln_band_f(int64_t d, int64_t ql, int64_t tl, int M, const AlnScoring& s) {
  const int64_t D = ql - tl;
  return (int64_t)M * (ql < tl ? ql : tl) - aln_gap(d < 0 ? -d : d, s) - aln_gap(D - d < 0 ? d - D : D - d, s);
}

// S_lb and the query column x in front of which its gap run sits (0 for ql == tl): columns / rows [x, x + |D|) are the gap.
// `pre` is scratch of min(ql, tl) + 1 entries.
inline int64_t aln_band_slb(const uint8_t* q, int64_t ql, const uint8_t* t, int64_t tl, const AlnScoring& s, int64_t* x_out,
                            std::vector<int32_t>& pre) {
  const int64_t n = ql < tl ? ql : tl, D = ql - tl, k = D < 0 ? -D : D;
  const int64_t qs = D > 0 ? D : 0, ts = D < 0 ? -D : 0;   // where the suffix diagonal starts
  pre.resize((size_t)n + 1);
  int32_t acc = 0;
  pre[0] = 0;
  for (int64_t x = 0; x < n; ++x) { acc += s.mat[t[x] * s.m + q[x]]; pre[(size_t)x + 1] = acc; }
  if (D == 0) { *x_out = 0; return acc; }
  // the gap in front of position x = n, n - 1, ..., 0: prefix [0, x) on diagonal 0, suffix [x, n) on diagonal D
  int64_t best = pre[(size_t)n], best_x = n;
  int32_t suf = 0;
  for (int64_t x = n - 1; x >= 0; --x) {
    suf += s.mat[t[x + ts] * s.m + q[x + qs]];
    const int64_t v = (int64_t)pre[(size_t)x] + suf;
    if (v >= best) { best = v; best_x = x; }
  }
  *x_out = best_x;
  return best - aln_gap(k, s);
}

// the plan of one pair from its S_lb.  level 0: the full matrix; 1: the hull; 2: the hull without a dead interior.
// (the library has the two diagonal sums of S_lb from a kernel, aln_slb_kernel, and plans from here)
inline AlnBand aln_band_plan_slb(int64_t ql, int64_t tl, const AlnScoring& s, int level, int64_t slb) {
  AlnBand b = aln_band_full(ql, tl);
  int M = 0;
  if (level <= 0 || ql <= 0 || tl <= 0 || !aln_band_provable(s, &M)) return b;
  const int64_t D = ql - tl;
  const int64_t h0 = D < 0 ? D : 0, h1 = D < 0 ? 0 : D;   // the humps, left and right
  auto f = [&](int64_t d) { return aln_band_f(d, ql, tl, M, s); };
  int64_t lo = h0, hi = h1, c1 = h0, c2 = h1;
  // (as far as -tl and ql: the diagonals of the border cells (tl - 1, -1) and (-1, ql - 1), where an alignment that is
  // all gap turns from one run into the other)
  while (lo - 1 >= -tl && f(lo - 1) >= slb) --lo;
  while (hi + 1 <= ql && f(hi + 1) >= slb) ++hi;
  while (c1 + 1 < h1 && f(c1 + 1) >= slb) ++c1;
  while (c2 - 1 > c1 && f(c2 - 1) >= slb) --c2;
  b.lo = (int32_t)lo;
  b.hi = (int32_t)hi;
  if (level >= 2 && c2 - c1 - 1 >= ALN_BAND_MIN_DEAD) {
    b.c1 = (int32_t)c1;
    b.c2 = (int32_t)c2;
    b.mode = ALN_CARRY;
  } else {
    b.c1 = b.hi;
    b.c2 = b.hi + 1;
    b.mode = ALN_ONE_BAND;
  }
  return b;
}

// the plan of one pair, S_lb computed here
inline AlnBand aln_band_plan(const uint8_t* q, int64_t ql, const uint8_t* t, int64_t tl, const AlnScoring& s, int level,
                             std::vector<int32_t>& scratch, int64_t* slb_out = nullptr, int64_t* x_out = nullptr) {
  int M = 0;
  int64_t x = 0, slb = 0;
  if (level > 0 && ql > 0 && tl > 0 && aln_band_provable(s, &M)) slb = aln_band_slb(q, ql, t, tl, s, &x, scratch);
  if (slb_out) *slb_out = slb;
  if (x_out) *x_out = x;
  return aln_band_plan_slb(ql, tl, s, level, slb);
}

ALN_HD inline bool aln_band_live(int d, const AlnBand& b) {
  return (unsigned)(d - b.lo) <= (unsigned)(b.hi - b.lo) && !((unsigned)(d - b.c1 - 1) < (unsigned)(b.c2 - b.c1 - 1));
}

// The wavefront steps stripe s (target rows 64 s ...) executes: [a[0], e[0]) and, after a jump, [a[1], e[1]) (empty
// unless the pair carries a gap).  Lane l computes column tau - l of row 64 s + l at step tau, diagonal tau - 64 s - 2 l:
// the steps in which some lane's cell is in a live interval, the start rounded down to the kernel's blocks of 64 columns.
// A jump skips at least two steps (what a lane reads from two steps back is then "no path" as well).
struct AlnStripeSteps { int a[2], e[2]; };
ALN_HD inline AlnStripeSteps aln_band_stripe_steps(int ql, int tl, int s, const AlnBand& b) {
  const int i0 = s << 6, rows = tl - i0 < 64 ? tl - i0 : 64, n_steps = ql + rows - 1;
  AlnStripeSteps r;
  r.a[1] = r.e[1] = n_steps;
  if (b.mode == ALN_FULL) { r.a[0] = 0; r.e[0] = n_steps; return r; }
  const int64_t spread = 2 * (rows - 1) + 1;
  const bool two = b.mode == ALN_CARRY;
  int64_t a0 = (int64_t)b.lo + i0, e0 = (int64_t)(two ? b.c1 : b.hi) + i0 + spread;
  a0 = a0 < 0 ? 0 : a0 & ~(int64_t)63;
  e0 = e0 < 0 ? 0 : e0 > n_steps ? n_steps : e0;
  if (a0 > e0) a0 = e0;
  r.a[0] = (int)a0; r.e[0] = (int)e0;
  if (two) {
    int64_t a1 = (int64_t)b.c2 + i0, e1 = (int64_t)b.hi + i0 + spread;
    a1 = a1 < 0 ? 0 : a1 & ~(int64_t)63;
    if (e1 > n_steps) e1 = n_steps;
    if (a1 < e1) {
      if (a1 < e0 + 2) r.e[0] = (int)e1;                      // no room to jump: one range
      else { r.a[1] = (int)a1; r.e[1] = (int)e1; }
    }
  }
  return r;
}

// steps the kernel executes for the pair, and those of its full matrix
inline int64_t aln_band_steps(int64_t ql, int64_t tl, const AlnBand& b, int64_t* full_out = nullptr) {
  int64_t steps = 0, full = 0;
  if (ql > 0 && tl > 0)
    for (int s = 0; s < (int)((tl + 63) >> 6); ++s) {
      const AlnStripeSteps r = aln_band_stripe_steps((int)ql, (int)tl, s, b);
      steps += (r.e[0] - r.a[0]) + (r.e[1] - r.a[1]);
      full += ql + (tl - 64 * (int64_t)s < 64 ? tl - 64 * (int64_t)s : 64) - 1;
    }
  if (full_out) *full_out = full;
  return steps;
}
