// call_dp.hip -- gfx950 kernels + C-ABI for the two third-party DP seams of `SVDSS call`:
//   * ksw_extd2_sse(..., w=-1, zdrop=-1, end_bonus=-1, flag=0)  /root/reference/caller.cpp:348-349
//     (consensus -> reference window, global, dual affine gap, full matrix, CIGAR)
//   * rapidfuzz::fuzz::ratio(a, b)                              /root/reference/caller.cpp:456,458
//
// Both are integer DPs whose anti-diagonals are independent.
//   realignment: one WAVEFRONT per pair, no LDS and no barrier.  The target is cut into stripes of 64 rows, lane l
//     owns row 64 s + l; at step tau the lane computes column tau - l, so the wave sweeps an anti-diagonal per step:
//     H/F/F2 of (i, j-1) are the lane's own registers, H/E/E2 of (i-1, j) arrive from lane l-1 with one DPP shift
//     each, H of (i-1, j-1) is last step's shifted H.  The last row of a stripe leaves H/E/E2 per column in a
//     boundary buffer the next stripe's lane 0 reads 64 columns at a time.  ~1 wave instruction per cell; the chip is
//     filled by running thousands of pairs at once (longest first).
//   ratio: one workgroup per pair sweeps the anti-diagonals, the previous two diagonals stay resident in LDS.
// Not HBM- and not MFMA-bound: the figure of merit is cell updates/s.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/svdss_hip.h"
#include "aln_band.h"
#include "call_streams.h"
#include "dev_arena.h"
#include "hip_check.h"

#define DP_NEG (-0x20000000)
#define DP_THREADS 256

struct GapModel { int q, e, q2, e2; };

__device__ __forceinline__ int dp_gap(int l, const GapModel& g) {
  const int a = g.q + l * g.e, b = g.q2 + l * g.e2;
  return a < b ? a : b;
}

struct AlnPair {
  int64_t q_off, t_off;   // into the concatenated query / target symbol buffers
  int64_t bnd_off;        // int32 workspace: (waves + 1) x 3 arrays of (ql + 64): H, E, E2 of a stripe's last row
  int64_t dir_off;        // (tl+ql)*tl direction bytes, diagonal-major: cell (i, j) at (i+j)*tl + i
  int64_t cig_off;        // uint32 ops in backtrack order, capacity tl + ql + 2
  int32_t ql, tl;
  int32_t slot;           // index of the pair in the caller's order (results are written there)
  int32_t waves;          // wavefronts that share the pair's stripes (1, or the kernel's W for the longest pairs)
  AlnBand band;           // the diagonals an optimal alignment can cross (aln_band.h); ALN_FULL: the whole matrix
};

__device__ __forceinline__ int dp_shr1(int x) {   // value of the lane below (lane 0: unchanged, it is overwritten)
  return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false);
}

// One wavefront per pair -- or, for the longest pairs of a batch, W wavefronts (round 5): a pair is a chain of
// (tl / 64) x (ql + 63) dependent steps, so a launch lasts as long as its longest pair (with full matrices: 26 ms of a bench
// step's realignment, all of it the 2.6 kb x 2.6 kb pairs, while the whole batch was 8 ms of work).  The stripes of a pair only
// depend on each other through the boundary row, column by column: stripe s + 1 can run three blocks of 64 columns behind
// stripe s.  Wavefront v of the pair's workgroup takes stripes v, v + W, ...; the boundary rows go through W + 1 buffers
// in HBM (workgroup-scope release / loads: producer and consumer sit on the same CU and share its L1), progress through one LDS word per buffer, (stripe + 1) << 20 | columns done -- the stripe number in
// it, so that what an earlier stripe left in the word reads as "not yet".  Nobody waits for a stripe with a higher number,
// the lowest unfinished stripe never waits: no deadlock; a wait that does not end all the same (1 << 22 polls) raises
// *abort_flag and the host runs the batch again with one wavefront per pair.
// Cell (i, j): i indexes the target, j the query.
// Recurrences and tie rules are those of ksw2's extd2 (left-aligned), see the oracle
// (oracle/svdss_oracle_call.c, orc_ksw_extd2_global) which this kernel must match bit for bit.
//
// BAND (aln_band.h has the bound and why the result stays bit-exact): only the cells on the pair's live diagonals are
// computed.  A stripe runs the steps in which some lane's cell is live (aln_band_stripe_steps: one range, or two with a
// jump between them); in an executed step a lane whose cell is not live hands on "no path" (DP_NEG) instead.  After a jump
// every value a lane takes from the skipped steps is "no path", set in one place (`repair` below).  The boundary row of the
// stripe above holds only the columns that stripe's lane 63 found live: the READER substitutes "no path" for every other
// column (fetch, and lane 0's diagonal value after a jump), so nothing a buffer holds from an earlier stripe or an earlier
// call is ever used.  A dead interior is crossed by one gap run (ALN_CARRY): horizontally the lane keeps F / F2 in its own
// registers, - e and - e2 per cell; vertically the cell on diagonal c2 leaves what the cell below it would receive in two
// per-column arrays behind the boundary buffers, and the cell of that column on diagonal c1 -- at least two stripes
// further down, so after every stripe above it has passed the column -- takes it, less e and e2 per skipped row.
// The backtrack never reads a direction byte of a cell that was not computed.
template <int W, bool BAND>
__device__ __forceinline__ void align_pair(
    const AlnPair& P, const uint8_t* qsyms, const uint8_t* tsyms, int m, const int8_t* mat_g,
    const GapModel& gm, int32_t* ws, uint8_t* dirs, uint32_t* cigars, int32_t* scores, int32_t* n_cigar, int32_t* abort_flag) {
  const int ql = P.ql, tl = P.tl;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Wp = W > 1 ? P.waves : 1, NB = Wp + 1;
  // (the kernel holds both instantiations of this function, so these W + 2 words are allocated twice: 2 x 24 bytes at W = 4)
  __shared__ volatile int32_t prog[W + 1];
  __shared__ int32_t s_score;
  const uint8_t* q = qsyms + P.q_off;
  const uint8_t* t = tsyms + P.t_off;
  uint8_t* dir = dirs + P.dir_off;
  const int bstride = ql + 64;
  int32_t* bnd = ws + P.bnd_off;
  const AlnBand B = P.band;
  const bool horiz = BAND && B.mode == ALN_CARRY && ql > tl, vert = BAND && B.mode == ALN_CARRY && ql < tl;
  const int dead_w = B.c2 - B.c1 - 1;
  int32_t* xarr = bnd + (int64_t)NB * 3 * bstride;   // vert: E, E2 arriving below the upper band's last cell, per column
  auto decayed = [](int32_t v, int per, int n) {     // v - per * n, not below "no path"
    const int64_t x = (int64_t)v - (int64_t)per * n;
    return x < DP_NEG ? (int32_t)DP_NEG : (int32_t)x;
  };
  // boundary above row 0 ("stripe -1", buffer NB - 1): H(-1, j) = -gap(j + 1), no gap state
  {
    int32_t* b0 = bnd + (int64_t)(NB - 1) * 3 * bstride;
    for (int j = threadIdx.x; j < ql; j += 64 * Wp) { b0[j] = -dp_gap(j + 1, gm); b0[bstride + j] = DP_NEG; b0[2 * bstride + j] = DP_NEG; }
    if ((int)threadIdx.x < NB) prog[threadIdx.x] = (int)threadIdx.x == NB - 1 ? ql : 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  }
  __syncthreads();
  const int n_stripes = (tl + 63) >> 6;
  int32_t final_score = 0;
  bool aborted = false;
  for (int s = wave; s < n_stripes && !aborted; s += Wp) {
    const int in_slot = (s + NB - 1) % NB, out_slot = s % NB;
    const int32_t* bin = bnd + (int64_t)in_slot * 3 * bstride;
    int32_t* bout = bnd + (int64_t)out_slot * 3 * bstride;
    if (W > 1 && lane == 0) prog[out_slot] = (s + 1) << 20;
    const int i = (s << 6) + lane;
    const bool row_ok = i < tl;
    const int rows = tl - (s << 6) < 64 ? tl - (s << 6) : 64;
    const bool writes_bnd = lane == 63 && s + 1 < n_stripes;
    // substitution scores of this row's target symbol, one byte per query symbol (m <= 8)
    uint64_t rowbits = 0;
    {
      const int ti = row_ok ? t[i] : 0;
      for (int k = 0; k < m; ++k) rowbits |= (uint64_t)(uint8_t)mat_g[ti * m + k] << (8 * k);
    }
    // (i, j-1): the column left of j = 0, exact where column 0 is live for the row
    int32_t Hl = !BAND || aln_band_live(-i, B) ? -dp_gap(i + 1, gm) : DP_NEG, Fl = DP_NEG, F2l = DP_NEG;
    int32_t Hout = 0, Eout = DP_NEG, E2out = DP_NEG;                    // what the lane above reads next step
    int32_t Hd = 0;                                                     // (i-1, j-1)
    int qcur = 0;
    const int n_steps = ql + rows - 1;
    AlnStripeSteps R;
    if (BAND) R = aln_band_stripe_steps(ql, tl, s, B);
    else { R.a[0] = 0; R.e[0] = n_steps; R.a[1] = R.e[1] = n_steps; }
    const int dl = (s << 6) + 2 * lane;                                 // the lane's cell at step tau is on diagonal tau - dl
    // vert: the carried gap arrives at the row's cell on diagonal c1, column xcol, step xcol + lane
    const int xcol = B.c1 + i;
    int32_t Xv = DP_NEG, X2v = DP_NEG;
    // the next 64 columns of the query and of the boundary row, one per lane, fetched a block ahead
    int32_t nH = 0, nE = 0, nE2 = 0;
    int nq = 0;
    const int32_t none = BAND ? DP_NEG : 0;
    // several wavefronts: wait until the stripe above has announced `need` columns
    auto wait_above = [&](int need) {
      int polls = 0;
      for (;;) {
        const int32_t v = prog[in_slot];
        if ((v >> 20) == s && (v & 0xFFFFF) >= need) return;
        if (++polls > (1 << 22)) { aborted = true; return; }
        __builtin_amdgcn_s_sleep(2);
      }
    };
    auto fetch = [&](int tau0) {
      const int jj = tau0 + lane;
      // BAND: a column the stripe above did not find live reads as "no path", whatever the buffer holds
      const bool in = jj < ql && (!BAND || aln_band_live(jj - (s << 6) + 1, B));
      const bool xin = vert && row_ok && xcol >= 0 && xcol < ql && xcol + lane >= tau0 && xcol + lane < tau0 + 64;
      nq = jj < ql ? q[jj] : 0;
      if (W > 1 && Wp > 1) {
        // columns tau0 .. tau0 + 63 of the stripe above: wait until its wavefront has them in memory
        wait_above(tau0 + 64 < ql ? tau0 + 64 : ql);
        if (aborted) { nH = 0; nE = 0; nE2 = 0; return; }
        // acquire side of the producer's workgroup-scope release: the boundary row is read after the progress word
        // whatever the CU mode (relaxed loads alone are only ordered while both waves share one L1)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        nH = in ? __hip_atomic_load(&bin[jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : none;
        nE = in ? __hip_atomic_load(&bin[bstride + jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : none;
        nE2 = in ? __hip_atomic_load(&bin[2 * bstride + jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : none;
        if (BAND && xin) {   // (the stripes above have all passed column xcol <= tau0 + 63: the wait above)
          Xv = decayed(__hip_atomic_load(&xarr[xcol], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), gm.e, dead_w);
          X2v = decayed(__hip_atomic_load(&xarr[bstride + xcol], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), gm.e2, dead_w);
        }
      } else {
        nH = in ? bin[jj] : none; nE = in ? bin[bstride + jj] : none; nE2 = in ? bin[2 * bstride + jj] : none;
        if (BAND && xin) { Xv = decayed(xarr[xcol], gm.e, dead_w); X2v = decayed(xarr[bstride + xcol], gm.e2, dead_w); }
      }
    };
    for (int r = 0; r < (BAND ? 2 : 1) && !aborted; ++r) {
    const int ra = r ? R.a[1] : R.a[0], re = r ? R.e[1] : R.e[0];
    if (ra >= re) continue;
    fetch(ra);
    if (BAND && ra > 0 && !aborted) {
      // repair: the steps before `ra` were not run, and every cell of them was dead (or, on a lane that has not started
      // its row, is still to come): what a lane takes from them is "no path", the query symbol is read again
      const int jq = ra - 1 - lane;
      qcur = jq >= 0 && jq < ql ? q[jq] : 0;
      Hout = DP_NEG; Eout = DP_NEG; E2out = DP_NEG;
      Hd = DP_NEG;
      if (lane == 0 && ra - 1 < ql && aln_band_live(ra - (s << 6), B))   // (i-1, ra-1), if the stripe above found it live
        Hd = W > 1 && Wp > 1 ? __hip_atomic_load(&bin[ra - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : bin[ra - 1];
      if (ra - lane > 0) {
        // horizontal carry: the gap run went on through the skipped cells of the row
        // (it may open at the lane's last live cell: Hl is that cell's H there, "no path" on a lane already past it)
        if (horiz && r == 1) {
          Fl = decayed(Hl - gm.q > Fl ? Hl - gm.q : Fl, gm.e, ra - R.e[0]);
          F2l = decayed(Hl - gm.q2 > F2l ? Hl - gm.q2 : F2l, gm.e2, ra - R.e[0]);
        }
        else { Fl = DP_NEG; F2l = DP_NEG; }
        Hl = DP_NEG;
      }
    }
    uint8_t* dcell = dir + (int64_t)((s << 6) + ra) * tl + i;   // cell (i, j) at (i + j) * tl + i: + tl per step
    for (int tau0 = ra; tau0 < re && !aborted; tau0 += 64) {
      // wait for the block here, once, so that the 64 steps below never wait on memory (their direction-byte stores
      // stay in flight: vmcnt counts stores too)
      asm volatile("" : "+v"(nq), "+v"(nH), "+v"(nE), "+v"(nE2));
      if (BAND) asm volatile("" : "+v"(Xv), "+v"(X2v));
      const int qblk = nq;
      const int32_t bH = nH, bE = nE, bE2 = nE2;
      if (tau0 + 64 < re) fetch(tau0 + 64);
      const int kmax = re - tau0 < 64 ? re - tau0 : 64;
      for (int k = 0; k < kmax; ++k) {
        const int tau = tau0 + k;
        const int qs = __builtin_amdgcn_readlane(qblk, k);
        const int32_t hb = __builtin_amdgcn_readlane(bH, k), eb = __builtin_amdgcn_readlane(bE, k),
                      e2b = __builtin_amdgcn_readlane(bE2, k);
        qcur = dp_shr1(qcur);
        int32_t Hu = dp_shr1(Hout), Eu = dp_shr1(Eout), E2u = dp_shr1(E2out);
        if (lane == 0) { qcur = qs; Hu = hb; Eu = eb; E2u = e2b; }
        const int j = tau - lane;
        const bool inr = row_ok && j >= 0 && j < ql;
        const int dg = tau - dl;
        if (BAND && inr && !aln_band_live(dg, B)) {
          // not computed: no path through the cell -- but for the gap run that crosses the dead interior along the row
          if (horiz && dg > B.c1 && dg < B.c2) {
            Fl = (Hl - gm.q > Fl ? Hl - gm.q : Fl) - gm.e;
            F2l = (Hl - gm.q2 > F2l ? Hl - gm.q2 : F2l) - gm.e2;
          } else { Fl = DP_NEG; F2l = DP_NEG; }
          Hl = DP_NEG;
          Hout = DP_NEG; Eout = DP_NEG; E2out = DP_NEG;
        } else if (inr) {
          const int32_t hdiag = j == 0 ? (i == 0 ? 0 : -dp_gap(i, gm)) : Hd;
          int32_t Ein = (Hu - gm.q > Eu ? Hu - gm.q : Eu) - gm.e;
          int32_t E2in = (Hu - gm.q2 > E2u ? Hu - gm.q2 : E2u) - gm.e2;
          if (BAND && vert && dg == B.c1) { Ein = Xv; E2in = X2v; }   // the cells above are the dead interior
          const int32_t Fin = (Hl - gm.q > Fl ? Hl - gm.q : Fl) - gm.e;
          const int32_t F2in = (Hl - gm.q2 > F2l ? Hl - gm.q2 : F2l) - gm.e2;
          int32_t z = hdiag + (int32_t)(int8_t)(rowbits >> (8 * qcur));
          uint32_t d = 0;
          if (Ein > z) { d = 1; z = Ein; }
          if (Fin > z) { d = 2; z = Fin; }
          if (E2in > z) { d = 3; z = E2in; }
          if (F2in > z) { d = 4; z = F2in; }
          if (Ein > z - gm.q) d |= 0x08;
          if (Fin > z - gm.q) d |= 0x10;
          if (E2in > z - gm.q2) d |= 0x20;
          if (F2in > z - gm.q2) d |= 0x40;
          *dcell = (uint8_t)d;   // diagonal-major: the lanes of a step write consecutive bytes
          Hout = z; Eout = Ein; E2out = E2in;
          Hl = z; Fl = Fin; F2l = F2in;
          if (writes_bnd) { bout[j] = z; bout[bstride + j] = Ein; bout[2 * bstride + j] = E2in; }
          if (BAND && vert && dg == B.c2) {   // what the dead cell below would receive
            xarr[j] = (z - gm.q > Ein ? z - gm.q : Ein) - gm.e;
            xarr[bstride + j] = (z - gm.q2 > E2in ? z - gm.q2 : E2in) - gm.e2;
          }
          if (i == tl - 1 && j == ql - 1) final_score = z;
        }
        Hd = Hu;
        dcell += tl;
      }
      if (W > 1 && Wp > 1 && s + 1 < n_stripes) {
        // lane 63 has finished columns 0 .. tau0 + kmax - 64 of the boundary row: in memory, then announced
        // (workgroup scope: the stores have reached the L2 of this XCD, which the reader's CU -- the same one -- reads
        // through the L1 it shares with the writer.  An agent-scope fence writes the whole L2 back on this multi-die part:
        // the first version of this kernel spent more time in it than it saved)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        const int done = tau0 + kmax - 63;
        if (lane == 63) prog[out_slot] = ((s + 1) << 20) | (done < 0 ? 0 : done > ql ? ql : done);
      }
    }
    // (no announcement for the columns a jump skips: a stripe only ever announces a column after a block that waited
    // for the stripe above to announce it, so "stripe s - 1 has passed column c" still means every stripe above has --
    // which is what lets a lane read the carried gap of column c from the exit arrays)
    }
    if (W == 1 || Wp == 1) __syncthreads();   // (one wavefront: the boundary row is in memory before the next stripe reads it)
    else if (s + 1 < n_stripes) {
      // vert: a stripe whose bands end short of the last column has not waited for it; it ends after the stripe above, so
      // that its "all columns done" says the same of every stripe above (whose exit arrays the stripes below read)
      if (BAND && vert && !aborted) { wait_above(ql); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 63) prog[out_slot] = ((s + 1) << 20) | ql;
    }
    if (s == n_stripes - 1) {   // the lane that owned (tl-1, ql-1) has the score
      const int owner = (tl - 1) & 63;
      final_score = __builtin_amdgcn_readlane(final_score, owner);
      if (lane == 0) s_score = final_score;
    }
  }
  if (aborted && lane == 0) atomicExch(abort_flag, 1);
  __syncthreads();   // the direction bytes are in HBM, the score in LDS
  if (wave != 0) return;
  final_score = s_score;
  {
    // ksw_backtrack from (tl-1, ql-1); ops are left in backtrack order, the host reverses
    // them.  A register window holds the direction bytes of 64 rows x 4 columns along the current diagonal (one HBM
    // latency per ~60 steps of a mostly diagonal path instead of one per step); runs are merged in registers.
    if (lane == 0) scores[P.slot] = final_score;
    uint32_t* cg = cigars + P.cig_off;
    int n = 0, i = tl - 1, j = ql - 1, state = 0;
    uint32_t cur_op = 0xffffffffu, cur_len = 0;
    auto push = [&](uint32_t op, uint32_t len) {
      if (op == cur_op) { cur_len += len; return; }
      if (cur_op != 0xffffffffu) { if (lane == 0) cg[n] = (cur_len << 4) | cur_op; ++n; }
      cur_op = op; cur_len = len;
    };
    int i0 = -(1 << 28), j0 = 0;
    uint32_t win = 0;
    while (i >= 0 && j >= 0) {
      if (BAND && !aln_band_live(j - i, B)) {
        // a cell that was not computed has no direction byte.  In the dead interior the walk is inside the one gap run that
        // crosses it (aln_band.h: the stored bits would say "extended" all the way): the run goes on to the live band.
        // Any other state there, or a cell outside the hull, cannot occur; the walk then moves on as if "extended" were
        // stored as well, without reading anything.
        const int dg = j - i;
        if (horiz && dg > B.c1 && dg < B.c2 && (state == 2 || state == 4)) { push(1, (uint32_t)(dg - B.c1)); j -= dg - B.c1; }
        else if (vert && dg > B.c1 && dg < B.c2 && (state == 1 || state == 3)) { push(2, (uint32_t)(B.c2 - dg)); i -= B.c2 - dg; }
        else if (state == 0) { push(0, 1); --i; --j; }
        else if (state == 1 || state == 3) { push(2, 1); --i; }
        else { push(1, 1); --j; }
        continue;
      }
      int k = i0 - i, d = j - (j0 - k);
      if (k < 0 || k > 63 || d < 0 || d > 3) {
        i0 = i; j0 = j - 1; k = 0; d = 1;       // columns j0-k .. j0-k+3 of row i0-k (room for two D and one I moves)
        const int ii = i0 - lane;
        const int64_t jj = (int64_t)j0 - lane;
        win = 0;
        if (ii >= 0) {
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const int64_t c = jj + x;
            if (c >= 0 && c < ql) win |= (uint32_t)dir[(int64_t)(ii + c) * tl + ii] << (8 * x);
          }
        }
        asm volatile("" : "+v"(win));   // wait for the window here, not at the join below
      }
      const uint32_t tmp = ((uint32_t)__builtin_amdgcn_readlane((int)win, k) >> (8 * d)) & 0xffu;
      if (state == 0) state = tmp & 7;
      else if (!((tmp >> (state + 2)) & 1)) state = 0;
      if (state == 0) state = tmp & 7;
      if (state == 0) { push(0, 1); --i; --j; }
      else if (state == 1 || state == 3) { push(2, 1); --i; }
      else { push(1, 1); --j; }
    }
    if (i >= 0) push(2, (uint32_t)(i + 1));
    if (j >= 0) push(1, (uint32_t)(j + 1));
    if (cur_op != 0xffffffffu) { if (lane == 0) cg[n] = (cur_len << 4) | cur_op; ++n; }
    if (lane == 0) n_cigar[P.slot] = n;
  }
}

template <int W>
__global__ void __launch_bounds__(64 * W) align_wave_kernel(
    const AlnPair* pairs, const uint8_t* qsyms, const uint8_t* tsyms, int m, const int8_t* mat_g,
    GapModel gm, int32_t* ws, uint8_t* dirs, uint32_t* cigars, int32_t* scores, int32_t* n_cigar, int32_t* abort_flag) {
  const AlnPair P = pairs[blockIdx.x];
  if ((int)(threadIdx.x >> 6) >= (W > 1 ? P.waves : 1)) return;
  if (P.ql <= 0 || P.tl <= 0) {   // ksw2 returns before touching ez: score 0, no CIGAR
    if ((threadIdx.x & 63) == 0) { scores[P.slot] = 0; n_cigar[P.slot] = 0; }
    return;
  }
  // a pair planned "full matrix" runs the code without the masks (the branch is uniform over the workgroup)
  if (P.band.mode != ALN_FULL) align_pair<W, true>(P, qsyms, tsyms, m, mat_g, gm, ws, dirs, cigars, scores, n_cigar, abort_flag);
  else align_pair<W, false>(P, qsyms, tsyms, m, mat_g, gm, ws, dirs, cigars, scores, n_cigar, abort_flag);
}

// The two diagonal sums of a pair's S_lb (aln_band.h), one wavefront per pair: sum_out = max over x of (prefix [0, x) on
// diagonal 0 + suffix [x, n) on diagonal D), n = min(ql, tl) -- the sum of the suffix diagonal plus the largest prefix sum
// of (diagonal 0 - diagonal D), the empty prefix included; the plain diagonal for D = 0.  The host subtracts the gap and
// plans.  Lane l takes positions [l per, (l + 1) per).  A symbol outside the matrix raises *bad (the batch then runs its
// full matrices, as the host's look-ups have no entry for it either).
__global__ void __launch_bounds__(64) aln_slb_kernel(const uint8_t* qsyms, const int64_t* q_off, const uint8_t* tsyms, const int64_t* t_off,
                                                     int m, const int8_t* mat_g, int64_t* sum_out, int32_t* bad) {
  const int64_t p = blockIdx.x;
  const int64_t ql = q_off[p + 1] - q_off[p], tl = t_off[p + 1] - t_off[p];
  const int64_t n = ql < tl ? ql : tl, D = ql - tl;
  const int lane = threadIdx.x;
  if (n <= 0) { if (lane == 0) sum_out[p] = 0; return; }
  const uint8_t* q = qsyms + (q_off[p] - q_off[0]);
  const uint8_t* t = tsyms + (t_off[p] - t_off[0]);
  const int64_t qs = D > 0 ? D : 0, ts = D < 0 ? -D : 0;
  const int64_t per = (n + 63) >> 6, k0 = lane * per, k1 = k0 + per < n ? k0 + per : n;
  bool off = false;
  auto score = [&](int tsym, int qsym) {
    if (tsym >= m || qsym >= m) { off = true; return 0; }
    return (int)mat_g[tsym * m + qsym];
  };
  int64_t sb = 0, sc = 0, mp = 0;   // the chunk's sum on diagonal D, of the difference, and its largest prefix of the difference
  for (int64_t k = k0; k < k1; ++k) {
    const int a = score(t[k], q[k]), bq = D != 0 ? score(t[k + ts], q[k + qs]) : a;
    sb += bq;
    sc += a - bq;
    mp = sc > mp ? sc : mp;
  }
  if (__any(off) && lane == 0) atomicExch(bad, 1);
  // in lane order: sum of the chunks before + the chunk's own largest prefix
  int64_t before = sc;
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t v = __shfl_up(before, o, 64);
    if (lane >= o) before += v;
  }
  int64_t best = before - sc + mp, tot = sb;
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t v = __shfl_xor(best, o, 64), w = __shfl_xor(tot, o, 64);
    best = v > best ? v : best;
    tot += w;
  }
  if (lane == 0) sum_out[p] = tot + (best > 0 ? best : 0);
}

// barrier that orders LDS traffic only
__device__ __forceinline__ void dp_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

struct LcsPair {
  int64_t a_off, b_off, ws_off;   // ws: 3 arrays of (la + 1) int32
  int32_t la, lb;
};

// LCS length by anti-diagonals, then rapidfuzz::fuzz::ratio's arithmetic.
// (LDS = true: the three rotating diagonals and both strings live in LDS)
template <bool LDS>
__global__ void __launch_bounds__(DP_THREADS) lcs_ratio_kernel(const LcsPair* pairs, const uint8_t* as,
                                                              const uint8_t* bs, int32_t* ws,
                                                              int64_t* lcs_out, double* ratio_out) {
  extern __shared__ int32_t dp_lds[];
  const LcsPair P = pairs[blockIdx.x];
  const int la = P.la, lb = P.lb;
  int64_t lcs = 0;
  if (la > 0 && lb > 0) {
    const uint8_t* a = as + P.a_off;
    const uint8_t* b = bs + P.b_off;
    const int stride = la + 1;
    int32_t* buf = LDS ? dp_lds : ws + P.ws_off;
    if (LDS) {
      uint8_t* sa = (uint8_t*)(dp_lds + 3 * stride);
      uint8_t* sb = sa + la;
      for (int x = threadIdx.x; x < la; x += DP_THREADS) sa[x] = a[x];
      for (int x = threadIdx.x; x < lb; x += DP_THREADS) sb[x] = b[x];
      a = sa;
      b = sb;
      __syncthreads();
    }
    const int n_diag = la + lb - 1;
    for (int r = 0; r < n_diag; ++r) {
      const int32_t* Lm1 = buf + ((r + 2) % 3) * stride;
      const int32_t* Lm2 = buf + ((r + 1) % 3) * stride;
      int32_t* Lc = buf + (r % 3) * stride;
      const int ilo = r - (lb - 1) > 0 ? r - (lb - 1) : 0;
      const int ihi = r < la - 1 ? r : la - 1;
      for (int i = ilo + (int)threadIdx.x; i <= ihi; i += DP_THREADS) {
        const int j = r - i;
        const int32_t diag = (i > 0 && j > 0) ? Lm2[i - 1] : 0;
        const int32_t up = i > 0 ? Lm1[i - 1] : 0;
        const int32_t left = j > 0 ? Lm1[i] : 0;
        Lc[i] = a[i] == b[j] ? diag + 1 : (up > left ? up : left);
      }
      if (LDS) dp_lds_barrier(); else __syncthreads();
    }
    lcs = buf[((n_diag - 1) % 3) * stride + la - 1];
  }
  if (threadIdx.x == 0) {
    const int64_t maximum = (int64_t)la + lb;
    const int64_t dist = maximum - 2 * lcs;
    const double norm_dist = maximum ? (double)dist / (double)maximum : 0.0;
    const double norm_sim = 1.0 - norm_dist;
    lcs_out[blockIdx.x] = lcs;
    ratio_out[blockIdx.x] = norm_sim * 100.0;
  }
}

// LCS length bit-parallel (Crochemore et al. / Hyyro: V = (V + U) | (V - U) with U = V & PM[text symbol]; the LCS is the
// number of zero bits of V), one wavefront per pair: lane w holds word w of the bit vector over the shorter string (up to
// 64 x 64 = 4,096 symbols), the carries of the multi-word addition come from two ballots -- lanes that generate a carry
// and lanes that would pass one on -- and one 64-bit scalar addition: carry-in mask = ((pass + (gen << 1)) ^ pass).  The
// match masks PM[symbol] (at most 8 distinct symbols, `sym_id` maps bytes to 0..7, 255 = absent) sit in LDS, the one of
// the next text symbol is fetched while the current step computes.  ~20 instructions per text symbol instead of one DP
// cell per lane per step: 5,092 pairs of ~1.2 kb take well under a millisecond (the anti-diagonal kernel: 11.6 ms).
__global__ void __launch_bounds__(64) lcs_bits_kernel(const LcsPair* pairs, const uint8_t* as, const uint8_t* bs,
                                                      const uint8_t* sym_id, int64_t* lcs_out, double* ratio_out) {
  __shared__ unsigned long long pm[8][64];
  const LcsPair P = pairs[blockIdx.x];
  const int lane = threadIdx.x;
  // pattern = the shorter string, text = the longer one
  const bool swap = P.la > P.lb;
  const uint8_t* pat = swap ? bs + P.b_off : as + P.a_off;
  const uint8_t* txt = swap ? as + P.a_off : bs + P.b_off;
  const int m = swap ? P.lb : P.la, n = swap ? P.la : P.lb;
  int64_t lcs = 0;
  if (m > 0) {
    unsigned long long mk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 64; ++i) {
      const int pos = 64 * lane + i;
      const int id = pos < m ? (int)sym_id[pat[pos]] : 255;
#pragma unroll
      for (int k = 0; k < 8; ++k) mk[k] |= (unsigned long long)(id == k) << i;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) pm[k][lane] = mk[k];
    __syncthreads();
    unsigned long long V = ~0ull;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int tid = j0 + lane < n ? (int)sym_id[txt[j0 + lane]] : 255;
      const int cnt = n - j0 < 64 ? n - j0 : 64;
      int id = __builtin_amdgcn_readlane(tid, 0);
      unsigned long long cur = id < 8 ? pm[id][lane] : 0ull;
      for (int t = 0; t < cnt; ++t) {
        const int idn = __builtin_amdgcn_readlane(tid, t + 1 < cnt ? t + 1 : t);
        const unsigned long long nxt = idn < 8 ? pm[idn][lane] : 0ull;
        const unsigned long long U = V & cur;
        unsigned long long sum = V + U;
        const unsigned long long gen = __ballot(sum < V), pass = __ballot(sum == ~0ull);
        const unsigned long long carry = (pass + (gen << 1)) ^ pass;
        sum += (carry >> lane) & 1ull;
        V = sum | (V - U);
        cur = nxt;
      }
    }
    // zeros of V among the pattern's m bits
    const int valid = m - 64 * lane;
    const unsigned long long vm = valid >= 64 ? ~0ull : valid <= 0 ? 0ull : ((1ull << valid) - 1);
    int z = (int)__popcll(~V & vm);
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
    lcs = z;
  }
  if (lane == 0) {
    const int64_t maximum = (int64_t)P.la + P.lb;
    const int64_t dist = maximum - 2 * lcs;
    const double norm_dist = maximum ? (double)dist / (double)maximum : 0.0;
    const double norm_sim = 1.0 - norm_dist;
    lcs_out[blockIdx.x] = lcs;
    ratio_out[blockIdx.x] = norm_sim * 100.0;
  }
}

// ------------------------------------------------------------------- ABI

struct svdss_aln_batch {
  int64_t n_pairs = 0;
  int64_t total_cigar = 0;
  int64_t cells = 0;
  double kernel_ms = 0.0;
  int64_t info[4] = {0, 0, 0, 0};   // the last call: chunks, pairs with several wavefronts, largest W, chunks run again
  int64_t band[4] = {0, 0, 0, 0};   // the last call: wavefront steps executed, those of the full matrices, pairs with one band, pairs with a carried gap
  std::vector<int32_t> scores;
  std::vector<int64_t> n_cigar;
  std::vector<uint32_t> cigar;   // per pair, forward order, concatenated
  // device state kept between calls
  int device = -1;
  DevArena arena;      // a chunk's workspace
  DevArena in_arena;   // the call's symbols, matrix and offsets, uploaded once, and the planning kernel's sums
};

namespace {
struct DevMem {
  void* p = nullptr;
  ~DevMem() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) {
    HIPCHK(hipMalloc(&p, bytes ? bytes : 16));
    return SVDSS_OK;
  }
};
}  // namespace

extern "C" int svdss_align_global_batch(const uint8_t* queries, const int64_t* q_off,
                                        const uint8_t* targets, const int64_t* t_off, int64_t n_pairs,
                                        int32_t m, const int8_t* mat, int32_t gapo, int32_t gape,
                                        int32_t gapo2, int32_t gape2, int32_t device,
                                        svdss_aln_batch_t** out) {
  if (!out || n_pairs < 0 || m < 1 || m > 8 || !mat || device < 0) return SVDSS_EINVAL;
  if (n_pairs > 0 && (!queries || !q_off || !targets || !t_off)) return SVDSS_EINVAL;
  HIPCHK(hipSetDevice(device));
  svdss_aln_batch* b = *out ? *out : new (std::nothrow) svdss_aln_batch();
  if (!b) return SVDSS_ENOMEM;
  *out = b;
  b->n_pairs = n_pairs;
  b->total_cigar = 0;
  b->cells = 0;
  b->kernel_ms = 0.0;
  b->info[0] = b->info[1] = b->info[2] = b->info[3] = 0;
  b->band[0] = b->band[1] = b->band[2] = b->band[3] = 0;
  b->scores.assign((size_t)n_pairs, 0);
  b->n_cigar.assign((size_t)n_pairs, 0);
  b->cigar.clear();
  if (n_pairs == 0) return SVDSS_OK;
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int64_t ql = q_off[i + 1] - q_off[i], tl = t_off[i + 1] - t_off[i];
    if (ql < 0 || tl < 0) return SVDSS_EINVAL;
    if (ql >= (1 << 28) || tl >= (1 << 28)) return SVDSS_ERANGE;
  }
  const int64_t qtot = q_off[n_pairs] - q_off[0], ttot = t_off[n_pairs] - t_off[0];
  if (b->device != device) {
    b->arena.drop();
    b->in_arena.drop();
    b->device = device;
  }
  // the call's one stream, from the call side's pool (call_streams.h): calls of different threads overlap
  CallStreamLease lease;
  HIPCHK(lease.acquire(device));
  const hipStream_t st = lease.get();
  const GapModel gm{gapo, gape, gapo2, gape2};
  hipEvent_t ev0, ev1;
  HIPCHK(hipEventCreate(&ev0));
  HIPCHK(hipEventCreate(&ev1));
  // chunks of pairs whose direction matrices fit the workspace budget (HBM has 288 GB; the index may hold half of it)
  int64_t dir_budget = (int64_t)24 << 30;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      dir_budget = std::min<int64_t>(dir_budget, (int64_t)((free_b + b->arena.cap) / 2));
    if (dir_budget < ((int64_t)1 << 30)) dir_budget = (int64_t)1 << 30;
    // SVDSS_ALIGN_DIR_MB: the budget in MB, no floor (tests: several chunks from a small batch)
    if (getenv("SVDSS_ALIGN_DIR_MB") && atoll(getenv("SVDSS_ALIGN_DIR_MB")) > 0) dir_budget = atoll(getenv("SVDSS_ALIGN_DIR_MB")) << 20;
  }
  std::vector<int32_t> h_nc((size_t)n_pairs, 0);
  std::vector<std::pair<int64_t, int64_t>> cig_at((size_t)n_pairs);   // (chunk-local offset, chunk index)
  std::vector<std::vector<uint32_t>> chunk_cigs;
  int64_t start = 0;
  // the longest pairs of the batch get ALN_W wavefronts each (align_wave_kernel): within a factor of four of the largest
  // matrix (SVDSS_ALIGN_FRAC, default eight), or every pair of a batch too small to fill the GPU with one wavefront per pair.
  // SVDSS_ALIGN_WAVES=1: never; =8: eight.  Measured on a bench step (5,093 pairs) with full matrices: 26.5 -> 16.5 ms.
  // The choice still goes by ql x tl, not by the steps a pair is planned to run (aln_band.h); whether several wavefronts
  // pay for a pair that runs two blocks of 64 steps per stripe has not been measured.
  const int ALN_W = getenv("SVDSS_ALIGN_WAVES") && atoi(getenv("SVDSS_ALIGN_WAVES")) == 8 ? 8 : 4;
  const int64_t aln_frac = getenv("SVDSS_ALIGN_FRAC") && atoll(getenv("SVDSS_ALIGN_FRAC")) > 0 ? atoll(getenv("SVDSS_ALIGN_FRAC")) : 8;
  int64_t max_cells = 0;
  for (int64_t i = 0; i < n_pairs; ++i) max_cells = std::max(max_cells, (q_off[i + 1] - q_off[i]) * (t_off[i + 1] - t_off[i]));
  bool multi = !(getenv("SVDSS_ALIGN_WAVES") && atoi(getenv("SVDSS_ALIGN_WAVES")) <= 1);
  auto waves_of = [&](int64_t ql, int64_t tl) {
    if (!multi || tl < 8 * 64 || ql >= (1 << 20)) return 1;
    return (ql * tl * aln_frac >= max_cells || n_pairs < 2048) ? ALN_W : 1;
  };
  // the symbols and the matrix go up once per call
  HIPCHK(b->in_arena.reserve(DevArena::padded((size_t)qtot) + DevArena::padded((size_t)ttot) + DevArena::padded(64) +
                             3 * DevArena::padded(sizeof(int64_t) * (size_t)(n_pairs + 1)) + DevArena::padded(64)));
  void* d_q = b->in_arena.take((size_t)qtot);
  void* d_t = b->in_arena.take((size_t)ttot);
  void* d_mat = b->in_arena.take(64);
  if (qtot) HIPCHK(hipMemcpyAsync(d_q, queries + q_off[0], (size_t)qtot, hipMemcpyHostToDevice, st));
  if (ttot) HIPCHK(hipMemcpyAsync(d_t, targets + t_off[0], (size_t)ttot, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_mat, mat, (size_t)(m * m), hipMemcpyHostToDevice, st));
  // SVDSS_ALIGN_BAND: 0 the full matrix of every pair, 1 one band of diagonals per pair, 2 (default) two bands with the
  // gap carried across where the plan finds a dead interior (aln_band.h).  Planned here, before the pairs are laid out:
  // the two diagonal sums of every pair on the device, the intervals from them on the host.  (Planned on the host
  // alone, a table look-up per symbol, a bench step's 5,093 pairs took 3.3 ms and the call 4 ms longer; the kernel takes
  // 0.07 ms and costs the two offset arrays up, the sums down and one stream synchronise: profiles/realign_band.txt 3a.)
  int band_level = getenv("SVDSS_ALIGN_BAND") ? std::max(0, std::min(2, atoi(getenv("SVDSS_ALIGN_BAND")))) : 2;
  std::vector<AlnBand> bands((size_t)n_pairs);
  std::vector<int64_t> band_steps((size_t)n_pairs), full_steps((size_t)n_pairs);
  {
    const AlnScoring sc{(int)m, mat, gapo, gape, gapo2, gape2};
    int M = 0;
    std::vector<int64_t> sums((size_t)n_pairs, 0);
    if (band_level > 0 && aln_band_provable(sc, &M)) {
      void* d_qo = b->in_arena.take(sizeof(int64_t) * (size_t)(n_pairs + 1));
      void* d_to = b->in_arena.take(sizeof(int64_t) * (size_t)(n_pairs + 1));
      void* d_sum = b->in_arena.take(sizeof(int64_t) * (size_t)n_pairs);
      void* d_bad = b->in_arena.take(64);
      int32_t bad = 0;
      HIPCHK(hipMemcpyAsync(d_qo, q_off, sizeof(int64_t) * (size_t)(n_pairs + 1), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_to, t_off, sizeof(int64_t) * (size_t)(n_pairs + 1), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(d_bad, 0, 64, st));
      hipLaunchKernelGGL(aln_slb_kernel, dim3((unsigned)n_pairs), dim3(64), 0, st, (const uint8_t*)d_q, (const int64_t*)d_qo,
                         (const uint8_t*)d_t, (const int64_t*)d_to, (int)m, (const int8_t*)d_mat, (int64_t*)d_sum, (int32_t*)d_bad);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(sums.data(), d_sum, sizeof(int64_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (bad) band_level = 0;   // a symbol outside the matrix
    } else {
      band_level = 0;
    }
    for (int64_t i = 0; i < n_pairs; ++i) {
      const int64_t ql = q_off[i + 1] - q_off[i], tl = t_off[i + 1] - t_off[i], k = ql < tl ? tl - ql : ql - tl;
      bands[(size_t)i] = aln_band_plan_slb(ql, tl, sc, band_level, sums[(size_t)i] - aln_gap(k, sc));
      band_steps[(size_t)i] = aln_band_steps(ql, tl, bands[(size_t)i], &full_steps[(size_t)i]);
    }
  }
  while (start < n_pairs) {
    std::vector<AlnPair> hp;
    int64_t ws = 0, dirb = 0, cig = 0, end = start;
    bool any_multi = false;
    while (end < n_pairs) {
      const int64_t ql = q_off[end + 1] - q_off[end], tl = t_off[end + 1] - t_off[end];
      const int64_t need = (ql + tl) * tl;   // direction bytes, one row of tl per anti-diagonal
      if (end > start && dirb + need > dir_budget) break;
      AlnPair a;
      memset(&a, 0, sizeof a);
      a.q_off = q_off[end] - q_off[0];
      a.t_off = t_off[end] - t_off[0];
      a.bnd_off = ws;
      a.dir_off = dirb;
      a.cig_off = cig;
      a.ql = (int32_t)ql;
      a.tl = (int32_t)tl;
      a.slot = (int32_t)(end - start);
      a.waves = waves_of(ql, tl);
      a.band = bands[(size_t)end];
      any_multi = any_multi || a.waves > 1;
      hp.push_back(a);
      cig_at[(size_t)end] = {cig, (int64_t)chunk_cigs.size()};
      ws += (3 * (a.waves + 1) + 2) * (ql + 64);   // the boundary buffers, and the two arrays of a vertically carried gap
      dirb += need;
      cig += ql + tl + 2;
      b->cells += ql * tl;
      ++end;
    }
    const int64_t np = end - start;
    // longest pairs first: a pair is one chain of dependent steps (aln_band_steps: (tl / 64) x (ql + 63) for a full matrix),
    // the longest ones decide when the launch ends
    std::stable_sort(hp.begin(), hp.end(), [&](const AlnPair& x, const AlnPair& y) {
      return band_steps[(size_t)(start + x.slot)] > band_steps[(size_t)(start + y.slot)];
    });
    const size_t need_bytes = DevArena::padded(sizeof(AlnPair) * (size_t)np) + DevArena::padded(sizeof(int32_t) * (size_t)ws) +
                              DevArena::padded((size_t)dirb) + DevArena::padded(sizeof(uint32_t) * (size_t)cig) +
                              2 * DevArena::padded(sizeof(int32_t) * (size_t)np) + DevArena::padded(64);
    HIPCHK(b->arena.reserve(need_bytes));
    void* d_pairs = b->arena.take(sizeof(AlnPair) * (size_t)np);
    void* d_ws = b->arena.take(sizeof(int32_t) * (size_t)ws);
    void* d_dir = b->arena.take((size_t)dirb);
    void* d_cig = b->arena.take(sizeof(uint32_t) * (size_t)cig);
    void* d_sc = b->arena.take(sizeof(int32_t) * (size_t)np);
    void* d_nc = b->arena.take(sizeof(int32_t) * (size_t)np);
    void* d_abort = b->arena.take(64);
    HIPCHK(hipMemcpyAsync(d_pairs, hp.data(), sizeof(AlnPair) * (size_t)np, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_abort, 0, 64, st));
    HIPCHK(hipEventRecord(ev0, st));
    if (any_multi && ALN_W == 8)
      hipLaunchKernelGGL(align_wave_kernel<8>, dim3((unsigned)np), dim3(64 * 8), 0, st, (const AlnPair*)d_pairs,
                         (const uint8_t*)d_q, (const uint8_t*)d_t, (int)m, (const int8_t*)d_mat, gm, (int32_t*)d_ws,
                         (uint8_t*)d_dir, (uint32_t*)d_cig, (int32_t*)d_sc, (int32_t*)d_nc, (int32_t*)d_abort);
    else if (any_multi)
      hipLaunchKernelGGL(align_wave_kernel<4>, dim3((unsigned)np), dim3(64 * 4), 0, st, (const AlnPair*)d_pairs,
                         (const uint8_t*)d_q, (const uint8_t*)d_t, (int)m, (const int8_t*)d_mat, gm, (int32_t*)d_ws,
                         (uint8_t*)d_dir, (uint32_t*)d_cig, (int32_t*)d_sc, (int32_t*)d_nc, (int32_t*)d_abort);
    else
      hipLaunchKernelGGL(align_wave_kernel<1>, dim3((unsigned)np), dim3(64), 0, st, (const AlnPair*)d_pairs,
                         (const uint8_t*)d_q, (const uint8_t*)d_t, (int)m, (const int8_t*)d_mat, gm, (int32_t*)d_ws,
                         (uint8_t*)d_dir, (uint32_t*)d_cig, (int32_t*)d_sc, (int32_t*)d_nc, (int32_t*)d_abort);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev1, st));
    if (any_multi) {
      int32_t ab = 0;
      HIPCHK(hipMemcpyAsync(&ab, d_abort, sizeof ab, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (ab) {   // a wavefront gave up waiting for its neighbour (never seen): the chunk again, one wavefront per pair
        fprintf(stderr, "[svdss] realignment: a multi-wavefront pair did not finish; the batch runs again with one wavefront per pair\n");
        multi = false;
        ++b->info[3];
        b->cells -= [&] { int64_t c = 0; for (const AlnPair& a : hp) c += (int64_t)a.ql * a.tl; return c; }();
        for (int64_t k = start; k < end; ++k) cig_at[(size_t)k] = {0, 0};
        continue;   // (same `start`: the chunk is laid out again with waves = 1)
      }
    }
    ++b->info[0];
    for (const AlnPair& a : hp) {
      b->info[1] += a.waves > 1;
      b->band[0] += band_steps[(size_t)(start + a.slot)];
      b->band[1] += full_steps[(size_t)(start + a.slot)];
      b->band[2] += a.band.mode == ALN_ONE_BAND;
      b->band[3] += a.band.mode == ALN_CARRY;
    }
    b->info[2] = std::max<int64_t>(b->info[2], any_multi ? ALN_W : 1);
    chunk_cigs.emplace_back((size_t)cig);
    HIPCHK(hipMemcpyAsync(&b->scores[(size_t)start], d_sc, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&h_nc[(size_t)start], d_nc, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, st));
    if (cig) HIPCHK(hipMemcpyAsync(chunk_cigs.back().data(), d_cig, sizeof(uint32_t) * (size_t)cig, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    b->kernel_ms += ms;
    start = end;
  }
  {
    int64_t total = 0;
    for (int64_t k = 0; k < n_pairs; ++k) total += h_nc[(size_t)k];
    b->cigar.resize((size_t)total);
    int64_t o = 0;
    for (int64_t k = 0; k < n_pairs; ++k) {
      const int32_t nc = h_nc[(size_t)k];
      b->n_cigar[(size_t)k] = nc;
      const uint32_t* src = chunk_cigs[(size_t)cig_at[(size_t)k].second].data() + cig_at[(size_t)k].first;
      for (int x = nc - 1; x >= 0; --x) b->cigar[(size_t)o++] = src[x];  // reverse (ksw_backtrack tail)
    }
  }
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  b->total_cigar = (int64_t)b->cigar.size();
  return SVDSS_OK;
}

extern "C" int64_t svdss_aln_batch_npairs(const svdss_aln_batch_t* b) { return b ? b->n_pairs : -1; }
extern "C" int64_t svdss_aln_batch_total_cigar(const svdss_aln_batch_t* b) { return b ? b->total_cigar : -1; }
extern "C" int64_t svdss_aln_batch_cells(const svdss_aln_batch_t* b) { return b ? b->cells : -1; }
extern "C" double svdss_aln_batch_kernel_ms(const svdss_aln_batch_t* b) { return b ? b->kernel_ms : -1.0; }

extern "C" int svdss_aln_batch_launch_info(const svdss_aln_batch_t* b, int64_t out[4]) {
  if (!b || !out) return SVDSS_EINVAL;
  memcpy(out, b->info, sizeof b->info);
  return SVDSS_OK;
}

extern "C" int svdss_aln_batch_band_info(const svdss_aln_batch_t* b, int64_t out[4]) {
  if (!b || !out) return SVDSS_EINVAL;
  memcpy(out, b->band, sizeof b->band);
  return SVDSS_OK;
}

extern "C" int svdss_aln_batch_fetch(const svdss_aln_batch_t* b, int32_t* scores, int64_t* n_cigar,
                                     uint32_t* cigar) {
  if (!b) return SVDSS_EINVAL;
  if (scores) memcpy(scores, b->scores.data(), sizeof(int32_t) * b->scores.size());
  if (n_cigar) memcpy(n_cigar, b->n_cigar.data(), sizeof(int64_t) * b->n_cigar.size());
  if (cigar) memcpy(cigar, b->cigar.data(), sizeof(uint32_t) * b->cigar.size());
  return SVDSS_OK;
}

extern "C" void svdss_aln_batch_free(svdss_aln_batch_t* b) { delete b; }

// the kernel of the calling thread's last svdss_indel_ratio_batch that launched one: 0 bit-parallel, 1 diagonals in LDS,
// 2 diagonals in HBM, -1 none yet
static thread_local int32_t g_ratio_last_kernel = -1;
extern "C" int32_t svdss_indel_ratio_last_kernel(void) { return g_ratio_last_kernel; }

extern "C" int svdss_indel_ratio_batch(const uint8_t* a, const int64_t* a_off, const uint8_t* bsy,
                                       const int64_t* b_off, int64_t n_pairs, int32_t device,
                                       double* ratio_out, int64_t* lcs_out) {
  if (n_pairs < 0 || device < 0) return SVDSS_EINVAL;
  if (n_pairs == 0) return SVDSS_OK;
  if (!a || !a_off || !bsy || !b_off || !ratio_out) return SVDSS_EINVAL;
  HIPCHK(hipSetDevice(device));
  std::vector<LcsPair> hp((size_t)n_pairs);
  int64_t ws = 0, la_max = 0, lb_max = 0;
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int64_t la = a_off[i + 1] - a_off[i], lb = b_off[i + 1] - b_off[i];
    if (la < 0 || lb < 0) return SVDSS_EINVAL;
    if (la >= (1 << 30) || lb >= (1 << 30)) return SVDSS_ERANGE;
    hp[(size_t)i].a_off = a_off[i] - a_off[0];
    hp[(size_t)i].b_off = b_off[i] - b_off[0];
    hp[(size_t)i].ws_off = ws;
    hp[(size_t)i].la = (int32_t)la;
    hp[(size_t)i].lb = (int32_t)lb;
    ws += 3 * (la + 1);
    if (la > la_max) la_max = la;
    if (lb > lb_max) lb_max = lb;
  }
  const int64_t atot = a_off[n_pairs] - a_off[0], btot = b_off[n_pairs] - b_off[0];
  // workspace of the calling thread, kept between calls (no hipMalloc / hipFree -- a device-wide synchronisation
  // each); the stream is the call's one lease of the call side's pool (call_streams.h): nothing on the default stream
  struct RatioState {
    int device = -1;
    DevArena arena;
  };
  static thread_local RatioState R;
  if (R.device != device) {
    R.arena.drop();
    R.device = device;
  }
  CallStreamLease lease;
  HIPCHK(lease.acquire(device));
  const hipStream_t st = lease.get();
  HIPCHK(R.arena.reserve(DevArena::padded((size_t)atot) + DevArena::padded((size_t)btot) +
                          DevArena::padded(sizeof(LcsPair) * (size_t)n_pairs) + DevArena::padded(sizeof(int32_t) * (size_t)ws) +
                          DevArena::padded(sizeof(int64_t) * (size_t)n_pairs) + DevArena::padded(sizeof(double) * (size_t)n_pairs) +
                          DevArena::padded(256)));
  struct { void* p; } d_a{R.arena.take((size_t)atot)}, d_b{R.arena.take((size_t)btot)},
      d_pairs{R.arena.take(sizeof(LcsPair) * (size_t)n_pairs)}, d_ws{R.arena.take(sizeof(int32_t) * (size_t)ws)},
      d_lcs{R.arena.take(sizeof(int64_t) * (size_t)n_pairs)}, d_ratio{R.arena.take(sizeof(double) * (size_t)n_pairs)};
  if (atot) HIPCHK(hipMemcpyAsync(d_a.p, a + a_off[0], (size_t)atot, hipMemcpyHostToDevice, st));
  if (btot) HIPCHK(hipMemcpyAsync(d_b.p, bsy + b_off[0], (size_t)btot, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_pairs.p, hp.data(), sizeof(LcsPair) * (size_t)n_pairs, hipMemcpyHostToDevice, st));
  // the bit-parallel kernel takes batches over at most 8 distinct symbols whose shorter strings fit 64 x 64 bits
  bool bits_ok = !getenv("SVDSS_RATIO_DP");
  uint8_t sym_id[256];
  if (bits_ok) {
    for (int64_t i = 0; i < n_pairs && bits_ok; ++i) bits_ok = std::min(hp[(size_t)i].la, hp[(size_t)i].lb) <= 4096;
    uint8_t any = 0;
    for (int64_t i = 0; i < atot; ++i) any |= a[a_off[0] + i];
    for (int64_t i = 0; i < btot; ++i) any |= bsy[b_off[0] + i];
    memset(sym_id, 255, sizeof sym_id);
    if (any < 8) {
      for (int k = 0; k < 8; ++k) sym_id[k] = (uint8_t)k;
    } else if (bits_ok) {
      bool seen[256] = {false};
      for (int64_t i = 0; i < atot; ++i) seen[a[a_off[0] + i]] = true;
      for (int64_t i = 0; i < btot; ++i) seen[bsy[b_off[0] + i]] = true;
      int nd = 0;
      for (int c = 0; c < 256; ++c)
        if (seen[c]) { if (nd < 8) sym_id[c] = (uint8_t)nd; ++nd; }
      if (nd > 8) bits_ok = false;
    }
  }
  if (bits_ok) {
    void* d_map = R.arena.take(256);
    HIPCHK(hipMemcpyAsync(d_map, sym_id, 256, hipMemcpyHostToDevice, st));
    g_ratio_last_kernel = 0;
    hipLaunchKernelGGL(lcs_bits_kernel, dim3((unsigned)n_pairs), dim3(64), 0, st, (const LcsPair*)d_pairs.p,
                       (const uint8_t*)d_a.p, (const uint8_t*)d_b.p, (const uint8_t*)d_map, (int64_t*)d_lcs.p, (double*)d_ratio.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ratio_out, d_ratio.p, sizeof(double) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
    if (lcs_out) HIPCHK(hipMemcpyAsync(lcs_out, d_lcs.p, sizeof(int64_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // (sym_id is a local: the copy must have left it)
    return SVDSS_OK;
  }
  const size_t lds_need = sizeof(int32_t) * 3 * (size_t)(la_max + 1) + (size_t)la_max + (size_t)lb_max + 16;
  if (lds_need <= 150 * 1024) {
    HIPCHK(hipFuncSetAttribute((const void*)lcs_ratio_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_need));
    g_ratio_last_kernel = 1;
    hipLaunchKernelGGL(lcs_ratio_kernel<true>, dim3((unsigned)n_pairs), dim3(DP_THREADS), lds_need, st,
                       (const LcsPair*)d_pairs.p, (const uint8_t*)d_a.p, (const uint8_t*)d_b.p, (int32_t*)d_ws.p,
                       (int64_t*)d_lcs.p, (double*)d_ratio.p);
  } else {
    g_ratio_last_kernel = 2;
    hipLaunchKernelGGL(lcs_ratio_kernel<false>, dim3((unsigned)n_pairs), dim3(DP_THREADS), 0, st,
                       (const LcsPair*)d_pairs.p, (const uint8_t*)d_a.p, (const uint8_t*)d_b.p, (int32_t*)d_ws.p,
                       (int64_t*)d_lcs.p, (double*)d_ratio.p);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ratio_out, d_ratio.p, sizeof(double) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
  if (lcs_out) HIPCHK(hipMemcpyAsync(lcs_out, d_lcs.p, sizeof(int64_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return SVDSS_OK;
}
