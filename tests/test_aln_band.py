"""The planner of the realignment's diagonal bands (svdss_amd/csrc/aln_band.h) on the CPU, against the oracle: the lower
bound is the score of an alignment that exists, the diagonal bound holds for arbitrary alignments, the oracle's own path
stays inside what the plan computes, parameters outside the proof plan the full matrix, and three plans pinned by hand."""
import functools

import numpy as np
import pytest

from tests import aln_band_lib as A
from tests import calldp_cases as K
from tests import oracle_lib as O
from tests.mirror import caller

MAT = caller.KSW_MAT
GM = (caller.GAPO, caller.GAPE, caller.GAPO2, caller.GAPE2)
KINDS = K.MATRIX_KINDS + ("extreme",)


def op(ln, code):
    return (ln << 4) | code


def slb_cigar(p, ql, tl):
    """the alignment the header says scores S_lb: one gap run of |ql - tl| in front of position x"""
    n, k = min(ql, tl), abs(ql - tl)
    if k == 0:
        return [op(n, 0)]
    c = [op(p.x, 0)] if p.x else []
    c.append(op(k, 1 if ql > tl else 2))
    if n - p.x:
        c.append(op(n - p.x, 0))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """(q, t, mat, gm, oracle score, oracle cigar) over every gap model and matrix kind: small pairs with and without an
    indel, pairs of a few hundred symbols with one indel just above the carry threshold or far above it, unrelated pairs"""
    out = []
    rng = np.random.default_rng(4242)
    for gi, gm in enumerate(K.GAP_MODELS):
        for kind in KINDS:
            m = 5 if (gi + len(kind)) % 2 else 4
            mat = K.matrix(kind, m, rng)
            pairs = [K.small_pair(rng, m, indel) for indel in (False, True, True)]
            t = rng.integers(0, m, size=int(rng.integers(150, 400))).astype(np.uint8)
            pairs.append((K.resized(rng, t, len(t) + int(rng.integers(130, 300)), m=m), t))
            pairs.append((K.resized(rng, t, max(1, len(t) - int(rng.integers(130, 149))), m=m), t))
            # (symbols 0..3: the N of a five-symbol "match" matrix scores 0 and would widen the bands)
            t4 = rng.integers(0, 4, size=int(rng.integers(150, 400))).astype(np.uint8)
            big = rng.integers(0, 4, size=int(rng.integers(900, 1200))).astype(np.uint8)
            pairs.append((K.resized(rng, t4, len(t4) + int(rng.integers(500, 800)), sub=0.0), t4))
            pairs.append((K.resized(rng, big, len(big) - int(rng.integers(500, 800)), sub=0.0), big))
            pairs.append((t.copy(), t))
            pairs.append((rng.integers(0, m, size=int(rng.integers(1, 200))).astype(np.uint8), t))
            for q, t_ in pairs:
                s, c = O.ksw_extd2_global(q, t_, mat, *gm)
                out.append((q, t_, mat, gm, s, c.tolist()))
    return out


def test_lower_bound_is_the_score_of_its_alignment():
    n_gap = 0
    for q, t, mat, gm, s, _ in cases():
        p = A.plan(q, t, mat, gm)
        if not p.provable:
            assert p.mode == A.FULL
            continue
        assert p.slb == O.cigar_score(q, t, mat, slb_cigar(p, len(q), len(t)), *gm), (len(q), len(t), gm)
        assert p.slb <= s
        n_gap += len(q) != len(t)
    assert n_gap > 50


def random_cigar(rng, ql, tl):
    """a random path from (0, 0) to (tl, ql): M, I and D runs that use up both sequences exactly"""
    i = j = 0
    ops = []
    while i < tl or j < ql:
        code = int(rng.integers(0, 3))
        if code == 0 and i < tl and j < ql:
            ln = int(rng.integers(1, min(tl - i, ql - j) + 1))
            i, j = i + ln, j + ln
        elif code == 1 and j < ql:
            ln = int(rng.integers(1, ql - j + 1))
            j += ln
        elif code == 2 and i < tl:
            ln = int(rng.integers(1, tl - i + 1))
            i += ln
        else:
            continue
        if ops and ops[-1][1] == code:
            ops[-1][0] += ln
        else:
            ops.append([ln, code])
    return [op(ln, code) for ln, code in ops]


def test_diagonal_bound_holds_for_arbitrary_alignments():
    rng = np.random.default_rng(77)
    n = 0
    for gm in K.GAP_MODELS:
        for kind in KINDS:
            mat = K.matrix(kind, 4, rng)
            for _ in range(40):
                ql, tl = int(rng.integers(1, 25)), int(rng.integers(1, 25))
                q = rng.integers(0, 4, size=ql).astype(np.uint8)
                t = rng.integers(0, 4, size=tl).astype(np.uint8)
                if not A.plan(q, t, mat, gm).provable:
                    continue
                cg = random_cigar(rng, ql, tl)
                score = O.cigar_score(q, t, mat, cg, *gm)
                match, runs = A.walk(cg)
                for d in match | {r[1] for r in runs} | {r[2] for r in runs}:
                    assert A.f(d, ql, tl, mat, gm) >= score, (gm, kind, ql, tl, d, cg)
                    n += 1
    assert n > 2000


def test_oracle_path_stays_inside_the_plan():
    n_carry = n_band = 0
    for q, t, mat, gm, _, cg in cases():
        for level in (1, 2):
            p = A.plan(q, t, mat, gm, level)
            if p.mode == A.FULL:
                continue
            match, runs = A.walk(cg)
            for d in match | {r[1] for r in runs} | {r[2] for r in runs}:
                assert A.live(d, p), (len(q), len(t), gm, p, d)
            for r in runs:                       # a run's own cells: inside the hull, every one of them
                assert p.lo <= min(r[1], r[2]) and max(r[1], r[2]) <= p.hi
            if p.mode == A.CARRY:
                assert level == 2 and p.c2 - p.c1 - 1 >= 128
                crossing = [r for r in runs if min(r[1], r[2]) <= p.c1 and max(r[1], r[2]) >= p.c2]
                touching = [r for r in runs if any(p.c1 < d < p.c2 for d in (range(r[1] + 1, r[2] + 1) if r[0] == 1 else range(r[2], r[1])))]
                assert len(crossing) == 1 and touching == crossing, (p, runs)
                assert crossing[0][0] == (1 if len(q) > len(t) else 2)
                n_carry += 1
            else:
                n_band += 1
    # the two long indels without substitutions under a "match" matrix carry their gap whenever opening one costs
    # anything: six of the seven gap models, g(d) + g(D - d) > g(D) for every d in between
    assert n_carry >= 12 and n_band > 100


def test_parameters_outside_the_proof_plan_the_full_matrix():
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, size=300).astype(np.uint8)
    q = K.resized(rng, t, 500)
    neg = np.full(16, -3, dtype=np.int8)
    zero = np.where(np.eye(4, dtype=bool), 0, -4).astype(np.int8).reshape(-1)
    for mat, gm in ((neg, GM), (zero, GM), (MAT, (-1, 2, 41, 1)), (MAT, (16, -2, 41, 1)), (MAT, (16, 2, -41, 1)), (MAT, (16, 2, 41, -1))):
        p = A.plan(q, t, mat, gm)
        assert p.mode == A.FULL and not p.provable
        assert (p.lo, p.hi) == (-len(t), len(q)) and p.steps == p.full
        assert all(A.live(d, p) for d in range(p.lo, p.hi + 1))
    assert A.plan(q, t, MAT, GM, level=0).mode == A.FULL
    assert A.plan(q, t, MAT, GM).mode == A.CARRY
    assert A.plan(q[:0], t, MAT, GM).mode == A.FULL


def test_hand_pinned_plans():
    rng = np.random.default_rng(9)
    t = rng.integers(0, 4, size=600).astype(np.uint8)
    p = A.plan(t, t, MAT, GM)
    assert (p.lo, p.hi, p.mode, p.slb) == (0, 0, A.ONE_BAND, 600)
    assert p.steps < p.full // 4
    # one insertion of 1,000: 600 - g(1000) = 600 - 1041; nothing between the two diagonals can carry a match
    q = np.concatenate([t[:300], rng.integers(0, 4, size=1000).astype(np.uint8), t[300:]])
    p = A.plan(q, t, MAT, GM)
    assert (p.lo, p.c1, p.c2, p.hi, p.mode) == (0, 0, 1000, 1000, A.CARRY)
    assert p.slb == 600 - 1041 and 290 <= p.x <= 300
    one = A.plan(q, t, MAT, GM, level=1)
    assert (one.lo, one.hi, one.mode) == (0, 1000, A.ONE_BAND)
    assert p.steps < one.steps < p.full
    # ... and the deletion the other way round
    p = A.plan(t, q, MAT, GM)
    assert (p.lo, p.c1, p.c2, p.hi, p.mode) == (-1000, -1000, 0, 0, A.CARRY)
    # an indel of 100: the interior is narrower than a wavefront's spread of diagonals, one band
    q = np.concatenate([t[:300], rng.integers(0, 4, size=100).astype(np.uint8), t[300:]])
    p = A.plan(q, t, MAT, GM)
    assert (p.lo, p.hi, p.mode) == (0, 100, A.ONE_BAND)


def test_substitutions_turn_a_carried_gap_into_one_band():
    """an indel of 129 leaves exactly 128 dead diagonals; two substitutions (10 each off S_lb) make diagonals 1 and 128
    live, g(1) + g(128) = 187 <= g(129) + 20, and the pair keeps one band"""
    rng = np.random.default_rng(3)
    t = rng.integers(0, 4, size=600).astype(np.uint8)
    long_ = np.concatenate([t[:300], rng.integers(0, 4, size=129).astype(np.uint8), t[300:]])
    for k in range(4):
        sub = t.copy()
        sub[[10, 40, 500][:k]] = (sub[[10, 40, 500][:k]] + 1) % 4
        for q, t_ in ((long_, sub), (sub, long_)):
            p = A.plan(q, t_, MAT, GM)
            assert p.slb == 600 - 170 - 10 * k
            assert p.mode == (A.CARRY if k < 2 else A.ONE_BAND), (k, p)
            if k < 2:
                assert p.c2 - p.c1 - 1 == 128


def test_stripe_steps_cover_every_live_cell():
    """every live cell of a stripe is in an executed step, and a jump skips two steps or more"""
    rng = np.random.default_rng(11)
    for ql, tl in ((1600, 600), (600, 1600), (700, 700), (900, 650), (10, 900), (900, 10), (257, 129)):
        t = rng.integers(0, 4, size=tl).astype(np.uint8)
        q = K.resized(rng, t, ql, sub=0.0)
        for level in (1, 2):
            p = A.plan(q, t, MAT, GM, level)
            total = 0
            for s in range((tl + 63) // 64):
                (a0, e0), (a1, e1) = A.stripe_steps(ql, tl, s, p)
                rows = min(64, tl - 64 * s)
                assert 0 <= a0 <= e0 <= ql + rows - 1 and a0 % 64 == 0
                if a1 < e1:
                    assert a1 >= e0 + 2 and a1 % 64 == 0 and e1 <= ql + rows - 1
                total += (e0 - a0) + max(0, e1 - a1)
                for lane in range(rows):
                    i = 64 * s + lane
                    js = np.arange(ql)
                    lv = np.array([A.live(int(j) - i, p) for j in (js if ql < 300 else js[::7])])
                    tau = (js if ql < 300 else js[::7])[lv] + lane
                    assert (((tau >= a0) & (tau < e0)) | ((tau >= a1) & (tau < e1))).all(), (ql, tl, s, lane)
            assert total == p.steps


@pytest.mark.parametrize("level", [1, 2])
def test_bench_like_batch_plans_most_of_the_work_away(level):
    """pairs as `SVDSS call` produces them: the window against itself, or with one long indel"""
    rng = np.random.default_rng(13)
    steps = full = 0
    for k in range(24):
        t = rng.integers(0, 4, size=int(rng.integers(600, 1700))).astype(np.uint8)
        q = t.copy() if k % 3 == 0 else K.resized(rng, t, len(t) + (-1) ** k * int(rng.integers(150, 500)), sub=0.002)
        p = A.plan(q, t, MAT, GM, level)
        steps, full = steps + p.steps, full + p.full
    assert steps < (0.75 if level == 1 else 0.45) * full
