"""Every launch shape of the call-side DP (svdss_amd/csrc/call_dp.hip) against the oracle, bit for bit: the wave counts
of align_wave_kernel (<1>, <4>, <8>), the launch of a product-sized batch that mixes one- and several-wavefront pairs,
several chunks, the stripe / block edges, unbalanced pairs, other scoring parameters, a reused batch object, and the
three LCS kernels at their dispatch edges.  Each test first asserts, through svdss_aln_batch_launch_info /
svdss_indel_ratio_last_kernel, that the path it was written for is the one that ran.

The oracle times in the docstrings are those of the test's own oracle calls on one core of the build machine."""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np
import pytest

from svdss_amd._lib import check, lib
from svdss_amd.pingpong import pack_reads
from tests import calldp_cases as K
from tests import oracle_lib as O
from tests.mirror import caller

pytestmark = pytest.mark.gpu
MAT = caller.KSW_MAT
GM = (caller.GAPO, caller.GAPE, caller.GAPO2, caller.GAPE2)
KNOBS = ("SVDSS_ALIGN_WAVES", "SVDSS_ALIGN_FRAC", "SVDSS_ALIGN_DIR_MB", "SVDSS_RATIO_DP")
# setting -> (environment, the W launch_info must report when the batch has a pair of 8 stripes or more)
WAVES = {"default": ({}, 4), "one": ({"SVDSS_ALIGN_WAVES": "1"}, 1), "eight": ({"SVDSS_ALIGN_WAVES": "8"}, 8)}

Result = namedtuple("Result", "scores cigars npairs cells total_cigar info")


def under(env, fn, *args, **kw):
    """fn(*args) with exactly `env` of the library's call-side knobs set; the environment is put back afterwards"""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        return fn(*args, **kw)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class Batch:
    """one svdss_aln_batch_t over the C-ABI, kept between calls"""

    def __init__(self):
        self.h = C.c_void_p()

    def run(self, qs, ts, mat=MAT, gm=GM):
        q, qo = pack_reads(list(qs))
        t, to = pack_reads(list(ts))
        n = len(qo) - 1
        assert len(to) - 1 == n
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        m = int(round(len(mat) ** 0.5))
        check(lib.svdss_align_global_batch(q.ctypes.data, qo.ctypes.data, t.ctypes.data, to.ctypes.data, n, m,
                                           mat.ctypes.data, *gm, 0, C.byref(self.h)), "svdss_align_global_batch")
        npairs, total = lib.svdss_aln_batch_npairs(self.h), lib.svdss_aln_batch_total_cigar(self.h)
        scores = np.zeros(npairs, dtype=np.int32)
        nc = np.zeros(npairs, dtype=np.int64)
        cg = np.zeros(total, dtype=np.uint32)
        check(lib.svdss_aln_batch_fetch(self.h, scores.ctypes.data, nc.ctypes.data, cg.ctypes.data), "svdss_aln_batch_fetch")
        info = np.full(4, -1, dtype=np.int64)
        check(lib.svdss_aln_batch_launch_info(self.h, info.ctypes.data), "svdss_aln_batch_launch_info")
        assert int(nc.sum()) == total
        cg, ends = cg.tolist(), np.cumsum(nc).tolist()
        cigars = [cg[e - k:e] for e, k in zip(ends, nc.tolist())]
        return Result(scores.tolist(), cigars, npairs, lib.svdss_aln_batch_cells(self.h), total, info.tolist())

    def close(self):
        if self.h:
            lib.svdss_aln_batch_free(self.h)
            self.h = C.c_void_p()


def run(qs, ts, mat=MAT, gm=GM, env=None):
    """one batch on a fresh batch object, under `env`"""
    b = Batch()
    try:
        return under(env or {}, b.run, qs, ts, mat, gm)
    finally:
        b.close()


def oracle(qs, ts, mat=MAT, gm=GM):
    out = []
    for q, t in zip(qs, ts):
        s, c = O.ksw_extd2_global(q, t, mat, *gm)
        out.append((s, c.tolist()))
    return out


def n_long(qs, ts):
    """pairs the host may give several wavefronts: eight stripes or more"""
    return sum(1 for q, t in zip(qs, ts) if len(t) >= 8 * 64 and 0 < len(q) < (1 << 20))


def check_result(res, qs, ts, want, mat=MAT, gm=GM):
    assert res.npairs == len(qs)
    for k, (q, t, (es, ec)) in enumerate(zip(qs, ts, want)):
        where = (k, len(q), len(t))
        assert res.scores[k] == es, where
        assert res.cigars[k] == ec, where
        if len(q) and len(t):
            assert O.cigar_score(q, t, mat, res.cigars[k], *gm) == res.scores[k], where
    assert res.cells == sum(len(q) * len(t) for q, t in zip(qs, ts))
    assert res.total_cigar == sum(len(c) for _, c in want)


def check_waves(res, qs, ts, w):
    """the launch the setting stands for is the one that ran: W, the pairs with several wavefronts, no second run"""
    nl = n_long(qs, ts)
    assert nl > 0
    assert res.info[2] == w, res.info
    assert res.info[1] == (nl if w > 1 else 0), res.info
    assert res.info[3] == 0, res.info


def with_n(rng, s, k):
    """symbol 4 (N: scores 0 against everything) at up to k places"""
    s = s.copy()
    if len(s):
        s[rng.integers(0, len(s), size=k)] = 4
    return s


# ------------------------------------------------------------------ (a) the stripe and block grid

@functools.lru_cache(maxsize=None)
def grid():
    rng = np.random.default_rng(101)
    qs, ts = [], []
    for tl in K.STRIPE_EDGE_TL:
        for ql in K.BLOCK_EDGE_QL:
            t = rng.integers(0, 4, size=tl).astype(np.uint8)
            unit = rng.permutation(4)[:3].astype(np.uint8)
            cases = [(K.resized(rng, t, ql), t),
                     (rng.integers(0, 4, size=ql).astype(np.uint8), t),
                     (np.tile(unit, ql // 3 + 2)[int(rng.integers(0, 3)):][:ql], np.tile(unit, tl // 3 + 1)[:tl])]
            for q, t_ in cases:
                if len(qs) % 5 == 4:
                    q, t_ = with_n(rng, q, 2), with_n(rng, t_, 3)
                qs.append(np.ascontiguousarray(q, dtype=np.uint8))
                ts.append(np.ascontiguousarray(t_, dtype=np.uint8))
    return qs, ts, oracle(qs, ts)


@pytest.mark.parametrize("setting", list(WAVES))
def test_stripe_and_block_grid(setting):
    """every tl around a stripe edge x every ql around a block edge x {related, unrelated, period-3 repeat}: 714 pairs,
    26.7 M cells, the same batch under each wave setting.  Oracle: 0.5 s, once for the three settings."""
    qs, ts, want = grid()
    assert len(qs) == 3 * len(K.STRIPE_EDGE_TL) * len(K.BLOCK_EDGE_QL) and any((q == 4).any() for q in qs)
    env, w = WAVES[setting]
    res = run(qs, ts, env=env)
    check_waves(res, qs, ts, w)
    assert res.info[0] == 1
    check_result(res, qs, ts, want)


# ------------------------------------------------------------------ (b) unbalanced pairs

@functools.lru_cache(maxsize=None)
def unbalanced():
    rng = np.random.default_rng(102)
    qs, ts = [], []

    def slices(long_len, short_len):
        a = rng.integers(0, 4, size=long_len).astype(np.uint8)
        for at in (0, (long_len - short_len) // 2, long_len - short_len):
            yield a, a[at:at + short_len].copy()

    for ql in (1, 2, 5, 40, 63, 64, 65):
        for tl in (512, 600, 1500, 2049):
            for t, q in slices(tl, ql):                      # a large deletion
                qs.append(q), ts.append(t)
    for tl in (1, 2, 5, 40):
        for ql in (600, 1500, 2049):
            for q, t in slices(ql, tl):                      # a large insertion
                qs.append(q), ts.append(t)
    return qs, ts, oracle(qs, ts)


@pytest.mark.parametrize("setting", list(WAVES))
def test_unbalanced_pairs(setting):
    """a few bases against a window of up to 2,049 and the reverse, the short side cut from the start, the middle and
    the end of the long one: with several wavefronts and ql < 64 the consumer needs ql columns and the first progress
    announced is 1.  120 pairs, 4 M cells.  Oracle: 0.07 s."""
    qs, ts, want = unbalanced()
    env, w = WAVES[setting]
    res = run(qs, ts, env=env)
    check_waves(res, qs, ts, w)
    check_result(res, qs, ts, want)


# ------------------------------------------------------------------ (c) the product's mixed launch

@functools.lru_cache(maxsize=None)
def product_batch():
    rng = np.random.default_rng(103)
    qs, ts = [], []
    for _ in range(2040):
        t = rng.integers(0, 4, size=int(rng.integers(20, 121))).astype(np.uint8)
        qs.append(K.resized(rng, t, int(rng.integers(20, 121)), sub=0.02)), ts.append(t)
    for _ in range(2):
        t = rng.integers(0, 4, size=1100).astype(np.uint8)
        q = K.resized(rng, K.resized(rng, t, 1060), 1100)     # a deletion and an insertion of 40
        qs.append(q), ts.append(t)
    for tl in (512, 520, 577, 640):
        for ql in (30, 100, 200):
            t = rng.integers(0, 4, size=tl).astype(np.uint8)
            qs.append(K.resized(rng, t, ql)), ts.append(t)
    order = rng.permutation(len(qs)).tolist()
    qs, ts = [qs[i] for i in order], [ts[i] for i in order]
    return qs, ts, oracle(qs, ts)


def test_mixed_launch_of_a_product_sized_batch():
    """2,054 pairs as a bench step has them: from 2,048 pairs on only the pairs within a factor SVDSS_ALIGN_FRAC (8) of
    the largest matrix get several wavefronts, so ONE <4> launch holds 4-wavefront pairs (1,100 x 1,100) and pairs of
    8 to 10 stripes with one wavefront whose three other wavefronts return at once.  Then every long pair with several
    wavefronts (SVDSS_ALIGN_FRAC), the same mix in the <8> launch, and the <1> launch.  13 M cells.  Oracle: 0.3 s."""
    qs, ts, want = product_batch()
    assert len(qs) >= 2048
    nl = n_long(qs, ts)
    big = max(len(q) * len(t) for q, t in zip(qs, ts))
    n_multi = sum(1 for q, t in zip(qs, ts) if len(t) >= 512 and len(q) * len(t) * 8 >= big)
    assert nl == 14 and n_multi == 2
    res = run(qs, ts)
    assert res.info[2] == 4 and 0 < res.info[1] < nl, res.info          # the mix is the point
    assert res.info == [1, n_multi, 4, 0]
    check_result(res, qs, ts, want)
    res = run(qs, ts, env={"SVDSS_ALIGN_FRAC": "1000000"})
    assert res.info == [1, nl, 4, 0]
    check_result(res, qs, ts, want)
    res = run(qs, ts, env={"SVDSS_ALIGN_WAVES": "8"})
    assert res.info == [1, n_multi, 8, 0]
    check_result(res, qs, ts, want)
    res = run(qs, ts, env={"SVDSS_ALIGN_WAVES": "1"})
    assert res.info == [1, 0, 1, 0]
    check_result(res, qs, ts, want)


# ------------------------------------------------------------------ (d) chunking

@functools.lru_cache(maxsize=None)
def chunk_batch():
    rng = np.random.default_rng(104)
    qs, ts = [], []
    for k in range(40):
        t = rng.integers(0, 4, size=int(rng.integers(200, 400))).astype(np.uint8)
        qs.append(K.resized(rng, t, int(rng.integers(200, 400)))), ts.append(t)
        if k == 12:
            qs.append(np.zeros(0, np.uint8)), ts.append(t.copy())           # an empty pair
        if k == 20:
            big = rng.integers(0, 4, size=1200).astype(np.uint8)
            qs.append(K.resized(rng, K.resized(rng, big, 1130), 1200)), ts.append(big)
    return qs, ts, oracle(qs, ts)


def test_chunks():
    """SVDSS_ALIGN_DIR_MB=1: 40 pairs of about 300 x 300 (180 KB of direction bytes each) go five or so to a chunk, the
    1,200 x 1,200 pair in the middle (2.9 MB) passes as a chunk of its own, an empty pair sits in another: scores and
    CIGARs come back in the caller's order, the same as from one chunk.  5 M cells.  Oracle: 0.06 s."""
    qs, ts, want = chunk_batch()
    one = run(qs, ts)
    assert one.info[0] == 1
    check_result(one, qs, ts, want)
    for extra in ({}, {"SVDSS_ALIGN_WAVES": "1"}, {"SVDSS_ALIGN_WAVES": "8"}):
        res = run(qs, ts, env=dict(extra, SVDSS_ALIGN_DIR_MB="1"))
        assert res.info[0] >= 5 and res.info[3] == 0, res.info
        assert res.info[2] == (1 if extra.get("SVDSS_ALIGN_WAVES") == "1" else int(extra.get("SVDSS_ALIGN_WAVES", 4)))
        assert res.scores == one.scores and res.cigars == one.cigars
        assert res.cells == one.cells and res.total_cigar == one.total_cigar
        check_result(res, qs, ts, want)


# ------------------------------------------------------------------ (e) scoring parameters

def scoring_pairs(rng, m, n_extra):
    qs, ts = [], []
    for tl in [63, 64, 65, 512, 513] + rng.integers(1, 200, size=n_extra).tolist():
        t = rng.integers(0, m, size=tl).astype(np.uint8)
        ql = max(1, tl + int(rng.integers(-40, 41)))
        q = K.resized(rng, t, ql, m=m, sub=0.05) if rng.random() < 0.8 else rng.integers(0, m, size=ql).astype(np.uint8)
        qs.append(q), ts.append(t)
    return qs, ts


@pytest.mark.parametrize("gm", K.GAP_MODELS, ids=lambda g: "-".join(map(str, g)))
def test_scoring_parameters(gm):
    """m = 4, 5, 8 x {match / mismatch, random int8, random with -128 and 127} under one gap model: 9 batches of 7 pairs
    over the stripe edges 63, 64, 65, 512, 513, symbols up to m - 1 (a row's scores sit as bytes in one 64-bit register),
    each under the three wave settings.  5 M cells.  Oracle: 0.1 s."""
    for m in (4, 5, 8):
        for kind in K.MATRIX_KINDS + ("extreme",):
            rng = np.random.default_rng([105, m, len(kind), K.GAP_MODELS.index(gm)])
            mat = K.matrix(kind, m, rng)
            qs, ts = scoring_pairs(rng, m, 2)
            assert max(int(q.max()) for q in qs) == m - 1
            want = oracle(qs, ts, mat, gm)
            for env, w in WAVES.values():
                res = run(qs, ts, mat, gm, env=env)
                check_waves(res, qs, ts, w)
                check_result(res, qs, ts, want, mat, gm)


# ------------------------------------------------------------------ (f) one batch object, several calls

def test_batch_object_reuse():
    """three calls on one svdss_aln_batch_t -- the grid, three pairs, then a batch with a larger workspace than the
    first (the grid twice and the unbalanced pairs) -- and an empty batch: each as from a fresh object.  The oracle's
    results are those of the tests above."""
    gq, gt, gw = grid()
    uq, ut, uw = unbalanced()
    calls = [(gq, gt, gw), (gq[400:403], gt[400:403], gw[400:403]), (gq + uq + gq[::-1], gt + ut + gt[::-1], gw + uw + gw[::-1])]
    b = Batch()
    try:
        for qs, ts, want in calls:
            res = b.run(qs, ts)
            fresh = run(qs, ts)
            assert res == fresh
            check_result(res, qs, ts, want)
        res = b.run([], [])
        assert res.npairs == 0 and res.total_cigar == 0 and res.cells == 0 and res.info == [0, 0, 0, 0]
        assert lib.svdss_aln_batch_npairs(b.h) == 0 and lib.svdss_aln_batch_total_cigar(b.h) == 0
        qs, ts, want = calls[1]
        check_result(b.run(qs, ts), qs, ts, want)             # and it still works afterwards
    finally:
        b.close()


# ------------------------------------------------------------------ (g) LCS ratio

BITS, LDS, HBM = 0, 1, 2


def ratio(a_list, b_list, env=None):
    """(ratio, lcs, the kernel that ran)"""
    def go():
        r, l = caller.fuzz_ratio(a_list, b_list)
        return r.tolist(), l.tolist(), lib.svdss_indel_ratio_last_kernel()
    return under(env or {}, go)


def check_ratio(got, a_list, b_list, kernel):
    r, l, k = got
    assert k == kernel
    for a, b, rr, ll in zip(a_list, b_list, r, l):
        assert ll == O.lcs(a, b), (len(a), len(b))
        assert rr == O.fuzz_ratio(a, b), (len(a), len(b))


def edited(rng, a, syms, n_edit):
    b = np.frombuffer(a, dtype=np.uint8).copy()
    for _ in range(n_edit):
        if len(b):
            b[int(rng.integers(0, len(b)))] = rng.choice(syms)
    if len(b) > 20:
        at = int(rng.integers(0, len(b) - 10))
        b = np.delete(b, slice(at, at + int(rng.integers(1, 10))))
    return bytes(b)


def small_ratio_pairs(rng, syms, n, max_len=300):
    a_list, b_list = [], []
    for k in range(n):
        a = bytes(rng.choice(syms, size=int(rng.integers(0, max_len))).astype(np.uint8))
        b = edited(rng, a, syms, 5) if k % 3 else bytes(rng.choice(syms, size=int(rng.integers(0, max_len))).astype(np.uint8))
        a_list.append(a), b_list.append(b)
    return a_list, b_list


SYMS9 = np.array([0, 1, 65, 67, 71, 78, 84, 200, 255], dtype=np.uint8)


def test_ratio_diagonals_in_hbm():
    """lcs_ratio_kernel<false>: 12,800 bytes against 150 (12 * 12,801 + 12,800 + 150 + 16 bytes of LDS would be 163 KB)
    and the pair swapped, beside small pairs whose workspace lies behind theirs; over 9 symbols, and over 4 with
    SVDSS_RATIO_DP=1.  2 x 1.9 M cells per batch.  Oracle: 0.05 s."""
    rng = np.random.default_rng(106)
    for syms, env in ((SYMS9, {}), (SYMS9[[0, 2, 7, 8]], {"SVDSS_RATIO_DP": "1"})):
        a = bytes(rng.choice(syms, size=12800).astype(np.uint8))
        at = int(rng.integers(0, 12800 - 162))
        b = edited(rng, a[at:at + 162], syms, 8)[:150]
        assert len(b) == 150 and len(set(a)) == len(syms)
        sa, sb = small_ratio_pairs(rng, syms, 6)
        a_list, b_list = sa[:3] + [a, b] + sa[3:], sb[:3] + [b, a] + sb[3:]
        check_ratio(ratio(a_list, b_list, env), a_list, b_list, HBM)


def test_ratio_dispatch_edges():
    """8 distinct byte values (0 and 255 among them): bit-parallel; one byte of a ninth: the diagonals; a shorter string of
    exactly 4,096: bit-parallel; one pair of 4,097 x 4,097 more: the diagonals for the whole batch.  92 M cells.
    Oracle: 0.9 s."""
    rng = np.random.default_rng(107)
    syms = SYMS9[[0, 1, 2, 3, 4, 6, 7, 8]]
    a_list, b_list = small_ratio_pairs(rng, syms, 20)
    assert len(set(b"".join(a_list + b_list))) == 8
    check_ratio(ratio(a_list, b_list), a_list, b_list, BITS)
    a9, b9 = a_list + [a_list[1]], b_list + [b_list[1] + bytes([int(SYMS9[5])])]
    check_ratio(ratio(a9, b9), a9, b9, LDS)
    p = bytes(rng.choice(syms, size=4096).astype(np.uint8))
    x = bytes(rng.choice(syms, size=700).astype(np.uint8))
    al, bl = a_list + [p, x + edited(rng, p, syms, 40)], b_list + [edited(rng, p, syms, 40) + x, p]
    assert min(len(al[-1]), len(bl[-1])) == 4096 == min(len(al[-2]), len(bl[-2])) and len(bl[-2]) > 4096 < len(al[-1])
    al, bl = al + [p, p], bl + [p + x, p]                     # shorter side 4,096 on the left, and both sides
    check_ratio(ratio(al, bl), al, bl, BITS)
    p1 = p + bytes([int(syms[3])])
    q1 = edited(rng, p1, syms, 60)
    q1 = q1 + bytes(rng.choice(syms, size=4097 - len(q1)).astype(np.uint8))
    al, bl = al + [p1], bl + [q1]
    assert len(p1) == len(q1) == 4097
    check_ratio(ratio(al, bl), al, bl, LDS)


def test_ratio_lds_to_hbm_edge():
    """the largest batch the LDS kernel takes and the smallest it does not: 12 (la_max + 1) + la_max + lb_max + 16 bytes
    against 150 KB, la_max = 11,805 and lb_max = 107 (153,600: LDS) / 108 (153,601: HBM).  2 x 1.3 M cells.
    Oracle: 0.02 s."""
    rng = np.random.default_rng(108)
    la = 11805
    a = bytes(rng.choice(SYMS9, size=la).astype(np.uint8))
    sa, sb = small_ratio_pairs(rng, SYMS9, 5, max_len=100)
    for lb, kernel in ((107, LDS), (108, HBM)):
        assert (12 * (la + 1) + la + lb + 16 <= 150 * 1024) == (kernel == LDS)
        b = edited(rng, a[5000:5000 + lb + 12], SYMS9, 6)[:lb]
        assert len(b) == lb
        a_list, b_list = sa + [a], sb + [b]
        check_ratio(ratio(a_list, b_list), a_list, b_list, kernel)
