"""Realignment over the diagonals an optimal alignment can cross (svdss_amd/csrc/aln_band.h, align_wave_kernel): scores and
CIGARs bit for bit against the oracle under SVDSS_ALIGN_BAND 0 / 1 / 2 and SVDSS_ALIGN_WAVES default / 1 / 8, and through
svdss_aln_batch_band_info that the path a case was written for is the one that ran.

The cases are built and aligned by the oracle once (about two seconds) and shared by all tests."""
import functools
import os

import numpy as np
import pytest

from svdss_amd._lib import check, lib
from tests import aln_band_lib as A
from tests.mirror import caller
from tests.test_call_dp_shapes_gpu import Batch, check_result, oracle, with_n

pytestmark = pytest.mark.gpu
MAT = caller.KSW_MAT
KNOBS = ("SVDSS_ALIGN_BAND", "SVDSS_ALIGN_WAVES", "SVDSS_ALIGN_FRAC", "SVDSS_ALIGN_DIR_MB")
BANDS = ("0", "1", "2")
WAVES = {"default": {}, "one": {"SVDSS_ALIGN_WAVES": "1"}, "eight": {"SVDSS_ALIGN_WAVES": "8"}}
INDEL_LENGTHS = (1, 24, 25, 26, 63, 64, 65, 127, 128, 129, 500, 1000)


def run(qs, ts, env, batch=None):
    """-> (Result, band_info) of one call under exactly `env` of the realignment's knobs"""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    b = batch or Batch()
    try:
        res = b.run(qs, ts)
        info = np.full(4, -1, dtype=np.int64)
        check(lib.svdss_aln_batch_band_info(b.h, info.ctypes.data), "svdss_aln_batch_band_info")
        return res, info.tolist()
    finally:
        if batch is None:
            b.close()
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def indel_pair(rng, n, ln, where, ins):
    """a window of n symbols and the same with ln more at the start, in the middle or at the end; the longer one is the
    query for an insertion, the target for a deletion"""
    short = rng.integers(0, 4, size=n).astype(np.uint8)
    at = {"start": 0, "middle": n // 2, "end": n}[where]
    long_ = np.concatenate([short[:at], rng.integers(0, 4, size=ln).astype(np.uint8), short[at:]])
    return (long_, short) if ins else (short, long_)


def substituted(rng, q, k):
    q = q.copy()
    at = rng.choice(len(q), size=k, replace=False)
    q[at] = (q[at] + rng.integers(1, 4, size=k)) % 4
    return q


@functools.lru_cache(maxsize=None)
def groups():
    """name -> (qs, ts, oracle results)"""
    rng = np.random.default_rng(2024)
    g = {}

    def put(name, pairs):
        qs = [np.ascontiguousarray(q, dtype=np.uint8) for q, _ in pairs]
        ts = [np.ascontiguousarray(t, dtype=np.uint8) for _, t in pairs]
        g[name] = (qs, ts, oracle(qs, ts))

    ident = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (1, 63, 64, 65, 129, 513, 600)]
    put("identical", [(t.copy(), t) for t in ident])
    # windows of 300 and 600: a deletion's target is n + ln rows, so carried gaps (ln >= 129) are crossed by one wavefront
    # (300 + 129 rows) and by several (512 rows and more)
    put("indels", [indel_pair(rng, n, ln, where, ins) for n in (300, 600) for ln in INDEL_LENGTHS for where in ("start", "middle", "end")
                   for ins in (True, False)])
    # the same indel pairs with 1 .. 6 substitutions (every count with every length), and all six counts on three of them
    wide = [(substituted(rng, q, 1 + (k // 6 + k) % 6), t) for k, (q, t) in enumerate(zip(*g["indels"][:2]))]
    for ln in (26, 129, 500):
        for ins in (True, False):
            q, t = indel_pair(rng, 600, ln, "middle", ins)
            wide += [(substituted(rng, q, k), t) for k in range(1, 7)]
    put("widening", wide)
    ties = []
    left, right = rng.integers(0, 4, size=150).astype(np.uint8), rng.integers(0, 4, size=170).astype(np.uint8)
    for unit in ([2], [0, 3], [1, 0, 2]):
        for few, many in ((10, 30), (5, 140), (0, 200)):
            a = np.concatenate([left, np.tile(np.array(unit, dtype=np.uint8), few), right])
            b = np.concatenate([left, np.tile(np.array(unit, dtype=np.uint8), many), right])
            ties += [(a, b), (b, a)]
    put("ties", ties)
    base = rng.integers(0, 4, size=700).astype(np.uint8)
    x, y = rng.integers(0, 4, size=200).astype(np.uint8), rng.integers(0, 4, size=150).astype(np.uint8)
    two = [(np.concatenate([base[:100], x, base[100:400], y, base[400:]]), base),
           (base, np.concatenate([base[:100], x, base[100:400], y, base[400:]])),
           (np.concatenate([base[:150], x, base[150:450], base[600:]]), base),
           (np.concatenate([base[:150], base[330:500], y, base[500:]]), base)]
    put("two_indels", two)
    sym_n = []
    for ln, ins in ((0, True), (40, True), (300, True), (300, False)):
        q, t = indel_pair(rng, 560, ln, "middle", ins) if ln else (base.copy(), base)
        sym_n += [(with_n(rng, q, 3), with_n(rng, t, 4)), (q, with_n(rng, t, 40))]
    put("symbol_n", sym_n)
    # (128 x 63 and 63 x 128: all gap, the two runs turn into each other on the border's diagonals ql and -tl)
    put("unrelated", [(rng.integers(0, 4, size=a).astype(np.uint8), rng.integers(0, 4, size=b).astype(np.uint8))
                      for a, b in ((1, 1), (70, 70), (300, 300), (520, 520), (700, 700), (128, 63), (63, 128))])
    return g


def everything():
    qs, ts, want = [], [], []
    for name in sorted(groups()):
        q, t, w = groups()[name]
        qs, ts, want = qs + q, ts + t, want + w
    return qs, ts, want


def test_band_info_refuses_null():
    out = np.zeros(4, dtype=np.int64)
    assert lib.svdss_aln_batch_band_info(None, out.ctypes.data) != 0
    b = Batch()
    try:
        b.run([np.zeros(3, np.uint8)], [np.zeros(3, np.uint8)])
        assert lib.svdss_aln_batch_band_info(b.h, None) != 0
    finally:
        b.close()


@pytest.mark.parametrize("waves", sorted(WAVES))
@pytest.mark.parametrize("band", BANDS)
def test_every_case_bit_exact(band, waves):
    qs, ts, want = everything()
    res, info = run(qs, ts, {"SVDSS_ALIGN_BAND": band, **WAVES[waves]})
    check_result(res, qs, ts, want)
    assert res.info[3] == 0 and res.info[2] == {"default": 4, "one": 1, "eight": 8}[waves]
    steps, full, one_band, carried = info
    if band == "0":
        assert steps == full and one_band == 0 and carried == 0
    else:
        assert steps < full and one_band + carried == len(qs)
        assert (carried > 0) == (band == "2")


@pytest.mark.parametrize("band", ("1", "2"))
def test_plan_is_the_one_of_the_header(band):
    """the library takes the two diagonal sums of S_lb from a kernel: the steps it reports are those of the header's own
    plan of every pair (tests/test_aln_band.py holds that plan against the oracle)"""
    qs, ts, _ = everything()
    _, info = run(qs, ts, {"SVDSS_ALIGN_BAND": band})
    plans = [A.plan(q, t, MAT, caller_gm(), int(band)) for q, t in zip(qs, ts)]
    assert info == [sum(p.steps for p in plans), sum(p.full for p in plans), sum(p.mode == A.ONE_BAND for p in plans),
                    sum(p.mode == A.CARRY for p in plans)]


def caller_gm():
    return (caller.GAPO, caller.GAPE, caller.GAPO2, caller.GAPE2)


@pytest.mark.parametrize("band", BANDS)
def test_identical_pairs_run_one_diagonal(band):
    qs, ts, want = groups()["identical"]
    res, (steps, full, one_band, carried) = run(qs, ts, {"SVDSS_ALIGN_BAND": band})
    check_result(res, qs, ts, want)
    if band == "0":
        assert steps == full
    else:
        # per stripe of r rows the band [0, 0] takes 2 r - 1 steps, rounded to blocks of 64 columns at the start
        assert one_band == len(qs) and carried == 0
        assert steps <= sum(((len(t) + 63) // 64) * 128 for t in ts) and steps < full // 2


@pytest.mark.parametrize("waves", sorted(WAVES))
def test_single_indels_carry_their_gap_from_129(waves):
    qs, ts, want = groups()["indels"]
    res2, info2 = run(qs, ts, {"SVDSS_ALIGN_BAND": "2", **WAVES[waves]})
    check_result(res2, qs, ts, want)
    res1, info1 = run(qs, ts, {"SVDSS_ALIGN_BAND": "1", **WAVES[waves]})
    check_result(res1, qs, ts, want)
    n_carry = sum(1 for q, t in zip(qs, ts) if abs(len(q) - len(t)) - 1 >= 128)
    assert info2[3] == n_carry and info2[2] == len(qs) - n_carry     # exact copies plus one indel: the interior is |D| - 1 wide
    assert info1[3] == 0 and info1[2] == len(qs)
    assert info2[0] < info1[0] < info1[1] == info2[1]
    if waves != "one":
        # both one wavefront and several cross a carried gap
        assert any(len(t) < 512 and abs(len(q) - len(t)) >= 129 for q, t in zip(qs, ts))
        assert any(len(t) >= 512 and abs(len(q) - len(t)) >= 129 for q, t in zip(qs, ts))
        assert res2.info[1] == sum(1 for t in ts if len(t) >= 512)


@pytest.mark.parametrize("name", ["widening", "ties", "two_indels", "symbol_n"])
@pytest.mark.parametrize("band", ("1", "2"))
def test_group_prunes_and_stays_exact(name, band):
    qs, ts, want = groups()[name]
    for w in sorted(WAVES):
        res, (steps, full, one_band, carried) = run(qs, ts, {"SVDSS_ALIGN_BAND": band, **WAVES[w]})
        check_result(res, qs, ts, want)
        # (two separate indels leave a lower bound so poor that every diagonal may stay live: exactness is the point there)
        assert (steps <= full if name == "two_indels" else steps < full) and one_band + carried == len(qs)


def test_substitutions_turn_a_carried_gap_into_one_band():
    """an indel of 129 leaves a dead interior of exactly 128 diagonals; a substitution costs S_lb 10, and two of them make
    diagonals 1 and 128 live (g(1) + g(128) = 187 <= g(129) + 20): the interior is narrower than 128, one band"""
    rng = np.random.default_rng(3)
    t = rng.integers(0, 4, size=600).astype(np.uint8)
    long_ = np.concatenate([t[:300], rng.integers(0, 4, size=129).astype(np.uint8), t[300:]])
    qs, ts = [], []
    for k in range(4):
        sub = t.copy()
        sub[[10, 40, 500][:k]] = (sub[[10, 40, 500][:k]] + 1) % 4
        qs += [long_, sub]
        ts += [sub, long_]
    want = oracle(qs, ts)
    for w in sorted(WAVES):
        res, info = run(qs, ts, {"SVDSS_ALIGN_BAND": "2", **WAVES[w]})
        check_result(res, qs, ts, want)
        assert info[3] == 4 and info[2] == 4
    for k in range(4):
        res, info = run(qs[2 * k:2 * k + 2], ts[2 * k:2 * k + 2], {"SVDSS_ALIGN_BAND": "2"})
        check_result(res, qs[2 * k:2 * k + 2], ts[2 * k:2 * k + 2], want[2 * k:2 * k + 2])
        assert (info[2], info[3]) == ((0, 2) if k < 2 else (2, 0)), (k, info)


def test_unrelated_pairs_run_their_full_matrix():
    qs, ts, want = groups()["unrelated"]
    for band in BANDS:
        res, (steps, full, one_band, carried) = run(qs, ts, {"SVDSS_ALIGN_BAND": band})
        check_result(res, qs, ts, want)
        assert steps == full and carried == 0


def test_parameters_outside_the_proof_run_the_full_matrix():
    qs, ts, _ = groups()["two_indels"]
    mat = np.where(np.eye(5, dtype=bool), 0, -4).astype(np.int8).reshape(-1)   # no positive entry
    want = oracle(qs, ts, mat)
    old = os.environ.pop("SVDSS_ALIGN_BAND", None)
    b = Batch()
    try:
        res = b.run(qs, ts, mat)
        info = np.full(4, -1, dtype=np.int64)
        check(lib.svdss_aln_batch_band_info(b.h, info.ctypes.data), "svdss_aln_batch_band_info")
    finally:
        b.close()
        if old is not None:
            os.environ["SVDSS_ALIGN_BAND"] = old
    check_result(res, qs, ts, want, mat)
    assert info[0] == info[1] and info[2] == 0 and info[3] == 0


@pytest.mark.parametrize("waves", ["default", "one"])
def test_batch_object_reuse_leaves_nothing_behind(waves):
    """a second, smaller call on one batch object: the same lengths in another order with other contents, so that every
    boundary row and exit array of the first call lies where the second one's are"""
    qs, ts, want = groups()["indels"]
    pick = [k for k, (q, t) in enumerate(zip(qs, ts)) if abs(len(q) - len(t)) in (26, 129, 500)]
    rng = np.random.default_rng(31)
    qs2, ts2 = [], []
    for k in pick[::-1]:
        ins, ln = len(qs[k]) > len(ts[k]), abs(len(qs[k]) - len(ts[k]))
        q, t = indel_pair(rng, min(len(qs[k]), len(ts[k])), ln, "middle", ins)
        qs2.append(substituted(rng, q, 2))
        ts2.append(t)
    want2 = oracle(qs2, ts2)
    b = Batch()
    try:
        env = {"SVDSS_ALIGN_BAND": "2", **WAVES[waves]}
        res, _ = run(qs, ts, env, batch=b)
        check_result(res, qs, ts, want)
        res, info = run(qs2, ts2, env, batch=b)
        check_result(res, qs2, ts2, want2)
        assert info[3] > 0 and info[2] > 0 and info[0] < info[1]
        res, info = run(qs2[:3], ts2[:3], {"SVDSS_ALIGN_BAND": "0", **WAVES[waves]}, batch=b)
        check_result(res, qs2[:3], ts2[:3], want2[:3])
        assert info[0] == info[1]
    finally:
        b.close()


@pytest.mark.parametrize("band", BANDS)
def test_several_chunks(band):
    qs, ts, want = everything()
    res, info = run(qs, ts, {"SVDSS_ALIGN_BAND": band, "SVDSS_ALIGN_DIR_MB": "1"})
    check_result(res, qs, ts, want)
    assert res.info[0] > 10
    whole, info_whole = run(qs, ts, {"SVDSS_ALIGN_BAND": band})
    assert info == info_whole and whole.info[0] == 1


def test_largest_pair_is_within_the_limit():
    qs, ts, _ = everything()
    assert max(max(len(q), len(t)) for q, t in zip(qs, ts)) <= 1700
