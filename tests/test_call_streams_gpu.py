"""The call side on few streams: the first stage's two whole-wavefront variants as one launch (poa_quad_pair_kernel), one
pooled stream per call of POA / realignment / ratio (svdss_amd/csrc/call_streams.h), leases borrowed only by a wave of several
launches.  Results against the oracle bit for bit, the pool through svdss_call_side_stat."""
import ctypes as C
import threading

import numpy as np
import pytest

from svdss_amd import calldp
from svdss_amd._lib import check, lib
from tests import oracle_lib as O
from tests import poa_plan_lib as P
from tests.mirror import caller
from tests.test_oracle_poa import mutate

pytestmark = pytest.mark.gpu
LET = np.frombuffer(b"ACGTN", dtype=np.uint8)


def _to_str(a):
    return bytes(LET[a]).decode()


def _stat(device=0):
    out = (C.c_int64 * 4)()
    check(lib.svdss_call_side_stat(device, out), "svdss_call_side_stat")
    return list(out)   # [streams of the device, streams created, launches with both variants, leases borrowed]


def _subst(rng, t, rate):
    r = t.copy()
    e = rng.random(len(r)) < rate
    r[e] = (r[e] + rng.integers(1, 4, size=int(e.sum()))) % 4
    return r


def _cluster(rng, length, n_reads=4, rate=0.005):
    t = rng.integers(0, 4, size=length).astype(np.uint8)
    return [_subst(rng, t, rate) for _ in range(n_reads)]


def test_the_stat_refuses_bad_arguments():
    out = (C.c_int64 * 4)()
    assert lib.svdss_call_side_stat(0, None) != 0 and lib.svdss_call_side_stat(-1, out) != 0 and lib.svdss_call_side_stat(0, out) == 0


# ---------------------------------------------------------------------------------------------------------------- merged launch
# the longest read decides the variant: 1,799 bp -> band 2 * 27 + 1 + 8 = 63 columns, one per lane; 1,800 bp -> 65, two per lane
# (tests/test_poa_merge.py holds the planner to that)
@pytest.mark.parametrize("n2,n1", [(1, 1), (1, 3), (3, 1), (2, 2), (0, 3), (3, 0)])
def test_merged_launch_equals_oracle_and_separate_launches(n2, n1, monkeypatch):
    rng = np.random.default_rng(100 + 10 * n2 + n1)
    clusters = [_cluster(rng, 1800) for _ in range(n2)] + [_cluster(rng, 1799) for _ in range(n1)]
    clusters[-1] = clusters[-1][:1]                       # a one-read sub-cluster (of the last one's variant) ...
    order = rng.permutation(len(clusters))
    clusters = [clusters[k] for k in order]
    clusters.insert(1, [])                                # ... and an empty one among them
    want = [_to_str(O.poa_consensus(cl)) if cl else "" for cl in clusters]
    s0 = _stat()
    got, stats = caller.run_poa(clusters)
    s1 = _stat()
    assert got == want and stats["quad_back"] == 0
    assert s1[2] - s0[2] == (1 if n2 and n1 else 0)
    monkeypatch.setenv("SVDSS_POA_MERGE", "0")
    sep, sep_stats = caller.run_poa(clusters)
    s2 = _stat()
    assert sep == got and sep_stats["quad_back"] == 0 and sep_stats["cells"] == stats["cells"]
    assert s2[2] == s1[2]


# ---------------------------------------------------------------------------------------------------------------- the pool
def _sequence(clusters, refs):
    """POA, realignment of the consensus sequences against `refs`, ratio of adjacent consensus pairs: one call each"""
    cons, stats = caller.run_poa(clusters)
    scores, cigs, _ = calldp.ksw_extd2_global(cons, refs)
    ratio, lcs = calldp.fuzz_ratio(cons[:-1], cons[1:])
    return cons, stats["quad_back"], scores.tolist(), [c.tolist() for c in cigs], ratio.tolist(), lcs.tolist()


def _batch(seed, n, n_reads):
    rng = np.random.default_rng(seed)
    templates = [rng.integers(0, 4, size=int(rng.integers(600, 1901))).astype(np.uint8) for _ in range(n)]
    clusters = [[_subst(rng, t, 0.005) for _ in range(n_reads)] for t in templates]
    return clusters, [_to_str(t) for t in templates]


def test_one_stream_per_call():
    clusters, refs = _batch(7, 6, 5)
    before = _stat()
    first = _sequence(clusters, refs)
    again = _sequence(clusters, refs)
    after = _stat()
    assert first == again and first[1] == 0
    assert first[0] == [_to_str(O.poa_consensus(cl)) for cl in clusters]
    assert after[1] - before[1] <= (0 if before[0] >= 1 else 1)     # every call of the thread on the pool's one stream
    assert after[3] == before[3]                                   # a wave of one launch borrows nothing


def test_three_threads_three_streams():
    clusters, refs = _batch(8, 8, 5)
    single = _sequence(clusters, refs)
    assert single[1] == 0
    before = _stat()
    out, errs = [None] * 3, []

    def work(k):
        try:
            a = _sequence(clusters, refs)
            b = _sequence(clusters, refs)
            out[k] = (a, b)
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    after = _stat()
    for a, b in out:
        assert a == single and b == single
    assert after[1] - before[1] <= 3 and after[0] <= before[0] + 3
    assert _sequence(clusters, refs) == single                      # a fourth caller afterwards finds a stream waiting
    assert _stat()[1] == after[1]


# ---------------------------------------------------------------------------------------------------------------- borrowed leases
def _mixed_clusters(seed, n_clusters):
    """Short sub-clusters with indels between the haplotypes, and every fourth one beyond 1,800 bp: without the first stage
    round 0 has a launch of one-column rows and one of two-column rows."""
    rng = np.random.default_rng(seed)
    clusters = []
    for k in range(n_clusters):
        length = int(rng.integers(1900, 2400)) if k % 4 == 3 else int(rng.integers(200, 900))
        t = rng.integers(0, 4, size=length).astype(np.uint8)
        if k % 3 == 0:
            cut = int(rng.integers(20, 120))
            alt = np.concatenate([t[:length // 3], t[length // 3 + cut:]])
        elif k % 3 == 1:
            alt = np.concatenate([t[:length // 2], rng.integers(0, 4, size=int(rng.integers(20, 150))).astype(np.uint8), t[length // 2:]])
        else:
            alt = t
        n = int(rng.integers(3, 10))
        clusters.append([mutate(rng, alt if (i % 2) else t, float(rng.choice([0.002, 0.01, 0.03]))) for i in range(n)])
    return clusters


def test_a_wave_of_several_launches_borrows_and_returns(monkeypatch):
    clusters = _mixed_clusters(41, 16)
    p = P.Batch([[len(r) for r in cl] for cl in clusters], P.knobs(use_quad=False)).plan(0)
    assert len(p["groups"]) >= 2 and p["cuts"] == [0, len(p["groups"])]      # round 0: one wave of two launches or more
    want = [_to_str(O.poa_consensus(cl)) for cl in clusters]
    monkeypatch.setenv("SVDSS_POA_QUAD", "0")
    before = _stat()
    got, stats = caller.run_poa(clusters)
    after = _stat()
    assert got == want and stats["quad_back"] == 0
    assert after[3] > before[3]
    monkeypatch.delenv("SVDSS_POA_QUAD")
    one, _ = caller.run_poa(clusters[:2])                                    # every lease is back: a single call creates nothing
    assert one == want[:2] and _stat()[0] == after[0]
