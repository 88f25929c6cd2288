"""What `SVDSS search` decides once for the process from the counters of its early front ends -- one per region of the
file with --gpus N (csrc/early_estimate.h): the summed estimate of the reads to search, when the wait for it is over, the
choice of the rank blocks alone against SVDSS_SEARCH_LF_MAX, and how regions that share a GPU share its park bytes.  On
hand-made counters, through a small program (tests/native/early_estimate.cpp): no GPU, no library."""
import os
import subprocess

import pytest

from tests.common import ROOT

SRC = os.path.join(ROOT, "tests", "native", "early_estimate.cpp")
EXE = os.path.join(ROOT, "tests", "native", "_early_estimate")
HDR = os.path.join(ROOT, "svdss_amd", "csrc", "early_estimate.h")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", EXE, SRC], check=True)
    return EXE


def estimate(exe, regions, waited=0.0, lf_max=-1.0, index_n=6_180_000_000):
    r = subprocess.run([exe, "estimate", repr(waited), repr(lf_max), str(index_n)] + [",".join(str(int(x)) for x in reg) for reg in regions],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = dict(l.split(" ", 1) for l in r.stdout.splitlines())
    return {"each": [float(x) for x in out["each"].split()], "sum": float(out["sum"]), "wait_over": out["wait_over"] == "1",
            "lf": out["rank_blocks_alone"] == "1"}


# a region as the program takes it: records, searched, compressed bytes read, bytes of the region, front finished
def test_regions_that_have_seen_nothing_contribute_nothing(exe):
    seen = (60000, 6000, 100 << 20, 1 << 30, 0)          # a tenth of the records searched, a tenth of the region read
    nothing = (0, 0, 0, 1 << 30, 0)
    one = estimate(exe, [seen])
    assert one["each"] == [pytest.approx(6000 * (1 << 30) / (100 << 20))] and one["sum"] == one["each"][0]
    got = estimate(exe, [nothing, seen, nothing, nothing])
    assert got["each"] == [-1, one["each"][0], -1, -1]
    assert got["sum"] == one["sum"] >= 0                  # (not 3 below it)
    # nobody has seen anything: no estimate (-1), and no estimate never chooses the rank blocks alone
    none = estimate(exe, [nothing, nothing], waited=2.0, lf_max=1e12)
    assert none["sum"] == -1 and not none["lf"]
    # records walked of which none is to be searched: an estimate of 0, which is "few"
    zero = estimate(exe, [(60000, 0, 100 << 20, 1 << 30, 0), nothing])
    assert zero["sum"] == 0 and zero["lf"]


def test_the_wait_ends_when_every_region_has_seen_enough_or_finished_or_time_is_up(exe):
    enough = (50000, 100, 1 << 20, 1 << 30, 0)
    short = (49999, 100, 1 << 20, 1 << 30, 0)
    short_done = (120, 3, 1 << 16, 1 << 16, 1)            # a small region, read to its end: it will see no more
    nothing = (0, 0, 0, 1 << 30, 0)
    assert estimate(exe, [enough, enough, enough])["wait_over"]
    assert not estimate(exe, [enough, short, enough])["wait_over"]
    assert not estimate(exe, [enough, nothing])["wait_over"]
    assert estimate(exe, [enough, short_done, enough])["wait_over"]          # does not hold the decision up
    assert estimate(exe, [short_done])["wait_over"]
    assert not estimate(exe, [short], waited=1.5)["wait_over"]               # (as the one-GPU wait: up to and including 1.5 s)
    assert estimate(exe, [short, nothing], waited=1.51)["wait_over"]
    # one region: exactly the one-GPU condition
    assert estimate(exe, [enough])["wait_over"] and not estimate(exe, [short])["wait_over"]


@pytest.mark.parametrize("n", [2, 3, 4, 7, 8])
def test_equal_regions_sum_to_the_one_region_estimate_of_the_whole_file(exe, n):
    file_bytes, comp, recs, srch = 7 * 8 * 3 * (1 << 22), 50 << 20, 52000, 4100        # (divisible by every n)
    whole = estimate(exe, [(recs, srch, comp, file_bytes, 0)])["sum"]
    parts = estimate(exe, [(recs, srch, comp, file_bytes // n, 0)] * n)
    assert parts["sum"] == pytest.approx(whole, rel=1e-12)
    # regions that differ are counted each as it is: a dense one among sparse ones is not lost, nor taken for the whole
    dense = (recs, 10 * srch, comp, file_bytes // n, 0)
    mixed = estimate(exe, [dense] + [(recs, srch, comp, file_bytes // n, 0)] * (n - 1))
    assert mixed["sum"] == pytest.approx(whole * (n + 9) / n, rel=1e-12)


def test_lf_max_compares_against_the_sum(exe):
    reg = (50000, 5000, 100 << 20, 1000 << 20, 0)          # 50,000 reads to search per region
    assert estimate(exe, [reg])["sum"] == pytest.approx(50000)
    # each region alone is below the threshold, their sum is not
    assert estimate(exe, [reg], lf_max=120000)["lf"]
    assert estimate(exe, [reg, reg], lf_max=120000)["lf"]
    assert not estimate(exe, [reg, reg, reg], lf_max=120000)["lf"]
    assert estimate(exe, [reg, reg, reg], lf_max=150001)["lf"] and not estimate(exe, [reg, reg, reg], lf_max=149999)["lf"]
    # the default threshold: 2 M reads per 6.18e9 BWT symbols, in proportion for a smaller index -- against the sum as well
    assert estimate(exe, [reg] * 39, index_n=6_180_000_000)["lf"] and not estimate(exe, [reg] * 41, index_n=6_180_000_000)["lf"]
    assert estimate(exe, [reg] * 3, index_n=618_000_000)["lf"] and not estimate(exe, [reg] * 5, index_n=618_000_000)["lf"]


@pytest.mark.parametrize("n_regions,n_devices", [(1, 1), (2, 1), (3, 1), (7, 1), (2, 2), (3, 2), (7, 2), (8, 8), (9, 8), (7, 3), (4, 8)])
def test_regions_that_share_a_device_split_its_park(exe, n_regions, n_devices):
    park = 32 << 30
    r = subprocess.run([exe, "park", str(park), str(n_regions), str(n_devices)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]
    assert [g for g, _, _ in rows] == list(range(n_regions))
    per_device = {}
    for g, d, b in rows:
        assert d == g % n_devices and b > 0
        per_device.setdefault(d, []).append(b)
    for d, parts in per_device.items():
        assert sum(parts) <= park                                             # never more than park_bytes per device
        assert len(set(parts)) == 1 and parts[0] == park // len(parts)        # equal parts, nothing held back
        if len(parts) == 1:
            assert parts[0] == park                                           # a device to itself: the whole of it
