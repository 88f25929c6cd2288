"""`SVDSS search --gpus N` with the front end of every region started beside the index restore (search_host.cpp:
an EarlySearch, a park and a drain thread per region, each on its region's GPU and released with that GPU's replica).
The file of tests/test_bam_device_gpu.py's binary test -- a 150 kb reference, 3,200 records (400 reads under eight names),
BGZF members of mixed levels -- through the binary, more regions than GPUs (SVDSS_GPUS_OVERSUBSCRIBE), batches of 1 MB, the
index held back 1.5 s so that every region parks its batches although this index is resident in milliseconds.  Every
run's stdout against `--gpus 1` with SVDSS_SEARCH_EARLY=0, the index-first order."""
import os
import re
import subprocess

import numpy as np
import pytest

from svdss_amd import synth
from tests.common import BIN
from tests.test_bam_device_gpu import _bgzf_levels, _raw_bam, _records, case  # noqa: F401  (case: a fixture)

pytestmark = pytest.mark.gpu

OPTIONS = {"t4_b100": ("--threads", "4", "--bsize", "100"), "t3_b1000_noputative_noassemble": ("--threads", "3", "--bsize", "1000", "--noputative", "--noassemble")}
# what every run sets
BASE = {"SVDSS_GPUS_OVERSUBSCRIBE": "1", "SVDSS_REGION_MIN_KB": "128", "SVDSS_BAM_SLAB_KB": "64", "SVDSS_BAM_BATCH_MB": "1", "SVDSS_SEARCH_EARLY": "1",
        "SVDSS_EARLY_HOLD_MS": "1500"}
EARLY_LINE = re.compile(r"region (\d+): front end beside the index restore: (\d+) batches \((\d+) records\) .* their (\d+) reads searched in (\d+) launch")
REGIONS_LINE = re.compile(r"(\d+) regions of the file, one per GPU: (\d+) seam\(s\) run, (\d+) region\(s\) run again")
N_SHORT = 8        # one read below 100 bases, under eight names


@pytest.fixture(scope="module")
def files(case, tmp_path_factory):  # noqa: F811
    tmp = tmp_path_factory.mktemp("gpus_early")
    ref, ix, fm, reads, names = case
    rng = np.random.default_rng(23)
    recs = []
    for rep in range(8):
        r, _ = _records([f"{n}/{rep}" for n in names], reads, rng, decoys=(rep % 2 == 0))
        recs += r
    bam = tmp / "reads.bam"
    bam.write_bytes(_bgzf_levels(_raw_bam([("chr1", 150000)], recs), rng, block=60000))
    # (through `SVDSS index`: its sidecar carries the rank blocks the rank-blocks form needs)
    fa = tmp / "ref.fa"
    fa.write_text("".join(f">chr{i + 1}\n{synth.to_ascii(c)}\n" for i, c in enumerate(ref)))
    fmd = tmp / "ref.fmd"
    r = subprocess.run([BIN, "index", "-d", str(fa), "-o", str(fmd)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return {"bam": bam, "fmd": fmd, "n_records": len(recs), "expected": {}}


def search(files, options, gpus, env):
    r = subprocess.run([BIN, "search", "--index", str(files["fmd"]), "--bam", str(files["bam"]), "--verbose", "--gpus", str(gpus), *OPTIONS[options]],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def expected(files, options):
    """the comparison text: one GPU, the index first -- once per option set"""
    if options not in files["expected"]:
        r = search(files, options, 1, dict(BASE, SVDSS_SEARCH_EARLY="0"))
        assert "front end beside the index restore" not in r.stderr and r.stdout.count("\n") > 5000
        assert r.stderr.count("Alignment filtered due to l_qseq") == N_SHORT
        files["expected"][options] = r.stdout
    return files["expected"][options]


def early_lines(stderr):
    """region -> (batches parked, records seen, reads parked, launches) of the per-region lines"""
    return {int(m.group(1)): tuple(int(m.group(k)) for k in (2, 3, 4, 5)) for m in EARLY_LINE.finditer(stderr)}


def check_every_region_has_its_line(r, n):
    """a per-region line for every region, with at least one launch; returns region -> figures"""
    lines = early_lines(r.stderr)
    print(lines)
    assert sorted(lines) == list(range(n)), r.stderr[-3000:]
    assert all(launches >= 1 for _, _, _, launches in lines.values()), lines
    m = REGIONS_LINE.search(r.stderr)
    assert m and int(m.group(1)) == n, r.stderr[-3000:]
    return lines


def held_back(files, options, n):
    """n regions with nothing but what every run sets -- once per option set and n"""
    key = (n, options)
    if key not in files["expected"]:
        files["expected"][key] = search(files, options, n, BASE)
    return files["expected"][key]


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("n", [2, 3, 4, 7])
def test_every_region_parks_beside_the_restore_and_the_bytes_are_those_of_one_gpu(files, options, n):
    r = held_back(files, options, n)
    assert r.stdout == expected(files, options)
    check_every_region_has_its_line(r, n)
    assert r.stderr.count("Alignment filtered due to l_qseq") == N_SHORT
    assert REGIONS_LINE.search(r.stderr).group(3) == "0"


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("n", [2, 3, 4, 7])
def test_every_region_parks_at_least_two_batches(files, options, n):
    """The same runs: on every region's line at least 2 batches parked and at least 1 launch.  The file inflates to
    5,673,112 bytes and a batch is 1 MB, so a seventh of it (0.8 MB) is two batches only because a region's front end cuts
    its first batch at a quarter of the batch size and its second at half (BamSelectRegion::small_start)."""
    lines = early_lines(held_back(files, options, n).stderr)
    print(lines)
    assert sorted(lines) == list(range(n))
    for g, (batches, records, reads, launches) in lines.items():
        assert batches >= 2 and launches >= 1, (g, lines)


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("lf", ["1", "0"])
@pytest.mark.parametrize("n", [2, 3, 4, 7])
def test_rank_blocks_alone_on_every_replica_and_the_full_restore(files, options, n, lf):
    r = search(files, options, n, dict(BASE, SVDSS_SEARCH_LF=lf))
    assert r.stdout == expected(files, options)
    check_every_region_has_its_line(r, n)
    if lf == "1":
        # the form, said once, and the blocks read once for all the GPUs; every replica says when it was resident
        assert r.stderr.count("the index as a rank structure alone") == 1 and f"blocks read once for {n} GPUs" in r.stderr, r.stderr[-3000:]
        assert r.stderr.count("(rank blocks alone, uploaded from the one host copy)") == n
    else:
        assert "rank structure alone" not in r.stderr and "rank blocks alone" not in r.stderr
        assert r.stderr.count(f"the index as a full restore on each of {n} GPUs") == 1
        assert len(re.findall(r"replica \d+ of the index resident at", r.stderr)) == n


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("n,knob", [(3, "1"), (2, "2")])
def test_regions_that_run_again_with_parks_in_play(files, options, n, knob):
    """SVDSS_REGION_TEST: 1 = every guess is no record (the regions fail and run again), 2 = the seams do not fit (the regions
    run again): what the failed run parked is discarded, nothing is dealt twice"""
    r = search(files, options, n, dict(BASE, SVDSS_REGION_TEST=knob))
    assert r.stdout == expected(files, options)
    m = REGIONS_LINE.search(r.stderr)
    assert m and int(m.group(1)) == n, r.stderr[-3000:]
    if knob == "1":
        assert m.group(3) == str(n - 1)
    else:
        assert int(m.group(3)) >= 1
    assert r.stderr.count("Alignment filtered due to l_qseq") == N_SHORT
    assert 0 in early_lines(r.stderr)


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("pressure", ["park_too_small", "tiny_groups"])
def test_parks_under_pressure(files, options, pressure):
    env = {"park_too_small": {"SVDSS_PARK_MB": "2", "SVDSS_PARK_ARENA_MB": "1", "SVDSS_PARK_GROUP_READS": "200"},
           "tiny_groups": {"SVDSS_PARK_GROUP_READS": "7", "SVDSS_SEARCH_FEEDERS": "2"}}[pressure]
    r = search(files, options, 3, dict(BASE, **env))
    assert r.stdout == expected(files, options)
    lines = early_lines(r.stderr)
    print(lines)
    assert sorted(lines) == [0, 1, 2], r.stderr[-3000:]
    assert r.stderr.count("Alignment filtered due to l_qseq") == N_SHORT
    if pressure == "park_too_small":
        # three regions on one device split 2 MB: fewer reads are parked than the region holds -- what it holds is what the
        # same region parks when the park is large enough (the index is held back longer than the front ends take)
        holds = early_lines(held_back(files, options, 3).stderr)
        for g, (batches, records, reads, launches) in lines.items():
            assert reads < holds[g][2], (g, lines, holds)


@pytest.mark.parametrize("options", sorted(OPTIONS))
def test_orderly_teardown_frees_every_park_and_replica(files, options):
    r = search(files, options, 2, dict(BASE, SVDSS_CLEAN_EXIT="1"))      # (search() asserts exit 0)
    assert r.stdout == expected(files, options)
    lines = check_every_region_has_its_line(r, 2)
    assert all(batches >= 2 for batches, _, _, _ in lines.values()), lines


@pytest.mark.parametrize("options", sorted(OPTIONS))
def test_the_index_first_order_is_still_there(files, options):
    r = search(files, options, 2, dict(BASE, SVDSS_SEARCH_EARLY="0"))
    assert "front end beside the index restore" not in r.stderr and "replicated on 2 GPUs" in r.stderr
    assert REGIONS_LINE.search(r.stderr).group(1) == "2"
    assert r.stdout == expected(files, options)
