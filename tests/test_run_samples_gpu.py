"""`SVDSS run --samples LIST` (csrc/run_host.cpp's session): many BAMs in one process, the reference, the index and the pools
resident between them.  The yardstick in every case is `SVDSS run --bam` of this tree on each sample alone with the same
options (tests/test_run_gpu.py holds that one against the three-step chain, under every knob: knobs move work around, never
results -- so the alone runs are made once per sample and option set, with small batches, and kept).  Every VCF and SFS of a
list must have the bytes of the sample's alone run, whatever ran before it in the process."""
import re
import subprocess

import pytest

from tests.common import BIN
from tests.run_fixture import env0
from tests import run_samples_fixture as F

pytestmark = pytest.mark.gpu

TIMEOUT = 240
SMALL = {"SVDSS_BAM_BATCH_MB": "1", "SVDSS_BAM_SLAB_KB": "64"}
STOP = {}      # set by the first abort, segmentation fault or time-out of the module: nothing more is started on the GPU


@pytest.fixture(autouse=True)
def _nothing_after_a_crash():
    if STOP:
        pytest.fail("not started: " + STOP["why"])


def svdss(cmd, env, tag):
    try:
        r = subprocess.run([BIN, *map(str, cmd)], capture_output=True, timeout=TIMEOUT, env=env)
    except subprocess.TimeoutExpired:
        STOP["why"] = f"{tag} ran into its time limit"
        raise
    if r.returncode in (-6, -11, 134, 139, 124, 137):
        STOP["why"] = f"{tag} ended with status {r.returncode}"
        pytest.fail(STOP["why"] + "\n" + r.stderr.decode()[-3000:])
    return r


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("run_samples")
    fx = F.reference(tmp)
    ref = fx["ref"]
    S = {}
    # three different samples: a contig the FASTA lacks, the contigs in another order, the order before once more
    S["abc"] = F.sample(ref, tmp / "abc.bam", ["chrA", "chrB", "chrC"], seed=21, orphans=True, unmapped=40)
    S["ba"] = F.sample(ref, tmp / "ba.bam", ["chrB", "chrA"], seed=31)
    S["ba2"] = F.sample(ref, tmp / "ba2.bam", ["chrB", "chrA"], seed=41, n_svs=4)
    S["empty"] = F.header_only(tmp / "empty.bam", ["chrA", "chrB"])
    # few reads to search / every read searched (and an unmapped tail of nine or more batches of 1 MB)
    S["few"] = F.sample(ref, tmp / "few.bam", ["chrA", "chrB"], seed=51, first=100)
    S["many"] = F.sample(ref, tmp / "many.bam", ["chrA", "chrB"], seed=61, clip_all=True, unmapped=700)
    S["cut"] = {"bam": F.cut_inside_last_record(S["ba"]["bam"], tmp / "cut.bam"), "order": ["chrB", "chrA"]}
    fx["S"], fx["alone"], fx["n_lists"] = S, {}, 0
    return fx


def alone(fx, name, opts=()):
    """(VCF, SFS, stderr) of `run --bam` on the sample alone; made once"""
    key = (name,) + tuple(map(str, opts))
    if key not in fx["alone"]:
        sfs = fx["tmp"] / f"alone{len(fx['alone'])}.sfs"
        r = svdss(["run", "--reference", fx["fa"], "--index", fx["fmd"], "--bam", fx["S"][name]["bam"], "--sfs", sfs, "--verbose", *opts], env0(**SMALL),
                  f"run --bam {name}")
        assert r.returncode == 0, (name, r.stderr.decode()[-2500:])
        fx["alone"][key] = (r.stdout, sfs.read_bytes(), r.stderr.decode())
    return fx["alone"][key]


class Listed:
    """One `run --samples` process: its files and its stderr, cut at the `[run] sample K of N` lines of --verbose"""

    def __init__(self, fx, names, opts=(), env=None, sfs=True, ok=True):
        fx["n_lists"] += 1
        d = fx["tmp"] / f"list{fx['n_lists']}"
        d.mkdir()
        self.names, self.vcf, self.sfs = names, [d / f"{k + 1}_{n}.vcf" for k, n in enumerate(names)], [d / f"{k + 1}_{n}.sfs" for k, n in enumerate(names)]
        lines = ["# " + " ".join(names), ""]
        for k, n in enumerate(names):
            lines.append("\t".join(map(str, [fx["S"][n]["bam"], self.vcf[k]] + ([self.sfs[k]] if sfs else []))))
        (d / "list.txt").write_text("\r\n".join(lines) + "\r\n" if fx["n_lists"] % 2 else "\n".join(lines))
        self.r = svdss(["run", "--reference", fx["fa"], "--index", fx["fmd"], "--samples", d / "list.txt", "--verbose", *opts], env0(**dict(SMALL, **(env or {}))),
                       "run --samples " + " ".join(names))
        self.err = self.r.stderr.decode()
        self.dir = d
        if ok:
            assert self.r.returncode == 0, self.err[-3000:]
            assert self.r.stdout == b""
            assert not [p for p in d.iterdir() if p.name.endswith(".tmp")]
        cuts = [m.start() for m in re.finditer(r"^\[run\] sample \d+ of \d+: ", self.err, re.M)] + [len(self.err)]
        self.part = [self.err[a:b] for a, b in zip(cuts, cuts[1:])]

    def same_as_alone(self, fx, opts=(), sfs=True):
        for k, n in enumerate(self.names):
            V, T, _ = alone(fx, n, opts)
            assert self.vcf[k].read_bytes() == V, (k + 1, n)
            if sfs:
                assert self.sfs[k].read_bytes() == T, (k + 1, n)
        done = re.findall(r"^\[run\] sample (\d+): (\S+) -> (\S+): (\d+) VCF record\(s\), [\d.]+ s$", self.err, re.M)
        assert [(int(a), b, c) for a, b, c, _ in done] == [(k + 1, str(fx["S"][n]["bam"]), str(self.vcf[k])) for k, n in enumerate(self.names)]
        for k, (_, _, _, n_rec) in enumerate(done):
            assert int(n_rec) == sum(1 for l in self.vcf[k].read_bytes().split(b"\n") if l and not l.startswith(b"#"))


def n_records(vcf):
    return sum(1 for l in vcf.split(b"\n") if l and not l.startswith(b"#"))


def test_three_different_samples(fx):
    L = Listed(fx, ["abc", "ba", "ba2"])
    L.same_as_alone(fx)
    vcfs = [alone(fx, n)[0] for n in L.names]
    print("VCF records alone:", [n_records(v) for v in vcfs])
    assert all(n_records(v) >= 2 for v in vcfs) and len(set(vcfs)) == 3          # (not vacuous: three different, non-empty answers)
    assert all(alone(fx, n)[1] for n in L.names)
    # the FASTA and the index file are read once; the copy in HBM goes up again exactly where the header changed
    assert L.err.count("[run] reference: FASTA read") == 1 and "FASTA read" in L.part[0]
    assert L.err.count("[run] index: file read") == 1 and "index: file read" in L.part[0]
    up, re_ = "[run] reference: uploaded to the GPU", "[run] reference: copy on the GPU reused"
    assert [(up in p, re_ in p) for p in L.part] == [(True, False), (True, False), (False, True)], L.err[-3000:]
    assert "3 sample(s): the FASTA read 1 time(s), the index file 1 time(s), the chromosomes uploaded 2 time(s)" in L.err
    # every sample has its own stopwatches, and the process says "All done" once
    assert L.err.count("[run] [time] total") == 3 and L.err.count("All done!") == 1


def test_the_same_sample_three_times_and_around_an_empty_one(fx):
    L = Listed(fx, ["ba", "ba", "ba"])
    L.same_as_alone(fx)
    L = Listed(fx, ["ba", "empty", "ba"])
    L.same_as_alone(fx)
    V = alone(fx, "empty")[0]
    assert n_records(V) == 0 and V.startswith(b"##fileformat=VCF") and alone(fx, "empty")[1] == b""
    # the header changes to the empty sample's and back: three uploads
    assert "the chromosomes uploaded 3 time(s)" in L.err


@pytest.mark.parametrize("lf", ["by_estimate", "lf0", "lf1"])
def test_index_form(fx, lf):
    """`few` leaves a handful of reads to search, every read of `many` is searched: SVDSS_SEARCH_LF_MAX between the two"""
    few, many = (float(re.search(r"sfs: (\d+) reads parked", alone(fx, n)[2]).group(1)) for n in ("few", "many"))
    est = {n: re.search(r"\[smooth\] device path: (\d+) records, (\d+) kept \(XF 0/1/2/3: (\d+) ", alone(fx, n)[2]) for n in ("few", "many")}
    n_few, n_many = int(est["few"].group(3)), int(est["many"].group(3))
    print("reads with XF = 0 (searched):", n_few, n_many, "; parked alone:", few, many)
    assert n_few <= 40 and n_many >= 200
    env = {"by_estimate": {"SVDSS_SEARCH_LF_MAX": "100"}, "lf0": {"SVDSS_SEARCH_LF": "0"}, "lf1": {"SVDSS_SEARCH_LF": "1"}}[lf]
    rank, full, swap = "rank blocks alone made resident", "full restore made resident", "full restore replaces the rank blocks alone"
    re_full, re_rank = "resident index reused (full restore)", "resident index reused (rank blocks alone)"

    def said(L):
        return [[w for w in (rank, swap, full, re_full, re_rank) if w in p] for p in L.part]

    A = Listed(fx, ["few", "many", "few"], env=env)
    A.same_as_alone(fx)
    B = Listed(fx, ["many", "few"], env=env)
    B.same_as_alone(fx)
    print(lf, said(A), said(B))
    if lf == "by_estimate":
        assert said(A) == [[rank], [swap, full], [re_full]] and said(B) == [[full], [re_full]]
    elif lf == "lf0":
        assert said(A) == [[full], [re_full], [re_full]] and said(B) == [[full], [re_full]]
    else:
        assert said(A) == [[rank], [re_rank], [re_rank]] and said(B) == [[rank], [re_rank]]
    assert A.err.count("[run] index: file read") == 1 and B.err.count("[run] index: file read") == 1


STORE_LINE = re.compile(r"\[run\] record store: (\d+) records, (\d+) bytes in (\d+) of (\d+) batches, (complete|incomplete: the call stage reads the file)")


def test_store_too_small_for_the_middle_sample(fx):
    L = Listed(fx, ["few", "ba", "few"], env={"SVDSS_CALL_STORE_MB": "1"})
    L.same_as_alone(fx)
    got = [STORE_LINE.search(p).group(5).split(":")[0] for p in L.part]
    print([STORE_LINE.search(p).group(0) for p in L.part])
    assert got == ["complete", "incomplete", "complete"]
    assert ["pass 1 from the records kept in HBM" in p for p in L.part] == [True, False, True]


def test_park_too_small_and_tiny_groups(fx):
    """the index is resident from the start of samples 2 and 3; the park fills, so feeders search batches themselves; `many`
    ends in nine or more batches of unmapped reads behind a partly filled group"""
    env = {"SVDSS_PARK_MB": "1", "SVDSS_PARK_ARENA_MB": "1", "SVDSS_PARK_GROUP_READS": "16"}
    L = Listed(fx, ["many", "many", "ba"], env=env)
    L.same_as_alone(fx)
    sfs = [re.search(r"sfs: (\d+) reads parked in (\d+) batch\(es\), (\d+) group\(s\) searched \([\d.]+ s\), (\d+) batch\(es\) searched by their feeding thread", p) for p in L.part]
    print([m.group(0) for m in sfs])
    batches = [int(STORE_LINE.search(p).group(4)) for p in L.part]
    assert batches[0] >= 12 and batches[1] == batches[0]          # (the mapped reads' batches + nine or more of the tail)
    assert int(sfs[1].group(4)) >= 1 and int(sfs[1].group(1)) >= 1          # (some batches by their feeders, some reads parked)
    # ... and with room in the park the reused index is held back: everything of sample 2 goes in groups, nothing per batch
    L = Listed(fx, ["many", "many"], env={"SVDSS_PARK_GROUP_READS": "16"})
    L.same_as_alone(fx)
    m = re.search(r"sfs: (\d+) reads parked in (\d+) batch\(es\), (\d+) group\(s\) searched \([\d.]+ s\), (\d+) batch\(es\) searched by their feeding thread", L.part[1])
    print(m.group(0))
    assert int(m.group(4)) == 0 and int(m.group(1)) >= 200


def test_region_on_samples_with_different_headers(fx):
    opts = ("--region", "chrB:20,001-90000", "--region", "chrA:1-60000")
    L = Listed(fx, ["abc", "ba", "few"], opts=opts)
    L.same_as_alone(fx, opts)
    whole = [alone(fx, n)[1] for n in L.names]
    part = [alone(fx, n, opts)[1] for n in L.names]
    assert all(p and p != w for p, w in zip(part[:2], whole[:2]))          # (the regions took something away, and left something)
    assert L.err.count("[regions] 2 interval(s)") == 3
    # a name one sample's header lacks is refused for that sample, as `run --bam` refuses it
    L = Listed(fx, ["abc", "ba", "abc"], opts=("--region", "chrC"), ok=False)
    assert L.r.returncode == 1 and L.r.stdout == b""
    assert "sample 2 (" + str(fx["S"]["ba"]["bam"]) + "): --region chrC: the BAM header has no reference of that name" in L.err
    assert L.vcf[0].read_bytes() == alone(fx, "abc", ("--region", "chrC"))[0]
    assert sorted(p.name for p in L.dir.iterdir()) == ["1_abc.sfs", "1_abc.vcf", "list.txt"]


def test_truncated_bam_as_the_second_of_three(fx):
    L = Listed(fx, ["abc", "cut", "ba"], ok=False)
    assert L.r.returncode == 1 and L.r.stdout == b""
    crit = [l for l in L.err.split("\n") if "[critical]" in l]
    print(crit)
    assert len(crit) == 1 and "sample 2 (" + str(fx["S"]["cut"]["bam"]) + "): " in crit[0] and "error reading" in crit[0]
    assert L.vcf[0].read_bytes() == alone(fx, "abc")[0] and L.sfs[0].read_bytes() == alone(fx, "abc")[1]
    assert sorted(p.name for p in L.dir.iterdir()) == ["1_abc.sfs", "1_abc.vcf", "list.txt"]
    assert "[run] sample 1: " in L.err and "[run] sample 3" not in L.err
    # the same damage, the same message, from `run --bam`
    r = svdss(["run", "--reference", fx["fa"], "--index", fx["fmd"], "--bam", fx["S"]["cut"]["bam"]], env0(**SMALL), "run --bam cut")
    assert r.returncode == 1
    alone_crit = [l for l in r.stderr.decode().split("\n") if "[critical]" in l]
    assert len(alone_crit) == 1 and crit[0].split("): ", 1)[1] == alone_crit[0].split("] ", 2)[2]


def test_no_growth_over_eight_samples(fx):
    """The session pools no per-sample object: record store and park are freed completely when their sample ends.  What
    stays -- the index, the chromosomes in HBM with their placement arena, the calling thread's LCS-ratio arena -- has its
    final size when sample 2 starts, because the sample is the same.  The allowance is the largest single object a sample
    takes and gives back, for the allocator's own rounding: one arena of the record store (SVDSS_STORE_ARENA_MB = 2) or of
    the park (SVDSS_PARK_ARENA_MB = 2), 2 MiB."""
    env = {"SVDSS_STORE_ARENA_MB": "2", "SVDSS_PARK_ARENA_MB": "2"}
    allowance = 2 << 20
    L = Listed(fx, ["ba"] * 8, env=env, sfs=False)
    L.same_as_alone(fx, sfs=False)
    at = [re.search(r"^\[run\] sample \d+ of 8: \S+; (\d+) bytes of HBM free, (\d+) thread\(s\)$", p, re.M) for p in L.part]
    free = [int(m.group(1)) for m in at]
    threads = [int(m.group(2)) for m in at]
    print("free HBM at the start of samples 1..8:", free)
    print("threads at the start of samples 1..8:", threads)
    assert len(free) == 8
    for k in range(2, 8):
        assert free[k] >= free[1] - allowance, (k + 1, free)
        assert threads[k] <= threads[1], (k + 1, threads)
