"""`SVDSS smooth / search --bam / call / run` with --region and --regions-file, each against ITSELF on the BAM that holds the
regions' records alone (tests/region_lib.py writes it): stdout of `search` and the VCF of `call` / `run` byte for byte, --poa,
--clusters, --sfs as well, the inflated stream of `smooth` and of --smoothed.  Every command with a BAI beside the input,
with a CSI (the ranges the index names are read: their number and the compressed bytes read are held against the plan),
with an index older than the BAM (a warning, the whole file), with no index, through the host reader (SVDSS_BAM_DEVICE=0),
with --gpus 2 on one GPU (SVDSS_GPUS_OVERSUBSCRIBE) with and without an index, `call` also with SVDSS_PLACE_HOST=1 -- but
`run`, which refuses the host reader and --gpus 2 with or without regions.  The data set is that of
tests/test_run_gpu.py in BGZF members of 4 KB, read in batches of 1 MB."""
import os
import re
import subprocess

import pytest

from tests import bam_writer
from tests import region_lib as R
from tests.common import BIN
from tests.run_fixture import TIMEOUT, build, env0

pytestmark = pytest.mark.gpu

REGION_ARGS = ["--region", "chrA:50,001-120,000", "--region", "chrA:100001-130000"]
BED = "# loci\nchrB\t20000\t40000\tx\nchrB\t30000\t45000\n"
INTERVALS = [(0, 50000, 130000), (1, 20000, 45000)]
SMALL = {"SVDSS_BAM_BATCH_MB": "1", "SVDSS_BAM_SLAB_KB": "64"}
CONDITIONS = {
    "bai": ([], {}),
    "csi": ([], {}),
    "stale_bai": ([], {}),
    "noindex": ([], {}),
    "gpus2_bai": (["--gpus", "2"], {"SVDSS_GPUS_OVERSUBSCRIBE": "1", "SVDSS_REGION_MIN_KB": "256"}),
    "place_host": ([], {"SVDSS_PLACE_HOST": "1"}),
    "host_reader": ([], {"SVDSS_BAM_DEVICE": "0"}),
    "gpus2": (["--gpus", "2"], {"SVDSS_GPUS_OVERSUBSCRIBE": "1", "SVDSS_REGION_MIN_KB": "256"}),
}
GATED = re.compile(r"\[regions\] (\d+) interval\(s\).* (\d+) compressed bytes read, (\d+) records gated out")
PLAN = re.compile(r"\[regions\] \d+ interval\(s\); (\d+) range\(s\) of (\d+) bytes named by (\S+),")
INDEXED = ("bai", "csi", "gpus2_bai")
PASSES = {"search": 1, "call": 1, "smooth": 2, "run": 2}     # smooth measures before it runs: the ranges are read twice


def sh(cmd, stdout_path=None, env=None):
    if stdout_path is not None:
        with open(stdout_path, "wb") as fh:
            r = subprocess.run([BIN, *map(str, cmd)], stdout=fh, stderr=subprocess.PIPE, timeout=TIMEOUT, env=env)
    else:
        r = subprocess.run([BIN, *map(str, cmd)], capture_output=True, timeout=TIMEOUT, env=env)
    assert r.returncode == 0, (cmd, r.stderr.decode()[-2000:])
    return r


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("region")
    f = build(tmp, coverage=20)
    data = bam_writer.bgzf(R.inflate(f["bam"].read_bytes()), 4096)
    f["bam"] = tmp / "reads4k.bam"
    f["bam"].write_bytes(data)
    f["data"] = data
    sub, n_in, n_all = R.subset_bam(data, INTERVALS, 4096)
    assert 0.05 * n_all <= n_in <= 0.60 * n_all, (n_in, n_all)
    f["n_in"], f["n_all"] = n_in, n_all
    f["sub"] = tmp / "subset.bam"
    f["sub"].write_bytes(sub)
    f["bed"] = tmp / "loci.bed"
    f["bed"].write_text(BED)
    f["region_args"] = REGION_ARGS + ["--regions-file", str(f["bed"])]
    # the specific strings `call` is given: those of the whole file's chain (lines of reads outside the regions are ignored,
    # as they are for a file that lacks those reads)
    e = env0(**SMALL)
    sh(["smooth", "--reference", f["fa"], "--bam", f["bam"]], tmp / "S.bam", e)
    sh(["search", "--index", f["fmd"], "--bam", tmp / "S.bam"], tmp / "T.sfs", e)
    f["sfs"] = tmp / "T.sfs"
    assert os.path.getsize(f["sfs"]) > 0
    f["want"] = {}
    return f


def index_for(fx, cond):
    for ext in (".bai", ".csi"):
        if os.path.exists(str(fx["bam"]) + ext):
            os.remove(str(fx["bam"]) + ext)
    if cond in ("bai", "gpus2_bai", "stale_bai"):
        open(str(fx["bam"]) + ".bai", "wb").write(bam_writer.bai(fx["data"]))
        if cond == "stale_bai":
            old = os.path.getmtime(fx["bam"]) - 100
            os.utime(str(fx["bam"]) + ".bai", (old, old))
    elif cond == "csi":
        open(str(fx["bam"]) + ".csi", "wb").write(bam_writer.csi(fx["data"]))


def outputs(fx, command, bam, tag, extra, env):
    """the command on `bam`: what it wrote, as a dict of bytes (BAM outputs inflated)"""
    tmp = fx["tmp"]
    if command == "search":
        r = sh(["search", "--index", fx["fmd"], "--bam", bam, "--threads", "3", "--bsize", "60", "--verbose", *extra], env=env)
        return {"stdout": r.stdout}, r.stderr.decode()
    if command == "smooth":
        out = tmp / f"{tag}.smooth.bam"
        r = sh(["smooth", "--reference", fx["fa"], "--bam", bam, "--accp", "0.9", "--verbose", *extra], out, env)
        return {"stream": R.inflate(out.read_bytes())}, r.stderr.decode()
    if command == "call":
        poa, clu = tmp / f"{tag}.poa.sam", tmp / f"{tag}.clusters.txt"
        r = sh(["call", "--reference", fx["fa"], "--bam", bam, "--sfs", fx["sfs"], "--poa", poa, "--clusters", clu, "--verbose", *extra], env=env)
        return {"vcf": r.stdout, "poa": poa.read_bytes(), "clusters": clu.read_bytes()}, r.stderr.decode()
    poa, clu, sfs, smo = tmp / f"{tag}.run.poa.sam", tmp / f"{tag}.run.clusters.txt", tmp / f"{tag}.run.sfs", tmp / f"{tag}.run.bam"
    r = sh(["run", "--reference", fx["fa"], "--bam", bam, "--index", fx["fmd"], "--poa", poa, "--clusters", clu, "--sfs", sfs, "--smoothed", smo,
            "--verbose", *extra], env=env)
    return {"vcf": r.stdout, "poa": poa.read_bytes(), "clusters": clu.read_bytes(), "sfs": sfs.read_bytes(), "smoothed": R.inflate(smo.read_bytes())}, r.stderr.decode()


def wanted(fx, command):
    if command not in fx["want"]:
        fx["want"][command] = outputs(fx, command, fx["sub"], "want", [], env0(**SMALL))[0]
        w = fx["want"][command]
        # not vacuous: the subset has something to say, and not what the whole file says
        whole = outputs(fx, command, fx["bam"], "whole", [], env0(**SMALL))[0]
        assert all(len(v) > 0 for v in w.values()) and any(w[k] != whole[k] for k in w), command
        if command in ("call", "run"):
            assert sum(1 for l in w["vcf"].split(b"\n") if l and not l.startswith(b"#")) >= 2
    return fx["want"][command]


CASES = [(c, k) for c in ("search", "smooth", "call", "run") for k in CONDITIONS
         if not (c == "run" and k in ("host_reader", "gpus2", "gpus2_bai")) and not (k == "place_host" and c != "call")]


@pytest.mark.parametrize("command,cond", CASES)
def test_a_region_run_is_the_run_on_the_subset_bam(fx, command, cond):
    want = wanted(fx, command)
    index_for(fx, cond)
    opts, env = CONDITIONS[cond]
    got, err = outputs(fx, command, fx["bam"], cond, fx["region_args"] + opts, env0(**SMALL, **env))
    for k in want:
        assert got[k] == want[k], (command, cond, k)
    m = GATED.search(err)
    assert m and int(m.group(1)) == 2, err[-1500:]
    read, gated = int(m.group(2)), int(m.group(3))
    print(command, cond, m.group(0))
    size = len(fx["data"])
    if cond in INDEXED:
        # the ranges of the index: at most their bytes plus two BGZF members each, every pass -- a condition of how the
        # ranges are built; fewer records reach the gate than the file holds
        p = PLAN.search(err)
        assert p and p.group(3).endswith(".csi" if cond == "csi" else ".bai"), err[-1500:]
        n_ranges, plan_bytes = int(p.group(1)), int(p.group(2))
        assert 1 <= n_ranges <= 2 and plan_bytes < size
        assert 0 < read <= PASSES[command] * (plan_bytes + 131072 * n_ranges) and read < PASSES[command] * size
        assert 0 < gated <= PASSES[command] * (fx["n_all"] - fx["n_in"])
        assert "older than" not in err
    else:
        # the whole file, every pass of the command: the file's data bytes (with or without its empty last member) and
        # every record outside the regions, each pass once
        assert "no usable index" in err and not PLAN.search(err)
        assert ("older than" in err) == (cond == "stale_bai")
        assert gated == PASSES[command] * (fx["n_all"] - fx["n_in"])
        if cond == "host_reader":                # (the host reader's bytes are not counted, and the line says so)
            assert read == 0 and "host reader(s) read the WHOLE file" in err
        else:
            assert read in (PASSES[command] * size, PASSES[command] * (size - 28)), (read, size)
            assert "host reader(s)" not in err


def test_the_empty_subset_and_the_whole_file(fx):
    index_for(fx, "noindex")
    e = env0(**SMALL)
    got, err = outputs(fx, "search", fx["bam"], "empty", ["--region", "chrC:45,001-"], e)
    sub, n_in, n_all = R.subset_bam(fx["data"], [(2, 45000, 2**31 - 1)], 4096)
    assert n_in == 0
    (fx["tmp"] / "empty.bam").write_bytes(sub)
    assert got == outputs(fx, "search", fx["tmp"] / "empty.bam", "empty_want", [], e)[0] and got["stdout"] == b""
    assert int(GATED.search(err).group(3)) == n_all
    got, err = outputs(fx, "search", fx["bam"], "all", ["--region", "chrA", "--region", "chrB", "--region", "chrC:1-"], e)
    sub, n_in, n_all = R.subset_bam(fx["data"], [(0, 0, 2**31 - 1), (1, 0, 2**31 - 1), (2, 0, 2**31 - 1)], 4096)
    assert n_in == n_all - 300                      # (all but the unmapped tail)
    (fx["tmp"] / "all.bam").write_bytes(sub)
    assert got == outputs(fx, "search", fx["tmp"] / "all.bam", "all_want", [], e)[0] and len(got["stdout"]) > 0
    assert got == outputs(fx, "search", fx["bam"], "whole2", [], e)[0]     # the unmapped records never were slots
    assert int(GATED.search(err).group(3)) == 300


def test_without_the_options_nothing_is_gated(fx):
    r = sh(["search", "--index", fx["fmd"], "--bam", fx["bam"], "--verbose"], env=env0(**SMALL))
    assert b"gated" not in r.stderr and b"[regions]" not in r.stderr


def test_smooth_with_its_search_follows(fx):
    """smooth --index --sfs --nobam with regions: the SFS text of the same command on the subset BAM"""
    index_for(fx, "bai")
    e = env0(**SMALL)
    tmp = fx["tmp"]
    sh(["smooth", "--reference", fx["fa"], "--bam", fx["sub"], "--index", fx["fmd"], "--sfs", tmp / "want.nobam.sfs", "--nobam"], env=e)
    sh(["smooth", "--reference", fx["fa"], "--bam", fx["bam"], "--index", fx["fmd"], "--sfs", tmp / "got.nobam.sfs", "--nobam", *fx["region_args"]], env=e)
    assert (tmp / "got.nobam.sfs").read_bytes() == (tmp / "want.nobam.sfs").read_bytes() and os.path.getsize(tmp / "want.nobam.sfs") > 0


def test_a_region_that_names_no_chunk_reads_nothing(fx):
    """with an index, a region on a reference without records: no range, no byte of the file's records read, nothing out"""
    import struct
    head, recs = R.split(R.inflate(fx["data"]))
    l_text = struct.unpack_from("<i", head, 4)[0]
    text = head[8:8 + l_text] + b"@SQ\tSN:chrD\tLN:70000\n"
    n_ref = struct.unpack_from("<i", head, 8 + l_text)[0]
    new_head = (b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref + 1) + head[12 + l_text:] +
                struct.pack("<i", 5) + b"chrD\0" + struct.pack("<i", 70000))
    data = bam_writer.bgzf(new_head + b"".join(r for r, tid, pos, end in recs), 4096)
    bam = fx["tmp"] / "with_chrD.bam"
    bam.write_bytes(data)
    open(str(bam) + ".bai", "wb").write(bam_writer.bai(data))
    r = sh(["search", "--index", fx["fmd"], "--bam", bam, "--region", "chrD", "--verbose"], env=env0(**SMALL))
    err = r.stderr.decode()
    p, m = PLAN.search(err), GATED.search(err)
    assert r.stdout == b"" and p and m, err[-1500:]
    assert int(p.group(1)) == 0 and int(p.group(2)) == 0 and int(m.group(2)) == 0 and int(m.group(3)) == 0
    # ... and the same file still gives its records where the region has some
    r2 = sh(["search", "--index", fx["fmd"], "--bam", bam, *REGION_ARGS, "--verbose"], env=env0(**SMALL))
    assert len(r2.stdout) > 0 and int(PLAN.search(r2.stderr.decode()).group(1)) >= 1
