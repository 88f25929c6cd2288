"""`SVDSS run` (csrc/run_host.cpp): smooth, search and call as one process and one pass over the BAM.  The reference point
is existing code alone: S = `smooth`, T = `search` on S, V = `call --bam <original> --sfs T` with the same option values
(run_svdss's chain).  stdout of `run` is held against V byte for byte under every option and every knob that may move work
around but never results; the optional outputs (--sfs, --smoothed, --write-index, --poa, --clusters) against the files of
the three steps."""
import os
import re
import subprocess

import pytest

from tests.common import BIN
from tests.run_fixture import TIMEOUT, build, env0
from tests.test_smooth_index import members, records

pytestmark = pytest.mark.gpu

SMALL = {"SVDSS_BAM_BATCH_MB": "1", "SVDSS_BAM_SLAB_KB": "64"}


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return build(tmp_path_factory.mktemp("run"))


def sh(cmd, stdout_path=None, env=None):
    if stdout_path is not None:
        with open(stdout_path, "wb") as fh:
            r = subprocess.run([BIN, *map(str, cmd)], stdout=fh, stderr=subprocess.PIPE, timeout=TIMEOUT, env=env or env0())
    else:
        r = subprocess.run([BIN, *map(str, cmd)], capture_output=True, timeout=TIMEOUT, env=env or env0())
    assert r.returncode == 0, (cmd, r.stderr.decode()[-2000:])
    return r


class Chain:
    """The three existing commands, each step computed once per option set and kept."""

    def __init__(self, fx):
        self.fx, self.tmp = fx, fx["tmp"]
        self.cache = {}

    def smooth(self, *opts):
        key = ("S",) + opts
        if key not in self.cache:
            out = self.tmp / f"S{len(self.cache)}.bam"
            sh(["smooth", "--reference", self.fx["fa"], "--bam", self.fx["bam"], *opts], out)
            self.cache[key] = out
        return self.cache[key]

    def search(self, *opts):
        key = ("T",) + opts
        if key not in self.cache:
            out = self.tmp / f"T{len(self.cache)}.sfs"
            threads = tuple(opts[opts.index("--threads"):opts.index("--threads") + 2]) if "--threads" in opts else ()
            sh(["search", "--index", self.fx["fmd"], "--bam", self.smooth(*threads), *opts], out)
            self.cache[key] = out
        return self.cache[key]

    def call(self, search_opts=(), call_opts=()):
        """(V, the --poa file, the --clusters file)"""
        key = ("V",) + tuple(search_opts) + ("|",) + tuple(call_opts)
        if key not in self.cache:
            k = len(self.cache)
            poa, clu = self.tmp / f"V{k}.poa.sam", self.tmp / f"V{k}.clusters.txt"
            r = sh(["call", "--reference", self.fx["fa"], "--bam", self.fx["bam"], "--sfs", self.search(*search_opts), "--poa", poa, "--clusters", clu,
                    *call_opts])
            self.cache[key] = (r.stdout, poa, clu)
        return self.cache[key]


@pytest.fixture(scope="module")
def chain(fx):
    """... and the fixture is not vacuous, on V, T and S alone"""
    c = Chain(fx)
    V = c.call()[0]
    rows = [l for l in V.split(b"\n") if l and not l.startswith(b"#")]
    T = c.search().read_bytes()
    print("V: %d records; T: %d lines, %d '*' lines" % (len(rows), T.count(b"\n"), sum(l.startswith(b"*") for l in T.split(b"\n"))))
    assert len(rows) >= 6
    assert b"SVTYPE=INS" in V and b"SVTYPE=DEL" in V
    assert any(l.startswith(b"*") for l in T.split(b"\n"))
    data = c.smooth().read_bytes()
    _, raw = members(data)
    xf = set()
    for name, tid, beg, end, start, stop in records(data):
        at = raw.find(b"XFC", start, stop)
        assert at > 0
        xf.add(raw[at + 3])
    assert {0, 1, 2} <= xf
    assert c.call(call_opts=("--noht",))[0] != V          # (otherwise the HP path is untested)
    return c


def run(fx, tag, *opts, env=None, ok=True):
    cmd = [BIN, "run", "--reference", str(fx["fa"]), "--bam", str(fx["bam"]), "--index", str(fx["fmd"]), *map(str, opts)]
    r = subprocess.run(cmd, capture_output=True, timeout=TIMEOUT, env=env or env0())
    if ok:
        assert r.returncode == 0, (tag, r.stderr.decode()[-2500:])
    return r


# case -> (run's options, environment, search's options of the chain, call's options of the chain)
CASES = {
    "defaults": ((), {}, (), ()),
    "threads3_bsize64": (("--threads", "3", "--bsize", "64"), {}, ("--threads", "3", "--bsize", "64"), ("--threads", "3")),
    "noputative": (("--noputative",), {}, ("--noputative",), ()),
    "noassemble": (("--noassemble",), {}, ("--noassemble",), ()),
    "noht": (("--noht",), {}, (), ("--noht",)),
    "call_thresholds": (("--min-sv-length", "100", "--min-cluster-weight", "3", "-l", "0.9"), {}, (),
                        ("--min-sv-length", "100", "--min-cluster-weight", "3", "-l", "0.9")),
    "lf0": ((), {"SVDSS_SEARCH_LF": "0"}, (), ()),
    "lf1": ((), {"SVDSS_SEARCH_LF": "1"}, (), ()),
    "small_batches": ((), SMALL, (), ()),
    "park_full_index_held_back": ((), dict(SMALL, SVDSS_PARK_MB="1", SVDSS_PARK_ARENA_MB="1", SVDSS_EARLY_HOLD_MS="1500"), (), ()),
    "store_too_small": ((), {"SVDSS_CALL_STORE_MB": "1"}, (), ()),
    "place_host": ((), {"SVDSS_PLACE_HOST": "1"}, (), ()),
    "clipped": (("--clipped",), {}, (), ("--clipped",)),
}
STORE_LINE = re.compile(r"\[run\] record store: (\d+) records, (\d+) bytes in (\d+) of (\d+) batches, (complete|incomplete: the call stage reads the file)")


@pytest.mark.parametrize("case", sorted(CASES))
def test_stdout_is_the_vcf_of_the_three_steps(fx, chain, case):
    opts, env, s_opts, c_opts = CASES[case]
    want = chain.call(s_opts, c_opts)[0]
    r = run(fx, case, *opts, "--verbose", env=env0(**env))
    err = r.stderr.decode()
    m = STORE_LINE.search(err)
    print(case, len(r.stdout), "bytes of VCF;", m.group(0) if m else "no store line")
    assert r.stdout == want
    assert m, err[-2000:]
    assert "[run] [time] smooth + search" in err and "[run] [time] call" in err and "sfs: " in err and "[call] [time]" in err
    # without --smoothed nothing is deflated and nothing brought down
    d = re.search(r"deflate \+ down ([\d.]+)", err)
    assert d and float(d.group(1)) == 0.0 and " 0 BGZF bytes" in err, err[-2000:]
    if case == "store_too_small":
        assert m.group(5).startswith("incomplete") and "pass 1 from the records kept in HBM" not in err
    else:
        assert m.group(5) == "complete" and m.group(3) == m.group(4) and int(m.group(1)) > 0
    if case in ("small_batches", "park_full_index_held_back"):
        assert int(m.group(4)) >= 8


def test_side_files_of_call(fx, chain):
    want, poa, clu = chain.call()
    tmp = fx["tmp"]
    r = run(fx, "side", "--poa", tmp / "run.poa.sam", "--clusters", tmp / "run.clusters.txt")
    assert r.stdout == want
    assert (tmp / "run.poa.sam").read_bytes() == poa.read_bytes() and os.path.getsize(poa) > 0
    assert (tmp / "run.clusters.txt").read_bytes() == clu.read_bytes() and os.path.getsize(clu) > 0


def test_sfs_file(fx, chain):
    tmp = fx["tmp"]
    r = run(fx, "sfs", "--sfs", tmp / "run.sfs")
    assert r.stdout == chain.call()[0]
    assert (tmp / "run.sfs").read_bytes() == chain.search().read_bytes()


def test_smoothed_bam_and_its_index(fx, chain):
    tmp = fx["tmp"]
    S = chain.smooth("--write-index", tmp / "S.bai")
    r = run(fx, "smoothed", "--smoothed", tmp / "run.bam", "--write-index", tmp / "run.bai")
    assert r.stdout == chain.call()[0]
    assert (tmp / "run.bam").read_bytes() == S.read_bytes() == chain.smooth().read_bytes()
    assert (tmp / "run.bai").read_bytes() == (tmp / "S.bai").read_bytes()


def test_smoothed_bam_lz(fx, chain):
    tmp = fx["tmp"]
    S = chain.smooth("--compress", "lz")
    r = run(fx, "lz", "--smoothed", tmp / "run_lz.bam", "--compress", "lz")
    assert r.stdout == chain.call()[0]
    assert (tmp / "run_lz.bam").read_bytes() == S.read_bytes()
    assert S.read_bytes() != chain.smooth().read_bytes()


def test_refusals(fx):
    tmp = fx["tmp"]
    sfs, bam = tmp / "refused.sfs", tmp / "refused.bam"
    for opts, env, word in ((["--gpus", "2"], {}, "out of scope"),
                            ([], {"SVDSS_SMOOTH_HOST": "1"}, "SVDSS_SMOOTH_HOST"),
                            ([], {"SVDSS_BAM_DEVICE": "0"}, "SVDSS_BAM_DEVICE"),
                            ([], {"SVDSS_GPU_DEFLATE": "0"}, "SVDSS_GPU_DEFLATE")):
        r = run(fx, "refused", "--sfs", sfs, "--smoothed", bam, *opts, env=env0(**env), ok=False)
        assert r.returncode != 0 and word in r.stderr.decode(), (opts, env, r.stderr.decode())
        assert r.stdout == b"" and not sfs.exists() and not bam.exists()
