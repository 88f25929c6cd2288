"""`SVDSS run --build-index` on the command line (csrc/svdss_main.cpp): the usage text, who may use the option, and the
refusals -- each before anything is opened for writing.  No GPU needed."""
import os
import subprocess

import pytest

from tests import bam_writer
from tests.common import BIN

KNOBS = ("SVDSS_INDEX_CPU", "SVDSS_SMOOTH_HOST", "SVDSS_BAM_DEVICE", "SVDSS_GPU_DEFLATE", "SVDSS_FMD_ENCODE_DEVICE")


def run(*args, env=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS} if env is None else env
    return subprocess.run([BIN, *map(str, args)], capture_output=True, timeout=120, env=env)


@pytest.fixture()
def data(tmp_path):
    fa = tmp_path / "r.fa"
    fa.write_text(">c\n" + "ACGT" * 500 + "\n")
    bam = tmp_path / "x.bam"
    bam.write_bytes(bam_writer.bam([("c", 2000)], [bam_writer.record("q", 0, 0, 10, 60, [("M", 100)], "ACGT" * 25)]))
    return tmp_path, fa, bam


def left_behind(tmp_path, keep):
    return sorted(p.name for p in tmp_path.iterdir() if p.name not in keep)


def test_usage_lists_the_option():
    r = run("run", "--help")
    assert r.returncode == 0 and b"--build-index" in r.stderr
    # without --index the usage text, with or without the option (tests/test_run_cli.py pins the first)
    r = run("run", "--reference", "a.fa", "--bam", "b.bam", "--build-index")
    assert r.returncode == 1 and b"Usage: SVDSS run" in r.stderr and b"--build-index" in r.stderr and r.stdout == b""


@pytest.mark.parametrize("mode", ["smooth", "search", "call", "bamindex", "index"])
def test_build_index_is_runs_alone(mode, data):
    tmp, fa, bam = data
    fmd = tmp / "r.fmd"
    args = {"index": ["-d", fa, "-o", fmd, "--build-index"],
            "bamindex": ["--bam", bam, "--build-index"]}.get(mode, ["--reference", fa, "--bam", bam, "--index", fmd, "--sfs", tmp / "c.sfs", "--build-index"])
    r = run(mode, *args)
    assert r.returncode == 1 and b"--build-index is an option of `SVDSS run` only" in r.stderr and r.stdout == b""
    assert left_behind(tmp, {"r.fa", "x.bam"}) == []


def test_unreadable_reference_is_refused_first(data):
    tmp, fa, bam = data
    r = run("run", "--reference", tmp / "none.fa", "--bam", bam, "--index", tmp / "r.fmd", "--build-index", "--sfs", tmp / "o.sfs")
    assert r.returncode == 1 and b"run --build-index: cannot read" in r.stderr and b"none.fa" in r.stderr and r.stdout == b""
    assert left_behind(tmp, {"r.fa", "x.bam"}) == []


def test_index_directory_that_cannot_be_written_is_refused(data):
    tmp, fa, bam = data
    (tmp / "plain").write_text("a file, not a directory")
    for fmd in (tmp / "no_such_dir" / "r.fmd", tmp / "plain" / "r.fmd"):
        r = run("run", "--reference", fa, "--bam", bam, "--index", fmd, "--build-index", "--sfs", tmp / "o.sfs")
        assert r.returncode == 1 and b"run --build-index: cannot write" in r.stderr and r.stdout == b""
        assert b"no GPU found" not in r.stderr
    if os.geteuid() != 0:          # (root writes anywhere: the two cases above hold for every user)
        locked = tmp / "locked"
        locked.mkdir()
        locked.chmod(0o555)
        r = run("run", "--reference", fa, "--bam", bam, "--index", locked / "r.fmd", "--build-index")
        locked.chmod(0o755)
        assert r.returncode == 1 and b"run --build-index: cannot write" in r.stderr
    assert left_behind(tmp, {"r.fa", "x.bam", "plain", "locked"}) == []


def test_missing_index_without_a_gpu(data):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a GPU")
    tmp, fa, bam = data
    fmd = tmp / "sub.r.fmd"
    r = run("run", "--reference", fa, "--bam", bam, "--index", fmd, "--build-index", "--sfs", tmp / "o.sfs", "--smoothed", tmp / "o.bam")
    assert r.returncode == 1 and b"no GPU found" in r.stderr and r.stdout == b""
    assert b"Building FMD index" not in r.stderr
    assert left_behind(tmp, {"r.fa", "x.bam"}) == []
    # ... and with a samples list
    (tmp / "list.txt").write_text(f"{bam}\t{tmp / 'a.vcf'}\n")
    r = run("run", "--reference", fa, "--samples", tmp / "list.txt", "--index", fmd, "--build-index")
    assert r.returncode == 1 and b"no GPU found" in r.stderr
    assert left_behind(tmp, {"r.fa", "x.bam", "list.txt"}) == []


def _no_stamp(stderr):
    """stderr without the time stamps of the log lines"""
    import re
    return re.sub(rb"\[\d{4}-\d\d-\d\d \d\d:\d\d:\d\d\]", b"[]", stderr)


def test_existing_index_is_not_touched_without_a_gpu(data):
    """the option changes nothing where FMD exists: the run says what it says without it (no GPU: that message, not a usage
    text or an unknown option) and the file keeps its bytes and its mtime"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a GPU")
    tmp, fa, bam = data
    fmd = tmp / "r.fmd"
    fmd.write_bytes(b"not an index, but there")
    os.utime(fmd, (1_600_000_000, 1_600_000_000))
    a = run("run", "--reference", fa, "--bam", bam, "--index", fmd)
    b = run("run", "--reference", fa, "--bam", bam, "--index", fmd, "--build-index")
    assert a.returncode == b.returncode == 1 and b"no GPU found: SVDSS run" in b.stderr
    assert _no_stamp(b.stderr) == _no_stamp(a.stderr) and b.stdout == a.stdout == b""
    assert fmd.read_bytes() == b"not an index, but there" and os.stat(fmd).st_mtime == 1_600_000_000
    assert left_behind(tmp, {"r.fa", "x.bam", "r.fmd"}) == []


def test_runs_own_refusals_come_before_the_build(data):
    """a command `run` refuses anyway builds no index first (the host builder stands in for the GPU: it would build)"""
    tmp, fa, bam = data
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["SVDSS_INDEX_CPU"] = "1"
    fmd = tmp / "r.fmd"
    base = ["run", "--reference", fa, "--index", fmd, "--build-index"]
    (tmp / "bad.txt").write_text(f"{bam}\n")                               # one column
    (tmp / "gone.txt").write_text(f"{tmp / 'none.bam'}\t{tmp / 'a.vcf'}\n")
    for args, extra, says in ((["--bam", bam, "--gpus", "2"], {}, b"--gpus other than 1"),
                              (["--bam", bam], {"SVDSS_SMOOTH_HOST": "1"}, b"run needs the device path"),
                              (["--bam", bam], {"SVDSS_BAM_DEVICE": "0"}, b"run needs the device path"),
                              (["--bam", tmp / "none.bam"], {}, b"cannot read"),
                              (["--bam", bam, "--bsize", "0"], {}, b"batch size"),
                              (["--samples", tmp / "bad.txt"], {}, b"bad.txt"),
                              (["--samples", tmp / "gone.txt"], {}, b"cannot read")):
        r = run(*base, *args, env=dict(env, **extra))
        assert r.returncode == 1 and says in r.stderr and b"Building FMD index" not in r.stderr, (args, r.stderr)
        assert left_behind(tmp, {"r.fa", "x.bam", "bad.txt", "gone.txt"}) == []
    # ... and a command it does not refuse gets as far as the build
    r = run(*base, "--bam", bam, env=env)
    assert b"Building FMD index" in r.stderr and fmd.exists() and (tmp / "r.fmd.svdss").exists()


def test_failed_build_leaves_no_file(data):
    """a build that fails (the host builder, on a reference without a sequence) takes FMD, FMD.svdss and FMD.svdss.tmp with it"""
    tmp, fa, bam = data
    empty = tmp / "empty.fa"
    empty.write_text("\n")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["SVDSS_INDEX_CPU"] = "1"
    r = run("run", "--reference", empty, "--bam", bam, "--index", tmp / "e.fmd", "--build-index", "--sfs", tmp / "o.sfs", env=env)
    assert r.returncode == 1 and b"Building FMD index" in r.stderr and b"no sequence in" in r.stderr and r.stdout == b""
    assert left_behind(tmp, {"r.fa", "x.bam", "empty.fa"}) == []
