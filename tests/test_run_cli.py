"""`SVDSS run` on the command line (csrc/svdss_main.cpp, csrc/cli_options.h): its usage text, what it requires, its own
option --smoothed and who else may use it, and what it says on a machine without a GPU.  No GPU needed."""
import os
import subprocess

import pytest

from tests import bam_writer
from tests.common import BIN

KNOBS = ("SVDSS_INDEX_CPU", "SVDSS_SMOOTH_HOST", "SVDSS_BAM_DEVICE", "SVDSS_GPU_DEFLATE")


def run(*args, env=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS} if env is None else env
    return subprocess.run([BIN, *map(str, args)], capture_output=True, timeout=120, env=env)


def test_help_and_usage():
    r = run("run", "--help")
    assert r.returncode == 0 and b"Usage: SVDSS run" in r.stderr and r.stdout == b""
    for opt in (b"--smoothed", b"--sfs", b"--write-index", b"--compress", b"--poa", b"--clusters", b"--clipped", b"--noht", b"--bsize"):
        assert opt in r.stderr, opt
    r = run()
    assert r.returncode == 1 and b"run " in r.stderr and b"|run>" in r.stderr          # MAIN_USAGE has a line for it
    r = run("run", "--reference", "a.fa", "--bam", "b.bam")                               # no --index
    assert r.returncode == 1 and b"Usage: SVDSS run" in r.stderr and r.stdout == b""
    r = run("run", "--index", "a.fmd", "--bam", "b.bam")
    assert r.returncode == 1 and b"Usage: SVDSS run" in r.stderr
    r = run("run", "--reference", "a.fa", "--bam", "b.bam", "--index", "a.fmd", "--frobnicate")
    assert r.returncode == 1 and b"does not exist" in r.stderr


@pytest.mark.parametrize("mode", ["smooth", "search", "call"])
def test_smoothed_is_runs_alone(mode, tmp_path):
    out = tmp_path / "s.bam"
    r = run(mode, "--reference", "a.fa", "--bam", "b.bam", "--index", "a.fmd", "--sfs", "c.sfs", "--smoothed", out)
    assert r.returncode == 1 and b"--smoothed is an option of `SVDSS run` only" in r.stderr and r.stdout == b"" and not out.exists()


def test_write_index_and_compress_need_smoothed(tmp_path):
    ix = tmp_path / "s.bai"
    r = run("run", "--reference", "a.fa", "--bam", "b.bam", "--index", "a.fmd", "--write-index", ix)
    assert r.returncode == 1 and b"--write-index needs --smoothed" in r.stderr and r.stdout == b"" and not ix.exists()
    r = run("run", "--reference", "a.fa", "--bam", "b.bam", "--index", "a.fmd", "--compress", "lz")
    assert r.returncode == 1 and b"--compress needs --smoothed" in r.stderr
    r = run("run", "--reference", "a.fa", "--bam", "b.bam", "--index", "a.fmd", "--smoothed", tmp_path / "s.bam", "--compress", "zip")
    assert r.returncode == 1 and b"failed to parse" in r.stderr
    # --write-index on `search` / `call` is refused as before
    r = run("call", "--reference", "a.fa", "--bam", "b.bam", "--sfs", "c.sfs", "--write-index", ix)
    assert r.returncode == 1 and b"--write-index is an option of `SVDSS smooth` only" in r.stderr


def test_run_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a GPU")
    fa = tmp_path / "r.fa"
    fa.write_text(">c\n" + "ACGT" * 500 + "\n")
    bam = tmp_path / "x.bam"
    bam.write_bytes(bam_writer.bam([("c", 2000)], [bam_writer.record("q", 0, 0, 10, 60, [("M", 100)], "ACGT" * 25)]))
    sfs, out, ix = tmp_path / "o.sfs", tmp_path / "o.bam", tmp_path / "o.bai"
    r = run("run", "--reference", fa, "--bam", bam, "--index", tmp_path / "r.fmd", "--sfs", sfs, "--smoothed", out, "--write-index", ix)
    assert r.returncode == 1 and b"no GPU found" in r.stderr and r.stdout == b""
    assert not sfs.exists() and not out.exists() and not ix.exists()
