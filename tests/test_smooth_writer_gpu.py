"""The three ways the device path of `SVDSS smooth` (csrc/smooth_host.cpp) gets its batches to stdout -- in order to a
pipe, side-by-side pwrite writers into a regular file, and the ordered route an O_APPEND stdout or
SVDSS_SMOOTH_SERIAL_WRITE=1 forces -- write the same bytes, and those are the host pipeline's.  Batches of one megabyte:
the stream has several of them."""
import os
import subprocess

import pytest

from tests import test_smooth
from tests.common import BIN

pytestmark = pytest.mark.gpu
SMALL = {"SVDSS_BAM_BATCH_MB": "1", "SVDSS_BAM_SLAB_KB": "64"}


@pytest.fixture(scope="module")
def smooth_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("writer")
    fa, bam, _, _, _ = test_smooth.mirror_input(d)
    cmd = [BIN, "smooth", "--reference", str(fa), "--bam", str(bam), "--threads", "3"]

    def run(stdout, **env):
        r = subprocess.run(cmd, stdout=stdout, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, **SMALL, **env))
        assert r.returncode == 0, r.stderr.decode()
        return r

    piped = run(subprocess.PIPE, SVDSS_DEBUG="1")
    assert b"device path" in piped.stderr and len(piped.stdout) > 100000
    return d, run, piped.stdout


def to_file(run, path, mode="wb", **env):
    with open(path, mode) as fh:
        run(fh, **env)
    return path.read_bytes()


def test_pipe_and_side_by_side_writers_write_the_same_bytes(smooth_input):
    d, run, piped = smooth_input
    assert to_file(run, d / "default.bam") == piped
    assert to_file(run, d / "one_writer.bam", SVDSS_SMOOTH_WRITERS="1") == piped


def test_serial_write_to_a_file_writes_the_same_bytes(smooth_input):
    d, run, piped = smooth_input
    assert to_file(run, d / "serial.bam", SVDSS_SMOOTH_SERIAL_WRITE="1") == piped


def test_append_keeps_what_the_file_held(smooth_input):
    d, run, piped = smooth_input
    old = bytes(range(100))
    (d / "append.bam").write_bytes(old)
    got = to_file(run, d / "append.bam", mode="ab")
    assert got[:100] == old and got[100:] == piped


def test_every_route_writes_the_host_pipeline_s_bytes(smooth_input):
    d, run, piped = smooth_input
    assert run(subprocess.PIPE, SVDSS_SMOOTH_HOST="1").stdout == piped
