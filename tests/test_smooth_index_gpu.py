"""`SVDSS smooth --write-index` on the device path: the index fragments reduced on the GPU (csrc/bam_smooth.hip) and folded
on the host give the bytes the host paths give, batch size and carried blocks notwithstanding; with --gpus N (regions, other
member cuts) each run's index describes its own output."""
import os
import subprocess

import pytest

from tests.common import BIN
from tests.test_smooth_index import check_index, exe, smooth, write_fixture  # noqa: F401

pytestmark = pytest.mark.gpu


def test_every_path_writes_the_same_index(tmp_path, exe):  # noqa: F811
    fa, bam = write_fixture(tmp_path)
    env0 = {k: v for k, v in os.environ.items() if k != "SVDSS_SMOOTH_HOST"}
    for ext in ("bai", "csi"):
        got = {}
        for tag, env in (("device", {"SVDSS_DEBUG": "1"}), ("device small batches", {"SVDSS_BAM_BATCH_MB": "1", "SVDSS_BAM_SLAB_KB": "64"}),
                         ("host + gpu walk", {"SVDSS_BAM_DEVICE": "0"}), ("host", {"SVDSS_SMOOTH_HOST": "1"})):
            out = tmp_path / f"{tag.replace(' ', '_')}.bam"
            idx = tmp_path / f"{tag.replace(' ', '_')}.bam.{ext}"
            r = smooth(fa, bam, out, "--write-index", str(idx), env=dict(env0, **env))
            assert r.returncode == 0, r.stderr.decode()
            if tag == "device":
                assert b"device path" in r.stderr
            got[tag] = (out.read_bytes(), idx.read_bytes())
        for tag in got:
            assert got[tag] == got["host"], (ext, tag)
        check_index(exe, tmp_path, tmp_path / "host.bam", tmp_path / f"host.bam.{ext}", n_queries=300)


def test_regions_on_several_gpus_index_their_own_output(tmp_path, exe):  # noqa: F811
    fa, bam = write_fixture(tmp_path)
    env0 = {k: v for k, v in os.environ.items() if k != "SVDSS_SMOOTH_HOST"}
    small = {"SVDSS_GPUS_OVERSUBSCRIBE": "1", "SVDSS_REGION_MIN_KB": "256", "SVDSS_BAM_BATCH_MB": "1", "SVDSS_BAM_SLAB_KB": "64"}
    for k, (gpus, env) in enumerate((("2", {}), ("3", {"SVDSS_SEARCH_FEEDERS": "2"}), ("4", {"SVDSS_REGION_TEST": "1"}),
                                     ("2", {"SVDSS_REGION_TEST": "2"}))):
        e = dict(env0, **small, **env)
        out = tmp_path / f"g{k}.bam"
        idx = tmp_path / f"g{k}.bam.bai"
        r = smooth(fa, bam, out, "--gpus", gpus, "--write-index", str(idx), env=e)
        assert r.returncode == 0, r.stderr.decode()
        check_index(exe, tmp_path, out, idx, n_queries=60, seed=k)
        # to a pipe: the same output and index
        piped, pidx = tmp_path / f"p{k}.bam", tmp_path / f"p{k}.bam.bai"
        with open(piped, "wb") as fh:
            p = subprocess.Popen([BIN, "smooth", "--reference", str(fa), "--bam", str(bam), "--threads", "4", "--min-mapq", "20", "--gpus", gpus,
                                  "--write-index", str(pidx)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
            c = subprocess.Popen(["cat"], stdin=p.stdout, stdout=fh)
            p.stdout.close()
            _, err = p.communicate(timeout=900)
            c.wait(timeout=60)
        assert p.returncode == 0, err.decode()
        check_index(exe, tmp_path, piped, pidx, n_queries=60, seed=k)
