"""The index of the INPUT BAM on the device path (`SVDSS bamindex`, `call / run --write-bam-index`, `bamdev.index_bam`): the
fragments reduced on the GPU (in_ix_* kernels, csrc/bam_device.hip) and folded on the host give, byte for byte, the file the
host reader writes (SVDSS_BAM_DEVICE=0, held against tests/bam_writer.py by tests/test_bam_input_index.py) -- with batches of
1 MB (records straddle batches; one record is larger than a batch), over the regions of --gpus N with their seams, with regions
that run again, as a by-product of `call` and `run`; and the index is one `--region` reads through."""
import re
import struct
import subprocess

import numpy as np
import pytest

from svdss_amd import bamdev
from tests import bam_input_index_lib as L
from tests import bam_writer
from tests.common import BIN
from tests.test_smooth_index import parse_index

pytestmark = pytest.mark.gpu

SMALL = {"SVDSS_BAM_BATCH_MB": "1", "SVDSS_BAM_SLAB_KB": "64"}
EXTS = ("bai", "csi")


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """the four files, and the host reader's BAI and CSI of each (the reference of every test below)"""
    tmp = tmp_path_factory.mktemp("inix")
    files = L.write_files(tmp)
    files["long"] = L.long_record_file(tmp)
    want = {}
    for tag, bam in files.items():
        for ext in EXTS:
            out = tmp / f"{tag}.host.{ext}"
            r = L.bamindex(bam, out, env=L.env0(SVDSS_BAM_DEVICE="0"))
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            want[tag, ext] = out.read_bytes()
    return {"tmp": tmp, "files": files, "want": want}


@pytest.mark.parametrize("tag", ["b60000", "b997", "concat", "long"])
def test_bamindex_on_the_device_writes_the_host_readers_bytes(fx, tag):
    for ext in EXTS:
        out = fx["tmp"] / f"{tag}.dev.{ext}"
        r = L.bamindex(fx["files"][tag], out, "--verbose", env=L.env0(**SMALL))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"device path" in r.stderr
        assert out.read_bytes() == fx["want"][tag, ext], (tag, ext)
        assert not (fx["tmp"] / f"{tag}.dev.{ext}.tmp").exists()
    if tag == "long":      # the long record did straddle batches: more batches than its own bytes fill
        data = fx["files"][tag].read_bytes()
        recs, _ = L.records(data)
        longest = max(r[6] - r[5] for r in recs)
        assert longest > (1 << 20) + 200000


@pytest.mark.parametrize("gpus", [2, 3, 4, 7])
def test_bamindex_over_regions(fx, gpus):
    env = L.env0(SVDSS_GPUS_OVERSUBSCRIBE="1", SVDSS_REGION_MIN_KB="128", **SMALL)
    seams = 0
    for tag, bam in fx["files"].items():
        for ext in EXTS:
            out = fx["tmp"] / f"{tag}.g{gpus}.{ext}"
            r = L.bamindex(bam, out, "--gpus", str(gpus), "--verbose", env=env)
            assert r.returncode == 0, (tag, r.stderr.decode()[-2000:])
            m = re.search(rb"(\d+) region\(s\), (\d+) seam\(s\), (\d+) region\(s\) run again", r.stderr)
            assert m and int(m.group(1)) == gpus, r.stderr.decode()[-1000:]
            seams += int(m.group(2))
            assert out.read_bytes() == fx["want"][tag, ext], (tag, ext, gpus)
    assert seams > 0


@pytest.mark.parametrize("mode", ["1", "2"])
def test_bamindex_when_regions_run_again(fx, mode):
    """SVDSS_REGION_TEST=1: every region's guess is no record, so every region runs again; =2: the seams do not fit"""
    env = L.env0(SVDSS_GPUS_OVERSUBSCRIBE="1", SVDSS_REGION_MIN_KB="128", SVDSS_REGION_TEST=mode, **SMALL)
    for tag in ("b60000", "long"):
        out = fx["tmp"] / f"{tag}.again{mode}.bai"
        r = L.bamindex(fx["files"][tag], out, "--gpus", "3", "--verbose", env=env)
        assert r.returncode == 0, (tag, r.stderr.decode()[-2000:])
        m = re.search(rb"(\d+) region\(s\), (\d+) seam\(s\), (\d+) region\(s\) run again", r.stderr)
        assert m and int(m.group(3)) >= 1, r.stderr.decode()[-1000:]
        assert out.read_bytes() == fx["want"][tag, "bai"], (tag, mode)


def test_index_bam_returns_the_same_bytes(fx):
    for tag, bam in fx["files"].items():
        data = bam.read_bytes()
        for ext in EXTS:
            assert bamdev.index_bam(data, csi=ext == "csi", batch_bytes=1 << 20) == fx["want"][tag, ext], (tag, ext)
    assert bamdev.index_bam(fx["files"]["b60000"].read_bytes(), batch_bytes=256 << 20) == fx["want"]["b60000", "bai"]      # one batch


def test_the_switch_changes_nothing_else(fx):
    """select_bam and smooth_bam return what they return with the switch off"""
    from tests.test_smooth_index import fixture_records
    from svdss_amd import synth
    data = fx["files"]["b60000"].read_bytes()
    off = bamdev.select_bam(data, min_mapq=20, batch_bytes=1 << 20)
    on = bamdev.select_bam(data, min_mapq=20, batch_bytes=1 << 20, input_index=(14, 5))
    assert off[0] == on[0] and off[1] == on[1] and len(off[0]) > 100
    gate = [(0, 100000, 150000), (1, 0, 30000)]
    assert bamdev.select_bam(data, batch_bytes=1 << 20, gate=gate) == bamdev.select_bam(data, batch_bytes=1 << 20, gate=gate, input_index=(14, 6))
    ref, _ = fixture_records()
    contigs = [synth.to_ascii(c) for c in ref[:2]]
    a = bamdev.smooth_bam(data, contigs, batch_bytes=1 << 20)
    b = bamdev.smooth_bam(data, contigs, batch_bytes=1 << 20, input_index=(14, 5))
    assert a == b and len(a[0]) > 100000


def swap_two_records(bam_path, out_path):
    data = bam_path.read_bytes()
    recs, _ = L.records(data)
    from tests.test_smooth_index import members
    _, raw = members(data)
    k = next(i for i in range(50, len(recs) - 1) if recs[i][1] == recs[i + 1][1] == 0 and recs[i][2] < recs[i + 1][2])
    a, b = recs[k], recs[k + 1]
    raw2 = raw[:a[5]] + raw[b[5]:b[6]] + raw[a[5]:a[6]] + raw[b[6]:]
    out_path.write_bytes(bam_writer.bgzf(raw2, 60000))


def test_an_unsorted_bam_is_refused_by_bamindex(fx):
    bad = fx["tmp"] / "unsorted.bam"
    swap_two_records(fx["files"]["b60000"], bad)
    for env in (L.env0(**SMALL), L.env0()):
        out = fx["tmp"] / "unsorted.bai"
        r = L.bamindex(bad, out, env=env)
        assert r.returncode != 0 and b"not sorted" in r.stderr
        assert not out.exists() and not (fx["tmp"] / "unsorted.bai.tmp").exists()


# ---- the by-product of `call` and `run`, on the data set of tests/test_run_gpu.py
@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    from tests import run_fixture
    tmp = tmp_path_factory.mktemp("inix_run")
    f = run_fixture.build(tmp, coverage=12)
    env = run_fixture.env0(SVDSS_DEBUG="1")

    def sh(*cmd, env=env, ok=True):
        r = subprocess.run([BIN, *map(str, cmd)], capture_output=True, timeout=run_fixture.TIMEOUT, env=env)
        if ok:
            assert r.returncode == 0, (cmd, r.stderr.decode()[-2500:])
        return r
    f["sh"] = sh
    f["env"] = env
    f["run0"] = sh("run", "--reference", f["fa"], "--bam", f["bam"], "--index", f["fmd"], "--sfs", tmp / "T.sfs", "--verbose")
    f["sfs"] = tmp / "T.sfs"
    f["call0"] = sh("call", "--reference", f["fa"], "--bam", f["bam"], "--sfs", f["sfs"])
    r = L.bamindex(f["bam"], tmp / "want.bai", env=run_fixture.env0())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    f["want"] = (tmp / "want.bai").read_bytes()
    assert parse_index(f["want"])["n_no_coor"] == 300
    assert f["call0"].stdout.count(b"\n") > 10 and f["call0"].stdout == f["run0"].stdout
    return f


def _store_line(stderr):
    lines = [l for l in stderr.decode().splitlines() if "record store" in l]
    return [re.sub(r"\d+\.\d+ s", "_ s", l) for l in lines]


@pytest.mark.parametrize("gpus", [1, 3])
def test_call_writes_the_index_of_its_bam(chain, gpus):
    from tests import run_fixture
    tmp = chain["tmp"]
    idx = tmp / f"call{gpus}.bai"
    env = run_fixture.env0(SVDSS_GPUS_OVERSUBSCRIBE="1", SVDSS_REGION_MIN_KB="128", SVDSS_DEBUG="1", **SMALL)
    plain = chain["sh"]("call", "--reference", chain["fa"], "--bam", chain["bam"], "--sfs", chain["sfs"], "--gpus", gpus, env=env)
    r = chain["sh"]("call", "--reference", chain["fa"], "--bam", chain["bam"], "--sfs", chain["sfs"], "--gpus", gpus, "--write-bam-index", idx, env=env)
    assert r.stdout == plain.stdout == chain["call0"].stdout
    assert idx.read_bytes() == chain["want"] and not (tmp / f"call{gpus}.bai.tmp").exists()
    if gpus > 1:
        assert re.search(rb"3 regions of the file", r.stderr), r.stderr.decode()[-1500:]


def test_run_writes_the_index_of_its_bam(chain):
    tmp = chain["tmp"]
    idx = tmp / "run.csi"
    r = chain["sh"]("run", "--reference", chain["fa"], "--bam", chain["bam"], "--index", chain["fmd"], "--sfs", tmp / "T2.sfs", "--verbose",
                    "--write-bam-index", idx)
    assert r.stdout == chain["run0"].stdout
    assert (tmp / "T2.sfs").read_bytes() == chain["sfs"].read_bytes()
    assert _store_line(r.stderr) == _store_line(chain["run0"].stderr) and _store_line(r.stderr)
    want = L.bamindex(chain["bam"], tmp / "want.csi", env=chain["env"])
    assert want.returncode == 0 and idx.read_bytes() == (tmp / "want.csi").read_bytes()
    assert parse_index(idx.read_bytes())["n_no_coor"] == 300


def test_the_written_index_is_one_region_reads_through(chain):
    import shutil
    tmp = chain["tmp"]
    d = tmp / "beside"
    d.mkdir()
    bam = d / "reads.bam"
    shutil.copy(chain["bam"], bam)
    args = ("call", "--reference", chain["fa"], "--bam", bam, "--sfs", chain["sfs"], "--region", "chrB", "--verbose")

    def read_bytes(stderr):
        m = re.search(rb"(\d+) compressed bytes read", stderr)
        assert m, stderr.decode()[-1500:]
        return int(m.group(1))
    without = chain["sh"](*args)
    assert b"no usable index" in without.stderr
    r = L.bamindex(bam, str(bam) + ".bai", env=chain["env"])
    assert r.returncode == 0
    with_ix = chain["sh"](*args)
    assert read_bytes(with_ix.stderr) < read_bytes(without.stderr)
    assert with_ix.stdout == without.stdout and with_ix.stdout.count(b"\n") > 5
    from tests import run_fixture
    ignored = chain["sh"](*args, env=run_fixture.env0(SVDSS_REGION_INDEX="0", SVDSS_DEBUG="1"))
    assert ignored.stdout == without.stdout and read_bytes(ignored.stderr) == read_bytes(without.stderr)


def test_call_on_an_unsorted_bam_warns_and_writes_no_index(chain):
    tmp = chain["tmp"]
    bad = tmp / "unsorted.bam"
    swap_two_records(chain["bam"], bad)
    idx = tmp / "unsorted.bai"
    plain = chain["sh"]("call", "--reference", chain["fa"], "--bam", bad, "--sfs", chain["sfs"])
    r = chain["sh"]("call", "--reference", chain["fa"], "--bam", bad, "--sfs", chain["sfs"], "--write-bam-index", idx)
    assert r.stdout == plain.stdout and r.stdout.count(b"\n") > 10
    assert b"warning" in r.stderr and b"not sorted" in r.stderr
    assert not idx.exists() and not (tmp / "unsorted.bai.tmp").exists()
