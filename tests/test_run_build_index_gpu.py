"""`SVDSS run --build-index` on the data set of tests/run_fixture.py: a missing index is built in place -- the files
`SVDSS index -d FA -o FMD` writes -- and the run goes on to the VCF of a run with a prebuilt index; an index that exists
is not touched; a samples list builds once.  And `SVDSS index --verbose` with the device encoder of the .fmd."""
import ctypes as C
import os
import subprocess

import pytest

from svdss_amd._lib import lib
from tests import run_fixture
from tests.common import BIN
from tests.run_fixture import env0

pytestmark = pytest.mark.gpu

TIMEOUT = 240
SMALL = {"SVDSS_BAM_BATCH_MB": "1", "SVDSS_BAM_SLAB_KB": "64"}
STOP = {}      # set by the first abort, segmentation fault or time-out of the module: nothing more is started on the GPU


@pytest.fixture(autouse=True)
def _nothing_after_a_crash():
    if STOP:
        pytest.fail("not started: " + STOP["why"])


def svdss(cmd, tag, **env):
    try:
        r = subprocess.run([BIN, *map(str, cmd)], capture_output=True, timeout=TIMEOUT, env=env0(**dict(SMALL, **env)))
    except subprocess.TimeoutExpired:
        STOP["why"] = f"{tag} ran into its time limit"
        raise
    if r.returncode in (-6, -11, 134, 139, 124, 137):
        STOP["why"] = f"{tag} ended with status {r.returncode}"
        pytest.fail(STOP["why"] + "\n" + r.stderr.decode()[-3000:])
    return r


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("run_build_index")
    fx = run_fixture.build(tmp, coverage=8)                    # (ref.fa.fmd by `SVDSS index -t 8 -d ref.fa -o`)
    r = svdss(["run", "--reference", fx["fa"], "--bam", fx["bam"], "--index", fx["fmd"]], "run with a prebuilt index")
    assert r.returncode == 0, r.stderr.decode()[-2500:]
    fx["vcf"] = r.stdout
    assert fx["vcf"].count(b"\n") > 10
    fx["built"] = tmp / "built" / "x.fmd"
    fx["built"].parent.mkdir()
    r = svdss(["run", "--reference", fx["fa"], "--bam", fx["bam"], "--index", fx["built"], "--build-index"], "run --build-index")
    fx["first"] = r
    return fx


def test_missing_index_is_built_and_the_vcf_is_that_of_a_prebuilt_one(fx):
    r = fx["first"]
    assert r.returncode == 0, r.stderr.decode()[-2500:]
    assert r.stderr.decode().count("[run] [info] Building FMD index: " + str(fx["built"])) == 1
    assert r.stdout == fx["vcf"]
    assert sorted(p.name for p in fx["built"].parent.iterdir()) == ["x.fmd", "x.fmd.svdss"]


def test_the_files_are_those_of_svdss_index(fx):
    """(the sidecar holds no time stamp: all of it is compared)"""
    assert fx["built"].read_bytes() == fx["fmd"].read_bytes()
    assert (fx["built"].parent / "x.fmd.svdss").read_bytes() == (fx["tmp"] / "ref.fa.fmd.svdss").read_bytes()


def test_search_accepts_the_sidecar(fx):
    h, source = C.c_void_p(), C.c_int32(-1)
    assert lib.svdss_index_records_open(str(fx["built"]).encode(), -1, C.byref(h), C.byref(source)) == 0
    lib.svdss_index_free(h)
    assert source.value == 0                                   # REC_SIDECAR: not recovered from the .fmd's BWT
    a = svdss(["search", "--index", fx["built"], "--bam", fx["bam"]], "search --index built")
    b = svdss(["search", "--index", fx["fmd"], "--bam", fx["bam"]], "search --index prebuilt")
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and len(a.stdout) > 1000


def test_a_second_run_leaves_the_index_alone(fx):
    side = fx["built"].parent / "x.fmd.svdss"
    for p in (fx["built"], side):
        os.utime(p, (1_700_000_000, 1_700_000_000))
    r = svdss(["run", "--reference", fx["fa"], "--bam", fx["bam"], "--index", fx["built"], "--build-index"], "second run --build-index")
    assert r.returncode == 0 and r.stdout == fx["vcf"] and b"Building FMD index" not in r.stderr
    assert os.stat(fx["built"]).st_mtime == 1_700_000_000 and os.stat(side).st_mtime == 1_700_000_000
    assert sorted(p.name for p in fx["built"].parent.iterdir()) == ["x.fmd", "x.fmd.svdss"]


def test_samples_build_once(fx):
    d = fx["tmp"] / "samples"
    d.mkdir()
    (d / "list.txt").write_text(f"{fx['bam']}\t{d / 'a.vcf'}\n{fx['bam']}\t{d / 'b.vcf'}\n")
    r = svdss(["run", "--reference", fx["fa"], "--samples", d / "list.txt", "--index", d / "s.fmd", "--build-index", "--verbose"], "run --samples --build-index")
    assert r.returncode == 0, r.stderr.decode()[-2500:]
    assert r.stderr.decode().count("Building FMD index") == 1
    assert (d / "a.vcf").read_bytes() == fx["vcf"] and (d / "b.vcf").read_bytes() == fx["vcf"]
    assert (d / "s.fmd").read_bytes() == fx["fmd"].read_bytes()
    assert (d / "s.fmd.svdss").read_bytes() == (fx["tmp"] / "ref.fa.fmd.svdss").read_bytes()


def test_index_verbose_names_the_encoder(fx):
    out = fx["tmp"] / "dev.fmd"
    r = svdss(["index", "-t", "8", "-d", fx["fa"], "-o", out, "--verbose"], "index, device encoder", SVDSS_FMD_ENCODE_DEVICE="1")
    assert r.returncode == 0, r.stderr.decode()[-2500:]
    line = [l for l in r.stderr.decode().splitlines() if l.startswith("fmd: ")]
    assert len(line) == 1 and line[0].startswith("fmd: encoded on the device: ") and "runs" in line[0] and "planes/plan/chain/emit/download" in line[0]
    assert out.read_bytes() == fx["fmd"].read_bytes()
    r = svdss(["index", "-t", "8", "-d", fx["fa"], "-o", out, "--verbose"], "index, host encoder", SVDSS_FMD_ENCODE_DEVICE="0")
    assert r.returncode == 0 and "fmd: encoded on the host (SVDSS_FMD_ENCODE_DEVICE=0)" in r.stderr.decode()
    assert out.read_bytes() == fx["fmd"].read_bytes()
    # to stdout (the writer never seeks), the variable unset: the device is the default (profiles/fmd_encode.txt)
    r = subprocess.run([BIN, "index", "-t", "8", "--verbose", "-d", str(fx["fa"])], capture_output=True, timeout=TIMEOUT,
                       env={k: v for k, v in env0().items() if k != "SVDSS_FMD_ENCODE_DEVICE"})
    assert r.returncode == 0 and r.stdout == fx["fmd"].read_bytes() and "fmd: encoded on the device: " in r.stderr.decode()
