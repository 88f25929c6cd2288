"""`SVDSS smooth --compress runs|lz` (csrc/deflate.hip's two modes through svdss_bam_smooth_set_deflate): the same
records in a smaller file, `runs` the default byte for byte, --write-index still right for the lz file's own member
offsets, `search` blind to the difference, several GPUs, a bad value refused."""
import gzip
import io
import os
import subprocess

import numpy as np
import pytest

from svdss_amd import synth
from tests import bam_writer
from tests.common import BIN
from tests.test_smooth_index import check_index, exe, normaliser, parse_index, records, smooth  # noqa: F401

pytestmark = pytest.mark.gpu
REF_LEN = 150000


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    """a coordinate-sorted BAM of overlapping 8-12 kb reads, 25x over a 150 kb reference, qualities absent"""
    tmp = tmp_path_factory.mktemp("compress")
    rng = np.random.default_rng(21)
    ref = synth.make_reference([REF_LEN], seed=6)
    fa = tmp / "ref.fa"
    fa.write_text(">chr1\n" + synth.to_ascii(ref[0]) + "\n")
    recs, bases = [], 0
    while bases < 25 * REF_LEN:
        l = int(rng.integers(8000, 12000))
        st = int(rng.integers(0, REF_LEN - l))
        seq = ref[0][st:st + l].copy()
        e = rng.random(l) < 0.003
        seq[e] = (seq[e] % 4) + 1
        recs.append((st, bam_writer.record(f"r{len(recs):05d}", 0, 0, st, 60, [("M", l)], synth.to_ascii(seq))))
        bases += l
    recs.sort(key=lambda r: r[0])
    bam = tmp / "in.bam"
    bam.write_bytes(bam_writer.bam([("chr1", REF_LEN)], [r for _, r in recs]))
    return tmp, fa, bam


def env0():
    return {k: v for k, v in os.environ.items() if k not in ("SVDSS_SMOOTH_HOST", "SVDSS_GPU_DEFLATE", "SVDSS_BAM_DEVICE")}


def inflated(path):
    return gzip.GzipFile(fileobj=io.BytesIO(open(path, "rb").read())).read()


@pytest.fixture(scope="module")
def outputs(fixture):
    tmp, fa, bam = fixture
    out = {}
    for tag, extra in (("default", ()), ("runs", ("--compress", "runs")), ("lz", ("--compress", "lz", "--write-index", str(tmp / "lz.bam.bai")))):
        r = smooth(fa, bam, tmp / f"{tag}.bam", *extra, env=dict(env0(), SVDSS_DEBUG="1"))
        assert r.returncode == 0, r.stderr.decode()
        assert b"device path" in r.stderr
        out[tag] = tmp / f"{tag}.bam"
    return out


def test_same_records_smaller_file(outputs):
    a, b = inflated(outputs["lz"]), inflated(outputs["default"])
    assert a == b and len(a) > 5_000_000
    n_lz, n_runs = os.path.getsize(outputs["lz"]), os.path.getsize(outputs["default"])
    print("smoothed BAM: lz %d bytes, runs %d bytes (%.3f)" % (n_lz, n_runs, n_lz / n_runs))
    assert n_lz < n_runs


def test_runs_is_the_default(outputs):
    assert open(outputs["runs"], "rb").read() == open(outputs["default"], "rb").read()


def test_the_index_is_still_right(fixture, outputs, exe):  # noqa: F811
    tmp, fa, bam = fixture
    data = open(outputs["lz"], "rb").read()
    idx = parse_index(open(tmp / "lz.bam.bai", "rb").read())
    norm = normaliser(data)                                   # (asserts that an offset names a member of this file)
    starts = {r[4] for r in records(data)}
    n = 0
    for ref in idx["refs"]:
        for b, (lo, chunks) in ref["bins"].items():
            if b == 37450:                                     # the pseudo-bin: counts, not offsets, in its second chunk
                chunks = chunks[:1]
            for v0, v1 in chunks:
                assert norm(v0) in starts, hex(v0)
                n += 1
        for v in ref["linear"]:
            assert norm(v) in starts or v == 0, hex(v)
    assert n > 10
    # and the whole index against the test writer's own for these bytes, region queries included
    check_index(exe, tmp, outputs["lz"], tmp / "lz.bam.bai", n_queries=60)


def test_search_does_not_care(fixture, outputs):
    import svdss_amd
    tmp, fa, bam = fixture
    ref = synth.make_reference([REF_LEN], seed=6)
    fmd = tmp / "ref.fmd"
    svdss_amd.FMDIndex.build(ref).save(str(fmd))
    got = {}
    for tag in ("lz", "default"):
        r = subprocess.run([BIN, "search", "--index", str(fmd), "--bam", str(outputs[tag]), "--threads", "4"], capture_output=True,
                           timeout=900, env=env0())
        assert r.returncode == 0, r.stderr.decode()
        got[tag] = r.stdout
    assert got["lz"] == got["default"]


def test_two_gpus(fixture, outputs):
    tmp, fa, bam = fixture
    e = dict(env0(), SVDSS_GPUS_OVERSUBSCRIBE="1", SVDSS_REGION_MIN_KB="32", SVDSS_BAM_BATCH_MB="1", SVDSS_BAM_SLAB_KB="64")
    r = smooth(fa, bam, tmp / "lz2.bam", "--gpus", "2", "--compress", "lz", env=e)
    assert r.returncode == 0, r.stderr.decode()
    assert inflated(tmp / "lz2.bam") == inflated(outputs["default"])
    r = smooth(fa, bam, tmp / "runs2.bam", "--gpus", "2", env=e)
    assert r.returncode == 0, r.stderr.decode()
    assert os.path.getsize(tmp / "lz2.bam") < os.path.getsize(tmp / "runs2.bam")


def test_bad_value(fixture):
    tmp, fa, bam = fixture
    r = smooth(fa, bam, tmp / "bad.bam", "--compress", "zip", env=env0())
    assert r.returncode != 0
    assert "zip" in r.stderr.decode() and "failed to parse" in r.stderr.decode(), r.stderr.decode()
