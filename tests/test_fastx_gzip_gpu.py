"""`SVDSS search --fastx reads.fq.gz` on plain (single-stream) gzip with SVDSS_FASTX_GZIP_DEVICE=1: the file is inflated
chunk-parallel on the GPU (csrc/gzip_stream.hip) and its text goes through the FASTX device path as plain-text batches.
The stdout bytes are those of the host reader, of the uncompressed file and of three replicas; the --verbose line says that
the device did the work, and where zlib took over where it did."""
import gzip
import os
import re
import subprocess

import pytest

from svdss_amd import synth
from tests import fastx_cases as FC
from tests import gzip_cases as G
from tests.common import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "svdss_amd", "SVDSS")
SMALL = {"SVDSS_FASTX_GZIP_DEVICE": "1", "SVDSS_GZIP_CHUNK_KB": "16", "SVDSS_GZIP_WINDOW_KB": "128", "SVDSS_FASTX_BATCH_KB": "64"}
LINE = re.compile(r"fastx: gzip on the device: (\d+) windows, (\d+) chunks \((\d+) merged, (\d+) false starts\), (\d+) bytes, "
                  r"find/measure/decode/resolve [\d.]+/[\d.]+/[\d.]+/[\d.]+ ms(?:; the host \(zlib\) took over at byte (\d+) bit (\d) \(([^)]*)\): (\d+) bytes)?")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastxgzip")
    ref = synth.make_reference([120000, 40000, 300], seed=71, repeat_frac=0.3, n_runs=(200,))
    hap, _ = synth.implant_svs(ref[:2], 6, seed=72, min_len=50, max_len=400)
    flat, offs, _ = synth.simulate_reads(hap, 300, 4000, 0.005, seed=73)
    with open(d / "ref.fa", "w") as fh:
        for i, c in enumerate(ref):
            fh.write(f">c{i}\n{synth.to_ascii(c)}\n")
    r = subprocess.run([BIN, "index", "-t", "4", "-d", str(d / "ref.fa"), "-o", str(d / "ref.fmd")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    recs = [(b"r%d" % i, synth.to_ascii(flat[offs[i]:offs[i + 1]]).encode()) for i in range(len(offs) - 1)]
    texts = {"reads.fq": FC.fastq(recs), "reads.fa": FC.fasta(recs, wrap=60),
             "crlf.fq": FC.fastq(recs).replace(b"\n", b"\r\n"),
             "wrapped.fq": b"".join(b"@" + n + b"\n" + s[:2000] + b"\n" + s[2000:] + b"\n+\n" + b"I" * 2000 + b"\n" + b"I" * (len(s) - 2000) + b"\n"
                                    for n, s in recs)}
    for name, t in texts.items():
        (d / name).write_bytes(t)
        (d / (name + ".gz")).write_bytes(gzip.compress(t, 6))
    (d / "mixed.fq.gz").write_bytes(G.mixed_member(texts["reads.fq"]))
    return d


def run(d, name, args=(), env=None, ok=True):
    e = dict(os.environ, **(env or {}))
    r = subprocess.run([BIN, "search", "--index", str(d / "ref.fmd"), "--fastx", str(d / name), "--verbose"] + list(args),
                       capture_output=True, text=True, timeout=600, env=e)
    if ok:
        assert r.returncode == 0, r.stderr
    return r, LINE.search(r.stderr)


@pytest.mark.parametrize("name", ["reads.fq", "reads.fa"])
def test_plain_gzip_gives_the_host_reader_bytes(case, name):
    want, line = run(case, name + ".gz", (), {"SVDSS_FASTX_GZIP_DEVICE": "0"})
    assert line is None and want.stdout.count("\n") > 300
    plain, _ = run(case, name)
    assert plain.stdout == want.stdout
    got, line = run(case, name + ".gz", (), SMALL)
    assert got.stdout == want.stdout
    # the device did it: more than ten chunks and the text but for a last window too short to hold a block start
    assert line is not None, got.stderr
    n = len((case / name).read_bytes())
    assert int(line.group(2)) > 10 and int(line.group(5)) + int(line.group(9) or 0) == n and int(line.group(5)) > 0.8 * n
    assert "FASTX device path:" in got.stderr and ", 0 through the host reader, 300 records" in got.stderr
    three, line = run(case, name + ".gz", ("--gpus", "3"), dict(SMALL, SVDSS_GPUS_OVERSUBSCRIBE="1"))
    assert three.stdout == want.stdout and line is not None and int(line.group(2)) > 10


def test_default_knobs_and_one_window(case):
    want, _ = run(case, "reads.fq.gz", (), {"SVDSS_FASTX_GZIP_DEVICE": "0"})
    got, line = run(case, "reads.fq.gz", (), {"SVDSS_FASTX_GZIP_DEVICE": "1"})
    assert got.stdout == want.stdout and line is not None and int(line.group(1)) == 1
    assert int(line.group(5)) == len((case / "reads.fq").read_bytes()) and line.group(6) is None


@pytest.mark.parametrize("name", ["crlf.fq", "wrapped.fq"])
def test_device_inflate_then_host_tail(case, name):
    """what the FASTX parser declines is still inflated on the device"""
    want, _ = run(case, name + ".gz", (), {"SVDSS_FASTX_GZIP_DEVICE": "0"})
    got, line = run(case, name + ".gz", (), SMALL)
    assert got.stdout == want.stdout and want.stdout.count("\n") > 300
    n = len((case / name).read_bytes())
    assert line is not None and int(line.group(5)) + int(line.group(9) or 0) == n and int(line.group(5)) > 0.8 * n
    m = re.search(r"FASTX device path: (\d+) batches on the device, (\d+) through the host reader", got.stderr)
    assert m and int(m.group(2)) >= 1


def test_zlib_takes_over_mid_file(case):
    """level 6 / stored / level 6 under one header: windows of stored blocks hold no start to find"""
    want, _ = run(case, "reads.fq")
    host, _ = run(case, "mixed.fq.gz", (), {"SVDSS_FASTX_GZIP_DEVICE": "0"})
    assert host.stdout == want.stdout
    got, line = run(case, "mixed.fq.gz", (), SMALL)
    assert got.stdout == want.stdout
    n = len((case / "reads.fq").read_bytes())
    assert line is not None and line.group(6) is not None, got.stderr
    dev, at, host_bytes = int(line.group(5)), int(line.group(6)), int(line.group(9))
    assert n // 3 <= dev < 2 * n // 3 and dev + host_bytes == n and at > 10
    assert line.group(8) == "no dynamic block start in a window"


@pytest.mark.parametrize("kind", ["truncated", "crc"])
def test_damaged_files_end_the_run(case, tmp_path, kind):
    blob = bytearray((case / "reads.fq.gz").read_bytes())
    if kind == "truncated":
        del blob[len(blob) * 2 // 3:]
    else:
        blob[-8] ^= 0xff
    (tmp_path / "bad.fq.gz").write_bytes(bytes(blob))
    with pytest.raises(Exception):
        gzip.decompress(bytes(blob))
    r = subprocess.run([BIN, "search", "--index", str(case / "ref.fmd"), "--fastx", str(tmp_path / "bad.fq.gz")], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **SMALL))
    assert r.returncode != 0 and "bad.fq.gz" in r.stderr and "error reading" in r.stderr
