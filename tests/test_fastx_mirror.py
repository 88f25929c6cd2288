"""tests/mirror/fastx.py against the C++ reader: FastxReader::next restated in Python gives the records the reader gives
(tests/native/fastx_dump.cpp, built here), from files and through the reader's memory source; whenever the mirror calls a
file eligible for the device parser, its parallel restatement -- records from line starts alone -- and its plan over any
cut into batches give the reader's records; a plan that declines leaves the host reader exactly the remaining records."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import fastx_cases as FC
from tests.common import ROOT
from tests.mirror import fastx as M

SRC = os.path.join(ROOT, "tests", "native", "fastx_dump.cpp")
EXE = os.path.join(ROOT, "tests", "native", "_fastx_dump")


@pytest.fixture(scope="module")
def dump():
    hdr = os.path.join(ROOT, "svdss_amd", "csrc", "fastx_reader.h")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", EXE, SRC, "-lz"], check=True)

    def run(path, cut=None):
        r = subprocess.run([EXE, str(path)] + ([str(cut)] if cut else []), capture_output=True, timeout=60)
        assert r.returncode == 0
        lines = r.stdout.split(b"\n")[:-1]
        return [tuple(l.split(b"\t", 1)) for l in lines]
    return run


def _files():
    rng = np.random.default_rng(5)
    recs = [(b"r%d desc" % k, FC.seq_of(rng, n)) for k, n in enumerate([0, 1, 59, 60, 61, 500, 4100])]
    fa, fq = FC.fasta(recs, wrap=60), FC.fastq(recs)
    wrapped_fq = b"@w\nACGT\nGGCC\n+\nIIII\nIIII\n@v\nAC\n+\nII\n"
    out = [("fasta_wrapped", fa), ("fastq", fq), ("fastq_wrapped", wrapped_fq),
           ("fasta_crlf", fa.replace(b"\n", b"\r\n")), ("fastq_crlf", fq.replace(b"\n", b"\r\n")),
           ("blank_lines", b"\n\n" + fa.replace(b">r3", b"\n\n>r3") + b"\n\n"), ("junk_first", b"junk\nmore junk\n" + fq),
           ("truncated", fq + b"@t\nACGT\n+\n"), ("truncated_header", fa + b">t"),
           ("at_headed_fasta", b"@a\nACGT\n>b\nGG\n@c\nTT\nAA\n"), ("empty", b""), ("no_final_newline", fq[:-1])]
    out += [(i, d) for i, d in FC.delivered_cases() + FC.declined_cases() if len(d) < 40000]
    return out


FILES = _files()


@pytest.mark.parametrize("case", FILES, ids=[f[0] for f in FILES])
def test_mirror_reads_what_the_reader_reads(case, dump, tmp_path):
    _, data = case
    p = tmp_path / "f.txt"
    p.write_bytes(data)
    want = dump(p)
    assert M.reader_records(data) == want
    # the reader's memory source, cut into buffers of 1, 7 and 4096 bytes
    for cut in (1, 7, 4096):
        if len(data) < 20000 or cut > 1:
            assert dump(p, cut) == want


def test_compressed_files_read_the_same(dump, tmp_path):
    data = dict(FILES)["fastq"]
    (tmp_path / "f.txt").write_bytes(data)
    (tmp_path / "f.gz").write_bytes(gzip.compress(data))
    (tmp_path / "f.bgz").write_bytes(M.bgzf_pack([data[i:i + 3000] for i in range(0, len(data), 3000)]))
    want = dump(tmp_path / "f.txt")
    assert want == M.reader_records(data)
    assert dump(tmp_path / "f.gz") == want and dump(tmp_path / "f.bgz") == want


def test_eligible_files_parse_in_parallel_like_the_reader():
    for name, data in FC.delivered_cases():
        assert M.shape_of(data) or not data, name
        if data:
            assert M.parallel_records(data) == M.reader_records(data), name
    for name, data in FC.declined_cases():
        assert M.shape_of(data) is None, name


def test_plan_over_batches_property():
    """Seeded files cut into batches: an eligible file is delivered whole and equals the reader; a declined one delivers
    a prefix of the reader's records and leaves the host reader the rest.  At least half of the files are eligible."""
    rng = np.random.default_rng(2024)
    n_eligible = 0
    for k in range(200):
        data, batch, pieces = FC.fuzz_file(rng)
        chunks = FC.chunks_of(data, batch, pieces)
        assert b"".join(chunks) == data
        recs, declined_at, rest = M.plan(chunks, batch)
        want = M.reader_records(data)
        assert recs + M.reader_records(rest) == want, k
        if M.shape_of(data):
            assert M.parallel_records(data) == want, k
        if FC.eligible(data, chunks, batch):
            n_eligible += 1
            assert declined_at is None and recs == want, k
    assert n_eligible >= 100, n_eligible


def test_declined_cases_leave_the_rest_to_the_reader():
    for name, data in FC.declined_cases():
        for batch in (1 << 20, 4096, 1000):
            chunks = FC.chunks_of(data, batch, None)
            recs, declined_at, rest = M.plan(chunks, batch)
            assert declined_at is not None, name
            assert recs + M.reader_records(rest) == M.reader_records(data), (name, batch)
