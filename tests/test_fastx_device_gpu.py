"""`search --fastx` with the records found on the GPU (svdss_amd/csrc/fastx_device.hip).  Library level: parse only
(ix = NULL), record for record against tests/mirror/fastx.py -- names, nt6 symbols, offsets, the batch that declines and
the text it leaves -- over the shapes, sizes around the tile of the kernels, BGZF member cuts, batches down to one member
and the files the parser declines; a seeded fuzz in which no eligible file may go through the host reader.  Binary level:
the stdout bytes of `SVDSS search --fastx` against SVDSS_FASTX_DEVICE=0, and the --verbose line that says where the
batches went."""
import os
import re
import subprocess

import numpy as np
import pytest

import svdss_amd
from svdss_amd import fastxdev, synth
from tests import fastx_cases as FC
from tests.common import ROOT
from tests.mirror import fastx as M

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "svdss_amd", "SVDSS")
T = fastxdev.tile_bytes()


def check(data, batch, pieces=None, cap=None):
    """the device parser over `data` cut as fastxdev cuts it, against the mirror's plan; returns (declined_at, counters)"""
    chunks = FC.chunks_of(data, batch, pieces)
    want, want_declined, want_rest = M.plan(chunks, batch if cap is None else cap)
    blob = M.bgzf_pack(pieces) if pieces is not None else data
    names, flat, offs, declined_at, st = fastxdev.parse_fastx(blob, batch, bgzf=pieces is not None, carry_cap=cap)
    assert st["batches"] == len(chunks)
    assert names == [n for n, _ in want]
    assert list(np.diff(offs)) == [len(s) for _, s in want]
    assert flat.tobytes() == b"".join(M.nt6(s) for _, s in want)
    assert declined_at == want_declined
    assert st["rest"] == want_rest
    assert st["host_batches"] == (0 if want_declined is None else len(chunks) - want_declined)
    return declined_at, st


DELIVERED = FC.delivered_cases(T)
DECLINED = FC.declined_cases(T)


def test_tile_is_what_the_cases_were_sized_for():
    assert T == FC.T_DEFAULT or len(DELIVERED) > 0
    assert T >= 256 and T % 16 == 0


@pytest.mark.parametrize("case", DELIVERED, ids=[c[0] for c in DELIVERED])
def test_delivered_shapes(case):
    _, data = case
    assert M.shape_of(data) or not data
    declined_at, st = check(data, 1 << 20)
    assert declined_at is None and st["host_batches"] == 0
    # the same text as BGZF members cut at odd places, the batches down to 1 KB and to one member
    pieces = [data[i:i + 1777] for i in range(0, len(data), 1777)]
    for batch in (1 << 20, 1024, 1):
        declined_at, _ = check(data, batch, pieces, cap=1 << 20)
        assert declined_at is None
    declined_at, _ = check(data, 1024, cap=1 << 20)
    assert declined_at is None


def test_bgzf_member_cuts():
    rng = np.random.default_rng(21)
    recs = [(b"read_%d/1 some words" % k, FC.seq_of(rng, 300 + 7 * k)) for k in range(12)]
    for data in (FC.fastq(recs), FC.fasta(recs, wrap=60)):
        inside_name = data.index(b"read_5") + 3
        at_newline = data.index(b"\n", inside_name) + 1
        cuts = [0, 1, 2, 3, inside_name, at_newline, at_newline, len(data) // 2, len(data)]    # (1-byte members, an empty one)
        pieces = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        assert b"".join(pieces) == data and b"" in pieces
        for batch in (1 << 20, 1):
            declined_at, st = check(data, batch, pieces, cap=1 << 20)
            assert declined_at is None and st["host_batches"] == 0
        assert check(data, 1 << 20)[0] is None                                                  # the same text as a plain file


def test_records_across_batches():
    rng = np.random.default_rng(22)
    # every record straddles a batch; a record spans three batches under the cap; a batch that is carry alone; an empty last batch
    recs = [(b"s%d" % k, FC.seq_of(rng, 1500 + 13 * k)) for k in range(9)] + [(b"long", FC.seq_of(rng, 2900))]
    for data in (FC.fastq(recs), FC.fasta(recs, wrap=64), FC.fasta(recs)):
        declined_at, st = check(data, 1024, cap=1 << 16)
        assert declined_at is None and st["batches"] >= 15
        pieces = [data[i:i + 1024] for i in range(0, len(data), 1024)]
        declined_at, st = check(data, 1, pieces, cap=1 << 16)                                    # (the EOF member: an empty last batch)
        assert declined_at is None
    # a record beyond the carry cap declines, the records in front of it are delivered
    data = FC.fastq(recs)
    declined_at, st = check(data, 1024, cap=4000)
    assert declined_at is not None and st["host_batches"] > 0


@pytest.mark.parametrize("case", DECLINED, ids=[c[0] for c in DECLINED])
def test_declined(case):
    _, data = case
    assert M.shape_of(data) is None
    for batch in (1 << 20, T, 1000):
        declined_at, st = check(data, batch, cap=1 << 20)
        assert declined_at is not None
        want = M.reader_records(data)
        names, _, _, _, st = fastxdev.parse_fastx(data, batch, carry_cap=1 << 20)
        assert [(n,) for n in names] + [(n,) for n, _ in M.reader_records(st["rest"])] == [(n,) for n, _ in want]


def test_fuzz_eligible_files_never_reach_the_host_reader():
    rng = np.random.default_rng(2024)
    n_eligible = 0
    for k in range(200):
        data, batch, pieces = FC.fuzz_file(rng)
        chunks = FC.chunks_of(data, batch, pieces)
        declined_at, st = check(data, batch, pieces)
        if FC.eligible(data, chunks, batch):
            n_eligible += 1
            assert declined_at is None and st["host_batches"] == 0, k
    assert n_eligible >= 100


# ---- the binary

@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastxdev")
    ref = synth.make_reference([120000, 40000, 300], seed=71, repeat_frac=0.3, n_runs=(200,))
    hap, _ = synth.implant_svs(ref[:2], 6, seed=72, min_len=50, max_len=400)
    flat, offs, _ = synth.simulate_reads(hap, 300, 4000, 0.005, seed=73)
    with open(d / "ref.fa", "w") as fh:
        for i, c in enumerate(ref):
            fh.write(f">c{i}\n{synth.to_ascii(c)}\n")
    r = subprocess.run([BIN, "index", "-t", "4", "-d", str(d / "ref.fa"), "-o", str(d / "ref.fmd")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    recs = [(b"r%d" % i, synth.to_ascii(flat[offs[i]:offs[i + 1]]).encode()) for i in range(len(offs) - 1)]
    fq = FC.fastq(recs)
    (d / "reads.fq").write_bytes(fq)
    (d / "reads.fq.gz").write_bytes(M.bgzf_pack([fq[i:i + 0xff00] for i in range(0, len(fq), 0xff00)]))
    (d / "reads.fa").write_bytes(FC.fasta(recs, wrap=60))
    # declines in its middle batch (of three, at 512 KB): a CRLF record half way
    mid = len(recs) // 2
    (d / "mid.fq").write_bytes(FC.fastq(recs[:mid]) + b"@crlf\r\nACGT\r\n+\r\nIIII\r\n" + FC.fastq(recs[mid:]))
    return d


def run(d, name, args=(), env=None):
    e = dict(os.environ, **(env or {}))
    r = subprocess.run([BIN, "search", "--index", str(d / "ref.fmd"), "--fastx", str(d / name), "--verbose"] + list(args),
                       capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr
    m = re.search(r"FASTX device path: (\d+) batches on the device, (\d+) through the host reader, (\d+) records", r.stderr)
    assert "FASTX mode is not optimized" in r.stderr
    return r.stdout, (tuple(int(x) for x in m.groups()) if m else None)


@pytest.mark.parametrize("name", ["reads.fq", "reads.fq.gz", "reads.fa"])
@pytest.mark.parametrize("args", [(), ("--noassemble",), ("--threads", "3", "--bsize", "7")], ids=["default", "noassemble", "t3b7"])
def test_binary_writes_the_host_path_bytes(case, name, args):
    want, line = run(case, name, args, {"SVDSS_FASTX_DEVICE": "0"})
    assert line is None and want.count("\n") > 300
    got, line = run(case, name, args)
    assert got == want
    assert line is not None and line[0] >= 1 and line[1] == 0 and line[2] == 300
    got, line = run(case, name, args, {"SVDSS_FASTX_BATCH_KB": "64"})
    assert got == want
    assert line[0] > 10 and line[1] == 0 and line[2] == 300


def test_binary_on_three_replicas(case):
    want, _ = run(case, "reads.fq", (), {"SVDSS_FASTX_DEVICE": "0"})
    for name in ("reads.fq", "reads.fq.gz"):
        got, line = run(case, name, ("--gpus", "3"), {"SVDSS_GPUS_OVERSUBSCRIBE": "1", "SVDSS_FASTX_BATCH_KB": "64"})
        assert got == want and line[1] == 0 and line[2] == 300


def test_binary_falls_back_in_the_middle(case):
    want, _ = run(case, "mid.fq", (), {"SVDSS_FASTX_DEVICE": "0"})
    got, line = run(case, "mid.fq", (), {"SVDSS_FASTX_BATCH_KB": "512"})
    assert got == want and want.count("\n") > 300
    assert line[0] >= 1 and line[1] >= 2 and line[2] == 301, line


def test_declined_cases_through_the_binary(case, tmp_path):
    """the mirror's full record list: what the binary reads of every declined file is what the host reader reads"""
    for name, data in DECLINED:
        (tmp_path / "d.fx").write_bytes(data)
        e = dict(os.environ, SVDSS_FASTX_BATCH_KB="4")
        outs = []
        for dev in ("0", "1"):
            r = subprocess.run([BIN, "search", "--index", str(case / "ref.fmd"), "--fastx", str(tmp_path / "d.fx"), "--verbose"],
                               capture_output=True, text=True, timeout=600, env=dict(e, SVDSS_FASTX_DEVICE=dev))
            assert r.returncode == 0, (name, r.stderr)
            outs.append((r.stdout, re.search(r"(\d+) records read", r.stderr).group(1)))
        assert outs[0] == outs[1], name
        assert int(outs[1][1]) == len(M.reader_records(data)), name


def test_corrupt_member_ends_the_run(case, tmp_path):
    blob = bytearray((case / "reads.fq.gz").read_bytes())
    blob[len(blob) // 2] ^= 0x55
    (tmp_path / "bad.fq.gz").write_bytes(bytes(blob))
    r = subprocess.run([BIN, "search", "--index", str(case / "ref.fmd"), "--fastx", str(tmp_path / "bad.fq.gz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "error reading" in r.stderr
