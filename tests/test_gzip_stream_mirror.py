"""tests/mirror/gzipstream.py -- the pure-Python mirror of the chunk-parallel gzip unit (find, measure, chain, marker decode,
resolve, hand-over) -- against gzip.decompress, and the plan it gives for the FASTQ cases: which chunks hold a block start."""
import gzip
import zlib

import pytest

from tests import gzip_cases as G
from tests.mirror import gzipstream as M


def _text_of(data):
    """what zlib makes of the file, trailing bytes that are no header ignored (as gzread does)"""
    out, rest = bytearray(), data
    while rest[:2] == b"\x1f\x8b":
        z = zlib.decompressobj(31)
        out += z.decompress(rest)
        rest = z.unused_data
    return bytes(out)


@pytest.mark.parametrize("name", G.ALL)
def test_mirror_inflates_every_case(name):
    data, text = G.case(name)
    assert _text_of(data) == text
    out, s = M.inflate(data, 16384, 1 << 30)
    assert out == text
    if name in ("level0", "fixed"):
        assert s.declined == M.DECLINE_NO_START and s.declined_at == 10 and s.device_bytes == 0
    if name == "garbage":
        assert s.declined == M.DECLINE_TRAILING and s.device_bytes == len(text)
    if name.startswith("members"):
        assert s.stats["members_finished"] == int(name[-1])


@pytest.mark.parametrize("name", ["fastq1", "run", "repeat", "syncflush", "members3", "header"])
def test_mirror_small_chunks_and_windows(name):
    data, text = G.case(name)
    out, s = M.inflate(data, 4096, 131072)
    assert out == text
    assert s.stats["windows"] >= 1 and s.stats["chunks_on_chain"] > s.stats["windows"]


def test_fake_start_only_lengthens_the_predecessor():
    data, text = G.case("fastq6")
    out, s = M.inflate(data, 65536, 1 << 30, fake=3)
    assert out == text and s.stats["false_starts"] == 1 and s.declined == 0
    base = M.inflate(data, 65536, 1 << 30)[1]
    assert base.stats["false_starts"] == 0 and s.stats["chunks_on_chain"] == base.stats["chunks_on_chain"] - 1


# chunks of the three FASTQ cases, and how many of them hold a dynamic block start (the first one is the known start)
PLAN = {("fastq1", 65536): (14, 14), ("fastq1", 32768): (28, 27), ("fastq1", 16384): (55, 43),
        ("fastq6", 65536): (13, 13), ("fastq6", 32768): (25, 25), ("fastq6", 16384): (50, 49),
        ("fastq9", 65536): (13, 13), ("fastq9", 32768): (25, 25), ("fastq9", 16384): (50, 49)}


@pytest.mark.parametrize("name", ["fastq1", "fastq6", "fastq9"])
def test_plan_of_the_fastq_cases(name):
    data, text = G.case(name)
    w = M.Window(data[10:])
    cand, need = M.prefilter(w.d)
    # the finder meets every true block start and nothing else: the block ends of one walk over the whole stream
    ends = []
    m, end, n, final, bad = M.walk(w, 0, [0], 0, ends=ends)
    assert final and not bad and n == len(text)
    # (behind the last one comes the trailer; the finder looks for dynamic blocks that are not the last: BFINAL 0, BTYPE 2)
    ends = {e for e in ends[:-1] if w.peek(e) & 7 == 4}
    for C in (65536, 32768, 16384):
        n = -(-len(w.d) // C)
        starts = [0] + [M.find_start(w, cand, need, 8 * k * C, min(8 * (k + 1) * C, w.end)) for k in range(1, n)]
        assert (n, sum(1 for s in starts if s >= 0)) == PLAN[(name, C)]
        assert all(s in ends for s in starts[1:] if s >= 0)
        for k in range(1, n):
            first = min((e for e in ends if 8 * k * C <= e < 8 * (k + 1) * C), default=-1)
            assert starts[k] == first, (C, k)


def test_damaged_streams_are_errors():
    for kind in ("bitflip", "crc", "truncated"):
        with pytest.raises(zlib.error):
            M.inflate(G.damaged(kind), 16384, 131072)
    with pytest.raises(Exception):
        gzip.decompress(G.damaged("bitflip"))
