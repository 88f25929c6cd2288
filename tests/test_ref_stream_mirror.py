"""The reference stream's mirror (tests/mirror/refstream.py: the shape as a predicate, the batch-by-batch state machine)
against tests.mirror.fastx.reader_records with the sequences upper-cased -- what FastxReader::next and the toupper of
load_chromosomes give: on the cases of tests/ref_cases.py and on a seeded fuzz of 200 files under random cuts."""
import numpy as np
import pytest

from tests import ref_cases as RC
from tests.mirror import fastx as M
from tests.mirror import refstream as R

DELIVERED = RC.delivered_cases()
DECLINED = RC.declined_cases()


def want_of(data):
    return [(n, R.upper(s)) for n, s in M.reader_records(data)]


def all_ways(data):
    """the chunks of every way the GPU suite runs a delivered case, and a few cuts of its own"""
    for _, batch, bgzf in RC.WAYS:
        yield RC.chunks_of(data, batch, RC.members(data) if bgzf else None)
    yield [data[i:i + 1] for i in range(0, min(len(data), 3000))] + [data[3000:]]


@pytest.mark.parametrize("case", DELIVERED, ids=[c[0] for c in DELIVERED])
def test_delivered(case):
    _, data, cap = case
    cap = cap or R.DEFAULT_HEADER_CAP
    assert R.declines(data, cap) is None
    want = want_of(data)
    assert R.whole_file_records(data) == want
    for chunks in all_ways(data):
        assert b"".join(chunks) == data
        assert R.run(chunks, cap) == (want, None)


def test_cuts():
    data, cases = RC.cut_cases()
    want = want_of(data)
    assert R.declines(data) is None and len(want) == 8
    for _, pieces, _eof in cases:                      # (the text of the batches is the same with and without the EOF member)
        assert b"".join(pieces) == data
        for batch in (1 << 20, 1):
            assert R.run(RC.chunks_of(data, batch, pieces)) == (want, None)


@pytest.mark.parametrize("case", DECLINED, ids=[c[0] for c in DECLINED])
def test_declined(case):
    _, data, cap, why = case
    cap = cap or R.DEFAULT_HEADER_CAP
    assert R.declines(data, cap) == why
    for batch in (1 << 20, 1000, 7):
        recs, declined = R.run(RC.chunks_of(data, batch, None), cap)
        assert recs is None and declined[0] == why


def test_header_cap_edges():
    line = b">" + b"n" * 99
    for cap, ok in ((100, True), (99, False)):
        data = b">a\nAC\n" + line + b"\nGG\n"
        assert (R.declines(data, cap) is None) == ok
        for batch in (1 << 20, 64, 1):
            recs, declined = R.run(RC.chunks_of(data, batch, None), cap)
            assert (declined is None) == ok and (ok or declined[0] == R.LONG_HEADER)


def test_fuzz():
    rng = np.random.default_rng(4242)
    accepted = 0
    for _ in range(200):
        data, batch, pieces = RC.fuzz_file(rng)
        why = R.declines(data)
        cuts = sorted(int(x) for x in rng.integers(0, len(data) + 1, size=int(rng.integers(0, 9))))
        ways = [RC.chunks_of(data, batch, pieces), [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]]
        for chunks in ways:
            recs, declined = R.run(chunks)
            if why is None:
                assert declined is None and recs == want_of(data)
            else:
                assert recs is None and declined is not None
        accepted += why is None
    assert accepted >= 100
