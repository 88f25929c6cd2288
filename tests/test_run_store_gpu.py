"""svdss_bam_smooth_set_store and svdss_bam_store_select with a names filter (csrc/bam_smooth.hip, csrc/bam_device.hip),
through svdss_amd/bamdev.py.  The reference point is existing code: store A, filled by svdss_bam_select_store_run -- what
`SVDSS call`'s first pass leaves.  Store B, filled by svdss_bam_smooth_run from the same chunks, must hold the same bytes
under the same batch numbers; selections by name must hold every named record and next to nothing else."""
import struct

import pytest

from svdss_amd import bamdev
from tests.run_fixture import build

pytestmark = pytest.mark.gpu
MIN_MAPQ = 20


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = build(tmp_path_factory.mktemp("run_store"), with_index=False)
    f["data"] = f["bam"].read_bytes()
    return f


def everything(n_ref, lens):
    return bamdev.BamFilter(n_ref, regions=[(t, 0, l) for t, l in enumerate(lens)], min_mapq=MIN_MAPQ)


def slim_records(raw, off):
    return [raw[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]


def name_of(rec):
    return rec[36:36 + rec[12] - 1]


@pytest.fixture(scope="module")
def stores(fx):
    """(A, B, S without a store, S with one, batches) per batch size -- filled once, left unchanged"""
    out = {}
    for mb in (256, 1):
        A, B = bamdev.BamStore(), bamdev.BamStore()
        n_a = A.fill_by_select(fx["data"], min_mapq=MIN_MAPQ, batch_bytes=mb << 20)
        s_plain, _ = bamdev.smooth_bam(fx["data"], fx["contigs"], min_mapq=MIN_MAPQ, acc=0.01, batch_bytes=mb << 20)
        s_store, n_b = bamdev.smooth_bam(fx["data"], fx["contigs"], min_mapq=MIN_MAPQ, acc=0.01, batch_bytes=mb << 20, store=B)
        assert n_a == n_b
        out[mb] = (A, B, s_plain, s_store, n_a)
    yield out
    for A, B, *_ in out.values():
        A.close()
        B.close()


@pytest.mark.parametrize("mb", [256, 1])
def test_both_routes_leave_the_same_store(fx, stores, mb):
    A, B, s_plain, s_store, n = stores[mb]
    assert A.batches() == B.batches()
    n_b, complete, n_rec, n_bytes = B.batches()
    print("batches of %d MB: %d stored, %d records, %d bytes" % (mb, n_b, n_rec, n_bytes))
    assert complete and n_b == n and n_rec > 1500 and (mb != 1 or n_b >= 8)
    flt = everything(3, fx["lens"])
    try:
        total = 0
        for seq in range(n_b):
            ra, oa = A.select(seq, flt)
            rb, ob = B.select(seq, flt)
            assert ra == rb and (oa == ob).all(), seq
            total += len(oa) - 1
        assert total == n_rec        # (a region filter that covers every contig brings every stored record down)
    finally:
        flt.close()
    assert s_store == s_plain        # (the smoothing does not notice the store)


def test_the_store_keeps_what_call_keeps_and_smooth_drops(fx, stores):
    A, B, *_ = stores[256]
    flt = everything(3, fx["lens"])
    try:
        recs = [r for seq in range(B.batches()[0]) for r in slim_records(*B.select(seq, flt))]
    finally:
        flt.close()
    names = [name_of(r) for r in recs]
    assert sum(n.startswith(b"orphan") for n in names) == 12 and sum(n.startswith(b"short") for n in names) == 40
    assert b"unmapped" not in names
    for r in recs:
        bs, tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", r, 0)
        assert not flag & (4 | 256 | 2048) and mapq >= MIN_MAPQ
        n1 = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
        assert bs + 4 in (n1, n1 + 7) and len(r) == (bs + 4 + 3) & ~3
        assert r[bs + 4:] == bytes(len(r) - bs - 4)      # (the padding is zero, not what the arena held before)
        if bs + 4 == n1 + 7:
            assert r[n1:n1 + 3] == b"HPi" and struct.unpack_from("<i", r, n1 + 3)[0] in (1, 2)
    assert any(len(r) % 4 == 0 and struct.unpack_from("<i", r, 0)[0] % 4 for r in recs)     # (padding is exercised)


@pytest.mark.parametrize("mb", [256, 1])
def test_selection_by_name(fx, stores, mb):
    A, B, *_ = stores[mb]
    n_b = A.batches()[0]
    flt = everything(3, fx["lens"])
    try:
        all_a = [slim_records(*A.select(seq, flt)) for seq in range(n_b)]
    finally:
        flt.close()
    # the names a search would report: every seventh read, the name that occurs twice, and one that is absent
    present = sorted({name_of(r) for b in all_a for r in b})
    wanted = set(present[::7]) | {fx["twin_name"].encode()}
    by_name = bamdev.BamFilter(3, names=sorted(wanted) + [b"no_such_read"], min_mapq=MIN_MAPQ)
    regions = bamdev.BamFilter(3, regions=[(0, 10000, 60000), (1, 0, 5000)], min_mapq=MIN_MAPQ)
    try:
        extras = 0
        twins = 0
        for seq in range(n_b):
            got = slim_records(*B.select(seq, by_name))
            exact = [r for r in got if name_of(r) in wanted]
            assert exact == [r for r in all_a[seq] if name_of(r) in wanted], seq      # file order, nothing missing
            extras += len(got) - len(exact)
            twins += sum(name_of(r) == fx["twin_name"].encode() for r in got)
            # a regions-only filter gives what it gives without this change: store A's answer
            ra, oa = A.select(seq, regions)
            rb, ob = B.select(seq, regions)
            assert ra == rb and (oa == ob).all()
        print("selection by name: %d names wanted, %d extra record(s) from hash collisions" % (len(wanted), extras))
        assert extras <= 2 and twins == 2
    finally:
        by_name.close()
        regions.close()


def test_a_store_over_its_limit_stays_incomplete(fx, stores):
    _, _, s_plain, _, n = stores[1]
    small = bamdev.BamStore(max_bytes=1 << 20, initial_bytes=1 << 20)
    try:
        s, n_b = bamdev.smooth_bam(fx["data"], fx["contigs"], min_mapq=MIN_MAPQ, acc=0.01, batch_bytes=1 << 20, store=small)
        stored, complete, _, n_bytes = small.batches()
        assert not complete and stored < n_b == n and n_bytes <= 1 << 20
        assert s == s_plain
    finally:
        small.close()
