"""The record gate of the device path (svdss_bam_stream_set_regions, gate_kernel in csrc/bam_device.hip) alone, through
svdss_amd/bamdev.py: with intervals set on the stream, every front end -- svdss_bam_batch_run, svdss_bam_select_run,
svdss_bam_select_store_run + svdss_bam_store_select, svdss_bam_smooth_measure / _run -- gives what it gives, ungated, on the
BAM that holds exactly the records a Python filter lets in (tests/region_lib.py: tid >= 0 and [pos, bam_endpos) overlaps an
interval), and n_records still counts the records that were out.

One fixture: about 2,000 records on three references in BGZF members of 4 KB, run in batches of 64 KB, so that records
straddle members and batches everywhere.  Among them, at the boundaries of the interval [BEG, END) of reference 0: a record
that ends exactly at BEG (out), one that starts at END - 1 (in), records without reference length (only S / I, or no CIGAR
at all) at BEG - 1, BEG and END, a record with tid -1, records on a reference without interval, a record over two adjacent
intervals (once), a CIGAR of 60,000 operations in the record (n_cigar has 16 bits: the longest a record can carry is
65,535; this one is summed by a whole wavefront, and its last base decides) and one of 70,000 in a CG tag behind the
two-operation stand-in of the SAM specification (the gate reads the stand-in, on the per-lane path: the 70,000 operations
themselves never reach the long-CIGAR branch), each once with its last base on an
interval's first base (in) and once ending right in front of one (out)."""
import struct

import numpy as np
import pytest

import svdss_amd
from svdss_amd import bamdev, synth
from tests import bam_writer
from tests import region_lib as R

pytestmark = pytest.mark.gpu

LENS = [300000, 100000, 50000]
BEG, END = 100000, 150000
BATCH = 64 << 10
BIG0, BIG1 = 215000, 290000      # first bases of two intervals the long CIGARs run up to
END31 = 2**31 - 1


def _seq(rng, n):
    return synth.to_ascii(rng.integers(1, 5, size=n).astype(np.uint8))


def _with_cg_tag(rec, ops):
    """`rec` (bam_writer.record) with a CG:B,I tag of `ops` behind its other tags"""
    tag = b"CGBI" + struct.pack("<i", len(ops)) + b"".join(struct.pack("<I", (l << 4) | "MIDNSHP=X".index(op)) for op, l in ops)
    body = rec[4:] + tag
    return struct.pack("<i", len(body)) + body


def build_records():
    rng = np.random.default_rng(31)
    items = []     # (tid, pos, record bytes)

    def add(name, tid, pos, cigar, l_seq, flag=0, mapq=60, tags=()):
        items.append((tid if tid >= 0 else 1 << 30, pos,
                      bam_writer.record(name, flag, tid, pos, mapq, cigar, _seq(rng, l_seq), list(tags), bytes(rng.integers(1, 60, size=l_seq).astype(np.uint8)))))

    for k in range(1960):
        tid = int(rng.choice(3, p=[0.62, 0.25, 0.13]))
        l = int(rng.integers(100, 260))
        pos = int(rng.integers(0, LENS[tid] - 400))
        kind = k % 7
        cig = [("M", l)] if kind < 4 else [("S", 7), ("M", l - 50), ("D", 33), ("M", 43)] if kind < 6 else [("M", 60), ("I", l - 100), ("M", 40)]
        flag = 16 if k % 2 else 0
        flag |= 256 if k % 41 == 0 else 2048 if k % 43 == 0 else 0
        add(f"r{k:04d}", tid, pos, cig, l, flag, 5 if k % 37 == 0 else 60, [("HP", "C", 1 + k % 2)] if k % 3 == 0 else [])
    # the boundaries of [BEG, END) on reference 0
    add("ends_at_beg", 0, BEG - 120, [("M", 120)], 120)                  # out
    add("ends_1_past_beg", 0, BEG - 120, [("M", 121)], 121)              # in
    add("starts_at_end_m1", 0, END - 1, [("M", 130)], 130)               # in
    add("starts_at_end", 0, END, [("M", 130)], 130)                      # out
    for tag, pos in (("beg_m1", BEG - 1), ("beg", BEG), ("end_m1", END - 1), ("end", END)):
        add("noref_S_" + tag, 0, pos, [("S", 140)], 140)                 # no reference length: [pos, pos + 1)
        add("noref_I_" + tag, 0, pos, [("S", 20), ("I", 100), ("S", 20)], 140)
        add("nocigar_" + tag, 0, pos, [], 110, mapq=5)                   # n_cigar = 0 (mapq 5: `smooth` leaves them out, as it would)
    add("deletion_reaches_beg", 0, BEG - 300, [("M", 100), ("D", 200), ("M", 100)], 200)   # [BEG - 300, BEG + 100): in
    add("skip_ends_at_beg", 0, BEG - 300, [("M", 100), ("N", 100), ("=", 50), ("X", 50)], 200)   # [BEG - 300, BEG): out
    add("no_tid", -1, 5, [("M", 120)], 120)                              # tid -1, otherwise a record like the others
    add("no_tid_unplaced", -1, -1, [], 120, flag=4, mapq=0)
    add("over_two_adjacent", 0, 119900, [("M", 200)], 200)               # [119900, 120100): both halves of the two-interval gate
    add("last_base", 1, LENS[1] - 150, [("M", 150)], 150)                # covers the last base of reference 1
    add("ends_before_last_base", 1, LENS[1] - 151, [("M", 150)], 150)
    # CIGARs a lane must not walk alone.  60,000 operations in the record (1M 1D ...: 30,000 bases, 60,000 on the
    # reference); 70,000 in a CG tag, the record's own CIGAR the stand-in <l_seq>S <reference length>N
    long_ops = [("M", 1), ("D", 1)] * 30000
    cg_ops = [("M", 1), ("D", 1)] * 35000
    for tag, last in (("in", 0), ("out", -1)):
        add("cigar60k_" + tag, 0, BIG0 - 60000 + 1 + last, long_ops, 30000, mapq=0)
        rec = bam_writer.record("cigar70k_" + tag, 0, 0, BIG1 - 70000 + 1 + last, 0, [("S", 35000), ("N", 70000)], _seq(rng, 35000), [("HP", "C", 1)],
                                bytes(rng.integers(1, 60, size=35000).astype(np.uint8)))
        items.append((0, BIG1 - 70000 + 1 + last, _with_cg_tag(rec, cg_ops)))
    items.sort(key=lambda x: (x[0], x[1]))
    return [r for _, _, r in items]


# the gates: name -> sorted, merged intervals
def _gates():
    g300 = [(0, 1000 * k, 1000 * k + 100) for k in range(250)] + [(1, 2000 * k + 7, 2000 * k + 400) for k in range(49)] + [(1, LENS[1] - 1, LENS[1])]
    assert len(g300) == 300
    return {
        "one": [(0, BEG, END)],
        "two_adjacent": [(0, BEG, 120000), (0, 120000, END)],
        "main": [(0, BEG, END), (0, BIG0, BIG0 + 10), (0, BIG1, BIG1 + 10), (1, LENS[1] - 1, LENS[1])],
        "three_hundred": g300,
        "nothing": [],
        "everything": [(0, 0, END31), (1, 0, END31), (2, 0, END31)],
    }


GATES = _gates()


class Fx:
    pass


@pytest.fixture(scope="module")
def fx():
    f = Fx()
    recs = build_records()
    f.data = bam_writer.bam([(f"c{t}", l) for t, l in enumerate(LENS)], recs)
    raw = R.inflate(f.data)
    f.data = bam_writer.bgzf(raw, 4096)                       # members of 4 KB
    f.head, f.recs = R.split(raw)
    f.n_all = len(f.recs)
    assert 1950 <= f.n_all <= 2050
    f.sub, f.n_in = {}, {}
    for name, gate in GATES.items():
        f.sub[name], f.n_in[name], _ = R.subset_bam(f.data, gate, 4096)
    # the fixture is what the docstring says: the subset neither empty nor everything, the boundary records on their sides,
    # a gated decision on a record that straddles members and batches
    for name in ("one", "two_adjacent", "main", "three_hundred"):
        assert 0.05 * f.n_all <= f.n_in[name] <= 0.60 * f.n_all, (name, f.n_in[name])
    assert f.n_in["nothing"] == 0 and f.n_in["everything"] == f.n_all - 2      # (all but the two records with tid -1)
    names_in = {_name(r) for r, tid, pos, end in f.recs if R.is_in(tid, pos, end, GATES["main"])}
    want_in = {"ends_1_past_beg", "starts_at_end_m1", "noref_S_beg", "noref_I_beg", "nocigar_beg", "noref_S_end_m1", "noref_I_end_m1", "nocigar_end_m1",
               "deletion_reaches_beg", "over_two_adjacent", "last_base", "cigar60k_in", "cigar70k_in"}
    want_out = {"ends_at_beg", "starts_at_end", "noref_S_beg_m1", "noref_I_beg_m1", "nocigar_beg_m1", "noref_S_end", "noref_I_end", "nocigar_end",
                "skip_ends_at_beg", "no_tid", "no_tid_unplaced", "ends_before_last_base", "cigar60k_out", "cigar70k_out"}
    assert want_in <= names_in and not (want_out & names_in)
    assert not any(tid == 2 and R.is_in(tid, pos, end, GATES["main"]) for r, tid, pos, end in f.recs) and any(tid == 2 for r, tid, pos, end in f.recs)
    cuts, acc, at = [], 0, 0
    for coff, clen, isize, crc in svdss_amd.bgzf.bgzf_blocks(f.data):
        acc += isize
        at += isize
        if acc >= BATCH:
            cuts.append(at)
            acc = 0
    assert len(cuts) >= 8
    off = len(f.head)
    f.straddlers = set()
    for r, tid, pos, end in f.recs:
        if any(off < c < off + len(r) for c in cuts):
            f.straddlers.add(_name(r))
        off += len(r)
    assert {"cigar60k_in", "cigar60k_out", "cigar70k_in"} <= f.straddlers and len(f.straddlers) >= 8
    rng = np.random.default_rng(2)
    f.contigs = [_seq(rng, l) for l in LENS]
    return f


def _name(rec):
    return rec[36:36 + rec[12] - 1].decode()


def _call_keeps(rec, min_mapq=0):
    flag = struct.unpack_from("<H", rec, 18)[0]
    return not (flag & (4 | 256 | 2048)) and rec[13] >= min_mapq


def _python_filter(fx, gate):
    return [r for r, tid, pos, end in fx.recs if R.is_in(tid, pos, end, gate)]


@pytest.mark.parametrize("gate", sorted(GATES))
def test_select_run(fx, gate):
    got, stats = bamdev.select_bam(fx.data, min_mapq=0, batch_bytes=BATCH, gate=GATES[gate])
    want = [r[4:] for r in _python_filter(fx, GATES[gate]) if _call_keeps(r)]
    assert [g[32:32 + g[8] - 1] for g in got] == [w[32:32 + w[8] - 1] for w in want]     # (the names first: a readable failure)
    assert got == want
    # the records that were out are still records of their batches
    assert stats["records"] == fx.n_all and stats["gated"] == fx.n_all - fx.n_in[gate] and stats["batches"] >= 8
    # ... and the ungated run on the subset BAM says the same
    assert bamdev.select_bam(fx.sub[gate], min_mapq=0, batch_bytes=BATCH)[0] == got


@pytest.mark.parametrize("gate", ["main", "three_hundred", "nothing"])
def test_select_store_run_and_store_select(fx, gate):
    """the names filter of the first pass and the stored slim records, selected by position afterwards: neither sees a
    record that is out, whatever the filter says"""
    names = [_name(r) for r, tid, pos, end in fx.recs][::3] + ["no_tid", "ends_at_beg", "starts_at_end_m1", "cigar60k_in", "cigar60k_out"]
    regions = [(0, 0, LENS[0]), (1, 50000, LENS[1]), (2, 0, 10000)]
    got = bamdev.select_bam_store(fx.data, names, regions, min_mapq=20, batch_bytes=BATCH, gate=GATES[gate])
    want = bamdev.select_bam_store(fx.sub[gate], names, regions, min_mapq=20, batch_bytes=BATCH)
    assert got[0] == want[0] and got[1] == want[1]
    inside = [r for r in _python_filter(fx, GATES[gate]) if _call_keeps(r, 20)]
    assert got[2]["stored_records"] == want[2]["stored_records"] == len(inside) and got[2]["complete"] == 1
    assert got[2]["records"] == fx.n_all and got[2]["gated"] == fx.n_all - fx.n_in[gate]
    assert sorted({g[32:32 + g[8] - 1].decode() for g in got[0]}) == sorted({_name(r) for r in inside} & set(names))
    if gate == "main":
        assert got[0] and got[1]


@pytest.fixture(scope="module")
def index():
    ref = synth.make_reference([20000], seed=7)
    return svdss_amd.FMDIndex.build(ref).to_device(0)


@pytest.mark.parametrize("gate", ["one", "main", "three_hundred", "nothing", "everything"])
def test_batch_run(fx, index, gate):
    """svdss_bam_batch_run: an out record is no slot.  (Ungated, the record with tid -1 and no flag 4 ends the run with the
    reference's "core.tid < 0" -- gated it is out like on the subset BAM, which does not hold it.)"""
    got, stats = bamdev.search_bam(index, fx.data, batch_bytes=BATCH, gate=GATES[gate])
    want, wstats = bamdev.search_bam(index, fx.sub[gate], batch_bytes=BATCH)
    assert got == want
    slots = [_name(r) for r in _python_filter(fx, GATES[gate])
             if not (struct.unpack_from("<H", r, 18)[0] & (4 | 256 | 2048)) and struct.unpack_from("<i", r, 20)[0] >= 100]
    assert [g[0] for g in got] == slots
    assert stats["records"] == fx.n_all and stats["gated"] == fx.n_all - fx.n_in[gate] and wstats["records"] == fx.n_in[gate]
    if gate not in ("nothing",):
        assert any(g[2] for g in got)           # (random reads against a random reference: there are specific strings)


def test_batch_run_ungated_still_refuses_a_placed_record_without_reference(fx, index):
    with pytest.raises(svdss_amd._lib.SvdssError) as e:
        bamdev.search_bam(index, fx.data, batch_bytes=BATCH)
    assert "core.tid < 0" in getattr(e.value, "detail", "")


@pytest.mark.parametrize("gate", ["one", "two_adjacent", "main", "three_hundred", "nothing", "everything"])
def test_smooth_measure_and_run(fx, gate):
    """an out record is dropped like an unmapped one, in the measure pass and in the run: the inflated output stream and the
    measured matches / mismatches are those of the subset BAM (the members may be cut elsewhere: the batches end elsewhere)"""
    m_got, c_got = bamdev.smooth_bam(fx.data, fx.contigs, min_mapq=20, batch_bytes=BATCH, gate=GATES[gate], measure=True)
    m_want, c_want = bamdev.smooth_bam(fx.sub[gate], fx.contigs, min_mapq=20, batch_bytes=BATCH, measure=True)
    assert m_got == m_want and sum(k for n, k in c_got) == sum(k for n, k in c_want) == len(m_got)
    assert sum(n for n, k in c_got) == fx.n_all and sum(n for n, k in c_want) == fx.n_in[gate]
    got, _ = bamdev.smooth_bam(fx.data, fx.contigs, min_mapq=20, acc=0.5, batch_bytes=BATCH, gate=GATES[gate])
    want, _ = bamdev.smooth_bam(fx.sub[gate], fx.contigs, min_mapq=20, acc=0.5, batch_bytes=BATCH)
    assert R.inflate(got) == R.inflate(want)
    kept = [r for r in _python_filter(fx, GATES[gate]) if _call_keeps(r, 20)]
    assert [_name(r) for r, tid, pos, end in R.split(R.inflate(got))[1]] == [_name(r) for r in kept]
    if gate == "one":
        assert len(m_got) > 100


def test_set_regions_refuses_what_is_not_sorted_merged_or_in_time(fx):
    import ctypes as C
    from svdss_amd._lib import lib

    def rc_of(gate, n_ref=3):
        s = C.c_void_p()
        assert lib.svdss_bam_stream_create(n_ref, C.byref(s)) == 0
        try:
            bamdev.set_gate(s, gate)
            return 0
        except svdss_amd._lib.SvdssError as e:
            return e.code
        finally:
            lib.svdss_bam_stream_free(s)
    assert rc_of([(0, 5, 9), (0, 9, 12), (2, 0, 1)]) == 0
    for bad in ([(1, 0, 5), (0, 0, 5)], [(0, 10, 20), (0, 5, 8)], [(0, 0, 10), (0, 9, 12)], [(0, 5, 5)], [(3, 0, 5)], [(-1, 0, 5)], [(0, -1, 5)]):
        assert rc_of(bad) != 0, bad


def test_ranges_of_the_file_as_one_stream(fx):
    """SVDSS_BAM_SKIP_RESTART, the way a region run with an index reads the file: three ranges of members, each beginning
    at a record's start inside its first member and ending at a member's end, inside a record.  What comes out is every
    record that lies wholly in a range at or behind the range's first record, in order -- nothing of the record a range's
    end cut, nothing twice -- with and without a gate."""
    blocks = svdss_amd.bgzf.bgzf_blocks(fx.data)
    u_at = np.concatenate([[0], np.cumsum([b[2] for b in blocks])])          # inflated offset of every block
    starts, at = [], len(fx.head)
    for r, tid, pos, end in fx.recs:
        starts.append(at)
        at += len(r)
    ends = starts[1:] + [at]

    def block_of(u):
        return int(np.searchsorted(u_at, u, side="right") - 1)
    picks = [(0, 180), (400, 520), (900, 901)]           # records first .. last (exclusive) that bound each range
    ranges, want = [], []
    for k, (a, z) in enumerate(picks):
        b0 = 0 if k == 0 else block_of(starts[a])
        skip = len(fx.head) if k == 0 else starts[a] - int(u_at[b0])
        b1 = block_of(ends[z - 1] - 1) + 1
        ranges.append((b0, b1, skip))
        lo, hi = (len(fx.head) if k == 0 else starts[a]), int(u_at[b1])
        want.append([i for i in range(len(fx.recs)) if starts[i] >= lo and ends[i] <= hi])
    assert all(x[1] <= y[0] for x, y in zip(ranges, ranges[1:])) and all(0 <= r[2] < 65536 or k == 0 for k, r in enumerate(ranges))
    assert any(ends[w[-1]] < int(u_at[r[1]]) for w, r in zip(want, ranges))      # a range's end cuts a record
    flat = [i for w in want for i in w]
    for gate in (None, GATES["main"], GATES["three_hundred"]):
        got = bamdev.select_bam_ranges(fx.data, ranges, batch_blocks=16, gate=gate)
        exp = [fx.recs[i][0][4:] for i in flat if _call_keeps(fx.recs[i][0]) and (gate is None or R.is_in(*fx.recs[i][1:], gate))]
        assert got == exp
    assert len(flat) > 250
