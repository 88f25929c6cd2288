"""The BGZF batch intake (svdss_amd/csrc/bgzf_intake.h) through the three units that use it -- the BAM front end
(bamdev.search_bam, bamdev.select_bam), `search --fastx` (fastxdev.parse_fastx) and the reference stream
(refdev.load_reference) -- with a batch handed over as SEVERAL chunks: the 16-byte rounding of chunk offsets in the packed
buffer and the file position the input index carries across chunks, which one chunk per batch never reaches.

A small BAM, FASTQ and FASTA are cut into members of 1, 255, 256, 257, 4097 and 0xff00 inflated bytes with an empty member
in the middle.  How a batch is chunked must not matter (1, 2, 3 chunks; the whole file as one batch, and batches of one
member), and the one-chunk result is what the units' own tests assert for such input (test_bam_device_gpu._check, the
mirrors of test_fastx_device_gpu and test_ref_stream_gpu.want_of).  Damaged members are reported with the same words by
all four, wherever the member's chunk is; a damaged batch gives up its turn in file order."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

import svdss_amd
from svdss_amd import bamdev, bgzf, fastxdev, refdev
from svdss_amd._lib import SvdssError, lib
from tests import bam_input_index_lib as L
from tests import bam_writer
from tests import fastx_cases as FC
from tests import oracle_lib as O
from tests.common import small_workload
from tests.mirror import fastx as M
from tests.test_bam_device_gpu import _check, _raw_bam, _records
from tests.test_ref_stream_gpu import want_of
from tests.test_smooth_index import meta_bin, normaliser, parse_index

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 4097, 0xff00]
WHOLE, ONE_MEMBER = 1 << 30, 1            # batch_bytes: the file as one batch; every member a batch of its own
CHUNKINGS = (1, 2, 3)
MESSAGES = ("BGZF inflate failed", "BGZF block CRC mismatch")


def members_of(data, head=0):
    """`data` as BGZF members of SIZES inflated bytes, in turn, an empty member in the middle (and the EOF member last).
    head: the first `head` bytes -- a BAM's header, which the stream's first batch must hold whole -- are a member of their own
    in front of those."""
    assert len(data) - head >= sum(SIZES)
    pieces, i = [], head
    while i < len(data):
        n = SIZES[len(pieces) % len(SIZES)]
        pieces.append(data[i:i + n])
        i += n
    pieces.insert(len(pieces) // 2, b"")
    if head:
        pieces.insert(0, data[:head])
    return M.bgzf_pack(pieces), pieces


@pytest.fixture(scope="module")
def bam():
    ref, hap, svs, flat, offs = small_workload(seed=93, n_reads=80, read_len=900, ref_lens=(30000,), n_svs=3)
    ix = svdss_amd.FMDIndex.build(ref).to_device(0)
    fm = O.OracleFMD.build(ref)
    reads = [flat[offs[i]:offs[i + 1]].copy() for i in range(80)]
    reads[11] = reads[11][:99]            # l_qseq < 100: dropped, counted
    names = [f"m64/{(i * 37) % 80}/ccs" for i in range(80)]
    recs, slots = _records(names, reads, np.random.default_rng(6))
    data, _ = members_of(_raw_bam([("chr1", 30000)], recs), head=len(_raw_bam([("chr1", 30000)], [])))
    return {"ix": ix, "fm": fm, "recs": recs, "slots": slots, "data": data}


@pytest.fixture(scope="module")
def text():
    rng = np.random.default_rng(94)
    recs = [(b"read_%d/1 some words" % k, FC.seq_of(rng, 1200 + 7 * k)) for k in range(56)]
    out = {}
    for tag, data in (("fastq", FC.fastq(recs)), ("fasta", FC.fasta(recs, wrap=60))):
        blob, pieces = members_of(data)
        out[tag] = (data, blob, pieces)
    return out


def kept_by_call(recs, min_mapq=0):
    """what svdss_bam_select_run keeps without names or regions: no flag 4 / 256 / 2048, mapq >= min_mapq"""
    out = []
    for r in recs:
        mapq, flag = r[4 + 9], struct.unpack_from("<H", r, 4 + 14)[0]
        if not flag & (4 | 256 | 2048) and mapq >= min_mapq:
            out.append(r[4:])
    return out


# ------------------------------------------------------------------ chunking must not matter
def test_search_bam_whatever_the_chunks(bam):
    results = {}
    for batch in (WHOLE, ONE_MEMBER):
        for k in CHUNKINGS:
            results[batch, k] = bamdev.search_bam(bam["ix"], bam["data"], assemble=True, putative=True, batch_bytes=batch, chunks_per_batch=k)
    out, st = results[WHOLE, 1]
    assert st["records"] == len(bam["recs"]) and st["short"] == 1 and st["batches"] == 1
    _check(out, bam["slots"], bam["fm"], True, True)
    # (an empty member is no batch of its own: it goes with the member behind it, the EOF member with the closing batch)
    assert results[ONE_MEMBER, 1][1]["batches"] == sum(1 for b in bgzf.bgzf_blocks(bam["data"]) if b[2] > 0) + 1
    for batch in (WHOLE, ONE_MEMBER):
        for k in CHUNKINGS:
            assert results[batch, k][0] == out, (batch, k)
            assert results[batch, k][1] == results[batch, 1][1], (batch, k)     # records, short, batches, segments, rewalked, gated


def test_select_bam_whatever_the_chunks(bam):
    want = kept_by_call(bam["recs"])
    assert 0 < len(want) < len(bam["recs"])
    for batch in (WHOLE, ONE_MEMBER):
        stats = []
        for k in CHUNKINGS:
            got, st = bamdev.select_bam(bam["data"], batch_bytes=batch, chunks_per_batch=k)
            assert got == want, (batch, k)
            assert st["records"] == len(bam["recs"])
            stats.append(st)
        assert stats[0] == stats[1] == stats[2]


@pytest.mark.parametrize("tag", ["fastq", "fasta"])
def test_parse_fastx_whatever_the_chunks(text, tag):
    data, blob, pieces = text[tag]
    for batch in (WHOLE, ONE_MEMBER):
        chunks = FC.chunks_of(data, batch, pieces)
        want, want_declined, want_rest = M.plan(chunks, 1 << 20)
        assert want_declined is None and len(want) == 56
        stats = []
        for k in CHUNKINGS:
            names, flat, offs, declined_at, st = fastxdev.parse_fastx(blob, batch, bgzf=True, carry_cap=1 << 20, chunks_per_batch=k)
            assert names == [n for n, _ in want], (batch, k)
            assert list(np.diff(offs)) == [len(s) for _, s in want]
            assert flat.tobytes() == b"".join(M.nt6(s) for _, s in want)
            assert declined_at is None and st["rest"] == want_rest and st["host_batches"] == 0
            assert st["batches"] == len(chunks)
            stats.append({x: v for x, v in st.items() if x not in ("parse_ms", "inflate_ms")})
        assert stats[0] == stats[1] == stats[2]


def test_load_reference_whatever_the_chunks(text):
    data, blob, pieces = text["fasta"]
    want = want_of(data)
    for batch in (WHOLE, ONE_MEMBER):
        stats = []
        for k in CHUNKINGS:
            names, seqs, declined, st = refdev.load_reference(blob, batch, bgzf=True, chunks_per_batch=k)
            assert declined is None and list(zip(names, seqs)) == want, (batch, k)
            assert st["batches"] == len(FC.chunks_of(data, batch, pieces)) and st["text_bytes"] == len(data)
            stats.append({x: v for x, v in st.items() if x not in ("parse_ms", "inflate_ms")})
        assert stats[0] == stats[1] == stats[2]


# ------------------------------------------------------------------ the input index: the file position carried across chunks
def sorted_records():
    """a small coordinate-sorted file's records over bam_input_index_lib.REFS (c3 without any): alignments that cross
    16 kb windows, secondary / unmapped-but-placed ones, 10 records without a reference last"""
    rng = np.random.default_rng(95)
    recs = []
    for tid, n, span in ((0, 90, 290000), (1, 40, 85000), (2, 12, 19000)):
        for pos in sorted(int(p) for p in rng.integers(0, span, size=n)):
            k, l = len(recs), int(rng.integers(150, 900))
            cigar = [("M", l)] if k % 3 else [("S", 10), ("M", l - 60), ("N", 20000), ("M", 50)]
            flag = [0, 16, 256, 4, 0][k % 5]
            recs.append(bam_writer.record(f"r{k:03d}", flag, tid, pos, 60 if k % 4 else 0, [] if flag == 4 else cigar, L._seq(rng, l), [("HP", "C", k % 3)],
                                          bytes(rng.integers(1, 60, size=l).astype(np.uint8))))
    for k in range(10):
        recs.append(bam_writer.record(f"nowhere{k}", 4, -1, -1, 0, [], L._seq(rng, 300), [], bytes(rng.integers(1, 60, size=300).astype(np.uint8))))
    return recs


def test_input_index_whatever_the_chunks():
    data, _ = members_of(L.header() + b"".join(sorted_records()), head=len(L.header()))
    assert len(data) < 400 << 10
    got = {(batch, k): bamdev.index_bam(data, batch_bytes=batch, chunks_per_batch=k) for batch in (WHOLE, ONE_MEMBER) for k in CHUNKINGS}
    first = got[WHOLE, 1]
    for key, idx in got.items():
        assert idx == first, key
    # ... and they are the index the test writer builds of the file (as bam_input_index_lib.check_input_index compares them)
    ix, want, norm = parse_index(first), parse_index(bam_writer.bai(data) + struct.pack("<Q", 0)), normaliser(data)
    assert ix["n_no_coor"] == 10 and len(ix["refs"]) == len(L.REFS) == len(want["refs"])
    for g, w in zip(ix["refs"], want["refs"]):
        gb = {b: [(norm(a), norm(z)) for a, z in ch] for b, (_, ch) in g["bins"].items() if b != meta_bin(5)}
        assert gb == {b: [(norm(a), norm(z)) for a, z in ch] for b, (_, ch) in w["bins"].items()}
        assert [norm(v) for v in g["linear"]] == [norm(v) for v in w["linear"]]


# ------------------------------------------------------------------ damage
def damaged(blob, how):
    """`blob` with one member of its second half damaged: how = 'flip' (a bit inside its deflate stream) or 'crc' (its
    footer's CRC32 xor 1); the member is the one with the longest stream, so the flipped bit is well inside it"""
    blocks = bgzf.bgzf_blocks(blob)
    at = max(range(len(blocks) // 2 + 1, len(blocks)), key=lambda i: blocks[i][1])
    coff, clen, isize, crc = blocks[at]
    assert isize > 0 and clen > 64
    bad = bytearray(blob)
    if how == "flip":
        bad[coff + clen // 2] ^= 0x10
    else:
        bad[coff + clen:coff + clen + 4] = struct.pack("<I", crc ^ 1)
    return bytes(bad), at


@pytest.mark.parametrize("k", [1, 2], ids=["one_chunk", "second_of_two_chunks"])
@pytest.mark.parametrize("how", ["flip", "crc"])
def test_damage_is_reported_in_the_same_words(bam, text, how, k):
    def says(e):
        assert e.value.code == 3                                 # SVDSS_EIO
        assert e.value.detail in MESSAGES if how == "flip" else e.value.detail == "BGZF block CRC mismatch", e.value.detail

    bad, at = damaged(bam["data"], how)
    assert k == 1 or at >= len(bgzf.bgzf_blocks(bad)) // 2      # (BatchArgs.split: the second chunk begins there)
    with pytest.raises(SvdssError) as e:
        bamdev.search_bam(bam["ix"], bad, batch_bytes=WHOLE, chunks_per_batch=k)
    says(e)
    with pytest.raises(SvdssError) as e:
        bamdev.select_bam(bad, batch_bytes=WHOLE, chunks_per_batch=k)
    says(e)
    bad, _ = damaged(text["fastq"][1], how)
    with pytest.raises(SvdssError) as e:
        fastxdev.parse_fastx(bad, WHOLE, bgzf=True, carry_cap=1 << 20, chunks_per_batch=k)
    says(e)
    bad, _ = damaged(text["fasta"][1], how)
    with pytest.raises(SvdssError) as e:
        refdev.load_reference(bad, WHOLE, bgzf=True, chunks_per_batch=k)
    says(e)
    assert e.value.reason == 8                                   # SVDSS_REF_IO


# ------------------------------------------------------------------ a failed batch gives up its turn
def three_batches(blob):
    """the members of `blob` as three batches, one member of the second one with a wrong CRC in its footer"""
    bad, at = damaged(blob, "crc")
    blocks = bgzf.bgzf_blocks(bad)
    return bad, [blocks[:at - 1], blocks[at - 1:at + 1], blocks[at + 1:]]


def in_a_thread(work):
    """runs work(codes) in a daemon thread: a turn that was not passed on is a failed test, not a stuck run"""
    codes = []
    t = threading.Thread(target=work, args=(codes,), daemon=True)
    t.start()
    t.join(timeout=20)
    assert not t.is_alive(), f"a batch is still waiting for its turn (codes so far: {codes})"
    return codes


def test_a_failed_bam_batch_gives_up_its_turn(bam):
    bad, groups = three_batches(bam["data"])
    n_ref, skip = bamdev.bam_header(bad, bgzf.bgzf_blocks(bad))
    comp = np.frombuffer(bad, dtype=np.uint8)

    def work(codes):
        flt = bamdev.BamFilter(n_ref)
        stream, batch = C.c_void_p(), C.c_void_p()
        lib.svdss_bam_stream_create(n_ref, C.byref(stream))
        try:
            for seq, g in enumerate(groups):
                A = bgzf.BatchArgs.whole(comp, g)
                rc = lib.svdss_bam_select_run(stream, seq, 1 if seq == 2 else 0, skip if seq == 0 else 0, flt._h, *A.args, C.byref(batch))
                codes.append((rc, (lib.svdss_bam_batch_error(batch) or b"").decode(), lib.svdss_bam_stream_error(stream).decode()))
        finally:
            if batch:
                lib.svdss_bam_batch_free(batch)
            lib.svdss_bam_stream_free(stream)
            flt.close()

    assert in_a_thread(work) == [(0, "", ""), (3, MESSAGES[1], MESSAGES[1]), (3, MESSAGES[1], MESSAGES[1])]


def test_a_failed_fastx_batch_gives_up_its_turn(text):
    bad, groups = three_batches(text["fastq"][1])
    comp = np.frombuffer(bad, dtype=np.uint8)

    def work(codes):
        stream, batch = C.c_void_p(), C.c_void_p()
        lib.svdss_fastx_stream_create(0, 1 << 20, C.byref(stream))
        try:
            for seq, g in enumerate(groups):
                A = bgzf.BatchArgs.whole(comp, g)
                rc = lib.svdss_fastx_batch_run(stream, seq, 1 if seq == 2 else 0, None, *A.args, None, 0, 0, C.byref(batch))
                codes.append((rc, (lib.svdss_fastx_batch_error(batch) or b"").decode(), lib.svdss_fastx_stream_error(stream).decode()))
        finally:
            if batch:
                lib.svdss_fastx_batch_free(batch)
            lib.svdss_fastx_stream_free(stream)

    assert in_a_thread(work) == [(0, "", ""), (3, MESSAGES[1], MESSAGES[1]), (3, MESSAGES[1], MESSAGES[1])]
