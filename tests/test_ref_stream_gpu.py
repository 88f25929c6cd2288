"""The reference FASTA inflated and parsed on the GPU (svdss_amd/csrc/ref_stream.hip) at library level: names and
upper-cased sequences against tests.mirror.fastx.reader_records -- what FastxReader::next and load_chromosomes give -- over
the cases of tests/ref_cases.py (sizes around the tile of the kernels, plain slabs and BGZF members, batches down to one
member), member and batch cuts, the files the stream declines with their reasons, the resident svdss_ref_t of
svdss_ref_stream_finish against svdss_ref_upload_parts, and the seeded fuzz of the CPU suite."""
import ctypes as C

import numpy as np
import pytest

from svdss_amd import refdev
from svdss_amd._lib import SvdssError, lib
from tests import ref_cases as RC
from tests.mirror import fastx as M
from tests.mirror import refstream as R

pytestmark = pytest.mark.gpu
T = refdev.tile_bytes()
DELIVERED = RC.delivered_cases(T)
DECLINED = RC.declined_cases(T)


def want_of(data):
    return [(n, R.upper(s)) for n, s in M.reader_records(data)]


def load(data, batch, pieces=None, cap=None, eof=True):
    blob = M.bgzf_pack(pieces, eof=eof) if pieces is not None else data
    names, seqs, declined, st = refdev.load_reference(blob, batch, bgzf=pieces is not None, header_cap=cap)
    return list(zip(names, seqs)), declined, st


def test_tile():
    assert T >= 256 and T % 16 == 0


@pytest.mark.parametrize("case", DELIVERED, ids=[c[0] for c in DELIVERED])
def test_delivered(case):
    _, data, cap = case
    want = want_of(data)
    for _, batch, bgzf in RC.WAYS:
        pieces = RC.members(data) if bgzf else None
        got, declined, st = load(data, batch, pieces, cap)
        assert declined is None
        assert got == want
        assert st["batches"] == len(RC.chunks_of(data, batch, pieces)) and st["text_bytes"] == len(data)


def test_member_and_batch_cuts():
    data, cases = RC.cut_cases(T)
    want = want_of(data)
    for name, pieces, eof in cases:
        for batch in (1 << 20, 1):
            got, declined, _ = load(data, batch, pieces, eof=eof)
            assert declined is None and got == want, name
    # the same cuts as the slabs of a plain file
    for name, pieces, _ in cases:
        jobs, off = [], 0
        for p in pieces:
            jobs.append((off, len(p)))
            off += len(p)
        names, seqs, declined, _ = refdev.load_reference(data, 0, jobs=jobs)
        assert declined is None and list(zip(names, seqs)) == want, name


@pytest.mark.parametrize("case", DECLINED, ids=[c[0] for c in DECLINED])
def test_declined(case):
    _, data, cap, why = case
    for batch, bgzf in ((1 << 20, False), (1000, False), (1024, True)):
        got, declined, st = load(data, batch, RC.members(data) if bgzf else None, cap)
        assert declined == why and got == []
        if why in (R.CR, R.NUL, R.AT, R.NOT_FASTA):
            assert st["declined_at"] == R.run(RC.chunks_of(data, batch, None), cap or R.DEFAULT_HEADER_CAP)[1][1]


def test_damaged_member():
    data = RC.delivered_cases(T)[10][1]
    blob = bytearray(M.bgzf_pack(RC.members(data)))
    blob[len(blob) // 2] ^= 0x55                       # inside a member's deflate stream: its inflate fails or its CRC differs
    for batch in (1 << 20, 1):
        with pytest.raises(SvdssError) as e:
            refdev.load_reference(bytes(blob), batch, bgzf=True)
        assert e.value.code == 3                       # SVDSS_EIO
        assert e.value.reason == 8
        assert e.value.detail in ("BGZF block CRC mismatch", "BGZF inflate failed")


def test_finish_against_upload_parts():
    rng = np.random.default_rng(35)
    recs = [(b"k%d" % k, RC.seq_of(rng, n, RC.IUPAC)) for k, n in enumerate([T + 7, 0, 3 * T + 1, 61, 2 * T, 5])]
    data = RC.fasta(recs, wrap=60)
    seqs = [R.upper(s) for _, s in recs]
    for order in ([4, 0, 2], [5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5], [1], []):
        for batch, bgzf in ((1 << 20, False), (1000, False), (1024, True)):
            blob = M.bgzf_pack(RC.members(data)) if bgzf else data
            with refdev.resident(blob, batch, order=order, bgzf=bgzf) as got:
                bufs = [np.frombuffer(seqs[i] or b"\0", np.uint8) for i in order]
                lens = np.array([len(seqs[i]) for i in order], np.int64)
                ptrs = (C.c_void_p * max(1, len(order)))(*[b.ctypes.data for b in bufs])
                h = C.c_void_p()
                assert lib.svdss_ref_upload_parts(ptrs, lens.ctypes.data if len(order) else None, len(order), 0, C.byref(h)) == 0
                with refdev.ResidentRef(h, len(order)) as want:
                    w_off, w_seq = want.read()
                    g_off, g_seq = got.read()
                    assert list(g_off) == list(w_off) and g_seq == w_seq == b"".join(seqs[i] for i in order)


def test_fuzz_no_accepted_file_declines():
    rng = np.random.default_rng(4242)
    accepted = 0
    for _ in range(200):
        data, batch, pieces = RC.fuzz_file(rng)
        rng.integers(0, len(data) + 1, size=int(rng.integers(0, 9)))       # (the CPU suite's own cuts: the same files as there)
        why = R.declines(data)
        got, declined, _ = load(data, batch, pieces)
        if why is None:
            assert declined is None and got == want_of(data)
            accepted += 1
        else:
            assert declined is not None and got == []
    assert accepted >= 100
