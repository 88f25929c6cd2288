"""The index as its rank blocks alone (svdss_index_load_blocks / svdss_index_attach_blocks: what `SVDSS search` makes
resident for a smoothed BAM), on the host: the handle against the full one it was written from, the kernel's lane code
on it (no text, no suffix array: MULTI table entries of size 1..4, unique intervals walked by rank steps) against the
oracle and the golden vectors, and the reader of the "SVDSSBK1" section on damaged files -- in the stand-alone harness
built with AddressSanitizer / UndefinedBehaviorSanitizer (tests/host_io_harness.cpp, mode `blocks`) and through the
library.  None of this needs a GPU; tests/test_sfs_rank_only_gpu.py repeats the comparisons through the real kernel."""
import os
import struct

import numpy as np
import pytest

import svdss_amd
from svdss_amd import synth
from svdss_amd._lib import SvdssError
from tests import emulator_lib as E
from tests import oracle_lib as O
from tests import rank_only_cases as R
from tests.common import from_ascii, load_golden, small_workload, split
from tests.test_host_io_robustness import harness, run  # noqa: F401  (the sanitized stand-alone reader, built once)

HEADER = 88          # RecHeader of csrc/index_build.cpp: magic, n, acc[7], total, n_contigs, reserved


def _references():
    rng = np.random.default_rng(21)
    return {"workload": small_workload()[0],
            "one_base": [np.array([3], np.uint8)],
            "300_contigs": [rng.integers(1, 5, size=int(rng.integers(5, 41))).astype(np.uint8) for _ in range(300)]}


def _patterns(rng, ref, n=200):
    """substrings of either strand (some with an N put in, some with the '$' in front of a record's first bases), random
    words that do not occur, N alone and in runs"""
    pats = []
    for i in range(n):
        c = ref[int(rng.integers(0, len(ref)))]
        kind = i % 5
        if kind == 4:
            p = rng.integers(1, 5, size=int(rng.integers(1, 40))).astype(np.uint8)        # (long ones do not occur)
        else:
            ln = int(rng.integers(1, min(len(c), 30) + 1))
            a = int(rng.integers(0, len(c) - ln + 1))
            p = c[a:a + ln].copy()
            if kind == 1:
                p = synth.revcomp(p)
            elif kind == 2:
                p[int(rng.integers(0, ln))] = 5
            elif kind == 3:
                p = np.concatenate([[0], c[:ln]]).astype(np.uint8)                      # '$' + the start of a record
        pats.append(np.ascontiguousarray(p, np.uint8))
    pats += [np.array([0, s], np.uint8) for s in (1, 2, 3, 4, 5)]                         # the records by their first symbol
    pats += [np.array([5], np.uint8), np.full(3, 5, np.uint8), np.array([0], np.uint8)]
    return pats


@pytest.mark.parametrize("route", [True, False])
@pytest.mark.parametrize("name", ["workload", "one_base", "300_contigs"])
def test_round_trip_against_the_full_handle(name, route, tmp_path):
    ref = _references()[name]
    full = svdss_amd.FMDIndex.build(ref, threads=2)
    ro, k = R.rank_only(ref, full=full, route=route, path=str(tmp_path / "ix.svdss"))
    assert ro.size == full.size == 2 * (sum(len(c) for c in ref) + len(ref))
    assert (ro.acc == full.acc).all()
    assert (ro.bwt() == full.bwt()).all()
    pats = _patterns(np.random.default_rng(22), ref)
    want = [full.count(p) for p in pats]
    assert [ro.count(p) for p in pats] == want
    assert sum(w > 0 for w in want) > (20 if name != "one_base" else 2) and sum(w == 0 for w in want) > 20
    if name == "300_contigs":
        assert full.acc[1] == 600 and sum(want[-8:-3]) == 600      # every '$' row is there: more than 256 of them
    assert R.records_code(ro) == R.ENODEV and ro.kmer_k == 0     # (no records; the table comes with residency)
    assert k == {"workload": 9, "one_base": 1, "300_contigs": 6}[name]


def test_what_a_rank_only_handle_refuses_on_the_host(tmp_path):
    """No text, no suffix array, no records: the full layout and the records cannot be written (an error, not a file
    with a header and nothing behind it); the .fmd can, from the blocks, and is the full handle's."""
    ref = _references()["300_contigs"]
    full = svdss_amd.FMDIndex.build(ref, threads=2)
    ro, _ = R.rank_only(ref, full=full, path=str(tmp_path / "ix.svdss"))
    assert _code(ro.save, str(tmp_path / "a.svdss")) == R.ENODEV and not os.path.exists(tmp_path / "a.svdss")
    assert _code(ro.save_records, str(tmp_path / "b.svdss")) == R.ENODEV and not os.path.exists(tmp_path / "b.svdss")
    ro.save_fmd(str(tmp_path / "ro.fmd"))
    full.save_fmd(str(tmp_path / "full.fmd"))
    assert (tmp_path / "ro.fmd").read_bytes() == (tmp_path / "full.fmd").read_bytes()
    # its blocks can be appended to a records file again, and read back
    full.save_records(str(tmp_path / "again.svdss"))
    ro.append_blocks(str(tmp_path / "again.svdss"))
    assert (tmp_path / "again.svdss").read_bytes() == (tmp_path / "ix.svdss").read_bytes()


# ---- the kernel's lane code on the loaded handle

RO_K = (0, 5, 8)


def _same(got, c, q, l, e, what):
    assert (got[0] == c).all() and (got[3] == e).all(), what
    assert (got[1] == q).all() and (got[2] == l).all(), what


@pytest.mark.parametrize("wide", [False, True])
def test_lane_code_on_random_reads(wide, monkeypatch):
    """The reads of test_lane_logic.py::test_v2_random_reads_match_oracle (a short first read, an all-N read, an empty
    one, a 1-mer, N in a long one) on a handle that has no text at all, 32- and 64-bit intervals."""
    ref, hap, svs, flat, offs = small_workload(seed=33, n_reads=40, read_len=1500)
    reads = [flat[offs[i]:offs[i + 1]] for i in range(40)]
    reads = [ref[0][3:40].copy()] + reads + [np.full(70, 5, np.uint8), np.zeros(0, np.uint8), ref[1][:1].copy(),
                                              ref[0][0:900].copy(), hap[0][:700].copy()]
    reads[-2][450] = 5
    flat, offs = svdss_amd.pack_reads(reads)
    full = svdss_amd.FMDIndex.build(ref, threads=4)
    if wide:
        monkeypatch.setenv("SVDSS_FORCE_SA64", "1")
    ro, _ = R.rank_only(ref, full=full)
    fm = O.OracleFMD.build(ref)
    for assemble in (False, True):
        c, q, l, e = fm.search_batch(flat, offs, assemble)
        for K in RO_K:
            for n_seg in (1, 4):
                got = E.search2(ro, flat, offs, assemble, K, False, n_seg=n_seg)
                _same(got, c, q, l, e, (assemble, K, n_seg))
                ops = got[4]
                assert ops["TEXT"] == ops["SA"] == ops["SET"] == ops["SA_SET"] == ops["BS_SA"] == 0 and ops["LF"] > 0
                assert (ops["TABLE"] > 0) == (K > 0)
                if n_seg == 4:
                    assert ops["stitched"] > 30
    assert c.sum() > 40


def test_lane_code_on_the_golden_vectors():
    for case in load_golden():
        contigs = [from_ascii(c) for c in case["contigs"]]
        ro, _ = R.rank_only(contigs)
        reads = [from_ascii(r["read"]) for r in case["reads"]]
        flat, offs = svdss_amd.pack_reads(reads)
        for K in RO_K:
            for n_seg in (1, 4):
                c, q, l, e, ops = E.search2(ro, flat, offs, False, K, False, n_seg=n_seg)
                for got, rd, ne in zip(split(c, q, l), case["reads"], e.tolist()):
                    assert [list(x) for x in got] == rd["sfs"], (case["name"], K, n_seg)
                    assert ne == rd["n_ext"], (case["name"], K, n_seg)
                c, q, l, e, ops = E.search2(ro, flat, offs, True, K, False, n_seg=n_seg)
                for got, rd in zip(split(c, q, l), case["reads"]):
                    assert [list(x) for x in got] == rd["assembled"], (case["name"], K, n_seg)


# ---- damaged sidecars: the reader of the "SVDSSBK1" section

def _code(fn, *a):
    try:
        fn(*a)
    except SvdssError as e:
        return e.code
    return 0


@pytest.fixture(scope="module")
def sidecar(tmp_path_factory):
    """a good sidecar (records + blocks) and where its parts are"""
    ref = synth.make_reference([9000, 2000], seed=6, n_runs=(30,))
    full = svdss_amd.FMDIndex.build(ref, threads=2)
    path = str(tmp_path_factory.mktemp("blocks") / "good.svdss")
    full.save_records(path)
    records = open(path, "rb").read()
    full.append_blocks(path)
    good = open(path, "rb").read()
    n = full.size
    sec = len(records)
    assert sec == HEADER + 8 * 2 + 11000 and good[sec:sec + 8] == b"SVDSSBK1"
    nb, nd = struct.unpack_from("<qq", good, sec + 8)
    assert nb == n // 128 + 1 and nd == 4 and len(good) == sec + 24 + 64 * nb + 8 * nd
    return {"ref": ref, "full": full, "good": good, "records": records, "n": n, "sec": sec, "nb": nb, "nd": nd,
            "rows": sec + 24 + 64 * nb}


def _damaged(s):
    """(name, bytes, expected code) -- 0: loads"""
    good, sec, nb, nd, n, rows = s["good"], s["sec"], s["nb"], s["nd"], s["n"], s["rows"]
    out = [("no_section", s["records"], R.EINVAL),
           ("magic", good[:sec] + b"SVDSSBK2" + good[sec + 8:], R.EINVAL)]
    sec_len = len(good) - sec
    for i in range(1, 16):          # (cut at 0/16 is the file without the section, above)
        out.append((f"cut_{i}_16", good[:sec + sec_len * i // 16], R.EIO))
    out.append(("cut_last_byte", good[:-1], R.EIO))

    def patched(at, fmt, *v):
        d = bytearray(good)
        struct.pack_into(fmt, d, at, *v)
        return bytes(d)
    out += [("n_blocks_minus", patched(sec + 8, "<q", nb - 1), R.EIO),
            ("n_blocks_plus", patched(sec + 8, "<q", nb + 1), R.EIO),
            ("n_dollar_negative", patched(sec + 16, "<q", -1), R.EIO),
            ("n_dollar_min", patched(sec + 16, "<q", -2 ** 63), R.EIO),
            ("n_dollar_above_n", patched(sec + 16, "<q", n + 1), R.EIO),
            ("n_dollar_huge", patched(sec + 16, "<q", 2 ** 62), R.EIO),
            ("n_dollar_past_the_file", patched(sec + 16, "<q", nd + 1), R.EIO),
            ("n_dollar_past_the_file_n", patched(sec + 16, "<q", n), R.EIO)]
    r = list(struct.unpack_from(f"<{nd}q", good, rows))
    assert all(0 <= x < n for x in r) and all(a < b for a, b in zip(r, r[1:]))
    out += [("row_is_n", patched(rows + 8 * (nd - 1), "<q", n), R.EIO),
            ("row_negative", patched(rows, "<q", -1), R.EIO),
            ("row_equal", patched(rows + 16, "<q", r[1]), R.EIO),
            ("row_descending", patched(rows + 8, "<qq", r[2], r[1]), R.EIO),
            ("header_n", patched(8, "<q", n + 2), R.EIO),
            ("header_total", patched(72, "<q", 11001), R.EIO),
            ("header_n_contigs", patched(80, "<i", 3), R.EIO),
            ("header_n_contigs_zero", patched(80, "<i", 0), R.EIO),
            ("header_n_negative", patched(8, "<q", -n), R.EIO),
            ("section_twice", good + good[sec:], 0),
            ("good", good, 0)]
    return out


def test_damaged_sections_in_the_sanitized_reader(harness, sidecar, tmp_path):  # noqa: F811
    """Every damaged file through the stand-alone reader (its own process, nothing preloaded): exit 0 (it loads, and the
    BWT decodes from the loaded blocks) or 1 (refused, with the code), never a sanitizer's exit."""
    path = str(tmp_path / "x.svdss")
    for name, data, code in _damaged(sidecar):
        open(path, "wb").write(data)
        rc, out = run(harness, "blocks", path)
        assert rc == (0 if code == 0 else 1), (name, out)
        if code:
            assert f"error: blocks {code}\n" in out, (name, out)
        else:
            assert f"blocks: {sidecar['n']} symbols, 4 '$' rows" in out, (name, out)
    # bytes changed anywhere in the section: loads or is refused
    rng = np.random.default_rng(9)
    good = sidecar["good"]
    for k in range(40):
        d = bytearray(good)
        at = int(rng.integers(sidecar["sec"] + 8, sidecar["sec"] + 24)) if k % 2 else int(rng.integers(sidecar["rows"], len(d)))
        d[at] = int(rng.integers(0, 256))
        open(path, "wb").write(bytes(d))
        run(harness, "blocks", path)


def test_damaged_sections_through_the_library(sidecar, tmp_path):
    """The same files through FMDIndex.load_blocks: the code it raises, and what loads is the full handle's index."""
    path = str(tmp_path / "x.svdss")
    want = sidecar["full"].bwt()
    for name, data, code in _damaged(sidecar):
        open(path, "wb").write(data)
        if code:
            assert _code(svdss_amd.FMDIndex.load_blocks, path) == code, name
            continue
        ro = svdss_amd.FMDIndex.load_blocks(path)
        assert ro.size == sidecar["n"] and (ro.bwt() == want).all(), name
        for s in (1, 2, 3, 4, 5):                       # ('$' ranks: every row of the list is there)
            p = np.array([0, s], np.uint8)
            assert ro.count(p) == sidecar["full"].count(p), name
    assert _code(svdss_amd.FMDIndex.load_blocks, str(tmp_path / "missing.svdss")) == R.EIO


def test_sidecar_of_an_fmd_is_trusted_only_when_it_is_current(sidecar, tmp_path, monkeypatch):
    """load_blocks / attach_blocks of an .fmd read `<fmd>.svdss`: not one older than the .fmd, not under
    SVDSS_INDEX_NO_CACHE; and blocks are attached only to the handle of the same index."""
    monkeypatch.delenv("SVDSS_INDEX_NO_CACHE", raising=False)
    full = sidecar["full"]
    fmd = str(tmp_path / "i.fmd")
    full.save_fmd(fmd)
    assert _code(svdss_amd.FMDIndex.load_blocks, fmd) == R.EINVAL          # no sidecar at all
    open(fmd + ".svdss", "wb").write(sidecar["good"])
    t = os.stat(fmd).st_mtime
    os.utime(fmd + ".svdss", (t + 5, t + 5))
    ro = svdss_amd.FMDIndex.load_blocks(fmd)
    assert (ro.bwt() == full.bwt()).all()
    os.utime(fmd + ".svdss", (t - 5, t - 5))
    assert _code(svdss_amd.FMDIndex.load_blocks, fmd) == R.EINVAL          # older than the .fmd
    os.utime(fmd + ".svdss", (t + 5, t + 5))
    monkeypatch.setenv("SVDSS_INDEX_NO_CACHE", "1")
    assert _code(svdss_amd.FMDIndex.load_blocks, fmd) == R.EINVAL
    lazy = svdss_amd.FMDIndex.load(fmd + ".svdss")                          # (the records file itself: no cache involved)
    assert _code(lazy.attach_blocks, fmd) == R.EINVAL
    monkeypatch.delenv("SVDSS_INDEX_NO_CACHE")
    assert lazy.attach_blocks(fmd).size == full.size and R.records_code(lazy) == R.ENODEV
    # another index's blocks: same length, other symbol counts (what the check compares: n and acc -- A <-> C, G <-> T
    # changes them on both strands, a swap with the complement would not)
    other_ref = [c.copy() for c in sidecar["ref"]]
    other_ref[0][100] = {1: 2, 2: 1, 3: 4, 4: 3, 5: 1}[int(other_ref[0][100])]
    other = str(tmp_path / "other.svdss")
    R.write_sidecar(svdss_amd.FMDIndex.build(other_ref, threads=2), other)
    mine = svdss_amd.FMDIndex.load(fmd + ".svdss")
    assert _code(mine.attach_blocks, other) == R.EINVAL
    assert R.records_code(mine) == 0                                        # refused: the handle keeps its records
    shorter = str(tmp_path / "shorter.svdss")
    R.write_sidecar(svdss_amd.FMDIndex.build([sidecar["ref"][0]], threads=2), shorter)
    assert _code(mine.attach_blocks, shorter) == R.EINVAL
    assert (mine.bwt() == full.bwt()).all()
