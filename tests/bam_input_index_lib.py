"""What tests/test_bam_input_index.py (CPU) and tests/test_bam_input_index_gpu.py share: the BAM files whose index `SVDSS
bamindex` / `--write-bam-index` / `bamdev.index_bam` build, and the checks of an index of an INPUT BAM -- against the test
writer's own BAI / CSI (tests/bam_writer.py), against the file's own counts, and by region queries through the product's
reader (tests/native/bai_scan.cpp over csrc/bai_index.h)."""
import os
import struct
import subprocess

import numpy as np

from svdss_amd import synth
from tests import bam_writer
from tests.common import BIN
from tests.test_smooth_index import fixture_records, members, meta_bin, normaliser, parse_index

REFS = [("c0", 300000), ("c1", 90000), ("c2", 20000), ("c3", 50000)]     # c3: a reference with no record
WIN = 16384
KNOBS = ("SVDSS_BAM_DEVICE", "SVDSS_BAM_BATCH_MB", "SVDSS_BAM_SLAB_KB", "SVDSS_GPUS_OVERSUBSCRIBE", "SVDSS_REGION_MIN_KB", "SVDSS_REGION_TEST",
         "SVDSS_REGION_SHARDS", "SVDSS_REGION_INDEX", "SVDSS_CALL_STORE", "SVDSS_CALL_PASS2", "SVDSS_CALL_NO_BAI", "SVDSS_BAM_HEADROOM_MB",
         "SVDSS_BAM_SEG_KB")


def env0(**more):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(more)
    return e


def _seq(rng, n):
    return synth.to_ascii(rng.integers(1, 5, size=n).astype(np.uint8))


def _key(rec):
    tid, pos = struct.unpack_from("<ii", rec, 4)
    return (tid if tid >= 0 else 1 << 30, pos)


def header(refs=REFS):
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs)
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for n, l in refs:
        hdr += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return hdr


def extended_records():
    """test_smooth_index.fixture_records (secondary, supplementary and low-mapq records among them) and what an index of
    the input can go wrong on, sorted by coordinate, 40 records without a reference last."""
    from tests.test_region_gate_gpu import _with_cg_tag
    _, recs = fixture_records()
    rng = np.random.default_rng(77)
    more = []

    def add(name, tid, pos, cigar, l_seq, flag=0, mapq=60):
        more.append(bam_writer.record(name, flag, tid, pos, mapq, cigar, _seq(rng, l_seq), [], bytes(rng.integers(1, 60, size=l_seq).astype(np.uint8))))

    add("mapq0", 0, 1234, [("M", 300)], 300, mapq=0)
    add("secondary", 0, 1300, [("M", 300)], 300, flag=256)
    add("supplementary", 0, 1400, [("M", 300)], 300, flag=2048)
    for k in range(6):                                   # flag 4 and a position: indexed, counted as unmapped
        add(f"placed_unmapped{k}", k % 2, 5000 + 7000 * k, [], 150, flag=4 | (8 if k % 2 else 0), mapq=0)
    add("at_zero", 0, 0, [("M", 200)], 200)
    add("at_zero_c2", 2, 0, [("M", 100)], 100)
    add("ends_at_window", 0, 3 * WIN - 100, [("M", 100)], 100)             # [.., 3 WIN): window 2 alone
    add("ends_one_past_window", 0, 3 * WIN - 100, [("M", 101)], 101)       # one base into window 3
    add("ends_at_window_c1", 1, 2 * WIN - 250, [("S", 10), ("M", 250)], 260)
    add("five_windows", 0, 5 * WIN + 10, [("M", 100), ("N", 4 * WIN - 100), ("M", 100)], 200)   # windows 5 .. 9
    add("no_cigar", 0, 7 * WIN + 5, [], 120)
    add("no_cigar_c1", 1, 40000, [], 120, mapq=3)
    add("insertion_only", 0, 150000, [("S", 20), ("I", 100), ("S", 20)], 140)
    cg = bam_writer.record("cigar70k", 0, 0, 200000, 60, [("S", 35000), ("N", 70000)], _seq(rng, 35000), [("HP", "C", 1)],
                           bytes(rng.integers(1, 60, size=35000).astype(np.uint8)))
    more.append(_with_cg_tag(cg, [("M", 1), ("D", 1)] * 35000))
    out = sorted(recs + more, key=_key)                  # (stable: equal positions keep their order)
    for k in range(40):
        l = 200 + 3 * k
        out.append(bam_writer.record(f"nowhere{k:02d}", 4 | (64 if k % 2 else 128), -1, -1, 0, [], _seq(rng, l), [], bytes(rng.integers(1, 60, size=l).astype(np.uint8))))
    return out


def write_files(tmp):
    """{'b60000', 'b997', 'concat'}: the same records at blocks of 60,000, at blocks of 997 (records start and end on member
    boundaries) and as two concatenated parts, the second without a header, two empty members between them."""
    recs = extended_records()
    raw = header() + b"".join(recs)
    files = {}
    # blocks of 997, and a member boundary at the start of every 25th record: records start and end on member boundaries
    starts = np.cumsum([len(header())] + [len(r) for r in recs])
    cuts = sorted(set(range(0, len(raw), 997)) | {int(u) for u in starts[::25]} | {len(raw)})
    small = b"".join(bam_writer._bgzf_block(raw[a:b]) for a, b in zip(cuts, cuts[1:]) if b > a) + bam_writer._bgzf_block(b"")
    for tag, data in (("b60000", bam_writer.bgzf(raw, 60000)), ("b997", small)):
        files[tag] = tmp / f"{tag}.bam"
        files[tag].write_bytes(data)
    cut = len(raw) * 2 // 5 + 11                         # (inside a record)
    empty = bam_writer._bgzf_block(b"")
    files["concat"] = tmp / "concat.bam"
    files["concat"].write_bytes(bam_writer.bgzf(raw[:cut], 60000) + empty + bam_writer.bgzf(raw[cut:], 60000))
    return files


def long_record_file(tmp):
    """A file with a 1.3 MB record (650,000 bases with qualities and a long tag): at batches of 1 MB it straddles two of them
    and is larger than one; records that start in the batch it ends in follow."""
    rng = np.random.default_rng(5)
    recs = []

    def add(name, tid, pos, cigar, l_seq, tags=()):
        recs.append(bam_writer.record(name, 0, tid, pos, 60, cigar, _seq(rng, l_seq), list(tags), bytes(rng.integers(1, 60, size=l_seq).astype(np.uint8))))

    for k in range(60):
        add(f"a{k:03d}", 0, 100 + 997 * k, [("M", 9000)], 9000)
    noise = bytes(rng.integers(33, 127, size=325000).astype(np.uint8)).decode()
    add("long", 0, 70000, [("S", 640000), ("M", 10000)], 650000, [("ZZ", "Z", noise)])
    assert len(recs[-1]) > 1_290_000
    for k in range(80):
        add(f"b{k:03d}", 0 if k < 50 else 1, 70001 + 1500 * k if k < 50 else 300 + 900 * (k - 50), [("M", 8000)], 8000)
    p = tmp / "long.bam"
    p.write_bytes(bam_writer.bgzf(header() + b"".join(recs), 60000))
    return p


def records(data):
    """(name, tid, beg, end, flag, start, stop) of every record: end as the index sees it, start / stop in the inflated stream"""
    _, raw = members(data)
    l_text = struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, 8 + l_text)[0]
    p = 12 + l_text
    lens = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, p)[0]
        lens.append(struct.unpack_from("<i", raw, p + 4 + l_name)[0])
        p += 8 + l_name
    out = []
    while p + 4 <= len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        tid, pos = struct.unpack_from("<ii", raw, p + 4)
        l_name = raw[p + 12]
        n_cig, flag = struct.unpack_from("<HH", raw, p + 16)
        span = sum(c >> 4 for c in struct.unpack_from(f"<{n_cig}I", raw, p + 36 + l_name) if (c & 15) in (0, 2, 3, 7, 8))
        out.append((raw[p + 36:p + 36 + l_name - 1].decode(), tid, pos, pos + max(span, 1), flag, p, p + 4 + bs))
        p += 4 + bs
    return out, lens


def bamindex(bam, out, *extra, env=None):
    return subprocess.run([BIN, "bamindex", "--bam", str(bam), "-o", str(out), *extra], capture_output=True, timeout=600, env=env)


def check_input_index(exe, bam_path, idx_path, n_queries=200, seed=0):
    """bins, chunks, linear index and loffset against tests/bam_writer.py after `normaliser`; pseudo-bins and n_no_coor against
    the file's own counts; n_queries random multi-region queries through tests/native/_bai_scan."""
    data = open(bam_path, "rb").read()
    idx = open(idx_path, "rb").read()
    norm = normaliser(data)
    recs, lens = records(data)
    got = parse_index(idx)
    depth = got["depth"]
    assert got["min_shift"] == 14
    assert got["n_no_coor"] == sum(1 for r in recs if r[1] < 0)
    want = parse_index(bam_writer.csi(data, 14, depth) if got["csi"] else bam_writer.bai(data) + struct.pack("<Q", 0))
    n_ref = len(lens)
    assert len(got["refs"]) == n_ref == len(want["refs"])
    mb = meta_bin(depth)
    for t in range(n_ref):
        g, w = got["refs"][t], want["refs"][t]
        mine = [r for r in recs if r[1] == t]
        gb = {b: (norm(lo) if got["csi"] else 0, [(norm(a), norm(z)) for a, z in ch]) for b, (lo, ch) in g["bins"].items() if b != mb}
        wb = {b: (norm(lo) if got["csi"] else 0, [(norm(a), norm(z)) for a, z in ch]) for b, (lo, ch) in w["bins"].items()}
        assert gb == wb, t
        if not mine:
            assert mb not in g["bins"] and g["linear"] == []
            continue
        # the pseudo-bin: first start, last end, mapped, unmapped
        lo, ch = g["bins"][mb]
        assert lo == 0 and len(ch) == 2
        assert (norm(ch[0][0]), norm(ch[0][1])) == (mine[0][5], mine[-1][6])
        n_unm = sum(1 for r in mine if r[4] & 4)
        assert ch[1] == (len(mine) - n_unm, n_unm), t
        if not got["csi"]:
            assert [norm(v) for v in g["linear"]] == [norm(v) for v in w["linear"]], t
    # queries: the records read through the index that overlap a region are exactly those a sequential read finds
    rng = np.random.default_rng(seed)
    placed = [r for r in recs if r[1] >= 0]
    last_end = {t: max([r[3] for r in placed if r[1] == t], default=0) for t in range(n_ref)}
    cases = [[(t, 0, lens[t])] for t in range(n_ref)] + [[(t, last_end[t] + 1, last_end[t] + 5000)] for t in range(n_ref)]
    cases += [[(0, 3 * WIN, 3 * WIN + 1)], [(0, 3 * WIN - 1, 3 * WIN)], [(0, 0, 1)], [(0, 9 * WIN, 9 * WIN + 5)], [(0, 269999, 270000)], [(0, 270000, 270001)]]
    for _ in range(n_queries):
        reg = []
        for _ in range(int(rng.integers(1, 4))):
            t = int(rng.integers(0, n_ref))
            b = int(rng.integers(0, max(1, min(lens[t], last_end[t] + 20000))))
            reg.append((t, b, b + int(rng.integers(1, 40000))))
        cases.append(sorted(reg))
    for regions in cases:
        r = subprocess.run([exe, str(bam_path), str(idx_path)] + [f"{t}:{b}-{e}" for t, b, e in regions], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = [tuple(l.split("\t")) for l in r.stdout.splitlines()]
        want_q = [(r_[0], str(r_[1]), str(r_[2])) for r_ in placed if any(r_[1] == rt and r_[2] < re and r_[3] > rb for rt, rb, re in regions)]
        assert [x for x in out if x in set(want_q)] == want_q, regions
        assert len(set(out)) == len(out), regions
    return recs
