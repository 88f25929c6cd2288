"""`SVDSS smooth --write-index FILE` (csrc/bam_index_writer.h; on the device path the fragments come from
csrc/bam_smooth.hip): the index of the output BAM, held against the test writer's own BAI / CSI of the same bytes
(tests/bam_writer.py) after every virtual offset is turned into a position of the inflated stream, and against region
queries through the product's reader (csrc/bai_index.h) versus a sequential read."""
import bisect
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from svdss_amd import synth
from tests import bam_writer
from tests.common import BIN, ROOT
from tests.pipeline_sim import add_errors, simulate

SRC = os.path.join(ROOT, "tests", "native", "bai_scan.cpp")
EXE = os.path.join(ROOT, "tests", "native", "_bai_scan")
BLOCK = 0xff00


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(
            os.path.join(ROOT, "svdss_amd", "csrc", "bai_index.h")), os.path.getmtime(os.path.join(ROOT, "svdss_amd", "csrc", "bam_reader.h"))):
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", EXE, SRC, "-lz", "-ldl"], check=True)
    return EXE


# ---- reading what `smooth` wrote
def members(data):
    """(compressed offset, inflated offset, inflated size) of every BGZF member, and the inflated stream."""
    out, raw, pos = [], bytearray(), 0
    while pos + 18 <= len(data):
        bsize = struct.unpack_from("<H", data, pos + 16)[0] + 1
        blk = zlib.decompress(data[pos + 18:pos + bsize - 8], -15)
        out.append((pos, len(raw), len(blk)))
        raw += blk
        pos += bsize
    assert pos == len(data)
    return out, bytes(raw)


def normaliser(data):
    """virtual offset -> position in the inflated stream (either form of a block boundary gives the same position)"""
    blocks, _ = members(data)
    at = {c: u for c, u, n in blocks}
    size = {c: n for c, u, n in blocks}

    def norm(v):
        c, o = v >> 16, v & 0xffff
        assert c in at and o <= size[c], hex(v)
        return at[c] + o
    return norm


def records(data):
    """(name, tid, beg, end, start, stop) of every record: end as the index sees it, start / stop in the inflated stream"""
    _, raw = members(data)
    l_text = struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, 8 + l_text)[0]
    p = 12 + l_text
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    out = []
    while p + 4 <= len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        tid, pos = struct.unpack_from("<ii", raw, p + 4)
        l_name = raw[p + 12]
        n_cig = struct.unpack_from("<H", raw, p + 16)[0]
        span = sum(c >> 4 for c in struct.unpack_from(f"<{n_cig}I", raw, p + 36 + l_name) if (c & 15) in (0, 2, 3, 7, 8))
        out.append((raw[p + 36:p + 36 + l_name - 1].decode(), tid, pos, pos + max(span, 1), p, p + 4 + bs))
        p += 4 + bs
    return out


def parse_index(idx):
    """{'csi', 'min_shift', 'depth', 'refs': [{'bins': {bin: (loffset, [(v0, v1)])}, 'linear': [...]}], 'n_no_coor'}"""
    csi = idx[:2] == b"\x1f\x8b"
    if csi:
        _, idx = members(idx)
        assert idx[:4] == b"CSI\1"
        min_shift, depth, l_aux = struct.unpack_from("<iii", idx, 4)
        p = 16 + l_aux
    else:
        assert idx[:4] == b"BAI\1"
        min_shift, depth, p = 14, 5, 4
    n_ref = struct.unpack_from("<i", idx, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", idx, p)[0]
        p += 4
        bins = {}
        for _ in range(n_bin):
            b = struct.unpack_from("<I", idx, p)[0]
            p += 4
            lo = 0
            if csi:
                lo = struct.unpack_from("<Q", idx, p)[0]
                p += 8
            n = struct.unpack_from("<i", idx, p)[0]
            p += 4
            bins[b] = (lo, [struct.unpack_from("<QQ", idx, p + 16 * k) for k in range(n)])
            p += 16 * n
        lin = []
        if not csi:
            n = struct.unpack_from("<i", idx, p)[0]
            lin = list(struct.unpack_from(f"<{n}Q", idx, p + 4))
            p += 4 + 8 * n
        refs.append({"bins": bins, "linear": lin})
    n_no_coor = None
    if p + 8 <= len(idx):
        n_no_coor = struct.unpack_from("<Q", idx, p)[0]
        p += 8
    assert p == len(idx), (p, len(idx))
    return {"csi": csi, "min_shift": min_shift, "depth": depth, "refs": refs, "n_no_coor": n_no_coor}


def meta_bin(depth):
    return ((1 << (3 * depth + 3)) - 1) // 7 + 1


def check_index(exe, tmp_path, bam_path, idx_path, n_queries=200, seed=0):
    """The structure, linear index / loffsets, pseudo-bins and region queries of an index `smooth` wrote."""
    data = open(bam_path, "rb").read()
    idx = open(idx_path, "rb").read()
    norm = normaliser(data)
    recs = records(data)
    got = parse_index(idx)
    depth = got["depth"]
    assert got["n_no_coor"] == 0 and got["min_shift"] == 14
    want = parse_index(bam_writer.csi(data, 14, depth) if got["csi"] else bam_writer.bai(data) + struct.pack("<Q", 0))
    n_ref = len(want["refs"])
    assert len(got["refs"]) == n_ref
    mb = meta_bin(depth)
    for t in range(n_ref):
        g, w = got["refs"][t], want["refs"][t]
        mine = [r for r in recs if r[1] == t]
        # bins and chunks (and CSI loffsets), every offset normalised; the pseudo-bin apart
        gb = {b: (norm(lo) if got["csi"] else 0, [(norm(a), norm(z)) for a, z in ch]) for b, (lo, ch) in g["bins"].items() if b != mb}
        wb = {b: (norm(lo) if got["csi"] else 0, [(norm(a), norm(z)) for a, z in ch]) for b, (lo, ch) in w["bins"].items()}
        assert gb == wb, t
        if not mine:
            assert mb not in g["bins"] and g["linear"] == []
            continue
        # the pseudo-bin: first start, last end, mapped, unmapped
        lo, ch = g["bins"][mb]
        assert lo == 0 and len(ch) == 2
        assert (norm(ch[0][0]), norm(ch[0][1])) == (mine[0][4], mine[-1][5])
        assert ch[1] == (len(mine), 0)
        if not got["csi"]:
            lin = [norm(v) for v in g["linear"]]
            first = {}
            for name, tid, beg, end, a, z in mine:
                for win in range(beg >> 14, ((end - 1) >> 14) + 1):
                    first.setdefault(win, a)
            assert len(lin) == max(first) + 1
            assert all(x <= y for x, y in zip(lin, lin[1:]))
            covered = sorted(first)
            for win, v in enumerate(lin):
                if win in first:
                    assert v == first[win], (t, win)
                else:
                    assert v <= first[covered[bisect.bisect_left(covered, win)]], (t, win)
    # queries: the records read through the index that overlap a region are exactly those a sequential read finds
    rng = np.random.default_rng(seed)
    lens = {}
    _, raw = members(data)
    l_text = struct.unpack_from("<i", raw, 4)[0]
    p = 12 + l_text
    for t in range(n_ref):
        ln = struct.unpack_from("<i", raw, p)[0]
        lens[t] = struct.unpack_from("<i", raw, p + 4 + ln)[0]
        p += 8 + ln
    seq = subprocess.run([exe, str(bam_path), "-"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert seq == [f"{n}\t{t}\t{b}" for n, t, b, e, a, z in recs]
    last_end = {t: max([e for n, tt, b, e, a, z in recs if tt == t], default=0) for t in range(n_ref)}
    cases = [[(t, 0, lens[t])] for t in range(n_ref)] + [[(t, last_end[t] + 1, last_end[t] + 5000)] for t in range(n_ref)]
    for _ in range(n_queries):
        k = int(rng.integers(1, 4))
        reg = []
        for _ in range(k):
            t = int(rng.integers(0, n_ref))
            b = int(rng.integers(0, max(1, min(lens[t], last_end[t] + 20000))))
            reg.append((t, b, b + int(rng.integers(1, 40000))))
        cases.append(sorted(reg))
    for regions in cases:
        r = subprocess.run([exe, str(bam_path), str(idx_path)] + [f"{t}:{b}-{e}" for t, b, e in regions], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = [tuple(l.split("\t")) for l in r.stdout.splitlines()]
        want_q = [(n, str(t), str(b)) for n, t, b, e, a, z in recs if any(t == rt and b < re and e > rb for rt, rb, re in regions)]
        assert [x for x in out if x in set(want_q)] == want_q, regions
        assert len(set(out)) == len(out), regions
    return recs


# ---- the input
def bam_with_text(refs, recs, extra=""):
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs) + extra
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for n, l in refs:
        hdr += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return bam_writer.bgzf(hdr + b"".join(recs))


def fixture_records(seed=28, ref_lens=(300000, 90000, 20000)):
    """The records of test_smooth_gpu's device-versus-host fixture: XF tags of every kind already present, secondary,
    supplementary and low-MAPQ records, a CIGAR that does not add up (XF 3), reads on a contig the FASTA lacks."""
    ref, svs, reads = simulate(ref_lens=ref_lens, n_svs=12, coverage=10, read_len=7000, seed=seed)
    rng = np.random.default_rng(5)
    recs = []
    for k, (n, tid, pos, cig, seq, hp) in enumerate(reads):
        s2, c2 = add_errors(seq, cig, rng, 0.05 if k % 17 == 0 else 0.006)
        qual = bytes(rng.integers(1, 60, size=len(s2)).astype(np.uint8))
        tags = [("HP", "C", hp)] if hp else []
        if k % 5 == 1:
            tags.append(("XF", "C", 9))
        elif k % 5 == 2:
            tags = [("XF", "i", 70000)] + tags + [("ZZ", "Z", "after")]
        elif k % 5 == 3:
            tags.append(("XF", "Z", "text"))
        flag = 16 if k % 2 else 0
        if k % 23 == 0:
            flag |= 256
        if k % 29 == 0:
            flag |= 2048
        mapq = 5 if k % 31 == 0 else 60
        if k % 37 == 0:
            c2 = c2[:-1] + [(c2[-1][0], c2[-1][1] + 3)]
        recs.append(bam_writer.record(n, flag, tid, pos, mapq, c2, s2, tags, qual))
    return ref, recs


def write_fixture(tmp_path, extra_refs=(), extra_text=""):
    ref, recs = fixture_records()
    names = ["c0", "c1", "c2"]
    fa = tmp_path / "ref.fa"
    with open(fa, "w") as fh:
        for n, c in zip(names[:2], ref[:2]):          # (c2 is not in the FASTA: its records are dropped)
            fh.write(f">{n}\n{synth.to_ascii(c)}\n")
    refs = [(n, len(c)) for n, c in zip(names, ref)] + list(extra_refs)
    bam = tmp_path / "in.bam"
    bam.write_bytes(bam_with_text(refs, recs, extra_text))
    return fa, bam


def smooth(fa, bam, out, *extra, env=None, stdout=None):
    cmd = [BIN, "smooth", "--reference", str(fa), "--bam", str(bam), "--threads", "4", "--min-mapq", "20", *extra]
    if stdout is not None:
        return subprocess.run(cmd, stdout=stdout, stderr=subprocess.PIPE, timeout=900, env=env)
    with open(out, "wb") as fh:
        return subprocess.run(cmd, stdout=fh, stderr=subprocess.PIPE, timeout=900, env=env)


def padded_fixture(tmp_path):
    """The fixture with a @CO line sized so that a record of the output begins exactly at a multiple of 0xff00."""
    fa, bam = write_fixture(tmp_path)
    out = tmp_path / "probe.bam"
    r = smooth(fa, bam, out)
    assert r.returncode == 0, r.stderr.decode()
    recs = records(out.read_bytes())
    start = recs[len(recs) // 3][4]                  # where a record in the middle begins with no @CO line
    m = (start + 5) // BLOCK + 1
    pad = m * BLOCK - start                          # bytes of "@CO\t" + x... + "\n"
    return write_fixture(tmp_path, extra_text="@CO\t" + "x" * (pad - 5) + "\n")


def test_smooth_writes_its_bai_and_csi(tmp_path, exe):
    fa, bam = padded_fixture(tmp_path)
    out = tmp_path / "out.bam"
    r = smooth(fa, bam, out, "--write-index", str(tmp_path / "out.bam.bai"))
    assert r.returncode == 0, r.stderr.decode()
    assert not (tmp_path / "out.bam.bai.tmp").exists()
    recs = check_index(exe, tmp_path, out, tmp_path / "out.bam.bai")
    assert any(a % BLOCK == 0 for n, t, b, e, a, z in recs[1:]), "no record begins at a block boundary"
    assert len({t for n, t, b, e, a, z in recs}) == 2 and len(members(out.read_bytes())[0]) > 20
    # the same BAM bytes with a CSI beside them; with --write-index the BAM itself is what it is without
    r = smooth(fa, bam, tmp_path / "out2.bam", "--write-index", str(tmp_path / "out2.bam.csi"))
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "out2.bam").read_bytes() == out.read_bytes()
    assert parse_index((tmp_path / "out2.bam.csi").read_bytes())["depth"] == 5
    check_index(exe, tmp_path, tmp_path / "out2.bam", tmp_path / "out2.bam.csi", seed=1)
    # no option: the same bytes, no file beside them
    before = set(os.listdir(tmp_path))
    r = smooth(fa, bam, tmp_path / "plain.bam")
    assert r.returncode == 0 and (tmp_path / "plain.bam").read_bytes() == out.read_bytes()
    assert set(os.listdir(tmp_path)) - before == {"plain.bam"}
    # to a pipe: the same index
    with open(tmp_path / "piped.bam", "wb") as fh:
        p = subprocess.Popen([BIN, "smooth", "--reference", str(fa), "--bam", str(bam), "--threads", "4", "--write-index",
                              str(tmp_path / "piped.bai")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        c = subprocess.Popen(["cat"], stdin=p.stdout, stdout=fh)
        p.stdout.close()
        _, err = p.communicate(timeout=900)
        c.wait(timeout=60)
    assert p.returncode == 0, err.decode()
    assert (tmp_path / "piped.bam").read_bytes() == out.read_bytes()
    assert (tmp_path / "piped.bai").read_bytes() == (tmp_path / "out.bam.bai").read_bytes()


def test_a_reference_beyond_bai_needs_csi(tmp_path, exe):
    fa, bam = write_fixture(tmp_path, extra_refs=[("big", 600_000_000)])      # (not in the FASTA: no records on it)
    out = tmp_path / "out.bam"
    r = smooth(fa, bam, out, "--write-index", str(tmp_path / "out.bam.bai"))
    assert r.returncode != 0 and b".csi" in r.stderr
    assert out.read_bytes() == b""
    assert not (tmp_path / "out.bam.bai").exists() and not (tmp_path / "out.bam.bai.tmp").exists()
    r = smooth(fa, bam, out, "--write-index", str(tmp_path / "out.bam.csi"))
    assert r.returncode == 0, r.stderr.decode()
    got = parse_index((tmp_path / "out.bam.csi").read_bytes())
    assert got["depth"] == 6 and len(got["refs"]) == 4 and got["refs"][3]["bins"] == {}
    check_index(exe, tmp_path, out, tmp_path / "out.bam.csi", seed=2)


def test_a_failing_smooth_leaves_no_index_and_other_commands_refuse_the_option(tmp_path):
    fa, bam = write_fixture(tmp_path)
    data = bam.read_bytes()
    bad = tmp_path / "cut.bam"
    bad.write_bytes(data[:len(data) // 2])
    r = smooth(fa, bad, tmp_path / "out.bam", "--write-index", str(tmp_path / "out.bam.bai"))
    assert r.returncode != 0
    assert not (tmp_path / "out.bam.bai").exists() and not (tmp_path / "out.bam.bai.tmp").exists()
    r = subprocess.run([BIN, "call", "--reference", str(fa), "--bam", str(bam), "--sfs", "x", "--write-index", "y.bai"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--write-index" in r.stderr and "smooth" in r.stderr and not os.path.exists("y.bai")
    r = subprocess.run([BIN, "smooth", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--write-index" in r.stderr
