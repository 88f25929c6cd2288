"""The byte ranges a region run reads (csrc/bam_region_ranges.h), on BAI and CSI files of tests/bam_writer.py -- the default
CSI layout and min_shift 10 / depth 3: every record a sequential Python read finds overlapping a region lies wholly inside a
range, at or behind its first record (`skip`); the ranges begin and end at BGZF members, are disjoint and ascending; a
region that names no chunk reads nothing."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_writer
from tests import region_lib as R
from tests.common import ROOT

SRC = os.path.join(ROOT, "tests", "native", "region_ranges.cpp")
EXE = os.path.join(ROOT, "tests", "native", "_region_ranges")
CSRC = os.path.join(ROOT, "svdss_amd", "csrc")


@pytest.fixture(scope="module")
def exe():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("bam_region_ranges.h", "bam_regions.h", "bai_index.h", "bam_reader.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", EXE, SRC, "-lz", "-ldl"], check=True)
    return EXE


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ranges")
    rng = np.random.default_rng(17)
    lens = [400000, 30000, 150000]
    recs = []
    for tid, n in ((0, 1300), (2, 500)):                       # (no record on the second reference)
        for k, st in enumerate(np.sort(rng.integers(0, lens[tid] - 3000, size=n))):
            l = int(rng.integers(150, 2500))
            cig = [("S", 5), ("M", l - 105), ("D", 40), ("M", 100)] if k % 3 == 0 else [("M", l)]
            recs.append(bam_writer.record(f"t{tid}r{k}", 0, tid, int(st), 60, cig, "".join("ACGT"[x] for x in rng.integers(0, 4, size=l)),
                                          qual=bytes(rng.integers(20, 60, size=l, dtype=np.uint8).tolist())))
    data = bam_writer.bgzf(R.inflate(bam_writer.bam([(f"c{t}", l) for t, l in enumerate(lens)], recs)), 4096)
    bam = tmp / "x.bam"
    bam.write_bytes(data)
    # every record: (tid, pos, endpos, file offset of the member it starts in, offset in that member, file offset behind the
    # member it ends in)
    members, pos, u = [], 0, 0
    while pos + 18 <= len(data):
        bsize = struct.unpack_from("<H", data, pos + 16)[0] + 1
        isize = struct.unpack_from("<I", data, pos + bsize - 4)[0]
        members.append((u, pos, bsize, isize))
        u += isize
        pos += bsize
    head, rs = R.split(R.inflate(data))
    where, at, m = [], len(head), 0
    for r, tid, p, e in rs:
        while members[m][0] + members[m][3] <= at:
            m += 1
        m2 = m
        while members[m2][0] + members[m2][3] < at + len(r):
            m2 += 1
        where.append((tid, p, e, members[m][1], at - members[m][0], members[m2][1] + members[m2][2]))
        at += len(r)
    idx = {"bai": tmp / "x.bam.bai", "csi": tmp / "x.csi", "csi_10_3": tmp / "x.10.3.csi"}
    idx["bai"].write_bytes(bam_writer.bai(data))
    idx["csi"].write_bytes(bam_writer.csi(data))
    idx["csi_10_3"].write_bytes(bam_writer.csi(data, 10, 3))
    return {"bam": bam, "size": len(data), "where": where, "idx": idx, "member_starts": {mm[1] for mm in members} | {len(data)}, "lens": lens}


def ranges(exe, fx, kind, regions):
    r = subprocess.run([exe, str(fx["bam"]), str(fx["idx"][kind])] + [f"{t}:{b}-{e}" for t, b, e in regions], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [tuple(int(x) for x in l.split("\t")) for l in r.stdout.splitlines()]


@pytest.mark.parametrize("kind", ["bai", "csi", "csi_10_3"])
def test_the_ranges_hold_every_overlapping_record_and_are_disjoint_and_ascending(exe, fx, kind):
    rng = np.random.default_rng(3)
    cases = [[(0, 0, 400000)], [(0, 100000, 100001)], [(0, 16384, 32768)], [(2, 149000, 150000)], [(0, 399999, 400000), (2, 0, 1)],
             [(0, 50000, 52000), (0, 51000, 70000), (2, 10000, 13000), (0, 300000, 300100)], [(0, 0, 2**31 - 1), (1, 0, 2**31 - 1), (2, 0, 2**31 - 1)]]
    for _ in range(25):
        k = int(rng.integers(1, 9))
        cases.append([(int(t), int(b), int(b) + int(w)) for t, b, w in
                      zip(rng.choice([0, 0, 2], size=k), rng.integers(0, 145000, size=k), rng.integers(1, 20000, size=k))])
    for regions in cases:
        got = ranges(exe, fx, kind, regions)
        assert all(b < e <= fx["size"] and 0 <= s < 65536 and b in fx["member_starts"] and e in fx["member_starts"] for b, e, s in got), regions
        assert all(x[1] < y[0] for x, y in zip(got, got[1:])), regions                         # disjoint (not even touching), ascending
        n_over = 0
        for tid, p, e, m_off, in_off, end_off in fx["where"]:
            if not R.is_in(tid, p, e, regions):
                continue
            n_over += 1
            hit = [(b, z, s) for b, z, s in got if b <= m_off and end_off <= z]
            assert len(hit) == 1, (regions, tid, p)
            b, z, s = hit[0]
            assert (m_off, in_off) >= (b, s), (regions, tid, p)                                 # not in front of the range's first record
        assert n_over > 0 or regions == [(0, 399999, 400000), (2, 0, 1)] or len(got) <= len(regions)
    # one base: one range, not the whole file (how much less depends on the bins: a record that crosses a boundary of a
    # large bin is filed there, and that bin's chunk runs from the first such record to the last)
    small = ranges(exe, fx, kind, [(0, 100000, 100001)])
    assert len(small) == 1 and small[0][0] > 0 and small[0][1] - small[0][0] < fx["size"] - 28
    # no chunk named: nothing read
    assert ranges(exe, fx, kind, [(1, 0, 30000)]) == []
    # the whole of every reference: one range, from the first record to the last
    whole = ranges(exe, fx, kind, [(0, 0, 2**31 - 1), (2, 0, 2**31 - 1)])
    assert len(whole) == 1 and whole[0][1] >= fx["size"] - 28 - 4200
