"""What the tests of --region / --regions-file share: the Python statement of the option's meaning (the records of a BAM
that are IN for a list of intervals), the subset BAM a region run must be indistinguishable from, and the parser shim."""
import os
import struct
import subprocess
import zlib

from tests import bam_writer
from tests.common import ROOT

PARSE_SRC = os.path.join(ROOT, "tests", "native", "region_parse.cpp")
PARSE_EXE = os.path.join(ROOT, "tests", "native", "_region_parse")
REF_SPAN_OPS = (0, 2, 3, 7, 8)    # M D N = X


def parse_exe():
    hdr = os.path.join(ROOT, "svdss_amd", "csrc", "bam_regions.h")
    if not os.path.exists(PARSE_EXE) or os.path.getmtime(PARSE_EXE) < max(os.path.getmtime(PARSE_SRC), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", PARSE_EXE, PARSE_SRC], check=True)
    return PARSE_EXE


def inflate(data):
    raw, pos = bytearray(), 0
    while pos + 18 <= len(data):
        bsize = struct.unpack_from("<H", data, pos + 16)[0] + 1
        raw += zlib.decompress(data[pos + 18:pos + bsize - 8], -15)
        pos += bsize
    assert pos == len(data)
    return bytes(raw)


def split(raw):
    """(header bytes, [(record bytes with block_size, tid, pos, endpos)]) of an inflated BAM stream; endpos = pos + the
    reference length of the CIGAR, pos + 1 where that is 0 (bam_endpos)"""
    l_text = struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, 8 + l_text)[0]
    p = 12 + l_text
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    head, recs = raw[:p], []
    while p + 4 <= len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        tid, pos = struct.unpack_from("<ii", raw, p + 4)
        l_name = raw[p + 12]
        n_cig = struct.unpack_from("<H", raw, p + 16)[0]
        span = sum(c >> 4 for c in struct.unpack_from(f"<{n_cig}I", raw, p + 36 + l_name) if (c & 15) in REF_SPAN_OPS)
        recs.append((raw[p:p + 4 + bs], tid, pos, pos + max(span, 1)))
        p += 4 + bs
    assert p == len(raw)
    return head, recs


def is_in(tid, pos, endpos, intervals):
    """the definition: tid >= 0 and [pos, endpos) overlaps an interval (tid, beg, end) of its reference"""
    return tid >= 0 and any(t == tid and pos < e and endpos > b for t, b, e in intervals)


def subset_bam(data, intervals, block=60000):
    """the BAM with the same header that holds exactly the records of `data` that are in, in file order, each once;
    also (records in, records in all)"""
    head, recs = split(inflate(data))
    keep = [r for r, tid, pos, end in recs if is_in(tid, pos, end, intervals)]
    return bam_writer.bgzf(head + b"".join(keep), block), len(keep), len(recs)


def merged(intervals):
    out = []
    for t, b, e in sorted(intervals):
        if e <= b:
            continue
        if out and out[-1][0] == t and b <= out[-1][2]:
            out[-1] = (t, out[-1][1], max(out[-1][2], e))
        else:
            out.append((t, b, e))
    return out
