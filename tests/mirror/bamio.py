"""Minimal BAM reader for the Python mirrors of the host logic (test infrastructure) (BGZF = concatenated gzip members, so the
standard gzip module inflates it).  The C++ CLI uses csrc/bam_reader.h; this one also decodes
CIGAR and SEQ, which `call` needs."""
import gzip
import struct
from typing import List, Tuple

from .clusterer import Alignment
from .smoother import aux_value_size

SEQ16 = "=ACMGRSVTWYHKDBN"


def read_bam(path: str) -> Tuple[List[str], List[int], List[Alignment]]:
    with gzip.open(path, "rb") as fh:
        data = fh.read()
    if data[:4] != b"BAM\1":
        raise ValueError(f"{path}: not a BAM file")
    return parse_bam(data)


def parse_bam(data: bytes) -> Tuple[List[str], List[int], List[Alignment]]:
    """(reference names, reference lengths, records) of an inflated BAM stream"""
    o = 4
    (l_text,) = struct.unpack_from("<i", data, o)
    o += 4 + l_text
    (n_ref,) = struct.unpack_from("<i", data, o)
    o += 4
    names, lens = [], []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", data, o)
        o += 4
        names.append(data[o:o + l_name - 1].decode())
        o += l_name
        (l_ref,) = struct.unpack_from("<i", data, o)
        o += 4
        lens.append(l_ref)
    alns = []
    while o < len(data):
        (bs,) = struct.unpack_from("<i", data, o)
        o += 4
        rec = data[o:o + bs]
        o += bs
        tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 0)
        p = 32
        qname = rec[p:p + l_name - 1].decode()
        p += l_name
        cigar = []
        for k in range(n_cig):
            (v,) = struct.unpack_from("<I", rec, p + 4 * k)
            cigar.append((v >> 4, v & 0xf))
        p += 4 * n_cig
        packed = rec[p:p + (l_seq + 1) // 2]
        seq = "".join(SEQ16[(packed[i >> 1] >> (4 if i % 2 == 0 else 0)) & 0xf] for i in range(l_seq))
        p += (l_seq + 1) // 2
        qual = bytes(rec[p:p + l_seq])
        p += l_seq
        aux = bytes(rec[p:])
        alns.append(Alignment(qname, flag, tid, pos, mapq, cigar, seq, parse_tags(aux), qual, aux))
    return names, lens, alns


_INT_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}


def parse_tags(aux: bytes) -> dict:
    """The integer tags (value) and B arrays (list of values) of an aux block, by tag name (a later tag of the same name
    replaces an earlier one); the walk stops where csrc/bam_aux_walk.h gives up."""
    tags = {}
    p = 0
    while p < len(aux):
        sz = aux_value_size(aux, p)
        if sz is None:
            break
        tag, ty = aux[p:p + 2].decode("latin-1"), chr(aux[p + 2])
        if ty in _INT_FMT:
            (tags[tag],) = struct.unpack_from("<" + _INT_FMT[ty], aux, p + 3)
        elif ty == "B":
            st = chr(aux[p + 3])
            fmt = _INT_FMT.get(st, "f" if st == "f" else None)
            n = int.from_bytes(aux[p + 4:p + 8], "little")
            tags[tag] = list(struct.unpack_from(f"<{n}{fmt}", aux, p + 8)) if fmt else bytes(aux[p + 8:p + 3 + sz])
        p += 3 + sz
    return tags


from svdss_amd.bgzf import bgzf_blocks, gpu_inflate  # noqa: E402,F401  (kept importable from here)
