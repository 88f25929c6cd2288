"""Host-side mirror of `SVDSS smooth` (/root/reference/smoother.cpp): rewrite every primary
alignment so that it equals the reference except at long (> 20 bp) indels and soft clips, and tag
it with XF.  A CIGAR walk with copies from the reference -- no DP.
"""
import math
from typing import Dict, List, Sequence, Tuple

from .clusterer import (Alignment, BAM_CDEL, BAM_CDIFF, BAM_CEQUAL, BAM_CINS, BAM_CMATCH, BAM_CSOFT_CLIP,
                        FLAG_SECONDARY, FLAG_SUPPLEMENTARY, FLAG_UNMAP)

MIN_INDEL_LENGTH = 20   # config.hpp:95, not settable


def cigar_spans(aln: Alignment) -> Tuple[int, int]:
    """(bases of the reference, bases of the read) the CIGAR covers up to the first operation that is not M = X I D S
    (cigar_spans of csrc/smooth_host.cpp)."""
    rl = ql = 0
    for l, op in aln.cigar:
        if op in (BAM_CMATCH, BAM_CEQUAL, BAM_CDIFF):
            rl += l
            ql += l
        elif op == BAM_CINS or op == BAM_CSOFT_CLIP:
            ql += l
        elif op == BAM_CDEL:
            rl += l
        else:
            break
    return rl, ql


def fits(aln: Alignment, ref_len: int) -> bool:
    """cigar_fits of csrc/smooth_host.cpp: the alignment stays inside its contig and its CIGAR adds up to the read.  What does
    not fit is passed through with XF = 3 and left out of the accuracy sample (the reference walks off its buffers there)."""
    rl, ql = cigar_spans(aln)
    return aln.pos >= 0 and aln.pos + rl <= ref_len and ql == len(aln.seq)


def ratio_exceeds(n_mis: int, n_match: int, al_accuracy: float) -> bool:
    """`num_mismatch / num_match > al_accuracy` on IEEE doubles (smoother.cpp:213): 0/0 is NaN and greater than nothing,
    x/0 with x > 0 is +inf and greater than every finite threshold."""
    if n_match == 0:
        return n_mis > 0 and al_accuracy < math.inf
    return n_mis / n_match > al_accuracy


def _mismatch_counts(aln: Alignment, ref_seq: str):
    """(matches, mismatches) of the aligned stretches; None for a record that does not fit (no defined rate)."""
    if not fits(aln, len(ref_seq)):
        return None
    ref_off, q_off = aln.pos, 0
    n_match = n_mis = 0
    for l, op in aln.cigar:
        if op in (BAM_CMATCH, BAM_CEQUAL, BAM_CDIFF):
            for j in range(l):
                if ref_seq[ref_off + j] == aln.seq[q_off + j]:
                    n_match += 1
                else:
                    n_mis += 1
            ref_off += l
            q_off += l
        elif op == BAM_CINS or op == BAM_CSOFT_CLIP:
            q_off += l
        elif op == BAM_CDEL:
            ref_off += l
        else:
            break
    return n_match, n_mis


def eligible(aln: Alignment, ref_names, chromosomes, min_mapq) -> bool:
    """smoother.cpp:509-537: everything else is DROPPED from the output BAM."""
    if aln.flag & (FLAG_UNMAP | FLAG_SUPPLEMENTARY | FLAG_SECONDARY):
        return False
    if aln.mapq < min_mapq or len(aln.seq) < 2:
        return False
    return 0 <= aln.tid < len(ref_names) and ref_names[aln.tid] in chromosomes


def percentile(x: List[float], q: float) -> float:
    """smoother.cpp:246-255."""
    n = len(x)
    idx = (n - 1) * q
    lo, hi = math.floor(idx), math.ceil(idx)
    h = idx - lo
    return (1.0 - h) * x[lo] + h * x[hi]


def compute_maxaccuracy(alignments: Sequence[Alignment], ref_names, chromosomes, min_mapq=20, accp=0.98) -> float:
    """smoother.cpp:259-346: accp-percentile of mismatches/matches over the first 10 000 eligible alignments that fit
    (0 for no values, as the host's percentile).  A record without aligned bases has the rate 0/0 = NaN there; the order of
    a sort with NaN in it is undefined in the reference too, so inputs with such records are not given to this function."""
    acc = []
    for a in alignments:
        if len(acc) >= 10000:
            break
        if not eligible(a, ref_names, chromosomes, min_mapq):
            continue
        mx = _mismatch_counts(a, chromosomes[ref_names[a.tid]])
        if mx is None:
            continue
        m, x = mx
        acc.append(x / m if m else (math.inf if x else math.nan))
    if not acc:
        return 0.0
    acc.sort()
    return percentile(acc, float(accp))


def walk_read(aln: Alignment, qual: bytes, ref_seq: str):
    """The CIGAR walk of smoother.cpp:84-192 on a record that fits: (matches, mismatches, should_ignore, new_seq, new_qual,
    new_cigar) -- what svdss_smooth_batch (csrc/place.hip) returns per record, before the XF decision."""
    n_match = n_mis = 0
    new_seq: List[str] = []
    new_qual = bytearray()
    new_cigar: List[List[int]] = []
    ref_off, q_off, m_diff = aln.pos, 0, 0
    should_ignore = True

    def qslice(start, ln):   # the reference copies `ln` quality bytes from `start` (may run past the end)
        s = qual[start:start + ln]
        return s + b"\xff" * (ln - len(s))

    for l, op in aln.cigar:
        if op in (BAM_CMATCH, BAM_CEQUAL, BAM_CDIFF):
            new_seq.append(ref_seq[ref_off:ref_off + l])
            new_qual += qslice(q_off, l)
            for j in range(l):
                if ref_seq[ref_off + j] == aln.seq[q_off + j]:
                    n_match += 1
                else:
                    n_mis += 1
            ref_off += l
            q_off += l
            if new_cigar and new_cigar[-1][1] == BAM_CMATCH:
                new_cigar[-1][0] += l + m_diff
            else:
                new_cigar.append([l + m_diff, BAM_CMATCH])
            m_diff = 0
        elif op == BAM_CINS:
            if l > MIN_INDEL_LENGTH:
                should_ignore = False
                new_seq.append(aln.seq[q_off:q_off + l])
                new_qual += qslice(q_off, l)
                new_cigar.append([l, op])
            q_off += l
        elif op == BAM_CDEL:
            if l <= MIN_INDEL_LENGTH:
                new_seq.append(ref_seq[ref_off:ref_off + l])
                new_qual += qslice(q_off, l)       # qualities of the NEXT read bases (App. A#16)
                m_diff += l
            else:
                should_ignore = False
                new_cigar.append([l, op])
            ref_off += l
        elif op == BAM_CSOFT_CLIP:
            should_ignore = False
            new_seq.append(aln.seq[q_off:q_off + l])
            new_qual += qslice(q_off, l)
            q_off += l
            new_cigar.append([l, op])
        else:
            break
    return n_match, n_mis, should_ignore, "".join(new_seq), bytes(new_qual), [(l, op) for l, op in new_cigar]


def smooth_read(aln: Alignment, qual: bytes, ref_seq: str, al_accuracy: float):
    """smoother.cpp:84-232.  Returns (xf, new_seq, new_qual, new_cigar); for xf != 0 the record keeps
    its original SEQ/QUAL/CIGAR and only gets the tag.  xf = 3: the record does not fit (see fits)."""
    if not fits(aln, len(ref_seq)):
        return 3, None, None, None
    n_match, n_mis, should_ignore, new_seq, new_qual, new_cigar = walk_read(aln, qual, ref_seq)
    if ratio_exceeds(n_mis, n_match, al_accuracy):
        return 1, None, None, None
    if should_ignore:
        return 2, None, None, None
    return 0, new_seq, new_qual, new_cigar


_AUX_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def aux_value_size(aux: bytes, p: int):
    """The bytes of the value of the tag at aux[p:], or None where the walk gives up (csrc/bam_aux_walk.h, htslib's skip_aux):
    an unknown type, a tag cut off before its type byte, a Z / H without terminator, a B array whose header or elements do
    not fit (the count is unsigned: a negative one is a huge one), any value that ends behind the block."""
    room = len(aux) - p - 3
    if room < 0:
        return None
    ty = chr(aux[p + 2])
    if ty in _AUX_FIXED:
        sz = _AUX_FIXED[ty]
    elif ty in "ZH":
        z = aux.find(b"\0", p + 3)
        if z < 0:
            return None
        sz = z - (p + 3) + 1
    elif ty == "B":
        if room < 5:
            return None
        es = {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(aux[p + 3]), 4)
        sz = 5 + es * int.from_bytes(aux[p + 4:p + 8], "little")
    else:
        return None
    return sz if sz <= room else None


def update_xf(aux: bytes, v: int) -> bytes:
    """set_xf of csrc/smooth_host.cpp (bam_aux_update_int(aln, "XF", v)): the first XF of an integer type has its value
    bytes zeroed and v put in the first; without one XF:C is appended; a block the walk gives up on is returned untouched."""
    p = 0
    while p < len(aux):
        sz = aux_value_size(aux, p)
        if sz is None:
            return bytes(aux)
        if aux[p:p + 2] == b"XF" and chr(aux[p + 2]) in "cCsSiI":
            return bytes(aux[:p + 3]) + bytes([v]) + b"\0" * (sz - 1) + bytes(aux[p + 3 + sz:])
        p += 3 + sz
    return bytes(aux) + b"XFC" + bytes([v])
