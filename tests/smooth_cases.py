"""The edge battery of `SVDSS smooth` (tests/test_smooth_edges.py, test_smooth_edges_gpu.py): two contigs of about 4 kb
(the second with a run of N; a third one is in the BAM header only), and records of 2-450 bases whose names say what they
are -- indels on both sides of the 20 bp threshold, short deletions whose qualities are read past the read's end, runs that
merge, operations that end the walk, records without an aligned base, the exact accuracy threshold, alignments at and past
the contig's end, lengths and CIGAR operation counts round the 64 lanes of a wavefront, passed-through records of every
length and offset modulo 4, XF tags of every type and place, aux blocks the walk gives up on, IUPAC bases, and everything
the filters drop.  What a record must become comes from tests/mirror/smoother.py alone, never from the code under test.
Everything is built once per process from a fixed seed and never changed."""
import functools
import math
import random
import struct
from typing import List, NamedTuple, Optional

from tests import bam_writer
from tests.mirror import smoother
from tests.mirror.clusterer import Alignment

SEED = 20260117
NAMES = ["c0", "c1", "c2"]            # (c2: in the BAM header, not in the FASTA -- its records are dropped)
MIN_MAPQ = 20
OPCODE = {c: i for i, c in enumerate("MIDNSHP=X")}
ACC = 1 / 99                          # the rate of `onemis`: 1 mismatch on 99 matches
ACC_BELOW = math.nextafter(ACC, 0.0)  # the next double below it
ACCP = struct.unpack("<f", struct.pack("<f", 0.98))[0]   # --accp is a float in the CLI (cli_options.h)


class Case(NamedTuple):
    name: str
    flag: int
    tid: int
    pos: int
    mapq: int
    cigar: list                       # [(op character, length)]
    seq: str
    qual: Optional[bytes]             # None: absent (0xff)
    aux: bytes
    nomatch: bool                     # no aligned base: its mismatch rate is 0/0


class Battery(NamedTuple):
    contigs: List[str]                # upper case, those of the FASTA (c0, c1)
    ref_lens: List[int]               # of the BAM header (c0, c1, c2)
    fasta: str
    bam: bytes                        # BGZF members of about 1,000 bytes each, so that small batches cut through records
    cases: List[Case]                 # in file order
    alns: List[Alignment]


class Expect(NamedTuple):
    name: str
    xf: int
    seq: str
    qual: bytes
    cigar: list                       # [(length, op code)]
    aux: bytes


def tag(name, ty, value):
    fmt = {"A": "c", "c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}
    if ty in "ZH":
        return name.encode() + ty.encode() + value.encode() + b"\0"
    return name.encode() + ty.encode() + struct.pack("<" + fmt[ty], value.encode() if ty == "A" else value)


def b_array(name, sub, count, payload_elems=None):
    """A B array whose count field says `count` and which carries payload_elems elements (default: as many)."""
    es = {"c": 1, "C": 1, "s": 2, "S": 2}.get(sub, 4)
    n = count if payload_elems is None else payload_elems
    return name.encode() + b"B" + sub.encode() + struct.pack("<I", count & 0xffffffff) + bytes((7 * k + 1) & 0x7f for k in range(n * es))


def raw_record(c: Case) -> bytes:
    r = bam_writer.record(c.name, c.flag, c.tid, c.pos, c.mapq, c.cigar, c.seq, [], c.qual) + c.aux
    return struct.pack("<i", len(r) - 4) + r[4:]


@functools.lru_cache(maxsize=None)
def contigs():
    rng = random.Random(SEED)
    c0 = "".join(rng.choices("ACGT", k=4099))
    c1 = "".join(rng.choices("ACGT", k=3990))
    return [c0, c1[:1000] + "N" * 60 + c1[1060:]]


def fasta_text():
    """Lines of 61 columns, a lower-case stretch in c0 (load_chromosomes upper-cases)."""
    out = []
    for n, c in zip(NAMES, contigs()):
        t = c[:200] + c[200:900].lower() + c[900:] if n == "c0" else c
        out.append(f">{n} edge battery\n" + "".join(t[i:i + 61] + "\n" for i in range(0, len(t), 61)))
    return "".join(out)


class _Builder:
    def __init__(self):
        self.rng = random.Random(SEED + 1)
        self.ref = contigs()
        self.cases = []
        self.at = [40, 40]            # where the next record of a contig goes: the file stays sorted by (tid, pos)

    def bases(self, n):
        return "".join(self.rng.choices("ACGT", k=n))

    def read_of(self, tid, pos, ops):
        """The read a CIGAR describes at pos: M / = copy the reference, X differs from it everywhere, I / S are random."""
        ref, out, rp = self.ref[tid], [], max(pos, 0)
        for op, l in ops:
            if op in "M=X":
                s = ref[rp:rp + l]
                s += self.bases(l - len(s))             # (past the contig's end: anything)
                if op == "X":
                    s = "".join(self.rng.choice([b for b in "ACGT" if b != ch]) for ch in s)
                out.append(s)
                rp += l
            elif op in "IS":
                out.append(self.bases(l))
            elif op in "DN":
                rp += l
        return "".join(out)

    def mutate(self, tid, pos, ops, seq, n_mis):
        """n_mis mismatches at aligned positions of the read (spread evenly)"""
        aligned, q, rp = [], 0, pos
        for op, l in ops:
            if op in "M=X":
                aligned += [(q + j, rp + j) for j in range(l)]
                q += l
                rp += l
            elif op in "IS":
                q += l
            elif op in "DN":
                rp += l
            else:
                break
        s = list(seq)
        step = len(aligned) / max(1, n_mis)
        for k in range(n_mis):
            qi, ri = aligned[int(k * step)]
            s[qi] = self.rng.choice([b for b in "ACGT" if b != self.ref[tid][ri]])
        return "".join(s)

    def add(self, name, ops, *, tid=0, pos=None, flag=0, mapq=60, aux=b"", qual=True, seq=None, mis=0, nomatch=False, step=11):
        if pos is None:
            pos = self.at[tid]
            self.at[tid] += step
        if seq is None:
            seq = self.read_of(tid, pos, ops)
        if mis:
            seq = self.mutate(tid, pos, ops, seq, mis)
        q = bytes(self.rng.randrange(1, 60) for _ in seq) if qual else None
        assert all(c.name != name for c in self.cases), name
        self.cases.append(Case(name, flag, tid, pos, mapq, list(ops), seq, q, aux, nomatch))


def _alternating(n_ops, long_every=0, first=("S", 3)):
    """n_ops operations: a clip, then M1 with I1 / D1 in turn between them; long_every > 0: every so many indels one of 21"""
    ops, k = [first], 0
    while len(ops) < n_ops:
        if len(ops) % 2 == 1:
            ops.append(("M", 1))
        else:
            k += 1
            ops.append(("ID"[k % 2], 21 if long_every and k % long_every == 0 else 1))
    return ops[:n_ops]


def _build_cases():
    B = _Builder()
    add = B.add
    L0, L1 = len(B.ref[0]), len(B.ref[1])
    nm, rg = tag("NM", "i", 7), tag("RG", "Z", "grp")

    # ---- fit: pos = 0, and (further down) the contig's end
    add("fit_pos0", [("S", 3), ("M", 50)], pos=0)
    add("fit_pos0_rev", [("M", 50), ("S", 3)], pos=0, flag=16)

    # ---- threshold: I and D of 19, 20, 21, alone (XF 2, 2, 0) and with a clip
    for k in (19, 20, 21):
        add(f"thr_I{k}", [("M", 50), ("I", k), ("M", 50)])
        add(f"thr_D{k}", [("M", 50), ("D", k), ("M", 50)])
        add(f"thr_S7_I{k}", [("S", 7), ("M", 50), ("I", k), ("M", 50)])
        add(f"thr_D{k}_S7", [("M", 50), ("D", k), ("M", 50), ("S", 7)])

    # ---- qualities past the read's end: a short D with fewer read bases behind it than it has (0xff fill), as the last
    # operation (m_diff without a following M is dropped) and as the first; the same with absent qualities
    for qual in (True, False):
        s = "" if qual else "_noqual"
        add(f"qpast_D5_M3{s}", [("S", 10), ("M", 40), ("D", 5), ("M", 3)], qual=qual)
        add(f"qpast_D20_M3{s}", [("S", 10), ("M", 40), ("D", 20), ("M", 3)], qual=qual)
        add(f"qpast_D5_last{s}", [("S", 10), ("M", 40), ("D", 5)], qual=qual)
        add(f"qpast_D20_last{s}", [("S", 9), ("M", 40), ("D", 20)], qual=qual)
        add(f"qpast_D5_first{s}", [("D", 5), ("M", 40), ("S", 10)], qual=qual)
        add(f"qpast_S_D5_M2{s}", [("S", 10), ("D", 5), ("M", 2)], qual=qual)
        add(f"qpast_I30_D7_last{s}", [("M", 20), ("I", 30), ("M", 3), ("D", 7)], qual=qual)

    # ---- merging
    add("merge_eq_X_eq", [("S", 5), ("=", 30), ("X", 2), ("=", 30)])
    add("merge_M_eq_X_M", [("M", 10), ("=", 20), ("X", 1), ("M", 10), ("S", 4)])
    add("merge_M_D7_M", [("S", 5), ("M", 30), ("D", 7), ("M", 30)])
    add("merge_M_I7_M", [("S", 5), ("M", 30), ("I", 7), ("M", 30)])
    add("merge_M_D25_D6_M", [("M", 30), ("D", 25), ("D", 6), ("M", 30)])
    add("merge_M_D6_D25_M", [("M", 30), ("D", 6), ("D", 25), ("M", 30)])
    add("merge_M_I25_M_I3_M", [("M", 30), ("I", 25), ("M", 10), ("I", 3), ("M", 31)])
    for a in (20, 21):
        for b in (20, 21):
            add(f"adj_D{a}_I{b}", [("M", 30), ("D", a), ("I", b), ("M", 30)])
            add(f"adj_I{a}_D{b}", [("M", 30), ("I", a), ("D", b), ("M", 31)])

    # ---- operations that end the walk
    add("end_H_first", [("H", 5), ("M", 50)])
    add("end_H_last_fits", [("S", 5), ("M", 50), ("H", 5)])
    add("end_H_last_fits_plain", [("M", 50), ("H", 5)])
    add("end_N_middle", [("M", 30), ("N", 10), ("M", 30)])
    add("end_P_middle", [("S", 4), ("M", 30), ("P", 2), ("M", 30)])
    add("nomatch_S_H_fits", [("S", 31), ("H", 9)], nomatch=True)

    # ---- no aligned base: 0/0 is not greater than anything (XF 0 with a clip or a long I, XF 2 without)
    add("nomatch_all_S", [("S", 50)], nomatch=True)
    add("nomatch_all_I30", [("I", 30)], nomatch=True)
    add("nomatch_all_I10", [("I", 10)], nomatch=True)
    add("nomatch_S_I_S", [("S", 10), ("I", 25), ("S", 10)], nomatch=True)
    add("nomatch_S_D30", [("S", 12), ("D", 30)], nomatch=True)

    # ---- the exact accuracy threshold
    add("acc_all_X", [("X", 40)])                                    # x / 0 is greater than every threshold
    add("acc_S_all_X", [("S", 6), ("X", 41)])
    add("onemis", [("S", 5), ("M", 100)], mis=1)                       # 1 / 99: XF 0 at ACC, XF 1 at ACC_BELOW
    add("onemis_plain", [("M", 100)], mis=1)
    add("twomis_198", [("S", 5), ("M", 200)], mis=2)                   # 2 / 198 = 1 / 99 as doubles
    for k in range(5):                                               # dirty reads of several rates
        add(f"dirty_{k}", [("S", 4), ("M", 120 + k)], mis=6 + 9 * k)

    # ---- the shapes of the wavefront code: M, long I and S of 1, 63, 64, 65, 128, 129
    for n in (1, 63, 64, 65, 128, 129):
        add(f"wave_S{n}_M{n}_I{max(n, 21)}", [("S", n), ("M", n), ("I", max(n, 21)), ("M", 10)], step=17)
        add(f"wave_M{n}_D21_S{n}", [("M", n), ("D", 21), ("M", 1), ("S", n)], step=17)
    # CIGARs of 1, 2, 63, 64, 65, 127, 128, 129 and about 300 operations, all-short indels and with long ones
    add("ops_1", [("M", 20)])
    for n in (2, 63, 64, 65, 127, 128, 129, 300, 301):
        add(f"ops_{n}_short", _alternating(n), step=17)
        add(f"ops_{n}_long", _alternating(n, long_every=7), step=17)
        add(f"ops_{n}_short_noclip", _alternating(n, first=("M", 2)), step=17)       # XF 2: the copy of a long CIGAR
    add("ops_300_long_rev", _alternating(300, long_every=7), flag=16, step=17)
    # an operation that ends the walk as operation 64 and as operation 65
    for n in (63, 64):
        add(f"ops_{n}_then_H_fits", _alternating(n) + [("H", 5)])
        add(f"ops_{n}_long_then_H_fits", _alternating(n, long_every=5) + [("H", 5)])
        add(f"ops_{n}_then_N_M", _alternating(n) + [("N", 5), ("M", 10)])
        add(f"ops_{n}_then_P_I30", _alternating(n) + [("P", 1), ("I", 30)])
    # reads of 2 and 3 bases
    add("len2_S1_M1", [("S", 1), ("M", 1)])
    add("len2_M2", [("M", 2)])
    add("len3_S1_M2", [("S", 1), ("M", 2)])
    add("len3_M1_D1_M1_S1", [("M", 1), ("D", 1), ("M", 1), ("S", 1)])
    add("len3_noqual", [("S", 2), ("M", 1)], qual=False)

    # ---- the pass-through copy: XF 1 / 2 / 3 records, names of 1-8 characters, aux blocks of 0-7 bytes (those of 1-3 bytes
    # are a cut-off tag: left alone)
    aux_of = [b"", b"Z", b"ZA", b"ZAC", tag("ZA", "C", 200), tag("ZA", "s", -2), tag("ZA", "Z", "ab"), tag("ZA", "i", -70000)]
    for xf in (1, 2, 3):
        for nl in range(1, 9):
            name = (f"{xf}" + "pqrstuvw"[:nl - 1])[:nl] if nl > 1 else "abc"[xf - 1]
            n = 40 + (nl + xf) % 4
            aux = aux_of[(3 * nl + xf) % 8]
            if xf == 1:
                add(name, [("M", n)], mis=8 + 3 * nl, aux=aux, step=3)
            elif xf == 2:
                add(name, [("M", n)], aux=aux, step=3)
            else:
                add(name, [("M", n + 1)], seq=B.read_of(0, B.at[0], [("M", n)]), aux=aux, step=3)

    # ---- where XF is: absent, every integer type as the first, a middle and the last tag (rebuilt records; in the middle
    # also passed-through ones), behind XF:Z, as XF:A / XF:f, behind well-formed B arrays
    rebuilt, passed = [("S", 5), ("M", 50)], [("M", 50)]
    add("xf_absent_noaux", rebuilt)
    add("xf_absent_tags", rebuilt, aux=nm + rg)
    add("xf_absent_tags_pass", passed, aux=nm + rg)
    val = {"c": -100, "C": 200, "s": -30000, "S": 60000, "i": -2000000000, "I": 4000000000}
    for ty, v in val.items():
        xf = tag("XF", ty, v)
        add(f"xf_{ty}_first", rebuilt, aux=xf + nm + rg)
        add(f"xf_{ty}_middle", rebuilt, aux=nm + xf + rg)
        add(f"xf_{ty}_last", rebuilt, aux=nm + rg + xf)
        add(f"xf_{ty}_middle_pass", passed, aux=nm + xf + rg)
        add(f"xf_{ty}_alone_pass", passed, aux=xf)
    add("xf_Z_then_i", rebuilt, aux=tag("XF", "Z", "text") + tag("XF", "i", 77) + nm)
    add("xf_Z_then_i_pass", passed, aux=tag("XF", "Z", "text") + tag("XF", "i", 77) + nm)
    add("xf_Z_only", rebuilt, aux=nm + tag("XF", "Z", "text"))
    add("xf_A", rebuilt, aux=tag("XF", "A", "q") + nm)
    add("xf_f", rebuilt, aux=nm + tag("XF", "f", 1.5))
    add("xf_H", passed, aux=tag("XF", "H", "1AE3") + rg)
    add("xf_twice", rebuilt, aux=tag("XF", "C", 9) + tag("XF", "i", 99))
    arrays = b"".join(b_array("ZB", st, 0) + b_array("ZA", st, 3) for st in "cCsSiIf")
    add("xf_behind_B_arrays", rebuilt, aux=arrays + tag("XF", "i", 1234567) + rg)
    add("xf_behind_B_arrays_pass", passed, aux=arrays + tag("XF", "s", 1234))
    add("xf_absent_B_arrays", rebuilt, aux=arrays)
    add("xf_is_B_array", rebuilt, aux=b_array("XF", "C", 2))
    # what the walk gives up on is left untouched (never a negative count here: tests/test_aux_walk_host.py has those)
    add("aux_B_overrun", rebuilt, aux=nm + b_array("ZZ", "i", 100, 2) + tag("XF", "i", 5))
    add("aux_B_overrun_pass", passed, aux=b_array("ZZ", "s", 5, 4))
    add("aux_truncated_XFi", rebuilt, aux=nm + b"XFi\x01")
    add("aux_truncated_XFi_pass", passed, aux=nm + b"XFi\x01")
    add("aux_truncated_XFs_pass", passed, aux=b"XFs\x01")
    add("aux_unknown_type", rebuilt, aux=b"ZZQ1234" + tag("XF", "i", 5))
    add("aux_Z_unterminated", rebuilt, aux=tag("XF", "Z", "x") + b"RGZgrp")
    add("aux_after_give_up", rebuilt, aux=nm)                         # (the record behind them is whole)

    # ---- bases: IUPAC and = in the read
    iupac = "=ACMGRSVTWYHKDBN"
    add("iupac_in_S_and_I", [("S", 16), ("M", 40), ("I", 32), ("M", 21)],
        seq=iupac + B.ref[0][B.at[0]:B.at[0] + 40] + iupac[::-1] * 2 + B.ref[0][B.at[0] + 40:B.at[0] + 61])
    s = B.read_of(0, B.at[0], [("S", 3), ("M", 300)])
    add("iupac_in_M", [("S", 3), ("M", 300)], seq=s[:100] + "R" + s[101:200] + "=" + s[201:])
    add("long_clean_M400", [("M", 400)])
    add("long_S10_M390_3mis", [("S", 10), ("M", 390)], mis=3)
    add("long_M200_D40_M200_1mis", [("M", 200), ("D", 40), ("M", 200)], mis=1)

    # ---- what the filters drop; the reverse strand, MAPQ 19 and 20
    add("flag_reverse", [("S", 5), ("M", 50)], flag=16)
    add("drop_secondary", [("S", 5), ("M", 50)], flag=256)
    add("drop_supplementary", [("S", 5), ("M", 50)], flag=2048)
    add("drop_unmapped_flag", [("S", 5), ("M", 50)], flag=4)
    add("drop_mapq19", [("S", 5), ("M", 50)], mapq=19)
    add("keep_mapq20", [("S", 5), ("M", 50)], mapq=20)
    add("drop_len1", [("M", 1)])
    add("drop_len0", [], seq="")
    add("drop_len1_S", [("S", 1)])

    # ---- the second contig: N in the reference, and the contig's end
    B.at[1] = 940
    add("refN_read_copies_N", [("S", 5), ("M", 150)], tid=1)
    add("refN_read_has_bases", [("S", 5), ("M", 150)], tid=1, seq=B.bases(5) + B.read_of(1, B.at[1], [("M", 150)]).replace("N", "A"))
    add("refN_D_over_N", [("M", 40), ("D", 18), ("M", 40), ("S", 3)], tid=1, pos=985)
    add("refN_long_D_over_N", [("M", 40), ("D", 70), ("M", 40)], tid=1, pos=955)
    B.at[1] = 2000
    for k in range(16):
        add(f"c1_clean_{k}", [("M", 350 + k)], tid=1, step=29)
        add(f"c1_clip_{k}", [("S", 20 + k), ("M", 300), ("I", 40 + k), ("M", 30)], tid=1, step=29, mis=k)
    add("fit_ends_at_last_base", [("S", 3), ("M", 50)], tid=1, pos=L1 - 50)
    add("fit_D_reaches_the_end", [("S", 3), ("M", 30), ("D", 20)], tid=1, pos=L1 - 50)
    add("fit_long_D_reaches_the_end", [("S", 3), ("M", 29), ("D", 21)], tid=1, pos=L1 - 50)
    add("fit_one_past_the_end", [("S", 3), ("M", 50)], tid=1, pos=L1 - 49)
    add("fit_D_one_past_the_end", [("S", 3), ("M", 30), ("D", 20)], tid=1, pos=L1 - 49)
    add("fit_cigar_one_short", [("S", 3), ("M", 49)], tid=1, pos=L1 - 300, seq=B.read_of(1, L1 - 300, [("S", 3), ("M", 50)]))
    add("fit_cigar_one_long", [("S", 3), ("M", 51)], tid=1, pos=L1 - 300, seq=B.read_of(1, L1 - 300, [("S", 3), ("M", 50)]))
    add("fit_last_base_M1", [("S", 1), ("M", 1)], tid=1, pos=L1 - 1)
    add("fit_pos_is_the_length", [("S", 1), ("M", 1)], tid=1, pos=L1)
    add("last_whole_record", [("S", 5), ("M", 50)], tid=1, pos=L1 - 60)
    # ---- the contig the FASTA lacks
    add("drop_no_such_contig", [("S", 5), ("M", 50)], tid=2, pos=10, seq=B.bases(55))
    add("drop_no_such_contig_2", [("M", 50)], tid=2, pos=100, seq=B.bases(50))
    assert L0 > B.at[0] + 500, B.at
    return B.cases


def alignment_of(c: Case) -> Alignment:
    qual = b"\xff" * len(c.seq) if c.qual is None else c.qual
    return Alignment(c.name, c.flag, c.tid, c.pos, c.mapq, [(l, OPCODE[op]) for op, l in c.cigar], c.seq.upper(), {}, qual, c.aux)


@functools.lru_cache(maxsize=None)
def battery(nomatch=True) -> Battery:
    """nomatch=False: without the records that have no aligned base (their rate, NaN, would enter the percentile's sort)"""
    cases = [c for c in _all_cases() if nomatch or not c.nomatch]
    cs = contigs()
    lens = [len(cs[0]), len(cs[1]), 500]
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(NAMES, lens))
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(lens))
    for n, l in zip(NAMES, lens):
        hdr += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    data = bam_writer.bgzf(hdr + b"".join(raw_record(c) for c in cases), block=1000)
    return Battery(cs, lens, fasta_text(), data, cases, [alignment_of(c) for c in cases])


@functools.lru_cache(maxsize=None)
def _all_cases():
    cases = _build_cases()
    order = sorted(range(len(cases)), key=lambda i: (cases[i].tid, cases[i].pos, i))
    cases = [cases[i] for i in order]
    # (what the walk gives up on is never the file's last record: the parent's overwrite went into the record behind)
    assert not cases[-1].name.startswith("aux_") and all(len(c.seq) <= 460 for c in cases)
    return cases


def chromosomes():
    return dict(zip(NAMES[:2], contigs()))


def kept(b: Battery) -> List[Alignment]:
    ch = chromosomes()
    return [a for a in b.alns if smoother.eligible(a, NAMES, ch, MIN_MAPQ)]


def file_accuracy(b: Battery, accp: float = ACCP) -> float:
    """the threshold the CLI computes for the battery file (compute_maxaccuracy; the CLI's --accp is a float: pass one that
    a float holds exactly, such as 0.5, or the default)"""
    return smoother.compute_maxaccuracy(b.alns, NAMES, chromosomes(), MIN_MAPQ, accp)


def passed_through_sizes(want: List[Expect], xf: int):
    """the input record lengths modulo 4 of the records `want` passes through with that XF"""
    size = {c.name: len(raw_record(c)) for c in _all_cases()}
    return {size[e.name] % 4 for e in want if e.xf == xf}


@functools.lru_cache(maxsize=None)
def expected(nomatch: bool, acc: float) -> List[Expect]:
    """What `smooth` makes of the battery at the accuracy threshold acc, record by record in file order, by the mirror."""
    b, ch, out = battery(nomatch), chromosomes(), []
    for a in kept(b):
        xf, ns, nq, nc = smoother.smooth_read(a, a.qual, ch[NAMES[a.tid]], acc)
        if xf != 0:
            ns, nq, nc = a.seq, a.qual, list(a.cigar)
        out.append(Expect(a.qname, xf, ns, nq, nc, smoother.update_xf(a.aux, xf)))
    return out


def check_battery_covers_what_it_says():
    """The battery's own sanity, against the mirror: every XF value, both parities of a smoothed length, passed-through
    records of every length modulo 4, the threshold pair."""
    want = {e.name: e for e in expected(True, ACC)}
    below = {e.name: e for e in expected(True, ACC_BELOW)}
    assert [want[f"thr_{x}{k}"].xf for x in "ID" for k in (19, 20, 21)] == [2, 2, 0, 2, 2, 0]
    assert want["onemis"].xf == 0 and below["onemis"].xf == 1 and want["twomis_198"].xf == 0 and below["twomis_198"].xf == 1
    assert want["acc_all_X"].xf == 1 and want["nomatch_all_S"].xf == 0 and want["nomatch_all_I10"].xf == 2 and want["nomatch_S_I_S"].xf == 0
    assert want["end_H_first"].xf == 3 and want["end_H_last_fits"].xf == 0 and want["end_N_middle"].xf == 3 and want["end_P_middle"].xf == 3
    assert want["fit_ends_at_last_base"].xf == 0 and want["fit_one_past_the_end"].xf == 3 and want["fit_D_reaches_the_end"].xf == 0
    assert want["qpast_D5_last"].qual[-5:] == b"\xff" * 5 and want["qpast_D5_M3"].qual[-5:-3] == b"\xff" * 2
    assert want["aux_truncated_XFi"].aux.endswith(b"XFi\x01") and b"XFC" not in want["aux_B_overrun"].aux
    assert {len(e.seq) % 2 for e in want.values() if e.xf == 0} == {0, 1}
    assert "drop_mapq19" not in want and "keep_mapq20" in want and "drop_no_such_contig" not in want and "drop_len1" not in want
    b = battery(True)
    size = {c.name: len(raw_record(c)) for c in b.cases}
    for xf in (1, 2, 3):
        assert {size[e.name] % 4 for e in want.values() if e.xf == xf and len(e.name) <= 8} == {0, 1, 2, 3}, xf
    return want
