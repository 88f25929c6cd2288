"""Reference FASTA files for the tests of the reference stream (tests/test_ref_stream_mirror.py runs the mirror on them on
the CPU, tests/test_ref_stream_gpu.py the device): the files it delivers, at sizes around the tile of its kernels; member
and batch cuts; the files it declines with their reasons; a seeded generator of small files."""
import numpy as np

from tests.fastx_cases import IUPAC, chunks_of, fasta, seq_of
from tests.mirror import refstream as R

T_DEFAULT = 4096
CAP_SMALL = 3 * 4096 + 17          # a header cap the long-header cases reach with a small file
MEMBER = 1777                      # the delivered cases as BGZF: members of this many bytes
WAYS = [("plain_1M", 1 << 20, False), ("plain_1K", 1024, False), ("bgzf_1M", 1 << 20, True), ("bgzf_1K", 1024, True), ("bgzf_member", 1, True)]


def members(data, size=MEMBER):
    return [data[i:i + size] for i in range(0, len(data), size)]


def delivered_cases(T=T_DEFAULT):
    """(id, file bytes, header cap or None)"""
    rng = np.random.default_rng(31)
    out = []
    for n in (1, T - 1, T, T + 1, 3 * T + 5):
        for nl in (True, False):
            out.append(("one_line_%d_%s" % (n, "nl" if nl else "nonl"), fasta([(b"chr1", seq_of(rng, n))], final_nl=nl), None))
    recs = [(b"c%d" % k, seq_of(rng, n)) for k, n in enumerate([3 * T + 5, 61, 60, 1, 2 * T])]
    for w in (60, 61):
        out.append(("wrap_%d" % w, fasta(recs, wrap=w), None))
    out.append(("wrap_1", fasta(recs[1:4] + [(b"w", seq_of(rng, T + 3))], wrap=1), None))
    out.append(("header_across_tiles", fasta([(b"a", seq_of(rng, T - 10)), (b"name_across_the_edge some words", seq_of(rng, 70))]), None))
    long_name = b"n" * (CAP_SMALL - 1)                                            # '>' + name = the cap
    out.append(("header_as_long_as_cap", fasta([(b"a", seq_of(rng, 100)), (long_name, seq_of(rng, 100)), (b"z", seq_of(rng, 9))], wrap=60), CAP_SMALL))
    out.append(("records_3000", fasta([(b"r%d" % k, seq_of(rng, int(n))) for k, n in enumerate(rng.integers(1, 41, size=3000))]), None))
    out.append(("no_sequence_between_headers", b">a\nACGT\n>b\n>c\nGG\n>d\n", None))
    out.append(("empty_lines", b">a\n\nACGT\n\n\nGG\n>b\n\n>c\nTT\n\n\n", None))
    out.append(("names", fasta([(b"tab\tdescription", b"ACGT"), (b"blank description behind", b"GGA"), (b"eol", b"TT"), (b"", b"AC")]), None))
    out.append(("lower_iupac", fasta([(b"m%d" % k, seq_of(rng, n, IUPAC)) for k, n in enumerate([T + 1, 70, 3 * T])], wrap=70), None))
    out.append(("header_alone_no_newline", b">x", None))
    return out


def cut_cases(T=T_DEFAULT):
    """the file, and [(id, the text of every BGZF member, whether the EOF member follows)]"""
    rng = np.random.default_rng(32)
    recs = [(b"contig_%d some words" % k, seq_of(rng, 300 + 7 * k, IUPAC)) for k in range(8)]
    data = fasta(recs, wrap=60)
    inside_name = data.index(b"contig_5") + 3
    head_nl = data.index(b"\n", inside_name) + 1
    gt = data.index(b">contig_3")
    nl = data.index(b"\n", gt + 40)

    def at(cuts):
        cuts = [0] + list(cuts) + [len(data)]
        return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    out = [("one_byte_members_and_an_empty_one", at([1, 2, 3, 3, len(data) // 2]), True),
           ("inside_a_name", at([inside_name]), True),
           ("behind_a_headers_newline", at([head_nl]), True),
           ("gt_is_the_last_byte", at([gt + 1]), True),
           ("newline_is_the_first_byte", at([nl]), True),
           ("header_over_three_batches", at([inside_name - 2, inside_name, inside_name + 2]), True),
           ("no_eof_member", at([len(data) // 3]), False),
           ("empty_last_batch", at([len(data) // 3]) + [b""], True)]
    return data, out


def declined_cases(T=T_DEFAULT):
    """(id, file bytes, header cap or None, reason)"""
    rng = np.random.default_rng(33)
    front = fasta([(b"f%d" % k, seq_of(rng, T // 2 + 37 * k)) for k in range(5)], wrap=60)
    back = fasta([(b"b%d" % k, seq_of(rng, T // 3 + 11 * k)) for k in range(3)])
    return [("cr", front + b">x\r\nACGT\r\n" + back, None, R.CR),
            ("nul", front + b">x\nAC\0GT\n" + back, None, R.NUL),
            ("at_line", front + b"@x\nACGT\n" + back, None, R.AT),
            ("first_byte", b"ACGT\n" + front, None, R.NOT_FASTA),
            ("duplicate_name", front + b">f2 again\nACGT\n" + back, None, R.DUPLICATE),
            ("header_of_cap_plus_1", front + b">" + b"n" * CAP_SMALL + b"\nACGT\n" + back, CAP_SMALL, R.LONG_HEADER),
            ("empty_file", b"", None, R.EMPTY)]


def fuzz_file(rng):
    """(file bytes, batch bytes, BGZF pieces or None): a small FASTA, in shape more often than not."""
    recs = []
    for k in range(int(rng.integers(1, 10))):
        name = b"s%d_" % k + seq_of(rng, int(rng.integers(0, 12)), b"abcXYZ019_.:/") + (b" extra words" if rng.random() < 0.2 else b"")
        recs.append((name, seq_of(rng, int(rng.choice([0, 1, 5, 60, 61, 200, 900, 3000, 9000])), IUPAC if rng.random() < 0.4 else b"ACGT")))
    wrap = int(rng.choice([1, 60, 61, int(rng.integers(1, 201))])) if rng.random() < 0.85 else None
    if wrap is not None and wrap < 4:
        recs = [(n, s[:300]) for n, s in recs]
    data = fasta(recs, wrap=wrap, final_nl=rng.random() < 0.8)
    if rng.random() < 0.4:       # empty lines inside and at the end
        for _ in range(int(rng.integers(1, 4))):
            at = data.find(b"\n", int(rng.integers(0, len(data))))
            if at >= 0:
                data = data[:at] + b"\n" + data[at:]
    r = rng.random()
    if r < 0.30:                 # break it
        at = int(rng.integers(0, len(data) + 1))
        what = [b"\r", b"\0", b"\n@q\n", b"\n>s0_\n"][int(rng.integers(0, 4))]
        data = data[:at] + what + data[at:]
    batch = int(rng.choice([64, 257, 1024, 4096, 5000, 1 << 20]))
    pieces = None
    if rng.random() < 0.4:
        cuts = sorted(int(x) for x in rng.integers(0, len(data) + 1, size=int(rng.integers(0, 6))))
        pieces = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
    return data, batch, pieces


__all__ = ["chunks_of", "cut_cases", "declined_cases", "delivered_cases", "fuzz_file", "members", "WAYS"]
