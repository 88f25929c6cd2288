"""FASTA / FASTQ files for the tests of the device parser (tests/test_fastx_mirror.py checks the generators on the CPU,
tests/test_fastx_device_gpu.py runs the parser on them): the shapes it delivers, at sizes around the tile of its kernels,
the files it declines, and a seeded generator of small files."""
import numpy as np

from tests.mirror import fastx as M

T_DEFAULT = 4096
IUPAC = b"ACGTNacgtnRYKMSWBDHVrykmswbdhv*-"


def seq_of(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)]) if n else b""


def fasta(records, wrap=None, final_nl=True):
    out = []
    for name, seq in records:
        out.append(b">" + name)
        if wrap:
            out += [seq[i:i + wrap] for i in range(0, len(seq), wrap)]
        else:
            out.append(seq)
    return b"\n".join(out) + (b"\n" if final_nl else b"")


def fastq(records, final_nl=True):
    out = []
    for name, seq in records:
        out += [b"@" + name, seq, b"+", b"I" * len(seq)]
    return b"\n".join(out) + (b"\n" if final_nl else b"")


def length_records(rng, T, alphabet=b"ACGT"):
    return [(b"r%d" % k, seq_of(rng, n, alphabet)) for k, n in enumerate([0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])]


def delivered_cases(T=T_DEFAULT):
    """(id, file bytes): files in one of the two shapes."""
    rng = np.random.default_rng(11)
    recs = length_records(rng, T)
    out = [("fasta_one_line", fasta(recs)), ("fastq_fours", fastq(recs))]
    for w in (1, 60, 63, 64, 65, T - 1, T, T + 1):
        out.append(("fasta_wrap_%d" % w, fasta(recs[:7] if w == 1 else recs, wrap=w)))
    # a '\n' as the last byte of a tile and as the first byte of the next; a header across a tile edge
    out.append(("nl_ends_tile", fasta([(b"a", seq_of(rng, T - 4)), (b"b", seq_of(rng, 50))])))            # ">a\n" + T-4 + "\n" = T bytes
    out.append(("nl_begins_tile", fasta([(b"a", seq_of(rng, T - 3)), (b"b", seq_of(rng, 50))])))
    out.append(("header_across_tiles", fasta([(b"a", seq_of(rng, T - 10)), (b"name_across_the_edge some words", seq_of(rng, 70))])))
    names = [b"", b"x", b"n" * 300, b"id description behind a blank", b"id\tdescription behind a tab"]
    out.append(("names_fasta", fasta([(n, seq_of(rng, 40 + k)) for k, n in enumerate(names)])))
    out.append(("names_fastq", fastq([(n, seq_of(rng, 40 + k)) for k, n in enumerate(names)])))
    out.append(("no_final_newline_fasta", fasta(recs[:5], final_nl=False)))
    out.append(("no_final_newline_fastq", fastq(recs[:5], final_nl=False)))
    out.append(("trailing_empty_lines_fasta", fasta(recs[:5]) + b"\n\n\n"))
    out.append(("trailing_empty_lines_fastq", fastq(recs[:5]) + b"\n\n"))
    out.append(("empty_lines_inside_fasta", b">a\n\nACGT\n\n\nGG\n>b\n\n>c\nTT\n\n"))
    out.append(("bases_fasta", fasta(length_records(rng, T, IUPAC), wrap=70)))
    out.append(("bases_fastq", fastq(length_records(rng, T, IUPAC))))
    hi = bytes(c for c in range(1, 256) if c not in (10, 13))
    out.append(("high_bytes_fasta", fasta([(b"h", seq_of(rng, 700, hi).replace(b"\n@", b"\nA"))], wrap=61)))
    out.append(("high_bytes_fastq", fastq([(b"h", b"A" + seq_of(rng, 700, hi))])))
    out.append(("empty_file", b""))
    out.append(("one_header_alone", b">"))
    return out


def declined_cases(T=T_DEFAULT):
    """(id, file bytes): good records over a few tiles, then what the parser declines, then more records."""
    rng = np.random.default_rng(12)
    front = [(b"f%d" % k, seq_of(rng, T // 2 + 37 * k)) for k in range(6)]
    back = [(b"b%d" % k, seq_of(rng, T // 3 + 11 * k)) for k in range(4)]
    fa, fq = fasta(front, wrap=60), fastq(front)
    return [
        ("cr_fasta", fa + b">x\r\nACGT\r\n" + fasta(back)),
        ("cr_fastq", fq + b"@x\r\nACGT\r\n+\r\nIIII\r\n" + fastq(back)),
        ("nul_fasta", fa + b">x\nAC\0GT\n" + fasta(back)),
        ("nul_fastq", fq + b"@x\nAC\0GT\n+\nIIIII\n" + fastq(back)),
        ("at_line_in_fasta", fa + b"@x\nACGT\n+\nIIII\n" + fasta(back)),
        ("wrapped_fastq", fq + b"@x\nACGT\nACGT\n+\nIIII\nIIII\n" + fastq(back)),
        ("quality_of_wrong_length", fq + b"@x\nACGT\n+\nIII\n" + fastq(back)),
        ("missing_plus", fq + b"@x\nACGT\nIIII\n" + fastq(back)),
        ("truncated_last_record", fq + b"@x\nACGT\n+\n"),
        ("junk_first_line", b"junk\n" + fa),
        ("empty_first_line", b"\n" + fq),
    ]


def fuzz_file(rng):
    """(file bytes, batch bytes, BGZF pieces or None): a small file, in shape more often than not."""
    n = int(rng.integers(1, 12))
    recs = []
    for k in range(n):
        name = seq_of(rng, int(rng.integers(0, 20)), b"abcXYZ019_.:/") + (b" extra words" if rng.random() < 0.2 else b"")
        recs.append((name, seq_of(rng, int(rng.choice([0, 1, 5, 60, 61, 200, 900, 3000])), IUPAC if rng.random() < 0.3 else b"ACGT")))
    kind = int(rng.integers(0, 2))
    if kind == 0:
        data = fasta(recs, wrap=int(rng.choice([0, 1, 60, 61, 70])) or None, final_nl=rng.random() < 0.8)
    else:
        data = fastq(recs, final_nl=rng.random() < 0.8)
    if rng.random() < 0.25 and data.endswith(b"\n"):
        data += b"\n" * int(rng.integers(1, 3))
    r = rng.random()
    if r < 0.30:   # break it somewhere
        at = int(rng.integers(0, len(data) + 1))
        what = [b"\r", b"\0", b"\n@q\n", b"\n\n", b"\n+\n", b"\nACGT\n", b">", b"junk"][int(rng.integers(0, 8))]
        data = data[:at] + what + data[at:]
    batch = int(rng.choice([64, 257, 1024, 4096, 5000, 1 << 20]))
    pieces = None
    if rng.random() < 0.4:
        cuts = sorted(set(int(x) for x in rng.integers(0, len(data) + 1, size=int(rng.integers(0, 6)))))
        pieces = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
    return data, batch, pieces


def chunks_of(data, batch, pieces):
    """the fresh bytes of every batch, as svdss_amd.fastxdev cuts the input"""
    if pieces is None:
        out, off = [], 0
        while True:
            n = min(batch, len(data) - off)
            out.append(data[off:off + n])
            off += n
            if off >= len(data):
                return out
    groups, cur, acc = [], [], 0
    for p in list(pieces) + [b""]:     # (+ the EOF member)
        cur.append(p)
        acc += len(p)
        if acc >= batch:
            groups.append(b"".join(cur))
            cur, acc = [], 0
    groups.append(b"".join(cur))
    return groups


def eligible(data, chunks, cap):
    """in one of the two shapes, and no batch leaves more than `cap` bytes to the next"""
    if M.shape_of(data) is None and data:
        return False
    return M.plan(chunks, cap)[1] is None
