"""FastxReader::next (svdss_amd/csrc/fastx_reader.h) restated, the two shapes the device parser accepts
(svdss_amd/csrc/fastx_device.hip) as predicates over a whole file, their parallel restatement -- records from line starts
alone --, and the device path's plan for a file cut into batches: which records it delivers, which batch declines, what
text is left for the host reader.  tests/test_fastx_mirror.py holds the first against the C++ reader and the rest against
the first."""
import struct
import zlib


def _strip(line):
    return line.rstrip(b"\r")


def _lines(data):
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def reader_records(data):
    """[(name, sequence)] as FastxReader::next returns them, record after record."""
    lines = _lines(data)
    i, out = 0, []
    while True:
        while i < len(lines) and lines[i][:1] not in (b">", b"@"):
            i += 1
        if i >= len(lines):
            return out
        fastq = lines[i][:1] == b"@"
        head = _strip(lines[i])
        i += 1
        e = 1
        while e < len(head) and head[e] not in b" \t":
            e += 1
        seq = []
        while i < len(lines):
            c = lines[i][:1]
            if c == b">" or (not fastq and c == b"@") or (fastq and c == b"+"):
                break
            seq.append(_strip(lines[i]))
            i += 1
        seq = b"".join(seq)
        if fastq and i < len(lines) and lines[i][:1] == b"+":
            i += 1
            got = 0
            while got < len(seq) and i < len(lines):
                got += len(_strip(lines[i]))
                i += 1
        out.append((head[1:e], seq))


def _line_table(text):
    """(starts, L, n_newlines): line i is text[starts[i] : starts[i + 1] - 1]."""
    starts = [0] + [i + 1 for i, c in enumerate(text) if c == 10]
    nl = len(starts) - 1
    if text and text[-1] != 10:
        starts.append(len(text) + 1)
        return starts, nl + 1, nl
    return starts, nl, nl


def _badpos(text):
    p = [text.find(b"\r"), text.find(b"\0")]
    p = [x for x in p if x >= 0]
    return min(p) if p else None


def parse_batch(text, shape, is_last):
    """One batch as the device parses it: (records, offset of the first byte it leaves, declined)."""
    if not text:
        return [], 0, False
    starts, L, nl = _line_table(text)
    line = lambda i: text[starts[i]:starts[i + 1] - 1]
    badpos = _badpos(text)
    holds = lambda a, b: badpos is not None and a <= badpos < b
    bad = []
    if shape == "fasta":
        bad = [i for i in range(L) if line(i)[:1] == b"@" or holds(starts[i], starts[i + 1])]
        badline = min(bad) if bad else None
        heads = [i for i in range(L) if line(i)[:1] == b">"]
        if badline is None and is_last:
            limit = L
        else:
            limit = max([h for h in heads if badline is None or h <= badline], default=0)
    else:
        g4 = (L if is_last else nl) // 4 * 4
        for i in range(0, g4, 4):
            l0, l1, l2, l3 = line(i), line(i + 1), line(i + 2), line(i + 3)
            ok = l0[:1] == b"@" and l1[:1] not in (b">", b"+") and l2[:1] == b"+" and len(l3) == len(l1)
            if not ok or holds(starts[i], starts[i + 4]):
                bad.append(i)
        for i in range(g4, L):
            if (is_last and len(line(i)) > 0) or holds(starts[i], starts[i + 1]):
                bad.append(g4)
        badline = min(bad) if bad else None
        heads = list(range(0, g4, 4))
        limit = g4 if badline is None else min(badline, g4)
    recs = []
    for k, h in enumerate(h for h in heads if h < limit):
        head = line(h)
        e = 1
        while e < len(head) and head[e] not in b" \t":
            e += 1
        if shape == "fasta":
            nxt = min([x for x in heads if x > h] + [limit])
            seq = b"".join(line(i) for i in range(h + 1, min(nxt, limit)))
        else:
            seq = line(h + 1)
        recs.append((head[1:e], seq))
    carry_at = starts[limit] if limit < L else len(text)
    return recs, carry_at, badline is not None


def plan(chunks, cap):
    """The device path over batches whose fresh bytes are `chunks` (the last one closes the stream), carry cap `cap`:
    (records delivered, index of the batch that declines or None, the text from the first unparsed byte on)."""
    carry, shape, recs = b"", None, []
    for k, chunk in enumerate(chunks):
        is_last = k == len(chunks) - 1
        text = carry + chunk
        if shape is None and text:
            shape = {b">": "fasta", b"@": "fastq"}.get(text[:1], "none")
        if shape == "none":
            return recs, k, text + b"".join(chunks[k + 1:])
        r, carry_at, declined = parse_batch(text, shape, is_last)
        recs += r
        if not declined and not is_last and len(text) - carry_at > cap:
            declined = True
        if declined:
            return recs, k, text[carry_at:] + b"".join(chunks[k + 1:])
        carry = b"" if is_last else text[carry_at:]
    return recs, None, b""


def shape_of(data):
    """'fasta' / 'fastq' when the whole file has one of the two shapes the device parser delivers, else None."""
    if data[:1] not in (b">", b"@") or b"\r" in data or b"\0" in data:
        return None
    lines = _lines(data)
    if data[:1] == b">":
        return None if any(l[:1] == b"@" for l in lines) else "fasta"
    while lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        return None
    for i in range(0, len(lines), 4):
        l0, l1, l2, l3 = lines[i:i + 4]
        if not (l0[:1] == b"@" and l1[:1] not in (b">", b"+") and l2[:1] == b"+" and len(l3) == len(l1)):
            return None
    return "fastq"


def parallel_records(data):
    """The records of a file that has one of the two shapes, from its line starts alone: every record is found without
    looking at the records in front of it."""
    shape = shape_of(data)
    assert shape
    recs, _, declined = parse_batch(data, shape, True)
    assert not declined
    return recs


def nt6(seq):
    """svdss_nt6_encode: A/a 1, C/c 2, G/g 3, T/t 4, everything else 5."""
    t = bytearray([5]) * 256
    for k, c in enumerate(b"ACGT"):
        t[c] = t[c + 32] = k + 1
    return bytes(seq).translate(bytes(t))


def bgzf_pack(pieces, eof=True):
    """BGZF members, one per piece of text (a piece may be empty), and the 28-byte EOF member."""
    out = []
    for p in list(pieces) + ([b""] if eof else []):
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        c = z.compress(p) + z.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(c) + 25) + c +
                   struct.pack("<II", zlib.crc32(p), len(p)))
    return b"".join(out)
