"""The reference stream of svdss_amd/csrc/ref_stream.hip restated: the shape it accepts as a predicate over a whole file,
and the state machine that carries a file through batches cut anywhere -- the in-header bit, the at-line-start bit, the
partial header line and the running output offset; no sequence byte is carried.  tests/test_ref_stream_mirror.py holds it
against tests.mirror.fastx.reader_records (sequences upper-cased), which restates FastxReader::next."""

DEFAULT_HEADER_CAP = 64 << 10
# the reason codes of include/svdss_hip.h (SVDSS_REF_*) as svdss_amd.refdev.REASONS names them
CR, NUL, AT, NOT_FASTA, DUPLICATE, LONG_HEADER, EMPTY = "cr", "nul", "at-line", "not-fasta", "duplicate-name", "long-header", "empty"


def upper(seq):
    return bytes(c - 32 if 97 <= c <= 122 else c for c in seq)


def name_of(line):
    e = 1
    while e < len(line) and line[e] not in b" \t":
        e += 1
    return line[1:e]


def declines(data, header_cap=DEFAULT_HEADER_CAP):
    """None if the whole file has the shape, else one reason it has not (a file may have several: the stream names the
    one it meets first, batch by batch)."""
    if not data:
        return EMPTY
    if data[:1] != b">":
        return NOT_FASTA
    if b"\r" in data:
        return CR
    if b"\0" in data:
        return NUL
    lines = data.split(b"\n")
    if any(l[:1] == b"@" for l in lines):
        return AT
    heads = [l for l in lines if l[:1] == b">"]
    if any(len(l) > header_cap for l in heads):
        return LONG_HEADER
    names = [name_of(l) for l in heads]
    if len(set(names)) != len(names):
        return DUPLICATE
    return None


def whole_file_records(data):
    """[(name, upper-cased sequence)] of a file that has the shape, from the rule of the shape alone."""
    out = []
    for l in data.split(b"\n"):
        if l[:1] == b">":
            out.append([name_of(l), []])
        else:
            out[-1][1].append(l)
    return [(n, upper(b"".join(s))) for n, s in out]


class Stream:
    """The batches of one file in order.  After close(): records = [(name, sequence)], or declined = (reason, text offset)."""

    def __init__(self, header_cap=DEFAULT_HEADER_CAP):
        self.cap = header_cap
        self.in_header, self.at_line_start = False, True
        self.carry, self.carry_out, self.carry_at = b"", 0, 0
        self.out_off = self.text_off = 0
        self.names, self.seq_off, self.out = [], [], []
        self.declined = None
        self.batches = 0

    def _decline(self, why, at):
        if self.declined is None:
            self.declined = (why, at)

    def _record(self, line, out, at):
        if len(line) > self.cap:
            return self._decline(LONG_HEADER, at)
        if name_of(line) in self.names:
            return self._decline(DUPLICATE, at)
        self.names.append(name_of(line))
        self.seq_off.append(out)

    def batch(self, text, is_last=False):
        if self.declined is not None:
            return
        # the first byte that breaks the shape
        prev_nl = self.at_line_start
        for p, c in enumerate(text):
            if p == 0 and self.text_off == 0 and c != 62:
                return self._decline(NOT_FASTA, 0)
            if c == 13:
                return self._decline(CR, self.text_off + p)
            if c == 0:
                return self._decline(NUL, self.text_off + p)
            if prev_nl and c == 64:
                return self._decline(AT, self.text_off + p)
            prev_nl = c == 10
        # the kept bytes, and where the header lines begin in the text and in the output
        s, als, kept, heads = self.in_header, self.at_line_start, bytearray(), []
        for p, c in enumerate(text):
            if als:
                s = c == 62
                if s:
                    heads.append((p, len(kept)))
            if c == 10:
                s = False
            elif not s:
                kept.append(c)
            als = c == 10
        # the header lines' text: the one that goes on from the batch in front, the complete ones, the one that goes on
        entries = ([(0, None)] if self.in_header else []) + heads
        for pos, out in entries:
            end = text.find(b"\n", pos)
            term = end >= 0
            line = text[pos:end if term else len(text)]
            if out is None:
                self.carry += line
                if len(self.carry) > self.cap:
                    return self._decline(LONG_HEADER, self.carry_at)
                if term:
                    self._record(self.carry, self.carry_out, self.carry_at)
                    self.carry = b""
            elif term:
                self._record(line, self.out_off + out, self.text_off + pos)
            elif len(line) > self.cap:
                return self._decline(LONG_HEADER, self.text_off + pos)
            else:
                self.carry, self.carry_out, self.carry_at = line, self.out_off + out, self.text_off + pos
            if self.declined is not None:
                return
        if text:
            self.in_header, self.at_line_start = bool(s), als
        self.out.append(upper(kept))
        self.out_off += len(kept)
        self.text_off += len(text)
        self.batches += 1
        if is_last:
            self.close()

    def close(self):
        if self.declined is not None:
            return
        if self.text_off == 0:
            return self._decline(EMPTY, 0)
        if self.in_header:
            self._record(self.carry, self.carry_out, self.carry_at)
            self.carry = b""
        if self.declined is None:
            self.seq_off.append(self.out_off)

    @property
    def records(self):
        assert self.declined is None
        flat = b"".join(self.out)
        return [(n, flat[a:b]) for n, a, b in zip(self.names, self.seq_off[:-1], self.seq_off[1:])]


def run(chunks, header_cap=DEFAULT_HEADER_CAP):
    """The stream over `chunks` (the last one closes it): (records or None, declined or None)."""
    st = Stream(header_cap)
    for k, c in enumerate(chunks):
        st.batch(c, k == len(chunks) - 1)
    if not chunks:
        st.close()
    return (None, st.declined) if st.declined is not None else (st.records, None)
