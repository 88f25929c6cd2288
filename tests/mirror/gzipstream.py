"""Pure-Python mirror of csrc/gzip_stream.hip + gzip_stream.h: one deflate stream inflated chunk-parallel.

The same steps as the device unit, in the same order and with the same rules, so that it is the oracle for the PLAN of a
run -- which chunks have a start, the chain, the bytes per chunk, where the unit declines -- and, through marker decode and
resolve, for the bytes.  Bit positions are relative to the first byte of the window (bit 0 = its least significant bit).

  find      lowest bit offset of every chunk but the first that passes the dynamic-header tests (find_start)
  measure   walk block after block from a start to the first block end that is a later chunk's start (walk)
  chain     0 -> m0 -> m1 ...; chunks off the chain are merged (no start) or false starts
  decode    the same walk storing 16-bit symbols: 0..255 bytes, 256 + j = byte j of the 32 KB in front of the chunk
  window    dictionary k+1 from the last 32 KB of chunk k's symbols resolved through dictionary k
  resolve   byte = sym < 256 ? sym : dict[sym - 256]
"""
import zlib

import numpy as np

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)

# reasons a run declines (the values of include/svdss_hip.h)
DECLINE_NONE, DECLINE_HEADER, DECLINE_NO_START, DECLINE_NO_ADVANCE, DECLINE_DAMAGED, DECLINE_TRAILING = 0, 1, 2, 3, 4, 5
TAIL = 64       # an invalid code this close (bits) to the window's end is "the window ran out", not damage


def parse_header(b):
    """The gzip member header at b[0:]: its length, 0 = not complete yet, -1 = not one."""
    n = len(b)
    for i, v in enumerate((0x1f, 0x8b, 8)):
        if n > i and b[i] != v:
            return -1
    if n < 10:
        return 0
    flg = b[3]
    if flg & 0xe0:
        return -1
    p = 10
    if flg & 4:
        if n < p + 2:
            return 0
        p += 2 + b[p] + 256 * b[p + 1]
    for bit in (8, 16):
        if flg & bit:
            while True:
                if p >= n:
                    return 0
                p += 1
                if b[p - 1] == 0:
                    break
    if flg & 2:
        p += 2
    return p if p <= n else 0


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def _table(lens, bits):
    """Direct table of 2^bits entries (symbol << 4 | length, 0 = no code) of the canonical code; None if over-subscribed."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    left, code, nxt = 1, 0, [0] * 16
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            return None
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    tab = np.zeros(1 << bits, dtype=np.int32)
    for s, l in enumerate(lens):
        if l:
            tab[_rev(nxt[l], l)::1 << l] = (s << 4) | l
            nxt[l] += 1
    return tab.tolist()


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, 15), _table([5] * 30, 15))
    return _FIXED


class Window:
    """The compressed bytes of one window, read as bits; nothing behind its last byte exists (zeros)."""

    def __init__(self, data):
        self.d = bytes(data)
        self.end = 8 * len(self.d)

    def peek(self, pos):       # at least 57 bits from bit position pos
        return int.from_bytes(self.d[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)


def read_dynamic_header(w, pos, strict):
    """The header of a dynamic block whose 3 block bits are at pos.  (position behind it, literal/length lengths, distance
    lengths), or None.  strict: the finder's tests (complete codes); otherwise only what the decoder refuses."""
    x = w.peek(pos + 3)
    hlit, hdist, hclen = x & 31, (x >> 5) & 31, (x >> 10) & 15
    if hlit > 29 or hdist > 29:
        return None
    pos += 17
    cl = [0] * 19
    for i in range(hclen + 4):
        cl[ORDER[i]] = (w.peek(pos) & 7)
        pos += 3
    if pos > w.end:
        return None
    kraft = sum(128 >> l for l in cl if l)
    if kraft > 128 or (strict and kraft != 128):
        return None
    ctab = _table(cl, 7)
    n, lens, prev = hlit + 257 + hdist + 1, [], 0
    while len(lens) < n:
        e = ctab[w.peek(pos) & 127]
        if not e:
            return None
        pos += e & 15
        s = e >> 4
        if s < 16:
            lens.append(s)
            prev = s
            continue
        x = w.peek(pos)
        if s == 16:
            if not lens:
                return None
            rep, val = 3 + (x & 3), prev
            pos += 2
        elif s == 17:
            rep, val, prev = 3 + (x & 7), 0, 0
            pos += 3
        else:
            rep, val, prev = 11 + (x & 127), 0, 0
            pos += 7
        if len(lens) + rep > n:
            return None
        lens += [val] * rep
    if pos > w.end:
        return None
    ll, dl = lens[:hlit + 257], lens[hlit + 257:]
    if ll[256] == 0:
        return None
    kl = sum(32768 >> l for l in ll if l)
    kd = sum(32768 >> l for l in dl if l)
    if kl > 32768 or kd > 32768:
        return None
    if strict and (kl != 32768 or not (kd == 32768 or sum(1 for l in dl if l) <= 1)):
        return None
    return pos, ll, dl


def prefilter(data):
    """For every bit offset of data: BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29 and a complete code-length code.
    (bit offsets that pass, ascending; the bits of the code-length code each one needs)"""
    a = np.frombuffer(bytes(data) + b"\0" * 16, dtype=np.uint8)
    bits = np.unpackbits(a, bitorder="little").astype(np.int32)
    n = 8 * len(data)

    def val(off, k):       # the k-bit number at every offset p + off
        v = np.zeros(n, dtype=np.int32)
        for i in range(k):
            v |= bits[off + i:off + i + n] << i
        return v

    ok = (bits[:n] == 0) & (bits[1:n + 1] == 0) & (bits[2:n + 2] == 1)
    ok &= (val(3, 5) <= 29) & (val(8, 5) <= 29)
    p = np.nonzero(ok)[0]
    hclen = np.zeros(len(p), dtype=np.int32)
    for i in range(4):
        hclen |= bits[p + 13 + i] << i
    kraft = np.zeros(len(p), dtype=np.int32)
    for i in range(19):
        q = p + 17 + 3 * i
        q = np.minimum(q, len(bits) - 3)
        v = bits[q] | (bits[q + 1] << 1) | (bits[q + 2] << 2)
        kraft += np.where((i < hclen + 4) & (v > 0), 128 >> v, 0)
    keep = kraft == 128
    return p[keep], 17 + 3 * (hclen[keep] + 4)


def find_start(w, cand, need, lo, hi):
    """The lowest bit offset in [lo, hi) of window w that passes every test of the finder, or -1.  cand / need: prefilter()
    of the window's bytes."""
    i = int(np.searchsorted(cand, lo))
    while i < len(cand) and cand[i] < hi:
        p = int(cand[i])
        if p + int(need[i]) <= w.end and read_dynamic_header(w, p, True) is not None:
            return p
        i += 1
    return -1


def walk(w, start, starts, k, out=None, stop=None, ends=None):
    """Measure (out is None) or decode (out: a list that takes the 16-bit symbols, stop: the end bit measure gave) from the
    block start `start` of chunk k.  Measure returns (m, end bit, bytes, final, bad): m = the later chunk whose start the
    walk's last block end is, or -1."""
    pos, n = start, 0
    last_end, last_n, final, bad, m = start, 0, False, False, -1
    j = k + 1
    base = len(out) if out is not None else 0
    while True:
        if out is not None and pos == stop:
            break
        if pos + 3 > w.end:
            break
        x = w.peek(pos)
        bfinal, btype = x & 1, (x >> 1) & 3
        ok = True
        if btype == 3:
            ok = False
        elif btype == 0:
            p = (pos + 3 + 7) & ~7
            x = w.peek(p)
            ln, nl = x & 0xffff, (x >> 16) & 0xffff
            if p + 32 > w.end:
                break
            if ln ^ 0xffff != nl:
                ok = False
            else:
                p += 32
                if p + 8 * ln > w.end:
                    break
                if out is not None:
                    out.extend(w.d[p >> 3:(p >> 3) + ln])
                n += ln
                pos = p + 8 * ln
        else:
            if btype == 1:
                lt, dt = _fixed()
                pos += 3
            else:
                h = read_dynamic_header(w, pos, False)
                if h is None:
                    ok = False
                else:
                    pos = h[0]
                    lt, dt = _table(h[1], 15), _table(h[2], 15)
            while ok:
                x = w.peek(pos)
                e = lt[x & 0x7fff]
                if not e:
                    ok = False
                    break
                s = e >> 4
                pos += e & 15
                if s < 256:
                    if out is not None:
                        out.append(s)
                    n += 1
                    if pos > w.end:
                        break
                    continue
                if s == 256:
                    break
                if s > 285:
                    ok = False
                    break
                x >>= e & 15
                s -= 257
                ln = LBASE[s] + (x & ((1 << LEXT[s]) - 1))
                x >>= LEXT[s]
                pos += LEXT[s]
                e = dt[x & 0x7fff]
                if not e or (e >> 4) > 29:
                    ok = False
                    break
                ds = e >> 4
                x >>= e & 15
                dist = DBASE[ds] + (x & ((1 << DEXT[ds]) - 1))
                pos += (e & 15) + DEXT[ds]
                if pos > w.end:
                    break
                if out is not None:
                    o = len(out) - base
                    for t in range(ln):
                        sp = o - dist + (t % dist)
                        out.append(out[base + sp] if sp >= 0 else 256 + 32768 + sp)
                n += ln
        if not ok:
            bad = pos + TAIL <= w.end
            break
        if pos > w.end:
            break
        last_end, last_n = pos, n
        if ends is not None:
            ends.append(pos)        # (every block end the walk passes: the tests' list of true block starts)
        if bfinal:
            final = True
            break
        while j < len(starts) and (starts[j] < 0 or starts[j] < pos):
            j += 1
        if j < len(starts) and starts[j] == pos:
            m = j
            break
    if out is not None:
        del out[base + last_n:]
    return m, last_end, last_n, final, bad


class Stream:
    """svdss_gzip_stream_t: the carried state and one run per window."""

    def __init__(self, chunk_bytes, fake=None):
        self.chunk = chunk_bytes
        self.fake = fake
        self.in_member, self.want_trailer = False, False
        self.bit = 0
        self.dict = b""
        self.crc, self.count = 0, 0
        self.stats = dict(windows=0, n_chunks=0, chunks_on_chain=0, chunks_merged=0, false_starts=0, members_finished=0,
                          text_bytes=0)
        self.declined, self.ended, self.error = DECLINE_NONE, False, None
        self.chain_bytes = []         # (per window) the bytes of every chain chunk

    def run(self, comp, is_last):
        """(text, consumed)"""
        comp = bytes(comp)
        p = 0
        if self.want_trailer:
            if len(comp) < 8:
                if is_last:
                    self.error = "truncated trailer"
                return b"", 0
            crc, isize = int.from_bytes(comp[0:4], "little"), int.from_bytes(comp[4:8], "little")
            if crc != self.crc or isize != self.count & 0xffffffff:
                self.error = "CRC32 or ISIZE mismatch"
                return b"", 0
            self.want_trailer, self.in_member = False, False
            self.stats["members_finished"] += 1
            p = 8
        if not self.in_member:
            if p == len(comp) and is_last:
                self.ended = True
                return b"", p
            h = parse_header(comp[p:])
            if h == 0 and not is_last:
                return b"", p
            if h <= 0:
                self.declined = DECLINE_TRAILING if self.stats["members_finished"] else DECLINE_HEADER
                return b"", p
            p += h
            self.in_member, self.bit, self.dict, self.crc, self.count = True, 0, b"", 0, 0
        if p == len(comp) and not is_last:
            return b"", p
        w = Window(comp[p:])
        C = self.chunk
        n = max(1, -(-len(w.d) // C))
        starts = [self.bit] + [-1] * (n - 1)
        if n > 1:
            cand, need = prefilter(w.d)
            for k in range(1, n):
                starts[k] = find_start(w, cand, need, 8 * k * C, min(8 * (k + 1) * C, w.end))
            if all(s < 0 for s in starts[1:]):
                self.declined = DECLINE_NO_START
                return b"", p
            if self.fake is not None and self.fake < n and starts[self.fake] >= 0 and self.fake > 0:
                starts[self.fake] += 1
        res = {0: walk(w, starts[0], starts, 0)}
        chain = [0]
        while res[chain[-1]][0] >= 0:
            k = res[chain[-1]][0]
            res[k] = walk(w, starts[k], starts, k)
            chain.append(k)
        if len(chain) > 1 and res[chain[-1]][1] == starts[chain[-1]]:
            chain.pop()
        last = res[chain[-1]]
        if last[1] == starts[0]:
            self.declined = DECLINE_DAMAGED if last[4] else DECLINE_NO_ADVANCE
            return b"", p
        end_bit = last[1]
        covered = [k for k in range(n) if (starts[k] if starts[k] >= 0 else 8 * k * C) < end_bit]
        st = self.stats
        st["windows"] += 1
        st["n_chunks"] += len(covered)
        st["chunks_on_chain"] += len(chain)
        st["chunks_merged"] += sum(1 for k in covered if k not in chain and starts[k] < 0)
        st["false_starts"] += sum(1 for k in covered if k not in chain and starts[k] >= 0)
        # decode, window, resolve
        d = (b"\0" * 32768 + self.dict)[-32768:]
        text = bytearray()
        per = []
        for k in chain:
            sym = []
            walk(w, starts[k], starts, k, sym, res[k][1])
            assert len(sym) == res[k][2]
            hist = min(32768, self.count + len(text))
            piece = bytearray(len(sym))
            for i, s in enumerate(sym):
                if s >= 256:
                    if s - 256 < 32768 - hist:
                        self.error = "a match reaches in front of the member's first byte"
                        return b"", p
                    s = d[s - 256]
                piece[i] = s
            d = (d + bytes(piece))[-32768:]
            text += piece
            per.append(len(piece))
        self.chain_bytes.append(per)
        self.crc = zlib.crc32(bytes(text), self.crc)
        self.count += len(text)
        self.dict = (self.dict + bytes(text))[-32768:]
        st["text_bytes"] += len(text)
        consumed = p + (end_bit >> 3)
        self.bit = end_bit & 7
        if last[3]:
            self.bit = 0
            self.want_trailer = True
            consumed = p + ((end_bit + 7) >> 3)
        return bytes(text), consumed


def host_tail(s, comp):
    """The host's part behind a decline: comp = the file from the carried byte position on.  The rest of the member from the
    carried bit with the carried dictionary, its trailer against the carried CRC, further members as usual; bytes that are
    no gzip header end the input silently, as gzread does."""
    out = bytearray()
    comp = bytes(comp)
    if s.in_member and not s.want_trailer:
        # (Python's zlib has no inflatePrime, and a stream shifted by the carried bit offset would move the byte boundaries
        # its stored blocks align to: the mirror's own walk reads the rest of the member)
        w = Window(comp)
        sym = []
        m, end, n, final, bad = walk(w, s.bit, [s.bit], 0, sym, None)
        if not final:
            raise zlib.error("invalid code" if bad else "truncated stream")
        d = (b"\0" * 32768 + s.dict)[-32768:]
        hist = min(32768, s.count)
        if any(256 <= x < 256 + 32768 - hist for x in sym):
            raise zlib.error("a match reaches in front of the member's first byte")
        t = bytes(x if x < 256 else d[x - 256] for x in sym)
        out += t
        end = (end + 7) >> 3
        want = zlib.crc32(t, s.crc).to_bytes(4, "little") + ((s.count + len(t)) & 0xffffffff).to_bytes(4, "little")
        if comp[end:end + 8] != want:
            raise zlib.error("CRC32 or ISIZE mismatch")
        comp = comp[end + 8:]
    elif s.want_trailer:
        raise zlib.error("trailer")
    while len(comp) >= 2 and comp[0] == 0x1f and comp[1] == 0x8b:
        z = zlib.decompressobj(31)
        out += z.decompress(comp)
        if not z.eof:
            raise zlib.error("truncated stream")
        comp = z.unused_data
    return bytes(out)


def inflate(data, chunk_bytes, window_bytes, fake=None):
    """The driver of svdss_amd/gzipdev.py over the mirror: (bytes, stream)."""
    data = bytes(data)
    s = Stream(chunk_bytes, fake)
    out = bytearray()
    pos, win = 0, window_bytes
    while True:
        is_last = pos + win >= len(data)
        text, used = s.run(data[pos:pos + win], is_last)
        if s.error:
            raise zlib.error(s.error)
        out += text
        pos += used
        if s.declined:
            s.declined_at = pos
            out += host_tail(s, data[pos:])
            break
        if s.ended:
            break
        if used == 0 and not text:
            if is_last:
                raise zlib.error("truncated stream")
            win *= 2
        else:
            win = window_bytes
    s.device_bytes = s.stats["text_bytes"]
    return bytes(out), s
