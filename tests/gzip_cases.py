"""Inputs of the plain-gzip tests (tests/test_gzip_stream_mirror.py, test_gzip_stream_gpu.py, test_fastx_gzip_gpu.py,
fuzz_gzip.py): FASTQ-shaped text and the gzip files made of it.  Everything is built once per process and never changed."""
import functools
import gzip
import random
import struct
import zlib


def fastq_text(n_bytes, seed):
    """Reads of 800 to 3,000 random ACGT, qualities 33 + clamp(gauss(40, 12), 2, 60), names of about 30 bytes."""
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        n = rng.randint(800, 3000)
        seq = "".join(rng.choices("ACGT", k=n))
        qual = "".join(chr(33 + min(60, max(2, int(rng.gauss(40, 12))))) for _ in range(n))
        rec = f"@m64011_{seed:03d}/{rng.randrange(10 ** 8):08d}/ccs_{i}\n{seq}\n+\n{qual}\n"
        out.append(rec)
        size += len(rec)
        i += 1
    return "".join(out).encode()


def fasta_text(n_bytes, seed):
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        n = rng.randint(800, 3000)
        seq = "".join(rng.choices("ACGT", k=n))
        rec = f">read_{seed}_{i} len={n}\n" + "\n".join(seq[k:k + 60] for k in range(0, n, 60)) + "\n"
        out.append(rec)
        size += len(rec)
        i += 1
    return "".join(out).encode()


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None, flush=zlib.Z_FULL_FLUSH, header=None):
    """One gzip member around a raw deflate stream of `text`."""
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_every:
        body = b"".join(z.compress(text[i:i + flush_every]) + z.flush(flush) for i in range(0, len(text), flush_every)) + z.flush()
    else:
        body = z.compress(text) + z.flush()
    return wrap(body, text, header)


PLAIN_HEADER = b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03"


def full_header():
    """FEXTRA + FNAME + FCOMMENT + FHCRC"""
    h = b"\x1f\x8b\x08" + bytes([4 | 8 | 16 | 2]) + b"\0\0\0\0\x00\x03" + struct.pack("<H", 6) + b"AB\x02\x00xy" + b"reads.fq\0" + b"a comment\0"
    return h + struct.pack("<H", zlib.crc32(h) & 0xffff)


def wrap(body, text, header=None):
    return (header or PLAIN_HEADER) + body + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


def mixed_member(text):
    """Level 6 / stored / level 6 joined at full flushes under one hand-made header and trailer."""
    a, b = len(text) // 3, 2 * len(text) // 3
    z1 = zlib.compressobj(6, zlib.DEFLATED, -15)
    p1 = z1.compress(text[:a]) + z1.flush(zlib.Z_FULL_FLUSH)
    z2 = zlib.compressobj(0, zlib.DEFLATED, -15)
    p2 = z2.compress(text[a:b]) + z2.flush(zlib.Z_FULL_FLUSH)
    z3 = zlib.compressobj(6, zlib.DEFLATED, -15)
    p3 = z3.compress(text[b:]) + z3.flush()
    return wrap(p1 + p2 + p3, text)


@functools.lru_cache(maxsize=None)
def fastq(n_bytes=1_500_000, seed=11):
    return fastq_text(n_bytes, seed)


@functools.lru_cache(maxsize=None)
def case(name):
    """(gzip file, the text gzip.decompress gives for it)"""
    fq = fastq()
    small = fq[:300_000]
    rnd = random.Random(5)
    if name in ("fastq1", "fastq6", "fastq9"):
        data = member(fq, int(name[-1]))
    elif name == "fasta":
        t = fasta_text(600_000, 12)
        return member(t), t
    elif name == "repeat":
        # (a sync flush every 50 copies: the ~15 KB this compresses to would otherwise be ONE block, with no seam in it)
        one = fastq_text(2500, 13)
        t = one * 500
        return member(t, flush_every=50 * len(one), flush=zlib.Z_SYNC_FLUSH), t
    elif name == "run":
        t = small[:100_000] + b"A" * 200_000 + small[100_000:200_000]
        return member(t), t
    elif name == "level0":
        data = member(small, 0)
        return data, small
    elif name == "fixed":
        data = member(small, 6, zlib.Z_FIXED)
        return data, small
    elif name == "fullflush":
        t = fq[:700_000]
        return member(t, 6, flush_every=100_000, flush=zlib.Z_FULL_FLUSH), t
    elif name == "syncflush":
        t = fq[:700_000]
        return member(t, 6, flush_every=100_000, flush=zlib.Z_SYNC_FLUSH), t
    elif name == "mixed":
        t = fq[:900_000]
        return mixed_member(t), t
    elif name == "random":
        t = fq[:300_000] + bytes(rnd.getrandbits(8) for _ in range(200_000)) + fq[300_000:600_000]
        return member(t), t
    elif name in ("text1", "text100", "text40000", "empty"):
        n = {"text1": 1, "text100": 100, "text40000": 40000, "empty": 0}[name]
        t = fq[:n]
        return member(t), t
    elif name == "members2":
        a, b = fq[:250_000], fq[250_000:520_000]
        return member(a) + member(b, 1), a + b
    elif name == "members3":
        a, b, c = fq[:200_000], fq[200_000:200_100], fq[200_100:500_000]
        return member(a, 9) + member(b) + member(c), a + b + c
    elif name == "header":
        t = fq[:400_000]
        return member(t, header=full_header()), t
    elif name == "garbage":
        t = fq[:400_000]
        return member(t) + b"not a gzip header at all" * 3, t
    else:
        raise KeyError(name)
    assert gzip.decompress(data) == fq
    return data, fq


ALL = ("fastq1", "fastq6", "fastq9", "fasta", "repeat", "run", "level0", "fixed", "fullflush", "syncflush", "mixed", "random",
       "text1", "text100", "text40000", "empty", "members2", "members3", "header", "garbage")


def damaged(kind):
    """A gzip file that must end in an error: a flipped bit in the middle, or a wrong CRC32."""
    data, _ = case("fastq6")
    b = bytearray(data)
    if kind == "bitflip":
        b[len(b) // 2] ^= 0x10
    elif kind == "crc":
        b[-8] ^= 0xff
    elif kind == "truncated":
        del b[len(b) * 2 // 3:]
    else:
        raise KeyError(kind)
    return bytes(b)
