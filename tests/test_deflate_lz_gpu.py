"""The GPU encoder's second mode (csrc/deflate.hip, svdss_bgzf_deflate_mode, mode 1 "lz"): literals, runs and general
matches -- what a coordinate-sorted BAM repeats from one overlapping read to the next.  The output is held to the
standard the way mode 0's is: every member inflates on its own (zlib, libdeflate where present, csrc/inflate.hip) to the
bytes that went in; no match reaches in front of its member; on overlapping reads it is smaller than mode 0 and within
1.08 x zlib level 1; on data without repeats it costs header bits at most; mode 0 is svdss_bgzf_deflate byte for byte."""
import gzip
import io
import struct
import zlib

import numpy as np
import pytest

from svdss_amd.bgzf import bgzf_blocks, gpu_deflate, gpu_inflate

pytestmark = pytest.mark.gpu
B = 0xff00
LZ = 1


def members(stream):
    """[(raw deflate bytes, crc, isize, member length)] of a BGZF stream, by the SAM specification's layout"""
    out, pos = [], 0
    while pos < len(stream):
        assert stream[pos:pos + 4] == b"\x1f\x8b\x08\x04"
        xlen, = struct.unpack_from("<H", stream, pos + 10)
        assert xlen == 6 and stream[pos + 12:pos + 16] == b"BC\x02\x00"
        bsize, = struct.unpack_from("<H", stream, pos + 16)
        crc, isize = struct.unpack_from("<II", stream, pos + bsize + 1 - 8)
        out.append((stream[pos + 18:pos + bsize + 1 - 8], crc, isize, bsize + 1))
        pos += bsize + 1
    assert pos == len(stream)
    return out


def _libdeflate_inflate(raw, isize):
    """libdeflate's inflater through ctypes (stricter than zlib about incomplete codes), or None when the shared library
    is not on the machine"""
    import ctypes as C
    for name in ("libdeflate.so.0", "libdeflate.so"):
        try:
            lib = C.CDLL(name)
        except OSError:
            continue
        lib.libdeflate_alloc_decompressor.restype = C.c_void_p
        lib.libdeflate_deflate_decompress.restype = C.c_int
        lib.libdeflate_deflate_decompress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.libdeflate_free_decompressor.argtypes = [C.c_void_p]
        d = lib.libdeflate_alloc_decompressor()
        out = C.create_string_buffer(max(isize, 1))
        got = C.c_size_t()
        rc = lib.libdeflate_deflate_decompress(d, raw, len(raw), out, isize, C.byref(got))
        lib.libdeflate_free_decompressor(d)
        assert rc == 0, rc
        return out.raw[:got.value]
    return None


def check_roundtrip(data, block_bytes=B, every=1, **kw):
    """every member of gpu_deflate(data, mode=1) inflates ON ITS OWN to its block, under each inflater"""
    data = bytes(data)
    stream = gpu_deflate(data, block_bytes, mode=LZ, **kw)
    ms = members(stream)
    assert len(ms) == (len(data) + block_bytes - 1) // block_bytes
    for i, (raw, crc, isize, mlen) in enumerate(ms):
        want = data[i * block_bytes:(i + 1) * block_bytes]
        d = zlib.decompressobj(-15)                      # a fresh inflater: nothing of the members in front of this one
        got = d.decompress(raw) + d.flush()
        assert d.eof and d.unused_data == b""
        assert got == want, (i, len(got), len(want))
        if i % every == 0:
            ld = _libdeflate_inflate(raw, len(want))
            assert ld is None or ld == want, i
        assert isize == len(want) and crc == zlib.crc32(want) & 0xffffffff
        assert mlen <= 65536
    assert gzip.GzipFile(fileobj=io.BytesIO(stream)).read() == data
    blocks = bgzf_blocks(stream)
    assert bytes(gpu_inflate(stream, [(c, l, i) for c, l, i, _ in blocks])) == data
    return stream, ms


def overlapping_reads(n_bytes, err, seed=5):
    """BAM records of 12-16 kb reads cut from a random 400 kb reference, start positions advancing by a uniform 1..1000,
    4-bit packed bases, absent qualities, substitution errors at rate err; n_bytes of them at least (the walk starts over
    at the reference's end, like the next contig)"""
    rng = np.random.default_rng(seed)
    G = 400000
    ref = rng.integers(0, 4, G).astype(np.uint8)
    code = np.array([1, 2, 4, 8], np.uint8)
    out, pos, i, total = [], 0, 0, 0
    while total < n_bytes:
        L = int(rng.integers(12000, 16000))
        if pos + L > G:
            pos = 0
        s = ref[pos:pos + L].copy()
        if err > 0:
            m = rng.random(L) < err
            s[m] = (s[m] + rng.integers(1, 4, int(m.sum()))) % 4
        c = code[s]
        if L % 2:
            c = np.append(c, 0)
        packed = (c[0::2] << 4 | c[1::2]).astype(np.uint8).tobytes()
        name = b"read%07d\0" % i
        core = struct.pack("<iiBBHHHIiii", 0, pos, len(name), 60, 4681, 1, 0, L, -1, -1, 0)
        body = core + name + struct.pack("<I", L << 4) + packed + b"\xff" * L
        out.append(struct.pack("<I", len(body)) + body)
        total += len(out[-1])
        pos += int(rng.integers(1, 1001))
        i += 1
    return b"".join(out)


def records_without_overlap():
    """test_deflate_gpu.test_many_blocks...'s records: random bases and qualities, names; 300 blocks and 777 bytes"""
    rng = np.random.default_rng(8)
    rec = []
    while sum(len(r) for r in rec) < 300 * B + 777:
        l = int(rng.integers(9000, 16000))
        rec.append(b"read%07d\0" % len(rec) + bytes(rng.choice([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28], size=l // 2).astype(np.uint8))
                   + bytes(rng.integers(25, 50, size=l, dtype=np.uint8)))
    return b"".join(rec)[:300 * B + 777]


def test_any_inflater_reads_every_kind_of_block():
    rng = np.random.default_rng(7)
    fib = [1, 1]
    while len(fib) < 32:
        fib.append(fib[-1] + fib[-2])
    half = bytes(rng.integers(0, 256, size=B // 2, dtype=np.uint8))
    unit = bytes(rng.integers(0, 256, size=300, dtype=np.uint8))
    cases = {
        "one byte": b"x",
        "two bytes": b"ab",
        "all the same": bytes([9]) * B,
        "random (stored)": bytes(rng.integers(0, 256, size=B, dtype=np.uint8)),
        "packed bases": bytes(rng.choice([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88],
                                         size=50000).astype(np.uint8)),
        "qualities": bytes(rng.integers(20, 60, size=B, dtype=np.uint8)),
        "binned qualities": bytes(np.array([3, 10, 17, 22, 27, 33, 40], np.uint8)[rng.integers(0, 7, size=40000)]),
        "skewed (geometric)": bytes(np.minimum(255, rng.geometric(0.03, size=B)).astype(np.uint8)),
        "code lengths past 15 bits": b"".join(bytes([i]) * min(c, 9000) for i, c in enumerate(fib))[:B],
        "text": (b"@SQ\tSN:chr1\tLN:248956422\n" * 4000)[:B],
        "quarter boundaries": bytes(range(256)) * 3 + b"z",
        "exactly 0xff00": bytes(rng.integers(60, 70, size=B, dtype=np.uint8)),
        "short last block": bytes(rng.integers(60, 70, size=B + 777, dtype=np.uint8)),
        "second half repeats the first (distance 32,640)": half + half,
        "period 3": (b"abc" * 22000)[:B],
        "period 7": (b"ACGTTGA" * 9400)[:B],
        "period 300": (unit * 220)[:B],
    }
    for name, data in cases.items():
        stream, ms = check_roundtrip(data)
        if name in ("packed bases", "binned qualities", "all the same", "text"):
            assert len(stream) < 0.62 * len(data), (name, len(stream), len(data))
        if name == "random (stored)":
            assert len(data) < len(stream) <= len(data) + 26 + 6 * 4
        if name.startswith("second half"):
            assert len(stream) < 0.55 * len(data), (name, len(stream))       # the second half is matches
        if name.startswith("period"):
            # the first 2,048 positions have nothing to look up (at most a byte each), then a match per lane's slice of
            # 256 bytes (about 4 bytes), four headers of under 200 bytes: 4 KB of 65 KB, with a margin
            assert len(stream) < 0.12 * len(data), (name, len(stream))
    for n in (3, 63, 64, 65, 255, 256, 257, 1019, 1020, 1021, 4 * 16320 - 1, B - 1):
        check_roundtrip(bytes(rng.integers(60, 70, size=n, dtype=np.uint8)))
    # runs as mode 0 takes them, other block sizes, the library's own back-to-back output
    check_roundtrip(b"a" + bytes([7]) * 16319 + bytes([7]) * 5 + b"b" * 16315 + b"b" * 16320 + b"c" * 3)
    for n in (1, 2, 3, 4, 5, 257, 258, 259, 260, 261, 262, 263, 516, 517, 1000):
        check_roundtrip(b"q" + bytes([1]) * n + b"r")
    data = overlapping_reads(200000, 0.001)
    check_roundtrip(data, block_bytes=4096)
    check_roundtrip(data[:70001], block_bytes=333)
    assert gpu_deflate(data, mode=LZ, dense=True) == gpu_deflate(data, mode=LZ)


def test_no_match_leaves_its_member():
    rng = np.random.default_rng(12)
    block = overlapping_reads(B, 0.0, seed=9)[:B - 2000] + bytes(rng.integers(0, 256, size=2000, dtype=np.uint8))
    assert len(block) == B
    stream, ms = check_roundtrip(block + block)          # (each member inflated by a fresh inflater there)
    assert len(ms) == 2
    # identical input, independent streams: the second member has nothing more to copy from than the first (the two
    # BGZF headers and footers are the same 26 bytes, so the difference allowed is zero)
    assert ms[1][3] >= ms[0][3], (ms[0][3], ms[1][3])


@pytest.mark.parametrize("err", [0.0, 0.001])
def test_overlapping_reads_compress(err):
    data = overlapping_reads(16 << 20, err)
    assert len(data) >= 16 << 20
    lz = gpu_deflate(data, mode=LZ)
    runs = gpu_deflate(data, mode=0)
    z1 = sum(len(zlib.compress(data[i:i + B], 1)) - 6 + 26 for i in range(0, len(data), B))   # raw deflate + the container
    print("err %g: bytes out per byte in: lz %.4f runs %.4f zlib-1 %.4f" % (err, len(lz) / len(data), len(runs) / len(data), z1 / len(data)))
    assert gzip.GzipFile(fileobj=io.BytesIO(lz)).read() == data
    assert len(lz) < len(runs), (len(lz), len(runs))
    if err == 0.0:
        assert len(lz) < 1.08 * z1, (len(lz), z1)
    # mode 0 is svdss_bgzf_deflate itself, strided and dense
    part = data[:40 * B + 123]
    assert runs == gpu_deflate(data)
    assert gpu_deflate(part, mode=0, dense=True) == gpu_deflate(part, dense=True) == gpu_deflate(part)


def test_no_regression_without_repeats_and_mode_0_is_todays_encoder():
    data = records_without_overlap()
    n_blocks = (len(data) + B - 1) // B
    lz, _ = check_roundtrip(data, every=7)
    runs = gpu_deflate(data)
    print("no overlap: lz %d runs %d (%+d bytes over %d blocks)" % (len(lz), len(runs), len(lz) - len(runs), n_blocks))
    assert len(lz) <= len(runs) + 64 * n_blocks, (len(lz), len(runs))
    assert gpu_deflate(data, mode=0) == runs
    assert gpu_deflate(data, mode=0, dense=True) == gpu_deflate(data, dense=True) == runs
