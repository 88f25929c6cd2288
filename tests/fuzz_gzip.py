"""The chunk-parallel gzip unit (svdss_amd/csrc/gzip_stream.hip, through svdss_amd.gzipdev.inflate) on seeded random gzip
files against gzip.decompress: random texts, levels, strategies, flush points, member cuts, chunk and window sizes.

    python -m tests.fuzz_gzip --minutes 2 --seed 1 [--out DIR]

Outside pytest, like tests/fuzz_fastx.py.  A file the device and zlib read differently is written to DIR and ends the run
with status 1."""
import argparse
import os
import random
import sys
import time
import zlib

from tests import gzip_cases as G


def random_text(rng):
    kind = rng.randrange(6)
    n = rng.choice([0, 1, 100, 5000, 40000, 200000, 600000])
    if kind == 0:
        return G.fastq_text(n, rng.randrange(1 << 20))[:n]
    if kind == 1:
        return G.fasta_text(n, rng.randrange(1 << 20))[:n]
    if kind == 2:
        return bytes(rng.getrandbits(8) for _ in range(min(n, 100000)))
    if kind == 3:
        return bytes([rng.choice(b"ACGT")]) * n
    if kind == 4:
        unit = G.fastq_text(rng.randrange(50, 3000), rng.randrange(1 << 20))
        return (unit * (n // len(unit) + 1))[:n]
    a = G.fastq_text(n // 2, rng.randrange(1 << 20))
    return a + bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 30000))) + a[::-1]


def random_file(rng):
    """(gzip file, text)"""
    parts, texts = [], []
    for _ in range(rng.choice([1, 1, 1, 2, 3])):
        t = random_text(rng)
        level = rng.choice([0, 1, 3, 6, 9])
        strategy = rng.choice([zlib.Z_DEFAULT_STRATEGY] * 3 + [zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED])
        flush_every = rng.choice([None, None, 1000, 30000, 100000])
        flush = rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH])
        header = rng.choice([None, None, G.full_header()])
        parts.append(G.member(t, level, strategy, flush_every, flush, header))
        texts.append(t)
    return b"".join(parts), b"".join(texts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="fuzz_out")
    a = ap.parse_args()
    from svdss_amd import gzipdev
    rng = random.Random(a.seed)
    t_end = time.time() + 60 * a.minutes
    it = device = host = 0
    while time.time() < t_end:
        data, text = random_file(rng)
        chunk = rng.choice([1024, 1500, 4096, 16384, 65536, 1 << 20, 1 << 30])
        window = rng.choice([2048, 30000, 131072, 1 << 20, 1 << 30])
        try:
            out, st = gzipdev.inflate(data, chunk, window)
        except Exception as e:      # noqa: BLE001  (any exception on a valid file is a finding)
            out, st = None, {"error": repr(e)}
        if out != text:
            os.makedirs(a.out, exist_ok=True)
            path = os.path.join(a.out, f"gzip_{a.seed}_{it}.gz")
            with open(path, "wb") as fh:
                fh.write(data)
            print(f"MISMATCH iteration {it}: chunk {chunk}, window {window}, {st}: {path}")
            sys.exit(1)
        device += st["device_bytes"]
        host += st["host_bytes"]
        it += 1
    print(f"fuzz_gzip ok: {it} files, {device} bytes inflated on the device, {host} by the host behind a decline (seed {a.seed})")


if __name__ == "__main__":
    main()
