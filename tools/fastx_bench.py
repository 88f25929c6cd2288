"""`search --fastx` timed end to end, for profiles/fastx_device.txt.

Writes 65,536 seeded reads x 15 kb with 0.5 % errors as FASTQ with qualities -- once BGZF, once plain -- and a FASTA of the
same reads wrapped at 60, builds an index of a seeded reference (--ref-mb, default 8: a SMALLER index than the bench's
chr20-length one; the text says which), and runs `SVDSS search --index ... --fastx ... --verbose` three times per file,
every run under its own time limit.  Prints wall seconds, reads/s, the --verbose stage lines, the parse kernels'
milliseconds and their bytes over time as a fraction of 8 TB/s (each text byte is read three times and a base written once:
4 bytes moved per text byte is the figure used).

    python tools/fastx_bench.py --bin svdss_amd/SVDSS --out profiles/fastx_device.txt --tag "this tree"
    python tools/fastx_bench.py --bin <parent build>/SVDSS --out profiles/fastx_device.txt --tag parent --keep-data DIR

Run it on a build of the parent commit and on this tree, on the same machine, with the same --keep-data directory."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bgzf_pack(text):
    import struct
    import zlib
    out = []
    for i in list(range(0, len(text), 0xff00)) + [None]:
        p = b"" if i is None else text[i:i + 0xff00]
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        c = z.compress(p) + z.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(c) + 25) + c +
                   struct.pack("<II", zlib.crc32(p), len(p)))
    return b"".join(out)


def make_data(d, n_reads, read_len, ref_mb, binary):
    from svdss_amd import synth
    fa = os.path.join(d, "ref.fa")
    if os.path.exists(os.path.join(d, "reads.fa")):
        return
    ref = synth.make_reference([ref_mb << 20], seed=1)
    with open(fa, "w") as fh:
        fh.write(">chr\n" + synth.to_ascii(ref[0]) + "\n")
    subprocess.run([binary, "index", "-t", "16", "-d", fa, "-o", os.path.join(d, "ref.fmd")], check=True, timeout=1200)
    hap, _ = synth.implant_svs(ref, 64, seed=2, min_len=50, max_len=400)
    flat, offs, _ = synth.simulate_reads(hap, n_reads, read_len, 0.005, seed=3)
    letters = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    fq, fasta = [], []
    for i in range(len(offs) - 1):
        s = letters[flat[offs[i]:offs[i + 1]]].tobytes()
        fq.append(b"@read%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
        fasta.append(b">read%d\n" % i + b"\n".join(s[k:k + 60] for k in range(0, len(s), 60)) + b"\n")
    fq = b"".join(fq)
    open(os.path.join(d, "reads.fq"), "wb").write(fq)
    open(os.path.join(d, "reads.fq.gz"), "wb").write(bgzf_pack(fq))
    open(os.path.join(d, "reads.fa"), "wb").write(b"".join(fasta))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bin", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svdss_amd", "SVDSS"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--read-len", type=int, default=15000)
    ap.add_argument("--ref-mb", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--keep-data", default=None)
    a = ap.parse_args()
    d = a.keep_data or tempfile.mkdtemp(prefix="fastx_bench_")
    os.makedirs(d, exist_ok=True)
    make_data(d, a.reads, a.read_len, a.ref_mb, a.bin)
    lines = [f"== {a.tag}: {a.bin}; {a.reads} reads x {a.read_len}, index of a seeded {a.ref_mb} Mb reference (smaller than the bench's chr20-length one)"]
    for name in ("reads.fq.gz", "reads.fq", "reads.fa"):
        for k in range(a.runs):
            t0 = time.time()
            r = subprocess.run([a.bin, "search", "--index", os.path.join(d, "ref.fmd"), "--fastx", os.path.join(d, name), "--verbose"],
                               stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
            wall = time.time() - t0
            lines.append(f"{name} run {k}: rc {r.returncode}, {wall:.2f} s wall, {a.reads / wall:,.0f} reads/s")
            for l in r.stderr.splitlines():
                if "FASTX device" in l or "stage busy" in l or "records read" in l:
                    lines.append("    " + l.split("] ", 2)[-1])
                m = re.search(r"parse kernels ([0-9.]+) ms over ([0-9]+) text bytes", l)
                if m and float(m.group(1)) > 0:
                    ms, nb = float(m.group(1)), float(m.group(2))
                    lines.append(f"    parse kernels: {ms:.2f} ms, {4 * nb / (ms * 1e-3) / 1e12:.2f} TB/s moved = {4 * nb / (ms * 1e-3) / 8e12:.1%} of 8 TB/s")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
