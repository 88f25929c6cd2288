"""`search --fastx reads.fastq.gz` (plain single-stream gzip) timed end to end, for profiles/gzip_fastx.txt.

Writes a FASTQ of --text-gb (default 20) gigabytes of text -- the reads of tools/chain_dataset.cpp's kind: seeded 15 kb reads
with 0.5 % errors, qualities 33 + clamp(gauss(40, 12), 2, 60) -- through zlib at levels 1, 6 and 9 as `gzip -1 / -6 / -9`
would write it, builds an index of a seeded reference, and runs `SVDSS search --index ... --fastx ... --verbose` three times
per file, every run under its own time limit: wall seconds, the `fastx: gzip on the device` line and the four kernels'
milliseconds.  With --sweep it also runs this tree's binary once per pair of chunk size (32 KB .. 1 MB) and window size
(64 MB .. 1 GB) on the level-6 file.

    python tools/gzip_fastx_bench.py --bin svdss_amd/SVDSS --out profiles/gzip_fastx.txt --tag "this tree" --device 1 --sweep
    python tools/gzip_fastx_bench.py --bin <parent build>/SVDSS --out profiles/gzip_fastx.txt --tag parent --keep-data DIR

Run it on a build of the parent commit and on this tree, on the same machine, with the same --keep-data directory.  The
rule: the path is on by default only if, on each of the three files, this tree's slowest run beats the parent's fastest.
Measure and decode walk every stream twice: the text states what share of the kernels' time that second walk is."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LINE = re.compile(r"fastx: gzip on the device: .*")
MS = re.compile(r"find/measure/decode/resolve ([\d.]+)/([\d.]+)/([\d.]+)/([\d.]+) ms")


def make_data(d, text_gb, ref_mb, binary):
    from svdss_amd import synth
    if os.path.exists(os.path.join(d, "reads.9.fq.gz")):
        return
    fa = os.path.join(d, "ref.fa")
    ref = synth.make_reference([ref_mb << 20], seed=1)
    with open(fa, "w") as fh:
        fh.write(">chr\n" + synth.to_ascii(ref[0]) + "\n")
    subprocess.run([binary, "index", "-t", "16", "-d", fa, "-o", os.path.join(d, "ref.fmd")], check=True, timeout=1200)
    hap, _ = synth.implant_svs(ref, 64, seed=2, min_len=50, max_len=400)
    rng = np.random.default_rng(5)
    outs = {lv: (open(os.path.join(d, f"reads.{lv}.fq.gz"), "wb"), zlib.compressobj(lv, zlib.DEFLATED, 31)) for lv in (1, 6, 9)}
    written, k, target = 0, 0, int(text_gb * (1 << 30))
    while written < target:
        flat, offs, _ = synth.simulate_reads(hap, 4096, 15000, 0.005, seed=100 + k)
        parts = []
        for i in range(len(offs) - 1):
            seq = synth.to_ascii(flat[offs[i]:offs[i + 1]]).encode()
            q = np.clip(rng.normal(40, 12, size=len(seq)), 2, 60).astype(np.uint8) + 33
            parts.append(b"@read_%d_%d\n" % (k, i) + seq + b"\n+\n" + q.tobytes() + b"\n")
        text = b"".join(parts)
        for fh, z in outs.values():
            fh.write(z.compress(text))
        written += len(text)
        k += 1
    for fh, z in outs.values():
        fh.write(z.flush())
        fh.close()
    with open(os.path.join(d, "text_bytes"), "w") as fh:
        fh.write(str(written))


def run(binary, d, level, env, limit):
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit), binary, "search", "--index", os.path.join(d, "ref.fmd"), "--fastx",
                        os.path.join(d, f"reads.{level}.fq.gz"), "--verbose"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, **env))
    wall = time.time() - t0
    if p.returncode != 0:
        raise SystemExit(f"level {level}: exit {p.returncode}\n{p.stderr[-2000:]}")
    m = LINE.search(p.stderr)
    return wall, (m.group(0) if m else "(host reader)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bin", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--tag", required=True)
    ap.add_argument("--device", type=int, default=None, help="SVDSS_FASTX_GZIP_DEVICE for the runs (unset: the binary's default)")
    ap.add_argument("--text-gb", type=float, default=20.0)
    ap.add_argument("--ref-mb", type=int, default=8)
    ap.add_argument("--keep-data", default=None)
    ap.add_argument("--limit", type=int, default=900, help="seconds per run")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    d = a.keep_data or tempfile.mkdtemp(prefix="gzip_fastx_")
    os.makedirs(d, exist_ok=True)
    make_data(d, a.text_gb, a.ref_mb, a.bin)
    text_bytes = int(open(os.path.join(d, "text_bytes")).read())
    env = {} if a.device is None else {"SVDSS_FASTX_GZIP_DEVICE": str(a.device)}
    lines = [f"## {a.tag}: {a.bin}, {text_bytes / 1e9:.2f} GB of FASTQ text, index of a {a.ref_mb} MB reference, SVDSS_FASTX_GZIP_DEVICE={a.device}"]
    for level in (1, 6, 9):
        size = os.path.getsize(os.path.join(d, f"reads.{level}.fq.gz"))
        for k in range(3):
            wall, line = run(a.bin, d, level, env, a.limit)
            lines.append(f"gzip -{level} ({size / 1e9:.2f} GB) run {k}: {wall:.2f} s wall, {text_bytes / wall / 1e9:.2f} GB/s of text; {line}")
            m = MS.search(line)
            if m:
                f, me, de, re_ = (float(x) for x in m.groups())
                lines.append(f"    kernels {f + me + de + re_:.0f} ms; measure, the first of the two walks over every stream, is "
                             f"{100 * me / (f + me + de + re_):.0f} % of them: what a decoder that stores while it measures would save")
    if a.sweep:
        for chunk_kb in (32, 64, 128, 256, 512, 1024):
            for window_mb in (64, 256, 1024):
                wall, line = run(a.bin, d, 6, dict(env, SVDSS_GZIP_CHUNK_KB=str(chunk_kb), SVDSS_GZIP_WINDOW_MB=str(window_mb)), a.limit)
                lines.append(f"sweep gzip -6 chunk {chunk_kb} KB window {window_mb} MB: {wall:.2f} s wall; {line}")
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
