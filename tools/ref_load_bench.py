"""The reference FASTA read on the GPU (csrc/ref_stream.hip, csrc/ref_loader.h) end to end, files in and files out:

    python tools/ref_load_bench.py --parent-bin /path/to/parent/SVDSS [--commands index,smooth,call,run] [--scale 1.0]
                                   [--reads 200000 --svs 700] [--wrap 60] [--work DIR] [--out profiles/ref_device_load.txt]

builds the data set with tools/chain_dataset.cpp (GRCh38 lengths at --scale 1: 3.09 Gb, offsets beyond 2^31), wraps its
FASTA at --wrap columns, writes it a second time as BGZF -- with the repo's own writer, svdss_amd.bgzf.gpu_deflate -- and a third time as plain gzip,
then runs --runs (3) times each, for every command named,

  (a) the BGZF file      with --parent-bin (a build of the parent commit; without it THIS tree with SVDSS_REF_DEVICE=0, and
                         the file says that this is no comparison with the parent)
  (b) the BGZF file      this tree
  (c) the plain file     this tree, default (the mapped reader) and SVDSS_REF_DEVICE=2 (slabs on the device)
  (d) the gzip file      this tree, once (the line reader; the --verbose hint)

every step under a time limit of its own, the first failure ending the script.  What the file says per command: wall
seconds, the seconds until the reference is usable where the command prints them (smooth: SVDSS_DEBUG's `reference read
in`), the --verbose line of the device loader with its inflate and parse kernel milliseconds, the parse kernels' GB/s of
text against the 8 TB/s of the README, whether (b)'s slowest run beats (a)'s fastest, and that all outputs of a command
are the same bytes.  A command that is not named is not measured, and the file says so."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import e2e_call_wg as W  # noqa: E402
from tools.run_chain_bench import BIN, idle_state, step  # noqa: E402

LINE = re.compile(r"reference: (\d+) batches on the device, (\d+) records, (\d+) bases \(inflate kernels ([\d.]+) ms, parse kernels ([\d.]+) ms\)")
READ_IN = re.compile(r"reference read in ([\d.]+) s")


def spread(xs):
    return f"{min(xs):.2f} - {max(xs):.2f} s (" + ", ".join(f"{x:.2f}" for x in xs) + ")"


def write_bgzf(src, dst, piece=255 * 0xff00):
    """the repo's own BGZF writer (the GPU encoder), piece by piece, and the EOF member"""
    from svdss_amd.bgzf import gpu_deflate
    with open(src, "rb") as f, open(dst, "wb") as g:
        while True:
            data = f.read(piece)
            if not data:
                break
            g.write(gpu_deflate(data, dense=True))
        g.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def wrap_fasta(src, dst, width):
    """the generator writes a chromosome on one line; references are kept at 60 columns"""
    import numpy as np
    with open(src, "rb") as f, open(dst, "wb") as g:
        for line in f:
            if line.startswith(b">"):
                g.write(line)
                continue
            s = np.frombuffer(line.rstrip(b"\n"), np.uint8)
            n = len(s) // width * width
            body = np.empty((n // width, width + 1), np.uint8)
            body[:, :width] = s[:n].reshape(-1, width)
            body[:, width] = 10
            g.write(body.tobytes())
            if n < len(s):
                g.write(s[n:].tobytes() + b"\n")


def digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--svs", type=int, default=700)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--wrap", type=int, default=60, help="columns of the FASTA's sequence lines (0: one line per chromosome, as generated)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--commands", default="index,smooth,call,run")
    ap.add_argument("--limit", type=int, default=600, help="seconds a single step may take")
    ap.add_argument("--parent-bin", default=None, help="the SVDSS binary of the parent commit, for (a)")
    ap.add_argument("--no-gzip", action="store_true", help="leave (d) out")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_device_load.txt"))
    a = ap.parse_args()
    commands = [c for c in a.commands.split(",") if c]
    work = a.work or tempfile.mkdtemp(prefix="ref_load_")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def log(s=""):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    log(f"ref_load_bench: --scale {a.scale}, {a.reads} reads, {a.svs} SVs, --threads {a.threads}, {a.runs} runs of each; commands: {', '.join(commands)}")
    left_out = [c for c in ("index", "smooth", "call", "run") if c not in commands]
    if left_out:
        log("NOT measured in this run: " + ", ".join(left_out))
    log("(a) uses " + ("the parent commit's binary" if a.parent_bin else "THIS tree's binary with SVDSS_REF_DEVICE=0 (no --parent-bin given): not a comparison with the parent commit"))
    for l in idle_state():
        log("before: " + l)
    t0 = time.perf_counter()
    fa, bam, _, n, lens, _ = W.write_dataset_cxx(work, a.reads, a.svs, scale=a.scale, threads=a.threads)
    if a.wrap > 0:
        wrap_fasta(fa, os.path.join(work, "ref.wrap.fa"), a.wrap)
        os.remove(fa)
        fa = os.path.join(work, "ref.wrap.fa")
    text_bytes = os.path.getsize(fa)
    log(f"data set: {n} reads, reference {sum(lens)} bp in {len(lens)} chromosomes ({text_bytes} bytes of FASTA), generated in {time.perf_counter() - t0:.1f} s")
    files = {"plain": fa, "bgzf": os.path.join(work, "ref.bgzf.fa.gz"), "gzip": os.path.join(work, "ref.gzip.fa.gz")}
    t0 = time.perf_counter()
    write_bgzf(fa, files["bgzf"])
    log(f"BGZF by the repo's writer: {os.path.getsize(files['bgzf'])} bytes in {time.perf_counter() - t0:.1f} s")
    if not a.no_gzip:
        t0 = time.perf_counter()
        with open(files["gzip"], "wb") as g:
            subprocess.run(["gzip", "-1", "-c", fa], stdout=g, check=True)
        log(f"plain gzip: {os.path.getsize(files['gzip'])} bytes in {time.perf_counter() - t0:.1f} s")
    T = ["--threads", a.threads]
    fmd, sfs = os.path.join(work, "ref.fa.fmd"), os.path.join(work, "T.sfs")
    if any(c in commands for c in ("call", "run")):
        dt, _ = step(log, a.limit * 4, [BIN, "index", "-t", a.threads, "-d", fa, "-o", fmd])
        log(f"(setup) index of the plain file: {dt:.2f} s")
        step(log, a.limit * 2, [BIN, "run", "--reference", fa, "--bam", bam, "--index", fmd, *T, "--sfs", sfs], os.path.join(work, "setup.vcf"))

    def command(name, ref, tag):
        """(argv behind the binary, the files whose bytes are the command's output)"""
        o = os.path.join(work, f"{name}.{tag}")
        if name == "index":
            return ["index", "--verbose", "-t", a.threads, "-d", ref, "-o", o + ".fmd"], None, [o + ".fmd", o + ".fmd.svdss"]
        if name == "smooth":
            return ["smooth", "--reference", ref, "--bam", bam, *T, "--verbose"], o + ".bam", [o + ".bam"]
        if name == "call":
            return ["call", "--reference", ref, "--bam", bam, "--sfs", sfs, *T, "--verbose", "--clusters", o + ".clusters"], o + ".vcf", [o + ".vcf", o + ".clusters"]
        return (["run", "--reference", ref, "--bam", bam, "--index", fmd, *T, "--verbose", "--sfs", o + ".sfs", "--clusters", o + ".clusters"], o + ".vcf",
                [o + ".vcf", o + ".sfs", o + ".clusters"])

    parent = a.parent_bin or BIN
    variants = [("(a) BGZF, parent", parent, "bgzf", {} if a.parent_bin else {"SVDSS_REF_DEVICE": "0"}, a.runs),
                ("(b) BGZF, this tree", BIN, "bgzf", {}, a.runs),
                ("(c) plain, this tree, mapped reader", BIN, "plain", {}, a.runs),
                ("(c) plain, this tree, SVDSS_REF_DEVICE=2", BIN, "plain", {"SVDSS_REF_DEVICE": "2"}, a.runs)]
    if not a.no_gzip:
        variants.append(("(d) gzip, this tree", BIN, "gzip", {}, 1))
    verdicts = []
    for name in commands:
        wall, sums = {}, {}
        for k, (key, binary, kind, env, runs) in enumerate(variants):
            argv, stdout_path, outs = command(name, files[kind], str(k))
            wall[key] = []
            for i in range(runs):
                os.environ["SVDSS_DEBUG"] = "1"
                os.environ.update(env)
                d, err = step(log, a.limit, [binary, *argv], stdout_path)
                for e in list(env) + ["SVDSS_DEBUG"]:
                    os.environ.pop(e, None)
                wall[key].append(d)
                notes = []
                m = READ_IN.search(err)
                if m:
                    notes.append(f"reference usable after {m.group(1)} s")
                m = LINE.search(err)
                if m:
                    ms = float(m.group(5))
                    notes.append(f"{m.group(1)} batches, inflate kernels {m.group(4)} ms, parse kernels {m.group(5)} ms = {text_bytes / ms / 1e6:.1f} GB/s of text "
                                 f"({100 * text_bytes / ms / 1e6 / 8000:.1f} % of 8 TB/s)")
                if "bgzip it to have it read on the GPU" in err:
                    notes.append("said: bgzip it")
                log(f"{name} {key} run {i}: {d:.2f} s" + ("; " + "; ".join(notes) if notes else ""))
            sums[key] = [digest(p) for p in outs]
            log(f"{name} {key}: {spread(wall[key])}")
        same = len({tuple(s) for s in sums.values()}) == 1
        log(f"{name}: the outputs of all variants are {'the same bytes' if same else 'DIFFERENT'}")
        pa, tb = wall[variants[0][0]], wall[variants[1][0]]
        beats = max(tb) < min(pa)
        verdicts.append((name, beats))
        log(f"{name}: BGZF, this tree's slowest run {max(tb):.2f} s {'beats' if beats else 'DOES NOT beat'} the parent's fastest {min(pa):.2f} s")
        if not same:
            raise SystemExit(1)
    for l in idle_state():
        log("after: " + l)
    log("acceptance (DESIGN 7 item 0a's rule): " + "; ".join(f"{n}: {'device loader by default' if b else 'keeps the host reader by default'}" for n, b in verdicts))
    out.close()


if __name__ == "__main__":
    main()
