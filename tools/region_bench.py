"""`SVDSS call` and `SVDSS run` on the whole BAM, on `--region` of its shortest chromosome and of its longest, files in and
files out:

    python tools/region_bench.py [--reads 6176540 --svs 20388] [--work DIR] [--out profiles/region_runs.txt]

builds the data set of bench.py's e2e_chain_30x with tools/chain_dataset.cpp (sorted BAM with its BAI), the index, and the
specific strings `call` is given (smooth > S; search on S > T, once), then runs `call` and `run` three times each in the
three ways, round by round, every GPU step under a time limit of its own and the first failure ending the script.  The
output file holds every wall time and, for the region runs, what --verbose says about the ranges read, the compressed
bytes read and the records gated out; at the end, whether any region run was slower than a whole-file run of its command."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import e2e_call_wg as W  # noqa: E402

BIN = os.path.join(ROOT, "svdss_amd", "SVDSS")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=6_176_540)
    ap.add_argument("--svs", type=int, default=20_388)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a single step may take")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_runs.txt"))
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="region_runs_")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def log(s=""):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    def step(limit, cmd, stdout_path=None):
        full = ["timeout", "-k", "10", str(limit)] + [str(c) for c in cmd]
        t0 = time.perf_counter()
        with open(stdout_path or os.devnull, "wb") as fh:
            r = subprocess.run(full, stdout=fh, stderr=subprocess.PIPE, text=True)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            log(f"FAILED (exit {r.returncode}) after {dt:.2f} s: {' '.join(full)}")
            log(r.stderr[-3000:])
            raise SystemExit(1)
        return dt, r.stderr

    log(f"region_bench: {a.reads} reads, {a.svs} SVs, --threads {a.threads}, {a.runs} runs of each way")
    log("before: loadavg " + open("/proc/loadavg").read().strip())
    t0 = time.perf_counter()
    fa, bam, svs, n, lens, info = W.write_dataset_cxx(work, a.reads, a.svs, threads=a.threads)
    names = [l[1:].split()[0] for l in subprocess.run(["grep", "^>", fa], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(names) == len(lens), (len(names), len(lens))
    short, long_ = names[lens.index(min(lens))], names[lens.index(max(lens))]
    size = os.path.getsize(bam)
    log(f"data set: {n} reads, {len(lens)} references of {sum(lens)} bp, BAM {size} bytes (+ .bai), generated in {time.perf_counter() - t0:.1f} s")
    log(f"shortest reference {short} ({min(lens)} bp), longest {long_} ({max(lens)} bp)")
    fmd = os.path.join(work, "ref.fa.fmd")
    dt, _ = step(a.limit * 3, [BIN, "index", "-t", a.threads, "-d", fa, "-o", fmd])
    log(f"index: {dt:.2f} s")
    T = ["--threads", a.threads]
    S, sfs = os.path.join(work, "S.bam"), os.path.join(work, "T.sfs")
    d1, _ = step(a.limit, [BIN, "smooth", "--reference", fa, "--bam", bam, *T], S)
    d2, _ = step(a.limit, [BIN, "search", "--index", fmd, "--bam", S, *T], sfs)
    log(f"the specific strings of the whole file, for `call`: smooth {d1:.2f} s, search {d2:.2f} s, {os.path.getsize(sfs)} bytes")
    os.remove(S)
    ways = (("whole", []), ("shortest", ["--region", short]), ("longest", ["--region", long_]))
    cmds = {"call": [BIN, "call", "--reference", fa, "--bam", bam, "--sfs", sfs, *T, "--verbose"],
            "run": [BIN, "run", "--reference", fa, "--bam", bam, "--index", fmd, *T, "--verbose"]}
    wall = {(c, w): [] for c in cmds for w, _ in ways}
    keep = re.compile(r"\[regions\]|record store: |older than|not used")
    for i in range(a.runs):
        for c in ("call", "run"):
            for w, opts in ways:
                vcf = os.path.join(work, f"{c}.{w}.vcf")
                d, err = step(a.limit, cmds[c] + opts, vcf)
                wall[(c, w)].append(d)
                rows = sum(1 for l in open(vcf, "rb") if l.strip() and not l.startswith(b"#"))
                log(f"round {i}: {c:4s} {w:8s} {d:7.2f} s wall, {rows} VCF records" + (f", whole file: {size} bytes" if w == "whole" else ""))
                for l in err.splitlines():
                    if keep.search(l):
                        log("    " + l.strip())
    log()
    broken = []
    for c in cmds:
        for w, _ in ways:
            x = wall[(c, w)]
            log(f"{c:4s} {w:8s}: " + ", ".join(f"{v:.2f}" for v in x) + f" s (fastest {min(x):.2f}, slowest {max(x):.2f})")
        for w in ("shortest", "longest"):
            if max(wall[(c, w)]) > min(wall[(c, "whole")]):
                broken.append(f"{c} {w}")
    log("expectation (no region run slower than a whole-file run of the same command): " +
        ("met by every run" if not broken else "BROKEN by " + ", ".join(broken) + " (slowest region run against fastest whole-file run)"))
    log("after: loadavg " + open("/proc/loadavg").read().strip())
    out.close()


if __name__ == "__main__":
    main()
