"""`SVDSS run` against the three-step chain, end to end, files in and files out:

    python tools/run_chain_bench.py --reads 1030000 --svs 3400 --parent-bin /path/to/parent/SVDSS [--work DIR] [--out profiles/run_chain.txt]

builds the data set with tools/chain_dataset.cpp (e2e_chain_wg's scale: 1,030,000 reads / 3,400 SVs; e2e_chain_30x's:
6,176,540 / 20,388), then runs three times each

  (a) smooth > S; search on S > T; call --bam BAM --sfs T            with --parent-bin (a build of the commit before `run`;
                                                                      without it: this tree's binary, and the file says so)
  (b) smooth --index --sfs T --nobam; call --bam BAM --sfs T         this tree
  (c) run                                                            this tree

every GPU step under a time limit of its own, the first failure ending the script.  The output file holds every wall time,
the per-stage seconds of --verbose, the record store's size, whether the three VCFs are the same bytes, and how idle the
machine was (load average, other GPU processes) before and after."""
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


def idle_state():
    """what else the machine is doing: load average and the GPU's busy share (read-only queries)"""
    lines = ["loadavg: " + open("/proc/loadavg").read().strip()]
    try:
        r = subprocess.run(["rocm-smi", "--showuse", "--showmemuse"], capture_output=True, text=True, timeout=30)
        lines += ["rocm-smi: " + l.strip() for l in r.stdout.splitlines() if "GPU[0]" in l]
    except Exception as e:  # noqa: BLE001
        lines.append(f"rocm-smi: not available ({type(e).__name__})")
    return lines


def step(log, limit, cmd, stdout_path=None):
    """one command under `timeout -k 10 limit`; returns (seconds, stderr); a failure ends the script"""
    full = ["timeout", "-k", "10", str(limit)] + [str(c) for c in cmd]
    t0 = time.perf_counter()
    if stdout_path:
        with open(stdout_path, "wb") as fh:
            r = subprocess.run(full, stdout=fh, stderr=subprocess.PIPE, text=True)
    else:
        r = subprocess.run(full, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        log(f"FAILED (exit {r.returncode}) after {dt:.2f} s: {' '.join(full)}")
        log(r.stderr[-3000:])
        raise SystemExit(1)
    return dt, r.stderr


def stage_lines(err):
    keep = re.compile(r"\[(run|call)\] \[time\]|sfs: |device path: |record store: |pass 1 from the records|pass 2 from the records")
    return [l for l in err.splitlines() if keep.search(l)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_030_000)
    ap.add_argument("--svs", type=int, default=3400)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a single step may take")
    ap.add_argument("--parent-bin", default=None, help="the SVDSS binary of the parent commit, for (a)")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "run_chain.txt"))
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="run_chain_")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def log(s=""):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    parent = a.parent_bin or BIN
    log(f"run_chain_bench: {a.reads} reads, {a.svs} SVs, --threads {a.threads}, {a.runs} runs of each")
    log("(a) uses " + (f"the parent commit's binary {os.path.basename(os.path.dirname(parent))}/SVDSS" if a.parent_bin else
                       "THIS tree's binary (no --parent-bin given): not a comparison with the parent commit"))
    for l in idle_state():
        log("before: " + l)
    t0 = time.perf_counter()
    fa, bam, svs, n, lens, info = W.write_dataset_cxx(work, a.reads, a.svs, threads=a.threads)
    log(f"data set: {n} reads, reference {sum(lens)} bp, BAM {os.path.getsize(bam)} bytes, generated in {time.perf_counter() - t0:.1f} s")
    fmd = os.path.join(work, "ref.fa.fmd")
    dt, _ = step(log, a.limit * 4, [BIN, "index", "-t", a.threads, "-d", fa, "-o", fmd])
    log(f"index: {dt:.2f} s")
    T = ["--threads", a.threads]
    S, sfs = os.path.join(work, "S.bam"), os.path.join(work, "T.sfs")
    vcf = {k: os.path.join(work, k + ".vcf") for k in "abc"}
    wall = {k: [] for k in "abc"}
    for i in range(a.runs):
        # (a) three processes, three passes
        t = []
        t.append(step(log, a.limit, [parent, "smooth", "--reference", fa, "--bam", bam, *T], S)[0])
        t.append(step(log, a.limit, [parent, "search", "--index", fmd, "--bam", S, *T], sfs)[0])
        d, err = step(log, a.limit, [parent, "call", "--reference", fa, "--bam", bam, "--sfs", sfs, *T, "--verbose"], vcf["a"])
        t.append(d)
        wall["a"].append(sum(t))
        log(f"(a) run {i}: smooth {t[0]:.2f} + search {t[1]:.2f} + call {t[2]:.2f} = {sum(t):.2f} s")
        for l in stage_lines(err):
            log("    " + l)
        # (b) two processes, two passes
        t = []
        d, err1 = step(log, a.limit, [BIN, "smooth", "--reference", fa, "--bam", bam, "--index", fmd, "--sfs", sfs, "--nobam", *T, "--verbose"])
        t.append(d)
        d, err2 = step(log, a.limit, [BIN, "call", "--reference", fa, "--bam", bam, "--sfs", sfs, *T, "--verbose"], vcf["b"])
        t.append(d)
        wall["b"].append(sum(t))
        log(f"(b) run {i}: smooth --index --sfs --nobam {t[0]:.2f} + call {t[1]:.2f} = {sum(t):.2f} s")
        for l in stage_lines(err1) + stage_lines(err2):
            log("    " + l)
        # (c) one process, one pass
        d, err = step(log, a.limit, [BIN, "run", "--reference", fa, "--bam", bam, "--index", fmd, *T, "--verbose"], vcf["c"])
        wall["c"].append(d)
        log(f"(c) run {i}: run {d:.2f} s")
        for l in stage_lines(err):
            log("    " + l)
        same = [open(vcf[k], "rb").read() for k in "abc"]
        log(f"    cmp of the VCFs: a == b {same[0] == same[1]}, a == c {same[0] == same[2]} ({len(same[0])} bytes, "
            f"{sum(1 for l in same[0].splitlines() if l and not l.startswith(b'#'))} records)")
        if not (same[0] == same[1] == same[2]):
            log("FAILED: the VCFs differ")
            raise SystemExit(1)
    for k, what in (("a", "smooth; search; call"), ("b", "smooth --index --sfs --nobam; call"), ("c", "run")):
        log(f"({k}) {what}: " + ", ".join(f"{x:.2f}" for x in wall[k]) + f" s (fastest {min(wall[k]):.2f}, slowest {max(wall[k]):.2f})")
    log(f"run's slowest run {'beats' if max(wall['c']) < min(wall['a']) else 'does NOT beat'} the fastest run of (a)")
    for l in idle_state():
        log("after: " + l)
    out.close()


if __name__ == "__main__":
    main()
