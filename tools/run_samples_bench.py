"""A list of three samples, two ways, files in and files out:

    python tools/run_samples_bench.py --parent-bin /path/to/parent/SVDSS [--sets 6176540:20388,1030000:3400] [--work DIR]
                                      [--out profiles/run_samples.txt]

  (a) three `SVDSS run --bam` after each other                       with --parent-bin (a build of the commit before
                                                                      `--samples`; without it: this tree's binary, and the
                                                                      file says so)
  (b) one `SVDSS run --samples LIST`                                 this tree

For every data set (READS:SVS of tools/chain_dataset.cpp; the first default is bench.py's e2e_chain_30x, the second its 5x
sibling) the same BAM stands three times in the list under three output names -- the page cache is warm for both ways --,
each way runs three times, round by round, on the whole file and with --region on the shortest chromosome, every GPU step
under a time limit of its own and the first failure ending the script.  The output file holds the wall seconds of every way
and of every sample, the --verbose stage lines of samples 1 and 2 of (b) side by side, the load average, whether the three
VCFs of (b) equal those of (a), and the claim: the slowest (b) against the fastest (a)."""
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
KEEP = re.compile(r"\[run\] \[time\]|\[run\] (reference|index):|\[run\] record store|\[run\] sample \d+ of|sfs: ")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", default="6176540:20388,1030000:3400")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a single step may take")
    ap.add_argument("--parent-bin", default=None, help="the SVDSS binary of the parent commit, for (a)")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "run_samples.txt"))
    a = ap.parse_args()
    work0 = a.work or tempfile.mkdtemp(prefix="run_samples_")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def log(s=""):
        print(s, flush=True)
        out.write(s.replace(work0, "<work>") + "\n")
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

    parent = a.parent_bin or BIN
    log(f"run_samples_bench: three samples per list, --threads {a.threads}, {a.runs} runs of each way")
    log("(a) uses " + (f"the parent commit's binary {os.path.basename(os.path.dirname(parent))}/SVDSS" if a.parent_bin else
                       "THIS tree's binary (no --parent-bin given): not a comparison with the parent commit"))
    log("before: loadavg " + open("/proc/loadavg").read().strip())
    verdicts = []
    for spec in a.sets.split(","):
        reads, svs_n = (int(x) for x in spec.split(":"))
        work = os.path.join(work0, f"set{reads}")
        os.makedirs(work, exist_ok=True)
        t0 = time.perf_counter()
        fa, bam, svs, n, lens, info = W.write_dataset_cxx(work, reads, svs_n, threads=a.threads)
        names = [l[1:].split()[0] for l in subprocess.run(["grep", "^>", fa], capture_output=True, text=True, check=True).stdout.splitlines()]
        short = names[lens.index(min(lens))]
        log()
        log(f"==== data set: {n} reads, {svs_n} SVs, {len(lens)} references of {sum(lens)} bp, BAM {os.path.getsize(bam)} bytes (+ .bai), generated in "
            f"{time.perf_counter() - t0:.1f} s; shortest reference {short} ({min(lens)} bp)")
        fmd = os.path.join(work, "ref.fa.fmd")
        dt, _ = step(a.limit * 3, [BIN, "index", "-t", a.threads, "-d", fa, "-o", fmd])
        log(f"index: {dt:.2f} s")
        T = ["--threads", a.threads, "--verbose"]
        for what, opts in (("whole file", []), ("--region " + short, ["--region", short])):
            tag = "whole" if not opts else "region"
            vcf = {w: [os.path.join(work, f"{tag}.{w}{k}.vcf") for k in range(3)] for w in "ab"}
            lst = os.path.join(work, f"{tag}.list.txt")
            with open(lst, "w") as fh:
                fh.write("# the same BAM three times\n" + "".join(f"{bam}\t{v}\n" for v in vcf["b"]))
            wall = {"a": [], "b": []}
            for i in range(a.runs):
                per = [step(a.limit, [parent, "run", "--reference", fa, "--bam", bam, "--index", fmd, *T, *opts], v)[0] for v in vcf["a"]]
                wall["a"].append(sum(per))
                log(f"{what}, round {i}: (a) {sum(per):7.2f} s wall = " + " + ".join(f"{x:.2f}" for x in per) + " (three processes)")
                d, err = step(3 * a.limit, [BIN, "run", "--reference", fa, "--samples", lst, "--index", fmd, *T, *opts])
                wall["b"].append(d)
                per_b = re.findall(r"^\[run\] sample \d+: .* VCF record\(s\), ([\d.]+) s$", err, re.M)
                log(f"{what}, round {i}: (b) {d:7.2f} s wall, samples " + " + ".join(per_b) + " (one process; the rest: start, refusals, exit)")
                if i == 0:
                    cuts = [m.start() for m in re.finditer(r"^\[run\] sample \d+ of \d+: ", err, re.M)] + [len(err)]
                    parts = [[l.strip() for l in err[x:y].splitlines() if KEEP.search(l)] for x, y in zip(cuts, cuts[1:])]
                    log("    --verbose of (b), sample 1 | sample 2:")
                    for k in range(max(len(parts[0]), len(parts[1]))):
                        l1 = parts[0][k] if k < len(parts[0]) else ""
                        l2 = parts[1][k] if k < len(parts[1]) else ""
                        log(f"    {l1[:150]:150s} | {l2[:150]}")
                    same = all(open(x, "rb").read() == open(y, "rb").read() for x, y in zip(vcf["a"], vcf["b"]))
                    rows = sum(1 for l in open(vcf["b"][0], "rb") if l.strip() and not l.startswith(b"#"))
                    log(f"    the three VCFs of (b) {'equal' if same else 'DIFFER FROM'} those of (a); {rows} VCF records each")
                    if not same:
                        raise SystemExit(1)
            for w in "ab":
                log(f"{what}: ({w}) " + ", ".join(f"{v:.2f}" for v in wall[w]) + f" s (fastest {min(wall[w]):.2f}, slowest {max(wall[w]):.2f})")
            holds = max(wall["b"]) < min(wall["a"])
            verdicts.append(holds)
            log(f"{what}: the slowest --samples run ({max(wall['b']):.2f} s) is {'FASTER' if holds else 'NOT faster'} than the fastest loop of (a) "
                f"({min(wall['a']):.2f} s)")
    log()
    log("claim (the slowest --samples run is faster than the fastest loop of (a), on every data set and way): " + ("HOLDS" if all(verdicts) else "DOES NOT HOLD"))
    log("after: loadavg " + open("/proc/loadavg").read().strip())
    out.close()


if __name__ == "__main__":
    main()
