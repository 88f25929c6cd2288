"""The index of the input BAM (`SVDSS bamindex`, `call / run --write-bam-index`) end to end, files in and files out:

    python tools/bam_index_bench.py --reads 6176540 --svs 20388 --parent-bin /path/to/parent/SVDSS [--work DIR] [--out profiles/bam_input_index.txt]

builds the data set with tools/chain_dataset.cpp (e2e_chain_30x's scale by default; name a smaller one where it does not fit --
the file says which), then runs --runs (3) times each

  (1) call and run                                   with --parent-bin (a build of the parent commit; without it: this tree's
                                                     binary, and the file says that this is no comparison with the parent)
  (2) call and run                                   this tree, without the option
  (3) call and run with --write-bam-index            this tree
  (4) bamindex, and bamindex --gpus 2 oversubscribed this tree
  (5) call --region <shortest chromosome>            with no index beside the BAM, then with the index (4) wrote

every GPU step under a time limit of its own, the first failure ending the script.  What the file says: whether (2) lies inside
the min - max spread of (1); (3) as its difference to (1) beside that spread; (4) beside the seconds of `call`'s pass 1 from its
--verbose line; the compressed bytes (5) read with and without the index, and that its VCFs are the same bytes.  It makes no
comparison with `samtools index`, and seconds on N real GPUs are not measured."""
import argparse
import os
import re
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import e2e_call_wg as W  # noqa: E402
from tools.run_chain_bench import BIN, idle_state, stage_lines, step  # noqa: E402


def spread(xs):
    return f"{min(xs):.2f} - {max(xs):.2f} s (" + ", ".join(f"{x:.2f}" for x in xs) + ")"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=6_176_540)
    ap.add_argument("--svs", type=int, default=20_388)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds a single step may take")
    ap.add_argument("--parent-bin", default=None, help="the SVDSS binary of the parent commit, for (1)")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_input_index.txt"))
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="bam_index_")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def log(s=""):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    parent = a.parent_bin or BIN
    log(f"bam_index_bench: {a.reads} reads, {a.svs} SVs, --threads {a.threads}, {a.runs} runs of each")
    log("(1) uses " + ("the parent commit's binary" if a.parent_bin else "THIS tree's binary (no --parent-bin given): not a comparison with the parent commit"))
    for l in idle_state():
        log("before: " + l)
    t0 = time.perf_counter()
    fa, bam, svs, n, lens, info = W.write_dataset_cxx(work, a.reads, a.svs, threads=a.threads)
    log(f"data set: {n} reads, reference {sum(lens)} bp in {len(lens)} chromosomes, BAM {os.path.getsize(bam)} bytes, generated in {time.perf_counter() - t0:.1f} s")
    fmd, sfs = os.path.join(work, "ref.fa.fmd"), os.path.join(work, "T.sfs")
    dt, _ = step(log, a.limit * 4, [BIN, "index", "-t", a.threads, "-d", fa, "-o", fmd])
    log(f"index: {dt:.2f} s")
    T = ["--threads", a.threads]
    call = ["call", "--reference", fa, "--bam", bam, "--sfs", sfs, *T, "--verbose"]
    run = ["run", "--reference", fa, "--bam", bam, "--index", fmd, *T, "--verbose"]
    step(log, a.limit * 2, [BIN, *run, "--sfs", sfs], os.path.join(work, "first.vcf"))      # (the SFS file `call` reads)
    wall = {}
    pass1 = []
    vcfs = {}
    for tag, binary, extra in (("1", parent, ()), ("2", BIN, ()), ("3", BIN, ("--write-bam-index",))):
        for cmd_name, cmd in (("call", call), ("run", run)):
            key = f"({tag}) {cmd_name}"
            wall[key] = []
            for i in range(a.runs):
                idx = os.path.join(work, f"{cmd_name}{tag}.bai")
                opt = [extra[0], idx] if extra else []
                vcf = os.path.join(work, f"{cmd_name}{tag}.vcf")
                d, err = step(log, a.limit, [binary, *cmd, *opt], vcf)
                wall[key].append(d)
                log(f"{key} run {i}: {d:.2f} s")
                for l in stage_lines(err):
                    log("    " + l)
                    m = re.search(r"pass 1: placement\s+([0-9.]+) s", l)
                    if m and cmd_name == "call" and tag == "2":
                        pass1.append(float(m.group(1)))
                vcfs[key] = open(vcf, "rb").read()
    for cmd_name in ("call", "run"):
        ref = wall[f"(1) {cmd_name}"]
        same = vcfs[f"(1) {cmd_name}"] == vcfs[f"(2) {cmd_name}"] == vcfs[f"(3) {cmd_name}"]
        log(f"{cmd_name}: (1) {spread(ref)}; (2) {spread(wall[f'(2) {cmd_name}'])}: "
            f"{'inside' if min(ref) <= min(wall[f'(2) {cmd_name}']) and max(wall[f'(2) {cmd_name}']) <= max(ref) else 'NOT inside'} the spread of (1); "
            f"(3) {spread(wall[f'(3) {cmd_name}'])}: fastest {min(wall[f'(3) {cmd_name}']) - min(ref):+.2f} s, slowest {max(wall[f'(3) {cmd_name}']) - max(ref):+.2f} s "
            f"against (1); the VCFs are {'the same bytes' if same else 'DIFFERENT'}")
        if not same:
            raise SystemExit(1)
    # (4) bamindex alone
    idx = bam + ".bai"
    for key, extra, env in (("(4) bamindex", (), None), ("(4) bamindex --gpus 2 (oversubscribed)", ("--gpus", "2"), {"SVDSS_GPUS_OVERSUBSCRIBE": "1"})):
        wall[key] = []
        for i in range(a.runs):
            if env:
                os.environ.update(env)
            d, err = step(log, a.limit, [BIN, "bamindex", "--bam", bam, "-o", os.path.join(work, "alone.bai"), *extra, "--verbose"])
            for k in (env or {}):
                os.environ.pop(k, None)
            wall[key].append(d)
            log(f"{key} run {i}: {d:.2f} s")
            for l in err.splitlines():
                if l.startswith("[bamindex]"):
                    log("    " + l)
        log(f"{key}: {spread(wall[key])}" + (f"; call's pass 1 (placement included): {spread(pass1)}" if pass1 else ""))
    same = open(os.path.join(work, "alone.bai"), "rb").read() == open(os.path.join(work, "call3.bai"), "rb").read() == open(os.path.join(work, "run3.bai"), "rb").read()
    log(f"the index of bamindex, of call and of run: {'the same bytes' if same else 'DIFFERENT'}")
    # (5) a region with and without the index
    short = min(range(len(lens)), key=lambda t: lens[t])
    names = [l.split()[0][1:] for l in open(fa) if l.startswith(">")]
    region = ["--region", names[short]]
    if os.path.exists(idx):
        os.remove(idx)
    got = {}
    for key in ("no index", "with the index"):
        if key == "with the index":
            shutil.copy(os.path.join(work, "alone.bai"), idx)
        wall[key] = []
        for i in range(a.runs):
            vcf = os.path.join(work, "region.vcf")
            d, err = step(log, a.limit, [BIN, *call, *region], vcf)
            wall[key].append(d)
            m = re.search(r"(\d+) compressed bytes read", err)
            log(f"(5) call --region {names[short]}, {key}, run {i}: {d:.2f} s, {m.group(1) if m else '?'} compressed bytes read")
        got[key] = open(vcf, "rb").read()
        log(f"(5) {key}: {spread(wall[key])}")
    log(f"(5) the VCFs are {'the same bytes' if got['no index'] == got['with the index'] else 'DIFFERENT'}")
    for l in idle_state():
        log("after: " + l)
    out.close()


if __name__ == "__main__":
    main()
