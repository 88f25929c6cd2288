#!/usr/bin/env python3
"""Writes profiles/fmd_encode.txt: what `SVDSS index` takes with the rld0 `.fmd` encoded on the host (csrc/rld0.cpp) and on
the device (csrc/rld0_dev.hip), against the parent commit's binary.

    python tools/fmd_encode_bench.py --parent-bin <SVDSS of the parent commit> [--sizes 3100000000,400000000] [--records 48]
                                     [--runs 3] [--out profiles/fmd_encode.txt]

For every size an iid ACGT reference of that many bases in --records records (the reference of tools/fmd_import_bench.py:
3.1 Gb / 48 records is GRCh38's length) is written, then `SVDSS index --verbose -t 16 -d REF -o OUT` runs --runs times each
as (a) the parent's binary, (b) this tree with SVDSS_FMD_ENCODE_DEVICE=0 and (c) this tree with SVDSS_FMD_ENCODE_DEVICE=1,
alternating a, b, c, a, b, c, ...: wall seconds, the `fmd:` line of --verbose (the encoder's stage milliseconds), and
`cmp` of the three `.fmd` files at full size.

The rule the file decides: the device encoder becomes the default for an unset
SVDSS_FMD_ENCODE_DEVICE only if, on BOTH references, its slowest run beats the parent's fastest; the last line says which.
Without --parent-bin the file says so and decides nothing.  A run that ends with a non-zero status or runs into its time
limit ends the tool: what was collected is written, marked undecided, and no further program is started on the GPU."""
import argparse
import filecmp
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.fmd_import_bench import write_reference  # noqa: E402

BIN = os.path.join(ROOT, "svdss_amd", "SVDSS")
KNOBS = ("SVDSS_FMD_ENCODE_DEVICE", "SVDSS_INDEX_CPU", "SVDSS_FMD_TILE_RUNS", "SVDSS_FMD_DECLINE_SYMS", "SVDSS_FMD_SLICE_WORDS", "SVDSS_FMD_GRID_BLOCKS", "SVDSS_FMD_SCAN_ITEMS", "SVDSS_FMD_HBM_LIMIT_MB")


class Stopped(Exception):
    """an `SVDSS index` that failed or ran into its time limit: nothing more is started on the GPU after it"""


def one(binary, ref, out, device):
    """(wall seconds, the fmd: line) of one `SVDSS index`; Stopped for a run that failed or did not end in time"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    if device is not None:
        env["SVDSS_FMD_ENCODE_DEVICE"] = str(device)
    for p in (out, out + ".svdss"):
        if os.path.exists(p):
            os.remove(p)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([binary, "index", "--verbose", "-t", "16", "-d", ref, "-o", out], capture_output=True, env=env, timeout=1100)
    except subprocess.TimeoutExpired:
        raise Stopped("ran into its time limit of 1100 s")
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise Stopped(f"ended with status {r.returncode}: {r.stderr.decode(errors='replace')[-500:].strip()}")
    line = [l for l in r.stderr.decode().splitlines() if l.startswith("fmd: ")]
    return dt, line[0] if line else "(no fmd: line: a binary from before the device encoder)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", default="")
    ap.add_argument("--sizes", default="3100000000,400000000")
    ap.add_argument("--records", type=int, default=48)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmd_encode.txt"))
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    lines = []

    def say(line):   # (printed as it comes: a run at GRCh38's length is minutes of silence otherwise)
        lines.append(line)
        print(line, flush=True)

    say("fmd_encode_bench: `SVDSS index --verbose -t 16 -d REF -o OUT`, wall seconds; " + time.strftime("%Y-%m-%d"))
    forms = [("parent", a.parent_bin, None), ("tree, host encoder (SVDSS_FMD_ENCODE_DEVICE=0)", BIN, 0), ("tree, device encoder (SVDSS_FMD_ENCODE_DEVICE=1)", BIN, 1)]
    if not a.parent_bin:
        say("no --parent-bin: the parent commit's binary was NOT run; nothing is decided by this file")
        forms = forms[1:]
    wins = []
    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        for size in [int(x) for x in a.sizes.split(",")]:
            ref = os.path.join(tmp, f"ref_{size}.fa")
            write_reference(ref, size, a.records, seed=11)
            say(f"\nreference: {size} bases in {a.records} records (iid ACGT)")
            secs = {name: [] for name, _, _ in forms}
            for run in range(a.runs):
                for k, (name, binary, device) in enumerate(forms):
                    try:
                        dt, note = one(binary, ref, os.path.join(tmp, f"out{k}.fmd"), device)
                    except Stopped as e:
                        # what was collected is kept, nothing is decided, and NOTHING more is started on the GPU: a fault
                        # or an abort leaves the card in a state no further program should meet
                        say(f"  run {run + 1} {name}: FAILED, {e}")
                        say("\nstopped at the first run that failed: no further run was started; undecided, "
                            "NO -> the device encoder stays opt-in")
                        with open(a.out, "w") as fh:
                            fh.write("\n".join(lines) + "\n")
                        raise SystemExit(f"{name}: {e}")
                    secs[name].append(dt)
                    if os.path.exists(os.path.join(tmp, f"out{k}.fmd.svdss")):
                        os.remove(os.path.join(tmp, f"out{k}.fmd.svdss"))   # (gigabytes each; only the .fmd files are compared)
                    say(f"  run {run + 1} {name}: {dt:.2f} s   {note}")
            outs = [os.path.join(tmp, f"out{k}.fmd") for k in range(len(forms))]
            same = all(os.path.exists(p) for p in outs) and all(filecmp.cmp(outs[0], p, shallow=False) for p in outs[1:])
            say(f"  cmp of the {len(outs)} .fmd files ({os.path.getsize(outs[0]) if os.path.exists(outs[0]) else 0} bytes): {'identical' if same else 'DIFFERENT'}")
            if not same:
                for k in range(1, len(outs)):
                    if all(os.path.exists(p) for p in (outs[0], outs[k])):
                        say(f"    {forms[0][0]} | {forms[k][0]}: {'identical' if filecmp.cmp(outs[0], outs[k], shallow=False) else 'DIFFERENT'}")
            for name, _, _ in forms:
                if secs[name]:
                    say(f"  {name}: fastest {min(secs[name]):.2f} s, slowest {max(secs[name]):.2f} s of {len(secs[name])}")
            if a.parent_bin and secs[forms[0][0]] and len(secs[forms[2][0]]) == a.runs:
                wins.append(same and max(secs[forms[2][0]]) < min(secs[forms[0][0]]))
            else:
                wins.append(False)
            os.remove(ref)
    if a.parent_bin:
        say("\nrule: the device encoder's slowest run beats the parent's fastest on every reference, and the files are identical: "
            + ("YES -> the device encoder may be the default" if wins and all(wins) else "NO -> the device encoder stays opt-in"))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
