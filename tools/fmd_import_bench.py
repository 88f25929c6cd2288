#!/usr/bin/env python3
"""Writes profiles/fmd_import.txt: what it costs to get the records out of an `.fmd` that has no sidecar -- an index of
upstream `SVDSS index` / ropebwt3 -- by the serial LF walk per string (csrc/rld0.cpp), by the marked walks on the host
and on the GPU (csrc/bwt_invert.h, bwt_invert.hip), and what `search --index` of that file takes with either.

    python tools/fmd_import_bench.py [--bases 3100000000] [--records 48] [--parent-bin <SVDSS of the parent commit>]
                                     [--strides 1024,4096,16384] [--runs 3] [--skip-host] [--out profiles/fmd_import.txt]

The index is written by this tree's `SVDSS index` from an iid ACGT reference of --bases bases in --records records
(default: GRCh38's length) and its sidecar removed.  Then:
  1. svdss_bwt_strings alone on the BWT of that file: the serial walk, the host's marked walks, and the device's at every
     stride, with lane refill and as a plain grid -- milliseconds of the rank blocks' build, pass 1 and pass 2;
  2. whether the recovered records are the reference's, and rebuild (imported by the device walk) to the same acc;
  3. `search --index` of the file, --runs times each: the parent's binary (--parent-bin; without it the line says so), this
     tree with SVDSS_FMD_IMPORT_DEVICE=0 (the parent's route) and with SVDSS_FMD_IMPORT_DEVICE=1.
DESIGN section 4j says how the file decides the defaults.  At the default size this is also the one test of rows beyond 2^32."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import svdss_amd  # noqa: E402
from svdss_amd._lib import lib  # noqa: E402

BIN = os.path.join(ROOT, "svdss_amd", "SVDSS")


def write_reference(path, bases, records, seed):
    """iid ACGT, `records` records of decreasing length, lines of 60; returns the records' lengths"""
    rng = np.random.default_rng(seed)
    weights = np.array([1.0 / (i + 2) for i in range(records)])
    lens = np.maximum(60, (bases * weights / weights.sum()).astype(np.int64) // 60 * 60)
    letters = np.frombuffer(b"ACGT", np.uint8)
    with open(path, "wb") as fh:
        for i, n in enumerate(lens.tolist()):
            fh.write(f">r{i + 1}\n".encode())
            for s in range(0, n, 60 << 20):
                e = min(n, s + (60 << 20))
                rows = letters[rng.integers(0, 4, size=e - s, dtype=np.uint8)].reshape(-1, 60)
                fh.write(np.concatenate([rows, np.full((len(rows), 1), 10, np.uint8)], axis=1).tobytes())
    return lens


def walk(bwt, m, device, stride, env):
    """one svdss_bwt_strings; (seconds, last-call report, lengths, flat strings)"""
    for k, v in env.items():
        os.environ[k] = v
    n = len(bwt)
    out = np.empty(n - m, np.uint8)
    lens = np.zeros(m, np.int64)
    k = C.c_int32(0)
    t0 = time.perf_counter()
    rc = lib.svdss_bwt_strings(bwt.ctypes.data, n, device, stride, out.ctypes.data, n - m, lens.ctypes.data, m, C.byref(k))
    dt = time.perf_counter() - t0
    for k_ in env:
        del os.environ[k_]
    if rc != 0:
        raise SystemExit(f"svdss_bwt_strings(device={device}, stride={stride}): status {rc}")
    return dt, svdss_amd.bwt_strings_last(), lens, out


def timed(cmd, env):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stderr.decode()[-2000:]}")
    return dt, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=3_100_000_000)
    ap.add_argument("--records", type=int, default=48)
    ap.add_argument("--parent-bin", default="")
    ap.add_argument("--strides", default="1024,4096,16384")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true", help="leave the two host walks out (minutes at a human genome's length)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmd_import.txt"))
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    lines = [f"fmd_import_bench: {a.bases} bases in {a.records} records (iid ACGT), runs {a.runs}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        fa, fmd, fq = os.path.join(d, "ref.fa"), os.path.join(d, "ref.fmd"), os.path.join(d, "reads.fq")
        rec_lens = write_reference(fa, a.bases, a.records, seed=1)
        dt, _ = timed([BIN, "index", "-t", "16", "-d", fa, "-o", fmd], dict(os.environ))
        say(f"SVDSS index: {dt:.2f} s; .fmd {os.path.getsize(fmd)} bytes, sidecar {os.path.getsize(fmd + '.svdss')} bytes (removed)")
        want = svdss_amd.FMDIndex.load(fmd)
        want_acc, want_n = want.acc.copy(), want.size
        want.close()
        os.remove(fmd + ".svdss")
        n = C.c_int64()
        assert lib.svdss_fmd_read_bwt(fmd.encode(), None, 0, C.byref(n)) == 0
        bwt = np.empty(n.value, np.uint8)
        t0 = time.perf_counter()
        assert lib.svdss_fmd_read_bwt(fmd.encode(), bwt.ctypes.data, n.value, C.byref(n)) == 0
        m = int((bwt == 0).sum())
        say(f"rld0 decoded: {n.value} rows ({'beyond' if n.value >= 1 << 32 else 'below'} 2^32), {m} strings, {time.perf_counter() - t0:.2f} s")
        say("")
        say("1. svdss_bwt_strings alone (wall seconds of the call; ms of the rank blocks' build / pass 1 / pass 2)")
        ref = None
        if not a.skip_host:
            dt, last, ref_lens, ref = walk(bwt, m, -1, -1, {})
            say(f"   host, serial walk per string:            {dt:8.3f} s   (walks {last['pass1_ms']:.0f} ms)")
            dt, last, lens_, out = walk(bwt, m, -1, 0, {})
            say(f"   host, marked walks, stride {last['stride']:6d}:       {dt:8.3f} s   blocks {last['blocks_ms']:.0f} / {last['pass1_ms']:.0f} / {last['pass2_ms']:.0f} ms"
                f"   same strings: {bool((lens_ == ref_lens).all() and (out == ref).all())}")
        for stride in [int(s) for s in a.strides.split(",")]:
            for refill in ("1", "0"):
                for run in range(a.runs):
                    dt, last, lens_, out = walk(bwt, m, 0, stride, {"SVDSS_INVERT_REFILL": refill})
                    same = "" if ref is None else f"   same strings: {bool((lens_ == ref_lens).all() and (out == ref).all())}"
                    say(f"   device ({last['route']}), stride {stride:6d}, {'refill' if refill == '1' else 'plain '}, run {run + 1}: {dt:8.3f} s   "
                        f"blocks {last['blocks_ms']:.2f} / {last['pass1_ms']:.2f} / {last['pass2_ms']:.2f} ms, {last['walkers']} walkers{same}")
        if ref is None:
            ref_lens, ref = lens_, out
        say("")
        # 2. the records: every record of the reference and its reverse complement, by length; the rebuild's acc
        got_lens = np.sort(ref_lens)
        say(f"2. recovered strings' lengths are the records' (each twice): {bool((got_lens == np.sort(np.repeat(rec_lens, 2))).all())}")
        del bwt, ref, out
        os.environ["SVDSS_FMD_IMPORT_DEVICE"] = "1"
        t0 = time.perf_counter()
        again = svdss_amd.FMDIndex.load(fmd)                # the import: decode, device walk, pick strands, rebuild
        say(f"   imported by the device walk and rebuilt in {time.perf_counter() - t0:.2f} s: size {again.size} (want {want_n}), "
            f"acc equal: {bool((again.acc == want_acc).all())}")
        again.close()
        del os.environ["SVDSS_FMD_IMPORT_DEVICE"]
        say("")
        # 3. search --index of the file
        with open(fq, "w") as fh:
            rng = np.random.default_rng(2)
            for i in range(1000):
                fh.write(f"@r{i}\n{''.join(rng.choice(list('ACGT'), size=200))}\n+\n{'I' * 200}\n")
        say(f"3. search --index <that .fmd> --fastx <1000 reads>, wall seconds, {a.runs} runs each")
        texts = []
        routes = [("this tree, SVDSS_FMD_IMPORT_DEVICE=0 (the serial host walk)", BIN, {"SVDSS_FMD_IMPORT_DEVICE": "0"}),
                  ("this tree, SVDSS_FMD_IMPORT_DEVICE=1 (the device walk)     ", BIN, {"SVDSS_FMD_IMPORT_DEVICE": "1"})]
        if a.parent_bin:
            routes.insert(0, ("the parent commit's binary                              ", a.parent_bin, {}))
        else:
            say("   the parent commit's binary: NOT RUN (no --parent-bin)")
        for name, exe, env in routes:
            ts = []
            for _ in range(a.runs):
                dt, text = timed([exe, "search", "--index", fmd, "--fastx", fq, "--threads", "16"], dict(os.environ, **env))
                ts.append(dt)
                texts.append(text)
            say(f"   {name}: " + "  ".join(f"{t:.2f}" for t in ts))
        say(f"   every run wrote the same text: {all(t == texts[0] for t in texts)}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
