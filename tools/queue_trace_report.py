#!/usr/bin/env python3
"""What a rocprofv3 --kernel-trace of the pipelined bench says about hardware queues: which streams shared which queue
(the search kernel's among them), and how long the call-side kernels stood ready behind another stream's kernel on their
own queue.
  rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python bench.py --gpus 1 --steps 6 --warmup 2
  python tools/queue_trace_report.py DIR/NAME_kernel_trace.csv

A dispatch is `ready` when the kernel before it on its own stream ends, where that is a memset, a copy kernel or the
first-stage kernel whose output it reads (a call-side kernel is queued right behind those, so that is when it could
start; a kernel that is the first of its call on its stream has no such mark and is left out of the two columns).
`behind` is the part of [ready, start) during which a kernel of ANOTHER stream ran on the same hardware queue; `in-step`
dispatches are those between the first search kernel's start and the last one's end."""
import collections
import csv
import sys

SEARCH = "sfs_search2_kernel"
TARGETS = ("poa_quad_pair_kernel", "poa_quad_kernel", "poa_bundle_kernel", "align_wave_kernel", "lcs_bits_kernel")


def short(name):
    for t in TARGETS + (SEARCH,):
        if t in name:
            return t + (name[name.index(t) + len(t):].split("(")[0] if t == "poa_quad_kernel" else "")
    return name.split("(")[0][:48]


def covered(lo, hi, spans):
    """length of [lo, hi) covered by the union of spans"""
    tot, at = 0, lo
    for a, b in sorted(spans):
        a, b = max(a, at), min(b, hi)
        if b > a:
            tot += b - a
            at = b
    return tot


def main(path):
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append({"q": int(r["Queue_Id"]), "s": int(r["Stream_Id"]), "name": short(r["Kernel_Name"]),
                     "a": int(r["Start_Timestamp"]), "b": int(r["End_Timestamp"])})
    rows.sort(key=lambda r: r["a"])
    queues = collections.defaultdict(lambda: collections.defaultdict(collections.Counter))
    for r in rows:
        queues[r["q"]][r["s"]][r["name"]] += 1
    print(f"{len(rows)} dispatches, {len(queues)} hardware queues, {len({r['s'] for r in rows})} streams")
    search_q = {r["q"] for r in rows if r["name"] == SEARCH}
    for q in sorted(queues):
        print(f"queue {q}{' (the search kernel`s)' if q in search_q else ''}: {len(queues[q])} streams")
        for s in sorted(queues[q]):
            top = ", ".join(f"{n} x{c}" for n, c in queues[q][s].most_common(3))
            print(f"    stream {s}: {top}")
    searches = [(r["a"], r["b"]) for r in rows if r["name"] == SEARCH]
    window = [(min(a for a, _ in searches), max(b for _, b in searches))] if searches else []
    by_stream, by_queue = collections.defaultdict(list), collections.defaultdict(list)
    for r in rows:
        by_stream[r["s"]].append(r)
        by_queue[r["q"]].append(r)
    print("kernel                      where    calls   avg ms   max ms   avg ready->start ms   of it behind another stream on the queue")
    for t in sorted({r["name"] for r in rows if r["name"].startswith(TARGETS)}):
        for where in ("in-step", "alone"):
            durs, waits, behind = [], [], []
            for s, lst in by_stream.items():
                for k, r in enumerate(lst):
                    if r["name"] != t or (covered(r["a"], r["b"], window) > 0) != (where == "in-step"):
                        continue
                    durs.append(r["b"] - r["a"])
                    if k == 0 or not lst[k - 1]["name"].startswith(("__amd_rocclr", "poa_quad")):
                        continue
                    ready = lst[k - 1]["b"]
                    if r["a"] > ready:
                        waits.append(r["a"] - ready)
                        behind.append(covered(ready, r["a"], [(o["a"], o["b"]) for o in by_queue[r["q"]] if o["s"] != s and o["b"] > ready and o["a"] < r["a"]]))
                    else:
                        waits.append(0)
                        behind.append(0)
            if durs:
                print(f"{t:27s} {where:8s} {len(durs):5d} {sum(durs) / len(durs) / 1e6:8.3f} {max(durs) / 1e6:8.3f} "
                      f"{sum(waits) / max(1, len(waits)) / 1e6:12.3f} {sum(behind) / max(1, len(behind)) / 1e6:24.3f}")


if __name__ == "__main__":
    main(sys.argv[1])
