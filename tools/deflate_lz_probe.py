"""Kernel time and output size of the GPU deflate's two modes (csrc/deflate.hip; `smooth --compress runs|lz`) on 300
blocks of the overlapping-read data and of the no-overlap records of tests/test_deflate_lz_gpu.py: svdss_deflate_kernel_ms
(HIP events around the kernels: in lz mode the match finder and the coder together), one warm call, then REPEATS calls
per mode, alternating.  Usage: python tools/deflate_lz_probe.py [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from svdss_amd.bgzf import gpu_deflate  # noqa: E402
from tests.test_deflate_lz_gpu import B, overlapping_reads, records_without_overlap  # noqa: E402

REPEATS = 7


def main():
    lines = []
    for name, data in (("overlapping reads, no errors", overlapping_reads(300 * B, 0.0)[:300 * B]),
                       ("overlapping reads, 0.1 % errors", overlapping_reads(300 * B, 0.001)[:300 * B]),
                       ("records without overlap", records_without_overlap()[:300 * B])):
        ms = {0: [], 1: []}
        size = {}
        for mode in (0, 1):
            gpu_deflate(data, mode=mode)
        for _ in range(REPEATS):
            for mode in (0, 1):
                out, st = gpu_deflate(data, mode=mode, return_stats=True)
                ms[mode].append(st["kernel_ms"])
                size[mode] = len(out)
        for mode, tag in ((0, "runs"), (1, "lz")):
            t = sorted(ms[mode])
            med = t[len(t) // 2]
            lines.append("%-32s %-4s %8d bytes in %8d out (%.4f)  kernel ms median %.3f min %.3f max %.3f  %.1f GB/s in" % (
                name, tag, len(data), size[mode], size[mode] / len(data), med, t[0], t[-1], len(data) / med / 1e6))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
