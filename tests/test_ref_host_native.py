"""The host-only parts of the device reference loader (svdss_amd/csrc/host_common.h header_order, csrc/ref_pieces.h), built
as a stand-alone program with -fsanitize=address,undefined (tests/native/ref_host.cpp) and held against Python."""
import os
import subprocess

import numpy as np
import pytest

from tests.common import ROOT

SRC = os.path.join(ROOT, "tests", "native", "ref_host.cpp")
EXE = os.path.join(ROOT, "tests", "native", "_ref_host")
CSRC = os.path.join(ROOT, "svdss_amd", "csrc")


@pytest.fixture(scope="module")
def exe():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("host_common.h", "ref_pieces.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, SRC], check=True)
    return EXE


def run(exe, header, fasta, seg_lens, ranges):
    r = subprocess.run([exe, " ".join(n or "-" for n in header), " ".join(n or "-" for n in fasta), " ".join(map(str, seg_lens)),
                        " ".join(f"{a}:{b}" for a, b in ranges)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode().splitlines()


def test_header_order_and_pieces(exe):
    rng = np.random.default_rng(8)
    for _ in range(30):
        pool = ["chr%d" % k for k in range(8)] + [""]
        fasta = [pool[i] for i in rng.permutation(len(pool))[:int(rng.integers(0, len(pool) + 1))]]
        header = [pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(0, 12)))]          # (a name may occur twice)
        seg_lens = [int(x) for x in rng.choice([0, 1, 2, 16, 100, 4096], size=int(rng.integers(0, 9)))]
        total = sum(seg_lens)
        ranges = [tuple(sorted(int(x) for x in rng.integers(0, total + 1, size=2))) for _ in range(6)] + [(0, total), (total, total), (0, total + 1)]
        out = run(exe, header, fasta, seg_lens, ranges)
        order = [t for t, n in enumerate(header) if n in fasta]
        tid_map = [order.index(t) if n in fasta else -1 for t, n in enumerate(header)]
        assert out[0].split()[1:] == [str(t) for t in order]
        assert out[1].split()[1:] == [str(t) for t in tid_map]
        starts = np.cumsum([0] + [n for n in seg_lens if n > 0])
        for line, (a, b) in zip(out[2:], ranges):
            want = "uncovered" if b > total else "ok"
            pieces = sum(1 for s, e in zip(starts[:-1], starts[1:]) if max(a, s) < min(b, e))
            assert line == f"range {a}:{b} {want} pieces {pieces if want == 'ok' else line.split()[-1]}", (line, seg_lens)
