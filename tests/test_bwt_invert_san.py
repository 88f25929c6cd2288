"""The host driver of csrc/bwt_invert.h -- the walker arithmetic, the step, the store packer and the chaining that the GPU
kernels of csrc/bwt_invert.hip share -- under AddressSanitizer and UndefinedBehaviorSanitizer on the CPU:
tests/bwt_invert_harness.cpp is a program of its own that inverts generated collections at every stride into buffers that
end where their heap block ends.  A byte stored outside a walker's segment, a misaligned word store or an overflow in the
row arithmetic is a failure."""
import os
import subprocess

import pytest

from tests.common import ROOT

HARNESS = os.path.join(ROOT, "tests", "_bwt_invert_harness")
CSRC = os.path.join(ROOT, "svdss_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "bwt_invert_harness.cpp"), os.path.join(CSRC, "rld0.cpp"), os.path.join(CSRC, "index_build.cpp")]
DEPS = SRC + [os.path.join(CSRC, h) for h in ("bwt_invert.h", "fmd_layout.h", "rld0.h", "index_host.h")]


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(HARNESS) or any(os.path.getmtime(d) > os.path.getmtime(HARNESS) for d in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fopenmp", "-pthread", "-o", HARNESS] + SRC + ["-lz", "-ldl"], check=True)
    return HARNESS


@pytest.mark.parametrize("seed", [1, 2])
def test_host_driver_under_sanitizers(harness, seed):
    env = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1",
               OMP_NUM_THREADS="2")
    p = subprocess.run([harness, str(seed)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and p.stdout.startswith("ok: "), f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
