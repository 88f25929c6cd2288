"""csrc/bgzf_pack.h -- the host half of the BGZF batch intake -- on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/bgzf_pack_harness.cpp, a program of its own built from that header alone, checks every
clause of the three rejections with its message (and that the first failing clause wins), and the totals and tables of the
shapes the intake meets -- zero chunks, chunks without members or bytes, members of 0 and 65536 bytes, chunk offsets rounded
up to 16, a base offset -- entry by entry against a recomputation."""
import os
import subprocess

import pytest

from tests.common import ROOT

HARNESS = os.path.join(ROOT, "tests", "_bgzf_pack_harness")
DEPS = [os.path.join(ROOT, "tests", "bgzf_pack_harness.cpp"), os.path.join(ROOT, "svdss_amd", "csrc", "bgzf_pack.h"),
        os.path.join(ROOT, "include", "svdss_hip.h")]


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(HARNESS) or any(os.path.getmtime(d) > os.path.getmtime(HARNESS) for d in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-o", HARNESS, DEPS[0]], check=True)
    return HARNESS


@pytest.mark.parametrize("part,says", [("reject", "reject ok: 15 clauses"), ("tables", "tables ok: 18 shapes")])
def test_bgzf_pack_part(harness, part, says):
    env = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
    p = subprocess.run([harness, part], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and says in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
