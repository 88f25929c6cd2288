"""csrc/gzip_stream.h on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: tests/gzip_host_harness.cpp, a program
of its own, checks the gzip member header (every FLG combination, cut after every byte), gz_crc32_combine against zlib's
crc32 of the concatenation, and the zlib hand-over (inflatePrime + inflateSetDictionary) at block ends of every bit offset."""
import os
import subprocess

import pytest

from tests.common import ROOT

HARNESS = os.path.join(ROOT, "tests", "_gzip_host_harness")
DEPS = [os.path.join(ROOT, "tests", "gzip_host_harness.cpp"), os.path.join(ROOT, "svdss_amd", "csrc", "gzip_stream.h")]


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(HARNESS) or any(os.path.getmtime(d) > os.path.getmtime(HARNESS) for d in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-o", HARNESS, DEPS[0], "-lz"], check=True)
    return HARNESS


@pytest.mark.parametrize("part,says", [("headers", "headers ok: 32 FLG combinations"), ("combine", "combine ok"), ("resume", "resume ok")])
def test_gzip_host_part(harness, part, says):
    env = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
    p = subprocess.run([harness, part], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and says in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    if part == "resume":
        assert "every bit offset" in p.stdout
