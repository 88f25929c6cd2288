"""csrc/bam_aux_walk.h -- the one step through a BAM aux block that set_xf (smooth_host.cpp), the XF walk of
smooth_walk_kernel (bam_smooth.hip) and both aux_int (bam_reader.h, bam_device_internal.h) share -- on the CPU under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/aux_walk_harness.cpp, a program of its own built from that header
alone, against values written out there.  Every scalar type; Z / H with and without terminator; B arrays of every subtype
with counts 0, 1, exactly fitting, one byte too long, 0x7fffffff, -1, -2 and INT32_MIN; an unknown type; a block that ends
after 1, 2 and 3 bytes of a tag; a truncated value of every type; XF first / middle / last and behind an XF:Z.  A walk
that does not advance (the parent's did not, on a negative B count) never returns: the timeout shows it.

And the same through the CLI's host code (SVDSS_SMOOTH_HOST=1, no GPU needed): a record with a B array of count -2 in front
of its XF must come out untouched, and the command must finish."""
import gzip
import os
import struct
import subprocess

import pytest

from tests import bam_writer
from tests.common import BIN, ROOT
from tests.mirror import bamio

HARNESS = os.path.join(ROOT, "tests", "_aux_walk_harness")
DEPS = [os.path.join(ROOT, "tests", "aux_walk_harness.cpp"), os.path.join(ROOT, "svdss_amd", "csrc", "bam_aux_walk.h")]


def build_harness(sanitize=True):
    """sanitize=False: the same program from plain g++ under a name of its own (the gate of tests/test_smooth_edges_gpu.py:
    every value is still checked and a spin still shows as a timeout; sanitizers stay in this module, on the CPU)"""
    exe = HARNESS if sanitize else HARNESS + "_plain"
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *san, "-o", exe, DEPS[0]], check=True)
    return exe


def run_part(exe, part, sanitize=True):
    env = dict(os.environ)
    if sanitize:
        env.update(ASAN_OPTIONS="exitcode=99:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
    return subprocess.run([exe, part], capture_output=True, text=True, timeout=60, env=env)


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@pytest.mark.parametrize("part", ["step", "find"])
def test_aux_walk_part(harness, part):
    p = run_part(harness, part)
    assert p.returncode == 0 and f"{part} ok:" in p.stdout and "FAILED" not in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"


def test_host_smooth_finishes_on_a_negative_b_count(tmp_path):
    """ZZ:B:i with count -2: in size_t arithmetic its 5 + 4 * count bytes are -3, the walk's step 3 + (-3) = 0 -- set_xf spun
    on it for ever.  The walk now gives up: the record leaves with its aux block as it came, the records around it are
    tagged as usual."""
    ref = "ACGTTGCA" * 50
    fa = tmp_path / "ref.fa"
    fa.write_text(f">c0\n{ref}\n")
    read = ref[100:160]
    neg = b"ZZBi" + struct.pack("<i", -2) + b"XFi" + struct.pack("<i", 77)
    recs = [bam_writer.record("before", 0, 0, 100, 60, [("M", 60)], read, [("XF", "i", 9)], bytes([30] * 60)),
            bam_writer.record("neg", 0, 0, 100, 60, [("M", 60)], read, [], bytes([30] * 60)) + neg,
            bam_writer.record("after", 0, 0, 100, 60, [("M", 60)], read, [], bytes([30] * 60))]
    recs[1] = struct.pack("<i", len(recs[1]) - 4) + recs[1][4:]          # (block_size with the bytes appended)
    bam = tmp_path / "in.bam"
    bam.write_bytes(bam_writer.bam([("c0", len(ref))], recs))
    r = subprocess.run([BIN, "smooth", "--reference", str(fa), "--bam", str(bam), "--threads", "2"], capture_output=True, timeout=60,
                       env=dict(os.environ, SVDSS_SMOOTH_HOST="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = tmp_path / "out.bam"
    out.write_bytes(r.stdout)
    assert gzip.decompress(r.stdout)[:4] == b"BAM\1"
    _, _, got = bamio.read_bam(str(out))
    assert [(a.qname, a.aux) for a in got] == [("before", b"XFi" + struct.pack("<i", 2)), ("neg", neg), ("after", b"XFC\x02")]
