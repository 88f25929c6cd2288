"""`--compress runs|lz` on the command line (csrc/cli_options.h): the default, both spellings, the error text for any
other value, and the reference's options parsing as they did (through tests/prod_shim.cpp, the harness that
tests/test_ref_pins.py holds against the reference's own parser) when --compress stands among them."""
import ctypes as C
import os
import subprocess

import pytest

from tests.common import ROOT
from tests.test_ref_pins import config_parse, libs, parse_cases  # noqa: F401

SRC = os.path.join(ROOT, "tests", "native", "cli_compress_shim.cpp")
SO = os.path.join(ROOT, "tests", "native", "_cli_compress_shim.so")
HDR = os.path.join(ROOT, "svdss_amd", "csrc", "cli_options.h")


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC], check=True)
    return C.CDLL(SO)


def parse(shim, args):
    return config_parse(shim, "compress_parse", args)


def test_default_and_both_spellings(shim):
    assert parse(shim, []) == "compress=0 threads=4 bam="
    assert parse(shim, ["--compress=lz"]) == "compress=1 threads=4 bam="
    assert parse(shim, ["--compress", "lz"]) == "compress=1 threads=4 bam="
    assert parse(shim, ["--compress", "runs"]) == "compress=0 threads=4 bam="
    assert parse(shim, ["--compress=lz", "--compress=runs"]) == "compress=0 threads=4 bam="        # the last one wins
    assert parse(shim, ["--bam", "x.bam", "--compress", "lz", "--threads", "3"]) == "compress=1 threads=3 bam=x.bam"


def test_bad_values(shim):
    q = lambda s: "‘" + s + "’"   # noqa: E731
    assert parse(shim, ["--compress", "zip"]) == "error: Argument " + q("zip") + " failed to parse"
    assert parse(shim, ["--compress=LZ"]) == "error: Argument " + q("LZ") + " failed to parse"
    assert parse(shim, ["--compress="]) == "error: Argument " + q("") + " failed to parse"
    assert parse(shim, ["--compress"]) == "error: Option " + q("compress") + " is missing an argument"
    assert parse(shim, ["--compres", "lz"]) == "error: Option " + q("compres") + " does not exist"


def test_the_references_options_parse_as_before(libs):  # noqa: F811
    _, prod = libs
    fixed, rand = parse_cases()
    n = 0
    for args in fixed + rand[:120]:
        want = config_parse(prod, "prod_config_parse", args)
        if want.startswith("crash") or "--" in args:            # (behind a lone "--" nothing is an option)
            continue
        for extra in (["--compress", "lz"], ["--compress=runs"]):
            assert config_parse(prod, "prod_config_parse", extra + args) == want, args
            n += 1
    assert n > 200
