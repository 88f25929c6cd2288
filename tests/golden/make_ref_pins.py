#!/usr/bin/env python3
"""Generates tests/golden/ref_pins.json: what the reference's own sv.cpp and config.cpp give for the seeded cases of
tests/test_ref_pins.py.

Needs oracle/_ref/libsvdss_ref.so (`make -C oracle ref REF=<reference checkout>`).  Only outputs are stored: the VCF rows
as SHA-256 digests, the parses as text, and digests of the inputs they belong to.

Run from the repo root:  python tests/golden/make_ref_pins.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_ref_pins as T  # noqa: E402


def main():
    ref = C.CDLL(T.REF_SO)
    rows, less = T.sv_cases()
    fixed, rand = T.parse_cases()
    out = {
        "sv_rows_inputs": T.digest(rows),
        "sv_rows_sha256": [T.sha256(T.sv_row(ref, "ref_sv_row", *a)) for a in rows],
        "sv_less_inputs": T.digest(less),
        "sv_less": [T.sv_less(ref, "ref_sv_less", *c) for c in less],
        "config_fixed_inputs": T.digest(fixed),
        "config_fixed": [T.config_parse(ref, "ref_config_parse", a) for a in fixed],
        "config_random_inputs": T.digest(rand),
        "config_random": [T.config_parse(ref, "ref_config_parse", a) for a in rand],
    }
    bad = [a for a, s in zip(fixed, out["config_fixed"]) if s.startswith("crash")]
    if bad:
        raise SystemExit(f"the reference crashed on fixed cases: {bad}")
    with open(T.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print(f"wrote {T.GOLDEN}")


if __name__ == "__main__":
    main()
