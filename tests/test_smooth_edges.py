"""The edge battery of tests/smooth_cases.py through the host code of `SVDSS smooth` (SVDSS_SMOOTH_HOST=1, no GPU needed)
against the mirror, record by record: which records are dropped, their order, XF, SEQ, QUAL, CIGAR and the whole aux block.
The records without an aligned base are left out here: their mismatch rate, 0/0, would enter the sort of the accuracy
percentile, which has no defined order with a NaN in it (in the reference as well); tests/test_smooth_edges_gpu.py runs
them with a given threshold."""
import collections
import math
import os
import subprocess

import pytest

from tests import smooth_cases as S
from tests.common import BIN
from tests.mirror import bamio


def write_inputs(tmp_path, nomatch=False):
    b = S.battery(nomatch)
    fa, bam = tmp_path / "ref.fa", tmp_path / "in.bam"
    fa.write_text(b.fasta)
    bam.write_bytes(b.bam)
    return b, fa, bam


def run_cli(fa, bam, env, threads="3", accp=None):
    r = subprocess.run([BIN, "smooth", "--reference", str(fa), "--bam", str(bam), "--threads", threads, "--min-mapq", str(S.MIN_MAPQ)]
                       + (["--accp", str(accp)] if accp is not None else []), capture_output=True, timeout=120, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def assert_records(got, want):
    """got: Alignments of tests/mirror/bamio.py; want: smooth_cases.Expect -- the same records in the same order, field by field"""
    assert [g.qname for g in got] == [w.name for w in want]
    bad = []
    for g, w in zip(got, want):
        for what, a, b in (("XF", g.tags.get("XF"), bamio.parse_tags(w.aux).get("XF")), ("aux", g.aux, w.aux),
                           ("CIGAR", g.cigar, list(w.cigar)), ("SEQ", g.seq, w.seq), ("QUAL", g.qual, w.qual)):
            if a != b:
                bad.append(f"{w.name} (XF {w.xf}): {what} {a!r}, the mirror says {b!r}")
    assert not bad, f"{len(bad)} field(s) differ:\n" + "\n".join(bad[:12])


def test_the_battery_is_what_it_says():
    want = S.check_battery_covers_what_it_says()
    assert collections.Counter(e.xf for e in want.values()).keys() == {0, 1, 2, 3} and len(want) > 200


def expected_of_the_file(b, accp):
    """What the CLI must make of the battery file.  accp=None: the default percentile (0.98: a threshold above 1, a few XF 1
    records); accp=0.5: the median rate, which is 0 -- every record with a mismatch is XF 1, the passed-through copies of
    every length modulo 4 among them."""
    acc = S.file_accuracy(b) if accp is None else S.file_accuracy(b, accp)
    want = S.expected(False, acc)
    assert math.isfinite(acc) and (acc > 1 if accp is None else acc == 0.0)
    assert accp is None or (S.passed_through_sizes(want, 1) == {0, 1, 2, 3} and sum(w.xf == 1 for w in want) > 30)
    return want


@pytest.mark.parametrize("accp", [None, 0.5])
def test_host_code_matches_the_mirror_on_the_edge_battery(tmp_path, accp):
    b, fa, bam = write_inputs(tmp_path)
    out = tmp_path / "out.bam"
    out.write_bytes(run_cli(fa, bam, {"SVDSS_SMOOTH_HOST": "1"}, accp=accp))
    names, lens, got = bamio.read_bam(str(out))
    assert names == S.NAMES and lens == b.ref_lens
    want = expected_of_the_file(b, accp)
    assert collections.Counter(w.xf for w in want).keys() == {0, 1, 2, 3} and len(want) < len(b.cases)
    assert_records(got, want)
    by = {g.qname: g for g in got}
    for g, w in zip(got, want):       # the core fields travel unchanged
        c = next(c for c in b.cases if c.name == w.name)
        assert (g.flag, g.tid, g.pos, g.mapq) == (c.flag, c.tid, c.pos, c.mapq), w.name
    assert by["thr_I21"].tags["XF"] == 0 and by["thr_I20"].tags["XF"] == 2 and by["thr_D21"].tags["XF"] == 0 and by["thr_D20"].tags["XF"] == 2
    assert by["end_N_middle"].tags["XF"] == 3 and by["acc_all_X"].tags["XF"] == 1


def test_host_code_does_not_depend_on_threads(tmp_path):
    b, fa, bam = write_inputs(tmp_path)
    assert run_cli(fa, bam, {"SVDSS_SMOOTH_HOST": "1"}, "1") == run_cli(fa, bam, {"SVDSS_SMOOTH_HOST": "1"}, "5")
