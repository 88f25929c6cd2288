"""The edge battery of tests/smooth_cases.py on the two GPU paths of `SVDSS smooth`, against the mirror of smoother.cpp
(tests/mirror/smoother.py) -- not against another run of the same kernels:

- smooth_kernel (csrc/place.hip) directly, through svdss_amd.smoothdev.smooth_batch: length, CIGAR, packed bases, qualities,
  match / mismatch counts and the ignore flag of every record that fits;
- the device path (csrc/bam_smooth.hip: smooth_walk_kernel, smooth_size_kernel, smooth_write_kernel) through
  bamdev.smooth_bam: the inflated output record by record, with one batch and with batches of 4 KB (records straddle
  batches, the output more than one BGZF member), at the accuracy threshold of the `onemis` record and at the next double
  below it; and what svdss_bam_smooth_measure counts;
- the CLI on the battery file by its three paths (device path, SVDSS_BAM_DEVICE=0: host pipeline + GPU walk,
  SVDSS_SMOOTH_HOST=1: host code): the same bytes, and those the mirror's records.

The battery holds aux blocks the walk gives up on (a B count that overruns, cut-off tags; never a negative count): this
module runs nothing unless tests/aux_walk_harness.cpp -- the shared walk on the CPU, here from plain g++ (the ASan / UBSan
build of it is tests/test_aux_walk_host.py's, which needs no GPU) -- is green first."""
import gzip

import pytest

from svdss_amd import bamdev, bgzf, smoothdev
from tests import bam_writer, smooth_cases as S, test_aux_walk_host, test_smooth_edges
from tests.mirror import bamio, smoother

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def aux_walk_is_green_on_the_cpu():
    exe = test_aux_walk_host.build_harness(sanitize=False)
    for part in ("step", "find"):
        p = test_aux_walk_host.run_part(exe, part, sanitize=False)
        if p.returncode != 0 or f"{part} ok:" not in p.stdout:
            pytest.fail(f"the aux walk fails on the CPU ({part}): no record goes to the GPU\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", pytrace=False)


def pack(seq):
    b = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        b[i >> 1] |= bam_writer.SEQ16.get(ch, 15) << (4 if i % 2 == 0 else 0)
    return bytes(b)


def test_walk_kernel_matches_the_mirror():
    b, ch = S.battery(True), S.chromosomes()
    recs = [a for a in S.kept(b) if smoother.fits(a, len(ch[S.NAMES[a.tid]]))]
    assert len(recs) > 200 and any(smoother._mismatch_counts(a, ch[S.NAMES[a.tid]]) == (0, 0) for a in recs)
    got = smoothdev.smooth_batch(b.contigs, [a.tid for a in recs], [a.pos for a in recs], [[(l << 4) | op for l, op in a.cigar] for a in recs],
                                 [pack(a.seq) for a in recs], [a.qual for a in recs])
    bad = []
    for a, g in zip(recs, got):
        nm, nx, ign, ns, nq, nc = smoother.walk_read(a, a.qual, ch[S.NAMES[a.tid]])
        want = {"length": len(ns), "cigar": [(l << 4) | op for l, op in nc], "seq4": pack(ns), "qual": nq, "matches": nm, "mismatches": nx, "ignore": ign}
        g = dict(g, cigar=[int(w) for w in g["cigar"]])
        for k in want:
            if g[k] != want[k]:
                bad.append(f"{a.qname}: {k} {g[k]!r}, the mirror says {want[k]!r}")
    assert not bad, f"{len(bad)} field(s) differ:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("batch_bytes", [256 << 20, 4096])
@pytest.mark.parametrize("acc", [S.ACC, S.ACC_BELOW], ids=["acc=1/99", "acc=next_below"])
def test_device_path_matches_the_mirror(tmp_path, acc, batch_bytes):
    b = S.battery(True)
    stream, n_batches = bamdev.smooth_bam(b.bam, b.contigs, min_mapq=S.MIN_MAPQ, acc=acc, batch_bytes=batch_bytes)
    assert n_batches == (1 if batch_bytes > 4096 else len(bgzf.batches(b.bam, 4096))) and (batch_bytes > 4096 or n_batches > 10)
    assert len(bgzf.bgzf_blocks(stream)) >= 2 and len(gzip.decompress(stream)) > 0xff00        # more than one output member
    out = tmp_path / "out.bam"
    out.write_bytes(stream)
    names, lens, got = bamio.read_bam(str(out))
    assert names == S.NAMES and lens == b.ref_lens
    want = S.expected(True, acc)
    test_smooth_edges.assert_records(got, want)
    by = {w.name: w.xf for w in want}
    assert by["onemis"] == (0 if acc == S.ACC else 1) and by["twomis_198"] == by["onemis"] and by["nomatch_all_S"] == 0 and by["thr_I20"] == 2


@pytest.mark.parametrize("batch_bytes", [256 << 20, 4096])
def test_device_path_measures_what_the_mirror_counts(batch_bytes):
    b, ch = S.battery(True), S.chromosomes()
    measured, counts = bamdev.smooth_bam(b.bam, b.contigs, min_mapq=S.MIN_MAPQ, batch_bytes=batch_bytes, measure=True)
    want = []
    for a in S.kept(b):
        mx = smoother._mismatch_counts(a, ch[S.NAMES[a.tid]])
        want.append((0, 0, 0) if mx is None else (mx[0], mx[1], 1))
    assert sum(n for n, _ in counts) == len(b.cases) and sum(k for _, k in counts) == len(want)
    bad = [f"{a.qname}: {g}, the mirror says {w}" for a, g, w in zip(S.kept(b), measured, want) if g != w]
    assert len(measured) == len(want) and not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("accp", [None, 0.5])
def test_the_three_cli_paths_write_the_mirrors_records(tmp_path, accp):
    b, fa, bam = test_smooth_edges.write_inputs(tmp_path)
    outs = {}
    for path, env in (("device", {}), ("host + gpu walk", {"SVDSS_BAM_DEVICE": "0"}), ("host", {"SVDSS_SMOOTH_HOST": "1"})):
        outs[path] = test_smooth_edges.run_cli(fa, bam, env, accp=accp)
    assert outs["device"] == outs["host"] and outs["host + gpu walk"] == outs["host"]
    out = tmp_path / "out.bam"
    out.write_bytes(outs["device"])
    _, _, got = bamio.read_bam(str(out))
    test_smooth_edges.assert_records(got, test_smooth_edges.expected_of_the_file(b, accp))
