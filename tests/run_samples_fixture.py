"""The data of tests/test_run_samples_gpu.py (`SVDSS run --samples`): ONE reference (two contigs of 250 kb and 120 kb, as
tests/run_fixture.py) and one index, and several small samples on it -- each its own SVs and reads (6 kb, 6x, 0.5 % errors),
its own order of the contigs in the BAM header, and the oddities a session must not carry from one sample into the next:
a contig the FASTA lacks, records the filters drop, an unmapped tail of many batches, reads that are all searched, a file
without a record, a file that ends inside a record."""
import gzip
import subprocess

import numpy as np

from svdss_amd import synth
from tests import bam_writer
from tests.common import BIN
from tests.pipeline_sim import add_errors, hap_segments, read_alignment
from tests.run_fixture import TIMEOUT, env0

REF_LENS = {"chrA": 250000, "chrB": 120000}
CHRC_LEN = 50000      # (chrC: in some headers, never in the FASTA)
READ_LEN = 6000


def reference(tmp):
    """ref.fa and ref.fa.fmd in tmp; the contigs by name"""
    ref = dict(zip(REF_LENS, synth.make_reference(list(REF_LENS.values()), seed=5, repeat_frac=0.0)))
    fa = tmp / "ref.fa"
    with open(fa, "w") as fh:
        for n, c in ref.items():
            fh.write(f">{n}\n{synth.to_ascii(c)}\n")
    fmd = tmp / "ref.fa.fmd"
    r = subprocess.run([BIN, "index", "-t", "8", "-d", str(fa), "-o", str(fmd)], capture_output=True, timeout=TIMEOUT, env=env0())
    assert r.returncode == 0, r.stderr.decode()
    return {"tmp": tmp, "fa": fa, "fmd": fmd, "ref": ref}


def sample(ref, path, order, seed, n_svs=5, coverage=6, err=0.005, clip_all=False, orphans=False, unmapped=0, first=None):
    """One BAM at `path`.  order: the header's contigs (chrC allowed); clip_all: every read ends in 150 random soft-clipped
    bases, so `smooth` tags all of them XF = 0 and all are searched; orphans: reads on chrC; unmapped: that many unmapped
    records of 10 kb behind the mapped ones; first: only the first that many mapped reads.  Returns what the tests look up."""
    rng = np.random.default_rng(seed)
    names = [n for n in REF_LENS]
    hap, svs = synth.implant_svs([ref[n] for n in names], n_svs, seed=seed + 1, min_len=60, max_len=400)
    tid_of = {n: t for t, n in enumerate(order)}
    items = []
    k = 0
    for ci, n in enumerate(names):
        segs = hap_segments(len(ref[n]), [s for s in svs if s.contig == ci])
        for _ in range(int(coverage * len(hap[ci]) / READ_LEN)):
            a = int(rng.integers(0, len(hap[ci]) - READ_LEN))
            cig, pos = read_alignment(segs, a, a + READ_LEN)
            if pos is None:
                continue
            seq, cig = add_errors(synth.to_ascii(hap[ci][a:a + READ_LEN]), cig, rng, err)
            if clip_all or k % 10 == 0:
                seq, cig = seq + synth.to_ascii(rng.integers(1, 5, size=150).astype(np.uint8)), list(cig) + [("S", 150)]
            tags = [("HP", "C", 1 + (k // 3) % 2)] if k % 3 == 0 else []
            flag, mapq = (0, 10) if k % 53 == 7 else (256, 60) if k % 59 == 5 else (2048, 60) if k % 61 == 9 else (0, 60)
            items.append((tid_of[n], pos, f"s{seed}r{k:05d}", flag, mapq, cig, seq, tags))
            k += 1
    items.sort(key=lambda r: (r[0], r[1]))
    if first is not None:
        items = items[:first]
    if orphans:
        for j in range(8):
            l = 3001 + 2 * j
            items.append((tid_of["chrC"], 1000 + 3000 * j, f"s{seed}orphan{j}", 0, 60, [("M", l)], synth.to_ascii(rng.integers(1, 5, size=l).astype(np.uint8)), []))
        items.sort(key=lambda r: (r[0], r[1]))
    recs = [bam_writer.record(n, flag, tid, pos, mapq, cig, seq, tags, bytes(rng.integers(1, 60, size=len(seq)).astype(np.uint8)))
            for tid, pos, n, flag, mapq, cig, seq, tags in items]
    if unmapped:
        useq = synth.to_ascii(rng.integers(1, 5, size=10001).astype(np.uint8))
        recs += [bam_writer.record("unmapped", 4, -1, -1, 0, [], useq, [], bytes(rng.integers(1, 60, size=10001).astype(np.uint8)))] * unmapped
    lens = dict(REF_LENS, chrC=CHRC_LEN)
    path.write_bytes(bam_writer.bam([(n, lens[n]) for n in order], recs))
    return {"bam": path, "order": list(order), "n_mapped": len(items), "n_svs": len(svs)}


def header_only(path, order):
    lens = dict(REF_LENS, chrC=CHRC_LEN)
    path.write_bytes(bam_writer.bam([(n, lens[n]) for n in order], []))
    return {"bam": path, "order": list(order), "n_mapped": 0, "n_svs": 0}


def cut_inside_last_record(src, path):
    """src's inflated stream without its last 37 bytes, as BGZF again: the file ends inside a record (the damage of
    tests/test_bam_device_gpu.py::test_damage_is_reported)"""
    raw = gzip.decompress(src.read_bytes())
    path.write_bytes(bam_writer.bgzf(raw[:-37]))
    return path
