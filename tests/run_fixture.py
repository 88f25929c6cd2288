"""The data set of tests/test_run_gpu.py and tests/test_run_store_gpu.py (`SVDSS run`, svdss_bam_smooth_set_store): the chain of
tests/test_pipeline_gpu.py::test_run_svdss_chain_with_raw_reads -- two contigs of 250 kb and 120 kb, 8 implanted SVs, 6 kb
reads at 30x with 0.5 % errors -- plus what the record store can go wrong on: records the filters of `smooth` and of `call`
treat differently (a contig the FASTA does not have, reads of 2-99 bases), records both drop (mapq 10, flags 256 / 2048,
unmapped), HP tags of either width, random qualities, odd read lengths, one read name twice within a thread slice of
`search`, and an unmapped tail that makes a batch seam wherever the batches are small."""
import os
import subprocess

import numpy as np

from svdss_amd import synth
from tests import bam_writer
from tests.common import BIN
from tests.pipeline_sim import add_errors, simulate

NAMES = ["chrA", "chrB", "chrC"]      # (chrC: in the BAM's header, not in the FASTA)
CHRC_LEN = 50000
TIMEOUT = 300
KNOBS = ("SVDSS_SMOOTH_HOST", "SVDSS_GPU_DEFLATE", "SVDSS_BAM_DEVICE", "SVDSS_SEARCH_LF", "SVDSS_SEARCH_LF_MAX", "SVDSS_KMER", "SVDSS_PARK_MB",
         "SVDSS_PARK_GB", "SVDSS_PARK_ARENA_MB", "SVDSS_EARLY_HOLD_MS", "SVDSS_BAM_BATCH_MB", "SVDSS_BAM_SLAB_KB", "SVDSS_DEBUG", "SVDSS_SEARCH_EARLY",
         "SVDSS_CALL_STORE", "SVDSS_CALL_STORE_MB", "SVDSS_CALL_STORE_GB", "SVDSS_CALL_STORE_INITIAL_MB", "SVDSS_STORE_ARENA_MB", "SVDSS_PLACE_HOST",
         "SVDSS_CLEAN_EXIT", "SVDSS_CALL_PASS2", "SVDSS_CALL_NO_BAI")


def env0(**more):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(more)
    return e


def build(tmp, seed=9, coverage=30, with_index=True):
    """Writes ref.fa, reads.bam (and ref.fa.fmd) into tmp; returns a dict of paths and of what the tests look up."""
    rng = np.random.default_rng(4)
    ref, svs, reads = simulate(seed=seed, coverage=coverage)
    fa = tmp / "ref.fa"
    with open(fa, "w") as fh:
        for n, c in zip(NAMES, ref):
            fh.write(f">{n}\n{synth.to_ascii(c)}\n")
    items = []          # (tid, pos, name, flag, mapq, cigar, seq, tags, searched by `search`)
    for k, (n, tid, pos, cig, seq, _) in enumerate(reads):
        noisy = k % 67 == 3
        s2, c2 = add_errors(seq, cig, rng, 0.05 if noisy else 0.005)
        if k % 10 == 0 and not noisy:     # soft clips of random bases: SFS whatever else the read spans
            clip = synth.to_ascii(rng.integers(1, 5, size=150).astype(np.uint8))
            if k % 20 == 0:
                s2, c2 = clip + s2, [("S", 150)] + list(c2)
            else:
                s2, c2 = s2 + clip, list(c2) + [("S", 150)]
        tags = [("HP", "C", 1 + (k // 3) % 2)] if k % 3 == 0 else ([("HP", "i", 2)] if k % 11 == 0 else [])
        flag, mapq = 0, 60
        if k % 53 == 7:
            mapq = 10
        elif k % 59 == 5:
            flag = 256
        elif k % 61 == 9:
            flag = 2048
        items.append((tid, pos, n, flag, mapq, c2, s2, tags, flag == 0 and mapq >= 20))
    for k in range(40):   # reads of 2-99 bases, exact copies of the reference: `smooth` drops those of < 2, `search` those of < 100
        l = int(rng.integers(2, 100))
        pos = int(rng.integers(0, len(ref[0]) - 200))
        items.append((0, pos, f"short{k:03d}", 0, 60, [("M", l)], synth.to_ascii(ref[0][pos:pos + l]), [("HP", "C", 1)] if k % 2 else [], False))
    for k in range(12):   # reads on the contig the FASTA does not have: `smooth` drops them, `call`'s filters keep them
        l = 3001 + 2 * k
        items.append((2, 1000 + 3000 * k, f"orphan{k:02d}", 0, 60, [("M", l)], synth.to_ascii(rng.integers(1, 5, size=l).astype(np.uint8)),
                      [("HP", "i", 1)] if k % 2 else [], False))
    items.sort(key=lambda r: (r[0], r[1]))
    # one name twice within a thread slice: the sequence `search` deals is the reads of the smoothed BAM with >= 100 bases, in
    # file order; two clipped reads a multiple of 12 places apart (of 3 and of 4 threads), both inside one reference batch of
    # 63 or of 10,000 (the construction of tests/test_smooth_sfs_gpu.py)
    seq_ix = [i for i, it in enumerate(items) if it[8]]
    clipped = lambda it: it[5][0][0] == "S" or it[5][-1][0] == "S"   # noqa: E731
    twin = None
    for q, d in ((q, d) for q in range(len(seq_ix) - 60) for d in (12, 24, 36, 48, 60)):
        if q % 63 + d < 63 and clipped(items[seq_ix[q]]) and clipped(items[seq_ix[q + d]]):
            twin = (seq_ix[q], seq_ix[q + d])
            break
    assert twin is not None
    items[twin[1]] = items[twin[1]][:2] + (items[twin[0]][2],) + items[twin[1]][3:]
    recs = []
    for tid, pos, n, flag, mapq, cig, seq, tags, _ in items:
        qual = bytes(rng.integers(1, 60, size=len(seq)).astype(np.uint8))
        recs.append(bam_writer.record(n, flag, tid, pos, mapq, cig, seq, tags, qual))
    useq = synth.to_ascii(rng.integers(1, 5, size=10001).astype(np.uint8))
    unmapped = bam_writer.record("unmapped", 4, -1, -1, 0, [], useq, [], bytes(rng.integers(1, 60, size=10001).astype(np.uint8)))
    recs += [unmapped] * 300
    bam = tmp / "reads.bam"
    lens = [len(c) for c in ref] + [CHRC_LEN]
    bam.write_bytes(bam_writer.bam(list(zip(NAMES, lens)), recs))
    fmd = tmp / "ref.fa.fmd"
    if with_index:
        r = subprocess.run([BIN, "index", "-t", "8", "-d", str(fa), "-o", str(fmd)], capture_output=True, timeout=TIMEOUT, env=env0())
        assert r.returncode == 0, r.stderr.decode()
    return {"tmp": tmp, "fa": fa, "bam": bam, "fmd": fmd, "contigs": [synth.to_ascii(c) for c in ref], "lens": lens,
            "twin_name": items[twin[0]][2], "n_items": len(items)}
