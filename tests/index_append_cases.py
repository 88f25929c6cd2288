"""`SVDSS index` with several inputs, -i / --append and no -o: the files and the runs tests/test_index_append_cli.py
(host builder, host walk) and tests/test_index_append_gpu.py (GPU builder, device walk) share.  Test infrastructure only."""
import gzip
import os
import subprocess

import numpy as np

from svdss_amd import synth
from tests import rld0_py
from tests.common import ROOT

BIN = os.path.join(ROOT, "svdss_amd", "SVDSS")


def run(*args, env=None, stdout=subprocess.PIPE):
    return subprocess.run([BIN, *args], stdout=stdout, stderr=subprocess.PIPE, timeout=600, env=env)


def fasta_text(records, prefix):
    out = []
    for i, c in enumerate(records):
        s = synth.to_ascii(c)
        out.append(f">{prefix}{i + 1} x\n" + "\n".join(s[k:k + 60] for k in range(0, len(s), 60)) + "\n")
    return "".join(out)


def make_inputs(d):
    """a.fa (plain), b.fa.gz (gzip), ab.fa (their concatenation) under d: (records of a, records of b)"""
    a = synth.make_reference([3000, 700, 45], seed=31, n_runs=(20,))
    b = synth.make_reference([2100, 333], seed=32)
    (d / "a.fa").write_text(fasta_text(a, "a"))
    with gzip.open(d / "b.fa.gz", "wt") as fh:
        fh.write(fasta_text(b, "b"))
    (d / "ab.fa").write_text(fasta_text(a, "a") + fasta_text(b, "b"))
    return a, b


def index(d, *args, env=None):
    r = run("index", "-t", "2", *[str(x) for x in args], env=env)
    assert r.returncode == 0, r.stderr.decode()
    return r


def pair(fmd):
    """the bytes of an index and of its sidecar"""
    return open(fmd, "rb").read(), open(str(fmd) + ".svdss", "rb").read()


def rope_fmd(records, path):
    """the records and their reverse complements as ropebwt3 would index them: an .fmd without a sidecar"""
    strings = []
    for c in records:
        strings += [c, synth.revcomp(c)]
    open(path, "wb").write(rld0_py.encode_rld0(rld0_py.collection_bwt(strings)))


def sampled_substrings(records, k, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        c = records[int(rng.integers(0, len(records)))]
        l = int(rng.integers(1, min(30, len(c)) + 1))
        s = int(rng.integers(0, len(c) - l + 1))
        p = c[s:s + l].copy()
        if rng.random() < 0.3:
            p[int(rng.integers(0, l))] = int(rng.integers(1, 5))   # now and then one that may not occur
        out.append(synth.revcomp(p) if rng.random() < 0.5 else p)
    return out
