"""`SVDSS index` as a drop-in for `ropebwt3 build`: several inputs, -i / --append OLD (the records of an existing index
first -- from its sidecar, or recovered from the .fmd's BWT by svdss_bwt_strings), and the .fmd on stdout without -o.
Where there is no GPU the suite's conftest gives the binary its host builder, and the walks run on the host."""
import os
import pty
import subprocess

import pytest

import svdss_amd
from tests import index_append_cases as A


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("append")
    a, b = A.make_inputs(d)
    A.index(d, "-d", d / "ab.fa", "-o", d / "ab.fmd")
    A.index(d, "-d", d / "a.fa", "-o", d / "a.fmd")
    return d, a, b, A.pair(d / "ab.fmd")


def test_several_inputs_are_indexed_in_command_line_order(case):
    d, a, b, want = case
    A.index(d, "-d", d / "a.fa", d / "b.fa.gz", "-o", d / "x.fmd")
    assert A.pair(d / "x.fmd") == want
    A.index(d, "-d", d / "b.fa.gz", d / "a.fa", "-o", d / "ba.fmd")      # the other order is another index
    assert A.pair(d / "ba.fmd")[1] != want[1]


def test_append_takes_the_records_of_the_sidecar_first(case, tmp_path):
    d, a, b, want = case
    A.index(d, "-i", d / "a.fmd", "-d", d / "b.fa.gz", "-o", tmp_path / "y.fmd")
    assert A.pair(tmp_path / "y.fmd") == want
    r = A.index(d, "--append", d / "a.fmd", "--verbose", "-d", d / "b.fa.gz", "-o", tmp_path / "y2.fmd")
    assert A.pair(tmp_path / "y2.fmd") == want
    assert "3 record(s), 3745 bases from its sidecar" in r.stderr.decode()
    # the full layout as a sidecar serves as well
    A.index(d, "-d", d / "a.fa", "-o", tmp_path / "full.fmd", env=dict(os.environ, SVDSS_INDEX_FULL="1"))
    A.index(d, "-i", tmp_path / "full.fmd", "-d", d / "b.fa.gz", "-o", tmp_path / "y3.fmd")
    assert A.pair(tmp_path / "y3.fmd") == want
    # OLD is read completely before the output is opened: it may be the output
    for ext in ("", ".svdss"):
        (tmp_path / ("same.fmd" + ext)).write_bytes((d / ("a.fmd" + ext)).read_bytes())
    os.utime(tmp_path / "same.fmd.svdss")
    A.index(d, "-i", tmp_path / "same.fmd", "-d", d / "b.fa.gz", "-o", tmp_path / "same.fmd")
    assert A.pair(tmp_path / "same.fmd") == want


def test_append_to_an_index_in_ropebwt_order_without_a_sidecar(case, tmp_path):
    d, a, b, want = case
    A.rope_fmd(a, tmp_path / "up.fmd")
    r = A.index(d, "-i", tmp_path / "up.fmd", "--verbose", "-d", d / "b.fa.gz", "-o", tmp_path / "y.fmd")
    assert A.pair(tmp_path / "y.fmd") == want
    assert "3 record(s), 3745 bases from its BWT by the" in r.stderr.decode()
    # past the step limit the serial walk takes over: the same index
    r = A.index(d, "-i", tmp_path / "up.fmd", "--verbose", "-d", d / "b.fa.gz", "-o", tmp_path / "y4.fmd",
                env=dict(os.environ, SVDSS_INVERT_MAX_STEPS="5"))
    assert A.pair(tmp_path / "y4.fmd") == want and "one serial walk per string" in r.stderr.decode()


def test_append_to_an_fmd_whose_sidecar_is_gone(case, tmp_path):
    """the records come out of this library's own BWT then, in ITS sentinel order: another record order, so not the
    same bytes -- the same index for every question a search asks"""
    d, a, b, want = case
    (tmp_path / "a.fmd").write_bytes((d / "a.fmd").read_bytes())
    A.index(d, "-i", tmp_path / "a.fmd", "-d", d / "b.fa.gz", "-o", tmp_path / "y.fmd")
    got = svdss_amd.FMDIndex.load(str(tmp_path / "y.fmd"))
    ref = svdss_amd.FMDIndex.load(str(d / "ab.fmd"))
    assert got.size == ref.size and (got.acc == ref.acc).all()
    pats = A.sampled_substrings(a + b, 200, seed=5)
    counts = [ref.count(p) for p in pats]
    assert [got.count(p) for p in pats] == counts and sum(1 for c in counts if c > 0) > 100


def test_without_o_the_fmd_goes_to_stdout(case, tmp_path):
    d, a, b, want = case
    with open(tmp_path / "z.fmd", "wb") as fh:
        r = A.run("index", "-t", "2", "-d", str(d / "a.fa"), stdout=fh)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "z.fmd").read_bytes() == (d / "a.fmd").read_bytes()       # no log line among the bytes
    assert not os.path.exists(tmp_path / "z.fmd.svdss") and b"All done" in r.stderr
    r = A.run("index", "-t2", "-d", str(d / "a.fa"))                              # a pipe
    assert r.returncode == 0 and r.stdout == (d / "a.fmd").read_bytes()
    # a terminal: the usage text, as before (where the machine has a pseudo-terminal to give)
    try:
        master, slave = pty.openpty()
    except OSError:
        master = slave = None
    if slave is not None:
        try:
            r = A.run("index", "-d", str(d / "a.fa"), stdout=slave)
        finally:
            os.close(master)
            os.close(slave)
        assert r.returncode == 1 and b"Usage: SVDSS index" in r.stderr
    r = A.run("index", "-i", str(d / "a.fmd"), "-o", str(tmp_path / "none.fmd"))  # an input is still required
    assert r.returncode == 1 and b"Usage: SVDSS index" in r.stderr and not os.path.exists(tmp_path / "none.fmd")


def test_refusals_leave_no_file(case, tmp_path):
    d, a, b, want = case
    out = tmp_path / "out.fmd"

    def refused(old, *needles):
        r = A.run("index", "-i", str(old), "-d", str(d / "b.fa.gz"), "-o", str(out))
        err = r.stderr.decode()
        assert r.returncode == 1 and all(n in err for n in needles), err
        assert not os.path.exists(out) and not os.path.exists(str(out) + ".svdss") and not os.path.exists(str(out) + ".svdss.tmp")

    refused(tmp_path / "nothing.fmd", "cannot open", "nothing.fmd")
    (tmp_path / "ref.fmr").write_bytes(b"\x01\x02\x03\x04" + bytes(200))
    refused(tmp_path / "ref.fmr", ".fmr", "ropebwt3 build")
    import numpy as np
    from tests import rld0_py
    (tmp_path / "fwd.fmd").write_bytes(rld0_py.encode_rld0(rld0_py.collection_bwt([np.asarray(c) for c in a])))   # no reverse complements
    refused(tmp_path / "fwd.fmd", "reverse complements")
