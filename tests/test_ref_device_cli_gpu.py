"""The reference FASTA read on the GPU (csrc/ref_loader.h, csrc/ref_stream.hip) through the binaries: `index`, `smooth`,
`call` and `run` write the bytes they write with SVDSS_REF_DEVICE=0 -- the .fmd and its sidecar, stdout, the --sfs and the
--clusters file -- whether the reference is a plain file, BGZF, plain gzip or BGZF with CRLF; --verbose says where the
reference was read and, when the device loader declined, why."""
import gzip
import re
import subprocess

import pytest

from svdss_amd import bamdev, refdev
from tests import run_fixture as RF
from tests.common import BIN
from tests.mirror.fastx import bgzf_pack

pytestmark = pytest.mark.gpu
LINE = re.compile(rb"reference: (\d+) batches on the device, (\d+) records, (\d+) bases")
HINT = b"reference: plain gzip is read by one thread; bgzip it to have it read on the GPU"
SMALL = {"SVDSS_REF_BATCH_KB": "100", "SVDSS_BAM_SLAB_KB": "64"}       # several batches, several slabs per file


def wrapped(contigs, eol=b"\n"):
    """wrap 60, every third line in lower case"""
    out = []
    for name, c in zip(RF.NAMES, contigs):
        out.append(b">" + name.encode() + b" a description")
        lines = [c[i:i + 60].encode() for i in range(0, len(c), 60)]
        out += [l.lower() if k % 3 == 1 else l for k, l in enumerate(lines)]
    return eol.join(out) + eol


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("refdev")
    f = RF.build(tmp, coverage=20, with_index=False)
    text = wrapped(f["contigs"])
    members = lambda t: [t[i:i + 60000] for i in range(0, len(t), 60000)]     # noqa: E731
    f["refs"] = {"plain": tmp / "ref.wrapped.fa", "bgzf": tmp / "ref.bgzf.fa.gz", "gzip": tmp / "ref.gzip.fa.gz", "crlf": tmp / "ref.crlf.fa.gz"}
    f["refs"]["plain"].write_bytes(text)
    f["refs"]["bgzf"].write_bytes(bgzf_pack(members(text)))
    f["refs"]["gzip"].write_bytes(gzip.compress(text, 6))
    f["refs"]["crlf"].write_bytes(bgzf_pack(members(wrapped(f["contigs"], b"\r\n"))))
    f["bases"] = sum(len(c) for c in f["contigs"])
    f["text"] = text
    return f


def sh(cmd, env):
    r = subprocess.run([BIN, *map(str, cmd)], capture_output=True, timeout=RF.TIMEOUT, env=env)
    assert r.returncode == 0, (cmd, r.stderr.decode()[-2000:])
    return r


class Commands:
    """every command's outputs for one reference file and one environment, as bytes"""

    def __init__(self, fx, sfs=None, fmd=None):
        self.fx, self.n, self.sfs, self.fmd = fx, 0, sfs, fmd

    def all(self, ref, **env):
        tmp, e = self.fx["tmp"], RF.env0(**env)
        self.n += 1
        fmd, clu, sfs, rclu = tmp / f"o{self.n}.fmd", tmp / f"o{self.n}.clusters", tmp / f"o{self.n}.sfs", tmp / f"o{self.n}.run.clusters"
        out, err = {}, {}
        err["index"] = sh(["index", "--verbose", "-t", "8", "-d", ref, "-o", fmd], e).stderr
        out["fmd"], out["svdss"] = fmd.read_bytes(), (tmp / f"o{self.n}.fmd.svdss").read_bytes()
        r = sh(["smooth", "--verbose", "--reference", ref, "--bam", self.fx["bam"]], e)
        out["smooth"], err["smooth"] = r.stdout, r.stderr
        if self.sfs is None:       # (the first call of all: the SFS of the chain, and its index, for every later one)
            self.fmd = fmd
            smoothed = tmp / "smoothed.bam"
            smoothed.write_bytes(r.stdout)
            self.sfs = tmp / "chain.sfs"
            self.sfs.write_bytes(sh(["search", "--index", fmd, "--bam", smoothed], e).stdout)
        r = sh(["call", "--verbose", "--reference", ref, "--bam", self.fx["bam"], "--sfs", self.sfs, "--clusters", clu], e)
        out["call"], out["call_clusters"], err["call"] = r.stdout, clu.read_bytes(), r.stderr
        r = sh(["run", "--verbose", "--reference", ref, "--bam", self.fx["bam"], "--index", self.fmd, "--sfs", sfs, "--clusters", rclu], e)
        out["run"], out["run_sfs"], out["run_clusters"], err["run"] = r.stdout, sfs.read_bytes(), rclu.read_bytes(), r.stderr
        return out, err


@pytest.fixture(scope="module")
def base(fx):
    """the plain file with the device loader off: what every other run must write"""
    c = Commands(fx)
    out, err = c.all(fx["refs"]["plain"], SVDSS_REF_DEVICE="0")
    assert all(not LINE.search(e) for e in err.values())
    rows = [l for l in out["call"].split(b"\n") if l and not l.startswith(b"#")]
    assert len(rows) >= 3 and out["run"] == out["call"] and len(out["smooth"]) > 100000 and out["run_sfs"]
    return c, out


def same(out, want):
    for k in want:
        assert out[k] == want[k], k


def lines_of(fx, err, expect):
    for cmd, e in err.items():
        m = LINE.search(e)
        assert bool(m) == expect, (cmd, e.decode()[-1500:])
        if m:
            assert int(m.group(1)) > 0 and int(m.group(2)) == len(RF.NAMES) - 1 and int(m.group(3)) == fx["bases"]


def test_bgzf_default_reads_on_the_device(fx, base):
    c, want = base
    out, err = c.all(fx["refs"]["bgzf"], **SMALL)
    same(out, want)
    lines_of(fx, err, True)
    assert all(int(LINE.search(e).group(1)) > 3 for e in err.values())
    out, err = c.all(fx["refs"]["bgzf"])                         # one batch
    same(out, want)
    lines_of(fx, err, True)


def test_bgzf_with_the_loader_off(fx, base):
    c, want = base
    for env in ({"SVDSS_REF_DEVICE": "0"}, {"SVDSS_FASTA_SERIAL": "1"}):
        out, err = c.all(fx["refs"]["bgzf"], **env)
        same(out, want)
        lines_of(fx, err, False)


def test_plain_file(fx, base):
    c, want = base
    out, err = c.all(fx["refs"]["plain"])                        # the default: the mapped reader
    same(out, want)
    lines_of(fx, err, False)
    out, err = c.all(fx["refs"]["plain"], SVDSS_REF_DEVICE="2", **SMALL)
    same(out, want)
    lines_of(fx, err, True)


def test_plain_gzip_says_bgzip_it(fx, base):
    c, want = base
    out, err = c.all(fx["refs"]["gzip"])
    same(out, want)
    lines_of(fx, err, False)
    assert all(e.count(HINT) == 1 for e in err.values()), {k: e.count(HINT) for k, e in err.items()}


def test_crlf_declines_and_says_why(fx, base):
    c, want = base
    out, err = c.all(fx["refs"]["crlf"])
    same(out, want)
    lines_of(fx, err, False)
    assert all(b"reference: the device loader declined (a carriage return at byte" in e for e in err.values())


def test_resident_reference_feeds_smoothing(fx):
    """bamdev.smooth_bam over the svdss_ref_t of svdss_ref_stream_finish gives the bytes it gives over an uploaded one"""
    bam = fx["bam"].read_bytes()
    want, _ = bamdev.smooth_bam(bam, fx["contigs"])
    blob = bgzf_pack([fx["text"][i:i + 50000] for i in range(0, len(fx["text"]), 50000)])
    with refdev.resident(blob, 100000, bgzf=True) as r:
        got, _ = bamdev.smooth_bam(bam, r)
    assert got == want and len(got) > 100000
