"""--region REG / --regions-file BED on the command line (csrc/bam_regions.h, csrc/cli_options.h, csrc/svdss_main.cpp): every
form of REG against the header's names, the BED file, the refusals (with their messages, and with nothing written), and
`SVDSS smooth --region` through the host reader (no GPU needed): the output of `smooth` on the BAM that holds the region's
records alone."""
import os
import subprocess

import pytest

from tests import region_lib as R
from tests.common import BIN
from tests.test_smooth_index import check_index, exe, smooth, write_fixture   # noqa: F401  (exe: a fixture)

NAMES = ["chr1", "chr2", "HLA:A", "chr1:1-5", "chrM"]
END = 2**31 - 1


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    exe_ = R.parse_exe()
    names = tmp_path_factory.mktemp("names") / "names.txt"
    names.write_text("".join(n + "\n" for n in NAMES))

    def run(*args):
        r = subprocess.run([exe_, str(names), *args], capture_output=True, text=True, timeout=60)
        return r.returncode, [tuple(int(x) for x in l.split("\t")) for l in r.stdout.splitlines()], r.stderr
    return run


@pytest.mark.parametrize("text,want", [
    ("chr2", (1, 0, END)),                     # NAME
    ("chr2:101-200", (1, 100, 200)),           # NAME:BEG-END, 1-based inclusive
    ("chr2:1-1", (1, 0, 1)),
    ("chr2:1,001-", (1, 1000, END)),           # NAME:BEG-, commas ignored
    ("chr2:5", (1, 4, END)),                   # NAME:BEG: to the end of the reference, as samtools reads it
    ("chr2:1,000,000-2,000,000", (1, 999999, 2000000)),
    ("HLA:A", (2, 0, END)),                    # a name with ':' is that reference ...
    ("HLA:A:11-20", (2, 10, 20)),              # ... and a text is split at its LAST ':'
    ("chr1:1-5", (3, 0, END)),                 # a header name that reads like chr1's bases 1-5: the name as it stands wins
    ("chr1:1-6", (0, 0, 6)),
    ("chr1:1-5:2-3", (3, 1, 3)),
])
def test_every_form_of_a_region(parse, text, want):
    rc, got, err = parse(text)
    assert rc == 0 and got == [want], (got, err)


def test_regions_add_up_and_merge(parse):
    rc, got, err = parse("chr2:10-20", "chr1:5-8", "chr2:15-30", "chr2:31-40", "chr2:50-60", "chrM")
    assert rc == 0, err
    assert got == [(0, 4, 8), (1, 9, 40), (1, 49, 60), (4, 0, END)]       # sorted, overlapping and touching ones merged


def test_a_bed_file_with_comments_and_overlapping_lines(parse, tmp_path):
    bed = tmp_path / "x.bed"
    bed.write_text("# a comment\ntrack name=x\nbrowser position chr1:1-10\n\nchr2\t100\t200\tname\t0\t+\nchr2\t150\t300\n"
                   "chr1\t0\t10\r\nHLA:A\t5\t5\nchr2\t1000\t2000\n")
    rc, got, err = parse("--bed", str(bed))
    assert rc == 0, err
    assert got == [(0, 0, 10), (1, 100, 300), (1, 1000, 2000)]             # 0-based half open; the empty interval is none
    rc, got, err = parse("--bed", str(bed), "chr2:301-400", "chrM:7")      # the file adds to --region
    assert rc == 0 and got == [(0, 0, 10), (1, 100, 400), (1, 1000, 2000), (4, 6, END)], err


@pytest.mark.parametrize("args,words", [
    (["chr9"], ["chr9", "no reference"]),
    (["chr9:1-5"], ["chr9:1-5", "no reference"]),
    (["chr2:0-5"], ["chr2:0-5", "BEG", "at least 1"]),
    (["chr2:-5"], ["chr2:-5", "BEG"]),
    (["chr2:9-5"], ["chr2:9-5", "END", "below"]),
    (["chr2:x-5"], ["chr2:x-5", "BEG"]),
    (["chr2:5-y"], ["chr2:5-y", "END"]),
    (["chr2:"], ["chr2:", "BEG"]),
])
def test_a_bad_region_is_refused_with_its_text(parse, args, words):
    rc, got, err = parse(*args)
    assert rc == 1 and got == [] and all(w in err for w in words), err


@pytest.mark.parametrize("line,words", [
    ("chr2\t100", ["fewer than three"]),
    ("chr2 100 200", ["fewer than three"]),
    ("chr2\tabc\t200", ["not numbers"]),
    ("chr2\t100\t2e3", ["not numbers"]),
    ("chr2\t-1\t200", ["not numbers"]),
    ("chr9\t1\t2", ["no reference", "chr9"]),
    ("chr2\t9\t5", ["below"]),
])
def test_a_bad_bed_line_is_refused_with_its_text(parse, tmp_path, line, words):
    bed = tmp_path / "bad.bed"
    bed.write_text("chr1\t1\t2\n" + line + "\n")
    rc, got, err = parse("--bed", str(bed))
    assert rc == 1 and got == [] and line in err and "line 2" in err and all(w in err for w in words), err


def test_a_missing_bed_file_is_refused(parse, tmp_path):
    rc, got, err = parse("--bed", str(tmp_path / "none.bed"))
    assert rc == 1 and "none.bed" in err


# ---- the binary
def run_bin(args, cwd, **kw):
    return subprocess.run([BIN, *args], capture_output=True, timeout=600, cwd=cwd, **kw)


def test_the_binary_refuses_before_anything_is_opened_or_written(tmp_path):
    fa, bam = write_fixture(tmp_path)
    bed = tmp_path / "bad.bed"
    bed.write_text("c0\t1\n")
    work = tmp_path / "work"
    work.mkdir()
    common = ["--reference", str(fa), "--bam", str(bam)]
    cases = [
        (["smooth", *common, "--region", "nope", "--write-index", "o.bai", "--index", "i.fmd", "--sfs", "o.sfs"], b"nope"),
        (["smooth", *common, "--region", "c0:0-5"], b"c0:0-5"),
        (["smooth", *common, "--region", "c0:1-5", "--region", "c1:9-5"], b"c1:9-5"),          # the second of two
        (["smooth", *common, "--regions-file", str(bed)], b"c0\t1"),
        (["call", *common, "--sfs", "in.sfs", "--poa", "o.sam", "--clusters", "o.txt", "--region", "c7"], b"c7"),
        (["run", *common, "--index", "i.fmd", "--sfs", "o.sfs", "--smoothed", "o.bam", "--region", "c0:x"], b"c0:x"),
        (["search", "--index", "i.fmd", "--bam", str(bam), "--region", "c0:3-2"], b"c0:3-2"),
        (["search", "--index", "i.fmd", "--fastx", "reads.fq", "--region", "c0"], b"--fastx"),
        (["search", "--index", "i.fmd", "--fastx", "reads.fq", "--regions-file", str(bed)], b"--fastx"),
        (["index", "-d", str(fa), "-o", "o.fmd", "--region", "c0"], b"index"),
        (["index", "-d", str(fa), "-o", "o.fmd", "--regions-file=" + str(bed)], b"index"),
    ]
    for args, word in cases:
        r = run_bin(args, work)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
        assert b"region" in r.stderr
        assert r.stdout == b"" and os.listdir(work) == [], (args, os.listdir(work))


def test_the_usage_texts_name_the_options():
    for cmd in ("smooth", "search", "call", "run"):
        r = subprocess.run([BIN, cmd, "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "--region <REG>" in r.stderr and "--regions-file <BED>" in r.stderr, cmd


def test_smooth_of_a_region_is_smooth_of_the_subset_bam(tmp_path, exe):   # noqa: F811
    """SVDSS_SMOOTH_HOST=1 (set by the suite where there is no GPU; set here in any case): BamReader applies the record
    test.  The inflated stream is that of `smooth` on the subset BAM -- the --accp percentile taken over the subset alone
    -- with an index beside the input, without one, with a stale one; --write-index indexes the file actually written."""
    fa, bam = write_fixture(tmp_path)
    data = bam.read_bytes()
    env = dict(os.environ, SVDSS_SMOOTH_HOST="1")
    bed = tmp_path / "r.bed"
    bed.write_text("# two lines that overlap\nc0\t130000\t150000\nc0\t140000\t160000\n")
    args = ["--region", "c0:20,001-60,000", "--region", "c1:30001-", "--regions-file", str(bed)]
    intervals = [(0, 20000, 60000), (1, 30000, 2**31 - 1), (0, 130000, 160000)]
    sub, n_in, n_all = R.subset_bam(data, intervals)
    assert 0.05 * n_all <= n_in <= 0.60 * n_all, (n_in, n_all)
    (tmp_path / "sub.bam").write_bytes(sub)
    r = smooth(fa, tmp_path / "sub.bam", tmp_path / "want.bam", "--accp", "0.9", env=env)
    assert r.returncode == 0, r.stderr.decode()
    want = R.inflate((tmp_path / "want.bam").read_bytes())
    whole = tmp_path / "whole.bam"
    assert smooth(fa, bam, whole, "--accp", "0.9", env=env).returncode == 0
    assert R.inflate(whole.read_bytes()) != want
    for tag in ("no index", "bai", "csi", "stale bai"):
        for ext in (".bai", ".csi"):
            if os.path.exists(str(bam) + ext):
                os.remove(str(bam) + ext)
        if tag == "bai":
            (tmp_path / "in.bam.bai").write_bytes(R.bam_writer.bai(data))
        elif tag == "csi":
            (tmp_path / "in.bam.csi").write_bytes(R.bam_writer.csi(data))
        elif tag == "stale bai":
            (tmp_path / "in.bam.bai").write_bytes(R.bam_writer.bai(data))
            old = os.path.getmtime(bam) - 100
            os.utime(tmp_path / "in.bam.bai", (old, old))
        out = tmp_path / "got.bam"
        r = smooth(fa, bam, out, "--accp", "0.9", *args, "--verbose", "--write-index", str(tmp_path / "got.bam.bai"), env=env)
        assert r.returncode == 0, (tag, r.stderr.decode())
        # which index the command found (the host reader itself reads the whole file whatever the ranges are)
        err = r.stderr.decode()
        assert ("older than" in err and "in.bam.bai" in err) == (tag == "stale bai"), (tag, err)
        assert ("no usable index" in err) == (tag in ("no index", "stale bai")), (tag, err)
        if tag in ("bai", "csi"):
            assert "range(s) of" in err and ("in.bam." + tag) in err, (tag, err)
        assert "host reader(s) read the WHOLE file" in err, (tag, err)        # ... and says so
        assert R.inflate(out.read_bytes()) == want, tag
        check_index(exe, tmp_path, out, tmp_path / "got.bam.bai", n_queries=40)
    # the empty subset and the whole file
    none = tmp_path / "none.bam"
    assert smooth(fa, bam, none, "--region", "c2:19,999,999", env=env).returncode == 0
    assert R.split(R.inflate(none.read_bytes()))[1] == []
    every = tmp_path / "every.bam"
    assert smooth(fa, bam, every, "--accp", "0.9", "--region", "c0", "--region", "c1", "--region", "c2", env=env).returncode == 0
    assert R.inflate(every.read_bytes()) == R.inflate(whole.read_bytes())
