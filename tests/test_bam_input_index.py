"""The index of the INPUT BAM without a GPU (`SVDSS bamindex` through the host reader, SVDSS_BAM_DEVICE=0; the input-side fold
of csrc/bam_index_writer.h through tests/native/input_index_fold.cpp): bins, chunks, linear index and loffset against the test
writer's own BAI / CSI, pseudo-bin counts and n_no_coor against the file's own, region queries through the product's reader
(csrc/bai_index.h), the fold of batches / regions / seams against the host reader byte for byte, and what the command line
refuses.  tests/test_bam_input_index_gpu.py holds the device path against the files checked here."""
import os
import subprocess

import pytest

from tests import bam_input_index_lib as L
from tests.common import BIN, ROOT
from tests.test_smooth_index import bam_with_text, exe, fixture_records, parse_index  # noqa: F401  (exe: the fixture that builds _bai_scan)

FOLD_SRC = os.path.join(ROOT, "tests", "native", "input_index_fold.cpp")
FOLD_EXE = os.path.join(ROOT, "tests", "native", "_input_index_fold")
HOST = {"SVDSS_BAM_DEVICE": "0"}


@pytest.fixture(scope="module")
def fold_exe():
    deps = [FOLD_SRC] + [os.path.join(ROOT, "svdss_amd", "csrc", h) for h in ("bam_index_writer.h", "bam_writer.h")]
    if not os.path.exists(FOLD_EXE) or os.path.getmtime(FOLD_EXE) < max(map(os.path.getmtime, deps)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", FOLD_EXE, FOLD_SRC, "-lz", "-ldl"], check=True)
    return FOLD_EXE


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("inix_cpu")
    files = L.write_files(tmp)
    out = {}
    for tag, bam in files.items():
        for ext in ("bai", "csi"):
            out[tag, ext] = tmp / f"{tag}.{ext}"
            r = L.bamindex(bam, out[tag, ext], "--verbose", env=L.env0(**HOST))
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            assert b"host reader" in r.stderr and not (tmp / f"{tag}.{ext}.tmp").exists()
    return {"tmp": tmp, "files": files, "out": out}


def test_the_fixture_holds_what_it_should(fx):
    data = fx["files"]["b60000"].read_bytes()
    recs, lens = L.records(data)
    assert lens == [l for _, l in L.REFS]
    assert sum(1 for r in recs if r[1] < 0) == 40 and all(r[1] < 0 for r in recs[-40:])
    assert not any(r[1] == 3 for r in recs)                                      # a reference with no record
    assert sum(1 for r in recs if r[1] >= 0 and r[4] & 4) == 6                   # flag 4 and a position
    assert any(r[4] & 256 for r in recs) and any(r[4] & 2048 for r in recs)
    assert any(r[1] == 0 and r[2] == 0 for r in recs)
    by_name = {r[0]: r for r in recs}
    assert by_name["ends_at_window"][3] == 3 * L.WIN and by_name["ends_one_past_window"][3] == 3 * L.WIN + 1
    assert (by_name["five_windows"][3] - 1) // L.WIN - by_name["five_windows"][2] // L.WIN == 4
    assert by_name["no_cigar"][3] == by_name["no_cigar"][2] + 1
    assert by_name["cigar70k"][3] == 270000
    # blocks of 997: records that start and records that end on member boundaries; two empty members inside the third file
    from tests.test_smooth_index import members
    small = fx["files"]["b997"].read_bytes()
    bounds = {u for c, u, n in members(small)[0]}
    srecs, _ = L.records(small)
    assert sum(1 for r in srecs if r[5] in bounds) >= 20 and sum(1 for r in srecs if r[6] in bounds) >= 20
    blocks = members(fx["files"]["concat"].read_bytes())[0]
    assert sum(1 for c, u, n in blocks[:-1] if n == 0) == 2


@pytest.mark.parametrize("tag", ["b60000", "b997", "concat"])
@pytest.mark.parametrize("ext", ["bai", "csi"])
def test_host_reader_against_the_python_indexer_and_by_queries(fx, exe, tag, ext):   # noqa: F811
    idx = fx["out"][tag, ext]
    got = parse_index(idx.read_bytes())
    assert got["csi"] == (ext == "csi") and got["depth"] == 5 and got["n_no_coor"] == 40
    L.check_input_index(exe, fx["files"][tag], idx, n_queries=200, seed=len(tag))


@pytest.mark.parametrize("tag,cuts", [("b60000", ["1000000"]), ("b60000", ["7"]), ("b60000", ["1"]), ("b60000", ["3", "20", "41"]),
                                      ("b60000", ["5", "10", "30", "50", "60"]), ("b997", ["1"]), ("b997", ["64", "1500", "1501", "3000"]),
                                      ("concat", ["4"]), ("concat", ["2", "24", "27", "28", "29"])])
def test_the_fold_of_batches_regions_and_seams_gives_the_same_bytes(fx, fold_exe, tag, cuts):
    """batches of a few members (records straddle them; at one member of 997 bytes per batch every record is carried over many
    turns), regions cut anywhere (a seam completes the record that straddles each cut), empty members first in a batch"""
    for ext in ("bai", "csi"):
        out = fx["tmp"] / f"fold.{ext}"
        r = subprocess.run([fold_exe, str(fx["files"][tag]), str(out), *cuts], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == fx["out"][tag, ext].read_bytes(), (tag, ext, cuts)


def test_an_unsorted_bam_is_refused_and_leaves_no_file(fx, fold_exe):
    from tests.test_bam_input_index_gpu import swap_two_records
    bad = fx["tmp"] / "unsorted.bam"
    swap_two_records(fx["files"]["b60000"], bad)
    out = fx["tmp"] / "unsorted.bai"
    r = L.bamindex(bad, out, env=L.env0(**HOST))
    assert r.returncode != 0 and b"not sorted" in r.stderr
    assert not out.exists() and not (fx["tmp"] / "unsorted.bai.tmp").exists()
    r = subprocess.run([fold_exe, str(bad), str(out), "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not sorted" in r.stderr and not out.exists()
    # a record without a reference in front of one with: not sorted either
    data = fx["files"]["b60000"].read_bytes()
    from tests.test_smooth_index import members
    from tests import bam_writer
    recs, _ = L.records(data)
    _, raw = members(data)
    last, first = recs[-1], recs[10]
    moved = raw[:first[5]] + raw[last[5]:last[6]] + raw[first[5]:last[5]]
    bad.write_bytes(bam_writer.bgzf(moved, 60000))
    r = L.bamindex(bad, out, env=L.env0(**HOST))
    assert r.returncode != 0 and b"not sorted" in r.stderr and not out.exists()


def test_a_truncated_bam_leaves_no_file(fx):
    data = fx["files"]["b60000"].read_bytes()
    cut = fx["tmp"] / "cut.bam"
    cut.write_bytes(data[:len(data) // 2])
    out = fx["tmp"] / "cut.bai"
    r = L.bamindex(cut, out, env=L.env0(**HOST))
    assert r.returncode != 0 and not out.exists() and not (fx["tmp"] / "cut.bai.tmp").exists()


def _refused(cmd, words, leaves, env=None):
    before = {p: set(os.listdir(p)) for p in leaves}
    r = subprocess.run([BIN, *map(str, cmd)], capture_output=True, timeout=60, env=env or L.env0())
    assert r.returncode != 0 and r.stdout == b"", (cmd, r.stderr.decode()[-800:])
    for w in words:
        assert w.encode() in r.stderr, (cmd, w, r.stderr.decode()[-800:])
    for p in leaves:
        assert set(os.listdir(p)) == before[p], (cmd, set(os.listdir(p)) - before[p])


def test_what_the_command_line_refuses(fx, tmp_path):
    bam = fx["files"]["b60000"]
    idx = tmp_path / "x.bai"
    dirs = [tmp_path, fx["tmp"]]
    common = ["--reference", tmp_path / "ref.fa", "--bam", bam]
    (tmp_path / "ref.fa").write_text(">c0\nACGT\n")
    (tmp_path / "x.sfs").write_text("")
    # the option on any other sub-command
    for cmd in (["smooth", *common], ["search", "--index", tmp_path / "r.fmd", "--bam", bam], ["bamindex", "--bam", bam],
                ["index", "-d", tmp_path / "ref.fa", "-o", tmp_path / "r.fmd"]):
        _refused([*cmd, "--write-bam-index", idx], ["--write-bam-index", "call", "run"], dirs)
    _refused(["call", *common, "--sfs", tmp_path / "x.sfs", "-o", idx], ["-o", "bamindex"], dirs)
    # together with --region / --regions-file
    bed = tmp_path / "r.bed"
    bed.write_text("c0\t0\t100\n")
    for reg in (["--region", "c0:1-100"], ["--regions-file", bed]):
        _refused(["call", *common, "--sfs", tmp_path / "x.sfs", "--write-bam-index", idx, *reg], ["--write-bam-index", "--region"], dirs)
        _refused(["run", *common, "--index", tmp_path / "r.fmd", "--write-bam-index", idx, *reg], ["--write-bam-index", "--region"], dirs)
        _refused(["bamindex", "--bam", bam, "-o", idx, *reg], ["--region"], dirs)
    # with run --samples
    lst = tmp_path / "samples.txt"
    lst.write_text(f"{bam}\t{tmp_path / 'a.vcf'}\n")
    _refused(["run", "--reference", tmp_path / "ref.fa", "--index", tmp_path / "r.fmd", "--samples", lst, "--write-bam-index", idx],
             ["--samples", "--write-bam-index"], dirs)
    # FILE equal to an input
    _refused(["call", *common, "--sfs", tmp_path / "x.sfs", "--write-bam-index", bam], ["input"], dirs)
    _refused(["call", *common, "--sfs", tmp_path / "x.sfs", "--write-bam-index", tmp_path / "x.sfs"], ["input"], dirs)
    _refused(["run", *common, "--index", tmp_path / "r.fmd", "--write-bam-index", tmp_path / "ref.fa"], ["input"], dirs)
    _refused(["bamindex", "--bam", bam, "-o", bam], ["input"], dirs)
    os.symlink(bam, tmp_path / "link.bam")
    dirs_now = [tmp_path, fx["tmp"]]
    _refused(["bamindex", "--bam", bam, "-o", tmp_path / "link.bam"], ["input"], dirs_now)
    assert bam.read_bytes()[:4] == b"\x1f\x8b\x08\x04"
    # a BAI for a reference that is too long; the CSI of the same file is written
    _, recs = fixture_records()
    big = tmp_path / "big.bam"
    big.write_bytes(bam_with_text([("c0", 300000), ("c1", 90000), ("c2", 20000), ("big", 600_000_000)], recs))
    _refused(["bamindex", "--bam", big, "-o", tmp_path / "big.bai"], [".csi", "2^29"], dirs, env=L.env0(**HOST))
    _refused(["call", "--reference", tmp_path / "ref.fa", "--bam", big, "--sfs", tmp_path / "x.sfs", "--write-bam-index", tmp_path / "big.bai"],
             [".csi", "--write-bam-index"], dirs)
    r = L.bamindex(big, tmp_path / "big.csi", env=L.env0(**HOST))
    assert r.returncode == 0 and parse_index((tmp_path / "big.csi").read_bytes())["depth"] == 6
    # no --bam: the sub-command's own usage text
    r = subprocess.run([BIN, "bamindex"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"Usage: SVDSS bamindex" in r.stderr
    r = subprocess.run([BIN, "bamindex", "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"Usage: SVDSS bamindex" in r.stderr
    for cmd in ("call", "run"):
        r = subprocess.run([BIN, cmd, "--help"], capture_output=True, timeout=60)
        assert r.returncode == 0 and b"--write-bam-index" in r.stderr


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_without_a_gpu_and_without_the_variable_bamindex_stops(fx, tmp_path):
    out = tmp_path / "x.bai"
    r = L.bamindex(fx["files"]["b60000"], out, env=L.env0())
    assert r.returncode != 0 and b"no GPU found" in r.stderr and b"SVDSS_BAM_DEVICE=0" in r.stderr
    assert not out.exists() and not (tmp_path / "x.bai.tmp").exists()
