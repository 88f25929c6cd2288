"""The block plan of the rld0 (`.fmd`) encoder as a rule (svdss_amd/csrc/rld0_plan.h, shared by the host, the device
encoder csrc/rld0_dev.hip and tests/native/rld0_plan_dump.cpp) against the independent Python encoder of
tests/rld0_py.py: block starts, header types and headers -- the data words as a whole -- block by block and in tiles
(tables, the one walker, the tiles' own walks: the stages the device runs as kernels), with the format's piece length
and with a tiny one so that short blocks occur at small n; the exact fits; the decline rule; and
svdss_fmd_encode(device=-1) against the writer it wraps.  No GPU."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

import svdss_amd
from svdss_amd import synth
from tests import rld0_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "native", "_rld0_plan_dump.so")
_SRC = [os.path.join(ROOT, "tests", "native", "rld0_plan_dump.cpp"), os.path.join(ROOT, "svdss_amd", "csrc", "rld0_plan.h"),
        os.path.join(ROOT, "svdss_amd", "csrc", "fmd_layout.h")]


@pytest.fixture(scope="module")
def dump():
    if not (os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in _SRC)):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", _SO, _SRC[0]])
    so = C.CDLL(_SO)
    so.rld0_dump_code_width.argtypes = [C.c_int64]
    so.rld0_dump_next_type.argtypes = [C.c_int64]
    so.rld0_dump_declines.argtypes = [C.c_int64, C.c_int64]
    so.rld0_dump_short.argtypes = [C.c_int64, C.c_int64]
    so.rld0_dump_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    return so


def _encoder_with_piece(piece_words):
    """tests/rld0_py.encode_rld0 with another piece length: its own source, the one constant replaced."""
    if piece_words == 1 << 23:
        return rld0_py.encode_rld0
    src = inspect.getsource(rld0_py.encode_rld0)
    assert src.count("lsize = 1 << 23") == 1
    ns = {"np": np, "struct": struct, "_delta": rld0_py._delta}
    exec(src.replace("lsize = 1 << 23", f"lsize = {piece_words}"), ns)
    return ns["encode_rld0"]


def plan(dump, lens, syms, piece_words=1 << 23, tile=0, decline=1 << 30):
    lens = np.ascontiguousarray(lens, np.int64)
    syms = np.ascontiguousarray(syms, np.uint8)
    R = len(lens)
    desc = np.zeros(R + 2, np.int64)
    words = np.zeros(8 * (R + 1), np.uint64)
    k, nb = C.c_int64(0), C.c_int64(0)
    flags = dump.rld0_dump_encode(lens.ctypes.data, syms.ctypes.data, R, piece_words, tile, decline, desc.ctypes.data,
                                  words.ctypes.data, C.byref(k), C.byref(nb))
    assert flags >= 0
    return flags, words[:k.value], desc[:nb.value + 1]


def py_words(lens, syms, piece_words=1 << 23):
    raw = _encoder_with_piece(piece_words)(np.repeat(np.asarray(syms, np.uint8), np.asarray(lens, np.int64)))
    k = struct.unpack_from("<Q", raw, 8)[0]
    return np.frombuffer(raw, np.uint64, k, 72)


def random_runs(seed, n_runs, long_share):
    """maximal runs: neighbouring symbols differ; lengths mostly 1, some up to 40 / 5,000, a share at 0x4000 and above"""
    rng = np.random.default_rng(seed)
    syms = np.zeros(n_runs, np.uint8)
    syms[0] = rng.integers(0, 6)
    step = rng.integers(1, 6, n_runs)
    for i in range(1, n_runs):
        syms[i] = (syms[i - 1] + step[i]) % 6
    kind = rng.random(n_runs)
    lens = np.ones(n_runs, np.int64)
    lens[kind > 0.6] = rng.integers(1, 41, int((kind > 0.6).sum()))
    lens[kind > 0.9] = rng.integers(41, 5001, int((kind > 0.9).sum()))
    big = kind > 1.0 - long_share
    lens[big] = rng.integers(0x4000, 0x9000, int(big.sum()))
    return lens, syms


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("tile", [0, 96, 128, 4096])
def test_plan_reproduces_the_python_encoder(dump, seed, tile):
    lens, syms = random_runs(seed, 3000, 0.004)
    assert (lens >= 0x4000).any()
    flags, words, desc = plan(dump, lens, syms, tile=tile)
    assert flags == 0
    want = py_words(lens, syms)
    assert (desc >> 62).max() == 1          # type-1 blocks occur
    assert len(words) == len(want) and (words == want).all()


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("piece_words,tile", [(64, 0), (64, 96), (64, 128), (16, 96), (256, 4096), (128, 128)])
def test_plan_with_a_tiny_piece_length(dump, seed, piece_words, tile):
    """short blocks (the last of a piece: one word less) at small n, in the tiles' walker and in their own walks"""
    lens, syms = random_runs(100 + seed, 2500, 0.004)
    flags, words, desc = plan(dump, lens, syms, piece_words=piece_words, tile=tile)
    assert flags == 0
    assert len(desc) - 1 > piece_words // 8
    assert any(dump.rld0_dump_short(b, piece_words) for b in range(len(desc) - 1))
    want = py_words(lens, syms, piece_words)
    assert len(words) == len(want) and (words == want).all()


def starts_of(desc):
    return (desc & ((1 << 48) - 1)).tolist(), (desc >> 62).tolist()


def cycle(n):
    return np.ones(n, np.int64), (np.arange(n) % 4 + 1).astype(np.uint8)


@pytest.mark.parametrize("tile", [0, 96])
def test_exact_fits(dump, tile):
    # 96 one-symbol runs fill a type-0 block (6 words, 4 bits a code), the 97th starts the next
    assert dump.rld0_dump_code_width(1) == 4 and dump.rld0_dump_cap(0, 0) == 384
    lens, syms = cycle(97)
    _, words, desc = plan(dump, lens, syms, tile=tile)
    assert starts_of(desc) == ([0, 96, 97], [0, 0, 0])
    assert (words == py_words(lens, syms)).all()
    # 95 ones, then a 2 (7 bits): 380 + 7 > 384, the break is after 95
    lens, syms = cycle(100)
    lens[95] = 2
    assert dump.rld0_dump_code_width(2) == 7
    _, words, desc = plan(dump, lens, syms, tile=tile)
    assert starts_of(desc)[0][:2] == [0, 95]
    assert (words == py_words(lens, syms)).all()
    # a type-1 block (4 header words) holds 64 one-symbol runs
    lens, syms = cycle(200)
    lens[0] = 0x4000
    _, words, desc = plan(dump, lens, syms, tile=tile)
    r, t = starts_of(desc)
    assert t[:3] == [0, 1, 0] and r[2] - r[1] == 64 and dump.rld0_dump_cap(1, 0) == 256
    assert (words == py_words(lens, syms)).all()


def test_type_thresholds_and_short_blocks(dump):
    assert [dump.rld0_dump_next_type(s) for s in (0x3fff, 0x4000, (1 << 30) - 1, 1 << 30)] == [0, 1, 1, 2]
    pb = (1 << 23) // 8
    assert [dump.rld0_dump_short(b, 1 << 23) for b in (pb - 2, pb - 1, pb, 2 * pb - 1)] == [0, 1, 0, 1]
    assert dump.rld0_dump_cap(0, 1) == 320 and dump.rld0_dump_cap(1, 1) == 192
    # the issue's width rule
    for l in (1, 2, 3, 4, 7, 8, 1023, 1024, 0x4000, (1 << 30) - 1):
        y = l.bit_length() - 1
        assert dump.rld0_dump_code_width(l) == 2 * ((y + 1).bit_length() - 1) + 1 + y + 3 == len(rld0_py._delta(l)) + 3


def test_decline_rule_fires_at_its_threshold(dump):
    assert dump.rld0_dump_declines(999, 1000) == 0 and dump.rld0_dump_declines(1000, 1000) == 1
    assert dump.rld0_dump_declines((1 << 30) - 1, 1 << 30) == 0 and dump.rld0_dump_declines(1 << 30, 1 << 30) == 1
    for tile in (0, 96):
        lens, syms = cycle(300)
        lens[150] = 2000
        assert plan(dump, lens, syms, tile=tile, decline=1000)[0] == 1
        # a block's TOTAL counts, not its longest run: 904 + 95 ones stay below, one more symbol in the run does not
        lens[150] = 100
        first = plan(dump, lens, syms, tile=tile)[2] & ((1 << 48) - 1)
        b = int(np.searchsorted(first, 150, side="right")) - 1
        total = int(lens[first[b]:first[b + 1]].sum())
        assert plan(dump, lens, syms, tile=tile, decline=total + 1)[0] == 0
        assert plan(dump, lens, syms, tile=tile, decline=total)[0] == 1


def test_fmd_encode_on_the_host_writes_the_writers_bytes(tmp_path, monkeypatch):
    """svdss_fmd_encode(device=-1) is rld0_write: the bytes FMDIndex.save_fmd writes on the host, which are the Python
    encoder's"""
    monkeypatch.setenv("SVDSS_INDEX_CPU", "1")
    ref = synth.make_reference([30000, 9000, 40], seed=1, repeat_frac=0.3, n_runs=(700, 20))
    ref.append(np.full(5000, 1, np.uint8))
    ref.append(np.full(40000, 5, np.uint8))
    ix = svdss_amd.FMDIndex.build(ref, threads=4)
    ix.save_fmd(str(tmp_path / "a.fmd"), device=-1)
    assert svdss_amd.fmd_encode_last()["route"] == "host"
    svdss_amd.fmd_encode(ix.bwt(), str(tmp_path / "b.fmd"), -1)
    last = svdss_amd.fmd_encode_last()
    assert last["route"] == "host" and last["runs"] == 0
    a, b = open(tmp_path / "a.fmd", "rb").read(), open(tmp_path / "b.fmd", "rb").read()
    assert a == b == rld0_py.encode_rld0(ix.bwt())
    # forced onto the device without one: declined as a whole, the same bytes from the host
    ix.save_fmd(str(tmp_path / "c.fmd"), device=0)
    assert svdss_amd.fmd_encode_last()["route"] == "declined, no GPU"
    assert open(tmp_path / "c.fmd", "rb").read() == a
    # unset, SVDSS_FMD_ENCODE_DEVICE means the device (profiles/fmd_encode.txt); 0 asks for the host
    monkeypatch.delenv("SVDSS_FMD_ENCODE_DEVICE", raising=False)
    ix.save_fmd(str(tmp_path / "d.fmd"))
    assert svdss_amd.fmd_encode_last()["route"] == "declined, no GPU"
    monkeypatch.setenv("SVDSS_FMD_ENCODE_DEVICE", "0")
    ix.save_fmd(str(tmp_path / "e.fmd"))
    assert svdss_amd.fmd_encode_last()["route"] == "host"
    assert open(tmp_path / "d.fmd", "rb").read() == a and open(tmp_path / "e.fmd", "rb").read() == a
