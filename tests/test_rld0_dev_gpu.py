"""The rld0 (`.fmd`) encoder on the device (csrc/rld0_dev.hip) against the host encoder (csrc/rld0.cpp): every case
compares the two files byte for byte and -- unless it is the decline case -- asserts through fmd_encode_last() that the
device path ran: a decline must not hide a failure, and no input here makes the host rule alone decline."""
import struct

import numpy as np
import pytest

import svdss_amd
from svdss_amd import synth

pytestmark = pytest.mark.gpu

A, C_, G, T, N = 1, 2, 3, 4, 5


def both(tmp_path, bwt, expect="device"):
    """the .fmd of bwt from the device and from the host; asserts the route and the bytes, returns (bytes, last)"""
    bwt = np.ascontiguousarray(bwt, np.uint8)
    svdss_amd.fmd_encode(bwt, str(tmp_path / "dev.fmd"), 0)
    last = svdss_amd.fmd_encode_last()
    assert last["route"] == expect, last
    svdss_amd.fmd_encode(bwt, str(tmp_path / "host.fmd"), -1)
    assert svdss_amd.fmd_encode_last()["route"] == "host"
    dev, host = open(tmp_path / "dev.fmd", "rb").read(), open(tmp_path / "host.fmd", "rb").read()
    assert len(dev) == len(host)
    if dev != host:
        a, b = np.frombuffer(dev, np.uint8), np.frombuffer(host, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"first difference at byte {at} (data word {(at - 72) // 8}, block {(at - 72) // 64}) of {len(dev)}")
    return dev, last


def headers(raw, first, count):
    """(type, symbols of the block before) of the headers of blocks first .. first + count - 1"""
    out = []
    for b in range(first, first + count):
        w = struct.unpack_from("<4Q", raw, 72 + 64 * b)
        if w[0] >> 62:
            out.append((1, w[0] & 0x3fffffff))
        else:
            out.append((0, w[0] & 0xffff))
    return out


def cycle(n, shift=0):
    return ((np.arange(n, dtype=np.int64) + shift) % 4 + 1).astype(np.uint8)


def from_runs(lens, syms):
    return np.repeat(np.asarray(syms, np.uint8), np.asarray(lens, np.int64))


def test_known_answer(tmp_path):
    """T A A A $ T T $ (tests/test_rld0.py derives the words by hand)"""
    raw, last = both(tmp_path, [4, 1, 1, 1, 0, 4, 4, 0])
    k, = struct.unpack_from("<Q", raw, 8)
    words = struct.unpack_from(f"<{k}Q", raw, 72)
    assert k == 10 and words[2] >> (64 - 26) == 0b11000101001100001001001000
    assert (last["runs"], last["blocks"], last["pieces"]) == (5, 1, 1)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129])
def test_run_carries_across_words_and_rank_blocks(tmp_path, n):
    rng = np.random.default_rng(n)
    # runs that straddle symbols 31|32 and 127|128, single symbols, and one run of everything
    both(tmp_path, np.repeat(rng.integers(0, 6, n // 3 + 1), 3)[:n])
    both(tmp_path, rng.integers(0, 6, n))
    both(tmp_path, np.full(n, rng.integers(0, 6)))


@pytest.mark.parametrize("sym", [0, 3, 5])
def test_one_run_of_the_whole_array(tmp_path, sym):
    _, last = both(tmp_path, np.full(1_000_003, sym, np.uint8))
    assert (last["runs"], last["blocks"]) == (1, 1)


def random_bwt(seed, n, mix):
    rng = np.random.default_rng(seed)
    n_runs = n                                     # more than enough; cut to n symbols below
    top = {"ones": 1, "upto40": 40, "upto5000": 5000, "long": 40}[mix]
    lens = np.ones(n_runs, np.int64)
    if top > 1:
        some = rng.random(n_runs) < (0.5 if mix != "upto5000" else 0.05)
        lens[some] = rng.integers(1, top + 1, int(some.sum()))
    if mix == "ones":
        some = rng.random(n_runs) < 0.1
        lens[some] = rng.integers(2, 5, int(some.sum()))
    if mix == "long":
        some = rng.random(n_runs) < 2e-4
        lens[some] = rng.integers(0x4000, 0x20000, int(some.sum()))
    keep = int(np.searchsorted(np.cumsum(lens), n)) + 1
    lens = lens[:keep]
    syms = np.cumsum(rng.integers(1, 6, keep)) % 6   # neighbours differ: the runs are maximal
    return from_runs(lens, syms)[:n]


@pytest.mark.parametrize("tile", [128, None])
@pytest.mark.parametrize("mix", ["ones", "upto40", "upto5000", "long"])
def test_random_run_length_mixes(tmp_path, monkeypatch, mix, tile):
    if tile:
        monkeypatch.setenv("SVDSS_FMD_TILE_RUNS", str(tile))
    bwt = random_bwt(7, 2_000_003, mix)
    raw, last = both(tmp_path, bwt)
    assert last["runs"] == 1 + int((bwt[1:] != bwt[:-1]).sum())
    assert last["runs"] > 4096 * 4 or mix == "upto5000"        # the chain crosses many tiles
    if mix == "long":
        assert any(t for t, _ in headers(raw, 1, last["blocks"]))


@pytest.mark.parametrize("grid", [1, 3])
def test_items_beyond_the_grid(tmp_path, monkeypatch, grid):
    """Every kernel walks its items in a grid-stride loop, because a launch of 2^32 work-items or more -- the 4.6e9 runs of a
    3.1 Gb reference -- wraps without an error (tools/fmd_encode_bench.py compares the files at that size).  Here the grid is
    capped at a few workgroups instead, so that every lane takes many items."""
    monkeypatch.setenv("SVDSS_FMD_GRID_BLOCKS", str(grid))
    monkeypatch.setenv("SVDSS_FMD_TILE_RUNS", "128")
    _, last = both(tmp_path, random_bwt(11, 1_000_003, "upto40"))
    assert last["runs"] > 256 * grid * 4 and last["blocks"] > 256 * grid


@pytest.mark.parametrize("items", [2, 1000])
def test_scans_in_several_chunks(tmp_path, monkeypatch, items):
    """Both scans (first run of every quarter, prefix sums of the widths) go chunk by chunk where hipcub's int cannot count
    the items -- past 2^30, the runs of a human genome's BWT -- and k_carry hands the total on.  Here the chunk is a few
    items, so that the quarters' counts and the widths both take many chunks (items = 2: a carry at every other item)."""
    monkeypatch.setenv("SVDSS_FMD_SCAN_ITEMS", str(items))
    n = 4_003 if items == 2 else 400_009
    _, last = both(tmp_path, random_bwt(13, n, "upto40"))
    assert last["runs"] > 4 * items and n // 32 > 4 * items


def test_decline_memory(tmp_path, monkeypatch):
    """a plan that does not fit in free HBM (SVDSS_FMD_HBM_LIMIT_MB: as if no more were free): declined as a whole where the
    quarters' counts are asked for and where the runs are, the host's bytes; with room for all of it, the device"""
    bwt = random_bwt(17, 2_000_003, "ones")            # 0.5 MB of counts, ~28 MB of runs, each with 64 MB to spare
    for mb in (0, 70):
        monkeypatch.setenv("SVDSS_FMD_HBM_LIMIT_MB", str(mb))
        both(tmp_path, bwt, expect="declined, memory")
    monkeypatch.setenv("SVDSS_FMD_HBM_LIMIT_MB", "200")
    both(tmp_path, bwt)


def test_chain_that_crosses_no_tile(tmp_path):
    _, last = both(tmp_path, random_bwt(3, 5000, "upto40"))
    assert last["runs"] < 4096


def test_exact_fits_at_tile_edges(tmp_path, monkeypatch):
    monkeypatch.setenv("SVDSS_FMD_TILE_RUNS", "96")
    # 96 one-symbol runs fill a block: every block ends with a tile's last run, the 97th run is the next tile's first
    raw, last = both(tmp_path, cycle(500))
    assert headers(raw, 1, 5) == [(0, 96)] * 5
    # 95 ones, then a 2: the break is after 95 -- the next block starts with tile 0's last run
    lens = np.ones(500, np.int64)
    lens[95] = 2
    raw, _ = both(tmp_path, from_runs(lens, cycle(500)))
    assert headers(raw, 1, 2) == [(0, 95), (0, 96)]            # (the 2 and 94 ones: 7 + 376 bits)
    # a type-1 block holds 64 one-symbol runs; it starts with a tile's first run (runs 0-95 | N x 0x4000 + 90 | 64 | ...)
    monkeypatch.setenv("SVDSS_FMD_TILE_RUNS", "187")
    lens, syms = np.ones(500, np.int64), cycle(500)
    lens[96], syms[96] = 0x4000, N
    raw, _ = both(tmp_path, from_runs(lens, syms))
    assert headers(raw, 1, 4) == [(0, 96), (1, 0x4000 + 90), (0, 64), (0, 96)]


def test_block_of_0x3fff_and_of_0x4000_symbols(tmp_path):
    """a 23-bit code + 90 ones fill 383 of 384 bits: the block's total decides the next header's type"""
    for first, typ in ((0x3fff - 90, 0), (0x4000 - 90, 1)):
        lens, syms = np.ones(400, np.int64), cycle(400)
        lens[0], syms[0] = first, N
        raw, _ = both(tmp_path, from_runs(lens, syms))
        assert headers(raw, 1, 1) == [(typ, first + 90)]


PIECE_BLOCKS = 1 << 20


@pytest.mark.parametrize("variant", ["plain", "type1", "shifted"])
def test_piece_end(tmp_path, variant):
    """The smallest shape that reaches the end of a piece of 2^23 words: a cycle of A C G T (every code 4 bits), 96 runs
    per block, so block 2^20 - 1 -- one word short -- holds 80; with N x 0x4000 in the block before it, it carries a
    type-1 header and holds 48."""
    n = (PIECE_BLOCKS - 1) * 96 + 80 + 1000
    bwt = cycle(n)
    want = (0, 80)
    if variant == "type1":
        at = (PIECE_BLOCKS - 2) * 96
        bwt = np.concatenate([bwt[:at], np.full(0x4000, N, np.uint8), bwt[at:]])
        want = (0, 48)
    if variant == "shifted":
        bwt = np.concatenate([np.zeros(1, np.uint8), bwt[:-1]])
    raw, last = both(tmp_path, bwt)
    assert last["pieces"] == 2 and last["blocks"] > PIECE_BLOCKS
    h = headers(raw, PIECE_BLOCKS - 1, 3)
    assert h[1] == want                                    # block 2^20's header: the short block's symbols
    assert h[0] == ((1, 0x4000 + 90) if variant == "type1" else (0, 96))
    assert h[2] == (0, 96)


def test_decline_block_total(tmp_path, monkeypatch):
    monkeypatch.setenv("SVDSS_FMD_DECLINE_SYMS", "1000")
    lens, syms = np.ones(3000, np.int64), cycle(3000)
    lens[1500] = 2000
    both(tmp_path, from_runs(lens, syms), expect="declined, block total")
    monkeypatch.setenv("SVDSS_FMD_DECLINE_SYMS", "2200")   # ... and not a symbol earlier: 2,000 + 95 ones at most
    both(tmp_path, from_runs(lens, syms))


def test_index_saved_from_its_resident_blocks(tmp_path, monkeypatch):
    ref = synth.make_reference([30000, 9000, 40], seed=1, repeat_frac=0.3, n_runs=(700, 20))
    ref.append(np.full(5000, 1, np.uint8))
    ref.append(np.full(40000, 5, np.uint8))
    ix = svdss_amd.FMDIndex.build(ref, device=0)
    monkeypatch.setenv("SVDSS_FMD_ENCODE_DEVICE", "1")
    ix.save_fmd(str(tmp_path / "dev.fmd"))
    assert svdss_amd.fmd_encode_last()["route"] == "device"
    monkeypatch.setenv("SVDSS_FMD_ENCODE_DEVICE", "0")
    ix.save_fmd(str(tmp_path / "host.fmd"))
    assert svdss_amd.fmd_encode_last()["route"] == "host"
    ix.save_fmd(str(tmp_path / "dev2.fmd"), device=0)
    assert svdss_amd.fmd_encode_last()["route"] == "device"
    raw = open(tmp_path / "host.fmd", "rb").read()
    assert open(tmp_path / "dev.fmd", "rb").read() == raw and open(tmp_path / "dev2.fmd", "rb").read() == raw
    # a handle on the host uploads its blocks first
    host_ix = svdss_amd.FMDIndex.build(ref)
    host_ix.save_fmd(str(tmp_path / "dev3.fmd"), device=0)
    assert svdss_amd.fmd_encode_last()["route"] == "device"
    assert open(tmp_path / "dev3.fmd", "rb").read() == raw
    from tests.test_rld0 import read_bwt
    assert (read_bwt(tmp_path / "dev.fmd") == ix.bwt()).all()
