"""csrc/gzip_stream.hip through svdss_amd.gzipdev.inflate: plain gzip files inflated chunk-parallel on the GPU give the bytes
of gzip.decompress, and the counters say that the device did it -- the plan (chunks with a start, the chain, where the unit
hands over) is the one of the pure-Python mirror (tests/mirror/gzipstream.py)."""
import functools

import pytest

from tests import gzip_cases as G
from tests.mirror import gzipstream as M

pytestmark = pytest.mark.gpu

WHOLE = 1 << 30
CHUNKS = (4096, 16384, 65536, 1 << 30)
WINDOWS = (131072, WHOLE)
# the shapes at which the mirror is run beside the device (pure Python: seconds per megabyte)
MIRRORED = {(16384, WHOLE), (4096, 131072)}


@functools.lru_cache(maxsize=None)
def mirror(name, chunk, window):
    data, _ = G.case(name)
    return M.inflate(data, chunk, window)[1]


def run(name, chunk, window):
    from svdss_amd import gzipdev
    data, text = G.case(name)
    out, st = gzipdev.inflate(data, chunk, window)
    assert out == text
    assert st["device_bytes"] + st["host_bytes"] == len(text)
    return st


def check_against_mirror(name, chunk, window, st):
    m = mirror(name, chunk, window)
    for k in ("windows", "n_chunks", "chunks_on_chain", "chunks_merged", "false_starts"):
        assert st[k] == m.stats[k], (k, st, m.stats)
    assert st["device_bytes"] == m.device_bytes            # the device went as far as it must
    assert st["declined"] == m.declined
    assert st["declined_at"] == (m.declined_at if m.declined else None)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", G.ALL)
def test_gzip_case(name, chunk, window):
    st = run(name, chunk, window)
    if (chunk, window) in MIRRORED:
        check_against_mirror(name, chunk, window, st)
    if name in ("level0", "fixed") and chunk != 1 << 30:
        # no start to find: the hand-over gives every byte, from the member's first block on
        assert st["declined"] == M.DECLINE_NO_START and st["declined_at"] == 10 and st["device_bytes"] == 0
    if name == "garbage" and window == WHOLE and chunk >= 16384:
        data, text = G.case(name)
        assert st["declined"] == M.DECLINE_TRAILING and st["declined_at"] == len(data) - 72 and st["device_bytes"] == len(text)
    if chunk == 1 << 30:
        # one chunk per window: nothing to find, the wavefront of the known start walks everything
        assert st["chunks_merged"] == 0 and st["false_starts"] == 0 and st["chunks_on_chain"] == st["windows"]
        if name != "garbage" and window == WHOLE:
            assert st["declined"] == 0 and st["host_bytes"] == 0


@pytest.mark.parametrize("name", ["fastq1", "fastq6", "fastq9"])
def test_fastq_runs_on_the_device(name):
    """the caps: a fallback cannot stand in for a dead kernel"""
    st = run(name, 65536, WHOLE)
    assert st["declined"] == 0 and st["chunks_merged"] == 0 and st["false_starts"] == 0 and st["n_chunks"] >= 12
    assert st["chunks_on_chain"] == st["n_chunks"] and st["host_bytes"] == 0 and st["members_finished"] == 1
    st = run(name, 16384, WHOLE)
    assert st["chunks_on_chain"] == mirror(name, 16384, WHOLE).stats["chunks_on_chain"]
    assert st["declined"] == 0 and st["host_bytes"] == 0


def test_false_start_only_lengthens_the_predecessor(monkeypatch):
    base = run("fastq6", 65536, WHOLE)
    monkeypatch.setenv("SVDSS_GZIP_TEST", "fake:3")
    st = run("fastq6", 65536, WHOLE)
    assert st["false_starts"] == 1 and st["declined"] == 0 and st["host_bytes"] == 0
    assert st["chunks_on_chain"] == base["chunks_on_chain"] - 1 and st["n_chunks"] == base["n_chunks"]


@pytest.mark.parametrize("shape", [(16384, 131072), (65536, WHOLE), (1 << 30, WHOLE)])
@pytest.mark.parametrize("kind", ["bitflip", "crc", "truncated"])
def test_damage_is_an_error_not_a_wrong_answer(kind, shape):
    from svdss_amd import gzipdev
    with pytest.raises(gzipdev.GzipError) as e:
        gzipdev.inflate(G.damaged(kind), *shape)
    assert e.value.code == 3 and e.value.detail


def test_not_gzip_declines_at_the_first_byte():
    from svdss_amd import gzipdev
    out, st = gzipdev.inflate(b"@read\nACGT\n+\nIIII\n", 65536, WHOLE)
    assert out == b"" and st["declined"] == M.DECLINE_HEADER and st["declined_at"] == 0 and st["windows"] == 0
