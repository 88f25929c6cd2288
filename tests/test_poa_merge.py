"""Which first-stage launches of a wave become one (poa_merge_wave / poa_merged_group of svdss_amd/csrc/poa_plan.h), on the
CPU through a binding of its own (tests/native/poa_merge_dump.cpp): the two whole-wavefront variants (64, 2) and (64, 1) of
one wave, C = 2 tasks first, ids kept, workspace offsets of the second half moved behind the first's."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "native", "_poa_merge_dump.so")
_SRC = [os.path.join(ROOT, "tests", "native", "poa_merge_dump.cpp")] + [os.path.join(ROOT, "svdss_amd", "csrc", h)
                                                                         for h in ("poa_plan.h", "poa_quad_defs.h", "poa_task.h")]


@pytest.fixture(scope="module")
def lib():
    if not (os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in _SRC)):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", _SO, _SRC[0]])
    so = C.CDLL(_SO)
    so.poa_merge_json.restype = C.c_char_p
    so.poa_merge_json.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4
    return so


def _launches(lib, groups, merge=1, g0=0, g1=None):
    """groups: (gw, cols, wave, n_tasks) each"""
    a = [np.array([g[k] for g in groups], dtype=np.int32) for k in range(4)]
    g1 = len(groups) if g1 is None else g1
    return json.loads(lib.poa_merge_json(*[x.ctypes.data for x in a], len(groups), g0, g1, merge))


def _ids(g, n):
    return [1000 * g + i for i in range(n)]


def _need(g, n):
    return sum(100 + 7 * g + i for i in range(n))


def test_the_two_whole_wavefront_variants_of_a_wave_merge(lib):
    ls = _launches(lib, [(64, 2, 0, 3), (64, 1, 0, 4)])
    assert len(ls) == 1
    m = ls[0]
    assert (m["c2"], m["c1"], m["single"], m["n2"]) == (0, 1, -1, 3)
    assert m["ids"] == _ids(0, 3) + _ids(1, 4)                                   # C = 2 first, ids as they were
    assert m["w32"] == _need(0, 3) + _need(1, 4) and m["w8"] == sum(range(10, 13)) + sum(range(10, 14))
    # every task's workspace is its own: offsets ascend by what the task before needs, the second half behind the first
    need = [100 + i for i in range(3)] + [107 + i for i in range(4)]
    assert m["ws_off"] == [sum(need[:k]) for k in range(7)]
    assert m["cons_off"] == [sum(m["nc"][:k]) for k in range(7)]
    assert m["max_len"] == 100 + 3 and m["bundle_lds"] == 12 * 13 + 64
    # the plan's order is (64, 2) before (64, 1), but the answer does not depend on it
    r = _launches(lib, [(64, 1, 0, 4), (64, 2, 0, 3)])
    assert len(r) == 1 and (r[0]["c2"], r[0]["c1"], r[0]["n2"]) == (1, 0, 3) and r[0]["ids"] == _ids(1, 3) + _ids(0, 4)


def test_other_waves_and_other_widths_do_not_merge(lib):
    ls = _launches(lib, [(64, 2, 0, 2), (64, 1, 1, 2)])                           # different `wave`
    assert [(l["c2"], l["c1"], l["single"]) for l in ls] == [(0, -1, -1), (-1, 1, -1)]
    groups = [(64, 2, 0, 2), (32, 2, 0, 2), (32, 3, 0, 1), (16, 3, 0, 5), (64, 1, 0, 2), (0, 1, 0, 3), (0, 2, 0, 3)]
    ls = _launches(lib, groups)
    assert [(l["c2"], l["c1"], l["single"]) for l in ls] == [(0, 4, -1), (-1, -1, 1), (-1, -1, 2), (-1, -1, 3), (-1, -1, 5), (-1, -1, 6)]
    for l in ls[1:]:                                                               # a single launch is the group as it was
        g = l["single"]
        assert l["ids"] == _ids(g, groups[g][3]) and l["ws_off"][0] == 0 and l["w32"] == _need(g, groups[g][3])
    # every group is launched exactly once, whatever the mix
    seen = sorted(x for l in ls for x in (l["c2"], l["c1"], l["single"]) if x >= 0)
    assert seen == list(range(len(groups)))
    # several groups of a variant (a workspace beyond one launch's): the k-th of one pairs with the k-th of the other
    ls = _launches(lib, [(64, 2, 0, 2), (64, 2, 0, 1), (64, 1, 0, 2), (64, 1, 0, 3), (64, 1, 0, 1)])
    assert [(l["c2"], l["c1"]) for l in ls] == [(0, 2), (1, 3), (-1, 4)]
    # only the groups [g0, g1) of the wave of launches are looked at
    ls = _launches(lib, [(64, 2, 0, 2), (64, 1, 0, 2)], g0=0, g1=1)
    assert [(l["c2"], l["c1"]) for l in ls] == [(0, -1)]


def test_either_half_may_be_empty(lib):
    m, = _launches(lib, [(64, 1, 0, 3)])
    assert (m["c2"], m["c1"], m["single"], m["n2"]) == (-1, 0, -1, 0) and m["ids"] == _ids(0, 3) and m["ws_off"][0] == 0
    m, = _launches(lib, [(64, 2, 0, 3)])
    assert (m["c2"], m["c1"], m["single"], m["n2"]) == (0, -1, -1, 3) and m["ids"] == _ids(0, 3) and m["w32"] == _need(0, 3)


def test_the_knob_merges_nothing(lib, monkeypatch):
    groups = [(64, 2, 0, 3), (64, 1, 0, 4)]
    assert [(l["c2"], l["c1"], l["single"]) for l in _launches(lib, groups, merge=0)] == [(-1, -1, 0), (-1, -1, 1)]
    monkeypatch.setenv("SVDSS_POA_MERGE", "0")                                    # as PoaKnobs::from_env reads it
    assert [(l["c2"], l["c1"], l["single"]) for l in _launches(lib, groups, merge=-1)] == [(-1, -1, 0), (-1, -1, 1)]
    monkeypatch.setenv("SVDSS_POA_MERGE", "1")
    assert len(_launches(lib, groups, merge=-1)) == 1
    monkeypatch.delenv("SVDSS_POA_MERGE")
    assert len(_launches(lib, groups, merge=-1)) == 1


def test_the_lengths_on_both_sides_of_the_variant_boundary():
    """What tests/test_call_streams_gpu.py builds its batches from: a longest read of 1,799 bp wants 2 * 27 + 1 + 8 = 63 columns,
    one per lane; 1,800 bp wants 65, two per lane -- whatever the number of reads."""
    from tests import poa_plan_lib as P
    for n in (1, 4):
        a, b = P.Batch([[1799] * n]).size(0, -1), P.Batch([[1800] * n]).size(0, -1)
        assert (a["where"], a["gw"], a["cols"], a["width"]) == ("run", 64, 1, 63)
        assert (b["where"], b["gw"], b["cols"], b["width"]) == ("run", 64, 2, 65)
