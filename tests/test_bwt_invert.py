"""svdss_bwt_strings on the host (device = -1): the marked LF walks of csrc/bwt_invert.h -- the code the GPU kernels of
csrc/bwt_invert.hip share -- over the collections of tests/bwt_invert_cases.py, at every stride, in both BWT forms,
against the strings themselves and against a plain LF walk in numpy; what is not a BWT of a collection is refused, and
a walker past the step limit is reported and made good by the serial walk."""
import ctypes as C

import numpy as np
import pytest

import svdss_amd
from tests import bwt_invert_cases as K
from tests import rld0_py

NAMES = sorted(K.collections())
EINVAL, EIO, ERANGE = 1, 3, 6


def test_the_collections_have_the_shapes_they_are_named_for():
    c = K.collections()
    assert [len(s) for s in c["lengths"]] == [0, 1, 2, 127, 128, 129, 300]
    assert len(K.rope_bwt("rows_0_mod_128")[0]) % 128 == 0 and len(K.rope_bwt("rows_127_mod_128")[0]) % 128 == 127
    assert len(c["many_short"]) == 700 and min(len(s) for s in c["many_short"]) == 0
    assert len(c["one_record"]) == 1 and (c["runs_of_n"][1] == 5).all()


@pytest.mark.parametrize("name", NAMES)
def test_ropebwt_order_gives_the_strings_back_in_order(name):
    bwt, strings = K.rope_bwt(name)
    want = [bytes(s) for s in strings]
    assert K.numpy_walk(bwt) == want
    for k, stride in enumerate(K.STRIDES):
        rc, got, m = K.raw_strings(bwt, -1, stride, shift=k % 4)
        assert rc == 0 and m == len(want), (stride, rc, m)
        assert got == want, stride


@pytest.mark.parametrize("name", NAMES)
def test_own_order_gives_the_same_multiset(name):
    bwt, want = K.own_bwt(name)
    walk = K.numpy_walk(bwt)
    assert sorted(walk) == want
    for k, stride in enumerate(K.STRIDES):
        rc, got, _ = K.raw_strings(bwt, -1, stride, shift=(k + 1) % 4)
        assert rc == 0 and got == walk, stride      # string r is the one spelled from row r


def test_python_wrapper_and_default_stride():
    bwt, strings = K.rope_bwt("lengths")
    got = svdss_amd.bwt_strings(bwt, device=-1)
    assert [bytes(g) for g in got] == [bytes(s) for s in strings]
    last = svdss_amd.bwt_strings_last()
    assert last["route"] == "host" and last["stride"] == 1024 and last["walkers"] == len(strings)


def test_stride_from_the_environment(monkeypatch):
    bwt, strings = K.rope_bwt("one_record")
    monkeypatch.setenv("SVDSS_INVERT_STRIDE", "100")
    assert [bytes(g) for g in svdss_amd.bwt_strings(bwt, device=-1)] == [bytes(s) for s in strings]
    assert svdss_amd.bwt_strings_last()["stride"] == 100
    svdss_amd.bwt_strings(bwt, device=-1, stride=9)          # the argument goes first
    assert svdss_amd.bwt_strings_last()["stride"] == 9


def test_bad_arguments():
    bwt, strings = K.rope_bwt("own_revcomp")
    n, m = len(bwt), len(strings)
    out, lens, k = np.zeros(n, np.uint8), np.zeros(m, np.int64), C.c_int32(0)
    f = svdss_amd.lib.svdss_bwt_strings
    assert f(None, n, -1, 0, out.ctypes.data, n, lens.ctypes.data, m, C.byref(k)) == EINVAL
    assert f(bwt.ctypes.data, 0, -1, 0, out.ctypes.data, n, lens.ctypes.data, m, C.byref(k)) == EINVAL
    assert f(bwt.ctypes.data, n, -1, 0, None, n, lens.ctypes.data, m, C.byref(k)) == EINVAL
    assert f(bwt.ctypes.data, n, -1, 0, out.ctypes.data, n, None, m, C.byref(k)) == EINVAL
    assert f(bwt.ctypes.data, n, -1, 0, out.ctypes.data, n, lens.ctypes.data, m, None) == EINVAL
    six = bwt.copy()
    six[n // 2] = 6
    assert f(six.ctypes.data, n, -1, 0, out.ctypes.data, n, lens.ctypes.data, m, C.byref(k)) == EINVAL
    # capacities: the number of strings comes back with SVDSS_ERANGE
    k.value = 0
    assert f(bwt.ctypes.data, n, -1, 0, out.ctypes.data, n, lens.ctypes.data, m - 1, C.byref(k)) == ERANGE and k.value == m
    k.value = 0
    assert f(bwt.ctypes.data, n, -1, 0, out.ctypes.data, n - m - 1, lens.ctypes.data, m, C.byref(k)) == ERANGE and k.value == m


def flipped_bwt():
    """A BWT with ONE symbol flipped so that a cycle of LF misses every sentinel.  The collection has no N and its largest
    suffix is "T$": the last row n-1 is the only T row, and its BWT symbol is the C in front of that T.  Flipped to T,
    rows n-2 and n-1 are the T rows (acc[T] = n - 2): the T of the sentinel row in front maps to n-2, and row n-1 holds
    the second T, so LF(n-1) = acc[T] + 1 = n-1 -- a cycle of one row.  LF is a permutation, so no walk from a sentinel
    row ever reaches it: the strings cannot sum to n - m symbols."""
    strings = [svdss_amd.nt6_encode("ACGA"), svdss_amd.nt6_encode("CCT")]
    bwt = rld0_py.collection_bwt(strings).copy()
    n = len(bwt)
    assert bwt[n - 1] == 2 and (bwt == 4).sum() == 1 and not (bwt == 5).any()
    bwt[n - 1] = 4
    acc_t = int((bwt < 4).sum())
    assert acc_t == n - 2 and acc_t + int((bwt[:n - 1] == 4).sum()) == n - 1      # LF(n-1) == n-1
    return bwt


@pytest.mark.parametrize("stride", K.STRIDES)
def test_a_cycle_that_misses_every_sentinel_is_refused(stride):
    rc, got, _ = K.raw_strings(flipped_bwt(), -1, stride)
    assert rc == EIO and got is None


def test_step_limit_is_reported_and_the_serial_walk_makes_it_good(monkeypatch):
    bwt, strings = K.rope_bwt("one_record")
    monkeypatch.setenv("SVDSS_INVERT_MAX_STEPS", "5")
    rc, got, m = K.raw_strings(bwt, -1, 1 << 20)
    assert rc == ERANGE and got is None and m == 1
    rc, got, _ = K.raw_strings(bwt, -1, 1)          # every row marked, a step per walker: the limit is not in the way
    assert rc == 0 and got == [bytes(s) for s in strings]
    got = svdss_amd.bwt_strings(bwt, device=-1, stride=1 << 20)
    assert [bytes(g) for g in got] == [bytes(s) for s in strings]
    assert svdss_amd.bwt_strings_last()["route"] == "serial"
