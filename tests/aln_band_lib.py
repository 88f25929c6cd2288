"""ctypes wrapper of tests/native/_aln_band_dump.so: the planner of the realignment's diagonal bands
(svdss_amd/csrc/aln_band.h) on the CPU.  Test infrastructure only."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "native", "_aln_band_dump.so")
_SRC = [os.path.join(ROOT, "tests", "native", "aln_band_dump.cpp"), os.path.join(ROOT, "svdss_amd", "csrc", "aln_band.h")]


def _build():
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in _SRC):
        return
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", _SO, _SRC[0]])


_build()
_lib = C.CDLL(_SO)
_lib.aln_band_plan_c.restype = None
_lib.aln_band_plan_c.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
_lib.aln_band_f_c.restype = C.c_int64
_lib.aln_band_f_c.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
_lib.aln_band_live_c.argtypes = [C.c_int, C.c_void_p]
_lib.aln_band_stripe_c.restype = None
_lib.aln_band_stripe_c.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
_lib.aln_band_plan_batch_c.restype = C.c_int64
_lib.aln_band_plan_batch_c.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int]

FULL, ONE_BAND, CARRY = 0, 1, 2
Plan = namedtuple("Plan", "lo hi c1 c2 mode slb x provable M steps full")


def _mat(mat):
    mat = np.ascontiguousarray(mat, dtype=np.int8).reshape(-1)
    return mat, int(round(len(mat) ** 0.5))


def plan(q, t, mat, gm, level=2):
    q = np.ascontiguousarray(q, dtype=np.uint8)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    mat, m = _mat(mat)
    g = np.array(gm, dtype=np.int32)
    out = np.zeros(11, dtype=np.int64)
    _lib.aln_band_plan_c(q.ctypes.data, len(q), t.ctypes.data, len(t), m, mat.ctypes.data, g.ctypes.data, level, out.ctypes.data)
    return Plan(*out.tolist())


def f(d, ql, tl, mat, gm):
    mat, m = _mat(mat)
    g = np.array(gm, dtype=np.int32)
    return _lib.aln_band_f_c(d, ql, tl, m, mat.ctypes.data, g.ctypes.data)


def live(d, p):
    b = np.array([p.lo, p.hi, p.c1, p.c2, p.mode], dtype=np.int32)
    return bool(_lib.aln_band_live_c(int(d), b.ctypes.data))


def stripe_steps(ql, tl, s, p):
    """[(a0, e0), (a1, e1)]: the ranges of wavefront steps stripe s executes"""
    b = np.array([p.lo, p.hi, p.c1, p.c2, p.mode], dtype=np.int32)
    out = np.zeros(4, dtype=np.int32)
    _lib.aln_band_stripe_c(ql, tl, s, b.ctypes.data, out.ctypes.data)
    return [(int(out[0]), int(out[1])), (int(out[2]), int(out[3]))]


def plan_batch(q, q_off, t, t_off, mat, gm, level=2):
    """plans every pair of a packed batch as the library does before its upload; the steps planned"""
    mat, m = _mat(mat)
    g = np.array(gm, dtype=np.int32)
    return _lib.aln_band_plan_batch_c(q.ctypes.data, q_off.ctypes.data, t.ctypes.data, t_off.ctypes.data, len(q_off) - 1, m,
                                      mat.ctypes.data, g.ctypes.data, level)


def walk(cigar):
    """The diagonals (j - i) a CIGAR's path touches: -> (match, runs).  match: the set of diagonals with an M column;
    runs: (op, diagonal before the run, diagonal after it, length) per gap run, op 1 = I (along the query), 2 = D."""
    d, match, runs = 0, set(), []
    for c in cigar:
        op, ln = int(c) & 0xf, int(c) >> 4
        if op == 0:
            match.add(d)
        else:
            nd = d + ln if op == 1 else d - ln
            runs.append((op, d, nd, ln))
            d = nd
    return match, runs
