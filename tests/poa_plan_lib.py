"""ctypes wrapper of tests/native/_poa_plan_dump.so: the planner of the POA batch (svdss_amd/csrc/poa_plan.h: sizes, launches,
waves of launches, fallback tasks) on the CPU.  Test infrastructure only."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "native", "_poa_plan_dump.so")
_SRC = [os.path.join(ROOT, "tests", "native", "poa_plan_dump.cpp"), os.path.join(ROOT, "svdss_amd", "csrc", "poa_plan.h"),
        os.path.join(ROOT, "svdss_amd", "csrc", "poa_quad_defs.h"), os.path.join(ROOT, "svdss_amd", "csrc", "poa_task.h")]


def _build():
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in _SRC):
        return
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", _SO, _SRC[0]])


_build()
_lib = C.CDLL(_SO)
_lib.poa_plan_round_json.restype = C.c_char_p
_lib.poa_plan_round_json.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_uint64,
                                     C.c_void_p, C.c_void_p]
_lib.poa_plan_size.restype = None
_lib.poa_plan_size.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
_lib.poa_plan_hbm_json.restype = C.c_char_p
_lib.poa_plan_hbm_json.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
for _f, _n in (("poa_plan_ws_ints", 4), ("poa_plan_wave_lds", 4), ("poa_plan_bundle_lds", 1), ("poa_plan_quad_lds", 3)):
    getattr(_lib, _f).restype = C.c_int64
    getattr(_lib, _f).argtypes = [C.c_int] * _n
_lib.poa_plan_quad_supported.argtypes = [C.c_int, C.c_int]
_lib.poa_plan_ws_budget.restype = C.c_uint64
_lib.poa_plan_ws_budget.argtypes = [C.c_int64, C.c_int, C.c_uint64, C.c_uint64]

ws_ints = _lib.poa_plan_ws_ints
wave_lds = _lib.poa_plan_wave_lds
bundle_lds = _lib.poa_plan_bundle_lds
quad_lds = _lib.poa_plan_quad_lds
quad_supported = _lib.poa_plan_quad_supported
ws_budget = _lib.poa_plan_ws_budget

LDS_MAX = 160 * 1024 - 512
WAVE_COLS = (1, 2, 3, 5)
TASK_FIELDS = ("nc", "ec", "max_len", "ws", "rs", "ring", "prio", "ws_off", "cons_off", "n_seqs")
HBM_FIELDS = ("cap_nodes", "cap_edges", "max_len", "pool_cap", "node_off", "edge_off", "dp_off", "op_off", "row_off64", "base_off", "cons_off")


def knobs(use_lds=True, use_quad=True, quad_gw=-1, quad_short=0, quad_minwork=0, quad_rows16=0, quad_rows32=0, nc_pct=150, noprio=False,
          no_mix=False):
    """The knobs at their defaults (PoaKnobs), or as the SVDSS_POA_* variables would set them."""
    return np.array([use_lds, use_quad, quad_gw, quad_short, quad_minwork, quad_rows16, quad_rows32, nc_pct, noprio, no_mix], dtype=np.int64)


class Batch:
    """lengths: per sub-cluster the list of its reads' lengths."""

    def __init__(self, lengths, kn=None, n_cus=256, budget=32 << 30):
        self.lengths = [list(map(int, cl)) for cl in lengths]
        flat = [l for cl in self.lengths for l in cl]
        self.seq_off = np.zeros(len(flat) + 1, dtype=np.int64)
        self.seq_off[1:] = np.cumsum(flat)
        self.cluster_off = np.zeros(len(self.lengths) + 1, dtype=np.int64)
        self.cluster_off[1:] = np.cumsum([len(cl) for cl in self.lengths])
        self.n = len(self.lengths)
        self.kn = knobs() if kn is None else kn
        self.n_cus, self.budget = n_cus, budget
        self.skip_round0 = np.zeros(max(self.n, 1), dtype=np.uint8)
        self.round0_no_wider = np.zeros(max(self.n, 1), dtype=np.uint8)

    def plan(self, rnd, ids=None):
        """poa_plan_round for the sub-clusters `ids` (default: all); tasks come back as dicts of TASK_FIELDS."""
        ids = np.arange(self.n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
        p = json.loads(_lib.poa_plan_round_json(self.seq_off.ctypes.data, self.cluster_off.ctypes.data, self.n, ids.ctypes.data, len(ids), rnd,
                                                self.kn.ctypes.data, self.n_cus, self.budget, self.skip_round0.ctypes.data,
                                                self.round0_no_wider.ctypes.data))
        for g in p["groups"]:
            g["tasks"] = [dict(zip(TASK_FIELDS, t["t"])) for t in g["tasks"]]
        return p

    def size(self, c, rnd):
        """One sub-cluster in one round: dict with where ('run', 'next', 'hbm'), w_band, width, gw, cols, ws, rs, ring, nc, ec, lds."""
        out = np.zeros(11, dtype=np.int64)
        _lib.poa_plan_size(self.seq_off.ctypes.data, self.cluster_off.ctypes.data, self.n, c, rnd, self.kn.ctypes.data, out.ctypes.data)
        d = dict(zip(("where", "w_band", "width", "gw", "cols", "ws", "rs", "ring", "nc", "ec", "lds"), out.tolist()))
        d["where"] = ("run", "next", "hbm")[d["where"]]
        return d

    def hbm(self, todo, pas):
        """The launches of pass `pas` of the HBM kernel; tasks as dicts of HBM_FIELDS."""
        todo = np.asarray(todo, dtype=np.int64)
        ls = json.loads(_lib.poa_plan_hbm_json(self.seq_off.ctypes.data, self.cluster_off.ctypes.data, todo.ctypes.data, len(todo), pas))
        for l in ls:
            l["tasks"] = [dict(zip(HBM_FIELDS, t["t"])) for t in l["tasks"]]
        return ls
