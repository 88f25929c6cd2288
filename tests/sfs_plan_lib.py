"""ctypes wrapper of tests/native/_sfs_plan_dump.so: the knobs and the launch plan of the search batch
(svdss_amd/csrc/sfs_plan.h) on the CPU.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "native", "_sfs_plan_dump.so")
_SRC = [os.path.join(ROOT, "tests", "native", "sfs_plan_dump.cpp"), os.path.join(ROOT, "svdss_amd", "csrc", "sfs_plan.h")]


def _build():
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in _SRC):
        return
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", _SO, _SRC[0]])


_build()
_lib = C.CDLL(_SO)
_lib.sfs_plan_eval.restype = None
_lib.sfs_plan_eval.argtypes = [C.c_char_p, C.c_void_p, C.c_double, C.c_void_p, C.POINTER(C.c_double)]
_lib.sfs_plan_blocks_for.argtypes = [C.c_int, C.c_int64]
_lib.sfs_plan_next_level.argtypes = [C.c_int, C.c_uint64, C.c_uint64]
_lib.sfs_plan_bs_possible.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int64]

blocks_for = _lib.sfs_plan_blocks_for
next_level = _lib.sfs_plan_next_level

KNOB_FIELDS = ("use_set", "bs", "ticket_chunk", "segments_set", "segments", "blocks", "order", "extra_lds", "fallback_direct", "debug")
PLAN_FIELDS = ("use_bs", "n_seg", "cap_blocks", "gather_blocks", "use_order", "tiny", "rec_total", "seg_total", "seg_info_n", "fallback_n",
               "seg_take_n")
BS_MAX_DOLLAR = 256   # SV_BS_MAX_DOLLAR of sfs_core2.h
MAX_BLOCKS = 2048     # 256 CUs x 8


def bs_possible(have_sa=True, k=12, n_dollar=2, max_dollar=BS_MAX_DOLLAR):
    return bool(_lib.sfs_plan_bs_possible(int(have_sa), k, n_dollar, max_dollar))


def plan(env=None, n_reads=1024, total_syms=None, mean_len=15000, max_blocks=MAX_BLOCKS, bs=False, deep_frac=0.0, text_and_sa=True, k=12):
    """SfsKnobs::from_env with exactly the variables of the dict `env` set, then sfs_plan for the shape: one dict of
    KNOB_FIELDS, bs_deep and PLAN_FIELDS.  total_syms defaults to n_reads * mean_len; bs: SfsShape::bs_possible."""
    if total_syms is None:
        total_syms = n_reads * mean_len
    text = "\n".join("%s=%s" % kv for kv in (env or {}).items()).encode()
    shape = np.array([n_reads, total_syms, max_blocks, bs, text_and_sa, k], dtype=np.int64)
    out = np.zeros(len(KNOB_FIELDS) + len(PLAN_FIELDS), dtype=np.int64)
    bs_deep = C.c_double(0)
    _lib.sfs_plan_eval(text, shape.ctypes.data, float(deep_frac), out.ctypes.data, C.byref(bs_deep))
    d = dict(zip(KNOB_FIELDS + PLAN_FIELDS, out.tolist()))
    d["bs_deep"] = bs_deep.value
    return d
