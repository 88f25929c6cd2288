"""The knobs and the launch plan of the search batch (svdss_amd/csrc/sfs_plan.h) on the CPU: every rule of the plan at its
edges, and SfsKnobs::from_env for each variable set, unset and malformed.  The shape of the defaults is an MI355X's:
256 CUs x 8 blocks = 2048, so lanes = 2048 * 256 / 2 = 262,144."""
import ctypes as C

import pytest

from tests import sfs_plan_lib as S

LANES = S.MAX_BLOCKS * 256 // 2


def _n_seg(**kw):
    return S.plan(**kw)["n_seg"]


@pytest.mark.parametrize("n_reads,n_seg", [(1, 8), (131072, 8), (131073, 4), (200000, 4), (262144, 4), (262145, 1), (1048576, 1)])
def test_n_seg_defaults_full_index(n_reads, n_seg):
    """want = 4 * lanes / n_reads, 1 below 4, at most 8, rounded down to a power of two (mean read length 15,000)."""
    assert LANES == 262144
    assert _n_seg(n_reads=n_reads) == n_seg


def test_n_seg_rank_blocks_alone():
    """No text or no suffix array: one lane per read from half a lane-load of reads on."""
    assert _n_seg(n_reads=131071, text_and_sa=False) == 8
    assert _n_seg(n_reads=131072, text_and_sa=False) == 1
    assert _n_seg(n_reads=131072, text_and_sa=True) == 8


@pytest.mark.parametrize("value,n_seg", [("1", 1), ("2", 2), ("3", 2), ("4", 4), ("12", 8), ("16", 16), ("100", 16), ("0", 1), ("-5", 1),
                                         ("x", 1)])
def test_segments_knob(value, n_seg):
    """SVDSS_SEGMENTS replaces the default, then [1, 16] and down to a power of two; it holds on rank blocks alone too."""
    for n_reads in (512, 1048576):
        assert _n_seg(env={"SVDSS_SEGMENTS": value}, n_reads=n_reads) == n_seg
    assert _n_seg(env={"SVDSS_SEGMENTS": value}, n_reads=1048576, text_and_sa=False) == n_seg


def test_segments_knob_does_not_lift_the_last_two_rules():
    env = {"SVDSS_SEGMENTS": "8"}
    assert _n_seg(env=env, n_reads=512, total_syms=512 * 1024) == 8       # a mean length of exactly 1,024 keeps the value
    assert _n_seg(env=env, n_reads=512, total_syms=512 * 1024 - 1) == 1   # 1,023 (rounded down)
    assert _n_seg(env=env, n_reads=512, mean_len=1023) == 1
    assert _n_seg(n_reads=512, mean_len=1023) == 1 and _n_seg(n_reads=512, mean_len=1024) == 8
    # item tickets are 32-bit: n_reads * n_seg stays below 2^31
    assert _n_seg(env=env, n_reads=1 << 28, mean_len=1024) == 1
    assert _n_seg(env=env, n_reads=(1 << 28) - 1, mean_len=1024) == 8
    assert _n_seg(env={"SVDSS_SEGMENTS": "4"}, n_reads=1 << 28, mean_len=1024) == 4
    assert _n_seg(env={"SVDSS_SEGMENTS": "1"}, n_reads=1 << 31, mean_len=1024) == 1
    assert _n_seg(n_reads=0, total_syms=0) == 1


def test_bs_choice():
    assert S.bs_possible() and S.bs_possible(n_dollar=S.BS_MAX_DOLLAR) and S.bs_possible(k=1, n_dollar=1)
    assert not S.bs_possible(have_sa=False) and not S.bs_possible(k=0) and not S.bs_possible(n_dollar=0)
    assert not S.bs_possible(n_dollar=S.BS_MAX_DOLLAR + 1)
    use = lambda **kw: S.plan(**kw)["use_bs"]
    assert use(bs=True, deep_frac=0.35) == 1 and use(bs=True, deep_frac=0.3499) == 0      # >= at 0.35
    assert use(bs=False, deep_frac=0.9) == 0
    assert use(env={"SVDSS_BS_DEEP": "0.2"}, bs=True, deep_frac=0.25) == 1                # the threshold moves
    assert use(env={"SVDSS_BS_DEEP": "0.5"}, bs=True, deep_frac=0.4) == 0
    assert use(env={"SVDSS_BS_DEEP": "0.5"}, bs=True, deep_frac=0.5) == 1
    assert use(env={"SVDSS_BS": "1"}, bs=True, deep_frac=0.0) == 1
    assert use(env={"SVDSS_BS": "1"}, bs=False, deep_frac=0.9) == 0                       # only within what is possible
    assert use(env={"SVDSS_BS": "0"}, bs=True, deep_frac=0.9) == 0
    for ignored in ("2", "yes", ""):
        assert use(env={"SVDSS_BS": ignored}, bs=True, deep_frac=0.9) == 1
        assert use(env={"SVDSS_BS": ignored}, bs=True, deep_frac=0.0) == 0


def test_blocks_for_and_gather_blocks():
    cap = S.MAX_BLOCKS
    assert [S.blocks_for(cap, n) for n in (0, 1, 256, 257, 512, 513)] == [1, 1, 1, 2, 2, 3]
    assert [S.blocks_for(cap, n) for n in (cap * 256 - 1, cap * 256, cap * 256 + 1, 1 << 40)] == [cap] * 4
    assert S.blocks_for(cap, (cap - 1) * 256) == cap - 1
    assert S.blocks_for(7, 7 * 256 + 1) == 7 and S.blocks_for(7, 6 * 256) == 6
    assert S.plan()["cap_blocks"] == cap and S.plan(max_blocks=304 * 8)["cap_blocks"] == 2432
    assert S.plan(env={"SVDSS_BLOCKS": "7"})["cap_blocks"] == 7
    assert S.plan(env={"SVDSS_BLOCKS": "5000"})["cap_blocks"] == 5000
    for no_cap in ("0", "-3", "x", ""):
        assert S.plan(env={"SVDSS_BLOCKS": no_cap})["cap_blocks"] == cap
    # gather: 4 waves per block, one read per wave iteration, at most 4 x max_blocks; SVDSS_BLOCKS does not reach it
    gather = lambda n, **kw: S.plan(n_reads=n, **kw)["gather_blocks"]
    assert [gather(n) for n in (0, 1, 4, 5, 8, 9)] == [1, 1, 1, 2, 2, 3]
    assert [gather(n) for n in (4 * 4 * cap - 4, 4 * 4 * cap, 4 * 4 * cap + 1, 1 << 24)] == [4 * cap - 1, 4 * cap, 4 * cap, 4 * cap]
    assert gather(1 << 24, env={"SVDSS_BLOCKS": "7"}) == 4 * cap


def test_use_order_edges():
    order = lambda **kw: S.plan(**kw)["use_order"]
    assert order(n_reads=1024, k=8) == 1
    assert order(n_reads=1023, k=8) == 0 and order(n_reads=1024, k=7) == 0 and order(n_reads=1024, k=0) == 0
    assert order(env={"SVDSS_ORDER": "1"}, n_reads=1024, k=8) == 1
    assert order(env={"SVDSS_ORDER": "1"}, n_reads=1023, k=8) == 0          # the knob only switches off
    assert order(env={"SVDSS_ORDER": "0"}, n_reads=1 << 20, k=12) == 0
    assert order(env={"SVDSS_ORDER": ""}, n_reads=1 << 20, k=12) == 0       # set and atoi() == 0


def test_fallback_ladder():
    """A quarter of the segments per step, one lane per read at the end or as soon as few enough reads are left."""
    many = 1000
    assert S.next_level(8, many, 64) == 2 and S.next_level(2, many, 64) == 1
    assert S.next_level(16, many, 64) == 4 and S.next_level(4, many, 64) == 1
    assert S.next_level(1, many, 64) == 1
    for lvl in (16, 8, 4, 2, 1):
        assert S.next_level(lvl, 64, 64) == 1 and S.next_level(lvl, 1, 64) == 1
    assert S.next_level(16, 65, 64) == 4
    assert S.next_level(16, many, 0) == 4 and S.next_level(16, many, many) == 1


@pytest.mark.parametrize("n_reads,total_syms", [(1, 0), (1, 63), (1, 64), (3, 65), (512, 512 * 2048), (512, 512 * 2048 + 7), (100000, 1500000007)])
def test_buffer_sizes(n_reads, total_syms):
    for seg in ("1", "2", "8", "16"):
        p = S.plan(env={"SVDSS_SEGMENTS": seg}, n_reads=n_reads, total_syms=total_syms)
        n_seg = p["n_seg"]
        assert n_seg == (int(seg) if total_syms // n_reads >= 1024 else 1)
        assert p["rec_total"] == (total_syms >> 3) + 8 * n_reads + 16
        assert p["tiny"] == (1 if total_syms < 64 else 0)
        if n_seg == 1:
            assert (p["seg_total"], p["seg_info_n"], p["fallback_n"], p["seg_take_n"]) == (0, 0, 0, 0)
        else:
            assert p["seg_total"] == (total_syms >> 3) + (8 + 24 * n_seg) * n_reads + 64
            assert (p["seg_info_n"], p["fallback_n"], p["seg_take_n"]) == (n_reads * n_seg, n_reads, 2 * n_reads * n_seg)


# variable -> field of SfsKnobs, its default, and (value, field) pairs; malformed values parse as atoi / atof leave them
FROM_ENV = {
    "SVDSS_SET": ("use_set", 1, [("0", 0), ("1", 1), ("7", 1), ("x", 0), ("", 0)]),
    "SVDSS_BS": ("bs", -1, [("0", 0), ("1", 1), ("2", -1), ("yes", -1), ("", -1), ("10", 1)]),
    "SVDSS_BS_DEEP": ("bs_deep", 0.35, [("0.2", 0.2), ("1", 1.0), ("x", 0.0)]),
    "SVDSS_TICKETS": ("ticket_chunk", 8, [("16", 16), ("1", 1), ("0", 8), ("-2", 8), ("x", 8)]),
    "SVDSS_SEGMENTS": ("segments", 0, [("4", 4), ("-5", -5), ("x", 0)]),
    "SVDSS_BLOCKS": ("blocks", 0, [("100", 100), ("0", 0), ("-1", 0), ("x", 0)]),
    "SVDSS_ORDER": ("order", 1, [("0", 0), ("1", 1), ("", 0), ("x", 0)]),
    "SVDSS_EXTRA_LDS": ("extra_lds", 0, [("4096", 4096), ("x", 0)]),
    "SVDSS_FALLBACK_DIRECT": ("fallback_direct", 64, [("0", 0), ("1000", 1000), ("x", 0), ("-1", -1)]),   # -1: 2^64 - 1, every count is "few"
    "SVDSS_DEBUG": ("debug", 0, [("1", 1), ("0", 1), ("", 1)]),
}


@pytest.mark.parametrize("var", sorted(FROM_ENV))
def test_from_env(var):
    field, default, cases = FROM_ENV[var]
    defaults = S.plan()
    assert defaults[field] == default and defaults["segments_set"] == 0
    for value, want in cases:
        got = S.plan(env={var: value})
        assert got[field] == want, (var, value)
        assert got["segments_set"] == (1 if var == "SVDSS_SEGMENTS" else 0)
        for other in S.KNOB_FIELDS + ("bs_deep",):       # no variable moves another one's knob
            if other not in (field, "segments_set"):
                assert got[other] == defaults[other], (var, value, other)
    assert S.plan() == defaults                          # read per call: nothing of the last call is left


def test_from_env_leaves_the_process_environment(monkeypatch):
    """The dump library sets the variables for the length of one call and puts the process's own back."""
    libc = C.CDLL(None)
    libc.getenv.restype = C.c_char_p
    monkeypatch.setenv("SVDSS_SEGMENTS", "2")
    monkeypatch.delenv("SVDSS_BLOCKS", raising=False)
    assert S.plan(env={"SVDSS_BLOCKS": "9"})["segments_set"] == 0
    assert libc.getenv(b"SVDSS_SEGMENTS") == b"2" and libc.getenv(b"SVDSS_BLOCKS") is None
