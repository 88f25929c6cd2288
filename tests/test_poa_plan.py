"""The plan of the POA batch (svdss_amd/csrc/poa_plan.h) on the CPU: sizes pinned by hand, the invariants of the packing over
random length lists, and the plans the code before the planner was split off made for three batches
(tests/golden/poa_plan_parent.json, recorded on an MI355X: 256 CUs)."""
import json
import os

import numpy as np

from tests import poa_plan_lib as P

GB = 1 << 30


def _one(length, rnd, **kn):
    return P.Batch([[length] * 20], P.knobs(**kn)).size(0, rnd)


def test_sizes_pinned_by_hand():
    """All knobs at their defaults, 20 reads of equal length L.  w = 10 + L / 100; the first stage needs 2w + 1 + 8 columns
    in group width x columns per lane; round 0 has 2w + 33 (64 where 2w + 9 fit), round 1 the specification's 2w + 129."""
    s = _one(500, -1)
    assert (s["where"], s["w_band"], s["width"], s["gw"], s["cols"], s["ws"]) == ("run", 15, 39, 64, 1, 64)
    s = _one(3000, -1)
    assert (s["where"], s["w_band"], s["width"], s["gw"], s["cols"], s["ws"]) == ("run", 40, 89, 64, 2, 128)
    assert (s["nc"], s["ec"]) == (4724, 4724 + 1181 + 84)           # 1.5 x 3000 + 8 x 20 + 64; nc + nc / 4 + 20 + 64
    assert s["lds"] == P.quad_lds(64, 2, 3000) == 4 * (4 * 3 * 136 + 3 * 136 + 16) + 3152
    s = _one(6000, -1)                                              # 149 columns want (64, 3), which is not instantiated
    assert s["where"] == "next" and s["w_band"] == 70 and not P.quad_supported(64, 3)
    s = _one(6000, 0)
    assert (s["where"], s["width"], s["cols"], s["ws"], s["rs"], s["ring"]) == ("run", 173, 3, 256, 176, 4)
    assert s["lds"] == P.wave_lds(s["nc"], 6000, 176, 4) == 12 * 6 * 184 + 16 * 6 + 64 + 6000 + 64 + 256
    s = _one(6000, 1)
    assert (s["width"], s["cols"], s["ws"]) == (2 * 70 + 129, 5, 512)
    assert s["nc"] == 3 * 6000 + 8 * 20 + 64                        # later rounds: 3 x the longest read ...
    assert s["where"] == "hbm" and P.bundle_lds(s["nc"]) == 218752 > P.LDS_MAX       # ... whose consensus tables are beyond the LDS
    s = _one(4000, 1)
    assert (s["where"], s["width"], s["cols"], s["ws"], s["nc"]) == ("run", 2 * 50 + 129, 5, 256, 12224)
    s = _one(6000, 2)                                               # the full matrix: 6001 columns are beyond the 4096 of a row
    assert s["where"] == "hbm"
    assert _one(3000, 2)["where"] == "hbm"                          # 6 ring rows of 3004 columns x 12 bytes are beyond the LDS
    s = _one(2000, 2)
    assert (s["where"], s["width"], s["ws"], s["rs"], s["cols"]) == ("run", 2001, 2048, 2004, 5)
    s = _one(500, 0)                                                # 2w + 9 = 40 <= 64: one column per lane
    assert (s["width"], s["cols"], s["ws"], s["rs"]) == (64, 1, 64, 64)
    assert P.bundle_lds(1000) == 12064 and P.ws_ints(10, 20, 30, 64) == 13 * 10 + 50 + 3 * 74 + 5 * 20 + 4 * 44 + 4 * 640


def test_knobs_pinned():
    s = _one(3000, -1, quad_gw=16)                                  # SVDSS_POA_QUAD_GW: 89 columns in 16 lanes
    assert (s["where"], s["gw"], s["cols"], s["ws"]) == ("run", 16, 6, 96)
    s = _one(3000, -1, quad_gw=32)
    assert (s["where"], s["gw"], s["cols"], s["ws"]) == ("run", 32, 3, 96)
    s = _one(500, -1, quad_gw=16)                                   # at least 3 / 2 columns per lane at width 16 / 32
    assert (s["gw"], s["cols"], s["ws"]) == (16, 3, 48)
    s = _one(500, -1, quad_gw=32)
    assert (s["gw"], s["cols"], s["ws"]) == (32, 2, 64)
    assert _one(6000, -1, quad_gw=16)["where"] == "next"            # (16, 10)
    assert _one(500, -1, quad_gw=48)["where"] == "next" and _one(500, -1, quad_gw=0)["where"] == "next"
    assert _one(500, -1, quad_short=500)["gw"] == 16 and _one(501, -1, quad_short=500)["gw"] == 64      # SVDSS_POA_QUAD_SHORT
    assert _one(500, -1, quad_rows16=10000)["gw"] == 16 and _one(500, -1, quad_rows16=9999, quad_rows32=10000)["gw"] == 32
    b = P.Batch([[3000] * 20, [500] * 20, [1500] * 20], P.knobs(quad_minwork=50))                       # SVDSS_POA_QUAD_MINWORK
    p = b.plan(-1)
    assert p["next"] == [1] and sorted(i for g in p["groups"] for i in g["ids"]) == [0, 2]              # 1500 x 20 is the half
    b = P.Batch([[3000] * 20, [], [0], [500] * 3], P.knobs(use_lds=False, use_quad=False))              # SVDSS_POA_HBM=1
    p = b.plan(0)
    assert p["hbm"] == [0, 1, 2, 3] and p["groups"] == [] and p["next"] == [] and p["cuts"] == [0]
    s = _one(3000, 0, nc_pct=100)                                   # SVDSS_POA_NC=100
    assert (s["nc"], s["ec"]) == (3000 + 160 + 64, 3224 + 806 + 84)
    assert _one(3000, 1, nc_pct=100)["nc"] == 9000 + 224            # ... scales the first estimate only
    assert P.ws_budget(32, 0, 0, 0) == 32 * GB and P.ws_budget(1, 1, 64 * GB, 0) == GB                  # SVDSS_POA_WS_GB
    assert P.ws_budget(32, 1, 10 * GB, 2 * GB) == 6 * GB and P.ws_budget(32, 1, GB, 0) == GB            # half of the device; 1 GB floor


def _random_lengths(rng):
    n = int(rng.choice([0, 1, 2, 5, 30, 120, 400]))
    n = int(rng.integers(0, n + 1))
    top = int(rng.choice([80, 700, 3000, 8000]))
    lengths = [[int(x) for x in rng.integers(0, top + 1, size=int(rng.integers(0, 41)))] for _ in range(n)]
    return lengths + [[], [0], [0, 2], [top] * 40]


def _check_plan(b, p, ids, rnd):
    groups = p["groups"]
    assert sorted([i for g in groups for i in g["ids"]] + p["next"] + p["hbm"]) == sorted(ids)          # exactly one place each
    run = []
    for g in groups:
        quad = g["gw"] != 0
        assert (rnd < 0) == quad and len(g["ids"]) == len(g["tasks"]) > 0
        assert P.quad_supported(g["gw"], g["cols"]) if quad else g["cols"] in P.WAVE_COLS
        o32 = o8 = 0
        for i, t in zip(g["ids"], g["tasks"]):
            assert (t["ws_off"], t["cons_off"]) == (o32, o8)        # one after the other: disjoint
            o32 += P.ws_ints(t["nc"], t["ec"], t["max_len"], t["ws"])
            o8 += t["nc"]
            assert t["max_len"] == max(b.lengths[i]) and t["n_seqs"] == len(b.lengths[i]) and 0 < t["n_seqs"] <= 8191
            assert sum(b.lengths[i]) + 2 >= t["nc"] > 0 and t["ec"] > t["nc"]
            if quad:                                                # (the launch takes its LDS from the longest read of the group)
                assert t["ws"] == g["gw"] * g["cols"] and P.quad_lds(g["gw"], g["cols"], t["max_len"]) <= P.quad_lds(g["gw"], g["cols"], g["max_len"])
            else:
                assert P.wave_lds(t["nc"], t["max_len"], t["rs"], t["ring"]) <= g["lds"]
                assert (g["cols"] == 5 or t["rs"] <= 64 * g["cols"]) and t["rs"] <= t["ws"] <= 4096 and t["ws"] & (t["ws"] - 1) == 0 and t["ring"] == 4
            assert P.bundle_lds(t["nc"]) <= g["bundle_lds"]
            run.append((i, t, g["wave"]))
        assert (o32, o8) == (g["w32"], g["w8"])
        assert o32 <= 2 * GB or len(g["tasks"]) == 1                # ints of workspace per launch
        assert g["max_len"] == max(t["max_len"] for t in g["tasks"])
        assert max(g["lds"], g["bundle_lds"], P.quad_lds(g["gw"], g["cols"], g["max_len"]) if quad else 0) <= P.LDS_MAX
    cuts = p["cuts"]
    assert cuts[0] == 0 and cuts[-1] == len(groups) and all(x < y for x, y in zip(cuts, cuts[1:]))
    for x, y in zip(cuts, cuts[1:]):
        assert y - x == 1 or sum(g["bytes"] for g in groups[x:y]) <= b.budget
        assert len({g["wave"] for g in groups[x:y]}) == 1
    chain = lambda it: it[1]["n_seqs"] * it[1]["max_len"]
    if rnd < 0 and run:
        total = sum(4 * P.ws_ints(t["nc"], t["ec"], t["max_len"], t["ws"]) + t["nc"] + 256 for _, t, _ in run)
        per_wave = b.budget - b.budget // 8
        n_waves = max(1, -(-total // per_wave))
        for k, it in enumerate(sorted(run, key=lambda it: (-chain(it), it[0]))):                       # dealt longest first
            assert it[2] == (k % n_waves if n_waves > 1 else 0)
    else:
        assert all(w == 0 for _, _, w in run)
    wmax = max([1] + [chain(it) for it in run])
    for it in run:
        wk = chain(it)
        assert it[1]["prio"] == (3 if wk * 2 > wmax else 2 if wk * 4 > wmax else 1 if wk * 8 > wmax else 0)
    return len(cuts) - 1


def test_invariants_over_random_length_lists():
    rng = np.random.default_rng(2026)
    most_waves = 0
    for it in range(200):
        lengths = _random_lengths(rng)
        budget = int(rng.choice([32 * GB, GB, 256 << 20, 64 << 20]))
        n_cus = int(rng.choice([256, 8, 1]))
        ids = list(range(len(lengths))) if it % 3 else sorted(rng.choice(len(lengths), size=len(lengths) // 2, replace=False).tolist())
        for gw in (-1, 16, 32, 64):
            b = P.Batch(lengths, P.knobs(quad_gw=gw, quad_short=int(rng.choice([0, 600])) if gw < 0 else 0), n_cus, budget)
            p = b.plan(-1, ids)
            most_waves = max(most_waves, _check_plan(b, p, ids, -1))
            if gw < 0:
                for i in range(len(lengths)):                       # round 0 skips what could only fail the same way
                    b.skip_round0[i] = b.round0_no_wider[i] and i % 2
                for rnd in (0, 1, 2):
                    p = b.plan(rnd, ids)
                    _check_plan(b, p, ids, rnd)
                    if rnd == 0:
                        assert p["next"] == [i for i in ids if b.skip_round0[i]]
    assert most_waves >= 3


def test_fallback_tasks():
    rng = np.random.default_rng(7)
    budget = 3 << 30
    for it in range(40):
        lengths = _random_lengths(rng)
        todo = sorted(rng.choice(len(lengths), size=(len(lengths) + 1) // 2, replace=False).tolist())
        if it % 4 == 0:                                             # ~0.6 G ints each in pass 0, 15 G in pass 1: several launches
            todo += list(range(len(lengths), len(lengths) + 12))
            lengths = lengths + [[8000] * 40] * 12
        b = P.Batch(lengths)
        for pas in (0, 1):
            launches = b.hbm(todo, pas)
            assert [i for l in launches for i in l["ids"]] == todo
            for l in launches:
                o32 = o64 = o8 = 0
                for i, t in zip(l["ids"], l["tasks"]):
                    tot, maxl, n = sum(b.lengths[i]), max(b.lengths[i] + [0]), len(b.lengths[i])
                    band = 2 * (10 + maxl // 100) + 129
                    assert (t["cap_nodes"], t["cap_edges"], t["max_len"]) == (tot + 2, tot + n + 2, maxl)
                    assert t["pool_cap"] == (tot + 2) * (min(band, maxl + 1) if pas == 0 else maxl + 1)
                    assert (t["node_off"], t["row_off64"], t["base_off"]) == (o32, o64, o8)
                    assert t["edge_off"] == t["node_off"] + 17 * t["cap_nodes"] and t["dp_off"] == t["edge_off"] + 5 * t["cap_edges"]
                    assert t["op_off"] == t["dp_off"] + 6 * t["pool_cap"] and t["cons_off"] == t["base_off"] + t["cap_nodes"]
                    o32 = t["op_off"] + 2 * (t["cap_nodes"] + maxl + 4)
                    o64 += 2 * t["cap_nodes"]
                    o8 += 2 * t["cap_nodes"]
                assert (o32, o64, o8) == (l["w32"], l["w64"], l["w8"])
                assert o32 <= budget or len(l["tasks"]) == 1
            if it % 4 == 0:
                assert len(launches) > 1


def test_plans_of_the_parent_commit():
    """The groups, their tasks, what is sent on and the waves of launches, round by round, as the function made them before
    the plan became a function of its own: exactly."""
    rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "poa_plan_parent.json")))
    assert sorted(rec) == ["mixed_21_40", "multiwave_1gb", "quad_spec_gw64"]
    for name, r in rec.items():
        b = P.Batch(r["lengths"], P.knobs(**r["knobs"]), 256, r["ws_budget"])
        assert r["rounds"], name
        for rd in r["rounds"]:
            assert rd["n_cus"] == 256 and rd["ws_budget"] == r["ws_budget"]
            b.skip_round0[:] = 0
            b.skip_round0[rd["skip_round0"]] = 1
            p = b.plan(rd["round"], rd["cur"])
            assert (p["next"], p["hbm"], p["cuts"]) == (rd["next"], rd["hbm"], rd["cuts"]), (name, rd["round"])
            assert np.flatnonzero(b.round0_no_wider[:b.n]).tolist() == rd["round0_no_wider"]
            assert len(p["groups"]) == len(rd["groups"])
            for g, want in zip(p["groups"], rd["groups"]):
                for key in ("gw", "cols", "wave", "lds", "bundle_lds", "w32", "w8", "ids"):
                    assert g[key] == want[key], (name, rd["round"], key)
                got = [[t[f] for f in ("nc", "ec", "ws", "rs", "ws_off", "cons_off", "prio")] for t in g["tasks"]]
                assert got == want["tasks"], (name, rd["round"])
        if name == "multiwave_1gb":
            assert len(r["rounds"][0]["cuts"]) - 1 >= 2
