"""No GPU.  (1) The frames of tests/quadtree_table_cases.py reach, on the second reading alone, the branches they name; the levels a case
declares deep hold two candidates in one node at the planned table depth and end with every dot in a node of its own, the other
ladder cases hold none.  (2) The planner's choice of k_quadtree2's table depth (orbx_plan.h, through tests/qt_plan_dump.cpp): it
costs no LDS, the overlays fit, the path bits suffice, and the restated rule of the case file agrees with it."""
import os
import subprocess

import numpy as np
import pytest

import extract_cases as ec
import quadtree_table_cases as qc
import second_reading_extract as sr
import test_oracle_params_cpu as op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qc.all_cases()
LDS = 160 * 1024
# (w, h, nf, nl, sf, max_batch): bench.py's four geometries (c2, c5, c4, c3), then others around the rule's thresholds
BENCH = [(752, 480, 1000, 8, 1.2, 1024), (1920, 1080, 4000, 8, 1.2, 128), (512, 512, 1500, 8, 1.2, 16), (752, 480, 1200, 8, 1.2, 512)]
OTHER = [(1241, 376, 1000, 8, 1.2, 8), (1241, 376, 4000, 8, 1.2, 8), (160, 160, 94, 1, 1.2, 1), (160, 160, 95, 1, 1.2, 1), (160, 160, 503, 1, 1.2, 1),
         (160, 160, 504, 1, 1.2, 1), (160, 160, 512, 1, 1.2, 1), (160, 160, 1200, 1, 1.2, 1), (320, 240, 300, 4, 1.2, 2)]


def levels_of(c):
    """The level images the extractor would see: level 0 is the frame, the others the restated resize (tests/test_oracle_params_cpu.py)."""
    out = [c["img"]]
    for lw, lh in sr.level_sizes(c["img"].shape[1], c["img"].shape[0], c["sf"], c["nl"])[1:]:
        out.append(op._resize_linear(out[-1], lw, lh))
    return out


@pytest.fixture(scope="module")
def readings():
    return {c["name"]: sr.extract(levels_of(c), c["nf"], c["sf"], c["ini"], c["mn"], c["lap"]) for c in CASES}


def test_names_are_unique():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert all(64 <= c["area"][0] <= 180 and 35 <= c["area"][1] <= 180 and 1 <= c["nl"] <= 3 for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_case_reaches_what_it_names(c, readings):
    rd = readings[c["name"]]
    for k in c["want"]:
        assert rd["counters"][k] > 0, (k, dict(rd["counters"]))
    for k in c["never"]:
        assert rd["counters"][k] == 0, (k, dict(rd["counters"]))
    if c["n_out"] is not None:
        assert len(rd["fields"]) == c["n_out"]
    sharing = qc.levels_sharing_a_node(c, rd["candidates"])
    assert set(c["deep"]) <= set(sharing)
    falls = qc.levels_that_fall_back(c, rd)
    assert set(c["deep"]) <= set(falls) <= set(sharing), (falls, sharing)
    if c["name"].startswith(("ladder", "triple")):
        assert tuple(sharing) == tuple(falls) == c["deep"]                       # the halving helper and the watched reading agree
        assert len(rd["candidates"][0]) == c["n_out"]                            # every dot is a candidate and ends alone in its node


def test_depths_the_cases_claim(readings):
    by = {c["name"]: c for c in CASES}
    W = H = qc.A
    for D in (3, 4, 5):
        for s in (D - 1, D, D + 1):
            for kind, couples in (("ladder", 1), ("triple", 3)):               # one couple / the three couples of three dots part at depth s, all others earlier
                c = by["%s_D%d_s%d" % (kind, D, s)]
                k = readings[c["name"]]["candidates"][0]
                depths = [qc.separating_depth(tuple(p[:2]), tuple(q[:2]), W, H) for i, p in enumerate(k) for q in k[:i]]
                assert max(depths) == s and depths.count(s) == couples and c["D"] == D and (c["deep"] == (0,)) == (s > D), c["name"]
    # what the frames that are no ladders do, by the watched reading: the final phase after 1, 2, 3 full passes, two walks, zero-gain
    # splits, erased roots and the pyramids all stay on the tables; the clusters' second walk divides depth-3 nodes
    falls = {c["name"]: qc.levels_that_fall_back(c, readings[c["name"]]) for c in CASES}
    assert falls["second_walk_falls_back"] == [0]
    assert not any(v for n, v in falls.items() if not n.startswith(("ladder", "triple")) and n != "second_walk_falls_back"), falls
    assert readings["no_candidate"]["candidates"][0].shape[0] == 0
    assert len(readings["weak_second_level"]["candidates"][0]) > 0 and len(readings["weak_second_level"]["candidates"][1]) == 0
    assert by["tie_through_path_table"]["D"] == 3 and not qc.levels_sharing_a_node(by["tie_through_path_table"], readings["tie_through_path_table"]["candidates"])
    assert by["budget_below_4_roots"]["nf"] < 4 * qc.roots(*by["budget_below_4_roots"]["area"])[0]
    # the erased root leaves rows of the path table that no node owns, between rows that are owned
    for n_ini in (2, 3, 4):
        c = by["roots_%d_one_erased" % n_ini]
        used = {int(qc.node_path(int(x), int(y), *c["area"], 0)[0]) for x, y, _ in readings[c["name"]]["candidates"][0]}
        assert len(used) == n_ini - 1 and qc.roots(*c["area"])[0] == n_ini


# ---------------------------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("qt_plan")), "qt_plan_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "qt_plan_dump.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    keys = BENCH + OTHER + sorted({ec.key(c)[:2] + (c["nf"], c["nl"], c["sf"], 1) for c in CASES})
    text = "".join("%d %d %d %.9g %d %d\n" % (w, h, nf, sf, nl, mb) for w, h, nf, nl, sf, mb in keys)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(keys)
    return list(zip(keys, rows))


def parent_lds(cap, sort, max_cells, max_ini, fuse):
    """k_quadtree2's LDS before the tables went deeper (the formula tests/test_plan_cpu.py restates)."""
    hist, path = (340, 256) if fuse == 4 else (84, 64)
    return sort * 8 + cap * 68 + (max_cells + 1) * 4 + 64 + max_ini * (hist * 4 + path * 2) + cap * 4 + 8


def test_table_depth_costs_no_lds_and_fits(planned):
    for key, row in planned:
        rc, fuse, D, lds, cap, sort, max_ini, max_cells = row[:8]
        over = [(row[8 + 2 * i], row[9 + 2 * i]) for i in range(3)]                # (histogram bytes, path table bytes) at fuseD, +1, +2
        assert rc == 0, key
        assert lds == parent_lds(cap, sort, max_cells, max_ini, fuse), key       # D = fuseD reproduces the old size -- and so does every D
        assert LDS // lds == LDS // parent_lds(cap, sort, max_cells, max_ini, fuse)   # workgroups per CU
        assert fuse <= D <= fuse + 2 and (max_ini << (2 * D)) <= 4096, key        # a node's path | depth << 12
        fits = lambda i: i == 0 or (over[i][0] <= 10 * cap and over[i][1] <= 8 * sort and (max_ini << (2 * (fuse + i))) <= 4096)
        assert fits(D - fuse), key
        assert not any(fits(i) for i in range(D - fuse + 1, 3)), key              # the largest that fits
        w, h, nf, nl, sf, _ = key
        assert qc.table_depth((w, h, nf, nl, sf))[:2] == (fuse, D), key


def test_table_depth_of_the_bench_geometries(planned):
    got = {key[:3]: (row[1], row[2]) for key, row in planned}
    assert got[(752, 480, 1000)] == (3, 4)                                       # the headline: levels 0-2 leave state 0 at depth 3 and need depth 4
    assert got[(752, 480, 1200)] == (3, 4)
    assert got[(512, 512, 1500)] == (3, 4)
    assert got[(1920, 1080, 4000)] == (4, 5)
    # the thresholds of the rule on one 128 x 128 level (one root): 1 KiB of depth-4 counts wants 103 list entries, 5 KiB 512; depth 6
    # (20 KiB) would want 2048 entries, whose lists no longer fit the LDS
    assert [got[(160, 160, nf)] for nf in (94, 95, 503, 504, 512, 1200)] == [(3, 3), (3, 4), (3, 4), (3, 5), (4, 5), (4, 5)]
    for c in CASES:
        assert got[ec.key(c)[:2] + (c["nf"],)][1] == c["D"], c["name"]
