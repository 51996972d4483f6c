"""M3 with Nleft != -1 (ORBmatcher.cc:45-239): the CPU oracle's SearchByProjectionPointsFisheye against
tests/second_reading_points_fisheye.py, entry for entry (both rows and the count), on every case of tests/points_fisheye_cases.py but
the last -- and, from the reading's rule counters, the oracle and numpy alone, the proof that each case reaches the rule it was built
for.  No GPU.  tests/test_gpu_local_points_fisheye_batch.py runs the batched device call over the same cases."""
import os
import re

import numpy as np
import pytest

import points_fisheye_cases as pc
import second_reading as sr
import second_reading_points_fisheye as srp

NAMES = pc.NAMES
ORACLE_NAMES = [n for n in NAMES if n != "partner_out_of_range"]              # the oracle, as the reference, would write past its row there


@pytest.fixture(scope="module")
def OM(pkg, oracle):
    return oracle._oracle_matcher_class()()


@pytest.fixture(scope="module")
def CASES(oracle, synth):
    return pc.cases(oracle, synth)


@pytest.fixture(scope="module")
def POOLS(oracle, synth):
    return pc.pools(oracle, synth)


def grid_frames(P, p):
    """The second reading's frames of pair p (left, right), built once per pool."""
    G = P.setdefault("grid_frames", {})
    if p not in G:
        G[p] = tuple(sr.GridFrame(k, d, 0.0, 0.0, pc.INV_W, pc.INV_H) for k, d in (P["rows"][pc.FIRST_L + p], P["rows"][pc.FIRST_R + p]))
    return G[p]


def single_pair(pkg, backend, P, case, p):
    """One pair through a single-pair SearchByProjectionPointsFisheye (the oracle's, or the product's host entry point)."""
    (kl, dl), (kr, dr) = P["rows"][pc.FIRST_L + p], P["rows"][pc.FIRST_R + p]
    vl = pkg.FrameView(kl, dl, pc.W, pc.H, backend=backend); vr = pkg.FrameView(kr, dr, pc.W, pc.H, backend=backend)
    n, ml, mr = backend.SearchByProjectionPointsFisheye(vl, vr, **pc.reference_args(case, p))
    return int(n), ml, mr


def second_reading_pair(P, case, p, **variant):
    """One pair through the second reading: the depth gate is the reading's own (:59-60); a level outside the scale table, which the
    batched call skips and the reference would index the table with, is handed over as not in view."""
    gl, gr = grid_frames(P, p)
    q = case.Q[p]
    lv, lvr = q["level"].astype(np.int64), q["level_r"].astype(np.int64)
    gone = np.zeros(len(lv), bool) if case.th_far is None else (q["depth"] > np.float32(case.th_far))   # (the reading meets :59 before any level)
    iv = (q["in_view"] != 0) & (((lv >= 0) & (lv < pc.NLEV)) | gone)
    ivr = (q["in_view_r"] != 0) & (((lvr >= 0) & (lvr < pc.NLEV)) | (lvr == -1) | gone)
    l2r, r2l = case.partners(p)
    far = {} if case.th_far is None else dict(depth=q["depth"], th_far=case.th_far)
    return srp.search_by_projection_points_fisheye(gl, gr, case.blocked_l[p], case.blocked_r[p], l2r, r2l, pc.SF, iv, q["px"], q["py"], q["view_cos"],
                                                   np.where(iv, lv, 0), ivr, q["pxr"], q["pyr"], q["view_cos_r"], np.where(ivr, lvr, 0), q["qdesc"],
                                                   q["mp_obs"], case.th, case.nnratio, **variant, **far)


def test_second_reading_is_independent():
    """The second reading may not reach the oracle, the product or ctypes; it imports numpy, collections and second_reading only, and of
    second_reading nothing but the frame and the descriptor distance."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "second_reading_points_fisheye.py")).read()
    low = src.lower()
    for word in ("ctypes", "orbref", "liborb", "orb-slam3_amd", "orb_slam3_amd", "second_reading_fisheye", "second_reading_bow"):
        assert word not in low, "tests/second_reading_points_fisheye.py mentions %r" % word
    assert not re.search(r"^\s*(import|from)\s+(?!math\b|collections\b|numpy\b|second_reading\b)", low, re.M)
    imp = re.findall(r"^from second_reading import (.*?)(?:#.*)?$", src, re.M)
    assert len(imp) == 1 and {w.strip() for w in imp[0].split(",")} == {"GridFrame", "descriptor_distances"}
    assert "search_by_projection_points(" not in src and "sr." not in src


def test_case_list(CASES, POOLS):
    assert list(CASES) == NAMES
    c = POOLS["scene"]["counts"]
    assert c[pc.FIRST_L + 3] == 0 and c[pc.FIRST_R + 2] == 0 and c.max() <= 1000
    h = POOLS["hand"]["counts"]
    assert h.tolist() == [h[0], 0, h[0], 0, h[4], h[4], 0, 0] and 20 <= h[0] <= 64 and 20 <= h[4] <= 64
    for case in CASES.values():
        assert case.cap == POOLS[case.pool_name]["cap"]
        for q in case.Q:
            inl, inr = q["in_view"] != 0, q["in_view_r"] != 0
            far = np.zeros(len(inl), bool) if case.th_far is None else (q["depth"] > np.float32(case.th_far))
            # what must not be read is NaN / GARBAGE, what is read is finite
            assert np.isnan(q["px"][~inl | far]).all() and (q["level"][~inl | far] == pc.GARBAGE).all()
            assert np.isnan(q["pxr"][~inr | far]).all() and (q["level_r"][~inr | far] == pc.GARBAGE).all()
            assert np.isfinite(q["px"][inl & ~far]).all() and np.isfinite(q["view_cos"][inl & ~far]).all()
            live_r = inr & ~far & (q["level_r"] != -1)
            assert np.isfinite(q["pxr"][live_r]).all() and np.isnan(q["pxr"][inr & (q["level_r"] == -1)]).all()
            assert np.isfinite(q["depth"][inl | inr]).all()


@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_oracle_equals_second_reading(pkg, OM, POOLS, CASES, name):
    case = CASES[name]; P = POOLS[case.pool_name]
    for p in range(pc.NPAIRS):
        n, ml, mr = single_pair(pkg, OM, P, case, p)
        n2, ml2, mr2, t = second_reading_pair(P, case, p)
        assert n == n2, (name, p, n, n2)
        assert np.array_equal(ml, ml2), (name, p, np.flatnonzero(ml != ml2)[:8])
        assert np.array_equal(mr, mr2), (name, p, np.flatnonzero(mr != mr2)[:8])
        if case.rule is not None and p == case.rule_pair:
            assert t[case.rule] >= 1, (name, case.rule, dict(t))


def test_scene_cases_reach_both_rows_and_both_cross_writes(POOLS, CASES):
    P = POOLS["scene"]
    rejected = 0
    for name in pc.SCENE_NAMES:
        case = CASES[name]
        for p in (0, 1):
            n, ml, mr, t = second_reading_pair(P, case, p)
            rejected += t["left_ratio_rejected_right_in_view"]
            assert (ml >= 0).sum() >= 20 and (mr >= 0).sum() >= 20, (name, p)
            few = 1 if name == "scene_th10_blocked" else 5                    # (97 % of one row blocked there)
            assert t["l2r_cross_writes"] >= few and t["r2l_cross_writes"] >= few, (name, p, dict(t))
            assert t["left_only"] >= 1 and t["right_only"] >= 1 and t["neither_in_view"] >= 1 and t["level_r_minus_1"] >= 1
            if case.th_far is not None:
                assert t["far_point"] >= 20, (name, p)
        n, ml, mr, t = second_reading_pair(P, case, 3)                       # the empty left row: the right one is still searched
        assert t["left_row_empty"] == 1 and (mr >= 0).sum() >= 4 * few and len(ml) == 0
        n, ml, mr, t = second_reading_pair(P, case, 2)
        assert t["right_row_empty"] == 1 and (ml >= 0).sum() >= 4 * few and len(mr) == 0
    t = second_reading_pair(P, CASES["scene_no_obs"], 0)[3]
    assert t["overwrote"] >= 20 and t["l2r_cross_blocks"] == 0
    t = second_reading_pair(P, CASES["scene_th1"], 0)[3]
    assert t["later_query_sees_cross_block"] >= 1 and rejected >= 5, rejected
    assert CASES["scene_shared"].q_shared and not CASES["scene_th1"].q_shared
    assert {len(q["px"]) for q in CASES["scene_shared"].Q} == {600}


def test_th_is_not_applied_to_the_right_radius(POOLS, CASES):
    """A reading that multiplies the right radius by th as well gives other rows on the th-3 cases (:173-176 apply no factor)."""
    P = POOLS["scene"]
    for name in ("scene_th3", "scene_th3_far"):
        differ = 0
        for p in (0, 1):
            n, ml, mr, t = second_reading_pair(P, CASES[name], p)
            assert t["right_between_r_and_th_r"] >= 10
            n2, ml2, mr2, _ = second_reading_pair(P, CASES[name], p, th_on_right=True)
            differ += int(not np.array_equal(mr, mr2))
        assert differ >= 1, name
    case = CASES["right_radius_without_th"]
    n, ml, mr, t = second_reading_pair(POOLS["hand"], case, 0)
    assert n == 1 and (ml >= 0).sum() == 1 and (mr == -1).all()              # the left keypoint 9 px away is taken at th 3, the right one at 6 px is not
    n2, _, mr2, _ = second_reading_pair(POOLS["hand"], case, 0, th_on_right=True)
    assert n2 == 2 and (mr2 >= 0).sum() == 1


def _dry_lists(P, case, p, cam):
    """Queries of pair p whose window in camera cam holds more than 8 candidates of which fewer than two of the 8 nearest (distance, then
    visiting order) are free at the start: the listed candidates run dry and the window is scanned again."""
    g = grid_frames(P, p)[cam]
    q = case.Q[p]
    desc = P["rows"][(pc.FIRST_R if cam else pc.FIRST_L) + p][1]
    blk = (case.blocked_r if cam else case.blocked_l)[p]
    iv, x, y, vc, lv = [q[k] for k in (pc.RIGHT if cam else pc.LEFT)]
    n = 0
    for i in range(len(iv)):
        if not iv[i] or not 0 <= lv[i] < pc.NLEV or (case.th_far is not None and q["depth"][i] > case.th_far):
            continue
        r = np.float32(2.5) if float(vc[i]) > 0.998 else np.float32(4.0)
        if cam == 0 and case.th != 1.0:
            r = r * np.float32(case.th)
        c = g.features_in_area(x[i], y[i], r * pc.SF[lv[i]], int(lv[i]) - 1, int(lv[i]))
        if len(c) > 8:
            d = sr.descriptor_distances(q["qdesc"][i], desc[c])
            first8 = np.array(c)[np.argsort(d, kind="stable")[:8]]
            n += int((blk[first8] == 0).sum() < 2)
    return n


def test_dry_lists_provoked(POOLS, CASES):
    case = CASES["scene_th10_blocked"]
    assert abs(case.blocked_l[0].mean() - 0.97) < 0.02 and abs(case.blocked_r[1].mean() - 0.97) < 0.02
    assert _dry_lists(POOLS["scene"], case, 0, 0) >= 5 and _dry_lists(POOLS["scene"], case, 2, 0) >= 5
    # the right radius has no th factor: a right window of more than 8 comes from the handmade cluster
    H = POOLS["hand"]
    assert _dry_lists(H, CASES["rescan_left"], 0, 0) == 1 and _dry_lists(H, CASES["rescan_right"], 0, 1) == 1
    n, ml, mr, _ = second_reading_pair(H, CASES["rescan_left"], 0)
    assert n == 1 and (ml >= 0).sum() == 1                                    # best 5 of the listed ones, second 9 from beyond the list: 5 <= 0.8 * 9
    n, ml, mr, _ = second_reading_pair(H, CASES["rescan_right"], 0)
    assert n == 1 and (mr >= 0).sum() == 1                                    # best 11, second 30, both from beyond the list


def test_constructed_cases_give_what_they_were_built_for(POOLS, CASES):
    H = POOLS["hand"]

    def run(name, p=0):
        return second_reading_pair(H, CASES[name], p)

    n, ml, mr, t = run("ratio_reject_skips_right")
    assert n == 0 and (ml == -1).all() and (mr == -1).all() and t["right_claims"] == 0
    for name in ("left_empty", "left_above_th_high", "left_all_blocked"):
        n, ml, mr, t = run(name)
        assert n == 1 and (ml == -1).all() and (mr == 0).sum() == 1, name
    n, ml, mr, t = run("left_only")
    assert n == 1 and (ml == 0).sum() == 1 and (mr == -1).all()
    n, ml, mr, t = run("right_only")
    assert n == 1 and (mr == 0).sum() == 1 and (ml == -1).all()
    n, ml, mr, t = run("neither")
    assert n == 2 and t["neither_in_view"] == 2 and (ml == 1).sum() == 1 and (mr == 1).sum() == 1
    n, ml, mr, t = run("level_r_minus_1")
    assert n == 1 and (ml == 0).sum() == 1 and (mr == -1).all()
    n, ml, mr, t = run("l2r_blocks")
    assert n == 3 and (ml == 0).sum() == 1 and (mr == 0).sum() == 2 and (mr == 1).sum() == 0
    assert t["right_block_sees_own_cross_block"] == 1 and t["later_query_sees_cross_block"] >= 1
    n, ml, mr, t = run("l2r_open_counts_3")
    assert n == 3 and t["query_counted_3"] == 1 and (ml == 0).sum() == 1 and (mr == 0).sum() == 1
    n, ml, mr, t = run("cross_overwrites_observed")
    assert n == 3 and (mr == 1).sum() == 1 and (mr == 0).sum() == 0 and (ml == 1).sum() == 1
    n, ml, mr, t = run("r2l_cross")
    assert n == 5 and t["r2l_cross_writes"] == 2 and t["r2l_onto_own_left_claim"] == 1
    assert (ml == 0).sum() == 1 and (mr == 0).sum() == 1 and (ml == 1).sum() == 1 and (mr == 1).sum() == 1
    n, ml, mr, t = run("empty_left_row", 1)
    assert n == 2 and len(ml) == 0 and (mr >= 0).sum() == 2 and t["r2l_cross_writes"] == 0
    n, ml, mr, t = run("empty_right_row", 2)
    assert n == 2 and len(mr) == 0 and (ml >= 0).sum() == 2 and t["l2r_cross_writes"] == 0
    n, ml, mr, t = run("both_rows_empty", 3)
    assert n == 0 and len(ml) == 0 and len(mr) == 0 and t["left_row_empty"] == 1 and t["right_row_empty"] == 1
    n, ml, mr, t = run("nq0")
    assert n == 0 and (ml == -1).all() and (mr == -1).all()
    case = CASES["partner_out_of_range"]
    nl, nr = int(H["counts"][pc.FIRST_L]), int(H["counts"][pc.FIRST_R])
    assert ((case.l2r[0] >= nr) & (case.l2r[0] < case.cap)).sum() == 1 and ((case.r2l[0] >= nl) & (case.r2l[0] < case.cap)).sum() == 1
    assert (case.partners(0)[0] == -1).all() and (case.partners(0)[1] == -1).all() and not case.host_defined
    n, ml, mr, t = run("partner_out_of_range")
    assert n == 2 and t["l2r_cross_writes"] == 0 and t["r2l_cross_writes"] == 0


def test_an_unobserved_cross_write_keeps_the_block(pkg, OM, POOLS, CASES):
    """The one place where the entry points' blocked set is not `the slot's MapPoint has observations`: a cross write (:158, :225) puts a
    query WITHOUT observations into a slot whose MapPoint had them.  The oracle, the host entry point and the batched call keep such a
    slot blocked (a blocked set only grows); read to the letter, :102-104 / :194-196 would then find a MapPoint without observations and
    search the slot again.  The reading follows the entry points by default and counts the event; with free_on_cross it frees the slot,
    and only then do its rows leave the oracle's.  Callers' local map points have observations, so the event needs mp_obs = 0 rows."""
    P = POOLS["scene"]
    case = CASES["scene_th1"]
    seen = 0
    for p in (0, 1):
        want = single_pair(pkg, OM, P, case, p)
        n, ml, mr, t = second_reading_pair(P, case, p)
        assert (n, ml.tolist(), mr.tolist()) == (want[0], want[1].tolist(), want[2].tolist())
        seen += t["unobserved_cross_write_over_observed"]
        n2, ml2, mr2, t2 = second_reading_pair(P, case, p, free_on_cross=True)
        if t["unobserved_cross_write_over_observed"] == 0:
            assert (n2, ml2.tolist(), mr2.tolist()) == (n, ml.tolist(), mr.tolist())
    assert seen >= 1
    for name in ("scene_th3", "scene_th1_far", "scene_th10_blocked", "scene_no_obs"):   # every query observed, or none: the event cannot arise
        for p in range(pc.NPAIRS):
            assert second_reading_pair(P, CASES[name], p)[3]["unobserved_cross_write_over_observed"] == 0
