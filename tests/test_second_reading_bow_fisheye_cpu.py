"""M7 with F.Nleft != -1 (ORBmatcher.cc:314-547): the CPU oracle's SearchByBoWFisheye against tests/second_reading_bow_fisheye.py,
entry for entry (the combined row and the count), on every hand-laid pair and scene pair of tests/bow_fisheye_cases.py; the proof that
each hand-laid pair reaches the rule it was built for; and the CPU-side checks of orbm_search_by_bow_fisheye_batch_async (declared,
exported by both builds, bound, and every refusal fires before a device is touched).  No GPU.
tests/test_gpu_bow_fisheye_batch.py runs the batched device call over the same batches."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

import bow_fisheye_cases as bc
import second_reading_bow_fisheye as srb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "orbm_search_by_bow_fisheye_batch_async"
AB_LIB = os.path.join(ROOT, "orb-slam3_amd", "liborbslam3_amd_ab.so")
COUNTERS = ["right_claimed_left_ratio_failed", "right_refused_left_over_th_low", "right_refused_no_left_candidate",
            "right_claimed_best_equals_runner_up", "skipped_claimed_left", "skipped_claimed_right", "culled_left", "culled_right"]

TOTAL = Counter()                                                             # the branches every compared pair took, for test_every_counter


@pytest.fixture(scope="module")
def OM(pkg, oracle):
    return oracle._oracle_matcher_class()()


def _compare(OM, b):
    """Every in-range pair of batch b: oracle == reading; returns {pair name: (n, left row, right row, trace)}."""
    out = {}
    for p in range(b.npairs):
        a = bc.single_args(b, p)
        if a is None:
            continue
        n, fm, t = srb.search_by_bow_fisheye(*a)
        n2, fm2 = OM.SearchByBoWFisheye(*a)
        assert n == n2, (b.name, b.names[p], n, n2)
        assert np.array_equal(fm, fm2), (b.name, b.names[p], np.flatnonzero(fm != fm2)[:8])
        assert n == int((fm >= 0).sum())                                      # a slot is claimed at most once: the count is the row's
        TOTAL.update({k: v for k, v in t.items() if k in COUNTERS})
        out[b.names[p]] = (n, fm[:a[6]].tolist(), fm[a[6]:].tolist(), t)
    return out


def test_second_reading_is_independent():
    """The second reading may not reach the oracle, the product or ctypes; it imports numpy, collections and second_reading only."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "second_reading_bow_fisheye.py")).read().lower()
    for word in ("ctypes", "orbref", "liborb", "orb-slam3_amd", "orb_slam3_amd"):
        assert word not in src, "tests/second_reading_bow_fisheye.py mentions %r" % word
    assert not re.search(r"^\s*(import|from)\s+(?!math\b|collections\b|numpy\b|second_reading\b)", src, re.M)


@pytest.mark.parametrize("nnratio,check_ori,weights", bc.HAND_PARAMS)
def test_oracle_equals_second_reading_hand(OM, nnratio, check_ori, weights):
    _compare(OM, bc.hand(nnratio, check_ori, weights))


@pytest.mark.parametrize("levelsup,nnratio,check_ori,weights", bc.SCENE_PARAMS)
def test_oracle_equals_second_reading_scene(OM, oracle, synth, levelsup, nnratio, check_ori, weights):
    b = bc.scene(oracle, synth, levelsup, nnratio, check_ori, weights)
    assert b.npairs == 9
    r = _compare(OM, b)
    own = min(r[k][0] for k in ("own0", "own1", "own2"))
    assert own > 80 and r["unrelated"][0] < own // 4, {k: v[0] for k, v in r.items()}
    for k in ("own0", "own1", "own2", "swapped"):                             # both rows carry matches
        assert sum(v >= 0 for v in r[k][1]) > 30 and sum(v >= 0 for v in r[k][2]) > 15, k
    assert r["empty_left"][0] == 0 and r["empty_kf"][0] == 0 and r["empty_right"][0] > 50 and r["empty_right"][2] == []


def test_hand_pairs_reach_their_rules(OM):
    """Each hand-laid pair gives the rows it was laid out to give (nnratio 0.7, orientation on unless stated)."""
    r = _compare(OM, bc.hand(0.7, 1))
    assert r["th_50"][:3] == (2, [0, -1], [0])                                # 50 <= TH_LOW: both cameras
    assert r["th_51"][:3] == (0, [-1, -1], [-1]) and r["th_51"][3]["right_refused_left_over_th_low"] == 1
    assert r["no_left_in_node"][:3] == (0, [-1], [-1]) and r["no_left_in_node"][3]["right_refused_no_left_candidate"] == 1
    assert r["left_ratio_fails"][:3] == (1, [-1, -1, -1], [-1, 0]) and r["left_ratio_fails"][3]["right_claimed_left_ratio_failed"] == 1
    assert r["right_tie"][:3] == (2, [0, -1], [-1, 0, -1]) and r["right_tie"][3]["right_claimed_best_equals_runner_up"] == 1   # first index
    assert r["left_tie"][:3] == (1, [-1, -1, -1, -1], [0])
    assert r["second_best"][:3] == (4, [-1, 1, 0], [1, -1, 0])
    assert r["second_best"][3]["skipped_claimed_left"] == 1 and r["second_best"][3]["skipped_claimed_right"] == 1
    assert r["right_exhausted"][:3] == (3, [0, 1, -1], [0])
    assert r["hash_collision"][:3] == (4, [1, 0, -1, -1, -1], [1, 0, -1])
    assert r["stopped_and_holes"][:3] == (2, [-1, 2, -1], [-1, 2])
    n, le, ri, t = r["cull_both_rows"]
    assert n == 23 and le == list(range(11)) + [-1, -1] and ri == list(range(11)) + [11, -1] and t["culled_left"] == 2 and t["culled_right"] == 1
    for name, nl, nr in (("long_70_0", 70, 0), ("long_6_70", 6, 70), ("long_60_10", 60, 10), ("long_64_1", 64, 1), ("long_63_2", 63, 2),
                         ("long_100_60", 100, 60), ("long_130_5", 130, 5)):
        b = bc.hand(0.7, 0)
        p = b.names.index(name)
        assert int((b.F["node"][2 * p, :b.F["counts"][2 * p]] == 7).sum()) == nl and int((b.F["node"][2 * p + 1, :b.F["counts"][2 * p + 1]] == 7).sum()) == nr
    r0 = _compare(OM, bc.hand(0.7, 0))                                        # without the cull: every KeyFrame feature finds its near copies
    for name, nl, nr in (("long_70_0", 6, 0), ("long_6_70", 6, 6), ("long_60_10", 6, 6), ("long_64_1", 6, 1), ("long_63_2", 6, 2),
                         ("long_100_60", 6, 6), ("long_130_5", 6, 5)):
        assert (sum(v >= 0 for v in r0[name][1]), sum(v >= 0 for v in r0[name][2])) == (nl, nr), name
    assert r0["cull_both_rows"][:3] == (26, list(range(13)), list(range(13)))
    assert r["empty_right"][:3] == (2, [0, 1, -1], []) and r["empty_left"][:3] == (0, [], [-1]) and r["empty_kf"][:3] == (0, [-1], [-1])
    r125 = _compare(OM, bc.hand(1.25, 1))                                     # nnratio > 1 lets a left tie through: the first index takes it
    assert r125["left_tie"][:3] == (2, [-1, 0, -1, -1], [0])
    rw = _compare(OM, bc.hand(0.7, 1, weights=False))                         # NULL weights: no word is stopped; the good_kf hole stays
    assert rw["stopped_and_holes"][:3] == (4, [0, 2, -1], [0, 2])


def test_every_counter_was_reached(OM, oracle, synth):
    """Run after the comparisons above in file order; on its own it walks the batches itself."""
    if not TOTAL:
        _compare(OM, bc.hand(0.7, 1)); _compare(OM, bc.scene(oracle, synth, 1, 0.7, 1))
    for k in COUNTERS:
        assert TOTAL[k] > 0, (k, dict(TOTAL))


# ---- the entry point, without a device ------------------------------------------------------------------------------------------
def _declared_types():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", txt)
    assert decl, NAME + " is not declared in orbm.h"
    params = [a.strip() for a in decl.group(1).split(",") if a.strip()]
    return [C.c_void_p if "*" in a else C.c_float if re.match(r"(const\s+)?float\b", a) else C.c_int for a in params]


def test_declared_exported_and_bound(pkg):
    want = _declared_types()
    assert len(want) == 25
    ints, floats = {1, 2, 3, 10, 11, 21}, {20}                                # npairs, nkf_rows, cap_kf, nf_rows, cap_f, check_orientation; nnratio
    assert all((want[i] is C.c_int) == (i in ints) and (want[i] is C.c_float) == (i in floats) for i in range(25))
    assert NAME in pkg.EXPORTS
    pkg.build()
    assert os.path.exists(AB_LIB), "the -DORBX_AB build of the library is missing"
    for path in (pkg.LIB_PATH, AB_LIB):
        assert hasattr(C.CDLL(path), NAME), path
    at = getattr(pkg.lib(), NAME).argtypes
    assert at is not None and list(at) == want
    assert hasattr(pkg.ORBmatcher, "SearchByBoWFisheyeBatchAsync")
    txt = open(os.path.join(ROOT, "include", "orbm.h")).read()
    assert re.search(r"enum\s*\{\s*ORBM_BOW_FISHEYE_MAX_CAP_F\s*=\s*12288\s*\}", txt)
    assert 2 * 24576 + 8 * 12288 + 10408 == 157864 <= 160 * 1024              # the LDS bound the header publishes


def test_refusals_fire_without_a_device(pkg):
    """Every ORBM_E_INVALID / ORBM_E_CAPACITY check runs before the handle is read or a device is touched: the handle here is a block
    of zero bytes and the arrays are host memory nobody may read.  From both builds of the library."""
    want = _declared_types()
    pkg.build()
    for path in (pkg.LIB_PATH, AB_LIB):
        L = C.CDLL(path)
        fn = getattr(L, NAME)
        fn.argtypes = want
        fn.restype = C.c_int
        L.orbm_last_error.restype = C.c_char_p
        fake = (C.c_uint8 * 4096)()
        buf = (C.c_uint8 * 4096)()
        p = C.addressof(buf)

        def call(handle=C.addressof(fake), npairs=1, nkr=1, capk=4, nfr=1, capf=4, nn=0.7, **null):
            a = dict(kps_kf=p, desc_kf=p, counts_kf=p, node_kf=p, weight_kf=None, good_kf=p, kps_f=p, desc_f=p, counts_f=p, node_f=p,
                     weight_f=None, kf_row=None, fl_row=p, fr_row=p, f_match_l=p, f_match_r=p, nmatches=p)
            a.update(null)
            return fn(handle, npairs, nkr, capk, a["kps_kf"], a["desc_kf"], a["counts_kf"], a["node_kf"], a["weight_kf"], a["good_kf"],
                      nfr, capf, a["kps_f"], a["desc_f"], a["counts_f"], a["node_f"], a["weight_f"], a["kf_row"], a["fl_row"], a["fr_row"],
                      nn, 1, a["f_match_l"], a["f_match_r"], a["nmatches"])
        assert call(handle=None) == -2
        for k in ("kps_kf", "desc_kf", "counts_kf", "node_kf", "good_kf", "kps_f", "desc_f", "counts_f", "node_f", "fl_row", "fr_row",
                  "f_match_l", "f_match_r", "nmatches"):
            assert call(**{k: None}) == -2, k
        assert call(npairs=0) == -2 and call(nkr=0) == -2 and call(nfr=0) == -2 and call(capk=0) == -2 and call(capf=0) == -2
        assert call(nn=float("nan")) == -2 and call(nn=float("inf")) == -2
        assert call(capf=12289) == -3 and b"12288" in L.orbm_last_error()
        assert call(capk=24577) == -3 and b"24576" in L.orbm_last_error()
        assert call(npairs=65536) == -3 and b"65535" in L.orbm_last_error()
        assert bytes(fake) == bytes(4096) and bytes(buf) == bytes(4096)


def test_contract_comment_names_the_rules():
    """The header carries the contract where callers read it."""
    txt = open(os.path.join(ROOT, "include", "orbm.h")).read()
    c = txt[txt.index("/* " + NAME):txt.index("int " + NAME)]
    for phrase in (":406-433", ":473", ":409", "Tracking.cc:3006", "Tracking.cc:4201", "three differences", "fl_row[p]", "fr_row[p]", "Nleft + j",
                   "the LEFT distance", "|| true", "ONE histogram", "ONE stacked row", "ORBM_BOW_FISHEYE_MAX_CAP_F", "ORBM_BOW_MAX_CAP", "157864",
                   "orbx_capture_begin", "ORBM_E_INVALID", "ORBM_E_CAPACITY", "65535", "before the device is"):
        assert phrase in c, phrase
