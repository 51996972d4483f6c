"""The CPU oracle's DBoW2 transform (oracle/orbref_bow.cpp) and isInFrustum (oracle/orbref_frame.cpp) against the second reading of
TemplatedVocabulary.h:1126-1259 / :1338-1424 and Frame.cc:603-699 (tests/second_reading_frame.py), on the case sets of
tests/frame_cases.py: word, node and weight of every row, the BowVector's doubles byte for byte, every frustum output byte for byte
except the level of the cases the reading marks ambiguous.  Hand-computed answers keep the reading from drifting along with the
oracle, and the reading's branch counters prove that every constructed case reached the branch it was built for.  No GPU.

Outcome of the comparison when it was written: the oracle and the reading agree on every case; the only differences are levels of
ambiguous cases (the oracle's logf against the exact quotient), which is what the ambiguity band exists for."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import frame_cases as fc
import second_reading_frame as srf

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
_MEMO, _BOW_DONE, _FRUSTUM_DONE = {}, {}, {}     # each reading and each comparison runs once, whichever test asks first


def bow_reading(name):
    """name -> (voc, rows, {levelsup: transform(...)}), computed once and shared (the GPU file reuses it)."""
    if name not in _MEMO:
        tree = fc.bow_tree(name)
        voc, _ = srf.vocab_from_arrays(tree["k"], tree["L"], tree["parent"], tree["is_leaf"], tree["desc"], tree["weight"])
        rows = fc.bow_features(tree, voc)
        _MEMO[name] = (voc, rows, {lu: srf.transform(voc, rows, lu, unwritten_nid=0) for lu in fc.levelsups(tree["L"])})
    return _MEMO[name]


def nodes_as_documented(nids):
    """include/orbm.h: a node id the reference leaves unwritten is 0."""
    return np.array([0 if x is None else x for x in nids], np.int32)


def fv_csr(fv):
    """[(node, [features])] -> the (nodes, start, idx) arrays of the C ABI."""
    start = np.cumsum([0] + [len(l) for _, l in fv]).astype(np.int32)
    return np.array([n for n, _ in fv], np.int32), start, np.array([i for _, l in fv for i in l], np.int32)


def keys(t, kind):
    return {k[1:] for k in t if isinstance(k, tuple) and k[0] == kind}


def test_second_reading_imports_neither_oracle_nor_product():
    for name, allowed in (("second_reading_frame.py", {"math", "collections", "mpmath", "numpy", "second_reading"}),
                          ("frame_cases.py", {"mpmath", "numpy", "second_reading_frame"})):
        src = open(os.path.join(HERE, name)).read()
        assert set(re.findall(r"^\s*(?:from|import)\s+([\w\.]+)", src, flags=re.M)) == allowed, name
        for word in ("orbref", "orb-slam3_amd", "importlib", "ctypes", "__import__", "liborb"):
            assert word not in src, (name, word)


# ---------------------------------------------------------------------------------------------------------------------------
# DBoW2
# ---------------------------------------------------------------------------------------------------------------------------
def test_hand_computed_transform():
    """Two words, all-zero and all-one descriptors, weights 2 and 6, L = 1."""
    desc = np.zeros((3, 32), np.uint8); desc[2] = 255
    voc, t = srf.vocab_from_arrays(2, 1, [0, 0, 0], [0, 1, 1], desc, [0.0, 2.0, 6.0])
    assert voc.info() == dict(k=2, L=1, nnodes=3, nwords=2) and t["word"] == 2
    half = np.zeros(32, np.uint8); half[:16] = 255                          # 128 bits from either word: the earlier child keeps the tie
    near1 = np.full(32, 255, np.uint8); near1[0] = 0                         # 8 bits from word 1, 248 from word 0
    rows = np.array([desc[1], desc[2], near1, half])
    assert [srf.transform_one(voc, r, 0)[:3] for r in rows] == [(0, 2.0, 1), (1, 6.0, 2), (1, 6.0, 2), (0, 2.0, 1)]
    assert srf.transform_one(voc, half, 0)[3][("tie", 0, 1)] == 1 and srf.transform_one(voc, near1, 0)[3][("best_d", 8)] == 1
    assert [srf.transform_one(voc, r, 1)[2] for r in rows] == [0, 0, 0, 0]    # nid_level = 0: the root
    ids, vals, fv, w, nids, wt, t = srf.transform(voc, rows, 0)
    # v = {0: 2 + 2, 1: 6 + 6}, norm 16
    assert list(ids) == [0, 1] and list(vals) == [0.25, 0.75] and fv == [(1, [0, 3]), (2, [1, 2])]
    assert t["addWeight_insert"] == 2 and t["addWeight_accumulate"] == 2 and t["normalized"] == 1


def test_hand_computed_bow_vector_keeps_the_order_of_the_sums():
    # addWeight in feature order: 0.1 + 0.1 + 0.1 is not 3 * 0.1
    ids, vals, fv, t = srf.bow_and_feature_vector([5, 5, 5], [9, 9, 9], [0.1, 0.1, 0.1])
    assert list(ids) == [5] and list(vals) == [1.0] and fv == [(9, [0, 1, 2])]
    ids, vals, fv, t = srf.bow_and_feature_vector([5, 5, 5, 2], [9, 8, 9, 9], [0.1, 0.1, 0.1, 1.0])
    assert 0.1 + 0.1 + 0.1 == 0.30000000000000004
    assert list(ids) == [2, 5] and list(vals) == [1.0 / (1.0 + 0.30000000000000004), 0.30000000000000004 / (1.0 + 0.30000000000000004)]
    assert fv == [(8, [1]), (9, [0, 2, 3])]
    # normalize sums in ascending WORD id, whatever the feature order: (1e16 + 1) + 1 = 1e16, but (1 + 1) + 1e16 = 1e16 + 2
    ids, vals, _, _ = srf.bow_and_feature_vector([3, 1, 2], [0, 0, 0], [1e16, 1.0, 1.0])
    assert list(vals) == [1.0 / (1e16 + 2), 1.0 / (1e16 + 2), 1e16 / (1e16 + 2)]
    ids, vals, _, _ = srf.bow_and_feature_vector([1, 2, 3], [0, 0, 0], [1e16, 1.0, 1.0])
    assert list(vals) == [1.0, 1e-16, 1e-16]
    # stopped words: zero, negative (and NaN) weights enter neither vector; nothing left: no division
    ids, vals, fv, t = srf.bow_and_feature_vector([1, 2, 3], [4, 5, 6], [0.0, -2.0, float("nan")])
    assert len(ids) == 0 and len(vals) == 0 and fv == [] and t["norm_zero_no_division"] == 1
    assert t["stopped_zero"] == 1 and t["stopped_negative"] == 1 and t["stopped_nan"] == 1


def test_hand_computed_node_levels_and_the_unwritten_node():
    tree = fc.hand_tree()
    voc, _ = srf.vocab_from_arrays(tree["k"], tree["L"], tree["parent"], tree["is_leaf"], tree["desc"], tree["weight"])
    root = voc.nodes[0].children
    assert [len(voc.nodes[c].children) for c in root[:4]] == [16, 1, 31, 0] and len(root) == 31
    a, a0 = root[0], voc.nodes[root[0]].children[0]
    assert a0 == a + 1 and voc.nodes[a0].children == list(range(a0 + 1, a0 + 21))        # depth-first ids: a subtree before the next sibling
    leaf3 = voc.nodes[a0].children[7]; leaf2 = voc.nodes[a].children[5]; leaf1 = root[9]
    for leaf, depth, want in ((leaf3, 3, {0: leaf3, 1: a0, 2: a, 3: 0, 5: 0}), (leaf2, 2, {0: None, 1: leaf2, 2: a, 3: 0, 5: 0}),
                              (leaf1, 1, {0: None, 1: None, 2: leaf1, 3: 0, 5: 0})):
        for lu, nid in want.items():
            wid, w, got, t = srf.transform_one(voc, voc.nodes[leaf].descriptor, lu)
            assert (wid, w, got) == (voc.nodes[leaf].word_id, voc.nodes[leaf].weight, nid), (leaf, lu, got, nid)
            assert t[("leaf_depth", depth)] == 1 and t["nid_unwritten"] == (nid is None) and t["nid_root"] == (lu >= 3)
    # the TIES duplicates: the row of child 30 (a leaf at depth 1) ties with child 0 (A) at distance 0, and the descent goes on below A
    wid, w, nid, t = srf.transform_one(voc, voc.nodes[root[30]].descriptor, 2)
    assert nid == a and t[("tie", 0, 30)] == 1 and t[("leaf_depth", 1)] == 0
    assert srf.transform_one(voc, voc.nodes[root[17]].descriptor, 2)[2] == root[3]
    assert srf.transform_one(voc, voc.nodes[root[16]].descriptor, 2)[2] == root[15]


def test_text_and_arrays_build_the_same_vocabulary(tmp_path, oracle):
    tree = fc.bow_tree("k17_L3")
    path = str(tmp_path / "voc.txt")
    open(path, "w").write(fc.tree_text(tree))
    a, ta = srf.vocab_from_text(path)
    b, _ = srf.vocab_from_arrays(tree["k"], tree["L"], tree["parent"], tree["is_leaf"], tree["desc"], tree["weight"])
    assert ta["trailing_empty_line"] == 1 and a.info() == b.info() == oracle.Vocabulary(path).info()
    for x, y in zip(a.nodes, b.nodes):
        assert (x.id, x.parent, x.children, x.weight, x.word_id) == (y.id, y.parent, y.children, y.weight, y.word_id)
        assert x.id == 0 or np.array_equal(x.descriptor, y.descriptor)
    open(path, "w").write(fc.tree_text(tree).rstrip("\n"))                   # no final newline: the reference's loop ends on the last node
    c, tc = srf.vocab_from_text(path)
    assert tc["trailing_empty_line"] == 0 and c.info() == a.info()
    for bad in ("21 3 0 0\n", "10 0 0 0\n", "10 11 0 0\n", "10 3 6 0\n", "10 3 0 4\n", "-1 3 0 0\n"):     # :1359
        open(path, "w").write(bad)
        with pytest.raises(ValueError):
            srf.vocab_from_text(path)
    open(path, "w").write("10 3 1 2\n")                                      # in range: the reference loads it and switches transform on it
    d, _ = srf.vocab_from_text(path)
    assert (d.scoring, d.weighting) == (1, 2)
    with pytest.raises(AssertionError):
        srf.transform(d, np.zeros((1, 32), np.uint8), 0)


def bow_oracle_equals_reading(oracle, name):
    """Holds the oracle to the reading on one tree, once; returns the reading's counters summed over the tree's levelsups."""
    if name in _BOW_DONE:
        return _BOW_DONE[name]
    seen = Counter()
    voc, rows, by_lu = bow_reading(name)
    ref = oracle.Vocabulary(fc.bow_tree(name))
    assert ref.info() == voc.info()
    for lu, (ids, vals, fv, w, nids, wt, t) in by_lu.items():
        (rbi, rbv), (rfn, rfs, rfi), rw, rnd, rwt = ref.transform(rows, lu)
        assert np.array_equal(w, rw) and np.array_equal(nodes_as_documented(nids), rnd) and wt.tobytes() == rwt.tobytes(), lu
        assert np.array_equal(ids, rbi) and vals.tobytes() == rbv.tobytes(), lu
        fn, fs, fi = fv_csr(fv)
        assert np.array_equal(fn, rfn) and np.array_equal(fs, rfs) and np.array_equal(fi, rfi), lu
        seen.update(t)
    for n in fc.COUNTS:                                                       # the prefixes the device tests take
        ids, vals, fv, w, nids, wt, t = by_lu[0]
        got = srf.bow_and_feature_vector(w[:n], nodes_as_documented(nids[:n]), wt[:n])
        (rbi, rbv), (rfn, rfs, rfi), _, _, _ = ref.transform(rows[:n], 0)
        assert np.array_equal(got[0], rbi) and got[1].tobytes() == rbv.tobytes() and np.array_equal(fv_csr(got[2])[2], rfi)
    _BOW_DONE[name] = seen
    return seen


@pytest.mark.parametrize("name", fc.TREE_NAMES)
def test_bow_oracle_equals_second_reading(oracle, name):
    bow_oracle_equals_reading(oracle, name)


@pytest.fixture(scope="module")
def bow_seen(oracle):
    """tree name -> the reading's counters over that tree's comparison (run here if no test has run it yet)."""
    return {name: bow_oracle_equals_reading(oracle, name) for name in fc.TREE_NAMES}


def test_every_constructed_bow_case_reached_its_branch(bow_seen):
    for name, k in (("k17_L2", 17), ("k17_L3", 17), ("k20_L2", 20), ("k20_L3", 20)):
        t = bow_seen[name]
        assert keys(t, "children") == {(k,)}
        assert keys(t, "winner") == {(p,) for p in range(k)}, name            # every child position wins somewhere, the second chunk's included
        assert (15, 16) in keys(t, "tie") and ((3, 17) in keys(t, "tie")) == (k > 17)
        assert (0,) in keys(t, "best_d") and t["nid_root"] > 0 and t["nid_written"] > 0 and t["nid_unwritten"] == 0
        assert t["stopped_zero"] > 0 and t["stopped_negative"] > 0
    t = bow_seen["hand"]
    assert keys(t, "children") == {(31,), (16,), (1,), (20,)} and keys(t, "leaf_depth") == {(1,), (2,), (3,)}
    assert {(3, 17), (15, 16), (0, 30)} <= keys(t, "tie")
    assert {(19,), (29,)} <= keys(t, "winner")                               # strict minima in the second chunk of 16 (child 30 is a twin of child 0 in both nodes of 31)
    assert t["nid_unwritten"] > 0 and t["nid_unwritten_filed"] > 0
    t = bow_seen["hand_stopped"]
    assert t["addWeight_insert"] == 0 and t["norm_zero_no_division"] == 5 and t["stopped_zero"] > 0 and t["stopped_negative"] > 0
    t = bow_seen["identical"]
    assert (256,) in keys(t, "best_d") and {(0, 1), (0, 2)} <= keys(t, "tie") and keys(t, "winner") == {(0,)}
    t = bow_seen["magnitudes"]
    assert t["addWeight_accumulate"] >= 40 * 3


def test_rows_of_one_wave_end_at_different_depths():
    voc, rows, _ = bow_reading("hand")
    depth = [list(keys(srf.transform_one(voc, r, 0)[3], "leaf_depth"))[0][0] for r in rows[:68]]
    assert all(len(set(depth[i:i + 4])) == 3 for i in range(0, 68, 4)), depth


def test_forty_features_on_one_word_and_weights_of_very_different_magnitude(oracle, pkg):
    """orbm_bow_vectors' contract on arrays: 40 features of ONE word with weights over 30 decades (addWeight adds in feature order), between
    words that make the norm's order visible.  Any other order of either sum gives other doubles."""
    w, nd, wt = bow_arrays()
    ids, vals, fv, t = srf.bow_and_feature_vector(w, nd, wt)
    assert t["addWeight_accumulate"] == 39 + 2
    (bi, bv), (fn, fs, fi) = pkg.bow_vectors(oracle.lib().orbref_bow_vectors, len(w), w, nd, wt)
    assert np.array_equal(bi, ids) and bv.tobytes() == vals.tobytes() and np.array_equal(fi, fv_csr(fv)[2])
    acc = rev = 0.0
    for x in wt[w == 7]:
        acc += x
    for x in wt[w == 7][::-1]:
        rev += x
    assert acc != rev                                                        # the order IS visible in this data
    assert vals[list(ids).index(7)] == acc / sum_in_order(ids, w, wt)


def bow_arrays():
    rng = np.random.default_rng(40)
    wt7 = 10.0 ** rng.uniform(-15, 15, 40)
    w = np.concatenate([[3, 9], np.full(40, 7), [1, 9, 3]]).astype(np.int32)
    wt = np.concatenate([[1e15, 0.3], wt7, [1e-15, 0.3, 1.0]])
    nd = (np.arange(len(w)) % 5).astype(np.int32)
    return w, nd, wt


def sum_in_order(ids, w, wt):
    norm = 0.0
    for wid in ids:
        acc = 0.0
        for x in wt[w == wid]:
            acc += x
        norm += abs(acc)
    return norm


# ---------------------------------------------------------------------------------------------------------------------------
# isInFrustum + PredictScale
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def OM(oracle):
    return oracle._oracle_matcher_class()()


def compare_frustum(what, got, want, ambiguous):
    """Every output bit for bit (NaN included), everywhere; the one exception is the level of ambiguous cases.  Returns the number of
    ambiguous levels that differ."""
    for key in ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos"):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.tobytes() == b.tobytes(), (what, key, np.nonzero(a.view(np.uint8 if key == "in_view" else np.uint32) != b.view(np.uint8 if key == "in_view" else np.uint32))[0][:8])
    diff = np.asarray(got["level"]) != want["level"]
    assert not np.any(diff & ~ambiguous), (what, "level", np.nonzero(diff & ~ambiguous)[0][:8], np.asarray(got["level"])[diff & ~ambiguous][:8], want["level"][diff & ~ambiguous][:8])
    assert np.all((np.abs(np.asarray(got["level"]).astype(int) - want["level"]) <= 1)[ambiguous]), (what, "an ambiguous level is off by more than one")
    return int(np.sum(diff & ambiguous))


def check_frustum_expectations(case, out, ambiguous, t):
    for key, n in case.expect.items():
        assert t[key] >= n, (case.name, key, t[key], n)
    for i, w in case.points.items():
        assert out["in_view"][i] == w["in_view"], (case.name, i, w)
        if "proj_set" in w:
            assert (out["proj_x"][i] != -1 and out["proj_y"][i] != -1) == w["proj_set"], (case.name, i, w, out["proj_x"][i])
        if w.get("nan"):
            assert np.isnan(out["proj_x"][i]) and np.isnan(out["proj_y"][i]), (case.name, i)
        if w["in_view"] and "level" in w:
            assert out["level"][i] == w["level"], (case.name, i, w, out["level"][i])
        if w["in_view"] and "ambiguous" in w:
            assert ambiguous[i] == w["ambiguous"], (case.name, i, w)


def test_hand_computed_frustum():
    """Identity pose, fx = fy = 100, cx = 50, cy = 40, bf = 40, P = (1, 2, 4): u = 100 * 1 / 4 + 50 = 75, v = 100 * 2 / 4 + 40 = 90,
    uR = 75 - 40 / 4 = 65, depth = dist = sqrt(21), viewCos = 4 / sqrt(21) against the normal (0, 0, 1); max distance twice the distance:
    q = log 2 / log 1.2 = 3.8018, level 4."""
    s21 = F(np.sqrt(21.0))
    scene = dict(pw=np.array([[1, 2, 4]] * 6, F), normal=np.array([[0, 0, 1]] * 6, F), rcw=np.eye(3, dtype=F).reshape(9), tcw=np.zeros(3, F), ow=np.zeros(3, F),
                 min_dist=np.array([1, 1, 1, 1, 6, 1], F), max_dist=np.array([2 * s21, 2 * s21, 2 * s21, 2 * s21, 2 * s21, 3], F))
    scene["pw"][1] = [1, 2, -4]; scene["pw"][2] = [3, 2, 4]; scene["normal"][3] = [0, 1, 0]
    case = fc.FrustumCase("hand", scene, k=[100, 100, 50, 40], bounds=[0, 100, 0, 90], bf=40.0, cos_limit=0.5)
    out, amb, t = case.reading(init={"proj_xr": np.full(6, 7, F), "depth": np.full(6, 7, F), "view_cos": np.full(6, 7, F), "level": np.full(6, 7)})
    assert list(out["in_view"]) == [1, 0, 0, 0, 0, 0] and not amb.any()
    assert (out["proj_x"][0], out["proj_y"][0], out["proj_xr"][0], out["depth"][0], out["level"][0]) == (75, 90, 65, s21, 4) and t["v_on_maxY"] == 4
    assert out["view_cos"][0] == F(F(4) / s21)
    # 1: behind the camera; 2: u = 125 beyond maxX; 3: viewCos = 2 / sqrt(21) < 0.5; 4: dist < 0.8f * 6; 5: dist > 1.2f * 3.  3-5 keep their projection
    assert list(out["proj_x"][1:]) == [-1, -1, 75, 75, 75] and list(out["proj_y"][1:]) == [-1, -1, 90, 90, 90]
    assert t["PcZ_negative"] == 1 and t["u_above_maxX"] == 1 and t["viewCos_below_limit"] == 1 and t["dist_below_min"] == 1 and t["dist_above_max"] == 1
    for key in ("proj_xr", "depth", "view_cos", "level"):                    # written only where in view
        assert np.all(out[key][1:] == 7), key


def test_hand_computed_predict_scale():
    lsf = fc.LSF
    for ratio, level in ((1.0, 0), (1.1, 1), (1.2 ** 1.5, 2), (2.0, 4), (3.5, 7), (3.6, 7), (100.0, 7), (0.9, 0), (0.5, 0)):
        got, amb, q, t = srf.predict_scale(F(ratio), F(1.0), lsf, 8)
        assert got == level and not amb, (ratio, got, float(q))
        assert t["clamped_high"] == (ratio >= 3.6) and t["clamped_low"] == (ratio == 0.5) and t["ratio_one_exact"] == (ratio == 1.0)
    assert abs(float(srf.scale_quotient(F(2.0), lsf)) - np.log(2.0) / lsf) < 1e-12
    # ratio = 1.2f against logScaleFactor = (float)log(1.2f): q is 1 up to the rounding of logScaleFactor, inside the band around m = 1
    got, amb, q, t = srf.predict_scale(F(1.2), F(1.0), lsf, 8)
    assert amb and abs(float(q) - 1.0) <= fc.band(1.0) and t["ambiguous_level"] == 1
    assert srf.predict_scale(F(1.2), F(1.0), lsf, 3)[1] and not srf.predict_scale(F(1.2), F(1.0), lsf, 2)[1]       # m = 1 > nlevels - 2: both sides clamp
    for ratio in (0.0, -1.0, np.inf, np.nan):
        assert srf.predict_scale(F(ratio), F(1.0), lsf, 8)[0] is None


def test_ratios_around_every_level_lie_just_outside_the_band():
    for m in range(fc.NLEVELS):
        lo, inside, hi = fc.ratios_around(m)
        qlo, qhi = float(srf.scale_quotient(lo, fc.LSF)), float(srf.scale_quotient(hi, fc.LSF))
        assert m - 4 * fc.band(m) < qlo < m - fc.band(qlo) and m + fc.band(qhi) < qhi < m + 4 * fc.band(m), (m, qlo, qhi)
        assert inside and all(abs(float(srf.scale_quotient(r, fc.LSF)) - m) <= fc.band(m) * 1.0001 for r in inside)
        assert np.nextafter(lo, F(np.inf)) in inside + [F(1.0)] and np.nextafter(hi, F(-np.inf)) in inside + [F(1.0)]     # nothing skipped


def frustum_oracle_equals_reading(OM, name):
    """Holds the oracle to the reading on one constructed case, once; returns the reading's counters."""
    if name in _FRUSTUM_DONE:
        return _FRUSTUM_DONE[name]
    case = fc.frustum_case(name)
    out, amb, t = case.reading()
    cnt, exp = OM.isInFrustum(*case.args())
    # the oracle's wrapper hands in zeros and level -1, the reading's defaults
    differ = compare_frustum(case.name, exp, out, amb)
    assert cnt == int(out["in_view"].sum())
    print(case.name, dict(t), "ambiguous levels that differ from the oracle's logf:", differ)
    check_frustum_expectations(case, out, amb, t)
    _FRUSTUM_DONE[name] = t
    return t


def random_scene_oracle_equals_reading(OM, n):
    if ("random", n) in _FRUSTUM_DONE:
        return _FRUSTUM_DONE[("random", n)]
    case = fc.FrustumCase("random", fc.random_scene(n, 100 + n))
    out, amb, t = case.reading()
    cnt, exp = OM.isInFrustum(*case.args())
    compare_frustum("random %d" % n, exp, out, amb)
    assert cnt == t["in_view"]
    if n == fc.BIG:
        share = amb.sum() / n
        print("ambiguous share of the random scene: %d of %d" % (amb.sum(), n))
        assert share <= 0.001                                                # measured when written: 0 of 2000
        assert 0.2 * n < cnt < 0.8 * n and all(t[b] > 0 for b in srf.FRUSTUM_BRANCHES)
    _FRUSTUM_DONE[("random", n)] = t
    return t


@pytest.mark.parametrize("name", fc.FRUSTUM_NAMES)
def test_constructed_frustum_case_oracle_equals_second_reading(OM, name):
    frustum_oracle_equals_reading(OM, name)


@pytest.mark.parametrize("n", fc.POINT_COUNTS + (fc.BIG,))
def test_random_scene_oracle_equals_second_reading(OM, n):
    random_scene_oracle_equals_reading(OM, n)


def test_every_frustum_branch_and_edge_was_reached(OM):
    """Over the constructed cases and the large random scene (each compared here if no test has compared it yet)."""
    seen = Counter()
    for name in fc.FRUSTUM_NAMES:
        seen.update(frustum_oracle_equals_reading(OM, name))
    seen.update(random_scene_oracle_equals_reading(OM, fc.BIG))
    for b in srf.FRUSTUM_BRANCHES + ("u_on_minX", "u_on_maxX", "v_on_minY", "v_on_maxY", "dist_on_min", "dist_on_max", "viewCos_on_limit", "PcZ_zero",
                                     "PcZ_subnormal", "projection_non_finite", "proj_kept_after_reject", "ambiguous_level", "ratio_one_exact",
                                     "clamped_low", "clamped_high"):
        assert seen[b] > 0, b
    assert seen["level_undefined"] == 0                                      # no case relies on the undefined conversion


def test_projection_lies_within_its_rounding_margin_of_the_exact_value():
    """The reading itself against exact arithmetic: a wrong operation order in the reading (or in the rule it restates) would show here
    independently of the oracle.  The margin is derived in frame_cases.exact_projection."""
    case = fc.frustum_case("on_the_four_bounds")
    out, _, _ = case.reading()
    u, v, mu, mv = fc.exact_projection(case)
    s = (out["proj_x"] != -1) & np.isfinite(mu)
    assert s.sum() > 100
    assert np.all(np.abs(out["proj_x"][s].astype(np.float64) - u[s]) <= mu[s]) and np.all(np.abs(out["proj_y"][s].astype(np.float64) - v[s]) <= mv[s])
    ulps = mu[s] / np.spacing(np.abs(out["proj_x"][s])).astype(np.float64)
    assert np.median(ulps) < 8, np.median(ulps)                              # "a few float ulps" for a well-conditioned point
