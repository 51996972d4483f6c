"""The CPU oracle's matcher searches against tests/second_reading.py, entry for entry (no GPU).

The oracle (oracle/orbref_frame.cpp, orbref_match.cpp), the host claim replays and the device kernels are restatements of the
reference's ORBmatcher.cc by one author; second_reading.py is a separate reading of the same reference lines in Python that shares
no code with them.  Every search that has a batched device form is run here through both on extractor scenes, and on constructed
cases placed where two plausible readings of the reference differ; each constructed case proves from the second reading's trace
that it reached the branch it was built for.
"""
import os
import re

import numpy as np
import pytest

import second_reading as sr

F = np.float32
SCENES = {"pair": (376, 240, 500, 321), "large": (752, 480, 1000, 77)}


def _sf():
    return np.cumprod(np.concatenate([[F(1)], np.full(7, F(1.2))]).astype(np.float32)).astype(np.float32)


@pytest.fixture(scope="module")
def OM(pkg, oracle):
    return oracle._oracle_matcher_class()()


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene(request, pkg, oracle, synth, OM):
    W, H, NF, seed = SCENES[request.param]
    l, r = synth.gen_stereo_pair(W, H, seed)
    ex = oracle.Extractor(NF)
    _, kl, dl, _ = ex(l, (0, 0)); _, kr, dr, _ = ex(r, (0, 0))
    if request.param == "large":                       # one frame, matched against itself: ties are decided by visiting order
        kl, dl = kr.copy(), dr.copy()
    sf = _sf()
    return dict(name=request.param, W=W, H=H, kl=kl, dl=dl, kr=kr, dr=dr, sf=sf, sigma2=(sf * sf).astype(np.float32))


def _view(pkg, OM, k, d, W, H, ur=None):
    v = pkg.FrameView(k, d, W, H, uright=ur, backend=OM)
    g = sr.GridFrame(v.kps, v.desc, v.min_x, v.min_y, v.inv_w, v.inv_h, v.uright)
    return v, g


def _same(got, want, what=""):
    """oracle (count, row) == second reading (count, row, trace)."""
    assert int(got[0]) == int(want[0]), "%s: count %d (oracle) != %d (second reading)" % (what, got[0], want[0])
    bad = np.nonzero(np.asarray(got[1]) != np.asarray(want[1]))[0]
    assert len(bad) == 0, "%s: rows differ at %s: oracle %s, second reading %s" % (what, bad[:8], got[1][bad[:8]], want[1][bad[:8]])
    return want[2]


def _fv(pkg, nodes):
    return pkg.feature_vector_csr(np.asarray(nodes, np.int64))


def _fv_desc(pkg, desc, bits):
    return _fv(pkg, desc[:, 0].astype(np.int64) & ((1 << bits) - 1))


def _queries(k, rng, shift=12.0, jitter=3.0):
    n = len(k)
    return n, (k["x"] - F(shift) + rng.normal(0, jitter, n)).astype(np.float32), (k["y"] + rng.normal(0, jitter / 3, n)).astype(np.float32)


# ---- the pieces the searches stand on -------------------------------------------------------------------------------------
def test_second_reading_is_independent():
    """The second reading may not reach the oracle, the product or ctypes (modelled on test_abi.py's product / oracle wall)."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "second_reading.py")).read().lower()
    for word in ("ctypes", "orbref", "liborb", "orb-slam3_amd", "orb_slam3_amd"):
        assert word not in src, "tests/second_reading.py mentions %r" % word
    assert not re.search(r"^\s*(import|from)\s+(?!math\b|collections\b|numpy\b)", src, re.M), "only math, collections and numpy are imported"


def test_descriptor_distance_swar(oracle):
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (64, 32), dtype=np.uint8); b = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    a[0] = 0; b[0] = 255; a[1] = b[1]; a[2] = 0x80; b[2] = 0x7F
    for i in range(64):
        want = int(np.unpackbits(np.bitwise_xor(a[i], b[i])).sum())
        assert sr.descriptor_distance(a[i], b[i]) == want == oracle.hamming(a[i], b[i])
    assert sr.descriptor_distances(a[3], b).tolist() == [int(np.unpackbits(a[3] ^ x).sum()) for x in b]
    assert sr.descriptor_distance(a[0], b[0]) == 256


def test_three_maxima(oracle):
    rng = np.random.default_rng(2)
    cases = [np.zeros(30, int), np.full(30, 4), [20, 1] + [0] * 28, [20, 2] + [0] * 28, [20, 5, 1] + [0] * 27, [20, 5, 2] + [0] * 27,
             [0] * 27 + [3, 3, 3], [7, 7, 7, 7] + [0] * 26, [10, 1, 1] + [0] * 27, [0, 9, 0, 9, 9, 9] + [0] * 24, [11, 1] + [0] * 28, [29, 3, 2] + [0] * 27]
    cases += [rng.integers(0, m, 30) for m in (2, 3, 5, 12, 40, 200) for _ in range(20)]
    for c in cases:
        assert list(sr.compute_three_maxima(c)) == oracle.three_maxima(np.asarray(c)).tolist(), list(c)


def test_c_round_is_half_away_from_zero():
    assert [sr.c_round(x) for x in (0.5, 1.5, 2.5, -0.5, -2.5, 2.4999998, 29.5)] == [1, 2, 3, -1, -3, 2, 30]
    assert int(np.round(F(2.5))) == 2                                  # numpy's own round would not do


def test_grid_and_area_queries(pkg, OM, scene):
    W, H = scene["W"], scene["H"]
    v, g = _view(pkg, OM, scene["kr"], scene["dr"], W, H)
    start, idx = g.csr()
    assert g.placed == v.placed and np.array_equal(start, v.grid_start) and np.array_equal(idx, v.grid_idx[:v.placed])
    rng = np.random.default_rng(3)
    t = sr.Counter()
    for q in range(120):
        x, y, r = rng.uniform(-30, W + 30), rng.uniform(-30, H + 30), rng.uniform(2, 60)
        if q % 7 == 0:                                                  # a keypoint exactly r away: the box test is strict
            j = int(rng.integers(len(v.kps))); r = float(F(2 ** int(rng.integers(1, 5))))
            x, y = float(F(v.kps["x"][j]) - F(r)), float(v.kps["y"][j])
        if q % 13 == 1:                                                 # windows wholly outside the grid, on each side
            x, y = [(-80.0, 50.0), (W + 90.0, 50.0), (50.0, -90.0), (50.0, H + 90.0)][(q // 13) % 4]
        lo = int(rng.integers(-1, 6)); hi = lo + int(rng.integers(-2, 3))
        if q % 5 == 0:
            lo, hi = [(-1, 2), (0, -1), (-1, -1), (0, 0), (3, -1)][(q // 5) % 5]
        got = OM.features_in_area(v, x, y, r, lo, hi).tolist()
        assert got == g.features_in_area(x, y, r, lo, hi, t), (x, y, r, lo, hi)
        if lo <= 0 and hi < 0:
            assert got == g.kf_features_in_area(x, y, r, t)             # KeyFrame::GetFeaturesInArea: the same window without levels
    assert t["window_outside_grid"] > 0 and t["window_clipped"] > 0 and t["exactly_r_away"] > 0
    assert t["levels_unchecked_min0"] > 0 and t["levels_checked_min_negative"] > 0


def test_pos_in_grid_rounds_onto_the_far_edge(pkg, oracle, OM):
    W, H = 376, 240
    k = np.zeros(6, oracle.KP_DTYPE)
    k["x"] = [375.0, 10.0, 373.0, 0.0, 372.99, 5.875 * 2.5]; k["y"] = [10.0, 239.0, 237.0, 0.0, 237.4, 12.5]
    v, g = _view(pkg, OM, k, np.zeros((6, 32), np.uint8), W, H)
    start, idx = g.csr()
    assert g.placed == v.placed == 4 and np.array_equal(start, v.grid_start) and np.array_equal(idx, v.grid_idx[:4])
    assert g.trace["rounded_onto_edge"] == 2 and g.trace["not_placed"] == 2 and g.trace["half_way_cell"] >= 1


# ---- constructed scenes ---------------------------------------------------------------------------------------------------
class Lattice:
    """Clusters of keypoints 30 px apart, one query per cluster; a candidate is (dx, dy, octave, distance to the query)."""

    def __init__(self, oracle, W=376, H=240, seed=5):
        self.oracle, self.W, self.H = oracle, W, H
        self.rng = np.random.default_rng(seed)
        self.kp, self.desc, self.ur, self.blocked, self.q = [], [], [], [], []

    def add(self, cands, level=0, angle=0.0, obs=True, pos=None, same_as=None, **kw):
        if same_as is not None:
            pos, qd = self.q[same_as]["pos"], self.q[same_as]["desc"]
        else:
            k = len({q["pos"] for q in self.q})
            pos = pos or (30.0 + 30.0 * (k % 11), 30.0 + 30.0 * (k // 11))
            qd = self.rng.integers(0, 256, 32, dtype=np.uint8)
        first = len(self.kp)
        for c in cands:
            dx, dy, octv, dist = c[:4]
            o = dict(angle=0.0, ur=-1.0, blocked=False); o.update(c[4] if len(c) > 4 else {})
            bits = np.unpackbits(qd); bits[:dist] ^= 1
            self.kp.append((pos[0] + dx, pos[1] + dy, o["angle"], octv)); self.desc.append(np.packbits(bits))
            self.ur.append(o["ur"]); self.blocked.append(o["blocked"])
        q = dict(pos=pos, desc=qd, level=level, angle=angle, obs=obs, first=first, pxr=pos[0] - 5.0, view_cos=0.5, invzc=0.1, valid=True)
        q.update(kw)
        self.q.append(q)
        return len(self.q) - 1

    def arrays(self, pkg, OM, stereo=False):
        k = np.zeros(len(self.kp), self.oracle.KP_DTYPE)
        a = np.array(self.kp, np.float64).reshape(-1, 4)
        k["x"], k["y"], k["angle"], k["octave"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3].astype(np.int32)
        d = np.array(self.desc, np.uint8).reshape(-1, 32)
        ur = np.array(self.ur, np.float32) if stereo else None
        v, g = _view(pkg, OM, k, d, self.W, self.H, ur)
        col = lambda name, t: np.array([q[name] for q in self.q], t)
        Q = dict(x=np.array([q["pos"][0] for q in self.q], np.float32), y=np.array([q["pos"][1] for q in self.q], np.float32),
                 level=col("level", np.int32), angle=col("angle", np.float32), obs=col("obs", np.uint8), valid=col("valid", np.uint8),
                 pxr=col("pxr", np.float32), view_cos=col("view_cos", np.float32), invzc=col("invzc", np.float32),
                 desc=np.array([q["desc"] for q in self.q], np.uint8).reshape(-1, 32))
        return v, g, np.array(self.blocked, np.uint8), Q


def _m3(OM, v, g, blocked, Q, sf, th, nnratio, what):
    a = dict(blocked=blocked, scale_factors=sf, in_view=Q["valid"], px=Q["x"], py=Q["y"], pxr=Q["pxr"], view_cos=Q["view_cos"], level=Q["level"],
             qdesc=Q["desc"], mp_obs=Q["obs"], th=th, nnratio=nnratio)
    return _same(OM.SearchByProjectionPoints(v, **a), sr.search_by_projection_points(g, **a), what)


def _m4(OM, v, g, blocked, Q, sf, th, what, **kw):
    a = dict(scale_factors=sf, valid=Q["valid"], u=Q["x"], v=Q["y"], invzc=Q["invzc"], octave=Q["level"], angle=Q["angle"], qdesc=Q["desc"],
             mp_obs=Q["obs"], th=th, **kw)
    return _same(OM.SearchByProjectionFrame(v, cur_blocked=blocked, **a), sr.search_by_projection_frame(g, cur_blocked=blocked, **a), what)


def _m5(OM, v, g, blocked, Q, sf, th, orb_dist, check_ori, what):
    a = dict(blocked=blocked, scale_factors=sf, valid=Q["valid"], u=Q["x"], v=Q["y"], level=Q["level"], angle=Q["angle"], qdesc=Q["desc"], th=th,
             orb_dist=orb_dist, check_ori=check_ori)
    return _same(OM.SearchByProjectionKF(v, **a), sr.search_by_projection_kf(g, **a), what)


def _m6(OM, v, g, matched, Q, sf, th, ratio, what):
    a = dict(matched_in=matched, scale_factors=sf, valid=Q["valid"], u=Q["x"], v=Q["y"], level=Q["level"], qdesc=Q["desc"], th=th, ratio_hamming=ratio)
    return _same(OM.SearchByProjectionSim3(v, **a), sr.search_by_projection_sim3(g, **a), what)


def _m13(OM, v, g, Q, sf, th, chi2, what):
    a = dict(scale_factors=sf, inv_sigma2=(F(1) / (sf * sf)).astype(np.float32), valid=Q["valid"], u=Q["x"], v=Q["y"], ur=Q["pxr"], level=Q["level"],
             qdesc=Q["desc"], th=th, chi2_gate=chi2)
    return _same(OM.Fuse(v, **a), sr.fuse(g, **a), what)


def threshold_lattice(oracle):
    """Candidates on and beside every threshold, the ratio rule's edges, claims, window edges and the stereo gate."""
    L = Lattice(oracle)
    S = dict(ur=25.0)
    L.add([(1, 0, 0, 100)]); L.add([(1, 0, 0, 101)])                                  # TH_HIGH, TH_HIGH + 1
    L.add([(1, 0, 0, 50)]); L.add([(1, 0, 0, 51)])                                    # TH_LOW, TH_LOW + 1
    L.add([(1, 0, 0, 64)]); L.add([(1, 0, 0, 65)]); L.add([(1, 0, 0, 75)]); L.add([(1, 0, 0, 76)])   # M5's orb_dist 64, M6's 50 * 1.5
    L.add([(1, 0, 0, 45), (0, 1, 0, 50)])                                            # 45 == 0.9f * 50 in float, > in double
    L.add([(1, 0, 0, 46), (0, 1, 0, 50)])                                            # the ratio rule rejects: the slot stays untouched
    L.add([(1, 0, 0, 46), (0, 1, 1, 50)], level=1)                                   # levels differ: the ratio rule is bypassed
    L.add([(1, 0, 0, 30), (0, 1, 0, 30), (-1, 0, 0, 30)])                            # a three-way tie: the first in visiting order wins
    a = L.add([(1, 0, 0, 20), (0, 1, 0, 40)], obs=False); L.add([], same_as=a)       # a query without observations is overwritten
    b = L.add([(1, 0, 0, 20), (0, 1, 0, 40)], obs=True); L.add([], same_as=b)        # one with observations blocks its slot
    L.add([(1, 0, 0, 10, dict(blocked=True)), (0, 1, 0, 12, dict(blocked=True))])    # a window of blocked candidates only
    L.add([(4, 0, 0, 10)]); L.add([(0, -4, 0, 10)]); L.add([(3.5, 3.5, 0, 10)])      # exactly r = 4 away (M3 at th 1): strict <
    L.add([(1, 0, 0, 10, dict(ur=60.0)), (0, 1, 0, 30, dict(ur=0.0)), (-1, 0, 0, 35, dict(ur=-1.0))], pxr=10.0)   # stereo gate only where uright > 0
    L.add([(1, 0, 0, 10, S)], pxr=25.5)
    L.add([(1, 0, 2, 10), (0, 1, 0, 20)], level=1)                                   # level bands
    L.add([(1, 0, 0, 10), (0, 1, 3, 20)], level=2)
    L.add([(2.5, 0, 0, 10)], pos=(-2.0, 100.0)); L.add([], pos=(-100.0, 100.0)); L.add([], pos=(500.0, 100.0)); L.add([], pos=(100.0, 400.0))
    L.add([(-2.0, -2.0, 0, 10)], pos=(374.0, 238.0))
    L.add([(1, 0, 0, 10)], valid=False)
    # a tie across two grid columns (x = 26.3 and 31 round into different columns at 376 and at 752 px width): the candidate with the
    # HIGHER index is visited first and wins; octaves 0 and 1 so that M3's ratio rule is bypassed
    L.add([(1, 0, 1, 30), (-3.7, 0, 0, 30)], level=1, pos=(30.0, 180.0))
    return L


def test_m3_constructed(pkg, oracle, OM):
    sf = _sf()
    L = threshold_lattice(oracle)
    v, g, blocked, Q = L.arrays(pkg, OM, stereo=True)
    t = _m3(OM, v, g, blocked, Q, sf, 1.0, 0.9, "M3 th 1")
    for key in ("dist_on_th_high", "dist_on_th_high_plus_1", "ratio_exactly_equal", "ratio_rejected", "ratio_bypassed_by_level", "accepted_same_level",
                "accepted_levels_differ", "overwrote_unobserved", "all_candidates_blocked", "exactly_r_away", "stereo_gate_applied", "stereo_gate_rejected",
                "stereo_gate_skipped", "empty_window", "window_outside_grid", "window_clipped", "levels_checked_min_negative", "tie_kept_first_not_lowest_index"):
        assert t[key] > 0, key
    n, m, _ = sr.search_by_projection_points(g, blocked, sf, Q["valid"], Q["x"], Q["y"], Q["pxr"], Q["view_cos"], Q["level"], Q["desc"], Q["obs"], 1.0, 0.9)
    assert n > int((m >= 0).sum())                                       # the overwritten claim was counted twice (:163)
    assert float(F(0.9) * F(50)) == 45.0 and float(F(0.9)) * 50 < 45.0   # why 45 against 50 separates the float from the double product
    assert m[L.q[8]["first"]] == 8 and m[L.q[9]["first"]] < 0 and m[L.q[10]["first"]] == 10 and m[L.q[11]["first"]] < 0   # M3 reads a tie as a failed ratio test
    vc = Q["view_cos"].copy(); vc[::2] = 0.9985                          # RadiusByViewingCos: 2.5 above the double 0.998
    Q2 = dict(Q, view_cos=vc)
    _m3(OM, v, g, blocked, Q2, sf, 1.0, 0.9, "M3 view cos")
    _m3(OM, v, g, blocked, Q, sf, 3.0, 0.8, "M3 th 3")


def test_m4_constructed(pkg, oracle, OM):
    sf = _sf()
    v, g, blocked, Q = threshold_lattice(oracle).arrays(pkg, OM, stereo=True)
    t = _m4(OM, v, g, blocked, Q, sf, 4.0, "M4 th 4", mbf=40.0, check_ori=False)          # ur = u - 40 * 0.1
    for key in ("dist_on_th_high", "dist_on_th_high_plus_1", "overwrote_unobserved", "all_candidates_blocked", "exactly_r_away", "stereo_gate_applied",
                "stereo_gate_rejected", "stereo_gate_skipped", "empty_window", "window_outside_grid", "tie_kept_first_not_lowest_index"):
        assert t[key] > 0, key
    t = _m4(OM, v, g, blocked, Q, sf, 4.0, "M4 forward", forward=True, mbf=40.0, check_ori=False)
    assert t["forward_band"] > 0 and t["levels_unchecked_min0"] > 0
    t = _m4(OM, v, g, blocked, Q, sf, 4.0, "M4 backward", backward=True, mbf=40.0, check_ori=False)
    assert t["backward_band"] > 0


def rotation_lattice(oracle, bins, twice=True):
    """One accepted match per query; `bins` = [(rotation in degrees, how many queries)]."""
    L = Lattice(oracle)
    for rot, count in bins:
        for _ in range(count):
            L.add([(1, 0, 0, 10, dict(angle=10.0))], angle=(10.0 + rot) % 360.0)
    if twice:                          # a slot assigned twice: first by a query without observations whose bin is culled
        a = L.add([(1, 0, 0, 10, dict(angle=10.0))], angle=10.0 + 200.0, obs=False)
        L.add([], same_as=a, angle=10.0 + bins[0][0])
        b = L.add([(1, 0, 0, 10, dict(angle=10.0))], angle=10.0 + 250.0, obs=False)   # and one whose two bins are both culled
        L.add([], same_as=b, angle=10.0 + 300.0)
    return L


@pytest.mark.parametrize("bins,kept", [([(0.0, 20), (90.0, 1), (6.0, 1), (30.0, 1), (349.99, 1)], 1),
                                        ([(42.0, 20), (90.0, 5), (6.0, 1), (30.0, 1)], 2),
                                        ([(42.0, 20), (90.0, 5), (6.0, 3), (30.0, 2), (359.0, 2)], 3)])
def test_rotation_check_constructed(pkg, oracle, OM, bins, kept):
    sf = _sf()
    v, g, blocked, Q = rotation_lattice(oracle, bins).arrays(pkg, OM)
    t = _m4(OM, v, g, blocked, Q, sf, 7.0, "M4 rotation", check_ori=True)
    assert t["bins_kept"] == kept and t["culled_entries"] > 0 and t["half_way_bin"] > 0
    assert t["slots_in_histogram_twice"] == 2 and t["twice_in_histogram_and_culled"] == 2      # one cleared although its later bin is kept
    assert t["slot_culled_twice"] == 1                                                        # the other decrements the count twice
    if kept == 3:
        assert t["bin_30_wraps"] > 0
    v, g, blocked, Q = rotation_lattice(oracle, bins, twice=False).arrays(pkg, OM)
    t = _m5(OM, v, g, blocked, Q, sf, 3.0, 100, True, "M5 rotation")
    assert t["bins_kept"] == kept and t["culled_entries"] > 0 and t["half_way_bin"] > 0
    assert float(F(6.0) * sr.FACTOR_360) == 0.5 and float(F(30.0) * sr.FACTOR_360) == 2.5       # the half-way products are exact


def test_m5_m6_m13_constructed(pkg, oracle, OM):
    sf = _sf()
    L = threshold_lattice(oracle)
    v, g, blocked, Q = L.arrays(pkg, OM, stereo=True)
    t = _m5(OM, v, g, blocked, Q, sf, 4.0, 64, False, "M5 orb_dist 64")
    assert t["dist_on_orb_dist"] > 0 and t["dist_on_orb_dist_plus_1"] > 0 and t["all_candidates_blocked"] > 0 and t["claims"] > 0 and t["exactly_r_away"] > 0
    assert t["tie_kept_first_not_lowest_index"] > 0
    n, m, _ = sr.search_by_projection_kf(g, blocked, sf, Q["valid"], Q["x"], Q["y"], Q["level"], Q["angle"], Q["desc"], 4.0, 64, False)
    assert n == int((m >= 0).sum())                                      # every claim blocks: the second query of a pair finds nothing
    _m5(OM, v, g, blocked, Q, sf, 4.0, 100, False, "M5 orb_dist 100")
    for ratio, on in ((1.0, 50), (1.5, 75)):
        t = _m6(OM, v, g, blocked, Q, sf, 4, ratio, "M6 ratio %g" % ratio)
        assert t["dist_on_bound"] > 0 and t["dist_just_above_bound"] > 0 and t["all_candidates_blocked"] > 0 and t["claims"] > 0 and t["level_rejected"] > 0
        assert t["tie_kept_first_not_lowest_index"] > 0
        n, m, _ = sr.search_by_projection_sim3(g, blocked, sf, Q["valid"], Q["x"], Q["y"], Q["level"], Q["desc"], 4, ratio)
        assert n == int((m >= 0).sum()) and m[L.q[{50: 2, 75: 6}[on]]["first"]] >= 0 and m[L.q[{50: 3, 75: 7}[on]]["first"]] < 0
    assert float(F(50) * F(1.5)) == 75.0
    for chi2 in (True, False):
        t = _m13(OM, v, g, Q, sf, 4.0, chi2, "M13 chi2 %d" % chi2)
        assert t["dist_on_th_low"] > 0 and t["dist_on_th_low_plus_1"] > 0 and t["tie_kept_first"] > 0 and t["level_rejected"] > 0
        if not chi2:                                                     # (the chi2 test drops the tie's far candidate)
            assert t["tie_kept_first_not_lowest_index"] > 0
        if chi2:
            assert t["chi2_stereo"] > 0 and t["chi2_mono"] > 0 and t["chi2_rejected"] > 0


# ---- BoW searches: constructed buckets --------------------------------------------------------------------------------------
def bow_case(oracle, seed=9):
    """Side 1 features with a bucket each (node = case number); side 2 rows are the listed distances away from them."""
    rng = np.random.default_rng(seed)
    cases = [[50], [51], [49], [20, 20], [20, 40], [21, 35], [30, 30, 45], [12, 40], [256]]
    k1, d1, n1, k2, d2, n2 = [], [], [], [], [], []
    for node, dists in enumerate(cases):
        q = rng.integers(0, 256, 32, dtype=np.uint8)
        k1.append(float(node)); d1.append(q); n1.append(node)
        for d in dists:
            bits = np.unpackbits(q); bits[:d] ^= 1
            k2.append(0.0); d2.append(np.packbits(bits)); n2.append(node)
    node = len(cases)                                         # two side-1 features whose nearest side-2 row is the same one
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    for _ in range(2):
        k1.append(0.0); d1.append(q.copy()); n1.append(node)
    for d in (5, 25):
        bits = np.unpackbits(q); bits[:d] ^= 1
        k2.append(0.0); d2.append(np.packbits(bits)); n2.append(node)
    n1 += [40, 41]; d1 += [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2)]; k1 += [0.0, 0.0]      # nodes only one side has
    n2 += [39, 43]; d2 += [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2)]; k2 += [0.0, 0.0]
    K1 = np.zeros(len(k1), oracle.KP_DTYPE); K2 = np.zeros(len(k2), oracle.KP_DTYPE)
    K1["x"] = 20 + 10 * np.arange(len(k1)); K1["y"] = 50; K2["x"] = 20 + 5 * np.arange(len(k2)); K2["y"] = 50
    return K1, np.array(d1, np.uint8), np.array(n1), K2, np.array(d2, np.uint8), np.array(n2)


def test_m7_m8_constructed(pkg, oracle, OM):
    K1, D1, N1, K2, D2, N2 = bow_case(oracle)
    fv1, fv2 = _fv(pkg, N1), _fv(pkg, N2)
    good1 = np.ones(len(K1), np.uint8); good2 = np.ones(len(K2), np.uint8)
    a7 = dict(kkf=K1, dkf=D1, kf_good=good1, fvk=fv1, kf_=K2, df=D2, fvf=fv2, nnratio=0.6, check_ori=False)
    got = OM.SearchByBoW(**a7)
    n, m, t = sr.search_by_bow(K1, D1, good1, fv1, K2, D2, fv2, 0.6, False)
    _same(got, (n, m, t), "M7")
    for key in ("dist_on_th_low", "accepted_on_th_low", "dist_on_th_low_plus_1", "runner_up_equals_best", "ratio_rejected"):
        assert t[key] > 0, key
    assert float(F(0.6) * F(35)) == 21.0 and float(F(0.6)) * 35 > 21.0   # 21 against 35 at 0.6f: rejected on the float product only
    k2_of = lambda node: int(np.nonzero(N2 == node)[0][0])
    assert m[k2_of(0)] == 0 and m[k2_of(1)] < 0 and m[k2_of(3)] < 0 and m[k2_of(4)] == 4 and m[k2_of(5)] < 0
    got = OM.SearchByBoWKF(k1=K1, d1=D1, good1=good1, fv1=fv1, k2=K2, d2=D2, good2=good2, fv2=fv2, nnratio=0.6, check_ori=False)
    n, m, t = sr.search_by_bow_kf(K1, D1, good1, fv1, K2, D2, good2, fv2, 0.6, False)
    _same(got, (n, m, t), "M8")
    for key in ("rejected_on_th_low", "dist_on_th_low_plus_1", "runner_up_equals_best", "ratio_rejected", "skipped_claimed_side2"):
        assert t[key] > 0, key
    assert m[0] < 0 and m[2] == k2_of(2) and m[4] == k2_of(4)            # M8 is strict at TH_LOW, 49 passes
    good2[k2_of(4)] = 0; good1[7] = 0
    got = OM.SearchByBoWKF(k1=K1, d1=D1, good1=good1, fv1=fv1, k2=K2, d2=D2, good2=good2, fv2=fv2, nnratio=0.9, check_ori=True)
    _same(got, sr.search_by_bow_kf(K1, D1, good1, fv1, K2, D2, good2, fv2, 0.9, True), "M8 good flags")


M10_F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)       # the epipolar line of (x1, y1) is y2 = y1: dsqr = (y2 - y1)^2
M10_F12_ROW = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0]], np.float32)    # a = 0, b = 1, c = 0: dsqr = y2 * y2 whatever feature 1 is
M10_Y_ON_BOUND = F(1.9595917463302612)                                   # y * y == 3.84f in float32: below 3.84 * 1.0 (double), not below 3.84f * 1.0f
M10_EP = (300.0, 105.0)


def m10_case(oracle):
    """The hand-built M10 pair: one node per case.  Returns K1, D1, N1, U1, K2, D2, N2, U2."""
    rng = np.random.default_rng(10)
    k1, d1, n1, u1, k2, d2, n2, u2 = [], [], [], [], [], [], [], []

    def add(node, y1, ur1, cands, angle1=0.0, q=None):
        q = rng.integers(0, 256, 32, dtype=np.uint8) if q is None else q
        k1.append((100.0, y1, angle1, 0)); d1.append(q); n1.append(node); u1.append(ur1)
        for x2, y2, octv, dist, ur2 in cands:
            bits = np.unpackbits(q); bits[:dist] ^= 1
            k2.append((x2, y2, 0.0, octv)); d2.append(np.packbits(bits)); n2.append(node); u2.append(ur2)
        return q
    add(0, 50.0, -1.0, [(150.0, 50.5, 0, 20, -1.0), (160.0, 50.5, 0, 20, -1.0), (170.0, 50.5, 0, 20, -1.0)])   # a tie: the last one wins
    add(1, 60.0, -1.0, [(150.0, 62.0, 0, 10, -1.0), (160.0, 61.9, 0, 30, -1.0)])                              # dsqr 4.0 fails, 3.61 < 3.84 passes
    add(2, 70.0, -1.0, [(150.0, 72.3, 1, 10, -1.0)])                                                          # 5.29 < 3.84 * 1.44
    add(3, 80.0, -1.0, [(150.0, 80.0, 0, 50, -1.0)]); add(4, 90.0, -1.0, [(150.0, 90.0, 0, 51, -1.0)])        # TH_LOW is inclusive here
    add(5, 100.0, -1.0, [(302.0, 100.0, 0, 10, -1.0), (309.5, 100.0, 0, 30, 4.0)])                            # within 10 px of the epipole
    add(6, 110.0, 3.0, [(303.0, 110.0, 0, 10, -1.0)])                                                         # feature 1 is stereo: no epipole gate
    add(7, 120.5, -1.0, [], q=add(7, 120.0, -1.0, [(150.0, 120.0, 0, 10, 0.0)]))                                # two idx1 share one idx2
    add(8, 130.0, -1.0, [(150.0, float(M10_Y_ON_BOUND), 0, 10, -1.0)])                                        # under M10_F12_ROW: dsqr == 3.84f
    K1 = np.zeros(len(k1), oracle.KP_DTYPE); K2 = np.zeros(len(k2), oracle.KP_DTYPE)
    for K, rows in ((K1, k1), (K2, k2)):
        a = np.array(rows, np.float64)
        K["x"], K["y"], K["angle"], K["octave"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3].astype(np.int32)
    return K1, np.array(d1, np.uint8), np.array(n1), np.array(u1, np.float32), K2, np.array(d2, np.uint8), np.array(n2), np.array(u2, np.float32)


def test_m10_constructed(pkg, oracle, OM):
    sf = _sf(); sigma2 = (sf * sf).astype(np.float32)
    F12 = M10_F12
    K1, D1, n1, U1, K2, D2, n2, U2 = m10_case(oracle)
    fv1, fv2 = _fv(pkg, n1), _fv(pkg, n2)
    z1, z2 = np.zeros(len(K1), np.uint8), np.zeros(len(K2), np.uint8)

    def both(F, only_stereo=False, coarse=False, ori=False, what=""):
        a = dict(k1=K1, d1=D1, has_mp1=z1, ur1=U1, fv1=fv1, k2=K2, d2=D2, has_mp2=z2, ur2=U2, fv2=fv2, F12=F, ep=M10_EP, sf2=sf, sigma2_2=sigma2,
                 only_stereo=only_stereo, coarse=coarse, check_ori=ori)
        want = sr.search_for_triangulation(K1, D1, z1, U1, fv1, K2, D2, z2, U2, fv2, F, M10_EP, sf, sigma2, only_stereo, coarse, ori)
        return _same(OM.SearchForTriangulation(**a), want, "M10 " + what), want[1]
    t, m = both(F12, what="plain")
    for key in ("tie_goes_to_later", "epipolar_pass", "epipolar_fail", "dist_on_th_low", "epipole_gate_applied", "epipole_gate_rejected",
                "epipole_gate_skipped_stereo", "idx2_shared"):
        assert t[key] > 0, key
    assert m[0] == 2 and m[1] == 4 and m[3] >= 0 and m[4] < 0 and m[5] == int(np.nonzero(np.array(n2) == 5)[0][1]) and m[7] == m[8] >= 0
    t, _ = both(np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], np.float32), what="den == 0")
    assert t["den_zero"] > 0 and t["epipolar_pass"] == 0
    t, _ = both(np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], np.float32), coarse=True, what="coarse")
    assert t["den_zero"] > 0 and t["coarse_accepted"] > 0
    t, m = both(M10_F12_ROW, what="dsqr on the bound")
    on_bound = int(np.nonzero(n2 == 8)[0][0])
    assert t["double_product_decides"] > 0 and m[9] == on_bound and K2["y"][on_bound] == M10_Y_ON_BOUND
    assert M10_Y_ON_BOUND * M10_Y_ON_BOUND == F(3.84) and float(F(3.84)) < 3.84 and not F(3.84) < F(3.84) * sigma2[0]
    t, _ = both(F12, only_stereo=True, what="only_stereo")
    assert t["only_stereo_skipped"] > 0
    both(F12, ori=True, what="orientation")


M10_ROTATIONS = ([0.0, 10.0, 40.0, 100.0, 200.0], [0.5, 0.2, 0.12, 0.1, 0.08])


def test_m10_rotation_factor(pkg, oracle, OM, scene, monkeypatch):
    """M10 bins with 1.0f/30 where the other searches use 30/360.0f: a frame against itself, its angles turned by 0 / 10 / 40 / 100 /
    200 degrees in falling shares.  At 1/30 these fall into bins 0, 0, 1, 3, 7: bins 0, 1 and 3 stay and only the 200 degree group is
    culled.  At 30/360 they fall into bins 0, 1, 3, 8, 17: the 100 degree group is culled too.  So the two factors give different rows."""
    rng = np.random.default_rng(12)
    k, d = scene["kr"], scene["dr"]
    k2 = k.copy(); k2["angle"] = (k["angle"] + rng.choice(M10_ROTATIONS[0], len(k), p=M10_ROTATIONS[1])) % 360.0
    fv = _fv_desc(pkg, d, 3)
    z = np.zeros(len(k), np.uint8)
    a = dict(k1=k2, d1=d, has_mp1=z, ur1=None, fv1=fv, k2=k, d2=d, has_mp2=z, ur2=None, fv2=fv, F12=np.eye(3, dtype=np.float32), ep=(5000.0, 240.0),
             sf2=scene["sf"], sigma2_2=scene["sigma2"], only_stereo=False, coarse=True, check_ori=True)
    want = sr.search_for_triangulation(k2, d, z, None, fv, k, d, z, None, fv, np.eye(3, dtype=np.float32), (5000.0, 240.0), scene["sf"], scene["sigma2"], False, True, True)
    t = _same(OM.SearchForTriangulation(**a), want, "M10 1/30")
    assert want[0] > 100 and t["culled_entries"] > 0
    monkeypatch.setattr(sr, "FACTOR_INV", sr.FACTOR_360)              # what a reading with the other searches' factor would give
    other = sr.search_for_triangulation(k2, d, z, None, fv, k, d, z, None, fv, np.eye(3, dtype=np.float32), (5000.0, 240.0), scene["sf"], scene["sigma2"], False, True, True)
    assert other[0] < want[0] and not np.array_equal(other[1], want[1])


# ---- extractor scenes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.0, 0.35, 0.97])
def test_projection_searches_on_scenes(pkg, OM, scene, frac):
    rng = np.random.default_rng(int(frac * 100) + 1)
    W, H, kl, dl, kr, dr, sf = scene["W"], scene["H"], scene["kl"], scene["dl"], scene["kr"], scene["dr"], scene["sf"]
    ur = np.where(rng.random(len(kr)) < 0.6, kr["x"] - rng.uniform(2, 40, len(kr)), -1).astype(np.float32)
    ur[::17] = 0.0
    v, g = _view(pkg, OM, kr, dr, W, H, ur)
    shift = 0.0 if scene["name"] == "large" else 12.0
    n, qu, qv = _queries(kl, rng, shift)
    blocked = (rng.random(len(kr)) < frac).astype(np.uint8)
    obs = (rng.random(n) < 0.7).astype(np.uint8)
    lvl = np.clip(kl["octave"] + rng.integers(-1, 2, n), 0, 7).astype(np.int32)
    ang = ((kl["angle"] + rng.choice([0.0, 0.0, 0.0, 0.0, 40.0, 100.0, 200.0, 300.0], n)) % 360.0).astype(np.float32)
    Q = dict(x=qu, y=qv, level=kl["octave"].astype(np.int32), angle=ang, obs=obs, valid=(rng.random(n) < 0.85).astype(np.uint8),
             pxr=(qu - rng.uniform(2, 40, n)).astype(np.float32), view_cos=rng.uniform(0.99, 1.0, n).astype(np.float32),
             invzc=rng.uniform(0.05, 1.0, n).astype(np.float32), desc=dl)
    t = _m3(OM, v, g, blocked, Q, sf, 3.0, 0.8, "M3")
    t4 = _m4(OM, v, g, blocked, Q, sf, 7.0, "M4", mbf=47.9, check_ori=True)
    _m4(OM, v, g, blocked, Q, sf, 7.0, "M4 forward", forward=True, mbf=47.9, check_ori=True)
    _m4(OM, v, g, blocked, Q, sf, 15.0, "M4 backward", backward=True, mbf=47.9, check_ori=False)
    Ql = dict(Q, level=lvl)
    t5 = _m5(OM, v, g, blocked, Ql, sf, 10.0, 100, True, "M5")
    t6 = _m6(OM, v, g, blocked, Ql, sf, 8, 1.5, "M6 1.5")
    _m6(OM, v, g, blocked, Ql, sf, 5, 1.0, "M6 1.0")
    _m13(OM, v, g, Ql, sf, 3.0, True, "M13 chi2"); _m13(OM, v, g, Ql, sf, 3.0, False, "M13")
    if frac > 0.9:
        assert min(t["all_candidates_blocked"], t4["all_candidates_blocked"], t5["all_candidates_blocked"], t6["all_candidates_blocked"]) > 0
    if frac == 0.0:
        assert t4["culled_entries"] > 0 and t5["culled_entries"] > 0 and t["overwrote_unobserved"] + t4["overwrote_unobserved"] > 0
    a = dict(scale_factors=sf, valid=Q["valid"], u=Q["x"], v=Q["y"], invzc=Q["invzc"], octave=Q["level"], angle=Q["angle"], qdesc=Q["desc"], mp_obs=Q["obs"])
    n1, m1, _, retried = sr.search_by_projection_frame_with_retry(g, blocked, th=7.0, mbf=47.9, retry_below=10 ** 6, **a)   # the 2 * th retry, from an empty frame
    assert retried
    _same(OM.SearchByProjectionFrame(v, cur_blocked=np.zeros(len(kr), np.uint8), th=14.0, mbf=47.9, **a), (n1, m1, None), "M4 retry")


@pytest.mark.parametrize("bits,ori,nnratio", [(4, True, 0.7), (2, True, 0.9), (6, False, 0.75)])
def test_bow_searches_on_scenes(pkg, OM, scene, bits, ori, nnratio):
    rng = np.random.default_rng(bits)
    kl, dl, kr, dr = scene["kl"], scene["dl"], scene["kr"], scene["dr"]
    if scene["name"] == "large":                              # duplicated descriptor rows: ties inside a bucket
        dr = dr.copy(); dr[1::9] = dr[0:-1:9][:len(dr[1::9])]
    fvl, fvr = _fv_desc(pkg, dl, bits), _fv_desc(pkg, dr, bits)
    g1 = (rng.random(len(kl)) < 0.8).astype(np.uint8); g2 = (rng.random(len(kr)) < 0.8).astype(np.uint8)
    got = OM.SearchByBoW(kkf=kl, dkf=dl, kf_good=g1, fvk=fvl, kf_=kr, df=dr, fvf=fvr, nnratio=nnratio, check_ori=ori)
    want = sr.search_by_bow(kl, dl, g1, fvl, kr, dr, fvr, nnratio, ori)
    t = _same(got, want, "M7"); assert want[0] > 0 and (not ori or t["culled_entries"] > 0 or bits == 2)
    got = OM.SearchByBoWKF(k1=kl, d1=dl, good1=g1, fv1=fvl, k2=kr, d2=dr, good2=g2, fv2=fvr, nnratio=nnratio, check_ori=ori)
    want = sr.search_by_bow_kf(kl, dl, g1, fvl, kr, dr, g2, fvr, nnratio, ori)
    _same(got, want, "M8"); assert want[0] > 0
    F12 = np.array([[1e-7, -3e-6, 1.1e-3], [2.5e-6, 2e-7, -0.0231], [-1.3e-3, 0.0229, 0.35]], np.float32)
    u1 = np.where(rng.random(len(kl)) < 0.5, 5.0, -1.0).astype(np.float32); u2 = np.where(rng.random(len(kr)) < 0.5, 5.0, -1.0).astype(np.float32)
    mp1 = (rng.random(len(kl)) < 0.3).astype(np.uint8); mp2 = (rng.random(len(kr)) < 0.3).astype(np.uint8)
    for coarse, only in ((False, False), (True, False), (False, True)):
        a = dict(k1=kl, d1=dl, has_mp1=mp1, ur1=u1, fv1=fvl, k2=kr, d2=dr, has_mp2=mp2, ur2=u2, fv2=fvr, F12=F12, ep=(scene["W"] * 0.6, scene["H"] * 0.5),
                 sf2=scene["sf"], sigma2_2=scene["sigma2"], only_stereo=only, coarse=coarse, check_ori=ori)
        want = sr.search_for_triangulation(kl, dl, mp1, u1, fvl, kr, dr, mp2, u2, fvr, F12, (scene["W"] * 0.6, scene["H"] * 0.5), scene["sf"], scene["sigma2"], only, coarse, ori)
        t = _same(OM.SearchForTriangulation(**a), want, "M10 coarse %d only_stereo %d" % (coarse, only))
        if coarse:
            assert want[0] > 0 and t["epipole_gate_applied"] > 0 and t["epipole_gate_skipped_stereo"] > 0
