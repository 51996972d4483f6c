"""The product's single-frame host entry points (csrc/orbm_api.hip: device distance pass + host replay) against tests/second_reading.py
on the constructed scenes of the CPU tests, which prove from the second reading's trace that each branch is reached.  The helpers of
those tests take a backend; here it is a pkg.ORBmatcher where they pass the oracle.  Also the two resident forms, on the threshold
lattice and on a crowded cluster that makes the top-8 keys run dry so that the fallback to full candidate lists runs.

The second reading has no form of the legacy SearchForTriangulation overload (vbMatched2 kept, 30/360 bins): that one is held to the
oracle's, on the same constructed pair."""
import numpy as np
import pytest

import bow_fisheye_cases as bc
import fisheye_cases as fc
import points_fisheye_cases as pc
import second_reading as sr
import second_reading_bow_fisheye as srb
import test_second_reading_cpu as c
import test_second_reading_fisheye_cpu as f4
import test_second_reading_init_cpu as c9
import test_second_reading_points_fisheye_cpu as f3

pytestmark = pytest.mark.gpu

HAND_M3_FISHEYE = [n for n in pc.HAND_NAMES if n != "partner_out_of_range"]   # (not defined for a host form: it would write past its row)


@pytest.fixture(scope="module")
def M(pkg):
    return pkg.ORBmatcher(0.6, device=0)


@pytest.fixture(scope="module")
def OM(oracle):
    return oracle._oracle_matcher_class()()


def _a3(blocked, Q, sf, th, nnratio):
    return dict(blocked=blocked, scale_factors=sf, in_view=Q["valid"], px=Q["x"], py=Q["y"], pxr=Q["pxr"], view_cos=Q["view_cos"], level=Q["level"],
                qdesc=Q["desc"], mp_obs=Q["obs"], th=th, nnratio=nnratio)


def _a4(blocked, Q, sf, th, **kw):
    return dict(cur_blocked=blocked, scale_factors=sf, valid=Q["valid"], u=Q["x"], v=Q["y"], invzc=Q["invzc"], octave=Q["level"], angle=Q["angle"],
                qdesc=Q["desc"], mp_obs=Q["obs"], th=th, **kw)


def _m3_resident(M, rf, g, blocked, Q, sf, th, nnratio, what):
    a = _a3(blocked, Q, sf, th, nnratio)
    return c._same(M.SearchByProjectionPointsResident(rf, **a), sr.search_by_projection_points(g, **a), what)


def _m4_resident(M, rf, g, blocked, Q, sf, th, what, **kw):
    a = _a4(blocked, Q, sf, th, **kw)
    return c._same(M.SearchByProjectionFrameResident(rf, **a), sr.search_by_projection_frame(g, **a), what)


# ---- threshold_lattice ------------------------------------------------------------------------------------------------------
def test_m3_lattice(pkg, oracle, M):
    sf = c._sf()
    v, g, blocked, Q = c.threshold_lattice(oracle).arrays(pkg, M, stereo=True)
    rf = pkg.ResidentFrame(M, view=v)
    vc = Q["view_cos"].copy(); vc[::2] = 0.9985
    for q, th, nnratio, what in ((Q, 1.0, 0.9, "M3 th 1"), (dict(Q, view_cos=vc), 1.0, 0.9, "M3 view cos"), (Q, 3.0, 0.8, "M3 th 3")):
        t = c._m3(M, v, g, blocked, q, sf, th, nnratio, what)
        _m3_resident(M, rf, g, blocked, q, sf, th, nnratio, what + " resident")
    assert t["accepted_same_level"] > 0 and t["all_candidates_blocked"] > 0


def test_m4_lattice(pkg, oracle, M):
    sf = c._sf()
    v, g, blocked, Q = c.threshold_lattice(oracle).arrays(pkg, M, stereo=True)
    rf = pkg.ResidentFrame(M, view=v)
    for what, kw in (("M4 th 4", {}), ("M4 forward", dict(forward=True)), ("M4 backward", dict(backward=True))):
        t = c._m4(M, v, g, blocked, Q, sf, 4.0, what, mbf=40.0, check_ori=False, **kw)
        _m4_resident(M, rf, g, blocked, Q, sf, 4.0, what + " resident", mbf=40.0, check_ori=False, **kw)
    assert t["backward_band"] > 0


def test_m5_m6_m13_lattice(pkg, oracle, M):
    sf = c._sf()
    v, g, blocked, Q = c.threshold_lattice(oracle).arrays(pkg, M, stereo=True)
    for orb_dist in (64, 100):
        t = c._m5(M, v, g, blocked, Q, sf, 4.0, orb_dist, False, "M5 orb_dist %d" % orb_dist)
        assert t["claims"] > 0
    for ratio in (1.0, 1.5):
        t = c._m6(M, v, g, blocked, Q, sf, 4, ratio, "M6 ratio %g" % ratio)
        assert t["dist_on_bound"] > 0 and t["dist_just_above_bound"] > 0
    for chi2 in (True, False):
        t = c._m13(M, v, g, Q, sf, 4.0, chi2, "M13 chi2 %d" % chi2)
        assert t["dist_on_th_low"] > 0 and (not chi2 or t["chi2_rejected"] > 0)


# ---- rotation_lattice -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,kept", [([(0.0, 20), (90.0, 1), (6.0, 1), (30.0, 1), (349.99, 1)], 1),
                                        ([(42.0, 20), (90.0, 5), (6.0, 1), (30.0, 1)], 2),
                                        ([(42.0, 20), (90.0, 5), (6.0, 3), (30.0, 2), (359.0, 2)], 3)])
def test_rotation_lattice(pkg, oracle, M, bins, kept):
    sf = c._sf()
    v, g, blocked, Q = c.rotation_lattice(oracle, bins).arrays(pkg, M)
    t = c._m4(M, v, g, blocked, Q, sf, 7.0, "M4 rotation", check_ori=True)
    _m4_resident(M, pkg.ResidentFrame(M, view=v), g, blocked, Q, sf, 7.0, "M4 rotation resident", check_ori=True)
    assert t["bins_kept"] == kept and t["culled_entries"] > 0 and t["slots_in_histogram_twice"] == 2 and t["slot_culled_twice"] == 1
    v, g, blocked, Q = c.rotation_lattice(oracle, bins, twice=False).arrays(pkg, M)
    t = c._m5(M, v, g, blocked, Q, sf, 3.0, 100, True, "M5 rotation")
    assert t["bins_kept"] == kept and t["culled_entries"] > 0


# ---- bow_case, m10_case -----------------------------------------------------------------------------------------------------
def test_m7_m8_bow_case(pkg, oracle, M):
    K1, D1, N1, K2, D2, N2 = c.bow_case(oracle)
    fv1, fv2 = c._fv(pkg, N1), c._fv(pkg, N2)
    good1 = np.ones(len(K1), np.uint8); good2 = np.ones(len(K2), np.uint8)
    for ori in (False, True):
        got = M.SearchByBoW(kkf=K1, dkf=D1, kf_good=good1, fvk=fv1, kf_=K2, df=D2, fvf=fv2, nnratio=0.6, check_ori=ori)
        t = c._same(got, sr.search_by_bow(K1, D1, good1, fv1, K2, D2, fv2, 0.6, ori), "M7 ori %d" % ori)
        assert t["accepted_on_th_low"] > 0 and t["ratio_rejected"] > 0
        got = M.SearchByBoWKF(k1=K1, d1=D1, good1=good1, fv1=fv1, k2=K2, d2=D2, good2=good2, fv2=fv2, nnratio=0.6, check_ori=ori)
        t = c._same(got, sr.search_by_bow_kf(K1, D1, good1, fv1, K2, D2, good2, fv2, 0.6, ori), "M8 ori %d" % ori)
        assert t["rejected_on_th_low"] > 0 and t["skipped_claimed_side2"] > 0
    good2[int(np.nonzero(N2 == 4)[0][0])] = 0; good1[7] = 0
    got = M.SearchByBoWKF(k1=K1, d1=D1, good1=good1, fv1=fv1, k2=K2, d2=D2, good2=good2, fv2=fv2, nnratio=0.9, check_ori=True)
    c._same(got, sr.search_by_bow_kf(K1, D1, good1, fv1, K2, D2, good2, fv2, 0.9, True), "M8 good flags")


M10_VARIANTS = [("plain", c.M10_F12, {}), ("den == 0", np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], np.float32), {}),
                ("coarse", np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], np.float32), dict(coarse=True)), ("dsqr on the bound", c.M10_F12_ROW, {}),
                ("only_stereo", c.M10_F12, dict(only_stereo=True)), ("orientation", c.M10_F12, dict(check_ori=True))]


@pytest.mark.parametrize("what,F12,kw", M10_VARIANTS, ids=[v[0] for v in M10_VARIANTS])
def test_m10_case(pkg, oracle, M, OM, what, F12, kw):
    sf = c._sf(); sigma2 = (sf * sf).astype(np.float32)
    K1, D1, n1, U1, K2, D2, n2, U2 = c.m10_case(oracle)
    fv1, fv2 = c._fv(pkg, n1), c._fv(pkg, n2)
    z1, z2 = np.zeros(len(K1), np.uint8), np.zeros(len(K2), np.uint8)
    kw = dict(dict(only_stereo=False, coarse=False, check_ori=False), **kw)
    a = dict(k1=K1, d1=D1, has_mp1=z1, ur1=U1, fv1=fv1, k2=K2, d2=D2, has_mp2=z2, ur2=U2, fv2=fv2, F12=F12, ep=c.M10_EP, sf2=sf, sigma2_2=sigma2, **kw)
    want = sr.search_for_triangulation(K1, D1, z1, U1, fv1, K2, D2, z2, U2, fv2, F12, c.M10_EP, sf, sigma2, kw["only_stereo"], kw["coarse"], kw["check_ori"])
    t = c._same(M.SearchForTriangulation(**a), want, "M10 " + what)
    if what == "plain":
        assert t["tie_goes_to_later"] > 0 and t["idx2_shared"] > 0 and t["epipole_gate_rejected"] > 0
    if what == "dsqr on the bound":
        assert t["double_product_decides"] > 0
    n, m = M.SearchForTriangulation(legacy=True, **a)
    n_o, m_o = OM.SearchForTriangulation(legacy=True, **a)
    assert n == n_o and np.array_equal(m, m_o), ("M10 legacy " + what, n, n_o, np.flatnonzero(m != m_o)[:8])
    if what == "plain":
        assert n == want[0] - 1 and (m >= 0).sum() == n                  # vbMatched2: the shared idx2 is claimed once


# ---- M9: the constructed pairs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(c9.CASES))
def test_m9_constructed_pair(pkg, M, name):
    pair, _ = c9.CASES[name]
    k1, d1, k2, d2, prev = pair.arrays()
    c9._both(pkg, M, k1, d1, k2, d2, prev, pair.window, pair.nnratio, pair.check_ori)


# ---- the three fisheye forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", f4.NAMES)
def test_m4_fisheye_cases(pkg, oracle, synth, M, name):
    P = fc.pool(oracle, synth); case = fc.cases(oracle, synth)[name]
    for p in range(fc.NPAIRS):
        n, ml, mr = f4.single_pair(pkg, M, P, case, p)
        n2, ml2, mr2, _, _ = f4.second_reading_pair(P, case, p)
        assert n == n2, (name, p, n, n2)
        assert np.array_equal(ml, ml2) and np.array_equal(mr, mr2), (name, p, np.flatnonzero(ml != ml2)[:8], np.flatnonzero(mr != mr2)[:8])


@pytest.mark.parametrize("name", HAND_M3_FISHEYE)
def test_m3_fisheye_hand_cases(pkg, oracle, synth, M, name):
    case = pc.cases(oracle, synth)[name]; P = pc.hand_pool()
    assert case.pool_name == "hand" and case.host_defined
    for p in range(pc.NPAIRS):
        n, ml, mr = f3.single_pair(pkg, M, P, case, p)
        n2, ml2, mr2, t = f3.second_reading_pair(P, case, p)
        assert n == n2, (name, p, n, n2)
        assert np.array_equal(ml, ml2) and np.array_equal(mr, mr2), (name, p, np.flatnonzero(ml != ml2)[:8], np.flatnonzero(mr != mr2)[:8])
        if case.rule is not None and p == case.rule_pair:
            assert t[case.rule] >= 1, (name, case.rule, dict(t))


@pytest.mark.parametrize("nnratio,check_ori,weights", bc.HAND_PARAMS)
def test_m7_fisheye_hand_pairs(M, nnratio, check_ori, weights):
    b = bc.hand(nnratio, check_ori, weights)
    ran = 0
    for p in range(b.npairs):
        a = bc.single_args(b, p)
        if a is None:
            continue
        n, fm, _ = srb.search_by_bow_fisheye(*a)
        n2, fm2 = M.SearchByBoWFisheye(*a)
        assert n == n2 and np.array_equal(fm, fm2), (b.names[p], n, n2, np.flatnonzero(fm != fm2)[:8])
        ran += 1
    assert ran >= 20


# ---- a crowded cluster: the resident forms' fallback from the top-8 keys to full lists ---------------------------------------
CROWD = [(dx, -1) for dx in range(-3, 3)] + [(dx, 1) for dx in range(-3, 2)]   # eleven candidates around a query
CROWD_BLOCKED = (8, 7, 9, 0)                                                    # how many of the nearest are blocked, per cluster


def crowded_lattice(oracle):
    """Four clusters of eleven candidates at distances 10 + k, the first 8 / 7 / 9 / 0 of them blocked, one query each at level 1 and a
    fifth query on the unblocked cluster.  A resident search sees the 8 smallest (distance, visiting order) keys of a window: where
    they hold no unblocked candidate (M4), or fewer than two (M3), its replay cannot decide and the full lists are fetched."""
    L = c.Lattice(oracle)
    for nb in CROWD_BLOCKED:
        last = L.add([(dx, dy, k % 2, 10 + k, dict(blocked=k < nb)) for k, (dx, dy) in enumerate(CROWD)], level=1)
    L.add([], same_as=last, level=1)
    return L


def _unblocked_among_first8(g, blocked, Q, r, lo_hi):
    out = []
    for i in range(len(CROWD_BLOCKED)):
        lvl = int(Q["level"][i])
        cand = g.features_in_area(Q["x"][i], Q["y"][i], r, *lo_hi(lvl))
        assert len(cand) == len(CROWD) > 8, (i, cand)                     # more candidates than keys: the list is cut
        d = sr.descriptor_distances(Q["desc"][i], g.desc[cand])
        first8 = np.array(cand)[np.argsort(d, kind="stable")[:8]]          # (distance, visiting order)
        out.append(int((blocked[first8] == 0).sum()))
    return out


def test_crowded_cluster_resident_fallback(pkg, oracle, M):
    sf = c._sf()
    v, g, blocked, Q = crowded_lattice(oracle).arrays(pkg, M)
    rf = pkg.ResidentFrame(M, view=v)
    assert _unblocked_among_first8(g, blocked, Q, np.float32(4.0) * sf[1], lambda l: (l - 1, l)) == [0, 1, 0, 8]           # M3 th 1
    assert _unblocked_among_first8(g, blocked, Q, np.float32(4.0) * sf[1], lambda l: (l - 1, l + 1)) == [0, 1, 0, 8]       # M4 th 4
    a = _a3(blocked, Q, sf, 1.0, 0.9)
    want = sr.search_by_projection_points(g, **a)
    assert want[0] == 5
    c._same(M.SearchByProjectionPointsResident(rf, **a), want, "M3 crowded resident")
    c._same(M.SearchByProjectionPoints(v, **a), want, "M3 crowded")
    a = _a4(blocked, Q, sf, 4.0, check_ori=False)
    want = sr.search_by_projection_frame(g, **a)
    assert want[0] == 5
    c._same(M.SearchByProjectionFrameResident(rf, **a), want, "M4 crowded resident")
    c._same(M.SearchByProjectionFrame(v, **a), want, "M4 crowded")
