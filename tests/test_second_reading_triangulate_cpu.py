"""tests/second_reading_triangulate.py held to answers that do not come from it: a noise-free point comes back, every gate of
LocalMapping.cc:746-892 is tripped by a hand-placed point, the two rules that are easy to read otherwise (u2_r uses KeyFrame 1's mbf; the
`else if (bStereo2)`) are shown on inputs where the other reading differs, and every committed case of tests/triangulate_cases.py is
decisive: no comparison lies where the x3D tolerance could move it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_reading_triangulate as sr   # noqa: E402
import triangulate_cases as tc            # noqa: E402
import triangulate_results as res         # noqa: E402

T1 = np.eye(3, 4)
T2 = np.concatenate([np.eye(3), [[-0.5], [0.0], [0.0]]], axis=1)        # a camera at (0.5, 0, 0)
X = np.array([0.3, -0.2, 5.0])


def feature(T, Xw, octave=3, stereo=False, mbf=tc.MBF, du=0.0, dv=0.0, **kw):
    u, v, z = tc.project(T, Xw)
    o = {"x": u + du, "y": v + dv, "octave": octave}
    if stereo:
        o["uright"] = u + du - float(mbf) / z; o["depth"] = z
    o.update(kw)
    return o


def one(c):
    r = sr.read_case(c)
    return int(r["reason"][0, 0]), r["x3d"][0, 0], r


def test_a_noise_free_point_comes_back():
    for Xw in (X, np.array([-1.5, 0.7, 2.5]), np.array([2.0, 1.0, 11.0])):
        reason, x3d, _ = one(tc.single(feature(T1, Xw, octave=int(np.clip(np.round(np.log(np.linalg.norm(Xw) / 1.5) / np.log(1.2)), 0, 7))),
                                       feature(T2, Xw, octave=int(np.clip(np.round(np.log(np.linalg.norm(Xw) / 1.5) / np.log(1.2)), 0, 7))), T1, T2))
        assert reason == sr.OK_TRI
        assert np.abs(x3d - Xw).max() / np.linalg.norm(Xw) < 1e-4


def test_unproject_stereo_reads_mvKeys_and_comes_back():
    """Little ray parallax (motion along the axis) and a close stereo point: UnprojectStereo_ of KeyFrame 1, from the RAW keypoint."""
    Tf = np.concatenate([np.eye(3), [[0.0], [0.0], [-0.05]]], axis=1)
    Xw = np.array([0.02, 0.01, 1.0])
    o1 = feature(T1, Xw, octave=0, stereo=True); o2 = feature(Tf, Xw, octave=0)
    reason, x3d, _ = one(tc.single(o1, o2, T1, Tf))
    assert reason == sr.OK_ST1 and np.abs(x3d - Xw).max() < 1e-4
    o1["kx"] = o1["x"] + 4.2                                            # mvKeys off mvKeysUn: the unprojection follows mvKeys, the reprojection test reads mvKeysUn
    reason, _, r = one(tc.single(o1, o2, T1, Tf))
    assert reason == sr.CHI2_1 and abs(r["matches"][(0, 0)]["x3d"][0] - (Xw[0] + 4.2 / 420.0)) < 1e-4


GATES = {
    "low_parallax": (lambda: tc.single(feature(T1, X * 400), feature(T2, X * 400), T1, T2), sr.LOW_PARALLAX),
    "behind_1": (lambda: tc.single(feature(T1, X, du=-40.0), feature(T2, X, du=+40.0), T1, T2), sr.BEHIND_1),             # rays that diverge
    "behind_2": (lambda: tc.single(feature(T1, X), feature(T2, X), T1, np.concatenate([T2[:, :3], [[-0.5], [0.0], [-30.0]]], axis=1), ow2=[0.5, 0, 0]), sr.BEHIND_2),
    "chi2_1": (lambda: tc.single(feature(T1, X, dv=+12.0), feature(T2, X, dv=-12.0), T1, T2), sr.CHI2_1),
    "chi2_1_stereo": (lambda: tc.single(feature(T1, X, stereo=True, uright=100.0), feature(T2, X), T1, T2), sr.CHI2_1),
    "chi2_2": (lambda: tc.single(feature(T1, X, octave=7, dv=6.0), feature(T2, X, octave=0, dv=-6.0), T1, T2), sr.CHI2_2),     # 6 px: inside level 7's sigma, outside level 0's
    "dist_zero": (lambda: _dist_zero(), sr.DIST_ZERO),
    "far_on": (lambda: tc.single(feature(T1, X), feature(T2, X), T1, T2, th_far=4.0), sr.FAR),
    "far_off": (lambda: tc.single(feature(T1, X), feature(T2, X), T1, T2, th_far=0.0), sr.OK_TRI),
    "far_equal_rejects": (lambda: tc.single(feature(T1, np.array([0.0, 0.0, 4.0]), octave=3), feature(T2, np.array([0.0, 0.0, 4.0]), octave=3), T1, T2, th_far=4.0), sr.FAR),
    "scale_low": (lambda: tc.single(feature(T1, X, octave=7), feature(T2, X, octave=0), T1, T2), sr.SCALE),              # ratioOctave 3.58 > 1.8
    "scale_high": (lambda: tc.single(feature(T1, X, octave=0), feature(T2, X, octave=4), T1, T2), sr.SCALE),             # ratioOctave 0.48 < 1 / 1.8
    "octave_below": (lambda: tc.single(feature(T1, X, octave=-1), feature(T2, X), T1, T2), sr.BAD_OCTAVE),
    "octave_past": (lambda: tc.single(feature(T1, X), feature(T2, X, octave=tc.NLEVELS), T1, T2), sr.BAD_OCTAVE),
    "depth_zero_unprojects_to_zeros": (lambda: tc.single(feature(T1, X, stereo=True, depth=0.0), feature(T2, X), T1, T2), sr.BEHIND_1),
    "w_zero": (lambda: _w_zero(), sr.W_ZERO),
}


def _dist_zero():
    """A point on KeyFrame 2's camera centre as the caller gave it: x3D comes from UnprojectStereo_ of KeyFrame 1, ow2 is set to those bits."""
    Tf = np.concatenate([np.eye(3), [[0.0], [0.0], [0.05]]], axis=1)
    Xw = np.array([0.02, 0.01, 1.0])
    c = tc.single(feature(T1, Xw, octave=0, stereo=True), feature(Tf, Xw, octave=0), T1, Tf)
    x3d = sr.read_case(c)["x3d"][0, 0]
    c["pool2"]["ow"][0] = x3d
    return c


def _w_zero():
    """x3D_h(3) == 0 exactly: both features on the principal point, and a second `pose` whose third row is tilted while its first two are
    the unit rows -- no rotation, but column 2 of A is exactly zero, so the null vector is (0, 0, 1, 0), and the rays still part."""
    Tt = np.array([[1.0, 0, 0, -0.5], [0, 1.0, 0, 0.25], [np.sin(0.1), 0, np.cos(0.1), 0]])
    o = {"x": float(tc.K[2]), "y": float(tc.K[3]), "octave": 0}
    return tc.single(dict(o), dict(o), T1, Tt, ow2=[0.5, -0.25, 0])


@pytest.mark.parametrize("name", sorted(GATES))
def test_each_gate_is_tripped_by_a_hand_placed_point(name):
    make, want = GATES[name]
    reason, x3d, r = one(make())
    assert reason == want, (sr.NAMES[reason], sr.NAMES[want], r["matches"].get((0, 0), {}).get("trace"))
    if name == "depth_zero_unprojects_to_zeros":
        assert not np.any(x3d) and not np.any(r["matches"][(0, 0)]["x3d"])


def test_u2r_uses_keyframe_1s_mbf():
    """:861 subtracts mpCurrentKeyFrame->mbf * invz2 in the SECOND KeyFrame's stereo error.  With a neighbour whose own bf is 84 against the
    current KeyFrame's 46.2, a right coordinate laid with bf 46.2 passes and one laid with the neighbour's own 84 fails; the other reading
    (pKF2->mbf) would say the opposite: its error would be 37.8 / 5 = 7.6 px against a limit of sqrt(7.8 * 2.99) = 4.8 px."""
    mbf2 = np.float32(0.2) * tc.K[0]
    with_mbf1 = tc.single(feature(T1, X), feature(T2, X, stereo=True, mbf=tc.MBF), T1, T2, mb2=0.2)
    with_mbf2 = tc.single(feature(T1, X), feature(T2, X, stereo=True, mbf=mbf2), T1, T2, mb2=0.2)
    assert one(with_mbf1)[0] == sr.OK_TRI and one(with_mbf2)[0] == sr.CHI2_2
    assert ((float(mbf2) - float(tc.MBF)) / 5.0) ** 2 > 7.8 * float(tc.LS[3])


def test_else_if_bstereo2():
    """Both features stereo: cosParallaxStereo2 is NOT computed (`else if`), it stays cosParallaxRays + 1.  KeyFrame 1's depth says 200 m
    (cos 0.9999999), KeyFrame 2's says 0.4 m (cos 0.963), the rays make 0.995.  As written: 0.995 < min(0.9999999, 1.995) triangulates.
    Read as two independent ifs, min(...) = 0.963, the rays lose and UnprojectStereo_ of KeyFrame 2 would run."""
    o1 = feature(T1, X, stereo=True, depth=200.0); o2 = feature(T2, X, stereo=True, depth=0.4)
    reason, _, r = one(tc.single(o1, o2, T1, T2))
    assert reason == sr.OK_TRI
    cos_rays = dict((n, l) for n, l, _, _ in r["matches"][(0, 0)]["trace"])["rays_lt_stereo"]
    assert sr._cos_stereo(tc.MB, 0.4) < cos_rays < sr._cos_stereo(tc.MB, 200.0)
    only2 = tc.single(feature(T1, X), o2, T1, T2)                       # KeyFrame 1 not stereo: now cosParallaxStereo2 counts
    assert one(only2)[2]["matches"][(0, 0)]["how"] == sr.OK_ST2          # the branch taken (the point, 0.4 m away, then fails a gate)


def test_cross_pair_rule_on_a_hand_built_group():
    """idx1 0 is matched in pairs 0 and 2: where pair 0 succeeds pair 2 is dropped, where pair 0 fails pair 2 creates the point."""
    for fail0 in (False, True):
        c = tc.single(feature(T1, X), feature(T2, X, dv=40.0 if fail0 else 0.0), T1, T2)
        p2 = tc.empty_pool(3, 1)
        for row, dv in ((0, 40.0 if fail0 else 0.0), (1, 0.0), (2, 0.0)):
            Tn = np.concatenate([np.eye(3), [[-0.5 - 0.1 * row], [0.0], [0.0]]], axis=1)
            f = feature(Tn, X, dv=dv)
            p2["tcw"][row] = Tn.astype(np.float32).reshape(12); p2["ow"][row] = [0.5 + 0.1 * row, 0, 0]; p2["counts"][row] = 1
            p2["kps_un"][row]["x"][0], p2["kps_un"][row]["y"][0], p2["kps_un"][row]["octave"][0] = f["x"], f["y"], 3
        p2["kps"] = None
        c.update(pool2=p2, group_start=np.array([0, 3], np.int32), row1=np.zeros(3, np.int32), row2=np.arange(3, dtype=np.int32),
                 matches12=np.array([[0], [-1], [0]], np.int32))
        r = sr.read_case(c)
        if fail0:
            assert r["reason"][0, 0] in (sr.CHI2_1, sr.CHI2_2) and list(r["reason"][1:, 0]) == [sr.NO_MATCH, sr.OK_TRI] and r["won_pair"][0, 0] == 2 and list(r["ncreated"]) == [0, 0, 1]
        else:
            assert list(r["reason"][:, 0]) == [sr.OK_TRI, sr.NO_MATCH, sr.TAKEN] and r["won_pair"][0, 0] == 0 and list(r["ncreated"]) == [1, 0, 0]


@pytest.mark.parametrize("name", sorted(tc.CASES) + sorted(tc.GPU_CASES))
def test_committed_cases_are_decisive(name):
    und = res.undecided(res.cases()[name], res.reading(name))
    assert und == [], "replace the seed: %s" % und[:5]


def test_committed_cases_reach_the_exits():
    seen, both_ways = set(), [False, False]
    for name in tc.CASES:
        r = res.reading(name)
        seen |= set(int(v) for v in np.unique(r["reason"]))
        c = res.cases()[name]
        if len(c["row1"]) >= 3:
            ok = r["reason"] <= sr.OK_ST2
            tried0 = (r["reason"][0] > sr.TAKEN)
            both_ways[0] |= bool(np.any(tried0 & ok[2])); both_ways[1] |= bool(np.any(ok[0] & (r["reason"][2] == sr.TAKEN)))
        # the order is pair by pair, ascending idx1 inside a pair
        for g in range(len(r["ntotal"])):
            o = r["order"][g, :r["ntotal"][g]]; wp = r["won_pair"][g][o]
            assert np.all(np.diff(wp) >= 0) and all(np.all(np.diff(o[wp == p]) > 0) for p in np.unique(wp))
    assert {sr.OK_TRI, sr.OK_ST1, sr.OK_ST2, sr.NO_MATCH, sr.TAKEN, sr.BAD_OCTAVE, sr.LOW_PARALLAX, sr.BEHIND_1, sr.CHI2_1, sr.FAR, sr.SCALE} <= seen
    assert all(both_ways), "an idx1 matched in pairs 0 and 2 whose pair-0 attempt fails, and one whose attempt succeeds"
    assert np.any(res.reading("far_on")["reason"] == sr.FAR) and not np.any(res.reading("far_off")["reason"] == sr.FAR)
