"""tests/second_reading_poseopt.py against answers that do not come from it: the < 3 rule, one round at 3..9 edges, a noise-free scene
recovering the true pose, planted outliers flagged and clean points kept, the round-restart rule, the strict > of the chi2 test -- and the
decisiveness of the committed cases under all three summation orders."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseopt_cases as pc          # noqa: E402
import poseopt_results as res       # noqa: E402
import second_reading_poseopt as sr  # noqa: E402


def rounds(trace):
    return sum(1 for ev in trace if ev[0] == "round")


def flags_by_round(trace):
    out = []
    for ev in trace:
        if ev[0] == "round":
            out.append({})
        elif ev[0] == "chi2":
            out[-1][ev[1]] = ev[4]
    return out


@pytest.mark.parametrize("name", ["ncorr_0", "ncorr_2"])
def test_fewer_than_three_edges(name):
    c, r = res.cases()[name], res.reading(name)
    has = c["q_mp"] >= 0
    assert r["n_corr"] == int(has.sum()) and r["n_good"] == 0 and rounds(r["trace"]) == 0
    assert np.all(r["outlier"][has] == 0) and np.all(r["outlier"][~has] == -1)            # cleared where a MapPoint sits, untouched elsewhere
    assert np.array_equal(r["pose_f32"], c["tcw_in"])                                     # the pose is not touched


def test_one_round_below_ten_edges():
    assert rounds(res.reading("ncorr_3")["trace"]) == 1 and rounds(res.reading("ncorr_9")["trace"]) == 1
    assert rounds(res.reading("ncorr_10")["trace"]) == 4


def test_noise_free_scene_recovers_the_true_pose():
    c, r = res.cases()["noise_free"], res.reading("noise_free")
    # the observations are the float32 roundings of exact projections (3e-5 px): the pose comes back to float32 precision
    assert np.max(np.abs(r["pose"] - c["truth"])) < 2e-6
    assert r["n_good"] == r["n_corr"] == 70 and not np.any(r["outlier"] == 1)


@pytest.mark.parametrize("name", ["all_mono", "all_stereo", "mixed"])
def test_planted_outliers_flagged_and_clean_points_kept(name):
    c, r = res.cases()[name], res.reading(name)
    has = c["q_mp"] >= 0
    assert c["planted"].sum() >= 10
    assert np.all(r["outlier"][c["planted"]] == 1), "a planted gross outlier (15 px or more) was not flagged"
    assert np.all(r["outlier"][has & ~c["planted"]] == 0), "a clean point (noise clipped at 1.32 sigma per axis) was flagged"
    assert r["n_good"] == int((has & ~c["planted"]).sum())


def test_point_behind_the_camera_is_kept():
    """fx * x / z + cx is the same pixel for (x, y, z) and (-x, -y, -z), and the pose-only mono edge makes no depth test
    (isDepthPositive is never called): a point behind the camera whose mirror image projects onto its observation stays an inlier."""
    c, r = res.cases()["behind_camera"], res.reading("behind_camera")
    slots = np.nonzero(c["q_mp"] >= 0)[0][:c["behind"]]
    Xc = (c["truth"][:, :3] @ c["mp_pw"][c["q_mp"][slots]].astype(np.float64).T).T + c["truth"][:, 3]
    assert np.all(Xc[:, 2] < 0) and np.all(r["outlier"][slots] == 0)


def test_round_restart_rule():
    """Continuing each round from the previous round's pose is another function: on this scene it ends with another flag set."""
    args = pc.reading_args(res.cases()["restart_matters"])
    a, b = res.reading("restart_matters"), sr.pose_optimization(*args, restart=False)
    assert not np.array_equal(a["outlier"], b["outlier"]) and a["n_good"] != b["n_good"]


def test_rounds_one_and_two_start_alike():
    """Rounds 1 and 2 both run with the kernel from the input pose: when round 1 confirms round 0's flags they meet the same active set
    and their first chi sum is the same number, which a continued estimate would not give."""
    r = res.reading("mixed")
    fl = flags_by_round(r["trace"])
    assert fl[0] == fl[1]
    starts, want = [], False
    for ev in r["trace"]:
        if ev[0] == "round":
            want = True
        elif ev[0] == "rho" and want:
            starts.append(ev[1]); want = False
    assert len(starts) == 4 and starts[1] == starts[2] and starts[0] != starts[1]


def test_strict_greater_at_the_threshold():
    th = float(np.float32(5.991))
    up = float(np.nextafter(np.float32(5.991), np.float32(10)))
    assert not sr.classify_chi2(th, False) and sr.classify_chi2(up, False)                # a residual exactly on the threshold stays in
    assert not sr.classify_chi2(float(np.nextafter(th, 10.0)), False)                     # a double just above rounds to the float threshold
    th3 = float(np.float32(7.815))
    assert not sr.classify_chi2(th3, True) and sr.classify_chi2(float(np.nextafter(np.float32(7.815), np.float32(10))), True)


def test_readmitted_edge():
    fl = flags_by_round(res.reading("readmit")["trace"])
    back = [s for s in fl[0] if fl[0][s] and not fl[-1][s]]
    assert len(fl) == 4 and back, "no edge flagged by round 0 was readmitted"


def test_empty_active_set():
    c, r = res.cases()["empty_round1"], res.reading("empty_round1")
    assert sum(1 for ev in r["trace"] if ev[0] == "empty") == 3 and r["n_good"] == 0
    # the estimate stays where setEstimate put it: the input pose through SE3Quat
    assert np.max(np.abs(r["pose"] - c["tcw_in"].astype(np.float64))) < 1e-6


def test_rejected_last_trial():
    r = res.reading("rejected_last_trial")
    ends = [ev for ev in r["trace"] if ev[0] == "terminate"]
    assert any(ev[1] == 10 and ev[2] < 0 for ev in ends), "no round ended on a rejected tenth trial"


def test_float_invz_changes_the_third_residual():
    c = res.cases()["stereo_invz"]
    T = c["tcw_in"].astype(np.float64)
    s = np.nonzero(c["q_mp"] >= 0)[0]
    Xc = (T[:, :3] @ c["mp_pw"][c["q_mp"][s]].astype(np.float64).T).T + T[:, 3]
    fx, cx, bf = float(pc.K[0]), float(pc.K[2]), float(pc.BF)
    invz_f, invz_d = (1.0 / Xc[:, 2]).astype(np.float32).astype(np.float64), 1.0 / Xc[:, 2]
    r_f = c["uright"][s] - ((Xc[:, 0] * invz_f * fx + cx) - bf * invz_f)
    r_d = c["uright"][s] - ((Xc[:, 0] * invz_d * fx + cx) - bf * invz_d)
    assert np.any(r_f != r_d)


@pytest.mark.parametrize("name", pc.DECISIVE)
def test_decisive_cases(name):
    for o in res.ORDERS:
        assert sr.decisive(res.reading(name, o)["trace"]), "%s is not decisive under the %s order: replace the seed" % (name, o)


@pytest.mark.parametrize("name", pc.FLOOR)
def test_rounding_floor_cases_decide_their_flags(name):
    for o in res.ORDERS:
        r = res.reading(name, o)
        assert sr.flags_decisive(r["trace"]), "%s: a chi2 sits within 1e-6 of its threshold under the %s order" % (name, o)
        assert np.array_equal(r["outlier"], res.reading(name)["outlier"]) and r["n_good"] == res.reading(name)["n_good"]


def test_every_case_is_classified():
    names = set(res.cases())
    assert names == set(pc.DECISIVE) | set(pc.FLOOR) | set(pc.KNIFE_EDGE)
    assert not (set(pc.DECISIVE) & set(pc.FLOOR)) and set(pc.SEEDED) <= names


def test_spread_is_at_rounding_level():
    s = res.family_spread()
    assert 0 < s["all"] < 1e-11, s           # a few ulp of double per operation, accumulated over at most forty solves
