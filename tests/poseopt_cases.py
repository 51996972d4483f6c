"""Scenes for the pose-optimisation tests: seeded scenes (a true pose, points in front of the camera, observations with level-scaled noise,
a share of gross outliers, some points with uright, a start pose off by a motion-model-sized error) and constructed ones.  Every case is a
dict of flat arrays in the layout of orbm_pose_optimization: kps (KP_DTYPE rows), uright or None, q_mp (indices into the pool, -1 =
NULL), mp_pw, tcw_in [3][4] float32, K, bf, ils2 (mvInvLevelSigma2).

Every case is in exactly one of three lists (below, with the reasoning): DECISIVE -- every comparison of the second reading's trace
keeps 1e-6 from its threshold under all three summation orders, asserted by tests/test_second_reading_poseopt_cpu.py: flags, counts and
the pose before the final rounding are compared; KNIFE_EDGE -- constructed cases that sit on a threshold by design (the start is the
optimum, rho = +-tiny); FLOOR -- scenes in which Levenberg-Marquardt reaches the rounding floor, so that rho's sign is noise in the last
trials while every chi2 test stays decisive.  On the last two, flags, counts and the pose after rounding are compared exactly as on a
decisive case, and the pose before rounding within 4 max(s, the case's own spread between the reading's three summation orders).  A seeded case that should
be decisive and is not is replaced by another seed here, never skipped."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
K = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
BF = np.float32(47.90639384423901)
NLEVELS = 8
ILS2 = (1.0 / (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)) ** 2).astype(np.float32)
W, H = 752, 480


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def scene(seed, n_slots, n_corr, stereo_share=0.4, outlier_share=0.15, noise=0.6, rot_err=0.01, trans_err=0.03, behind=0, nmp_extra=7,
          outlier_px=(15.0, 80.0), noise_free=False, start_at_truth=False, clip=None):
    """n_slots keypoints of which n_corr hold a MapPoint (spread over the slots); returns the case dict with the truth attached."""
    rs = np.random.RandomState(seed)
    Rt = rodrigues(rs.uniform(-0.3, 0.3, 3))
    tt = rs.uniform(-1.0, 1.0, 3)
    fx, fy, cx, cy = [float(v) for v in K]
    kps = np.zeros(n_slots, KP_DTYPE)
    kps["x"] = rs.uniform(20, W - 20, n_slots); kps["y"] = rs.uniform(20, H - 20, n_slots)
    kps["octave"] = rs.randint(0, NLEVELS, n_slots); kps["size"] = 31.0; kps["angle"] = rs.uniform(0, 360, n_slots)
    uright = np.full(n_slots, -1.0, np.float32)
    nmp = n_corr + nmp_extra
    mp_pw = rs.uniform(-5, 5, (nmp, 3)).astype(np.float32)
    q_mp = np.full(n_slots, -1, np.int32)
    slots = np.sort(rs.choice(n_slots, n_corr, replace=False)) if n_corr else np.zeros(0, np.int64)
    pool = rs.permutation(nmp)[:n_corr]
    planted = np.zeros(n_slots, bool)
    for k, (s, j) in enumerate(zip(slots, pool)):
        z = rs.uniform(2.0, 12.0)
        if k < behind:
            z = -z
        u, v = float(kps["x"][s]), float(kps["y"][s])
        Xc = np.array([(u - cx) * z / fx, (v - cy) * z / fy, z])
        mp_pw[j] = (Rt.T @ (Xc - tt)).astype(np.float32)
        q_mp[s] = j
        Xc = Rt @ mp_pw[j].astype(np.float64) + tt                # the float32 point's own projection is the clean observation
        sig = 0.0 if noise_free else noise * 1.2 ** int(kps["octave"][s])
        du, dv, dr = (rs.normal(0, 1, 3) if clip is None else np.clip(rs.normal(0, 1, 3), -clip, clip)) * sig
        if k >= behind and rs.uniform() < outlier_share and not noise_free:
            a, r = rs.uniform(0, 2 * np.pi), rs.uniform(*outlier_px)
            du, dv = du + r * np.cos(a), dv + r * np.sin(a)
            planted[s] = True
        kps["x"][s] = fx * Xc[0] / Xc[2] + cx + du
        kps["y"][s] = fy * Xc[1] / Xc[2] + cy + dv
        if rs.uniform() < stereo_share and Xc[2] > 0:
            uright[s] = max(0.0, fx * Xc[0] / Xc[2] + cx - float(BF) / Xc[2] + dr)
    dR = rodrigues(rs.normal(0, 1, 3) * (0.0 if start_at_truth else rot_err))
    dt = rs.normal(0, 1, 3) * (0.0 if start_at_truth else trans_err)
    T0 = np.concatenate([dR @ Rt, (dR @ tt + dt).reshape(3, 1)], axis=1).astype(np.float32)
    Ttrue = np.concatenate([Rt, tt.reshape(3, 1)], axis=1)
    return {"kps": kps, "uright": uright if stereo_share > 0 else None, "q_mp": q_mp, "mp_pw": mp_pw, "tcw_in": T0, "K": K, "bf": BF, "ils2": ILS2,
            "truth": Ttrue, "planted": planted, "behind": behind}


def all_outliers(seed, n_slots=40, n_corr=14):
    """One world point seen by every edge, observed on a ring of 100 px around its projection: no pose brings any edge under its
    threshold, round 0 flags every edge and rounds 1 to 3 have an empty active set."""
    c = scene(seed, n_slots, n_corr, stereo_share=0.0, outlier_share=0.0, noise_free=True)
    slots = np.nonzero(c["q_mp"] >= 0)[0]
    j0 = c["q_mp"][slots[0]]
    c["q_mp"][slots] = j0
    u0, v0 = float(c["kps"]["x"][slots[0]]), float(c["kps"]["y"][slots[0]])
    a = 2 * np.pi * np.arange(len(slots)) / len(slots)
    c["kps"]["x"][slots] = u0 + 100.0 * np.cos(a); c["kps"]["y"][slots] = v0 + 100.0 * np.sin(a)
    c["kps"]["octave"][slots] = 0
    c["uright"] = None
    return c


# GPU shapes: the wave edge, the workgroup edge, two and three edges per thread with a ragged tail
GPU_NCORR = (0, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257, 513)
CAP = 600


def build_cases():
    cases = {}
    for k, nc in enumerate(GPU_NCORR):
        if nc in DECISIVE_SEED:
            cases["ncorr_%d" % nc] = scene(DECISIVE_SEED[nc], nc + 8, nc)
        else:
            cases["ncorr_%d" % nc] = scene(100 + k, min(CAP, max(nc + 5 + 7 * k, 12)), nc)
    # noise clipped at 2.2 standard deviations of 0.6 sigma: a clean point's chi2 stays under 3.5 (mono) / 5.3 (stereo) at the true pose,
    # a planted outlier's (15 px or more, sigma at most 3.6 px) above 12: which edges end flagged is known without running anything
    cases["all_mono"] = scene(201, 150, 120, stereo_share=0.0, clip=2.2)
    cases["all_stereo"] = scene(202, 150, 120, stereo_share=1.0, clip=2.2)
    cases["mixed"] = scene(203, 300, 220, stereo_share=0.5, clip=2.2)
    cases["readmit"] = scene(READMIT_SEED, 120, 80, stereo_share=0.3, outlier_share=0.2, rot_err=0.03, trans_err=0.15, outlier_px=(3.0, 9.0))
    cases["empty_round1"] = all_outliers(205)
    cases["behind_camera"] = scene(206, 90, 60, behind=3)
    cases["stereo_invz"] = scene(207, 40, 30, stereo_share=1.0, outlier_share=0.0)
    cases["noise_free"] = scene(208, 100, 70, noise_free=True)
    cases["rejected_last_trial"] = scene(REJECT_SEED, 60, 40, stereo_share=0.3)
    # a start so far off that ten iterations from it do not settle: continuing from round 0's pose would end elsewhere (the restart rule)
    cases["restart_matters"] = scene(RESTART_SEED, 90, 60, stereo_share=0.3, outlier_share=0.3, rot_err=0.25, trans_err=1.2)
    cases["start_at_optimum"] = scene(210, 80, 50, noise_free=True, start_at_truth=True)
    return cases


READMIT_SEED = 2042        # slots 75 and 101 are flagged after round 0 and readmitted later
REJECT_SEED = 3003         # every round after the first ends on a rejected tenth trial (qmax == 10)
RESTART_SEED = 4118
# Seeds found by search on the CPU whose every comparison keeps 1e-6 under all three summation orders: 5 of 25 seeds at 3 edges, 5 of
# 60 at 9, 5 of 291 at 10 -- and none of 400 at 24 edges, none of 150 at 65.  With 10 or more edges all four rounds run, each for up
# to ten iterations, and Levenberg-Marquardt reaches the rounding floor in every one of them: the last trials compare two chi sums that
# agree to 1e-9 .. 1e-16, so rho's sign sits on its threshold in every such scene whatever the seed.  Those scenes are therefore named in
# FLOOR below.  They are held to everything a decisive case is held to (flags, n_corr, n_good, the pose after rounding) except that the
# bound before rounding is 4 max(s, the case's own spread between the reading's three orders): where the reading's own orders part ways the
# reading's error IS that spread.  Also asserted on them: every comparison that decides a FLAG (chi2 against its threshold) keeps 1e-6.
DECISIVE_SEED = {3: 1000, 9: 1003, 10: 1099}
DECISIVE = ("ncorr_0", "ncorr_2", "ncorr_3", "ncorr_9", "ncorr_10", "empty_round1")
KNIFE_EDGE = ("start_at_optimum",)
FLOOR = tuple("ncorr_%d" % n for n in GPU_NCORR if n > 10) + ("all_mono", "all_stereo", "mixed", "readmit", "behind_camera", "stereo_invz",
                                                              "noise_free", "rejected_last_trial", "restart_matters")
SEEDED = tuple("ncorr_%d" % n for n in GPU_NCORR) + ("all_mono", "all_stereo", "mixed")


def reading_args(c):
    """The argument list of second_reading_poseopt.pose_optimization for a case."""
    has = c["q_mp"] >= 0
    Xw = np.zeros((len(has), 3), np.float32)
    Xw[has] = c["mp_pw"][c["q_mp"][has]]
    xy = np.stack([c["kps"]["x"], c["kps"]["y"]], axis=1)
    return (xy, c["kps"]["octave"], c["uright"], has, Xw, c["tcw_in"], c["K"], c["bf"], c["ils2"])
