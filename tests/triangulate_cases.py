"""Scenes for the CreateNewMapPoints tests: a current KeyFrame, its neighbours, features that observe common world points, and the
matches12 rows M10 would hand over -- as the arrays of orbm_triangulate_new_points.  Everything is float32 where the library reads float32;
nothing here looks at what any implementation answers.  case(...) builds a scene from a seed; CASES names the committed ones;
single(...) lays one hand-placed match."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
NLEVELS, SCALE = 8, np.float32(1.2)
SF = np.cumprod(np.concatenate([[np.float32(1)], np.full(NLEVELS - 1, SCALE, np.float32)])).astype(np.float32)      # mvScaleFactors
LS = (SF * SF).astype(np.float32)                                                                                    # mvLevelSigma2
W, H = 752, 480
K = np.array([420.0, 420.0, 376.0, 240.0, 1.0 / 420.0, 1.0 / 420.0], np.float32)        # fx fy cx cy invfx invfy (invfx = 1.0f / fx as Frame.cc)
K[4] = np.float32(1.0) / K[0]; K[5] = np.float32(1.0) / K[1]
MB = np.float32(0.11); MBF = np.float32(MB * K[0])
RATIO_FACTOR = np.float32(np.float32(1.5) * SCALE)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def pose_rows(Rcw, ow):
    """tcw [12] and ow [3] in float32 for a camera with rotation Rcw at centre ow: tcw = -Rcw ow, then Ow = -Rcw^T tcw from the float32 pose."""
    R = Rcw.astype(np.float32); t = (-(Rcw @ ow)).astype(np.float32)
    T = np.concatenate([R, t[:, None]], axis=1).astype(np.float32)
    o = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(np.float32)
    return T.reshape(12), o


def empty_pool(rows, cap):
    kp = np.zeros((rows, cap), KP_DTYPE)
    return {"kps_un": kp, "kps": kp.copy(), "counts": np.zeros(rows, np.int32), "uright": np.full((rows, cap), -1, np.float32),
            "depth": np.full((rows, cap), -1, np.float32), "tcw": np.zeros((rows, 12), np.float32), "ow": np.zeros((rows, 3), np.float32)}


def observe(pool, row, slot, Xw, rng, stereo, noise=0.4, octave=None, dist_shift=(0.6, -0.3)):
    """Slot `slot` of `row` sees the world point Xw: undistorted keypoint with pixel noise, the raw keypoint a little off it (a distortion
    model), the octave the distance asks for, and with `stereo` a right coordinate and a depth."""
    T = pool["tcw"][row].reshape(3, 4).astype(np.float64)
    Xc = T[:, :3] @ Xw + T[:, 3]
    z = Xc[2] if abs(Xc[2]) > 1e-6 else 1e-6
    lvl = int(np.clip(np.round(np.log(max(np.linalg.norm(Xc), 1e-3) / 1.5) / np.log(1.2)), 0, NLEVELS - 1)) if octave is None else octave
    s = noise * float(SF[min(max(lvl, 0), NLEVELS - 1)])
    u = K[0] * Xc[0] / z + K[2] + rng.normal(0, s); v = K[1] * Xc[1] / z + K[3] + rng.normal(0, s)
    kp = pool["kps_un"][row]; kr = pool["kps"][row]
    kp["x"][slot], kp["y"][slot], kp["octave"][slot], kp["size"][slot] = u, v, lvl, 31 * float(SF[min(max(lvl, 0), NLEVELS - 1)])
    kr[slot] = kp[slot]; kr["x"][slot] += np.float32(dist_shift[0]); kr["y"][slot] += np.float32(dist_shift[1])
    if stereo:
        ur = u - float(MBF) / z + rng.normal(0, s)
        pool["uright"][row, slot] = ur
        pool["depth"][row, slot] = np.float32(MBF) / np.float32(max(u - ur, 1e-3))
    return lvl


def case(seed, n1=40, cap=48, nneigh=2, stereo1=0.0, stereo2=0.0, th_far=0.0, groups=1, match_rate=0.7, wrong_rate=0.08, repeat_rate=0.5,
         far_rate=0.05, behind_rate=0.04, zero_depth_rate=0.0, octave_off_rate=0.06, bad_octave_rate=0.0, one_pool=False, depth_range=(2.0, 12.0), forward=0.0, later_extra=0.15):
    """`groups` current KeyFrames (rows 0 .. groups - 1 of pool 1) with `nneigh` neighbours each (pool 2, or the same pool with one_pool)."""
    rng = np.random.default_rng(seed)
    rows2 = groups * nneigh
    p1 = empty_pool(groups + (rows2 if one_pool else 0), cap)
    p2 = p1 if one_pool else empty_pool(rows2, cap)
    off2 = groups if one_pool else 0
    gs, row1, row2, m12 = [0], [], [], []
    for g in range(groups):
        c0 = np.array([0.3 * g, 0.0, 0.0]) + rng.normal(0, 0.05, 3)          # near the origin: the bound on x3D_h grows with |Ow| (sigma1)
        R0 = rot(*rng.normal(0, 0.03, 3))
        p1["tcw"][g], p1["ow"][g] = pose_rows(R0, c0)
        n = int(n1) if np.isscalar(n1) else int(n1[g])
        p1["counts"][g] = n
        # world points in front of the current KeyFrame
        z = rng.uniform(*depth_range, n)
        far = rng.random(n) < far_rate
        z[far] = rng.uniform(400.0, 2000.0, int(far.sum()))                 # low parallax: cos >= 0.9998 for every baseline here
        uu = rng.uniform(60, W - 60, n); vv = rng.uniform(40, H - 40, n)
        Xc = np.stack([(uu - K[2]) / K[0] * z, (vv - K[3]) / K[1] * z, z], 1)
        Xw = (R0.T @ Xc.T).T + c0
        for i in range(n):
            st = bool(rng.random() < stereo1) and not far[i]                # a far point is mono: with a stereo flag it would triangulate at the edge of rank
            observe(p1, g, i, Xw[i], rng, st)
            if st and rng.random() < zero_depth_rate:
                p1["depth"][g, i] = 0.0                                     # mvDepth <= 0 with mvuRight >= 0: UnprojectStereo_ returns zeros
            if rng.random() < bad_octave_rate:
                p1["kps_un"][g]["octave"][i] = rng.choice([-1, NLEVELS, NLEVELS + 3])
        for j in range(nneigh):
            r2 = off2 + g * nneigh + j
            ang = 2 * np.pi * j / max(nneigh, 1) + rng.normal(0, 0.2)
            c = c0 + np.array([np.cos(ang), 0.3 * np.sin(ang), 0.25 * np.sin(2 * ang)]) * rng.uniform(0.35, 0.8)
            if rng.random() < forward:                                      # motion along the optical axis: little ray parallax near the epipole
                c = c0 + R0.T @ np.array([rng.normal(0, 0.02), rng.normal(0, 0.02), rng.choice([-1.0, 1.0]) * rng.uniform(0.15, 0.4)])
            p2["tcw"][r2], p2["ow"][r2] = pose_rows(rot(*rng.normal(0, 0.04, 3)) @ R0, c)
            n2 = min(cap, n + int(rng.integers(0, max(cap - n, 0) + 1)))
            p2["counts"][r2] = n2
            perm = rng.permutation(n2)
            row = np.full(cap, -1, np.int32)
            for i in range(n2):
                slot = int(perm[i])
                src = Xw[i] if i < n else c + (rot(*rng.normal(0, 0.04, 3)) @ R0).T @ np.array([rng.normal(0, 1), rng.normal(0, 1), rng.uniform(2, 9)])
                st = bool(rng.random() < stereo2) and not (i < n and far[i])
                lvl = observe(p2, r2, slot, src, rng, st)
                if rng.random() < octave_off_rate:                          # an octave the distance does not ask for: the scale test's two sides
                    p2["kps_un"][r2]["octave"][slot] = int(np.clip(lvl + rng.choice([-4, -3, 3, 4]), 0, NLEVELS - 1))
                if i < n and rng.random() < (match_rate if j == 0 else match_rate * repeat_rate + later_extra):
                    row[i] = slot
            for i in range(n):
                if rng.random() < wrong_rate:
                    row[i] = int(rng.integers(0, n2))                       # a wrong match: most fail a reprojection test
                if rng.random() < behind_rate and n2 > 1:                   # rays that meet behind a camera
                    row[i] = int(perm[(i + 1 + int(rng.integers(0, n - 1))) % n]) if n > 1 else row[i]
            row1.append(g); row2.append(r2); m12.append(row)
        gs.append(len(row1))
    return {"pool1": p1, "pool2": p2, "group_start": np.array(gs, np.int32), "row1": np.array(row1, np.int32), "row2": np.array(row2, np.int32),
            "matches12": np.array(m12, np.int32), "k1": K.copy(), "k2": K.copy(), "mb1": MB, "mbf1": MBF, "mb2": MB, "sf1": SF.copy(),
            "ls1": LS.copy(), "sf2": SF.copy(), "ls2": LS.copy(), "ratio_factor": RATIO_FACTOR, "th_far": np.float32(th_far)}


# The committed scenes: (name, keyword arguments).  Every one is decisive for the reading (tests/test_second_reading_triangulate_cpu.py); a
# seed that is not gets replaced, not excused.
CASES = {
    "mono_2": dict(seed=1, nneigh=2),
    "mono_3": dict(seed=2, nneigh=3),
    "stereo1_2": dict(seed=3, nneigh=2, stereo1=0.6),
    "stereo2_3": dict(seed=4, nneigh=3, stereo2=0.6),
    "both_stereo_3": dict(seed=5, nneigh=3, stereo1=0.5, stereo2=0.5, zero_depth_rate=0.15),
    "close_stereo": dict(seed=6, nneigh=3, stereo1=0.6, stereo2=0.6, depth_range=(0.8, 4.0), forward=1.0),      # stereo parallax beats the rays: UnprojectStereo_
    "far_on": dict(seed=7, nneigh=2, th_far=9.0),
    "far_off": dict(seed=7, nneigh=2, th_far=0.0),
    "bad_octaves": dict(seed=8, nneigh=2, stereo1=0.3, bad_octave_rate=0.15),
    "two_groups_one_pool": dict(seed=9, nneigh=3, groups=2, one_pool=True, stereo1=0.3, stereo2=0.3),
}


# The shapes the GPU test adds: row counts around the wave and workgroup sizes at cap1 320 (eight current KeyFrames in one call), a group
# of one pair and a group of 64.  Decisive like the others (the same CPU test asks).
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 300)
GPU_CASES = {
    "row_counts": dict(seed=100, n1=ROW_COUNTS, cap=320, nneigh=3, groups=len(ROW_COUNTS), stereo1=0.3, stereo2=0.3, zero_depth_rate=0.05, bad_octave_rate=0.02),
    "one_pair": dict(seed=22, nneigh=1, stereo2=0.4),
    "pairs_64": dict(seed=23, n1=30, cap=32, nneigh=64, stereo1=0.2, match_rate=0.1, repeat_rate=0.3, later_extra=0.03),
}


def cases():
    return {name: case(**kw) for name, kw in CASES.items()}


def gpu_cases():
    return {name: case(**kw) for name, kw in GPU_CASES.items()}


def single(o1, o2, T1=None, T2=None, ow1=None, ow2=None, th_far=0.0, mbf1=MBF, mb1=MB, mb2=MB, k2=None):
    """One hand-placed match as a case: one group, one pair, one slot on each side.  o = dict(x, y, octave, uright, depth, and optionally kx,
    ky for the raw keypoint)."""
    p1, p2 = empty_pool(1, 1), empty_pool(1, 1)
    for pool, o, T, ow in ((p1, o1, T1, ow1), (p2, o2, T2, ow2)):
        T = np.eye(3, 4) if T is None else np.asarray(T)
        pool["tcw"][0] = np.asarray(T, np.float32).reshape(12)
        pool["ow"][0] = (-(T[:, :3].T @ T[:, 3])).astype(np.float32) if ow is None else np.asarray(ow, np.float32)
        pool["counts"][0] = 1
        kp = pool["kps_un"][0]
        kp["x"][0], kp["y"][0], kp["octave"][0] = o["x"], o["y"], o.get("octave", 0)
        pool["kps"][0] = kp
        pool["kps"][0]["x"][0] = o.get("kx", o["x"]); pool["kps"][0]["y"][0] = o.get("ky", o["y"])
        pool["uright"][0, 0] = o.get("uright", -1.0); pool["depth"][0, 0] = o.get("depth", -1.0)
    return {"pool1": p1, "pool2": p2, "group_start": np.array([0, 1], np.int32), "row1": np.zeros(1, np.int32), "row2": np.zeros(1, np.int32),
            "matches12": np.zeros((1, 1), np.int32), "k1": K.copy(), "k2": K.copy() if k2 is None else np.asarray(k2, np.float32), "mb1": np.float32(mb1),
            "mbf1": np.float32(mbf1), "mb2": np.float32(mb2), "sf1": SF.copy(), "ls1": LS.copy(), "sf2": SF.copy(), "ls2": LS.copy(),
            "ratio_factor": RATIO_FACTOR, "th_far": np.float32(th_far)}


def project(T, X, k=K):
    """The noise-free pixel of world point X in the camera T (3x4), float64."""
    Xc = np.asarray(T)[:, :3] @ np.asarray(X, np.float64) + np.asarray(T)[:, 3]
    return k[0] * Xc[0] / Xc[2] + k[2], k[1] * Xc[1] / Xc[2] + k[3], Xc[2]
