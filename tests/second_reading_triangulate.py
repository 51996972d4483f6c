"""A second reading of step 6 of LocalMapping::CreateNewMapPoints (LocalMapping.cc:611-892; KeyFrame::UnprojectStereo_, KeyFrame.cc:1337-1352;
Pinhole::project / unproject), pinhole cameras, NLeft == -1, !mpCamera2, in numpy.  It shares nothing with csrc/orbm_triangulate.h: the
float32 steps of the reference are np.float32 operations written from the reference's text, the trigonometry is numpy's, and the null
vector of the 4x4 comes from np.linalg.svd of A in float64 -- an INDEPENDENT answer to what cv::SVD computes, against which the header's
float32 Jacobi is held to a tolerance.  Every comparison the text makes is recorded with both sides, so a test can ask how far a case
is from flipping.

A case is the dict tests/triangulate_cases.py lays out (the arrays of orbm_triangulate_new_points).  read_case walks the groups as the
reference walks vpNeighKFs: pair by pair, and inside a pair in ascending idx1, skipping an idx1 that an earlier pair turned into a
MapPoint (the cross-pair rule of INTEGRATION.md)."""
import math

import numpy as np

f32 = np.float32
# the exits, numbered as the library reports them (include/orbm.h)
OK_TRI, OK_ST1, OK_ST2, NO_MATCH, TAKEN, BAD_OCTAVE, LOW_PARALLAX, W_ZERO, BEHIND_1, BEHIND_2, CHI2_1, CHI2_2, DIST_ZERO, FAR, SCALE, MIXED = range(16)
NAMES = ["ok_triangulated", "ok_stereo1", "ok_stereo2", "no_match", "taken", "bad_octave", "low_parallax", "w_zero", "behind_1", "behind_2",
         "chi2_1", "chi2_2", "dist_zero", "far", "scale", "mixed_row1"]


def _dot(a, b):
    """cv::Matx::dot / one entry of a Matx product: a float accumulator that starts at 0."""
    s = f32(0)
    for x, y in zip(a, b):
        s = f32(s + f32(f32(x) * f32(y)))
    return s


def _norm(a):
    """cv::norm of a small Matx: the square root of a double sum."""
    s = 0.0
    for x in a:
        s += float(x) * float(x)
    return math.sqrt(s)


def _rt_mul(T, x):
    """Rcw.t() * x for the rotation block of the row-major 3x4 T."""
    return [_dot((T[0][i], T[1][i], T[2][i]), x) for i in range(3)]


def _cos_stereo(mb, depth):
    """cos(2*atan2(mb/2, depth)): mb/2 in float, the rest in double, stored to float (LocalMapping.cc:733)."""
    half = f32(f32(mb) / f32(2))
    return f32(math.cos(2.0 * math.atan2(float(half), float(f32(depth)))))


def _unproject_stereo(K, T, ow, kx, ky, depth):
    z = f32(depth)
    if not z > 0:
        return [f32(0), f32(0), f32(0)]
    x = f32(f32(f32(f32(kx) - K[2]) * z) * K[4])
    y = f32(f32(f32(f32(ky) - K[3]) * z) * K[5])
    r = _rt_mul(T, (x, y, z))
    return [f32(r[i] + f32(ow[i])) for i in range(3)]


class Trace(list):
    """[(name, lhs, rhs, after_x3d)]: every comparison made, in order; after_x3d says whether x3D entered it."""
    def cmp(self, name, lhs, rhs, after_x3d):
        self.append((name, float(lhs), float(rhs), after_x3d))


def _reproj(tr, tag, K, T, o, stereo, mbf1, sigma2, x3d, z):
    x = f32(_dot(T[0][:3], x3d) + T[0][3]); y = f32(_dot(T[1][:3], x3d) + T[1][3])
    invz = f32(1.0 / float(z))
    if not stereo:
        u = f32(f32(f32(K[0] * x) / z) + K[2]); v = f32(f32(f32(K[1] * y) / z) + K[3])
        ex = f32(u - o["ux"]); ey = f32(v - o["uy"])
        e2 = f32(f32(ex * ex) + f32(ey * ey)); lim = 5.991 * float(sigma2)
    else:
        u = f32(f32(f32(K[0] * x) * invz) + K[2])
        ur = f32(u - f32(f32(mbf1) * invz))
        v = f32(f32(f32(K[1] * y) * invz) + K[3])
        ex = f32(u - o["ux"]); ey = f32(v - o["uy"]); er = f32(ur - o["uright"])
        e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er)); lim = 7.8 * float(sigma2)
    tr.cmp("chi2_" + tag, e2, lim, True)
    return float(e2) > lim


def read_match(K1, K2, mb1, mbf1, mb2, T1, ow1, T2, ow2, o1, o2, sf1, ls1, sf2, ls2, ratio_factor, th_far):
    """One match.  o = dict(ux, uy: mvKeysUn; kx, ky: mvKeys; octave, uright, depth).  -> dict(reason, x3d [3] float32, trace, and for the
    triangulated branch A (float32 4x4), xh64 (the unit null vector in float64), sigma (A's singular values in float64))."""
    with np.errstate(all="ignore"):
        return _read_match(K1, K2, mb1, mbf1, mb2, T1, ow1, T2, ow2, o1, o2, sf1, ls1, sf2, ls2, ratio_factor, th_far)


def _read_match(K1, K2, mb1, mbf1, mb2, T1, ow1, T2, ow2, o1, o2, sf1, ls1, sf2, ls2, ratio_factor, th_far):
    K1 = [f32(v) for v in K1]; K2 = [f32(v) for v in K2]
    T1 = np.asarray(T1, f32).reshape(3, 4); T2 = np.asarray(T2, f32).reshape(3, 4)
    o1 = {k: (int(v) if k == "octave" else f32(v)) for k, v in o1.items()}; o2 = {k: (int(v) if k == "octave" else f32(v)) for k, v in o2.items()}
    tr = Trace()
    out = {"reason": None, "x3d": np.zeros(3, f32), "trace": tr}
    nl = len(sf1)
    if not (0 <= o1["octave"] < nl and 0 <= o2["octave"] < nl):
        out["reason"] = BAD_OCTAVE
        return out
    st1 = bool(o1["uright"] >= 0); st2 = bool(o2["uright"] >= 0)
    xn1 = [f32(f32(o1["ux"] - K1[2]) / K1[0]), f32(f32(o1["uy"] - K1[3]) / K1[1]), f32(1)]
    xn2 = [f32(f32(o2["ux"] - K2[2]) / K2[0]), f32(f32(o2["uy"] - K2[3]) / K2[1]), f32(1)]
    ray1 = _rt_mul(T1, xn1); ray2 = _rt_mul(T2, xn2)
    cos_rays = f32(float(_dot(ray1, ray2)) / (_norm(ray1) * _norm(ray2)))
    cs = f32(cos_rays + f32(1)); cs1 = cs; cs2 = cs
    if st1:
        cs1 = _cos_stereo(mb1, o1["depth"])
    elif st2:
        cs2 = _cos_stereo(mb2, o2["depth"])
    cs = min(cs1, cs2)
    tr.cmp("rays_lt_stereo", cos_rays, cs, False); tr.cmp("rays_gt_0", cos_rays, 0.0, False)
    if not (st1 or st2):
        tr.cmp("rays_lt_0.9998", cos_rays, 0.9998, False)
    if cos_rays < cs and cos_rays > 0 and (st1 or st2 or float(cos_rays) < 0.9998):
        A = np.zeros((4, 4), f32)
        for c in range(4):
            A[0, c] = f32(f32(xn1[0] * T1[2, c]) - T1[0, c]); A[1, c] = f32(f32(xn1[1] * T1[2, c]) - T1[1, c])
            A[2, c] = f32(f32(xn2[0] * T2[2, c]) - T2[0, c]); A[3, c] = f32(f32(xn2[1] * T2[2, c]) - T2[1, c])
        _, s, vt = np.linalg.svd(A.astype(np.float64))
        xh = vt[3]
        out.update(A=A, xh64=xh, sigma=s)
        xh32 = xh.astype(f32)
        tr.cmp("w_ne_0", abs(xh32[3]), 0.0, False)
        if xh32[3] == 0:
            out["reason"] = W_ZERO
            return out
        x3d = [f32(xh32[i] / xh32[3]) for i in range(3)]
        how = OK_TRI
    elif st1 and cs1 < cs2:
        tr.cmp("stereo1_lt_stereo2", cs1, cs2, False)
        x3d = _unproject_stereo(K1, T1, ow1, o1["kx"], o1["ky"], o1["depth"]); how = OK_ST1
    elif st2 and cs2 < cs1:
        tr.cmp("stereo2_lt_stereo1", cs2, cs1, False)
        x3d = _unproject_stereo(K2, T2, ow2, o2["kx"], o2["ky"], o2["depth"]); how = OK_ST2
    else:
        out["reason"] = LOW_PARALLAX
        return out
    out["x3d"] = np.array(x3d, f32); out["how"] = how
    z1 = f32(_dot(T1[2][:3], x3d) + T1[2][3])
    tr.cmp("z1_gt_0", z1, 0.0, True)
    if z1 <= 0:
        out["reason"] = BEHIND_1
        return out
    z2 = f32(_dot(T2[2][:3], x3d) + T2[2][3])
    tr.cmp("z2_gt_0", z2, 0.0, True)
    if z2 <= 0:
        out["reason"] = BEHIND_2
        return out
    if _reproj(tr, "1", K1, T1, o1, st1, mbf1, f32(ls1[o1["octave"]]), x3d, z1):
        out["reason"] = CHI2_1
        return out
    if _reproj(tr, "2", K2, T2, o2, st2, mbf1, f32(ls2[o2["octave"]]), x3d, z2):       # :861: KeyFrame 1's mbf
        out["reason"] = CHI2_2
        return out
    d1 = f32(_norm([f32(x3d[i] - f32(ow1[i])) for i in range(3)])); d2 = f32(_norm([f32(x3d[i] - f32(ow2[i])) for i in range(3)]))
    tr.cmp("dist1_ne_0", d1, 0.0, True); tr.cmp("dist2_ne_0", d2, 0.0, True)
    if d1 == 0 or d2 == 0:
        out["reason"] = DIST_ZERO
        return out
    if th_far > 0:
        tr.cmp("dist1_lt_far", d1, f32(th_far), True); tr.cmp("dist2_lt_far", d2, f32(th_far), True)
        if d1 >= f32(th_far) or d2 >= f32(th_far):
            out["reason"] = FAR
            return out
    rd = f32(d2 / d1); ro = f32(f32(sf1[o1["octave"]]) / f32(sf2[o2["octave"]])); rf = f32(ratio_factor)
    tr.cmp("scale_lo", f32(rd * rf), ro, True); tr.cmp("scale_hi", rd, f32(ro * rf), True)
    if f32(rd * rf) < ro or rd > f32(ro * rf):
        out["reason"] = SCALE
        return out
    out["reason"] = how
    return out


def obs(pool, row, i):
    kp = pool["kps_un"][row, i]; k = kp if pool.get("kps") is None else pool["kps"][row, i]
    return {"ux": kp["x"], "uy": kp["y"], "kx": k["x"], "ky": k["y"], "octave": int(kp["octave"]),
            "uright": -1.0 if pool.get("uright") is None else pool["uright"][row, i], "depth": -1.0 if pool.get("depth") is None else pool["depth"][row, i]}


def read_case(c):
    """-> dict of won_pair, won_idx2 [ngroups][cap1], x3d [ngroups][cap1][3], reason [npairs][cap1], ncreated [npairs], order [ngroups][cap1],
    ntotal [ngroups] and matches: {(pair, idx1): read_match's dict} for every match that was tried."""
    p1, p2 = c["pool1"], c["pool2"]
    gs = np.asarray(c["group_start"]); ng = len(gs) - 1
    m12 = np.asarray(c["matches12"]); npairs, cap1 = m12.shape
    r = {"won_pair": np.full((ng, cap1), -1, np.int32), "won_idx2": np.full((ng, cap1), -1, np.int32), "x3d": np.zeros((ng, cap1, 3), f32),
         "reason": np.full((npairs, cap1), NO_MATCH, np.uint8), "ncreated": np.zeros(npairs, np.int32), "order": np.full((ng, cap1), -1, np.int32),
         "ntotal": np.zeros(ng, np.int32), "matches": {}}
    rows1, rows2 = len(p1["counts"]), len(p2["counts"])
    for g in range(ng):
        pairs = range(int(gs[g]), int(gs[g + 1]))
        if len(pairs) == 0:
            continue
        r1 = int(c["row1"][pairs[0]])
        if any(int(c["row1"][p]) != r1 for p in pairs):
            r["reason"][pairs[0]:pairs[-1] + 1] = MIXED
            continue
        if not 0 <= r1 < rows1:
            continue
        n1 = min(max(int(p1["counts"][r1]), 0), cap1)
        has_mp = np.zeros(cap1, bool)                      # the current KeyFrame's new MapPoints, as AddMapPoint leaves them
        for p in pairs:
            r2 = int(c["row2"][p])
            if not 0 <= r2 < rows2:
                continue
            n2 = min(max(int(p2["counts"][r2]), 0), p2["kps_un"].shape[1])
            for i1 in range(n1):                           # ascending idx1: the order vMatchedPairs is built in
                i2 = int(m12[p, i1])
                if not 0 <= i2 < n2:
                    continue
                if has_mp[i1]:
                    r["reason"][p, i1] = TAKEN
                    continue
                m = read_match(c["k1"], c["k2"], c["mb1"], c["mbf1"], c["mb2"], p1["tcw"][r1], p1["ow"][r1], p2["tcw"][r2], p2["ow"][r2],
                               obs(p1, r1, i1), obs(p2, r2, i2), c["sf1"], c["ls1"], c["sf2"], c["ls2"], c["ratio_factor"], c["th_far"])
                r["matches"][(p, i1)] = m
                r["reason"][p, i1] = m["reason"]
                if m["reason"] <= OK_ST2:
                    has_mp[i1] = True
                    r["won_pair"][g, i1] = p; r["won_idx2"][g, i1] = i2; r["x3d"][g, i1] = m["x3d"]
                    r["order"][g, r["ntotal"][g]] = i1; r["ntotal"][g] += 1; r["ncreated"][p] += 1
    return r


def gates64(m_ctx, x3d):
    """The decisions after x3D, evaluated in float64 at a given x3D: a tuple of booleans in the order of the text.  Used to ask whether a
    perturbation of x3D of the tolerance's size could flip one (tests/triangulate_results.py)."""
    K1, K2, mbf1, T1, ow1, T2, ow2, o1, o2, sig1, sig2, ro, rf, th_far = m_ctx
    x = np.asarray(x3d, np.float64)
    out = []
    zs = []
    for T in (T1, T2):
        zs.append(float(T[2, :3] @ x + T[2, 3]))
    out += [zs[0] <= 0, zs[1] <= 0]
    for K, T, o, sig, z in ((K1, T1, o1, sig1, zs[0]), (K2, T2, o2, sig2, zs[1])):
        z = z if z != 0 else 1e-300
        u = K[0] * float(T[0, :3] @ x + T[0, 3]) / z + K[2]; v = K[1] * float(T[1, :3] @ x + T[1, 3]) / z + K[3]
        e2 = (u - o["ux"]) ** 2 + (v - o["uy"]) ** 2
        if o["uright"] >= 0:
            e2 += (u - mbf1 / z - o["uright"]) ** 2
            out.append(e2 > 7.8 * sig)
        else:
            out.append(e2 > 5.991 * sig)
    d1 = float(np.linalg.norm(x - ow1)); d2 = float(np.linalg.norm(x - ow2))
    out += [d1 == 0 or d2 == 0, th_far > 0 and (d1 >= th_far or d2 >= th_far)]
    rd = d2 / d1 if d1 else float("inf")
    out += [rd * rf < ro, rd > ro * rf]
    return tuple(bool(b) for b in out)
