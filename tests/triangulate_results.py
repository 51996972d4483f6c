"""What the CreateNewMapPoints tests hold an implementation to, and the one measured number behind it.

The tolerance.  On the triangulated branch the sign-aligned unit x3D_h may differ from the reading's float64 null vector by at most
C * eps32 * sigma1 / (sigma3 - sigma4), the sigma being the float64 singular values of the match's A.  C is not chosen: it is 4 x the
largest such ratio an INDEPENDENT float32 SVD shows (np.linalg.svd on the float32 A, LAPACK sgesdd) over every triangulated match of
the committed cases -- the factor 4 is the one the pose-optimisation header test puts over its measured spread.
MEASURED_RATIO was measured on the CPU with measure_float32_svd() below and is checked again by tests/test_triangulate_header_cpu.py.
The header (csrc/orbm_triangulate.h, Jacobi carried in double, rounded once) measured 0.1007 on the same matches: like LAPACK's, its
error is the final rounding of the unit vector to float32.  With float32 columns the same Jacobi measured 0.78 and missed C."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_reading_triangulate as sr   # noqa: E402
import triangulate_cases as tc            # noqa: E402

EPS32 = 2.0 ** -23
MEASURED_RATIO = 0.1007        # np.linalg.svd(float32 A) against the float64 null vector, largest over the committed cases (0.10066)
C = 4 * MEASURED_RATIO         # 0.4028
FLAG_KEYS = ("reason", "won_pair", "won_idx2", "ncreated", "order", "ntotal")

_cache = {}


def cases():
    """The committed scenes, the GPU test's shapes among them, built once."""
    if "cases" not in _cache:
        _cache["cases"] = dict(tc.cases(), **tc.gpu_cases())
    return _cache["cases"]


def reading(name):
    """The second reading of a committed case, computed once and shared."""
    key = ("reading", name)
    if key not in _cache:
        _cache[key] = sr.read_case(cases()[name])
    return _cache[key]


def bound(sigma):
    return C * EPS32 * sigma[0] / (sigma[2] - sigma[3])


def unit_distance(xh, xh64):
    """|| sign-aligned unit xh - xh64 ||"""
    a = np.asarray(xh, np.float64)
    n = np.linalg.norm(a)
    a = a / n if n > 0 else a
    if a @ xh64 < 0:
        a = -a
    return float(np.linalg.norm(a - xh64))


def measure_float32_svd(all_cases=None):
    """The largest unit_distance / (eps32 sigma1 / (sigma3 - sigma4)) of np.linalg.svd run on the float32 A."""
    worst = 0.0
    for name in (all_cases or cases()):
        for m in reading(name)["matches"].values():
            if "xh64" in m:
                vt = np.linalg.svd(m["A"])[2]
                s = m["sigma"]
                worst = max(worst, unit_distance(vt[3], m["xh64"]) / (EPS32 * s[0] / (s[2] - s[3])))
    return worst


def _ctx(c, p, i1, i2):
    g1, g2 = int(c["row1"][p]), int(c["row2"][p])
    o1, o2 = sr.obs(c["pool1"], g1, i1), sr.obs(c["pool2"], g2, i2)
    f = lambda o: {k: float(v) for k, v in o.items()}
    T1 = c["pool1"]["tcw"][g1].reshape(3, 4).astype(np.float64); T2 = c["pool2"]["tcw"][g2].reshape(3, 4).astype(np.float64)
    return (c["k1"].astype(np.float64), c["k2"].astype(np.float64), float(c["mbf1"]), T1, c["pool1"]["ow"][g1].astype(np.float64), T2,
            c["pool2"]["ow"][g2].astype(np.float64), f(o1), f(o2), float(c["ls1"][o1["octave"]]), float(c["ls2"][o2["octave"]]),
            float(c["sf1"][o1["octave"]]) / float(c["sf2"][o2["octave"]]), float(c["ratio_factor"]), float(c["th_far"]))


def _effective(d):
    """The decisions up to and including the first exit taken."""
    out = []
    for b in d:
        out.append(b)
        if b:
            break
    return tuple(out)


def undecided(c, r):
    """[(pair, idx1, why)] for the matches of reading r of case c whose outcome the tolerance could move: a comparison before x3D whose
    sides are within 4 float32 ulps, a w within twice the bound of zero, or a gate after x3D that changes somewhere in the box x3D +-
    twice what the bound on x3D_h can move it.  A committed case has none."""
    bad = []
    for (p, i1), m in r["matches"].items():
        for name, lhs, rhs, after in m["trace"]:
            if not after and name != "w_ne_0" and abs(lhs - rhs) <= 4 * EPS32 * max(abs(lhs), abs(rhs), 2.0 ** -126):
                bad.append((p, i1, name))
        if "xh64" not in m or m["reason"] == sr.W_ZERO:
            if "xh64" in m:
                bad.append((p, i1, "w_zero"))
            continue
        b = bound(m["sigma"]); xh = m["xh64"]
        if abs(xh[3]) <= 2 * b:
            bad.append((p, i1, "w_ne_0")); continue
        x = xh[:3] / xh[3]
        dx = 2 * b * (1 + np.abs(x).max()) / abs(xh[3])
        ctx = _ctx(c, p, i1, int(c["matches12"][p, i1]))
        centre = _effective(sr.gates64(ctx, x))
        want = m["reason"] not in (sr.OK_TRI, sr.OK_ST1, sr.OK_ST2)
        if any(centre) != want:
            bad.append((p, i1, "float64 gates disagree with the float32 reading")); continue
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    if _effective(sr.gates64(ctx, x + dx * np.array([sx, sy, sz]))) != centre:
                        bad.append((p, i1, "a gate flips inside the box")); break
    return bad


def check_against_reading(c, r, got, who, xh=None):
    """Flags, winners, counts and order equal the reading exactly (no match is excluded); on the unproject branches x3d equals it bit for
    bit; on the triangulated branch the unit x3D_h (where `xh` [npairs][cap1][4] is given) lies within the bound and x3d is its float32
    quotient.  Returns the largest unit distance / bound seen."""
    for key in FLAG_KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(r[key]).astype(np.int64)), "%s: %s differs from the reading" % (who, key)
    worst = 0.0
    ng, cap1 = r["won_pair"].shape
    for g in range(ng):
        for i1 in range(cap1):
            p = int(r["won_pair"][g, i1])
            if p < 0:
                assert not np.any(got["x3d"][g, i1]), "%s: x3d is not zero where nothing was created" % who
                continue
            m = r["matches"][(p, i1)]
            if m["reason"] != sr.OK_TRI:
                assert got["x3d"][g, i1].tobytes() == m["x3d"].tobytes(), "%s: x3d of an unprojected point differs from the reading's bits" % who
            else:
                rel = np.abs(got["x3d"][g, i1].astype(np.float64) - m["x3d"]).max() / (1 + np.abs(m["x3d"]).max())
                b = bound(m["sigma"])
                assert rel <= 4 * b / abs(m["xh64"][3]) + 4 * EPS32, "%s: x3d off by %.3g relative at pair %d idx1 %d" % (who, rel, p, i1)
                if xh is not None:
                    v = xh[p, i1]
                    d = unit_distance(v, m["xh64"])
                    worst = max(worst, d / b)
                    assert d <= b, "%s: x3D_h off by %.3g, bound %.3g (pair %d idx1 %d)" % (who, d, b, p, i1)
                    q = np.array([np.float32(v[k]) / np.float32(v[3]) for k in range(3)], np.float32)
                    assert q.tobytes() == got["x3d"][g, i1].tobytes()
    return worst
