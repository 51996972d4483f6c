"""The numpy restatement of M13 Fuse's projection and geometric gates (fuse_project_np, sim3_pose_np) against the facade's own
expressions compiled with g++ on facade/cvcompat.h (tests/fuse_projection.cpp), bit for bit, for the pose variant and the Sim3 variant.
tests/test_gpu_fuse_batch.py checks orbm_fuse_batch_async against the same restatement.  Host-only: no GPU.

PredictScale: the restatement evaluates log(ratio) in double and rounds it to float, as k_frustum and the batched Fuse do; the reference's
logf is within one ulp of that, so the predicted level can differ only where log(ratio) / logScaleFactor lies within an ulp of an integer.
Cases within 1e-4 of an integer are left out of the level comparison (near_integer_level)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _dot3(r, x):
    """cvcompat's product row: a double sum from 0 in k order of exact double products, rounded once to float."""
    p = r.astype(F64) * x.astype(F64)
    return (((F64(0) + p[..., 0]) + p[..., 1]) + p[..., 2]).astype(F32)


def _dsum3(a, b):
    """A double sum from 0 of double products (cv::Mat::dot, the square of cv::norm)."""
    p = a.astype(F64) * b.astype(F64)
    return ((F64(0) + p[..., 0]) + p[..., 1]) + p[..., 2]


def sim3_pose_np(scw):
    """The Sim3 variant's pose as the facade derives it (ORBmatcher.cc:2062-2066 on cvcompat): scw [P][12] row-major 3x4 [sR | t].
    Returns tcw [P][12] ([Rcw | tcw] with Rcw = sRcw / scw, tcw = t / scw) and ow [P][3] = -Rcw^T tcw."""
    S = np.asarray(scw, F32).reshape(-1, 3, 4)
    s = np.sqrt(_dsum3(S[:, 0, :3], S[:, 0, :3])).astype(F32)                    # sqrt(sRcw.row(0).dot(sRcw.row(0))) -> float
    inv = (1.0 / s.astype(F64)).astype(F32)                                       # Mat / s multiplies by (float)(1.0 / s)
    T = (S * inv[:, None, None]).astype(F32)
    ow = np.stack([_dot3(-T[:, :, r], T[:, :, 3]) for r in range(3)], 1)          # -Rcw.t() * tcw
    return T.reshape(-1, 12), ow


def near_integer_level(pw, min_dist, max_dist, tcw, ow, log_sf, nlevels, tol=1e-4):
    """True where log(mfMaxDistance / dist3D) / logScaleFactor lies within tol of an integer m in [0, nlevels - 2] (the documented
    PredictScale caveat; at other integers both sides of m clamp to the same level)."""
    X = np.asarray(pw, F32)
    O = np.asarray(ow, F32).reshape(-1, 3)[:, None, :]
    d = np.sqrt(_dsum3(X - O, X - O)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.log((np.asarray(max_dist, F32) / d).astype(F64)) / F64(log_sf)
    m = np.rint(t)
    return (np.abs(t - m) < tol) & (m >= 0) & (m <= nlevels - 2)


def fuse_project_np(tcw, ow, pw, normal, min_dist, max_dist, valid, k, bounds, bf, log_sf, nlevels):
    """tcw [P][12] (row-major 3x4 [Rcw | tcw]), ow [P][3]; pw / normal [P or 1][Q][3], min_dist / max_dist [P or 1][Q] (mfMinDistance /
    mfMaxDistance), valid [P][Q] the caller-side tests; k = (fx, fy, cx, cy), bounds = (minX, maxX, minY, maxY).
    Returns ok [P][Q] uint8 (every gate passed), u, v, ur [P][Q] float32 (0 where not ok) and level [P][Q] int32 (-1 where not ok)."""
    T = np.asarray(tcw, F32).reshape(-1, 3, 4)
    O = np.asarray(ow, F32).reshape(-1, 3)[:, None, :]
    X = np.asarray(pw, F32); N = np.asarray(normal, F32)
    mn = np.asarray(min_dist, F32); mx = np.asarray(max_dist, F32)
    fx, fy, cx, cy = (F32(a) for a in k)
    minX, maxX, minY, maxY = (F32(a) for a in bounds)
    bf, log_sf = F32(bf), F32(log_sf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xc, yc, zc = ((_dot3(T[:, None, r, :3], X) + T[:, None, r, 3]).astype(F32) for r in range(3))
        invz = (F32(1) / zc).astype(F32)
        u = ((fx * xc) / zc + cx).astype(F32)
        v = ((fy * yc) / zc + cy).astype(F32)
        ur = (u - bf * invz).astype(F32)
        PO = (X - O).astype(F32)
        dist = np.sqrt(_dsum3(PO, PO)).astype(F32)
        ok = (np.asarray(valid) != 0) & ~(zc < F32(0))
        ok &= (u >= minX) & (u < maxX) & (v >= minY) & (v < maxY)
        ok &= ~((dist < F32(0.8) * mn) | (dist > F32(1.2) * mx))
        ok &= ~(_dsum3(PO, N) < 0.5 * dist.astype(F64))
        ratio = (mx / dist).astype(F32)
        lg = np.log(ratio.astype(F64)).astype(F32)
        ns = np.ceil((lg / log_sf).astype(F32))
        ns = np.where(np.isfinite(ns), ns, 0)
    ns = np.clip(ns, 0, nlevels - 1).astype(np.int32)
    z = F32(0)
    return (ok.astype(np.uint8), np.where(ok, u, z).astype(F32), np.where(ok, v, z).astype(F32), np.where(ok, ur, z).astype(F32),
            np.where(ok, ns, -1).astype(np.int32))


def random_pose(rng, ang=0.05, trans=0.3):
    a = rng.uniform(-ang, ang, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = rng.uniform(-trans, trans, 3)
    return np.concatenate([R, t[:, None]], 1).astype(F32).reshape(12)


def camera_centre_np(tcw):
    """GetCameraCenter of a [Rcw | tcw] pose: -Rcw^T tcw by cvcompat's product rule."""
    T = np.asarray(tcw, F32).reshape(-1, 3, 4)
    return np.stack([_dot3(-T[:, :, r], T[:, :, 3]) for r in range(3)], 1)


def edge_points(rng, tcw, k, bounds, n):
    """n world points whose projection through pose tcw lands EXACTLY on a bound: u == minX, u == maxX, v == minY, v == maxY in turn
    (found by stepping the point's x / y coordinate in camera ulps through the restatement's own arithmetic); hit is False where the search ends without one."""
    T = np.asarray(tcw, F32).reshape(3, 4)
    fx, fy, cx, cy = (F32(a) for a in k)
    which = np.arange(n) % 4
    target = np.array(bounds, F32)[which]
    z = rng.uniform(1, 10, n).astype(F32)
    out = np.zeros((n, 3), F32); hit = np.zeros(n, bool)
    Rt = T[:, :3].astype(F64).T
    for i in range(n):
        ax = 0 if which[i] < 2 else 1
        f, c = (fx, cx) if ax == 0 else (fy, cy)
        pc = np.array([0.0, 0.0, float(z[i])]); pc[ax] = float((target[i] - c) * z[i] / f)
        pc[1 - ax] = float(rng.uniform(-0.2, 0.2) * z[i])
        Xw = (Rt @ (pc - T[:, 3].astype(F64))).astype(F32)
        for _ in range(4000):
            xc = (_dot3(T[ax, :3], Xw) + T[ax, 3]).astype(F32)
            zc = (_dot3(T[2, :3], Xw) + T[2, 3]).astype(F32)
            w = ((f * xc) / zc + c).astype(F32)
            if w == target[i]:
                hit[i] = True
                break
            # move the world point along the camera axis direction that changes w, by one ulp of its largest component
            j = int(np.argmax(np.abs(T[ax, :3])))
            step = np.sign(T[ax, j]) * (1 if w < target[i] else -1)
            Xw[j] = np.nextafter(Xw[j], F32(np.inf) if step > 0 else F32(-np.inf))
        out[i] = Xw
    return out, hit, which


def _run(exe, tmp_path, hdr, S, Ow, X, N, mn, mx):
    n = len(S)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    body = np.concatenate([S, Ow, X, N, mn[:, None], mx[:, None]], 1).astype(F32)
    np.concatenate([np.asarray(hdr, F32), body.reshape(-1)]).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuse_projection ok" in r.stdout, r.stdout + r.stderr
    return np.fromfile(fout, F32).reshape(n, 20)


def _cases(rng, n, k, bounds, sim3):
    """Random poses (or Sim3 transforms with scale != 1), points in front of / behind / beside the camera, distance limits around the
    point's distance, normals at every angle to the viewing ray -- then the exact edges: projection on each bound, dist3D exactly at
    0.8f * min and 1.2f * max, PO . normal at the 0.5 dist3D boundary, levels 0 and nlevels - 1."""
    S = np.stack([random_pose(rng, ang=rng.choice([0.01, 0.5, 3.0]), trans=rng.choice([0.05, 0.5, 5.0])) for _ in range(n)])
    if sim3:
        s = rng.choice([0.25, 0.9, 1.0, 1.7, 6.0], n).astype(F32)
        S = S.reshape(n, 3, 4).copy(); S[:, :, :3] *= s[:, None, None]; S[:, :, 3] *= rng.uniform(0.5, 3, (n, 1)).astype(F32)
        S = S.reshape(n, 12).astype(F32)
        T, Ow = sim3_pose_np(S)
    else:
        T = S
        Ow = camera_centre_np(T)
        Ow[::9] += rng.normal(0, 1e-3, (len(Ow[::9]), 3)).astype(F32)            # the pose variant reads Ow as given
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(-3, 15, n)], 1).astype(F32)
    X[::7] *= F32(40)
    # exact bound hits for a tenth of the cases (identity pose)
    edge = np.arange(0, n, 10)
    S_id = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    if sim3:
        S[edge] = S_id
        T[edge], Ow[edge] = sim3_pose_np(S[edge])
    else:
        S[edge] = S_id; T[edge] = S_id; Ow[edge] = camera_centre_np(T[edge])
    Xe, hit, _ = edge_points(rng, S_id, k, bounds, len(edge))
    X[edge] = Xe
    X[X[:, 2] == 0, 2] = F32(0.5)                                                  # z == 0 exactly is outside the contract
    PO = (X - Ow).astype(F32)
    d = np.sqrt(_dsum3(PO, PO)).astype(F32)
    mx = (d * rng.uniform(0.7, 6.0, n)).astype(F32)
    mn = (mx / F32(2.0736 * 1.2 ** 4)).astype(F32)
    mn[::11] = (d[::11] * F32(1.3)).astype(F32)                                     # too near
    # dist3D exactly at 0.8f * min / 1.2f * max where a float min / max gives it
    for sel, at_max in ((np.arange(1, n, 13), False), (np.arange(2, n, 13), True)):
        for i in sel:
            base = d[i] / F32(1.2 if at_max else 0.8)
            c = base
            for _ in range(8):
                prod = (F32(1.2) * c) if at_max else (F32(0.8) * c)
                if prod == d[i]:
                    break
                c = np.nextafter(c, F32(np.inf) if prod < d[i] else F32(-np.inf))
            if at_max:
                mx[i] = c
            else:
                mn[i] = c
    # normals: random unit vectors, the viewing direction, and the 60 degree boundary (PO . n == 0.5 dist3D in exact arithmetic)
    Nn = rng.normal(0, 1, (n, 3)); Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    view = PO.astype(F64) / np.maximum(d.astype(F64), 1e-30)[:, None]
    Nn[::3] = view[::3]
    perp = np.cross(view, rng.normal(0, 1, (n, 3))); perp /= np.maximum(np.linalg.norm(perp, axis=1, keepdims=True), 1e-30)
    b = np.arange(1, n, 3)
    Nn[b] = 0.5 * view[b] + np.sqrt(0.75) * perp[b] + rng.choice([-1e-7, 0.0, 1e-7], (len(b), 1)) * view[b]
    N = Nn.astype(F32)
    return S, T, Ow, X, N, mn, mx, hit


def test_restatement_equals_facade_expressions(tmp_path):
    exe = str(tmp_path / "fuse_projection")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "fuse_projection.cpp")])
    k = (458.654, 457.296, 367.215, 248.375)
    bounds = (0.0, 752.0, 0.0, 480.0)
    bf = 47.90639384423901
    nlev = 8
    log_sf = float(np.log(F32(1.2)).astype(F32))
    n = 12000
    for sim3 in (False, True):
        rng = np.random.default_rng(23 + sim3)
        S, T, Ow, X, N, mn, mx, hit = _cases(rng, n, k, bounds, sim3)
        assert hit.mean() > 0.8
        hdr = list(k) + list(bounds) + [bf, log_sf, nlev, float(sim3), n]
        out = _run(exe, tmp_path, hdr, S, Ow if not sim3 else np.zeros((n, 3), F32), X, N, mn, mx)
        if sim3:                                                                    # the pose the Sim3 search used
            assert np.array_equal(out[:, 5:14].view(np.uint32), T.reshape(n, 3, 4)[:, :, :3].reshape(n, 9).view(np.uint32))
            assert np.array_equal(out[:, 14:17].view(np.uint32), T.reshape(n, 3, 4)[:, :, 3].view(np.uint32))
            assert np.array_equal(out[:, 17:20].view(np.uint32), Ow.view(np.uint32))
        ok, u, v, ur, lvl = fuse_project_np(T, Ow, X[:, None, :], N[:, None, :], mn[:, None], mx[:, None], np.ones((n, 1), np.uint8),
                                            k, bounds, bf, log_sf, nlev)
        ok, u, v, ur, lvl = ok[:, 0], u[:, 0], v[:, 0], ur[:, 0], lvl[:, 0]
        assert np.array_equal(out[:, 0].astype(np.uint8), ok)
        for col, a in ((1, u), (2, v), (3, ur)):
            assert np.array_equal(out[:, col].view(np.uint32), a.view(np.uint32)), col
        near = near_integer_level(X[:, None, :], mn[:, None], mx[:, None], T, Ow, log_sf, nlev)[:, 0]
        keep = ~near
        assert near.sum() < 0.01 * n
        assert np.array_equal(out[keep, 4].astype(np.int32), lvl[keep])
        # every branch is reached: each gate rejects some cases, many pass, both end levels occur, the bounds are hit exactly
        assert 0.1 * n < ok.sum() < 0.9 * n
        assert (lvl == 0).sum() > 50 and (lvl == nlev - 1).sum() > 20
        on_min = ok & ((u == F32(bounds[0])) | (v == F32(bounds[2])))
        assert on_min.sum() > 20                                                    # u == minX / v == minY accepted
        assert not np.any(ok & ((u == F32(bounds[1])) | (v == F32(bounds[3]))))     # u == maxX / v == maxY rejected
        PO = (X - Ow).astype(F32); d = np.sqrt(_dsum3(PO, PO)).astype(F32)
        assert np.any(ok & (d == F32(0.8) * mn)) and np.any(ok & (d == F32(1.2) * mx))
        dot = _dsum3(PO, N); rel = (dot - 0.5 * d.astype(F64)) / np.maximum(d.astype(F64), 1e-30)
        assert np.any(ok & (np.abs(rel) < 1e-6)) and np.any(~ok & (np.abs(rel) < 1e-6) & (dot < 0.5 * d))
