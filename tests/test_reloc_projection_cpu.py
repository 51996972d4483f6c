"""The numpy restatement of M5 relocalisation SearchByProjection's projection and gates (reloc_project_np) against the facade's own
expressions compiled with g++ on facade/cvcompat.h (tests/reloc_projection.cpp), bit for bit.  tests/test_gpu_reloc_batch.py checks
orbm_search_by_projection_kf_batch_async against the same restatement.  Host-only: no GPU.

Unlike M4 and Fuse, M5 has no depth test (a point behind the camera whose projection lands in the image passes) and its bounds are
closed (u == maxX, v == maxY pass).  PredictScale: the restatement evaluates log(ratio) in double and rounds it to float, as k_frustum
and the batched searches do; the reference's logf is within one ulp of that, so the predicted level can differ only where
log(ratio) / logScaleFactor lies within an ulp of an integer.  Cases within 1e-4 of an integer are left out of the level comparison
(near_integer_level)."""
import os
import subprocess

import numpy as np

from test_fuse_projection_cpu import F32, F64, _dot3, _dsum3, camera_centre_np, edge_points, near_integer_level, random_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reloc_project_np(tcw, ow, pw, min_dist, max_dist, valid, k, bounds, log_sf, nlevels):
    """tcw [P][12] (row-major 3x4 [Rcw | tcw]), ow [P][3]; pw [P or 1][Q][3], min_dist / max_dist [P or 1][Q] (mfMinDistance /
    mfMaxDistance), valid [P][Q] the caller-side tests; k = (fx, fy, cx, cy), bounds = (minX, maxX, minY, maxY).
    Returns ok [P][Q] uint8 (every gate passed), u, v [P][Q] float32 (0 where not ok) and level [P][Q] int32 (-1 where not ok)."""
    T = np.asarray(tcw, F32).reshape(-1, 3, 4)
    O = np.asarray(ow, F32).reshape(-1, 3)[:, None, :]
    X = np.asarray(pw, F32)
    mn = np.asarray(min_dist, F32); mx = np.asarray(max_dist, F32)
    fx, fy, cx, cy = (F32(a) for a in k)
    minX, maxX, minY, maxY = (F32(a) for a in bounds)
    log_sf = F32(log_sf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xc, yc, zc = ((_dot3(T[:, None, r, :3], X) + T[:, None, r, 3]).astype(F32) for r in range(3))
        u = ((fx * xc) / zc + cx).astype(F32)
        v = ((fy * yc) / zc + cy).astype(F32)
        PO = (X - O).astype(F32)
        dist = np.sqrt(_dsum3(PO, PO)).astype(F32)
        ok = np.asarray(valid) != 0
        ok &= ~((u < minX) | (u > maxX)) & ~((v < minY) | (v > maxY))
        ok &= ~((dist < F32(0.8) * mn) | (dist > F32(1.2) * mx))
        ratio = (mx / dist).astype(F32)
        lg = np.log(ratio.astype(F64)).astype(F32)
        ns = np.ceil((lg / log_sf).astype(F32))
        ns = np.where(np.isfinite(ns), ns, 0)
    ns = np.clip(ns, 0, nlevels - 1).astype(np.int32)
    z = F32(0)
    return (ok.astype(np.uint8), np.where(ok, u, z).astype(F32), np.where(ok, v, z).astype(F32), np.where(ok, ns, -1).astype(np.int32))


def behind_points(rng, tcw, k, bounds, n):
    """n world points BEHIND the camera of pose tcw (z in [-12, -0.5]) whose projection lands inside the bounds (the mirrored frustum)."""
    T = np.asarray(tcw, F64).reshape(3, 4)
    fx, fy, cx, cy = k
    uu = rng.uniform(bounds[0] + 1, bounds[1] - 1, n); vv = rng.uniform(bounds[2] + 1, bounds[3] - 1, n)
    z = -rng.uniform(0.5, 12, n)
    pc = np.stack([(uu - cx) * z / fx, (vv - cy) * z / fy, z], 1)
    return ((pc - T[:, 3]) @ T[:, :3]).astype(F32)                            # R^T (pc - t)


def reloc_cases(rng, n, k, bounds, nlev=8):
    """Random poses; points in front of / behind / beside the camera; distance limits around the point's distance; then the exact
    edges: a tenth of the cases project exactly onto a bound (identity pose), a tenth lie behind the camera but project into the image,
    and dist3D sits exactly at 0.8f * min or 1.2f * max for others.  Returns T, Ow, X, mn, mx, hit (the bound searches that landed)."""
    T = np.stack([random_pose(rng, ang=rng.choice([0.01, 0.5, 3.0]), trans=rng.choice([0.05, 0.5, 5.0])) for _ in range(n)])
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(-3, 15, n)], 1).astype(F32)
    X[::7] *= F32(40)
    edge = np.arange(0, n, 10)
    S_id = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    T[edge] = S_id
    Xe, hit, _ = edge_points(rng, S_id, k, bounds, len(edge))
    X[edge] = Xe
    beh = np.arange(5, n, 10)
    for i in beh:
        X[i] = behind_points(rng, T[i], k, bounds, 1)[0]
    Ow = camera_centre_np(T)
    Tm = T.reshape(n, 3, 4)
    zc = np.stack([(_dot3(Tm[i, 2, :3], X[i]) + Tm[i, 2, 3]) for i in range(n)]).astype(F32)
    X[zc == 0, 2] += F32(0.25)                                                     # z == 0 exactly is outside the contract
    PO = (X - Ow).astype(F32)
    d = np.sqrt(_dsum3(PO, PO)).astype(F32)
    wide = 1.2 ** (nlev - 8)                                                       # deeper pyramids: wider distance ranges
    mx = (d * rng.uniform(0.7, 6.0 * wide, n)).astype(F32)
    mn = (mx / F32(2.0736 * 1.2 ** 4 * wide)).astype(F32)
    mn[::11] = (d[::11] * F32(1.3)).astype(F32)                                    # too near
    for sel, at_max in ((np.arange(1, n, 13), False), (np.arange(2, n, 13), True)):
        for i in sel:
            c = d[i] / F32(1.2 if at_max else 0.8)
            for _ in range(8):
                prod = (F32(1.2) * c) if at_max else (F32(0.8) * c)
                if prod == d[i]:
                    break
                c = np.nextafter(c, F32(np.inf) if prod < d[i] else F32(-np.inf))
            if at_max:
                mx[i] = c
            else:
                mn[i] = c
    return T, Ow, X, mn, mx, hit, beh


def test_restatement_equals_facade_expressions(tmp_path):
    exe = str(tmp_path / "reloc_projection")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "reloc_projection.cpp")])
    k = (458.654, 457.296, 367.215, 248.375)
    bounds = (0.0, 752.0, 0.0, 480.0)
    n = 12000
    for nlev, seed in ((8, 31), (12, 32)):
        log_sf = float(np.log(F32(1.2)).astype(F32))
        rng = np.random.default_rng(seed)
        T, Ow, X, mn, mx, hit, beh = reloc_cases(rng, n, k, bounds, nlev)
        assert hit.mean() > 0.8
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        body = np.concatenate([T, X, mn[:, None], mx[:, None]], 1).astype(F32)
        np.concatenate([np.asarray(list(k) + list(bounds) + [log_sf, nlev, n], F32), body.reshape(-1)]).tofile(fin)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "reloc_projection ok" in r.stdout, r.stdout + r.stderr
        out = np.fromfile(fout, F32).reshape(n, 4)
        ok, u, v, lvl = (a[:, 0] for a in reloc_project_np(T, Ow, X[:, None, :], mn[:, None], mx[:, None], np.ones((n, 1), np.uint8),
                                                          k, bounds, log_sf, nlev))
        assert np.array_equal(out[:, 0].astype(np.uint8), ok)
        for col, a in ((1, u), (2, v)):
            assert np.array_equal(out[:, col].view(np.uint32), a.view(np.uint32)), col
        near = near_integer_level(X[:, None, :], mn[:, None], mx[:, None], T, Ow, log_sf, nlev)[:, 0]
        assert near.sum() < 0.01 * n
        assert np.array_equal(out[~near, 3].astype(np.int32), lvl[~near])
        # every branch is reached: gates reject some cases, many pass, both end levels occur
        assert 0.1 * n < ok.sum() < 0.9 * n
        assert (lvl == 0).sum() > 50 and (lvl == nlev - 1).sum() > 20
        # closed bounds: all four exact edges accepted
        for b, a in ((0, u), (1, u), (2, v), (3, v)):
            assert np.any(ok & (a == F32(bounds[b]))), b
        # no depth test: points behind the camera that project into the image pass
        Tm = T.reshape(n, 3, 4)
        zc = np.stack([(_dot3(Tm[i, 2, :3], X[i]) + Tm[i, 2, 3]) for i in range(n)]).astype(F32)
        assert (ok[beh] & (zc[beh] < 0)).sum() > 0.3 * len(beh)
        PO = (X - Ow).astype(F32); d = np.sqrt(_dsum3(PO, PO)).astype(F32)
        assert np.any(ok & (d == F32(0.8) * mn)) and np.any(ok & (d == F32(1.2) * mx))
