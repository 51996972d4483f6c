"""The numpy restatement of M6's projection and geometric gates (sim3_project_np, both projection forms) against the facade's own
sim3_projection / sim3_gates lines compiled with g++ on facade/cvcompat.h (tests/sim3_projection.cpp), bit for bit.
tests/test_gpu_sim3_projection_batch.py checks orbm_search_by_projection_sim3_batch_async against the same restatement.  Host-only: no GPU.

proj_form 0 is mpCamera->project, u = fx * x / z + cx (ORBmatcher.cc:602); proj_form 1 the vpPointsKFs overload's invz = 1 / z,
u = fx * (x * invz) + cx (:724-729).  The PredictScale caveat of tests/test_fuse_projection_cpu.py holds here too (near_integer_level)."""
import os
import subprocess

import numpy as np

from test_fuse_projection_cpu import F32, F64, _cases, _dot3, _dsum3, near_integer_level, sim3_pose_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (458.654, 457.296, 367.215, 248.375)
BOUNDS = (0.0, 752.0, 0.0, 480.0)
NLEV = 8
LOG_SF = float(np.log(F32(1.2)).astype(F32))
S_ID = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)


def sim3_project_np(tcw, ow, pw, normal, min_dist, max_dist, valid, k, bounds, log_sf, nlevels, proj_form):
    """tcw [P][12] (row-major 3x4 [Rcw | tcw], the Sim3's rotation and translation divided by its scale), ow [P][3]; pw / normal
    [P][Q][3], min_dist / max_dist [P][Q], valid [P][Q] the caller-side tests.  Returns ok [P][Q] uint8, u, v [P][Q] float32 (0 where not
    ok) and level [P][Q] int32 (-1 where not ok)."""
    T = np.asarray(tcw, F32).reshape(-1, 3, 4)
    O = np.asarray(ow, F32).reshape(-1, 3)[:, None, :]
    X = np.asarray(pw, F32); N = np.asarray(normal, F32)
    mn = np.asarray(min_dist, F32); mx = np.asarray(max_dist, F32)
    fx, fy, cx, cy = (F32(a) for a in k)
    minX, maxX, minY, maxY = (F32(a) for a in bounds)
    log_sf = F32(log_sf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xc, yc, zc = ((_dot3(T[:, None, r, :3], X) + T[:, None, r, 3]).astype(F32) for r in range(3))
        if proj_form:
            invz = (F32(1) / zc).astype(F32)
            u = (fx * (xc * invz).astype(F32) + cx).astype(F32)
            v = (fy * (yc * invz).astype(F32) + cy).astype(F32)
        else:
            u = ((fx * xc) / zc + cx).astype(F32)
            v = ((fy * yc) / zc + cy).astype(F32)
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
    return ok.astype(np.uint8), np.where(ok, u, z).astype(F32), np.where(ok, v, z).astype(F32), np.where(ok, ns, -1).astype(np.int32)


def edge_points_form(rng, k, bounds, n, proj_form):
    """n camera-frame points (identity pose) whose projection in the given form lands EXACTLY on a bound (minX, maxX, minY, maxY in
    turn), found by stepping the coordinate in ulps through the restatement's own arithmetic; hit is False where the search fails."""
    f4 = [F32(a) for a in k]
    out = np.zeros((n, 3), F32); hit = np.zeros(n, bool); which = np.arange(n) % 4
    for i in range(n):
        ax = 0 if which[i] < 2 else 1
        f, c = (f4[0], f4[2]) if ax == 0 else (f4[1], f4[3])
        t = F32(bounds[which[i]])
        z = F32(rng.uniform(1, 10))
        x = F32((t - c) * z / f)
        for _ in range(4000):
            w = (f * x) / z + c if not proj_form else f * F32(x * F32(F32(1) / z)) + c
            w = F32(w)
            if w == t:
                hit[i] = True
                break
            x = np.nextafter(x, F32(np.inf) if w < t else F32(-np.inf))
        out[i, ax] = x; out[i, 1 - ax] = F32(rng.uniform(-0.2, 0.2) * z); out[i, 2] = z
    return out, hit, which


def forms_differ_point(k, nsearch=20000, seed=5):
    """Camera-frame points (identity pose) for which the two projection forms give different float u or v: searched on the CPU."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, nsearch), rng.uniform(-1.5, 1.5, nsearch), rng.uniform(2, 12, nsearch)], 1).astype(F32)
    one = np.ones((1, nsearch), np.uint8)
    big = np.full((1, nsearch), 1e9, F32)
    N = X / np.linalg.norm(X, axis=1, keepdims=True)
    a = sim3_project_np(S_ID[None], np.zeros((1, 3), F32), X[None], N[None].astype(F32), big * 0, big, one, k, BOUNDS, LOG_SF, NLEV, 0)
    b = sim3_project_np(S_ID[None], np.zeros((1, 3), F32), X[None], N[None].astype(F32), big * 0, big, one, k, BOUNDS, LOG_SF, NLEV, 1)
    d = (a[0][0] & b[0][0]).astype(bool) & ((a[1][0] != b[1][0]) | (a[2][0] != b[2][0]))
    return X[d]


def sim3_cases(rng, n, proj_form):
    """test_fuse_projection_cpu's Sim3 cases (random similarity transforms, points all round the camera, the distance limits and the 60
    degree boundary hit exactly), with this form's exact bound hits, z just either side of 0, and points where the forms differ."""
    S, T, Ow, X, N, mn, mx, _ = _cases(rng, n, K, BOUNDS, True)
    edge = np.arange(0, n, 10)
    Xe, hit, _ = edge_points_form(rng, K, BOUNDS, len(edge), proj_form)
    X[edge] = Xe                                                                   # _cases gave these the identity transform
    zs = np.arange(5, n, 10)                                                       # z just either side of 0 (z == 0 itself is outside the contract)
    S[zs] = S_ID; T[zs], Ow[zs] = sim3_pose_np(S[zs])
    X[zs, 2] = np.tile(np.array([1e-6, -1e-6, 1e-20, -1e-20, 1e-3, -1e-3], F32), len(zs) // 6 + 1)[:len(zs)]
    X[zs, :2] = 0
    df = forms_differ_point(K)
    sel = np.arange(3, n, 10)[:len(df)]
    S[sel] = S_ID; T[sel], Ow[sel] = sim3_pose_np(S[sel]); X[sel] = df[:len(sel)]
    for s in (edge, zs, sel):                                                      # wide limits, normal along the ray: only the case's gate decides
        PO = (X[s] - Ow[s]).astype(F32); d = np.sqrt(_dsum3(PO, PO)).astype(F32)
        mx[s] = d * F32(2); mn[s] = d / F32(4)
        N[s] = (PO / np.maximum(d, F32(1e-30))[:, None]).astype(F32)
    return S, T, Ow, X, N, mn, mx, hit, edge, zs, sel


def test_forms_differ_somewhere():
    """The searched set holds points where the two forms round differently; the first one is evaluated here in scalar float arithmetic."""
    df = forms_differ_point(K)
    assert len(df) > 10
    x = df[0]
    u0 = F32((F32(K[0]) * x[0]) / x[2] + F32(K[2])); u1 = F32(F32(K[0]) * F32(x[0] * F32(F32(1) / x[2])) + F32(K[2]))
    v0 = F32((F32(K[1]) * x[1]) / x[2] + F32(K[3])); v1 = F32(F32(K[1]) * F32(x[1] * F32(F32(1) / x[2])) + F32(K[3]))
    assert u0 != u1 or v0 != v1


def test_restatement_equals_facade_expressions(tmp_path):
    exe = str(tmp_path / "sim3_projection")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "sim3_projection.cpp")])
    n = 12000
    outs = {}
    for form in (0, 1):
        rng = np.random.default_rng(61)                                             # the same cases for both forms but the bound hits
        S, T, Ow, X, N, mn, mx, hit, edge, zs, sel = sim3_cases(rng, n, form)
        assert hit.mean() > 0.8
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        hdr = list(K) + list(BOUNDS) + [LOG_SF, NLEV, float(form == 0), n]
        body = np.concatenate([S, X, N, mn[:, None], mx[:, None]], 1).astype(F32)
        np.concatenate([np.asarray(hdr, F32), body.reshape(-1)]).tofile(fin)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "sim3_projection ok" in r.stdout, r.stdout + r.stderr
        out = np.fromfile(fout, F32).reshape(n, 19)
        assert np.array_equal(out[:, 4:13].view(np.uint32), T.reshape(n, 3, 4)[:, :, :3].reshape(n, 9).view(np.uint32))
        assert np.array_equal(out[:, 13:16].view(np.uint32), T.reshape(n, 3, 4)[:, :, 3].view(np.uint32))
        assert np.array_equal(out[:, 16:19].view(np.uint32), Ow.view(np.uint32))
        ok, u, v, lvl = (a[:, 0] for a in sim3_project_np(T, Ow, X[:, None, :], N[:, None, :], mn[:, None], mx[:, None], np.ones((n, 1), np.uint8),
                                                          K, BOUNDS, LOG_SF, NLEV, form))
        assert np.array_equal(out[:, 0].astype(np.uint8), ok)
        assert np.array_equal(out[:, 1].view(np.uint32), u.view(np.uint32)) and np.array_equal(out[:, 2].view(np.uint32), v.view(np.uint32))
        near = near_integer_level(X[:, None, :], mn[:, None], mx[:, None], T, Ow, LOG_SF, NLEV)[:, 0]
        assert near.sum() < 0.01 * n
        assert np.array_equal(out[~near, 3].astype(np.int32), lvl[~near])
        # every branch is reached
        assert 0.1 * n < ok.sum() < 0.9 * n
        assert (lvl == 0).sum() > 50 and (lvl == NLEV - 1).sum() > 20
        eh = edge[hit]
        on = np.zeros(n, bool); on[eh] = True
        assert (ok & on & ((u == F32(BOUNDS[0])) | (v == F32(BOUNDS[2])))).sum() > 20     # on minX / minY: accepted
        assert (on & ~ok).sum() > 20                                                      # on maxX / maxY: rejected
        assert not np.any(ok & ((u == F32(BOUNDS[1])) | (v == F32(BOUNDS[3]))))
        zc = X[zs, 2]
        assert np.all(ok[zs][zc > 0] == 1) and np.all(ok[zs][zc < 0] == 0) and (zc > 0).sum() > 100 and (zc < 0).sum() > 100
        PO = (X - Ow).astype(F32); d = np.sqrt(_dsum3(PO, PO)).astype(F32)
        assert np.any(ok.astype(bool) & (d == F32(0.8) * mn)) and np.any(ok.astype(bool) & (d == F32(1.2) * mx))
        outs[form] = (ok[sel], u[sel], v[sel])
    both = (outs[0][0] & outs[1][0]).astype(bool)
    assert (both & ((outs[0][1] != outs[1][1]) | (outs[0][2] != outs[1][2]))).sum() > 10   # the forms differ on the pinned points, facade and numpy alike
