"""The numpy restatement of M4's pose and projection lines (project_last_frame_np) against the facade's own expressions compiled
with g++ on facade/cvcompat.h (tests/motion_projection.cpp), bit for bit.  tests/test_gpu_motion_model_batch.py checks
orbm_project_last_frame_batch_async against the same restatement.  Host-only: no GPU."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _dot3(r, x):
    """cvcompat's product row: a double sum from 0 in k order of exact double products, rounded once to float."""
    p = r.astype(F64) * x.astype(F64)
    return (((F64(0) + p[..., 0]) + p[..., 1]) + p[..., 2]).astype(F32)


def project_last_frame_np(tcw_cur, tcw_last, x3dw, has_mp, k, bounds, mb, mono):
    """tcw_cur, tcw_last [P][12] (row-major 3x4), x3dw [P][Q][3], has_mp [P][Q]; k = (fx, fy, cx, cy), bounds = (minX, maxX, minY, maxY).
    Returns valid [P][Q] uint8, u, v, invzc [P][Q] float32 (0 where not valid) and dir [P] uint8."""
    T = np.asarray(tcw_cur, F32).reshape(-1, 3, 4); Tl = np.asarray(tcw_last, F32).reshape(-1, 3, 4)
    X = np.asarray(x3dw, F32)
    fx, fy, cx, cy = (F32(a) for a in k)
    minX, maxX, minY, maxY = (F32(a) for a in bounds)
    mb = F32(mb)
    twc = np.stack([_dot3(-T[:, :, r], T[:, :, 3]) for r in range(3)], 1)                    # -Rcw.t() * tcw
    tlcz = (_dot3(Tl[:, 2, :3], twc) + Tl[:, 2, 3]).astype(F32)                               # (Rlw * twc + tlw)(2)
    fwd = (tlcz > mb) & (not mono)
    bwd = (-tlcz > mb) & (not mono)
    dir_ = np.where(fwd, 1, np.where(bwd, 2, 0)).astype(np.uint8)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xc, yc, zc = ((_dot3(T[:, None, r, :3], X) + T[:, None, r, 3]).astype(F32) for r in range(3))
        invzc = (1.0 / zc.astype(F64)).astype(F32)
        u = ((fx * xc) / zc + cx).astype(F32)
        v = ((fy * yc) / zc + cy).astype(F32)
    valid = (np.asarray(has_mp) != 0) & ~(invzc < 0) & ~((u < minX) | (u > maxX)) & ~((v < minY) | (v > maxY))
    z = F32(0)
    return (valid.astype(np.uint8), np.where(valid, u, z).astype(F32), np.where(valid, v, z).astype(F32),
            np.where(valid, invzc, z).astype(F32), dir_)


def random_pose(rng, ang=0.05, trans=0.3):
    a = rng.uniform(-ang, ang, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = rng.uniform(-trans, trans, 3)
    return np.concatenate([R, t[:, None]], 1).astype(F32).reshape(12)


def test_restatement_equals_facade_expressions(tmp_path):
    exe = str(tmp_path / "motion_projection")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "motion_projection.cpp")])
    rng = np.random.default_rng(11)
    k = (458.654, 457.296, 367.215, 248.375)
    bounds = (0.0, 752.0, 0.0, 480.0)
    mb = 0.11007784
    n = 20000
    cur = np.stack([random_pose(rng, ang=rng.choice([0.01, 0.5, 3.0]), trans=rng.choice([0.05, 0.5, 5.0])) for _ in range(n)])
    last = np.stack([random_pose(rng, ang=0.2, trans=0.5) for _ in range(n)])
    # points in front of, behind and beside the camera, and far away
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(-3, 15, n)], 1).astype(F32)
    X[::7] *= F32(40)
    # points that project just onto / just outside each bound of the current camera (identity-like poses: nudge until it lands)
    edge = np.arange(0, n, 5)
    cur[edge] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    z = rng.uniform(1, 10, len(edge)).astype(F32)
    bu = np.array([bounds[0], bounds[1], k[2], k[2]], F32)[edge % 4]
    bv = np.array([k[3], k[3], bounds[2], bounds[3]], F32)[edge % 4]
    eps = rng.choice([-1e-4, 0.0, 1e-4], len(edge))
    X[edge] = np.stack([(bu + eps - F32(k[2])) * z / F32(k[0]), (bv + eps - F32(k[3])) * z / F32(k[1]), z], 1).astype(F32)
    X[X[:, 2] == 0, 2] = F32(0.5)                                                  # z == 0 exactly is outside the contract
    for mono in (False, True):
        hdr = np.array(list(k) + list(bounds) + [mb, float(mono), n], F32)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        np.concatenate([hdr, np.concatenate([cur, last, X], 1).reshape(-1)]).astype(F32).tofile(fin)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "motion_projection ok" in r.stdout, r.stdout + r.stderr
        out = np.fromfile(fout, F32).reshape(n, 5)
        valid, u, v, invzc, dir_ = project_last_frame_np(cur, last, X[:, None, :], np.ones((n, 1), np.uint8), k, bounds, mb, mono)
        assert np.array_equal(out[:, 0].astype(np.uint8), valid[:, 0])
        for col, a in ((1, u), (2, v), (3, invzc)):
            assert np.array_equal(out[:, col].view(np.uint32), a[:, 0].view(np.uint32)), col
        assert np.array_equal(out[:, 4].astype(np.uint8), dir_)
        # the cases reach every branch: behind the camera, outside each bound, inside, and (stereo) all three directions
        assert 0.2 * n < valid.sum() < 0.9 * n
        if not mono:
            assert all((dir_ == d).sum() > 100 for d in (0, 1, 2))
        else:
            assert np.all(dir_ == 0)
