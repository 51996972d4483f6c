"""tests/second_reading_mappoint.py's UpdateNormalAndDepth against facade/MapPointRefresh.h's cv::Mat statement of MapPoint.cc:601-649
compiled with g++ on facade/cvcompat.h (tests/mappoint_normal.cpp), bit for bit.  tests/test_gpu_mappoint.py checks
orbm_update_normal_and_depth(_batch_async) against the same second reading.  Host-only: no GPU."""
import os
import subprocess

import numpy as np

import second_reading_mappoint as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MAXC = 8


def test_second_reading_equals_facade_expressions(tmp_path):
    exe = str(tmp_path / "mappoint_normal")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "mappoint_normal.cpp")])
    rng = np.random.default_rng(31)
    sf = (F(1.2) ** np.arange(8)).astype(F)
    n = 4000
    pos = rng.uniform(-6, 6, (n, 3)).astype(F)
    ncent = rng.integers(1, MAXC + 1, n)
    cent = rng.uniform(-3, 3, (n, MAXC, 3)).astype(F)
    ref = cent[:, 0].copy()
    level = rng.integers(0, len(sf), n)
    # the edge points: far away, very close to a centre, on an axis, huge and tiny coordinates, a point at distance exactly 5
    pos[0] = [3, 0, 4]; cent[0, 0] = 0; ref[0] = 0; ncent[0] = 1
    pos[1] = [1e18, -1e18, 1e18]; pos[2] = cent[2, 0] + F(1e-6); pos[3] = [0, 0, 7]; cent[3, :, :2] = 0
    pos[4] = [1e-20, 1e-20, 1e-20]; cent[4] = 0; ref[4] = 0
    pos[5] = cent[5, 1] + np.array([1e-30, 0, 0], F)                        # a denormal-sized offset that survives the float subtraction or not
    pos[6] = [2e19, 0, 0]                                                   # d^2 overflows float, not the double sum
    ncent[7] = MAXC; ncent[8] = 1
    for i in range(n):                                                      # a point exactly at a centre is outside what is pinned (NaN bits)
        for k in range(ncent[i]):
            if np.array_equal(pos[i], cent[i, k]):
                pos[i, 0] += F(0.5)
    rec = np.concatenate([pos, ref, level[:, None].astype(F), ncent[:, None].astype(F), cent.reshape(n, -1)], 1).astype(F)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array([len(sf), n], F), sf, rec.reshape(-1)]).astype(F).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mappoint_normal ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(fout, F).reshape(n, 5)
    want = np.zeros((n, 5), F)
    for i in range(n):
        nv, mn, mx = R.update_normal_and_depth(pos[i], cent[i, :ncent[i]], ref[i], int(level[i]), sf)
        want[i, :3] = nv; want[i, 3] = mn; want[i, 4] = mx
    finite = np.isfinite(want).all(1)
    assert finite.sum() > n - 4 and finite[[0, 1, 3, 4, 6]].all()
    bad = np.flatnonzero((out.view(np.uint32) != want.view(np.uint32)).any(1) & finite)
    assert len(bad) == 0, (bad[:5], out[bad[:5]], want[bad[:5]])
    assert np.array_equal(np.isnan(out), np.isnan(want))
    assert np.array_equal(out[0, :3], np.array([3, 0, 4], F) * F(0.2)) and out[0, 4] == F(5) * sf[level[0]]
