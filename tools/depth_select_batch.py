"""Depth point selection for a batch kept on the device: orbm_select_depth_points_batch_async (the sorted walk of UpdateLastFrame /
CreateNewKeyFrame) and orbm_adopt_new_points_batch_async on --frames rows of --keypoints slots (default 64 x 1200), --reps eager calls,
against what they replace: the depth rows copied to the host, a host selection (numpy: a stable argsort per row and the closed-form
bound), and the flags and the four patched M4 query rows uploaded again.  All three are timed with the host clock between the same two
stream points (the stream idle before, synchronised after).  Prints one JSON line; the kernels alone come from running the tool under
rocprofv3 --kernel-trace --stats (k_depth_select, k_adopt_new_points).  A record of what the calls cost, not a threshold."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("orb-slam3_amd")


def host_select(depth, keeps, th, max_points):
    """create_new [nf][cap] and nvisit [nf] on the host: per row a stable argsort of the depth points (ties keep slot order)."""
    nf, cap = depth.shape
    create = np.zeros((nf, cap), np.uint8); nvisit = np.zeros(nf, np.int32)
    for f in range(nf):
        d = depth[f]
        idx = np.flatnonzero(d > 0)
        idx = idx[np.argsort(d[idx], kind="stable")]
        c = int(np.count_nonzero(~(d[idx] > th)))
        nv = min(len(idx), max(c, max_points) + 1)
        vis = idx[:nv]
        create[f, vis[keeps[f, vis] == 0]] = 1
        nvisit[f] = nv
    return create, nvisit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--keypoints", type=int, default=1200)
    ap.add_argument("--th-depth", type=float, default=3.2)
    ap.add_argument("--max-points", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    nf, cap, th, mp = a.frames, a.keypoints, a.th_depth, a.max_points
    m = pkg.ORBmatcher(0.9)
    counts = np.full(nf, cap, np.int32)
    raw = rng.integers(2000, 40000, (nf, cap)).astype(np.uint16)             # a 16-bit depth camera at 5000 units per metre: 0.4 .. 8 m, ties
    raw[rng.random(raw.shape) < 0.1] = 0
    depth = (raw.astype(np.float32) * np.float32(1.0 / 5000.0)).astype(np.float32)
    depth[depth <= 0] = -1
    keeps = (rng.random((nf, cap)) < 0.4).astype(np.uint8)
    desc = rng.integers(0, 256, (nf, cap, 32)).astype(np.uint8)
    x3n = rng.uniform(-3, 3, (nf, cap, 3)).astype(np.float32)
    rows = dict(x3=rng.uniform(-3, 3, (nf, cap, 3)).astype(np.float32), has=keeps.copy(), obs=keeps.copy(), qd=rng.integers(0, 256, (nf, cap, 32)).astype(np.uint8))
    up = lambda arr: pkg.DeviceBuffer(arr.nbytes).upload(np.ascontiguousarray(arr))
    dc, dd, dk, ddesc, dx3n = up(counts), up(depth), up(keeps), up(desc), up(x3n)
    dx3, dhas, dobs, dqd = up(rows["x3"]), up(rows["has"]), up(rows["obs"]), up(rows["qd"])
    order = pkg.DeviceBuffer(nf * cap * 4); cn = pkg.DeviceBuffer(nf * cap); nv = pkg.DeviceBuffer(nf * 4); nc = pkg.DeviceBuffer(nf * 4)

    def select():
        m.SelectDepthPointsBatchAsync(nf, 0, cap, dc.ptr, dd.ptr, dk.ptr, None, th, mp, order.ptr, cn.ptr, nv.ptr, nc.ptr)

    def select_adopt():
        select()
        m.AdoptNewPointsBatchAsync(nf, 0, cap, dc.ptr, cn.ptr, dx3n.ptr, ddesc.ptr, None, dx3.ptr, dhas.ptr, dobs.ptr, dqd.ptr)

    def host_path():
        d = dd.download(np.float32, nf * cap).reshape(nf, cap)               # D2H of the depth rows
        create, _ = host_select(d, keeps, np.float32(th), mp)
        sel = create == 1
        x3, has, obs, qd = rows["x3"].copy(), rows["has"].copy(), rows["obs"].copy(), rows["qd"].copy()
        x3[sel] = x3n[sel]; has[sel] = 1; obs[sel] = 0; qd[sel] = desc[sel]
        cn.upload(create); dx3.upload(x3); dhas.upload(has); dobs.upload(obs); dqd.upload(qd)   # H2D of the flags and the patched rows

    def timed(fn):
        fn(); m.sync()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(); m.sync(); ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    t_sel = timed(select)
    t_both = timed(select_adopt)
    dev_create = cn.download(np.uint8, nf * cap).reshape(nf, cap); dev_nv = nv.download(np.int32, nf)
    t_host = timed(host_path)
    create, nvisit = host_select(depth, keeps, np.float32(th), mp)
    assert np.array_equal(dev_create, create) and np.array_equal(dev_nv, nvisit) and 0 < int(create.sum())
    print(json.dumps(dict(tool="depth_select_batch", frames=nf, keypoints=cap, th_depth=th, max_points=mp, reps=a.reps,
                          visited=int(nvisit.sum()), created=int(create.sum()),
                          select_ms_median=t_sel[0], select_ms_min=t_sel[1], select_adopt_ms_median=t_both[0], select_adopt_ms_min=t_both[1],
                          host_path_ms_median=t_host[0], host_path_ms_min=t_host[1])), flush=True)


if __name__ == "__main__":
    main()
