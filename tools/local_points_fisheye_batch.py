"""SearchLocalPoints (M3) for a batch of fisheye-rig frames: orbm_search_by_projection_points_fisheye_batch_async as ONE batch call
against (1) the loop of orbm_search_by_projection_points_fisheye host calls it replaces, on the same inputs -- both must produce the same
rows, which is checked BEFORE anything is timed -- and (2) the one-camera orbm_search_by_projection_points_batch_async on the left rows
alone, which shows what the right block and the cross writes cost.

Shape (BASELINE config C4): 512 x 512 images, 1500 features per camera (synthetic stereo pairs through the product extractor, 16 rows;
larger batches repeat them in a gathered pool), 1500 local map points per pair built as tests/points_fisheye_cases.py builds them (80 %
in view on the left, 70 % on the right), mvLeftToRightMatch / mvRightToLeftMatch from mutual nearest descriptors, every point with
observations, no blocked slots, nnratio 0.8, th 1 and th 3.  --pairs takes the pair counts, default 1 8 64.
The batch is timed eagerly after a warm-up with the host clock round enqueue + sync (the handle's event pair spans from its last grid
build, so it is not reported); every figure is the median of --reps repetitions with the quartiles beside it.  The host loop has its frame
views prepared beforehand: only the search calls are timed, which favours the loop.  One JSON line per measurement.
The kernels alone come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/local_points_fisheye_batch.py --batch-only --pairs 64"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
pkg = importlib.import_module("orb-slam3_amd")
synth = importlib.import_module("orb-slam3_amd.synth")
import points_fisheye_cases as pc  # noqa: E402

W = H = 512
NF, NLEV, NQ, NNRATIO = 1500, 8, 1500, 0.8
INV_W, INV_H = float(np.float32(64) / np.float32(W)), float(np.float32(48) / np.float32(H))
NSRC = 8                                                                       # distinct stereo pairs


def _emit(d, out):
    line = json.dumps(d)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _stats(ms):
    q = np.percentile(ms, [25, 50, 75])
    return dict(median_ms=float(q[1]), q25_ms=float(q[0]), q75_ms=float(q[2]), reps=len(ms))


def _time_batch(m, enqueue, reps):
    L = pkg.lib()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert enqueue() == 0, L.orbm_last_error()
        assert L.orbm_sync(m.h) == 0
        wall.append((time.perf_counter() - t0) * 1e3)
    return _stats(wall)


def source_rows():
    """NSRC left rows and NSRC right rows from the product extractor; per source pair its query rows and its partner arrays."""
    imgs = [synth.gen_stereo_pair(W, H, 8100 + i) for i in range(NSRC)]
    ex = pkg.ORBextractor(NF, 1.2, NLEV, 20, 7, max_size=(W, H), max_batch=2 * NSRC)
    res = ex.extract_batch([p[0] for p in imgs] + [p[1] for p in imgs], [(0, 0)] * (2 * NSRC))
    rows = [(np.ascontiguousarray(k).view(pc.KP_DTYPE).reshape(-1).copy(), np.ascontiguousarray(d, np.uint8).reshape(-1, 32).copy()) for _, k, d in res]
    sf = ex.GetScaleFactors().astype(np.float32)
    ex.close()
    rng = np.random.default_rng(83)
    Q, partners = [], []
    for i in range(NSRC):
        q = pc._scene_queries(rng, rows[i][0], rows[i][1], rows[NSRC + i][0], rows[NSRC + i][1], NQ, 1.0)
        q["in_view"][(q["level"] < 0) | (q["level"] >= NLEV)] = 0              # the host form has no level test: such rows stay out of view
        q["in_view_r"][(q["level_r"] < -1) | (q["level_r"] >= NLEV)] = 0
        Q.append(pc.mask_skipped(q))
        partners.append(pc.mutual_nearest(rows[i][1], rows[NSRC + i][1]))
    return rows, Q, partners, sf


def measure(m, rows, Q, partners, sf, P, th, reps, out, batch_only):
    L = pkg.lib()
    cap = max(len(k) for k, _ in rows) + 8
    kps = np.zeros((2 * P, cap), pc.KP_DTYPE); desc = np.zeros((2 * P, cap, 32), np.uint8); counts = np.zeros(2 * P, np.int32)
    l2r = np.full((P, cap), -1, np.int32); r2l = np.full((P, cap), -1, np.int32)
    for p in range(P):
        for side, r in ((0, p), (1, P + p)):
            k, d = rows[side * NSRC + p % NSRC]
            kps[r, :len(k)] = k; desc[r, :len(k)] = d; counts[r] = len(k)
        a, b_ = partners[p % NSRC]
        l2r[p, :len(a)] = a; r2l[p, :len(b_)] = b_
    dk, dd, dc = pkg.DeviceBuffer(kps.nbytes).upload(kps), pkg.DeviceBuffer(desc.nbytes).upload(desc), pkg.DeviceBuffer(counts.nbytes).upload(counts)
    dl2r, dr2l = pkg.DeviceBuffer(l2r.nbytes).upload(l2r), pkg.DeviceBuffer(r2l.nbytes).upload(r2l)
    gs = pkg.DeviceBuffer(2 * P * 3073 * 4); gi = pkg.DeviceBuffer(2 * P * cap * 4)
    assert L.orbm_grid_build_batch_async(m.h, dk.ptr, dc.ptr, 2 * P, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0, L.orbm_last_error()
    m.sync()
    b = {}
    for name, dt in pc.FIELDS:
        b[name] = pkg.DeviceBuffer(P * NQ * np.dtype(dt).itemsize).upload(np.stack([Q[p % NSRC][name] for p in range(P)]).astype(dt))
    b["qdesc"] = pkg.DeviceBuffer(P * NQ * 32).upload(np.stack([Q[p % NSRC]["qdesc"] for p in range(P)]))
    b["nq"] = pkg.DeviceBuffer(4 * P).upload(np.full(P, NQ, np.int32))
    ml, mr, nm = pkg.DeviceBuffer(P * cap * 4), pkg.DeviceBuffer(P * cap * 4), pkg.DeviceBuffer(P * 4)
    sfp = sf.ctypes.data_as(C.c_void_p)

    def two_cameras():
        return L.orbm_search_by_projection_points_fisheye_batch_async(
            m.h, dk.ptr, dd.ptr, dc.ptr, cap, gs.ptr, gi.ptr, 0.0, 0.0, INV_W, INV_H, 0, P, P, None, None, dl2r.ptr, dr2l.ptr, b["nq"].ptr, NQ,
            b["in_view"].ptr, b["px"].ptr, b["py"].ptr, b["view_cos"].ptr, b["level"].ptr,
            b["in_view_r"].ptr, b["pxr"].ptr, b["pyr"].ptr, b["view_cos_r"].ptr, b["level_r"].ptr,
            None, 0.0, b["qdesc"].ptr, b["mp_obs"].ptr, 0, th, NNRATIO, sfp, NLEV, ml.ptr, mr.ptr, nm.ptr)

    def left_only():
        return L.orbm_search_by_projection_points_batch_async(
            m.h, dk.ptr, dd.ptr, dc.ptr, cap, gs.ptr, gi.ptr, 0.0, 0.0, INV_W, INV_H, 0, P, None, None, b["nq"].ptr, NQ,
            b["in_view"].ptr, b["px"].ptr, b["py"].ptr, None, b["view_cos"].ptr, b["level"].ptr, None, 0.0, b["qdesc"].ptr, b["mp_obs"].ptr, 0,
            th, NNRATIO, sfp, NLEV, ml.ptr, nm.ptr)

    views = None
    if not batch_only:
        views = [(pkg.FrameView(*rows[p % NSRC], W, H, backend=m), pkg.FrameView(*rows[NSRC + p % NSRC], W, H, backend=m)) for p in range(P)]

    def loop():
        res = []
        for p in range(P):
            q = Q[p % NSRC]; vl, vr = views[p]
            left = dict(in_view=q["in_view"], px=q["px"], py=q["py"], view_cos=q["view_cos"], level=q["level"])
            right = dict(in_view=q["in_view_r"], px=q["pxr"], py=q["pyr"], view_cos=q["view_cos_r"], level=q["level_r"])
            res.append(m.SearchByProjectionPointsFisheye(vl, vr, np.zeros(vl.n, np.uint8), np.zeros(vr.n, np.uint8), l2r[p, :vl.n], r2l[p, :vr.n], sf,
                                                         left, right, q["qdesc"], q["mp_obs"], th, NNRATIO))
        return res

    # rows first: the batch against the host loop, before anything is timed
    assert two_cameras() == 0, L.orbm_last_error()
    m.sync()
    rows_l = ml.download(np.int32, P * cap).reshape(P, cap); rows_r = mr.download(np.int32, P * cap).reshape(P, cap); cnt = nm.download(np.int32, P)
    equal = None
    if not batch_only:
        res = loop()
        equal = all(n == cnt[p] and np.array_equal(a, rows_l[p, :len(a)]) and np.array_equal(c, rows_r[p, :len(c)]) and
                    np.all(rows_l[p, len(a):] == -1) and np.all(rows_r[p, len(c):] == -1) for p, (n, a, c) in enumerate(res))
        if not equal:
            _emit(dict(search="M3 fisheye", path="host_loop", pairs=P, th=th, rows_equal_batch=False), out)
            return False
    shape = dict(pairs=P, features=int(counts.mean()), queries=NQ, th=th)
    _time_batch(m, left_only, 3)
    wall = _time_batch(m, left_only, reps)
    _emit(dict(search="M3", path="batch_left_rows_only", wall=wall, matches=int(nm.download(np.int32, P).sum()), **shape), out)
    _time_batch(m, two_cameras, 3)
    wall = _time_batch(m, two_cameras, reps)
    _emit(dict(search="M3 fisheye", path="batch", wall=wall, matches=int(cnt.sum()), matches_left_row=int((rows_l >= 0).sum()),
               matches_right_row=int((rows_r >= 0).sum()), **shape), out)
    if batch_only:
        return True
    ms = []
    for it in range(reps + 1):
        t0 = time.perf_counter()
        loop()
        if it:                                                                 # the first pass is a warm-up
            ms.append((time.perf_counter() - t0) * 1e3)
    _emit(dict(search="M3 fisheye", path="host_loop", wall=_stats(ms), rows_equal_batch=True, **shape), out)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--th", type=float, nargs="+", default=[1.0, 3.0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, Q, partners, sf = source_rows()
    m = pkg.ORBmatcher(0.9)
    ok = True
    for th in a.th:
        for P in a.pairs:
            ok = measure(m, rows, Q, partners, sf, P, th, a.reps, a.out, a.batch_only) and ok
    m.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
