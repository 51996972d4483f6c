"""Fuse (M13) for a batch of (KeyFrame, MapPoint row) pairs: one orbm_fuse_batch_async call against a loop of host orbm_fuse calls over
the same pairs.

Shapes at 752 x 480 / 1000 features (tests/test_gpu_fuse_batch.py's scenes: 12 KeyFrame rows, right views of synthetic stereo scenes;
MapPoints = the left views' keypoints back-projected at depth bf / disparity):
- neighbours: P = 10 / 30 / 60 target KeyFrames x 1 500 shared MapPoints (SearchInNeighbors' first loop, th 3, chi2 gate, stereo);
- current: 1 KeyFrame x 30 000 MapPoints (its second loop).
The batch is timed eagerly: device events of the handle (orbm_last_timing: the grid build of the 12 rows plus the search, as for the
other batched searches) and the host clock around the search's enqueue + sync; rocprofv3 --kernel-trace --stats gives the kernels alone.  The host loop is
one orbm_fuse per pair with its FrameView (grid) built beforehand and the projections precomputed: only the search calls are timed, which
favours the loop.  Both must produce the same rows.  Prints one JSON line per measurement.

--fuzz N: N random calls (pairs per call, rows in and out of range, th 1-6, both variants, stereo or not, shared or per-pair rows, valid
rates, pose perturbations) compared pair by pair with the oracle's Fuse (and the host entry point) fed by fuse_project_np; prints one
JSON line with the mismatch count."""
import argparse
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
import test_gpu_fuse_batch as T  # noqa: E402
from test_fuse_projection_cpu import F32, camera_centre_np, fuse_project_np, near_integer_level  # noqa: E402

NB = 12


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _pairs(S, rng, P, qidx, shared=True):
    rows = (np.arange(P) % S.nb).astype(np.int32)
    tcw = np.stack([T.perturb(rng, T.scene_pose(int(r))) for r in rows]); ow = camera_centre_np(tcw)
    Q = len(qidx)
    valid = (rng.random((P, Q)) >= 0.2).astype(np.uint8)
    pw, nrm, mn, mx = S.pw[qidx], S.normal[qidx], S.min_dist[qidx], S.max_dist[qidx]
    valid[near_integer_level(pw[None], mn[None], mx[None], tcw, ow, T.LOG_SF, T.NLEV)] = 0
    return rows, tcw, ow, valid, pw, nrm, mn, mx, S.qdesc[qidx]


def measure(S, shape, P, Q, reps, out, rng):
    qidx = rng.choice(S.Q, Q, replace=False) if Q <= S.Q else np.concatenate([np.arange(S.Q)] * (Q // S.Q) + [rng.choice(S.Q, Q % S.Q, replace=False)])
    rows, tcw, ow, valid, pw, nrm, mn, mx, qd = _pairs(S, rng, P, qidx)
    if Q > S.Q:                                                                # repeated MapPoints: move the copies a little
        pw = (pw + rng.normal(0, 1e-3, pw.shape)).astype(F32)
        valid[near_integer_level(pw[None], mn[None], mx[None], tcw, ow, T.LOG_SF, T.NLEV)] = 0
    th, chi2, stereo = 3.0, 1, True
    c = T.Call(S, rows, tcw, ow, np.full(P, Q, np.int32), valid, pw, nrm, mn, mx, qd, True)
    best, nf, _ = c.run(th, chi2, stereo)                                     # warm-up (and the rows the loop must reproduce)
    dev, wall = [], []
    for _ in range(reps):
        S.grid()                                                               # orbm_last_timing spans grid build + the search
        t0 = time.perf_counter()
        assert c.enqueue(th, chi2, stereo) == 0
        assert S.L.orbm_sync(S.m.h) == 0
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(S.m.timing_ms())
    _emit(dict(path="batch", shape=shape, pairs=P, queries=Q, th=th, chi2_gate=chi2, stereo=stereo, kf_rows=S.nb,
               device_ms_grid_and_search=float(np.median(dev)), wall_ms_search_call=float(np.median(wall)), fused=int(nf.sum())), out)
    proj = fuse_project_np(tcw, ow, pw[None], nrm[None], mn[None], mx[None], valid, T.KCAM, T.BOUNDS, T.BF, T.LOG_SF, T.NLEV)
    views = {}
    for r in set(int(x) for x in rows):
        kk, dk = S.res[r][1], S.res[r][2]
        views[r] = pkg.FrameView(kk, dk, T.W, T.H, uright=S.uright[r, :len(kk)].copy(), backend=S.m)
    args = [dict(valid=proj[0][p], u=proj[1][p], v=proj[2][p], ur=proj[3][p], level=np.maximum(proj[4][p], 0)) for p in range(P)]
    loop = []
    equal = True
    for rep in range(max(1, reps // 4)):
        t0 = time.perf_counter()
        res = [S.m.Fuse(views[int(rows[p])], S.sf, S.isg, qdesc=qd, th=th, chi2_gate=bool(chi2), **args[p]) for p in range(P)]
        loop.append((time.perf_counter() - t0) * 1e3)
        equal &= all(n == nf[p] and np.array_equal(b, best[p]) for p, (n, b) in enumerate(res))
    _emit(dict(path="host_loop", shape=shape, pairs=P, queries=Q, wall_ms_per_batch=float(np.median(loop)),
               wall_ms_per_call=float(np.median(loop)) / P, rows_equal_batch=bool(equal)), out)


def fuzz(S, n, seed, out):
    rng = np.random.default_rng(seed)
    pairs = mism = fused = 0
    cases = []
    for _ in range(n):
        P = int(rng.integers(1, 25))
        shared = bool(rng.random() < 0.5)
        chi2, stereo = int(rng.random() < 0.5), bool(rng.random() < 0.5)
        th = float(np.float32(rng.uniform(1, 6)))
        rows = rng.integers(-1, S.nb + 2, P).astype(np.int32)
        ang, trans = float(rng.choice([0.0005, 0.002, 0.01])), float(rng.choice([0.001, 0.01, 0.05]))
        tcw = np.stack([T.perturb(rng, T.scene_pose(int(r) % S.nb), ang, trans) for r in rows]); ow = camera_centre_np(tcw)
        rate = float(rng.choice([0.1, 0.5, 0.9, 1.0]))
        if shared:
            Q = int(rng.integers(1, 3000)); qidx = rng.choice(S.Q, Q, replace=False)
            nq = np.full(P, Q, np.int32); qs = Q
            pw, nrm, mn, mx, qd = (a[qidx][None] for a in (S.pw, S.normal, S.min_dist, S.max_dist, S.qdesc))
        else:
            nq = rng.integers(0, 1500, P).astype(np.int32); qs = int(nq.max()) + int(rng.integers(1, 9))
            qidx = rng.integers(0, S.Q, (P, qs))
            pw, nrm, mn, mx, qd = (a[qidx] for a in (S.pw, S.normal, S.min_dist, S.max_dist, S.qdesc))
        valid = (rng.random((P, qs)) < rate).astype(np.uint8)
        valid[near_integer_level(pw, mn, mx, tcw, ow, T.LOG_SF, T.NLEV)] = 0
        c = T.Call(S, rows, tcw, ow, nq, valid, pw[0] if shared else pw, nrm[0] if shared else nrm, mn[0] if shared else mn,
                   mx[0] if shared else mx, qd[0] if shared else qd, shared)
        got = c.run(th, chi2, stereo)
        vin = valid * (np.arange(qs)[None, :] < nq[:, None])
        proj = fuse_project_np(tcw, ow, pw, nrm, mn, mx, vin, T.KCAM, T.BOUNDS, T.BF, T.LOG_SF, T.NLEV)
        proj[4][(rows < 0) | (rows >= S.nb)] = -1
        ref = T.reference(pkg, _oracle, S, rows, nq, proj, qd, th, chi2, stereo)
        bad = [p for p in range(P) if not (np.array_equal(got[0][p], ref[0][p]) and got[1][p] == ref[1][p] and np.array_equal(got[2][p], ref[2][p]))]
        pairs += P; mism += len(bad); fused += int(got[1].sum())
        cases.append(dict(pairs=P, shared=shared, q_stride=qs, th=round(th, 3), chi2_gate=chi2, stereo=stereo, valid_rate=rate,
                          perturb=[ang, trans], out_of_range=int(((rows < 0) | (rows >= S.nb)).sum()), fused=int(got[1].sum()),
                          mismatched_pairs=len(bad)))
    _emit(dict(path="fuzz", seed=seed, calls=n, pairs=pairs, fused=fused, mismatches=mism, cases=cases), out)
    return mism


_oracle = None


def main():
    global _oracle
    ap = argparse.ArgumentParser()
    ap.add_argument("--fuzz", type=int, default=0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = T.Scenes(pkg, synth, nb=NB)
    if a.fuzz:
        import orbref
        orbref.lib()
        _oracle = orbref
        sys.exit(1 if fuzz(S, a.fuzz, a.seed, a.out) else 0)
    rng = np.random.default_rng(a.seed)
    for P in (10, 30, 60):
        measure(S, "neighbours", P, 1500, a.reps, a.out, rng)
    measure(S, "current", 1, 30000, a.reps, a.out, rng)


if __name__ == "__main__":
    main()
