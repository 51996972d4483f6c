"""Relocalisation SearchByProjection (M5) for a batch of (frame row, candidate KeyFrame, pose) triples: one
orbm_search_by_projection_kf_batch_async call against a loop of host orbm_search_by_projection_kf calls over the same pairs.

Shapes (tests/test_gpu_reloc_batch.py's synthetic pools: 752 x 480 frame rows of 1 500 keypoints on 8 levels; each candidate KeyFrame has
1 000 MapPoints back-projected from frame keypoints, 30 % of the frame's slots blocked by the PnP inliers, 10 % of the MapPoints in
sAlreadyFound), at th 10 / ORBdist 100 and th 3 / ORBdist 64, orientation check on:
- reloc8 / reloc32: 1 frame x 8 / 32 candidates (Tracking::Relocalization);
- trackers64x8: 64 frame rows x 8 candidates each (many lost trackers).
The batch is timed eagerly after a warm-up: device events of the handle (orbm_last_timing: the grid build of the pool's rows plus the
search, as for the other batched searches) and the host clock around the search's enqueue + sync; rocprofv3 --kernel-trace --stats gives the kernels alone.  The host loop is one orbm_search_by_projection_kf per
pair with its FrameView (grid) built beforehand and the projections precomputed: only the search calls are timed, which favours the loop.
Both must produce the same rows.  Prints one JSON line per measurement.

--fuzz N: N random calls (pairs per call, rows in and out of range, empty rows, th 1-15, ORBdist 20-120, orientation on / off, blocked
and sAlreadyFound rates, duplicated MapPoints) compared pair by pair with the oracle's SearchByProjectionKF and the host entry point, both
fed by reloc_project_np; prints one JSON line with the mismatch count."""
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
import orbref  # noqa: E402
import test_gpu_reloc_batch as T  # noqa: E402


def _emit(d, out):
    line = json.dumps(d)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _pairs(rng, pool, rows, nq=1000, blocked=0.3, found=0.1):
    pairs = []
    for r in rows:
        src_row = r if 0 <= r < pool.R and pool.counts[r] > 0 else 0
        p = T.keyframe(rng, pool, src_row, nq, found=found)
        p.update(row=int(r), blocked=(rng.random(pool.cap) < blocked).astype(np.uint8))
        pairs.append(p)
    return pairs


def _reference(pool, p, th, od, ori, OM=None):
    """(n, row) of the host entry point (or the oracle with OM) for pair p; (0, None) where the batch must give an empty row."""
    r = p["row"]
    if not (0 <= r < pool.R) or len(p["valid"]) == 0 or pool.counts[r] == 0:
        return 0, None
    kt, dt = pool.row(r)
    ok, u, v, lvl = T.proj_of(pool, p)
    args = dict(blocked=p["blocked"][:len(kt)], scale_factors=pool.sf, valid=ok, u=u, v=v, level=np.maximum(lvl, 0), angle=p["angle"],
                qdesc=p["qdesc"], th=th, orb_dist=od, check_ori=ori)
    M = OM or pool.m
    return M.SearchByProjectionKF(p["view_om"] if OM else p["view"], **args)


def measure(pool, shape, rows, reps, out, rng):
    pairs = _pairs(rng, pool, rows)
    call = T.Call(pool, pairs, rng=rng)
    views = {r: pkg.FrameView(*pool.row(r), pool.w, pool.h, backend=pool.m) for r in set(rows)}
    for p in pairs:
        p["view"] = views[p["row"]]
    for th, od in ((10.0, 100), (3.0, 64)):
        match, nm = call.run(th, od, True)                                     # warm-up (and the rows the loop must reproduce)
        dev, wall = [], []
        for _ in range(reps):
            pool.grid()                                                        # orbm_last_timing spans grid build + the search
            t0 = time.perf_counter()
            assert call.enqueue(th, od, True) == 0
            assert pool.L.orbm_sync(pool.m.h) == 0
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(pool.m.timing_ms())
        _emit(dict(path="batch", shape=shape, pairs=len(pairs), frame_rows=len(set(rows)), queries_per_pair=1000, th=th, orb_dist=od,
                   device_ms_grid_and_search=float(np.median(dev)), wall_ms_search_call=float(np.median(wall)), matches=int(nm.sum())), out)
        args = []
        for p in pairs:                                                        # projections precomputed: only the searches are timed
            ok, u, v, lvl = T.proj_of(pool, p)
            args.append(dict(blocked=p["blocked"][:pool.counts[p["row"]]], scale_factors=pool.sf, valid=ok, u=u, v=v,
                             level=np.maximum(lvl, 0), angle=p["angle"], qdesc=p["qdesc"], th=th, orb_dist=od, check_ori=True))
        loop, equal = [], True
        for it in range(max(2, reps // 10) + 1):
            t0 = time.perf_counter()
            res = [pool.m.SearchByProjectionKF(p["view"], **a) for p, a in zip(pairs, args)]
            if it:                                                             # the first pass is a warm-up
                loop.append((time.perf_counter() - t0) * 1e3)
        for i, (n, row) in enumerate(res):
            nt = pool.counts[pairs[i]["row"]]
            equal &= n == nm[i] and np.array_equal(row, match[i, :nt])
        _emit(dict(path="host_loop", shape=shape, pairs=len(pairs), th=th, orb_dist=od, wall_ms_per_batch=float(np.median(loop)),
                   wall_ms_per_call=float(np.median(loop)) / len(pairs), rows_equal_batch=bool(equal)), out)


def fuzz(n, seed, out):
    rng = np.random.default_rng(seed)
    OM = orbref._oracle_matcher_class()()
    counts = [1500, 2500, 0, 4000, 800, 3000]
    pool = T.synth_pool(pkg, rng, counts, 4096)
    views = {r: (pkg.FrameView(*pool.row(r), pool.w, pool.h, backend=pool.m), pkg.FrameView(*pool.row(r), pool.w, pool.h, backend=OM))
             for r in range(pool.R) if pool.counts[r] > 0}
    cases, mism, total_pairs, total_m = [], 0, 0, 0
    for _ in range(n):
        P = int(rng.integers(1, 25))
        rows = rng.choice([-1, 0, 1, 2, 3, 4, 5, 6], P, p=[.04, .3, .15, .05, .2, .1, .12, .04])
        blocked, found = float(rng.choice([0.0, 0.35, 0.9, 0.97])), float(rng.choice([0.0, 0.5, 1.0, 0.1]))
        th, od, ori = float(np.round(rng.uniform(1, 15), 3)), int(rng.integers(20, 121)), bool(rng.integers(0, 2))
        nq = int(rng.integers(0, 1500))
        pairs = _pairs(rng, pool, rows, nq=nq, blocked=blocked, found=found)
        if rng.random() < 0.3:                                                 # duplicated MapPoints: colliding claims
            for p in pairs:
                if len(p["valid"]) > 4:
                    p["pw"][1::2] = p["pw"][0:-1:2][:len(p["pw"][1::2])]; p["qdesc"][1::2] = p["qdesc"][0:-1:2][:len(p["qdesc"][1::2])]
                    p["valid"][T.near_integer_level(p["pw"][None], p["mn"][None], p["mx"][None], p["tcw"][None], p["ow"][None], T.LOG_SF,
                                                    pool.nlev)[0]] = 0
        for p in pairs:
            if p["row"] in views:
                p["view"], p["view_om"] = views[p["row"]]
        call = T.Call(pool, pairs, rng=rng)
        match, nm = call.run(th, od, ori)
        bad = 0
        for i, p in enumerate(pairs):
            n_h, m_h = _reference(pool, p, th, od, ori)
            n_o, m_o = _reference(pool, p, th, od, ori, OM)
            if m_o is None:
                ok = nm[i] == 0 and np.all(match[i] == -1)
            else:
                nt = len(m_o)
                ok = n_h == n_o and np.array_equal(m_h, m_o) and nm[i] == n_o and np.array_equal(match[i, :nt], m_o) and np.all(match[i, nt:] == -1)
            bad += not ok
        mism += bad; total_pairs += P; total_m += int(nm.sum())
        cases.append(dict(pairs=P, q=nq, th=th, orb_dist=od, check_ori=ori, blocked=blocked, found=found,
                          out_of_range=int(((rows < 0) | (rows >= pool.R)).sum()), matches=int(nm.sum()), mismatched_pairs=bad))
    _emit(dict(path="fuzz", seed=seed, calls=n, pairs=total_pairs, matches=total_m, mismatches=mism, cases=cases), out)
    return mism


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--fuzz", type=int, default=0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--fuzz-out", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    one = T.synth_pool(pkg, rng, [1500], 1536)
    measure(one, "reloc8", [0] * 8, a.reps, a.out, rng)
    measure(one, "reloc32", [0] * 32, a.reps, a.out, rng)
    many = T.synth_pool(pkg, rng, [1500] * 64, 1536)
    measure(many, "trackers64x8", [r for r in range(64) for _ in range(8)], a.reps, a.out, rng)
    if a.fuzz:
        sys.exit(1 if fuzz(a.fuzz, a.seed, a.fuzz_out) else 0)


if __name__ == "__main__":
    main()
