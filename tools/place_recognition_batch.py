"""Place-recognition searches for a batch: M8 SearchByBoW(KeyFrame, KeyFrame) (orbm_search_by_bow_kf_batch_async) and M6 Sim3
SearchByProjection (orbm_search_by_projection_sim3_batch_async), each as ONE batch call against the loop of host entry-point calls
(orbm_search_by_bow_kf, orbm_search_by_projection_sim3) it replaces, on the same inputs.  Both must produce the same rows.

Shapes:
- M8 place36: the current KeyFrame (row 0 of a pool of extractor result rows, ~1000 features each, synthetic stereo images) against 36
  rows, nnratio 0.9, orientation on -- LoopClosing::DetectCommonRegionsFromBoW; M8 x8 / x64 / x512: that many pairs of distinct rows.
- M6 place6: one KeyFrame row of 1500 keypoints under 6 Sim3 poses, ~3000 MapPoints each, 30 % of the slots in matched_in, at th 8 /
  ratio 1.5 / proj_form 1 and th 5 / ratio 1.0 / proj_form 0; M6 x8 / x64 / x512 pairs of 1000 MapPoints.
The batch is timed eagerly after a warm-up with the host clock round enqueue + sync and with the handle's device events
(orbm_last_timing).  For M6 the handle's device figure spans from its last grid build to the search, as for the other window searches:
the pool's grid is rebuilt and synced before each timed call, outside the host clock, and the figure is named device_grid_and_search.
The host loop has its views, FeatureVectors and projections prepared beforehand: only the search calls are timed, which favours the
loop.  Every figure is the median of --reps repetitions with the quartiles beside it.  One JSON line per measurement.

--fuzz N: N random calls of each search (pair counts, rows in and out of range, good / matched / valid rates, nnratio, orientation,
th 1-12, ratios 0.5-2, both projection forms, duplicated MapPoints) compared pair by pair with the oracle and the host entry point;
prints one JSON line with the mismatch count and exits 1 if there is one."""
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
import orbref  # noqa: E402
import test_gpu_bow_batch as TB  # noqa: E402
import test_gpu_bow_kf_batch as T8  # noqa: E402
import test_gpu_reloc_batch as TR  # noqa: E402
import test_gpu_sim3_projection_batch as T6  # noqa: E402


def _emit(d, out):
    line = json.dumps(d)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _stats(ms):
    q = np.percentile(ms, [25, 50, 75])
    return dict(median_ms=float(q[1]), q25_ms=float(q[0]), q75_ms=float(q[2]), reps=len(ms))


def _time_batch(m, enqueue, reps, pre=None):
    L = pkg.lib()
    wall, dev = [], []
    for _ in range(reps):
        if pre:                                                                # outside the host clock
            pre()
            assert L.orbm_sync(m.h) == 0
        t0 = time.perf_counter()
        assert enqueue() == 0, L.orbm_last_error()
        assert L.orbm_sync(m.h) == 0
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(m.timing_ms())
    return _stats(wall), _stats(dev)


def _time_loop(fn, reps):
    ms = []
    for it in range(max(3, reps // 10) + 1):
        t0 = time.perf_counter()
        res = fn()
        if it:                                                                 # the first pass is a warm-up
            ms.append((time.perf_counter() - t0) * 1e3)
    return res, _stats(ms)


# ---- M8 ------------------------------------------------------------------------------------------------------------------------------
def bow_pool(mt, nimg, seed):
    imgs = []
    for i in range((nimg + 1) // 2):
        imgs.extend(synth.gen_stereo_pair(TB.W, TB.H, seed + i))
    pool = TB.Pool(pkg, mt, imgs[:nimg], 1000)
    voc = TB._vocab(pkg, synth, mt, 10, 6)
    pool.transform(voc, 4)
    return pool


def _m8_host_args(A, B, r1, r2, g1, g2, nnratio, ori, weights=True):
    k1, d1, k2, d2 = A.kps(r1), A.desc(r1), B.kps(r2), B.desc(r2)
    n1, n2 = len(k1), len(k2)
    keep1 = A.h_weight[r1, :n1] > 0 if weights else np.ones(n1, bool)
    keep2 = B.h_weight[r2, :n2] > 0 if weights else np.ones(n2, bool)
    return dict(k1=k1, d1=d1, good1=np.ascontiguousarray(g1[r1 * A.cap: r1 * A.cap + n1]), fv1=TB._fv(A.h_node[r1, :n1], keep1),
                k2=k2, d2=d2, good2=np.ascontiguousarray(g2[r2 * B.cap: r2 * B.cap + n2]), fv2=TB._fv(B.h_node[r2, :n2], keep2),
                nnratio=nnratio, check_ori=ori)


def measure_m8(mt, pool, shape, row1, row2, reps, out):
    L = pkg.lib()
    P = len(row1)
    good = np.ones(pool.rows * pool.cap, np.uint8)
    d1 = pkg.DeviceBuffer(4 * P).upload(np.asarray(row1, np.int32)); d2 = pkg.DeviceBuffer(4 * P).upload(np.asarray(row2, np.int32))
    dg = pkg.DeviceBuffer(good.nbytes).upload(good)
    mm = pkg.DeviceBuffer(4 * P * pool.cap); nm = pkg.DeviceBuffer(4 * P)

    def enqueue():
        return L.orbm_search_by_bow_kf_batch_async(mt.h, P, pool.rows, pool.cap, pool.r["kps"], pool.r["desc"], pool.r["counts"], pool.node.ptr,
                                                   pool.weight.ptr, dg.ptr, pool.rows, pool.cap, pool.r["kps"], pool.r["desc"], pool.r["counts"],
                                                   pool.node.ptr, pool.weight.ptr, dg.ptr, d1.ptr, d2.ptr, 0.9, 1, mm.ptr, nm.ptr)
    _time_batch(mt, enqueue, 3)
    wall, dev = _time_batch(mt, enqueue, reps)
    rows = mm.download(np.int32, P * pool.cap).reshape(P, pool.cap); cnt = nm.download(np.int32, P)
    _emit(dict(search="M8", path="batch", shape=shape, pairs=P, features=int(np.mean([len(pool.kps(r)) for r in set(row2)])),
               wall=wall, device=dev, matches=int(cnt.sum())), out)
    args = [_m8_host_args(pool, pool, a, b, good, good, 0.9, True) for a, b in zip(row1, row2)]
    res, loop = _time_loop(lambda: [mt.SearchByBoWKF(**a) for a in args], reps)
    equal = all(n == cnt[i] and np.array_equal(r, rows[i, :len(r)]) for i, (n, r) in enumerate(res))
    _emit(dict(search="M8", path="host_loop", shape=shape, pairs=P, wall=loop, rows_equal_batch=bool(equal)), out)
    return equal


def fuzz_m8(mt, pool, n, rng, OM):
    mism = pairs_total = matches = 0
    for _ in range(n):
        P = int(rng.integers(1, 40))
        r1 = rng.integers(-1, pool.rows + 1, P); r2 = rng.integers(-1, pool.rows + 1, P)
        if rng.random() < 0.5:
            r1[:] = r1[0]
        g1 = (rng.random(pool.rows * pool.cap) < rng.choice([0.0, 0.5, 0.9, 1.0])).astype(np.uint8)
        g2 = (rng.random(pool.rows * pool.cap) < rng.choice([0.0, 0.5, 0.9, 1.0])).astype(np.uint8)
        nnratio, ori, weights = float(rng.choice([0.6, 0.75, 0.9, 1.0])), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        rows, cnt = T8._run(pkg, mt, pool, pool, r1, r2, g1, g2, nnratio, ori, weights=weights)
        for i, (a, b) in enumerate(zip(r1, r2)):
            if not (0 <= a < pool.rows and 0 <= b < pool.rows) or not len(pool.kps(a)) or not len(pool.kps(b)):
                ok = cnt[i] == 0 and np.all(rows[i] == -1)
            else:
                args = _m8_host_args(pool, pool, a, b, g1, g2, nnratio, ori, weights)
                h, o = mt.SearchByBoWKF(**args), OM.SearchByBoWKF(**args)
                n1 = len(o[1])
                ok = h[0] == o[0] == cnt[i] and np.array_equal(h[1], o[1]) and np.array_equal(rows[i, :n1], o[1]) and np.all(rows[i, n1:] == -1)
            mism += not ok
        pairs_total += P; matches += int(cnt.sum())
    return dict(search="M8", calls=n, pairs=pairs_total, matches=matches, mismatches=mism)


# ---- M6 ------------------------------------------------------------------------------------------------------------------------------
def _m6_pairs(rng, pool, rows, nq, matched=0.3, found=0.1):
    pairs = []
    for r in rows:
        src = r if 0 <= r < pool.R and pool.counts[r] > 0 else 0
        p = T6.mappoints(rng, pool, src, nq, found=found)
        p.update(row=int(r), matched=(rng.random(pool.cap) < matched).astype(np.uint8))
        pairs.append(p)
    return pairs


def _m6_host_args(pool, p, th, ratio, form):
    ok, u, v, lvl = T6.proj_of(pool, p, form)
    return dict(matched_in=p["matched"][:pool.counts[p["row"]]], scale_factors=pool.sf, valid=ok, u=u, v=v, level=np.maximum(lvl, 0),
                qdesc=p["qdesc"], th=th, ratio_hamming=ratio)


def measure_m6(pool, shape, rows, nq, reps, out, rng):
    pairs = _m6_pairs(rng, pool, rows, nq)
    call = T6.Call(pool, pairs, rng=rng)
    views = {r: pkg.FrameView(*pool.row(r), pool.w, pool.h, backend=pool.m) for r in set(rows)}
    equal = True
    for th, ratio, form in ((8, 1.5, 1), (5, 1.0, 0)):
        match, nm = call.run(th, ratio, form)
        wall, dev = _time_batch(pool.m, lambda: call.enqueue(th, ratio, form), reps, pre=pool.grid)
        _emit(dict(search="M6", path="batch", shape=shape, pairs=len(pairs), queries_per_pair=nq, th=th, ratio=ratio, proj_form=form,
                   wall=wall, device_grid_and_search=dev, matches=int(nm.sum())), out)
        args = [_m6_host_args(pool, p, th, ratio, form) for p in pairs]
        res, loop = _time_loop(lambda: [pool.m.SearchByProjectionSim3(views[p["row"]], **a) for p, a in zip(pairs, args)], reps)
        eq = all(n == nm[i] and np.array_equal(r, match[i, :len(r)]) for i, (n, r) in enumerate(res))
        equal &= eq
        _emit(dict(search="M6", path="host_loop", shape=shape, pairs=len(pairs), th=th, ratio=ratio, wall=loop, rows_equal_batch=bool(eq)), out)
    return equal


def fuzz_m6(n, rng, OM):
    pool = TR.synth_pool(pkg, rng, [1500, 2500, 0, 4000, 800, 3000], 4096)
    views = {r: (pkg.FrameView(*pool.row(r), pool.w, pool.h, backend=pool.m), pkg.FrameView(*pool.row(r), pool.w, pool.h, backend=OM))
             for r in range(pool.R) if pool.counts[r] > 0}
    mism = pairs_total = matches = 0
    for _ in range(n):
        P = int(rng.integers(1, 25))
        rows = rng.choice([-1, 0, 1, 2, 3, 4, 5, 6], P, p=[.04, .3, .15, .05, .2, .1, .12, .04])
        matched, found = float(rng.choice([0.0, 0.35, 0.9, 0.97])), float(rng.choice([0.0, 0.5, 1.0, 0.1]))
        th, ratio, form = int(rng.integers(1, 13)), float(np.float32(rng.uniform(0.5, 2.0))), int(rng.integers(0, 2))
        pairs = _m6_pairs(rng, pool, rows, int(rng.integers(0, 1500)), matched, found)
        if rng.random() < 0.3:                                                 # duplicated MapPoints: colliding claims
            for p in pairs:
                if len(p["valid"]) > 4:
                    for key in ("pw", "normal", "qdesc", "mn", "mx"):
                        p[key][1::2] = p[key][0:-1:2][:len(p[key][1::2])]
                    p["valid"][T6.near_integer_level(p["pw"][None], p["mn"][None], p["mx"][None], p["tcw"][None], p["ow"][None], TR.LOG_SF,
                                                     pool.nlev)[0]] = 0
        call = T6.Call(pool, pairs, rng=rng)
        match, nm = call.run(th, ratio, form)
        for i, p in enumerate(pairs):
            if p["row"] not in views or len(p["valid"]) == 0:
                ok = nm[i] == 0 and np.all(match[i] == -1)
            else:
                a = _m6_host_args(pool, p, th, ratio, form)
                h = pool.m.SearchByProjectionSim3(views[p["row"]][0], **a); o = OM.SearchByProjectionSim3(views[p["row"]][1], **a)
                nt = len(o[1])
                ok = h[0] == o[0] == nm[i] and np.array_equal(h[1], o[1]) and np.array_equal(match[i, :nt], o[1]) and np.all(match[i, nt:] == -1)
            mism += not ok
        pairs_total += P; matches += int(nm.sum())
    return dict(search="M6", calls=n, pairs=pairs_total, matches=matches, mismatches=mism)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--fuzz", type=int, default=0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", choices=["place", "all"], default="all", help="place: the place-recognition shapes alone (for a kernel trace)")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    mt = pkg.ORBmatcher(0.9)
    bp = bow_pool(mt, 37, 4000)
    ok = measure_m8(mt, bp, "place36", [0] * 36, list(range(1, 37)), a.reps, a.out)
    one = TR.synth_pool(pkg, rng, [1500], 1536)
    ok &= measure_m6(one, "place6", [0] * 6, 3000, a.reps, a.out, rng)
    if a.only == "all":
        for P in (8, 64, 512):
            ok &= measure_m8(mt, bp, "x%d" % P, [i % bp.rows for i in range(P)], [(i * 7 + 1) % bp.rows for i in range(P)], a.reps, a.out)
        many = TR.synth_pool(pkg, rng, [1500] * 64, 1536)
        for P in (8, 64, 512):
            ok &= measure_m6(many, "x%d" % P, [i % 64 for i in range(P)], 1000, a.reps, a.out, rng)
    bad = 0
    if a.fuzz:
        OM = orbref._oracle_matcher_class()()
        f8, f6 = fuzz_m8(mt, bp, a.fuzz, rng, OM), fuzz_m6(a.fuzz, rng, OM)
        bad = f8["mismatches"] + f6["mismatches"]
        _emit(dict(path="fuzz", seed=a.seed, m8=f8, m6=f6, mismatches=bad), a.out)
    sys.exit(0 if ok and not bad else 1)


if __name__ == "__main__":
    main()
