"""TrackWithMotionModel (M4) for a batch of frame pairs: orbm_project_last_frame_batch_async + orbm_search_by_projection_frame_batch_async
against a loop of orbm_search_by_projection_frame_resident over the same pairs and queries.

64 pairs of 752 x 480 / 1000 features: pair p searches frame p with ~1000 MapPoints back-projected from frame p's keypoints under
a small pose change (descriptors with a few flipped bits), so most queries match.  Project + search are timed with the handle's
device events (orbm_last_timing: the search's kernels) and with the host clock around enqueue + sync, at th 15 (mono) and at th 7
with the stereo gate; the resident path is a host-clock loop of one call per pair fed with the downloaded projections.  All paths
must produce the same rows.  Prints one JSON line per measurement.

--fuzz N: N random calls (sizes, th 5-70, dir, blocked and observed rates, stereo on or off, rotation check, retry) compared row by
row with the host entry point (ORBmatcher.SearchByProjectionFrame); prints one JSON line with the mismatch count."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("orb-slam3_amd")
synth = importlib.import_module("orb-slam3_amd.synth")
from test_motion_projection_cpu import random_pose  # noqa: E402

W, H, NB, REPS = 752, 480, 64, 20
INV_W, INV_H = float(np.float32(64) / np.float32(W)), float(np.float32(48) / np.float32(H))
K = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
BOUNDS = np.array([0.0, W, 0.0, H], np.float32)
MBF = 47.90639384423901
MB = MBF / 435.2046959714599
vp = lambda a: a.ctypes.data_as(C.c_void_p)


class Rows:
    F = (("valid", np.uint8), ("u", np.float32), ("v", np.float32), ("invzc", np.float32), ("octave", np.int32), ("angle", np.float32),
         ("mp_obs", np.uint8))

    def __init__(self, npairs, qs):
        self.np_, self.qs = npairs, qs
        self.b = {n: pkg.DeviceBuffer(npairs * qs * np.dtype(t).itemsize) for n, t in self.F}
        self.b["qdesc"] = pkg.DeviceBuffer(npairs * qs * 32)
        self.b["nq"] = pkg.DeviceBuffer(4 * npairs)
        self.b["dir"] = pkg.DeviceBuffer(max(npairs, 4))

    def upload(self, Q, dirs):
        self.b["nq"].upload(np.array([len(q["octave"]) for q in Q], np.int32))
        for n, t in self.F + (("qdesc", np.uint8),):
            if n not in Q[0]:
                continue
            shape = (self.np_, self.qs, 32) if n == "qdesc" else (self.np_, self.qs)
            a = np.zeros(shape, t)
            for p, q in enumerate(Q):
                a[p, :len(q[n])] = q[n]
            self.b[n].upload(a)
        self.b["dir"].upload(np.asarray(list(dirs) + [0] * (max(self.np_, 4) - len(dirs)), np.uint8))

    def get(self, n, t):
        return self.b[n].download(t, self.np_ * self.qs).reshape(self.np_, self.qs)


def search(L, m, r, cap, gs, gi, t_first, rows, sf, nlev, th, dm, dn, ur=None, blk=None, retry_below=0, dr=None, check_ori=1):
    b = rows.b
    rc = L.orbm_search_by_projection_frame_batch_async(
        m.h, r["kps"], r["desc"], r["counts"], cap, gs.ptr, gi.ptr, 0.0, 0.0, INV_W, INV_H, t_first, rows.np_,
        None if ur is None else ur.ptr, MBF, None if blk is None else blk.ptr, b["dir"].ptr, b["nq"].ptr, rows.qs, b["valid"].ptr,
        b["u"].ptr, b["v"].ptr, b["invzc"].ptr, b["octave"].ptr, b["angle"].ptr, b["qdesc"].ptr, b["mp_obs"].ptr, float(th), int(retry_below),
        vp(sf), nlev, int(check_ori), dm.ptr, dn.ptr, None if dr is None else dr.ptr)
    assert rc == 0, L.orbm_last_error()


def flip(rng, d, nmax):
    d = d.copy()
    for j in range(nmax):
        sel = np.flatnonzero(rng.integers(0, nmax + 1, len(d)) > j); b = rng.integers(0, 256, len(sel))
        d[sel, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return d


def scene(rng, res, p, nq):
    """LastFrame MapPoints of pair p: back-projected from frame p's keypoints through pose `cur` at random depths."""
    kt, dt = res[p][1], res[p][2]
    src = rng.integers(0, len(kt), nq) if len(kt) else np.zeros(0, np.int64)
    cur = random_pose(rng, 0.002, 0.01)
    z = rng.uniform(1.0, 12.0, len(src))
    Pc = np.stack([(kt["x"][src] - K[2]) * z / K[0] + rng.normal(0, 0.002, len(src)), (kt["y"][src] - K[3]) * z / K[1], z], 1)
    R, t = cur.reshape(3, 4)[:, :3].astype(np.float64), cur.reshape(3, 4)[:, 3].astype(np.float64)
    X = ((Pc - t) @ R).astype(np.float32)
    ang = np.mod(kt["angle"][src] + rng.normal(0, 2, len(src)), 360).astype(np.float32)
    return cur, X, dict(octave=kt["octave"][src].astype(np.int32), angle=ang, qdesc=flip(rng, dt[src], 6),
                        mp_obs=(rng.random(len(src)) < 0.9).astype(np.uint8))


def host_rows(m, res, p, sf, q, th, blocked, d, ur, check_ori, mbf=MBF):
    kt, dt = res[p][1], res[p][2]
    valid = q["valid"]
    octv = np.where(valid != 0, q["octave"], 0).astype(np.int32)
    u = None if ur is None else np.ascontiguousarray(ur[:len(kt)])
    return m.SearchByProjectionFrame(pkg.FrameView(kt, dt, W, H, uright=u, backend=m), cur_blocked=blocked[:len(kt)], scale_factors=sf,
                                     valid=valid, u=q["u"], v=q["v"], invzc=q["invzc"], octave=octv, angle=q["angle"], qdesc=q["qdesc"],
                                     mp_obs=q["mp_obs"], th=th, forward=d == 1, backward=d == 2, mbf=mbf if ur is not None else 0.0,
                                     check_ori=check_ori)


def bench():
    imgs = [synth.gen_image(W, H, 500 + i) for i in range(NB)]
    ex = pkg.ORBextractor(1000, max_size=(W, H), max_batch=NB)
    res = ex.extract_batch(imgs, [(0, 1000)] * NB)
    r = ex.result_device(); cap = r["cap"]; sf = ex.GetScaleFactors()
    L = pkg.lib()
    mg, m = pkg.ORBmatcher(0.9), pkg.ORBmatcher(0.9)          # grid and projection on their own handle: m's event span is the search alone
    gs = pkg.DeviceBuffer(NB * 3073 * 4); gi = pkg.DeviceBuffer(NB * cap * 4)
    assert L.orbm_grid_build_batch_async(mg.h, r["kps"], r["counts"], NB, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0
    mg.sync()
    rng = np.random.default_rng(1)
    NQ = 1000
    cur, last, X, has = np.zeros((NB, 12), np.float32), np.zeros((NB, 12), np.float32), np.zeros((NB, NQ, 3), np.float32), np.zeros((NB, NQ), np.uint8)
    Q = []
    for p in range(NB):
        cur[p], Xp, q = scene(rng, res, p, NQ)
        last[p] = cur[p]; last[p, 11] -= np.float32(0.2 if p % 2 else -0.2)
        X[p, :len(Xp)] = Xp; has[p, :len(Xp)] = 1
        Q.append(q)
    rows = Rows(NB, NQ)
    rows.upload(Q, [0] * NB)
    dcur, dlast, dX, dhas = (pkg.DeviceBuffer(a.nbytes).upload(a) for a in (cur, last, X, has))
    blocked = (rng.random((NB, cap)) < 0.05).astype(np.uint8)
    dblk = pkg.DeviceBuffer(blocked.nbytes).upload(blocked)
    ur_h = np.full((NB, cap), -1, np.float32)
    for p in range(NB):
        k = res[p][1]
        ur_h[p, :len(k)] = np.where(rng.random(len(k)) < 0.6, k["x"] - rng.uniform(1, 43, len(k)), -1)
    dur = pkg.DeviceBuffer(ur_h.nbytes).upload(ur_h)
    dm = pkg.DeviceBuffer(NB * cap * 4); dn = pkg.DeviceBuffer(NB * 4)
    frames = [pkg.ResidentFrame(m, device=dict(kps=r["kps"] + p * cap * 28, desc=r["desc"] + p * cap * 32, n=len(res[p][1])),
                                uright=dur.ptr + p * cap * 4, width=W, height=H) for p in range(NB)]
    frames_mono = [pkg.ResidentFrame(m, device=dict(kps=r["kps"] + p * cap * 28, desc=r["desc"] + p * cap * 32, n=len(res[p][1])),
                                     width=W, height=H) for p in range(NB)]
    for th, mono, ur in ((15.0, True, None), (7.0, False, dur)):
        b = rows.b

        def call():
            assert L.orbm_project_last_frame_batch_async(m.h, NB, dcur.ptr, dlast.ptr, b["nq"].ptr, NQ, dX.ptr, dhas.ptr, vp(K), vp(BOUNDS), MB,
                                                         int(mono), b["valid"].ptr, b["u"].ptr, b["v"].ptr, b["invzc"].ptr, b["dir"].ptr) == 0
            search(L, m, r, cap, gs, gi, 0, rows, sf, 8, th, dm, dn, ur=ur, blk=dblk)

        for _ in range(3):
            call()
        m.sync()
        dev_ms, wall_ms = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            call()
            m.sync()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(m.timing_ms())
        match = dm.download(np.int32, NB * cap).reshape(NB, cap); nm = dn.download(np.int32, NB)
        valid, u, v, iz = rows.get("valid", np.uint8), rows.get("u", np.float32), rows.get("v", np.float32), rows.get("invzc", np.float32)
        dirs = rows.b["dir"].download(np.uint8, NB)
        print(json.dumps(dict(path="batch", pairs=NB, queries_per_pair=NQ, valid_per_pair=float(valid.sum()) / NB, th=th, stereo=ur is not None,
                              search_device_ms_per_call=float(np.median(dev_ms)), search_device_ms_per_pair=float(np.median(dev_ms)) / NB,
                              project_search_wall_ms_per_call=float(np.median(wall_ms)), matches=int(nm.sum()),
                              dirs=[int((dirs == d).sum()) for d in (0, 1, 2)])), flush=True)
        fr = frames if ur is not None else frames_mono
        args = lambda p: dict(cur_blocked=blocked[p, :len(res[p][1])], scale_factors=sf, valid=valid[p], u=u[p], v=v[p], invzc=iz[p],
                              octave=np.where(valid[p] != 0, Q[p]["octave"], 0).astype(np.int32), angle=Q[p]["angle"], qdesc=Q[p]["qdesc"],
                              mp_obs=Q[p]["mp_obs"], th=th, forward=dirs[p] == 1, backward=dirs[p] == 2, mbf=MBF if ur is not None else 0.0)
        out = [m.SearchByProjectionFrameResident(fr[p], **args(p)) for p in range(NB)]     # warm-up pass
        same = all(int(nm[p]) == out[p][0] and np.array_equal(match[p, :len(res[p][1])], out[p][1]) for p in range(NB))
        host = [host_rows(m, res, p, sf, dict(Q[p], valid=valid[p], u=u[p], v=v[p], invzc=iz[p]), th, blocked[p], int(dirs[p]),
                          None if ur is None else ur_h[p], True) for p in range(NB)]
        same_host = all(int(nm[p]) == host[p][0] and np.array_equal(match[p, :len(res[p][1])], host[p][1]) for p in range(NB))
        t0 = time.perf_counter()
        for _ in range(3):
            for p in range(NB):
                m.SearchByProjectionFrameResident(fr[p], **args(p))
        per_call = (time.perf_counter() - t0) * 1e3 / (3 * NB)
        print(json.dumps(dict(path="resident_loop", pairs=NB, queries_per_pair=NQ, th=th, stereo=ur is not None, wall_ms_per_call=per_call,
                              wall_ms_per_batch=per_call * NB, rows_equal_batch=bool(same), host_rows_equal_batch=bool(same_host))), flush=True)
        assert same and same_host, "batched rows differ from the resident / host rows"
    for f in frames + frames_mono:
        f.close()


def fuzz(n, seed):
    rng = np.random.default_rng(seed)
    L = pkg.lib()
    m = pkg.ORBmatcher(0.9)
    mismatches, pairs, matches, retries = 0, 0, 0, 0
    cases = []
    for it in range(n):
        nb = int(rng.integers(1, 7))
        nfeat = int(rng.choice([50, 300, 1000, 2500]))
        ex = pkg.ORBextractor(nfeat, max_size=(W, H), max_batch=nb)
        imgs = [synth.gen_image(W, H, 9000 + 17 * it + i) if rng.random() > 0.1 else np.full((H, W), 128, np.uint8) for i in range(nb)]
        res = ex.extract_batch(imgs, [(0, 1000)] * nb)
        r = ex.result_device(); cap = r["cap"]; sf = ex.GetScaleFactors()
        gs = pkg.DeviceBuffer(nb * 3073 * 4); gi = pkg.DeviceBuffer(nb * cap * 4)
        assert L.orbm_grid_build_batch_async(m.h, r["kps"], r["counts"], nb, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0
        th = float(rng.uniform(5, 70)); stereo = rng.random() < 0.5; check_ori = int(rng.random() < 0.7)
        brate, orate, vrate = float(rng.choice([0, 0.35, 0.97])), float(rng.choice([0, 0.5, 1])), float(rng.uniform(0.5, 1))
        retry_below = int(rng.choice([0, 0, 20, 200]))
        Q, dirs = [], rng.integers(0, 4, nb).astype(np.uint8)
        for p in range(nb):
            kt, dt = res[p][1], res[p][2]
            nq = int(rng.integers(0, 2 * max(len(kt), 1) + 1)) if len(kt) else int(rng.integers(0, 50))
            src = rng.integers(0, max(len(kt), 1), nq)
            base = kt if len(kt) else res[0][1] if len(res[0][1]) else None
            if base is None or len(base) == 0:
                q = dict(valid=np.zeros(nq, np.uint8), u=np.zeros(nq, np.float32), v=np.zeros(nq, np.float32), invzc=np.zeros(nq, np.float32),
                         octave=np.zeros(nq, np.int32), angle=np.zeros(nq, np.float32), qdesc=np.zeros((nq, 32), np.uint8), mp_obs=np.zeros(nq, np.uint8))
            else:
                src = rng.integers(0, len(base), nq)
                db = dt if len(kt) else res[0][2]
                q = dict(valid=(rng.random(nq) < vrate).astype(np.uint8),
                         u=(base["x"][src] + rng.normal(0, 3, nq)).astype(np.float32), v=(base["y"][src] + rng.normal(0, 3, nq)).astype(np.float32),
                         invzc=rng.uniform(0.01, 1.0, nq).astype(np.float32),
                         octave=np.clip(base["octave"][src] + rng.integers(-1, 2, nq), 0, 7).astype(np.int32),
                         angle=np.mod(base["angle"][src] + rng.normal(10, 8, nq), 360).astype(np.float32),
                         qdesc=flip(rng, db[src], int(rng.integers(0, 30))), mp_obs=(rng.random(nq) < orate).astype(np.uint8))
            Q.append(q)
        qs = max(1, max(len(q["u"]) for q in Q)) + int(rng.integers(0, 9))
        rows = Rows(nb, qs)
        rows.upload(Q, dirs)
        blocked = (rng.random((nb, cap)) < brate).astype(np.uint8)
        dblk = pkg.DeviceBuffer(blocked.nbytes).upload(blocked)
        ur_h, dur = None, None
        if stereo:
            ur_h = np.full((nb, cap), -1, np.float32)
            for p in range(nb):
                k = res[p][1]
                ur_h[p, :len(k)] = np.where(rng.random(len(k)) < 0.6, k["x"] - rng.uniform(1, 43, len(k)), -1)
            dur = pkg.DeviceBuffer(ur_h.nbytes).upload(ur_h)
        dm = pkg.DeviceBuffer(nb * cap * 4); dn = pkg.DeviceBuffer(nb * 4); dr = pkg.DeviceBuffer(max(nb, 4))
        search(L, m, r, cap, gs, gi, 0, rows, sf, 8, th, dm, dn, ur=dur, blk=dblk, retry_below=retry_below, dr=dr, check_ori=check_ori)
        m.sync()
        match = dm.download(np.int32, nb * cap).reshape(nb, cap); nm = dn.download(np.int32, nb); rt = dr.download(np.uint8, nb)
        bad = 0
        for p in range(nb):
            kt = res[p][1]
            d = int(dirs[p]) if dirs[p] in (1, 2) else 0
            ur = None if ur_h is None else ur_h[p]
            if len(kt) == 0 or len(Q[p]["u"]) == 0:
                n1, row = 0, np.full(len(kt), -1, np.int32)
            else:
                n1, row = host_rows(m, res, p, sf, Q[p], th, blocked[p], d, ur, check_ori)
            want_retry = retry_below > 0 and n1 < retry_below
            if want_retry and len(kt) and len(Q[p]["u"]):
                n1, row = host_rows(m, res, p, sf, Q[p], 2 * th, np.zeros(cap, np.uint8), d, ur, check_ori)
            ok = int(nm[p]) == n1 and np.array_equal(match[p, :len(kt)], row) and np.all(match[p, len(kt):] == -1) and rt[p] == int(want_retry)
            bad += 0 if ok else 1
            pairs += 1; matches += n1; retries += int(want_retry)
        mismatches += bad
        cases.append(dict(pairs=nb, nfeatures=nfeat, th=round(th, 2), stereo=bool(stereo), check_ori=check_ori, blocked=brate, observed=orate,
                          retry_below=retry_below, dirs=dirs.tolist(), mismatched_pairs=bad))
        ex.close()
    print(json.dumps(dict(path="fuzz", seed=seed, calls=n, pairs=pairs, matches=matches, retried_pairs=retries, mismatches=mismatches,
                          cases=cases)), flush=True)
    return mismatches


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fuzz", type=int, default=0)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    if a.fuzz:
        sys.exit(1 if fuzz(a.fuzz, a.seed) else 0)
    bench()
