"""SearchForTriangulation_ (M10) for a batch of KeyFrame pairs: orbm_search_for_triangulation_batch_async against a loop of host
orbm_search_for_triangulation calls over the same pairs, and against orbm_triangulation_batch_async on that entry's own shape.

Shapes at 752 x 480 / 1200 features (rectified synthetic stereo scenes, buckets from desc[:, 0] & 63, per pair F12 / epipole of a
sideways motion):
- mono:   one KeyFrame against 20 neighbour rows, no stereo feature;
- stereo: one KeyFrame against 10 neighbour rows, 60 % of the features stereo on both sides;
each with has_mp shares 0 and 0.7 on both sides.  (a) the batched call: device events of the handle (orbm_last_timing) and the host
clock around enqueue + sync, 5 warm-up calls, then the median of REPS calls with min / max / the inter-quartile range; (b) the host loop,
one orbm_search_for_triangulation per pair on host FeatureVectors; (c) the old entry against the new one on the old one's shape (256
pairs, row p against row p, one F12, no MapPoints), interleaved in one process.  All paths must produce the same rows.
--variants: with the -DORBX_AB library (ORB_LIB) the search kernel's lanes-per-feature variants (16 / 4 / 1) are timed interleaved in one
process (ORBM_TRI_LPF is read per call by that build only).  Prints one JSON line per measurement.

--fuzz N: N random calls (pool shapes, caps, has_mp / stereo / stopped-word shares, flags, rows out of range, empty rows, per pair
geometry including rotations, bits 2..9) compared pair by pair with the host entry point and the oracle; one JSON line with the
mismatch count."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pkg = importlib.import_module("orb-slam3_amd")
synth = importlib.import_module("orb-slam3_amd.synth")

W, H, REPS = 752, 480, 30
K_CAM = (435.2, 435.2, 367.2, 252.2)
NAME = "orbm_search_for_triangulation_batch_async"


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def fv(nodes, keep):
    idx = np.flatnonzero(keep).astype(np.int32)
    order = idx[np.argsort(nodes[idx], kind="stable")]
    un, start = np.unique(nodes[order], return_index=True)
    return un.astype(np.int32), np.append(start, len(order)).astype(np.int32), order.astype(np.int32)


def fundamental(k1, k2, R12, t12):
    def kinv(k):
        fx, fy, cx, cy = k
        return np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], np.float64)
    t = np.asarray(t12, np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)
    return (kinv(k1).T @ tx @ np.asarray(R12, np.float64) @ kinv(k2)).astype(np.float32).reshape(9)


def levels(n=8, f=1.2):
    sf = np.cumprod(np.concatenate([[np.float32(1)], np.full(n - 1, np.float32(f))]).astype(np.float32)).astype(np.float32)
    return sf, (sf * sf).astype(np.float32)


class Pool:
    """Rows of cap slots on the device with their host copies (slots beyond a row's count repeat slot 0: garbage that would match)."""

    def __init__(self, rows, cap, bits, mp_share, stereo_share, stop_share, rng):
        self.rows, self.cap, self.n = len(rows), cap, [min(len(k), cap) for k, _ in rows]
        self.k = np.zeros((self.rows, cap), pkg.KP_DTYPE); self.d = np.zeros((self.rows, cap, 32), np.uint8)
        for r, (k, d) in enumerate(rows):
            n = self.n[r]
            if n:
                self.k[r, :] = k[0]; self.d[r, :] = d[0]; self.k[r, :n] = k[:n]; self.d[r, :n] = d[:n]
        self.node = (self.d[:, :, 0].astype(np.int32) & ((1 << bits) - 1)).astype(np.int32)
        self.mp = (rng.random((self.rows, cap)) < mp_share).astype(np.uint8)
        self.ur = None if stereo_share is None else np.where(rng.random((self.rows, cap)) < stereo_share, 5.0, -1.0).astype(np.float32)
        self.w = None if stop_share is None else np.where(rng.random((self.rows, cap)) < stop_share, 0.0, 1.5)
        up = lambda a: pkg.DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a))
        self.dk, self.dd, self.dn, self.dm, self.dc = up(self.k), up(self.d), up(self.node), up(self.mp), up(np.asarray(self.n, np.int32))
        self.du = None if self.ur is None else up(self.ur)
        self.dw = None if self.w is None else up(self.w)

    def args(self):
        return (self.rows, self.cap, self.dk.ptr, self.dd.ptr, self.dc.ptr, self.dn.ptr, None if self.dw is None else self.dw.ptr, self.dm.ptr,
                None if self.du is None else self.du.ptr)

    def host(self, r):
        n = self.n[r]
        keep = np.ones(n, bool) if self.w is None else self.w[r, :n] > 0
        return (np.ascontiguousarray(self.k[r, :n]), np.ascontiguousarray(self.d[r, :n]), np.ascontiguousarray(self.mp[r, :n]),
                None if self.ur is None else np.ascontiguousarray(self.ur[r, :n]), fv(self.node[r, :n], keep))


class Call:
    def __init__(self, m, A, B, row1, row2, F, ep, sf, sig, nlevels=8, only_stereo=0, coarse=0, check_ori=0):
        self.L, self.m, self.A, self.B, self.P = pkg.lib(), m, A, B, len(F)
        self.row1, self.row2, self.F, self.ep, self.sf, self.sig = row1, row2, F, ep, sf, sig
        self.flags = (nlevels, int(only_stereo), int(coarse), int(check_ori))
        self.d1 = None if row1 is None else pkg.DeviceBuffer(4 * self.P).upload(np.asarray(row1, np.int32))
        self.d2 = None if row2 is None else pkg.DeviceBuffer(4 * self.P).upload(np.asarray(row2, np.int32))
        self.dF = pkg.DeviceBuffer(36 * self.P).upload(np.ascontiguousarray(F, np.float32))
        self.de = pkg.DeviceBuffer(8 * self.P).upload(np.ascontiguousarray(ep, np.float32))
        self.mm = pkg.DeviceBuffer(4 * self.P * A.cap); self.nm = pkg.DeviceBuffer(4 * self.P)

    def enqueue(self):
        rc = getattr(self.L, NAME)(self.m.h, self.P, *self.A.args(), *self.B.args(), None if self.d1 is None else self.d1.ptr,
                                   None if self.d2 is None else self.d2.ptr, self.dF.ptr, self.de.ptr, _p(self.sf), _p(self.sig), *self.flags,
                                   self.mm.ptr, self.nm.ptr)
        assert rc == 0, self.L.orbm_last_error()

    def result(self):
        self.m.sync()
        return self.mm.download(np.int32, self.P * self.A.cap).reshape(self.P, self.A.cap), self.nm.download(np.int32, self.P)

    def host_args(self, p):
        r1 = p if self.row1 is None else int(self.row1[p]); r2 = p if self.row2 is None else int(self.row2[p])
        if not (0 <= r1 < self.A.rows and 0 <= r2 < self.B.rows) or self.A.n[r1] == 0 or self.B.n[r2] == 0:
            return None
        k1, d1, m1, u1, f1 = self.A.host(r1); k2, d2, m2, u2, f2 = self.B.host(r2)
        return (k1, d1, m1, u1, f1, k2, d2, m2, u2, f2, self.F[p], (float(self.ep[p][0]), float(self.ep[p][1])), self.sf, self.sig,
                bool(self.flags[1]), bool(self.flags[2]), bool(self.flags[3]))

    def mismatches(self, rows, counts, matchers):
        bad = total = 0
        for p in range(self.P):
            a = self.host_args(p)
            if a is None:
                ok = counts[p] == 0 and np.all(rows[p] == -1)
            else:
                ok = True
                for M in matchers:
                    n, row = M.SearchForTriangulation(*a)
                    ok = ok and counts[p] == n and np.array_equal(rows[p, :len(row)], row) and np.all(rows[p, len(row):] == -1)
                total += n
            bad += int(not ok)
        return bad, total


def stats(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()), iqr=float(np.percentile(x, 75) - np.percentile(x, 25)))


def timed(call, m, reps=REPS, warm=5):
    for _ in range(warm):
        call.enqueue()
    m.sync()
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call.enqueue()
        m.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(m.timing_ms())
    return dev, wall


def scene(orbref, seed, nneigh, nf=1200):
    left, _ = synth.gen_stereo_pair(W, H, seed)
    _, k1, d1, _ = orbref.Extractor(nf)(left, (0, 0))
    neigh, F, ep = [], [], []
    for i in range(nneigh):
        _, k2, d2, _ = orbref.Extractor(nf)(synth.gen_stereo_pair(W, H, seed, dmin=2 + i % 12, dmax=40 + 2 * (i % 12))[1], (0, 0))
        neigh.append((k2, d2))
        F.append(fundamental(K_CAM, K_CAM, np.eye(3), (0.11 * (1 + i / 10.0), 0, 0)))
        ep.append((1e4 + 500.0 * i, K_CAM[3]))
    return (k1, d1), neigh, np.stack(F), np.asarray(ep, np.float32)


VARIANTS = [("lpf16", {"ORBM_TRI_LPF": "16"}), ("lpf4", {"ORBM_TRI_LPF": "4"}), ("lpf1", {"ORBM_TRI_LPF": "1"})]


def set_variant(env):
    os.environ.pop("ORBM_TRI_LPF", None)
    os.environ.update(env)


def bench(variants):
    import orbref
    orbref.lib()
    OM = orbref._oracle_matcher_class()()
    L = pkg.lib()
    m = pkg.ORBmatcher(0.6)
    sf, sig = levels()
    kf, neigh, F, ep = scene(orbref, 100, 20)
    for shape, P, stereo in (("mono_1x20", 20, None), ("stereo_1x10", 10, 0.6)):
        for share in (0.0, 0.7):
            rng = np.random.default_rng(17)
            A = Pool([kf], 1500, 6, share, stereo, None, rng); B = Pool(neigh[:P], 1500, 6, share, stereo, None, rng)
            call = Call(m, A, B, [0] * P, list(range(P)), F[:P], ep[:P], sf, sig)
            call.enqueue()
            rows, counts = call.result()
            bad, total = call.mismatches(rows, counts, [m, OM])
            assert bad == 0, "batched rows differ from the host / oracle rows"
            if variants:
                res = {name: [] for name, _ in VARIANTS}
                for rnd in range(6):                                        # interleaved rounds in one process
                    for name, env in VARIANTS:
                        set_variant(env)
                        dev, _ = timed(call, m, reps=10, warm=2)
                        res[name] += dev
                        r2, c2 = call.result()
                        assert np.array_equal(r2, rows) and np.array_equal(c2, counts), name
                set_variant({})
                for name, _ in VARIANTS:
                    print(json.dumps(dict(path="variant", variant=name, shape=shape, has_mp_share=share, pairs=P, matches=int(total),
                                          device_ms=stats(res[name]))), flush=True)
                continue
            dev, wall = timed(call, m)
            print(json.dumps(dict(path="batch", shape=shape, has_mp_share=share, pairs=P, matches=int(total), device_ms=stats(dev), wall_ms=stats(wall),
                                  device_ms_per_pair=float(np.median(dev)) / P)), flush=True)
            args = [call.host_args(p) for p in range(P)]
            for a in args:
                m.SearchForTriangulation(*a)                                # warm-up pass
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                for a in args:
                    m.SearchForTriangulation(*a)
                t.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps(dict(path="host_loop", shape=shape, has_mp_share=share, pairs=P, wall_ms_per_batch=stats(t),
                                  batch_wall_speedup=float(np.median(t) / np.median(wall)), rows_equal_batch=True)), flush=True)
    if variants:
        m.close()
        return
    # (c) the old entry's own shape at the C3 batch: 256 pairs, row p against row p, one F12, no MapPoints, NULL weights
    P, cap = 256, 1500
    rng = np.random.default_rng(3)
    A = Pool([kf] * P, cap, 6, 0.0, 0.6, None, rng); B = Pool([neigh[p % 20] for p in range(P)], cap, 6, 0.0, None, None, rng)
    new = Call(m, A, B, None, None, np.stack([F[0]] * P), np.stack([ep[0]] * P), sf, sig)
    mm = pkg.DeviceBuffer(4 * P * cap).upload(np.full(P * cap, -1, np.int32)); nm = pkg.DeviceBuffer(4 * P)

    class Old:
        def enqueue(self):
            rc = L.orbm_triangulation_batch_async(m.h, P, cap, A.dk.ptr, A.dd.ptr, A.dc.ptr, A.dn.ptr, A.du.ptr, B.dk.ptr, B.dd.ptr, B.dc.ptr, B.dn.ptr, None,
                                                  _p(F[0]), float(ep[0][0]), float(ep[0][1]), _p(sf), _p(sig), 8, 0, 0, mm.ptr, nm.ptr)
            assert rc == 0, L.orbm_last_error()
    old = Old()
    old.enqueue(); m.sync()
    new.enqueue()
    rows, counts = new.result()
    assert np.array_equal(mm.download(np.int32, P * cap).reshape(P, cap), rows) and np.array_equal(nm.download(np.int32, P), counts)
    res = {"old": [], "new": []}
    for rnd in range(6):                                                    # the old entry records no device events: host clock for both
        for name, c in (("old", old), ("new", new)):
            res[name] += _wall(c, m)
    print(json.dumps(dict(path="old_vs_new", shape="c3_256_pairs", pairs=P, matches=int(counts.sum()), old_wall_ms=stats(res["old"]),
                          new_wall_ms=stats(res["new"]), new_over_old=float(np.median(res["new"]) / np.median(res["old"])), rows_equal=True)), flush=True)
    m.close()


def _wall(c, m, reps=10, warm=2):
    for _ in range(warm):
        c.enqueue()
    m.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        c.enqueue()
        m.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def rot(rng, deg):
    a = rng.normal(0, 1, 3); a /= np.linalg.norm(a)
    th = np.deg2rad(rng.uniform(-deg, deg))
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def fuzz(n, seed):
    import orbref
    orbref.lib()
    OM = orbref._oracle_matcher_class()()
    rng = np.random.default_rng(seed)
    m = pkg.ORBmatcher(0.6)
    feats = {}

    def features(s, right, nf):
        if (s, right, nf) not in feats:
            img = synth.gen_stereo_pair(W, H, s)[right]
            feats[(s, right, nf)] = orbref.Extractor(nf)(img, (0, 0))[1:3]
        return feats[(s, right, nf)]
    pairs = matches = mismatches = 0
    cases = []
    for c in range(n):
        n1, n2 = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        nf1, nf2 = int(rng.choice([60, 400, 1200])), int(rng.choice([60, 400, 1200, 2000]))
        s0 = int(rng.integers(200, 204))
        rows1 = [features(s0 + (i % 2), 0, nf1) for i in range(n1)]; rows2 = [features(s0 + (i % 2), 1, nf2) for i in range(n2)]
        empty = (rows1[0][0][:0], rows1[0][1][:0])
        if rng.random() < 0.2:
            rows2[int(rng.integers(0, n2))] = empty
        cap1 = max(len(k) for k, _ in rows1) + int(rng.integers(0, 70)); cap2 = max(max(len(k) for k, _ in rows2), 1) + int(rng.integers(0, 70))
        if rng.random() < 0.15:
            cap1 = max(1, cap1 // 2)                                        # a cap below the feature count: the pool simply holds fewer
        bits = int(rng.integers(2, 10))
        sh1, sh2 = float(rng.choice([0.0, 0.5, 0.9])), float(rng.choice([0.0, 0.5, 0.9]))
        stereo = None if rng.random() < 0.4 else float(rng.choice([0.3, 0.7]))
        stop = None if rng.random() < 0.5 else 0.1
        A = Pool(rows1, cap1, bits, sh1, stereo, stop, rng); B = Pool(rows2, cap2, bits, sh2, stereo, stop, rng)
        P = int(rng.integers(1, 13))
        row1 = rng.integers(0, n1, P).astype(np.int32); row2 = rng.integers(0, n2, P).astype(np.int32)
        out = rng.random(P) < 0.1
        row1[out] = rng.choice([-1, n1, n1 + 7], int(out.sum())); row2[rng.random(P) < 0.05] = -2
        F, ep = [], []
        for p in range(P):
            kind = int(rng.integers(0, 3))
            if kind == 0:                                                   # the rectified geometry: rows are the epipolar lines
                F.append(fundamental(K_CAM, K_CAM, np.eye(3), (rng.uniform(0.05, 0.3), 0, 0))); ep.append((np.inf, np.inf) if rng.random() < 0.5 else (1e4, 240.0))
            else:                                                           # a small rotation and a general translation
                R = rot(rng, 3.0 if kind == 1 else 25.0); t = rng.normal(0, 0.1, 3) + np.array([0.11, 0, 0.02])
                F.append(fundamental(K_CAM, K_CAM, R, t))
                ep.append((K_CAM[0] * t[0] / t[2] + K_CAM[2], K_CAM[1] * t[1] / t[2] + K_CAM[3]))
        flags = dict(only_stereo=int(rng.random() < 0.25), coarse=int(rng.random() < 0.3), check_ori=int(rng.random() < 0.5))
        sf, sig = levels()
        use_rows = rng.random() < 0.85 or P > min(n1, n2)
        call = Call(m, A, B, row1 if use_rows else None, row2 if use_rows else None, np.stack(F), np.asarray(ep, np.float32), sf, sig, **flags)
        call.enqueue()
        rows, counts = call.result()
        bad, total = call.mismatches(rows, counts, [m, OM])
        pairs += P; matches += total; mismatches += bad
        cases.append(dict(pairs=P, rows1=n1, rows2=n2, cap1=cap1, cap2=cap2, bits=bits, has_mp=[sh1, sh2], stereo=stereo, stopped=stop,
                          null_rows=not use_rows, matches=int(total), mismatched_pairs=bad, **flags))
    print(json.dumps(dict(path="fuzz", seed=seed, calls=n, pairs=pairs, matches=int(matches), mismatches=mismatches, cases=cases)), flush=True)
    m.close()
    return mismatches


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fuzz", type=int, default=0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--variants", action="store_true")
    a = ap.parse_args()
    if a.fuzz:
        sys.exit(1 if fuzz(a.fuzz, a.seed) else 0)
    bench(a.variants)
