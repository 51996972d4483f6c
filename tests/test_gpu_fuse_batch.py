"""M13 Fuse batched on the device (orbm_fuse_batch_async): for every (KeyFrame row, query row) pair, best_idx, nfused and level_out equal,
entry for entry, (a) the host entry point ORBmatcher.Fuse on a FrameView of that KeyFrame row and (b) the oracle's Fuse, both fed by
fuse_project_np (tests/test_fuse_projection_cpu.py, pinned bit for bit to the facade's Fuse lines).  The KeyFrame pool is one extractor
result block of right views of synthetic stereo scenes; the MapPoints are the left views' keypoints back-projected at depth bf / disparity.

The host and oracle searches are per query, so every pair on one KeyFrame row is checked in ONE call on the concatenated queries.
Queries whose log(ratio) / logScaleFactor lies within 1e-4 of an integer (the documented PredictScale caveat) are cleared from valid."""
import ctypes as C

import numpy as np
import pytest

from test_fuse_projection_cpu import F32, _cases, camera_centre_np, fuse_project_np, near_integer_level, random_pose

pytestmark = pytest.mark.gpu

W, H = 752, 480
INV_W, INV_H = float(F32(64) / F32(W)), float(F32(48) / F32(H))
KCAM = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
BOUNDS = np.array([0, W, 0, H], np.float32)
BF = F32(47.90639384423901)
NLEV = 8
LOG_SF = F32(np.log(1.2))
NB = 10


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(pkg, a):
    a = np.ascontiguousarray(a)
    return pkg.DeviceBuffer(max(a.nbytes, 4)).upload(a)


def scene_pose(s):
    """KeyFrame row s: a yaw of 36 degrees per row, so that another row's MapPoints rarely land on its features."""
    a = np.deg2rad(36.0 * s)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.05 * s, -0.02 * s, 0.1 * s])
    return np.concatenate([R, t[:, None]], 1).astype(F32).reshape(12)


def perturb(rng, tcw, ang=0.001, trans=0.003):
    """A slightly different pose (a new KeyFrame of the neighbourhood): small rotation and translation on top of tcw."""
    D = random_pose(rng, ang, trans).reshape(3, 4).astype(np.float64)
    T = np.asarray(tcw, F32).reshape(3, 4).astype(np.float64)
    return np.concatenate([D[:, :3] @ T[:, :3], (D[:, :3] @ T[:, 3] + D[:, 3])[:, None]], 1).astype(F32).reshape(12)


def stereo_scenes(synth, nb, seed):
    """nb synthetic stereo pairs and the disparity fields gen_stereo_pair drew (right(x) = left(x + d(x)))."""
    pairs = [synth.gen_stereo_pair(W, H, seed + s) for s in range(nb)]
    disp = []
    for s in range(nb):
        rng = np.random.default_rng(seed + s + 7919)
        disp.append(synth._upsample(rng.uniform(2, 40, (4, 5)), W, H))
    return pairs, disp


def _field(d, x, y):
    return d[np.clip(np.asarray(y).astype(int), 0, H - 1), np.clip(np.asarray(x).astype(int), 0, W - 1)]


def mappoints(lefts, disp, sf, rng):
    """MapPoints of every scene from its left view's keypoints / descriptors (lefts[s] = (kps, desc)): the point seen by the right camera
    of scene s at depth bf / disparity (x_R solves x_R + d(x_R) = x_L), placed in the world by scene_pose(s); normal up to ~50 degrees off
    the viewing ray; mfMaxDistance = dist * scale[octave] * 1.2^-(0.2 .. 0.8), so that the predicted level is the octave and away from
    the PredictScale caveat, mfMinDistance = max / scale[nlevels - 1].  Returns pw, normal, min_dist, max_dist, qdesc and per scene its
    (offset, count) in the row."""
    b = float(BF) / float(KCAM[0])
    pw, nrm, mn, mx, qd, block = [], [], [], [], [], []
    off = 0
    for s, (kl, dl) in enumerate(lefts):
        u, v = kl["x"].astype(np.float64), kl["y"].astype(np.float64)
        xr = u - _field(disp[s], u, v)
        for _ in range(6):
            xr = u - _field(disp[s], xr, v)
        z = float(BF) / np.maximum(u - xr, 1.0)
        Xr = np.stack([(u - KCAM[2]) * z / KCAM[0] - b, (v - KCAM[3]) * z / KCAM[1], z], 1)
        T = scene_pose(s).reshape(3, 4).astype(np.float64)
        Xw = (Xr - T[:, 3]) @ T[:, :3]                                        # R^T (Xr - t)
        Ow = camera_centre_np(scene_pose(s))[0].astype(np.float64)
        ray = Xw - Ow
        dist = np.linalg.norm(ray, axis=1)
        tilt = rng.normal(0, 0.3, (len(u), 3))
        n_ = ray / dist[:, None] + tilt - (np.sum(tilt * ray, 1) / dist ** 2)[:, None] * ray
        n_ /= np.linalg.norm(n_, axis=1, keepdims=True)
        hi = dist * sf[kl["octave"]] * 1.2 ** (-rng.uniform(0.2, 0.8, len(u)))
        block.append((off, len(u))); off += len(u)
        pw.append(Xw); nrm.append(n_); mx.append(hi); mn.append(hi / sf[NLEV - 1]); qd.append(dl)
    return (np.concatenate(pw).astype(F32), np.concatenate(nrm).astype(F32), np.concatenate(mn).astype(F32),
            np.concatenate(mx).astype(F32), np.concatenate(qd).astype(np.uint8), block)


def kf_uright(kps_rows, disp, cap, rng):
    """mvuRight of the KeyFrame rows (right views): x - d(x) for 60 % of the slots, -1 for the rest."""
    ur = np.full((len(kps_rows), cap), -1, np.float32)
    for s, k in enumerate(kps_rows):
        ur[s, :len(k)] = np.where(rng.random(len(k)) < 0.6, k["x"] - _field(disp[s], k["x"], k["y"]), -1).astype(np.float32)
    return ur


class Scenes:
    """NB stereo scenes: the right views form the KeyFrame pool (device images -> one result block -> grid); the left views' keypoints
    are the MapPoints (mappoints)."""

    def __init__(self, pkg, synth, nb=NB, nfeat=1000, seed=700):
        self.pkg, self.nb, self.L = pkg, nb, pkg.lib()
        pairs, disp = stereo_scenes(synth, nb, seed)
        self.m = pkg.ORBmatcher(0.6)
        self.ex = pkg.ORBextractor(nfeat, max_size=(W, H), max_batch=nb)
        self.stride = (W + 63) // 64 * 64
        self.dimg = pkg.DeviceBuffer(nb * self.stride * H)
        for s in range(nb):
            pad = np.zeros((H, self.stride), np.uint8); pad[:, :W] = pairs[s][1]
            self.dimg.upload(pad, offset=s * self.stride * H)
        self.arr = (C.c_void_p * nb)(*[self.dimg.ptr + s * self.stride * H for s in range(nb)])
        self.extract()
        self.ex.sync()
        self.r = self.ex.result_device(); self.cap = self.r["cap"]
        self.res = self.ex.fetch_all()
        self.gs = pkg.DeviceBuffer(nb * 3073 * 4); self.gi = pkg.DeviceBuffer(nb * self.cap * 4)
        self.grid()
        self.m.sync()
        self.sf = np.ascontiguousarray(self.ex.GetScaleFactors(), np.float32)
        self.isg = np.ascontiguousarray(self.ex.GetInverseScaleSigmaSquares(), np.float32)
        rng = np.random.default_rng(seed)
        self.uright = kf_uright([self.res[s][1] for s in range(nb)], disp, self.cap, rng)
        self.d_uright = _dev(pkg, self.uright)
        exl = pkg.ORBextractor(nfeat, max_size=(W, H))
        lefts = [exl(pairs[s][0], (0, 0))[1:] for s in range(nb)]
        self.pw, self.normal, self.min_dist, self.max_dist, self.qdesc, self.block = mappoints(lefts, disp, self.sf, rng)
        self.Q = len(self.pw)

    @classmethod
    def gathered(cls, pkg, m, kps_ptr, desc_ptr, nrows, cap, gs, gi, sf, isg, uright):
        """A KeyFrame pool the caller laid out and built the grid of (device pointers kps_ptr / desc_ptr of nrows x cap slots, grid
        buffers gs / gi, host tables sf / isg, host uright [nrows][cap]) in place of the extractor block: every field Call reads."""
        S = cls.__new__(cls)
        S.pkg, S.nb, S.L, S.m, S.cap = pkg, nrows, pkg.lib(), m, cap
        S.r = dict(kps=kps_ptr, desc=desc_ptr)
        S.gs, S.gi = gs, gi
        S.sf, S.isg = np.ascontiguousarray(sf, np.float32), np.ascontiguousarray(isg, np.float32)
        S.uright = np.ascontiguousarray(uright, np.float32); S.d_uright = _dev(pkg, S.uright)
        return S

    def extract(self):
        self.ex.enqueue_device(self.arr, W, H, self.stride, np.zeros(4 * self.nb, np.int32))

    def grid(self):
        assert self.L.orbm_grid_build_batch_async(self.m.h, self.r["kps"], self.r["counts"], self.nb, self.cap, 0.0, 0.0, INV_W, INV_H,
                                                  self.gs.ptr, self.gi.ptr) == 0, self.L.orbm_last_error()


@pytest.fixture(scope="module")
def scenes(pkg, synth):
    return Scenes(pkg, synth)


class Call:
    """The device buffers of one orbm_fuse_batch_async call.  Per pair: kf_row, tcw, ow, nq, valid [P][qs]; queries [P][qs] or one
    shared row [qs] (q_shared)."""

    def __init__(self, S, kf_row, tcw, ow, nq, valid, pw, normal, mn, mx, qdesc, shared):
        pkg = S.pkg
        self.S, self.P, self.qs, self.shared = S, len(tcw), valid.shape[1], shared
        self.kf_row = None if kf_row is None else _dev(pkg, np.asarray(kf_row, np.int32))
        self.tcw, self.ow = _dev(pkg, np.asarray(tcw, F32)), _dev(pkg, np.asarray(ow, F32))
        self.nq, self.valid = _dev(pkg, np.asarray(nq, np.int32)), _dev(pkg, np.asarray(valid, np.uint8))
        self.pw, self.normal = _dev(pkg, np.asarray(pw, F32)), _dev(pkg, np.asarray(normal, F32))
        self.mn, self.mx, self.qdesc = _dev(pkg, np.asarray(mn, F32)), _dev(pkg, np.asarray(mx, F32)), _dev(pkg, np.asarray(qdesc, np.uint8))
        self.best = pkg.DeviceBuffer(4 * self.P * self.qs); self.nf = pkg.DeviceBuffer(4 * self.P); self.lvl = pkg.DeviceBuffer(4 * self.P * self.qs)

    def enqueue(self, th, chi2, stereo, **over):
        S = self.S
        a = dict(npairs=self.P, nkf_rows=S.nb, cap=S.cap, kps=S.r["kps"], desc=S.r["desc"], uright=S.d_uright.ptr if stereo else None,
                 gs=S.gs.ptr, gi=S.gi.ptr, kf_row=None if self.kf_row is None else self.kf_row.ptr, tcw=self.tcw.ptr, ow=self.ow.ptr,
                 nq=self.nq.ptr, qs=self.qs, valid=self.valid.ptr, pw=self.pw.ptr, normal=self.normal.ptr, mn=self.mn.ptr, mx=self.mx.ptr,
                 qdesc=self.qdesc.ptr, k=_vp(KCAM), bounds=_vp(BOUNDS), sf=_vp(S.sf), isg=_vp(S.isg), nlev=NLEV, th=th,
                 best=self.best.ptr, nf=self.nf.ptr, lvl=self.lvl.ptr)
        a.update(over)
        return S.L.orbm_fuse_batch_async(S.m.h, a["npairs"], a["nkf_rows"], a["cap"], a["kps"], a["desc"], a["uright"], a["gs"], a["gi"],
                                         0.0, 0.0, INV_W, INV_H, a["kf_row"], a["tcw"], a["ow"], a["nq"], a["qs"], a["valid"],
                                         a["pw"], a["normal"], a["mn"], a["mx"], a["qdesc"], int(self.shared), a["k"], a["bounds"], float(BF),
                                         float(a["th"]), int(chi2), a["sf"], a["isg"], float(LOG_SF), a["nlev"], a["best"], a["nf"], a["lvl"])

    def run(self, th, chi2, stereo):
        rc = self.enqueue(th, chi2, stereo)
        assert rc == 0, self.S.L.orbm_last_error()
        assert self.S.L.orbm_sync(self.S.m.h) == 0
        return self.download()

    def download(self):
        return (self.best.download(np.int32, self.P * self.qs).reshape(self.P, self.qs), self.nf.download(np.int32, self.P),
                self.lvl.download(np.int32, self.P * self.qs).reshape(self.P, self.qs))


def reference(pkg, oracle, S, rows, nq, proj, qdesc, th, chi2, stereo):
    """best [P][qs], nfused [P], level [P][qs] from the host entry point and the oracle (asserted equal), one call per KeyFrame row on
    the concatenated queries of its pairs.  proj = fuse_project_np's (ok, u, v, ur, level) [P][qs]; qdesc [P or 1][qs][32]."""
    ok, u, v, ur, lvl = proj
    P, qs = ok.shape
    best = np.full((P, qs), -1, np.int32); nf = np.zeros(P, np.int32); level = np.full((P, qs), -1, np.int32)
    OM = oracle._oracle_matcher_class()()
    for row in sorted(set(int(r) for r in rows)):
        ps = [p for p in range(P) if int(rows[p]) == row]
        if not (0 <= row < S.nb):
            continue                                                        # out of range: all -1 and 0
        sel = [(p, np.arange(min(max(int(nq[p]), 0), qs))) for p in ps]
        if sum(len(i) for _, i in sel) == 0:
            continue
        cat = lambda a: np.concatenate([a[p, i] for p, i in sel])           # noqa: E731
        d = np.concatenate([qdesc[p if len(qdesc) > 1 else 0][i] for p, i in sel])
        kk, dk = S.res[row][1], S.res[row][2]
        urr = S.uright[row, :len(kk)].copy() if stereo else None
        args = dict(scale_factors=S.sf, inv_sigma2=S.isg, valid=cat(ok), u=cat(u), v=cat(v), ur=cat(ur), level=np.maximum(cat(lvl), 0),
                    qdesc=d, th=th, chi2_gate=bool(chi2))
        n_h, b_h = S.m.Fuse(pkg.FrameView(kk, dk, W, H, uright=urr, backend=S.m), **args)
        n_o, b_o = OM.Fuse(pkg.FrameView(kk, dk, W, H, uright=urr, backend=OM), **args)
        assert n_h == n_o and np.array_equal(b_h, b_o), row
        off = 0
        for p, i in sel:
            best[p, i] = b_o[off:off + len(i)]; level[p, i] = lvl[p, i]; nf[p] = int((best[p, i] >= 0).sum()); off += len(i)
    return best, nf, level


def _check(got, ref):
    (b, n, l), (rb, rn, rl) = got, ref
    assert np.array_equal(l, rl), np.argwhere(l != rl)[:10]
    assert np.array_equal(b, rb), np.argwhere(b != rb)[:10]
    assert np.array_equal(n, rn), (n, rn)


def neighbours_call(S, rng, shared=True):
    """SearchInNeighbors shape: pairs on every KeyFrame row, three rows twice, two out-of-range rows; one shared query row."""
    rows = np.array(list(range(S.nb)) + [0, 3, 7, S.nb, -1], np.int32)
    P = len(rows)
    tcw = np.stack([perturb(rng, scene_pose(int(r) % S.nb)) for r in rows])
    ow = camera_centre_np(tcw)
    valid = (rng.random((P, S.Q)) >= rng.uniform(0.1, 0.3, (P, 1))).astype(np.uint8)
    near = near_integer_level(S.pw[None], S.min_dist[None], S.max_dist[None], tcw, ow, LOG_SF, NLEV)
    valid[near] = 0
    return rows, tcw, ow, valid


@pytest.mark.parametrize("th", [3.0, 4.0])
@pytest.mark.parametrize("chi2", [1, 0])
@pytest.mark.parametrize("stereo", [False, True])
def test_search_in_neighbors_shape(pkg, oracle, scenes, th, chi2, stereo):
    S = scenes
    rng = np.random.default_rng(int(th) * 10 + chi2 * 2 + stereo)
    rows, tcw, ow, valid = neighbours_call(S, rng)
    P = len(rows)
    nq = np.full(P, S.Q, np.int32)
    c = Call(S, rows, tcw, ow, nq, valid, S.pw, S.normal, S.min_dist, S.max_dist, S.qdesc, True)
    got = c.run(th, chi2, stereo)
    proj = fuse_project_np(tcw, ow, S.pw[None], S.normal[None], S.min_dist[None], S.max_dist[None], valid, KCAM, BOUNDS, BF, LOG_SF, NLEV)
    proj[4][(rows < 0) | (rows >= S.nb)] = -1
    ref = reference(pkg, oracle, S, rows, nq, proj, S.qdesc[None], th, chi2, stereo)
    _check(got, ref)
    # not vacuous: the pairs fuse a real share of their own scene's valid MapPoints; out-of-range rows give -1 rows and 0
    own = sum(int(valid[p, S.block[r][0]:S.block[r][0] + S.block[r][1]].sum()) for p, r in enumerate(rows) if 0 <= r < S.nb)
    fused = int(got[1][(rows >= 0) & (rows < S.nb)].sum())
    assert fused > 0.15 * own, (fused, own)
    assert np.all(got[0][P - 2:] == -1) and np.all(got[1][P - 2:] == 0) and np.all(got[2][P - 2:] == -1)
    assert (proj[4] == 0).sum() > 100 and (proj[4] == NLEV - 1).sum() > 10


@pytest.mark.parametrize("sim3", [False, True])
def test_gate_edges(pkg, oracle, scenes, sim3):
    """One query per pair, each with its own pose (per-pair rows): z < 0, the projection exactly on every image bound (minX / minY
    accepted, maxX / maxY rejected), dist3D exactly at 0.8f * min and 1.2f * max, the 60 degree normal boundary, levels 0 and nlevels - 1
    (tests/test_fuse_projection_cpu.py's cases); the Sim3 variant's pose from sim3_pose_np with scales != 1."""
    S = scenes
    rng = np.random.default_rng(5 + sim3)
    n = 3000
    Sc, T, Ow, X, N, mn, mx, hit = _cases(rng, n, KCAM, BOUNDS, sim3)
    assert hit.mean() > 0.8
    rows = (np.arange(n) % S.nb).astype(np.int32)
    valid = np.ones((n, 1), np.uint8)
    valid[near_integer_level(X[:, None], mn[:, None], mx[:, None], T, Ow, LOG_SF, NLEV)] = 0
    qdesc = S.qdesc[rng.integers(0, S.Q, n)][:, None, :]
    c = Call(S, rows, T, Ow, np.ones(n, np.int32), valid, X[:, None], N[:, None], mn[:, None], mx[:, None], qdesc, False)
    got = c.run(4.0, int(not sim3), False)
    proj = fuse_project_np(T, Ow, X[:, None], N[:, None], mn[:, None], mx[:, None], valid, KCAM, BOUNDS, BF, LOG_SF, NLEV)
    _check(got, reference(pkg, oracle, S, rows, np.ones(n), proj, qdesc, 4.0, int(not sim3), False))
    lv = got[2][:, 0]
    assert (lv == 0).sum() > 20 and (lv == NLEV - 1).sum() > 5 and 0.1 * n < (lv >= 0).sum() < 0.9 * n
    ok, u, v = proj[0][:, 0] != 0, proj[1][:, 0], proj[2][:, 0]
    assert np.any(ok & ((u == BOUNDS[0]) | (v == BOUNDS[2])))


def test_per_pair_rows_and_long_row(pkg, oracle, scenes):
    """q_shared = 0: each pair its own query row (its scene's MapPoints plus others), a different nq per pair and garbage in the padding
    (valid set, huge coordinates); then the second loop of SearchInNeighbors: one KeyFrame against >= 20 000 MapPoints; kf_row NULL."""
    S = scenes
    rng = np.random.default_rng(77)
    rows = np.array([0, 1, 2, 5, 5, 9], np.int32)
    P = len(rows)
    nq = np.array([S.block[r][1] + int(rng.integers(0, 200)) for r in rows], np.int32)
    qs = int(nq.max()) + 9
    pw = rng.normal(0, 1e6, (P, qs, 3)).astype(F32); nrm = rng.normal(0, 1, (P, qs, 3)).astype(F32)
    mn = rng.uniform(0, 1, (P, qs)).astype(F32); mx = rng.uniform(1e6, 1e7, (P, qs)).astype(F32)
    qd = rng.integers(0, 256, (P, qs, 32)).astype(np.uint8); valid = np.ones((P, qs), np.uint8)
    tcw = np.stack([perturb(rng, scene_pose(int(r))) for r in rows]); ow = camera_centre_np(tcw)
    for p, r in enumerate(rows):
        o, k = S.block[r]
        src = np.concatenate([np.arange(o, o + k), rng.integers(0, S.Q, nq[p] - k)])
        pw[p, :nq[p]] = S.pw[src]; nrm[p, :nq[p]] = S.normal[src]; mn[p, :nq[p]] = S.min_dist[src]; mx[p, :nq[p]] = S.max_dist[src]
        qd[p, :nq[p]] = S.qdesc[src]
        valid[p, :nq[p]] = rng.random(nq[p]) >= 0.2
    near = near_integer_level(pw, mn, mx, tcw, ow, LOG_SF, NLEV)
    valid[near & (np.arange(qs)[None, :] < nq[:, None])] = 0
    c = Call(S, rows, tcw, ow, nq, valid, pw, nrm, mn, mx, qd, False)
    got = c.run(3.0, 1, True)
    vin = valid * (np.arange(qs)[None, :] < nq[:, None])
    proj = fuse_project_np(tcw, ow, pw, nrm, mn, mx, vin, KCAM, BOUNDS, BF, LOG_SF, NLEV)
    _check(got, reference(pkg, oracle, S, rows, nq, proj, qd, 3.0, 1, True))
    assert np.all(got[0][np.arange(qs)[None, :] >= nq[:, None]] == -1) and got[1].min() > 20
    # one KeyFrame (row 4) x every MapPoint three times, the copies slightly moved
    rep = np.concatenate([S.pw] + [S.pw + rng.normal(0, 1e-3, S.pw.shape).astype(F32) for _ in range(2)]).astype(F32)
    Q2 = len(rep)
    assert Q2 >= 20000
    tcw1 = perturb(rng, scene_pose(4))[None]; ow1 = camera_centre_np(tcw1)
    args = (np.tile(S.normal, (3, 1)), np.tile(S.min_dist, 3), np.tile(S.max_dist, 3), np.tile(S.qdesc, (3, 1)))
    v1 = (rng.random((1, Q2)) >= 0.1).astype(np.uint8)
    v1[near_integer_level(rep[None], args[1][None], args[2][None], tcw1, ow1, LOG_SF, NLEV)] = 0
    c1 = Call(S, np.array([4], np.int32), tcw1, ow1, np.array([Q2], np.int32), v1, rep, args[0], args[1], args[2], args[3], True)
    got1 = c1.run(3.0, 1, False)
    proj1 = fuse_project_np(tcw1, ow1, rep[None], args[0][None], args[1][None], args[2][None], v1, KCAM, BOUNDS, BF, LOG_SF, NLEV)
    _check(got1, reference(pkg, oracle, S, [4], [Q2], proj1, args[3][None], 3.0, 1, False))
    assert got1[1][0] > 200
    # kf_row NULL: pair p reads row p
    c0 = Call(S, None, tcw[:1], ow[:1], nq[:1], valid[:1], pw[:1], nrm[:1], mn[:1], mx[:1], qd[:1], False)
    _check(c0.run(3.0, 1, True), tuple(a[:1] for a in got))


def test_capture_replay_equals_eager(pkg, scenes):
    """The step (KeyFrame extraction, grid, batched Fuse) captured into a graph and replayed gives the eager rows, counts and levels."""
    S = scenes
    L = S.L
    rng = np.random.default_rng(3)
    rows, tcw, ow, valid = neighbours_call(S, rng)
    c = Call(S, rows, tcw, ow, np.full(len(rows), S.Q, np.int32), valid, S.pw, S.normal, S.min_dist, S.max_dist, S.qdesc, True)
    assert L.orbm_set_stream(S.m.h, L.orbx_stream(S.ex.h)) == 0
    try:
        def enqueue():
            S.extract()
            S.grid()
            assert c.enqueue(3.0, 1, True) == 0, L.orbm_last_error()

        enqueue()
        assert L.orbm_sync(S.m.h) == 0
        eager = c.download()
        assert eager[1].sum() > 1000
        assert L.orbx_capture_begin(S.ex.h, 0) == 0, L.orbx_last_error()
        enqueue()
        assert L.orbx_capture_end(S.ex.h) == 0, L.orbx_last_error()
        for buf, n in ((c.best, c.P * c.qs), (c.nf, c.P), (c.lvl, c.P * c.qs)):
            buf.upload(np.full(n, -7, np.int32))
        assert L.orbx_graph_launch(S.ex.h, 0) == 0, L.orbx_last_error()
        S.ex.sync()
        replay = c.download()
        for a, b in zip(eager, replay):
            assert np.array_equal(a, b)
    finally:
        assert L.orbm_set_stream(S.m.h, None) == 0


def test_refusals_enqueue_nothing(pkg, scenes):
    """Each refusal returns its documented code; the outputs keep their sentinel."""
    S = scenes
    L = S.L
    rows = np.array([0, 1], np.int32)
    tcw = np.stack([scene_pose(0), scene_pose(1)]); ow = camera_centre_np(tcw)
    valid = np.ones((2, 64), np.uint8)
    c = Call(S, rows, tcw, ow, np.array([64, 64], np.int32), valid, S.pw[:64], S.normal[:64], S.min_dist[:64], S.max_dist[:64],
             S.qdesc[:64], True)
    for buf, n in ((c.best, 128), (c.nf, 2), (c.lvl, 128)):
        buf.upload(np.full(n, 12345, np.int32))
    E_INV, E_CAP = -2, -3
    for over in (dict(kps=None), dict(desc=None), dict(gs=None), dict(gi=None), dict(tcw=None), dict(ow=None), dict(nq=None),
                 dict(valid=None), dict(pw=None), dict(normal=None), dict(mn=None), dict(mx=None), dict(qdesc=None), dict(k=None),
                 dict(bounds=None), dict(sf=None), dict(isg=None), dict(best=None), dict(nf=None),
                 dict(npairs=0), dict(nkf_rows=0), dict(cap=0), dict(qs=0), dict(nlev=0)):
        assert c.enqueue(3.0, 1, False, **over) == E_INV, over
    assert c.enqueue(float("nan"), 1, False) == E_INV and c.enqueue(float("inf"), 0, False) == E_INV
    for over in (dict(cap=65536), dict(qs=(1 << 20) + 1), dict(nlev=13), dict(npairs=65536)):
        assert c.enqueue(3.0, 1, False, **over) == E_CAP, over
    assert L.orbm_sync(S.m.h) == 0
    b, n, lv = c.download()
    assert np.all(b == 12345) and np.all(n == 12345) and np.all(lv == 12345)
