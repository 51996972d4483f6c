"""Batched SearchByProjection(Frame, local MapPoints) -- M3, Tracking::SearchLocalPoints -- on the device
(orbm_search_by_projection_points_batch_async): for every frame of a batch the final match row and count equal, entry for
entry, the single-frame host entry point (ORBmatcher.SearchByProjectionPoints) AND the oracle's SearchByProjectionPoints on
the same inputs.  bFarPoints is applied to in_view on the host side before those two calls."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_extract import _device_batch

pytestmark = pytest.mark.gpu

# ORB_SCENE_SEEDS=100,101,... repeats the parity matrix on more synthetic scenes (as in test_gpu_search.py)
_SEEDS = [int(x) for x in os.environ.get("ORB_SCENE_SEEDS", "100").split(",")]

W, H = 752, 480
INV_W, INV_H = float(np.float32(64) / np.float32(W)), float(np.float32(48) / np.float32(H))
EUROC_K = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
MBF = 47.90639384423901
MB = MBF / 435.2046959714599
NLEV = 8


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class _Rows:
    """The per-query device arrays of one call: [nframes][q_stride] (qdesc / mp_obs: one shared row when q_shared)."""

    def __init__(self, pkg, nframes, qs, shared=False):
        self.nframes, self.qs, self.shared = nframes, qs, shared
        n, nd = nframes * qs, (qs if shared else nframes * qs)
        self.nq = pkg.DeviceBuffer(4 * nframes)
        self.in_view = pkg.DeviceBuffer(n); self.px = pkg.DeviceBuffer(4 * n); self.py = pkg.DeviceBuffer(4 * n)
        self.pxr = pkg.DeviceBuffer(4 * n); self.view_cos = pkg.DeviceBuffer(4 * n); self.level = pkg.DeviceBuffer(4 * n)
        self.depth = pkg.DeviceBuffer(4 * n)
        self.qdesc = pkg.DeviceBuffer(32 * nd); self.mp_obs = pkg.DeviceBuffer(nd)

    def upload(self, Q):
        """Q: per frame a dict of host arrays (length nq <= q_stride); padding rows are zero."""
        qs = self.qs
        nq = np.array([len(q["px"]) for q in Q], np.int32)
        self.nq.upload(nq)
        for name, dt, buf in (("in_view", np.uint8, self.in_view), ("px", np.float32, self.px), ("py", np.float32, self.py),
                              ("pxr", np.float32, self.pxr), ("view_cos", np.float32, self.view_cos), ("level", np.int32, self.level),
                              ("depth", np.float32, self.depth)):
            a = np.zeros((self.nframes, qs), dt)
            for f, q in enumerate(Q):
                if name in q:
                    a[f, :len(q[name])] = q[name]
            buf.upload(a)
        if self.shared:
            self.qdesc.upload(np.ascontiguousarray(Q[0]["qdesc"], np.uint8)); self.mp_obs.upload(np.ascontiguousarray(Q[0]["mp_obs"], np.uint8))
        else:
            d = np.zeros((self.nframes, qs, 32), np.uint8); o = np.zeros((self.nframes, qs), np.uint8)
            for f, q in enumerate(Q):
                d[f, :len(q["qdesc"])] = q["qdesc"]; o[f, :len(q["mp_obs"])] = q["mp_obs"]
            self.qdesc.upload(d); self.mp_obs.upload(o)


def _call(L, m, r, cap, gs, gi, t_first, rows, sf, th, nnratio, match, nm, uright=None, blocked=None, depth=False, th_far=0.0,
          inv_w=INV_W, inv_h=INV_H, nlev=NLEV):
    return L.orbm_search_by_projection_points_batch_async(
        m.h, r["kps"], r["desc"], r["counts"], cap, gs.ptr, gi.ptr, 0.0, 0.0, inv_w, inv_h, t_first, rows.nframes,
        None if uright is None else uright.ptr, None if blocked is None else blocked.ptr, rows.nq.ptr, rows.qs,
        rows.in_view.ptr, rows.px.ptr, rows.py.ptr, rows.pxr.ptr, rows.view_cos.ptr, rows.level.ptr,
        rows.depth.ptr if depth else None, float(th_far), rows.qdesc.ptr, rows.mp_obs.ptr, int(rows.shared),
        float(th), float(nnratio), _vp(sf), nlev, match.ptr, nm.ptr)


def _check_frame(pkg, m, OM, sf, kt, dt, q, row, n_dev, th, nnratio, ur=None, blocked=None, th_far=None, w=W, h=H):
    """Device row + count of one frame vs the host entry point and the oracle; returns (nmatches, matched slots)."""
    nt = len(kt)
    iv = np.asarray(q["in_view"], np.uint8).copy()
    if th_far is not None:
        iv[(iv != 0) & (q["depth"] > np.float32(th_far))] = 0
    nqf = len(iv)
    lev = np.where(iv != 0, q["level"], 0).astype(np.int32)          # rejected rows are never read; keep garbage out of the host index
    args = dict(blocked=np.zeros(nt, np.uint8) if blocked is None else blocked[:nt], scale_factors=sf, in_view=iv, px=q["px"], py=q["py"],
                pxr=q["pxr"] if "pxr" in q else np.zeros(nqf, np.float32), view_cos=q["view_cos"], level=lev, qdesc=q["qdesc"],
                mp_obs=q["mp_obs"], th=th, nnratio=nnratio)
    if nt == 0:
        assert n_dev == 0 and np.all(row == -1)
        return 0, 0
    u = None if ur is None else np.ascontiguousarray(ur[:nt], np.float32)
    n_h, m_h = m.SearchByProjectionPoints(pkg.FrameView(kt, dt, w, h, uright=u, backend=m), **args)
    n_o, m_o = OM.SearchByProjectionPoints(pkg.FrameView(kt, dt, w, h, uright=u, backend=OM), **args)
    assert n_h == n_o and np.array_equal(m_h, m_o)
    assert n_dev == n_o, (n_dev, n_o)
    assert np.array_equal(row[:nt], m_o), np.flatnonzero(row[:nt] != m_o)[:10]
    assert np.all(row[nt:] == -1)
    return n_o, int((m_o >= 0).sum())


def _queries(rng, kps, desc, nq, jitter=1.5, flips=6, own=False, nlev=NLEV):
    n = len(kps)
    src = np.arange(nq) % n if own else rng.integers(0, n, nq)
    px = kps["x"][src].astype(np.float32); py = kps["y"][src].astype(np.float32)
    d = desc[src].copy()
    if not own:
        px = (px + rng.normal(0, jitter, nq)).astype(np.float32); py = (py + rng.normal(0, jitter, nq)).astype(np.float32)
        nflip = rng.integers(0, flips + 1, nq)                         # a few flipped bits: close but rarely identical
        for j in range(flips):
            sel = np.flatnonzero(nflip > j); b = rng.integers(0, 256, len(sel))
            d[sel, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    vc = rng.uniform(0.994, 1.0, nq).astype(np.float32)
    vc[rng.random(nq) < 0.1] = np.float32(0.998)                        # float(0.998) > 0.998 (double): the 2.5 radius
    lev = kps["octave"][src].astype(np.int32)
    up = rng.random(nq) < 0.2
    lev[up] = np.minimum(lev[up] + 1, nlev - 1)                          # predicted one level up: the window's level-1 side
    return dict(in_view=(rng.random(nq) < 0.85).astype(np.uint8), px=px, py=py, pxr=(px - rng.uniform(2, 40, nq)).astype(np.float32),
                view_cos=vc, level=lev, qdesc=d, mp_obs=np.ones(nq, np.uint8), depth=rng.uniform(0.5, 12, nq).astype(np.float32))


@pytest.fixture(scope="module", params=_SEEDS)
def batch(request, pkg, oracle, synth):
    NB = 10
    s = request.param
    imgs = [synth.gen_image(W, H, 40 * s + i) for i in range(NB)]
    imgs[3] = np.full((H, W), 128, np.uint8)                                   # no corner anywhere: an empty frame
    ex = pkg.ORBextractor(1000, max_size=(W, H), max_batch=NB)
    res = ex.extract_batch(imgs, [(0, 1000)] * NB)
    assert len(res[3][1]) == 0
    m = pkg.ORBmatcher(0.9)
    OM = oracle._oracle_matcher_class()()
    L = pkg.lib()
    r = ex.result_device(); cap = r["cap"]
    gs = pkg.DeviceBuffer(NB * 3073 * 4); gi = pkg.DeviceBuffer(NB * cap * 4)
    assert L.orbm_grid_build_batch_async(m.h, r["kps"], r["counts"], NB, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0
    m.sync()
    return dict(NB=NB, seed=s, ex=ex, res=res, m=m, OM=OM, L=L, r=r, cap=cap, gs=gs, gi=gi, sf=ex.GetScaleFactors())


_MATRIX = [(th, nn, st) for th in (1.0, 3.0, 10.0) for nn in (0.8, 0.9) for st in (False, True)]


@pytest.mark.parametrize("th,nnratio,stereo", _MATRIX)
def test_parity_matrix(pkg, batch, th, nnratio, stereo):
    """Frames 1..9 of the block (frame 0 is skipped: t_first = 1).  Frame 3 is empty; frame 5's queries are all out of view; frame 8's
    queries are its own keypoints and descriptors (distance-0 ties across levels); slots blocked at 35 % (frame 2) and 97 % (frame 6:
    queries run into the device rescan); mp_obs half set (frame 4) and none set (frame 7: slots taken again, counts with overwrites).
    Half of the matrix shares one query row between the frames (q_shared)."""
    B = batch
    pkg_L, m, OM, res, cap, sf = B["L"], B["m"], B["OM"], B["res"], B["cap"], B["sf"]
    ix = _MATRIX.index((th, nnratio, stereo))
    shared = (ix + ix // 2) % 2 == 1
    rng = np.random.default_rng(B["seed"] * 1000 + int(th * 10) + int(nnratio * 10) + 2 * stereo)
    T0, NF = 1, B["NB"] - 1
    frames = list(range(T0, T0 + NF))
    Q = []
    kf = [(res[f][1], res[f][2]) if len(res[f][1]) else (res[f - 1][1], res[f - 1][2]) for f in frames]   # the empty frame: its neighbour's
    if not shared:
        for i, f in enumerate(frames):
            nq = int(rng.integers(1000, 3000))
            q = _queries(rng, *kf[i], nq, own=(f == 8))
            if f == 4:
                q["mp_obs"] = (rng.random(nq) < 0.5).astype(np.uint8)
            if f == 7:
                q["mp_obs"][:] = 0
            Q.append(q)
    else:
        # ONE row of MapPoints for all frames: block i (K rows) comes from frame i's keypoints and sits where frame i projects it; the
        # other blocks project to random keypoints of the frame (30 % in view, descriptors of another image: candidates, rarely matches)
        K = 250
        own = [_queries(rng, *kf[i], K) for i in range(NF)]
        own[4 - T0]["mp_obs"] = (rng.random(K) < 0.5).astype(np.uint8)
        own[7 - T0]["mp_obs"][:] = 0
        qd = np.concatenate([o["qdesc"] for o in own]); ob = np.concatenate([o["mp_obs"] for o in own])
        for i, f in enumerate(frames):
            g = _queries(rng, *kf[i], NF * K)
            g["in_view"] &= (rng.random(NF * K) < 0.3).astype(np.uint8)
            for key in ("in_view", "px", "py", "pxr", "view_cos", "level", "depth"):
                g[key][i * K:(i + 1) * K] = own[i][key]
            g["qdesc"], g["mp_obs"] = qd, ob
            Q.append(g)
    if 5 in frames:
        Q[5 - T0]["in_view"][:] = 0
    qs = max(len(q["px"]) for q in Q) + 5
    rows = _Rows(pkg, NF, qs, shared)
    rows.upload(Q)
    blocked = np.zeros((NF, cap), np.uint8)
    blocked[2 - T0] = rng.random(cap) < 0.35
    blocked[6 - T0] = rng.random(cap) < 0.97
    dblk = pkg.DeviceBuffer(NF * cap).upload(blocked)
    ur_h = None
    dur = None
    if stereo:
        ur_h = np.full((NF, cap), -1, np.float32)
        for i, f in enumerate(frames):
            k = res[f][1]
            ur_h[i, :len(k)] = np.where(rng.random(len(k)) < 0.6, k["x"] - rng.uniform(2, 40, len(k)), -1)
        dur = pkg.DeviceBuffer(NF * cap * 4).upload(ur_h)
    dm = pkg.DeviceBuffer(NF * cap * 4); dn = pkg.DeviceBuffer(NF * 4)
    rc = _call(pkg_L, m, B["r"], cap, B["gs"], B["gi"], T0, rows, sf, th, nnratio, dm, dn, uright=dur, blocked=dblk)
    assert rc == 0, pkg_L.orbm_last_error()
    m.sync()
    match = dm.download(np.int32, NF * cap).reshape(NF, cap); nm = dn.download(np.int32, NF)
    total, overwrites = 0, 0
    for i, f in enumerate(frames):
        kt, dt = res[f][1], res[f][2]
        n_ref, nslots = _check_frame(pkg, m, OM, sf, kt, dt, Q[i], match[i], nm[i], th, nnratio,
                                     ur=None if ur_h is None else ur_h[i], blocked=blocked[i])
        total += n_ref
        overwrites += n_ref - nslots
        if f == 5:
            assert nm[i] == 0
    assert total > 300
    if not shared:
        assert overwrites > 0                                                  # frame 7 (no observations) takes slots again


def _pose(rng):
    a = rng.uniform(-0.01, 0.01, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).astype(np.float32)
    t = rng.uniform(-0.03, 0.03, 3).astype(np.float32)
    return R, t, (-R.T @ t).astype(np.float32)


def test_frustum_chain(pkg, batch):
    """Per frame a local map made by back-projecting the frame's keypoints (two depths each) through the identity pose; isInFrustum
    (cos limit 0.5, Tracking.cc:3851) under a perturbed pose writes row f of the batch arrays ON THE DEVICE, then the batched search
    runs with bFarPoints on -- no host copy in between.  The rows equal the host M3 and the oracle fed with the frustum outputs
    downloaded from the device."""
    B = batch
    L, m, OM, res, cap, sf = B["L"], B["m"], B["OM"], B["res"], B["cap"], B["sf"]
    rng = np.random.default_rng(B["seed"] + 7)
    T0, NF = 0, 8
    fx, fy, cx, cy = EUROC_K
    maps = []
    for f in range(T0, T0 + NF):
        k, d = res[f][1], res[f][2]
        n = len(k)
        z = np.concatenate([rng.uniform(1.0, 4.0, n), rng.uniform(4.0, 14.0, n)]).astype(np.float32)
        u = np.concatenate([k["x"], k["x"]]); v = np.concatenate([k["y"], k["y"]]); octv = np.concatenate([k["octave"], k["octave"]])
        Pw = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1).astype(np.float32)
        dist = np.linalg.norm(Pw, axis=1).astype(np.float32)
        nrm = (Pw / dist[:, None]).astype(np.float32)
        mx = (dist * sf[octv]).astype(np.float32); mn = (mx / sf[NLEV - 1]).astype(np.float32)
        qd = np.concatenate([d, d]).copy()
        flip = rng.integers(0, 256, (len(qd), 3))
        for j in range(3):
            qd[np.arange(len(qd)), flip[:, j] >> 3] ^= (1 << (flip[:, j] & 7)).astype(np.uint8)
        maps.append(dict(Pw=Pw, nrm=nrm, mn=mn, mx=mx, qdesc=qd, mp_obs=(rng.random(len(qd)) < 0.9).astype(np.uint8)))
    qs = max(len(mp["Pw"]) for mp in maps) + 3
    rows = _Rows(pkg, NF, qs)
    rows.upload([dict(px=np.zeros(len(mp["Pw"]), np.float32), qdesc=mp["qdesc"], mp_obs=mp["mp_obs"]) for mp in maps])
    bounds = np.array([0.0, W, 0.0, H], np.float32)
    lsf = float(np.log(np.float32(1.2)))
    keep = []
    for i, mp in enumerate(maps):
        n = len(mp["Pw"])
        R, t, Ow = _pose(rng)
        dP, dN, dMn, dMx = (pkg.DeviceBuffer(a.nbytes).upload(a) for a in (mp["Pw"], mp["nrm"], mp["mn"], mp["mx"]))
        keep += [dP, dN, dMn, dMx]
        o = i * qs
        rc = L.orbm_is_in_frustum(m.h, pkg.DEVICE, n, dP.ptr, dN.ptr, dMn.ptr, dMx.ptr, _vp(R.reshape(9)), _vp(t), _vp(Ow), _vp(EUROC_K), _vp(bounds),
                                  MBF, 0.5, lsf, NLEV, rows.in_view.ptr + o, rows.px.ptr + 4 * o, rows.py.ptr + 4 * o, rows.pxr.ptr + 4 * o,
                                  rows.depth.ptr + 4 * o, rows.level.ptr + 4 * o, rows.view_cos.ptr + 4 * o)
        assert rc == 0, L.orbm_last_error()
    th, th_far = 3.0, 9.0
    dm = pkg.DeviceBuffer(NF * cap * 4); dn = pkg.DeviceBuffer(NF * 4)
    assert _call(L, m, B["r"], cap, B["gs"], B["gi"], T0, rows, sf, th, 0.8, dm, dn, depth=True, th_far=th_far) == 0, L.orbm_last_error()
    m.sync()
    match = dm.download(np.int32, NF * cap).reshape(NF, cap); nm = dn.download(np.int32, NF)
    get = lambda buf, dt: buf.download(dt, NF * qs).reshape(NF, qs)
    iv, px, py, pxr, dep, lev, vc = (get(rows.in_view, np.uint8), get(rows.px, np.float32), get(rows.py, np.float32), get(rows.pxr, np.float32),
                                     get(rows.depth, np.float32), get(rows.level, np.int32), get(rows.view_cos, np.float32))
    total, far = 0, 0
    for i, mp in enumerate(maps):
        n = len(mp["Pw"])
        q = dict(in_view=iv[i, :n], px=px[i, :n], py=py[i, :n], pxr=pxr[i, :n], depth=dep[i, :n], level=lev[i, :n], view_cos=vc[i, :n],
                 qdesc=mp["qdesc"], mp_obs=mp["mp_obs"])
        assert n == 0 or iv[i, :n].sum() > 0.5 * n                          # frame 3 is empty
        far += int(((iv[i, :n] != 0) & (dep[i, :n] > th_far)).sum())
        total += _check_frame(pkg, m, OM, sf, res[T0 + i][1], res[T0 + i][2], q, match[i], nm[i], th, 0.8, th_far=th_far)[0]
    assert total > 1000 and far > 100


def test_stereo_chain(pkg, oracle, synth):
    """mvuRight from orbm_stereo_batch_async (first_l == t_first) feeds the stereo gate of the batched search directly."""
    P = 3
    pairs = [synth.gen_stereo_pair(W, H, 610 + i) for i in range(P)]
    imgs = [p[0] for p in pairs] + [p[1] for p in pairs]
    stride = (W + 63) // 64 * 64
    dev = pkg.DeviceBuffer(2 * P * stride * H)
    for i, im in enumerate(imgs):
        pad = np.zeros((H, stride), np.uint8); pad[:, :W] = im
        dev.upload(pad, offset=i * stride * H)
    arr = (C.c_void_p * (2 * P))(*[dev.ptr + i * stride * H for i in range(2 * P)])
    L = pkg.lib()
    ex = pkg.ORBextractor(1200, max_size=(W, H), max_batch=2 * P)
    mt = pkg.ORBmatcher(0.6)
    OM = oracle._oracle_matcher_class()()
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    cap = ex.cap
    ex.enqueue_device(arr, W, H, stride, np.zeros(4 * P, np.int32))
    r = ex.result_device()
    ur = pkg.DeviceBuffer(P * cap * 4); dp = pkg.DeviceBuffer(P * cap * 4); sad = pkg.DeviceBuffer(P * cap * 4); kept = pkg.DeviceBuffer(P * 4)
    assert L.orbm_stereo_batch_async(mt.h, ex.h, 0, P, P, r["kps"], r["desc"], r["counts"], cap, MB, MBF, ur.ptr, dp.ptr, sad.ptr, kept.ptr) == 0, L.orbm_last_error()
    gs = pkg.DeviceBuffer(2 * P * 3073 * 4); gi = pkg.DeviceBuffer(2 * P * cap * 4)
    assert L.orbm_grid_build_batch_async(mt.h, r["kps"], r["counts"], 2 * P, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0
    ex.sync()
    res = ex.fetch_all()
    ur_h = ur.download(np.float32, P * cap).reshape(P, cap)
    rng = np.random.default_rng(5)
    Q = []
    for p in range(P):
        k, d = res[p][1], res[p][2]
        q = _queries(rng, k, d, 2000)
        q["pxr"] = np.where(rng.random(2000) < 0.7, q["px"] - rng.uniform(2, 40, 2000), q["pxr"]).astype(np.float32)
        Q.append(q)
    rows = _Rows(pkg, P, 2000)
    rows.upload(Q)
    sf = ex.GetScaleFactors()
    dm = pkg.DeviceBuffer(P * cap * 4); dn = pkg.DeviceBuffer(P * 4)
    assert _call(L, mt, r, cap, gs, gi, 0, rows, sf, 3.0, 0.8, dm, dn, uright=ur) == 0, L.orbm_last_error()
    mt.sync()
    match = dm.download(np.int32, P * cap).reshape(P, cap); nm = dn.download(np.int32, P)
    total = 0
    for p in range(P):
        assert (ur_h[p, :len(res[p][1])] > 0).sum() > 300
        total += _check_frame(pkg, mt, OM, sf, res[p][1], res[p][2], Q[p], match[p], nm[p], 3.0, 0.8, ur=ur_h[p])[0]
    assert total > 300
    ex.close(); mt.close()


def test_capture_replay(pkg, synth):
    """The matcher on the extractor's stream; extract + grid + this call captured into a slot after one eager run: the replay's
    rows equal the eager rows."""
    n = 4
    imgs, dev, arr, stride = _device_batch(pkg, synth, W, H, n, 880)
    L = pkg.lib()
    ex = pkg.ORBextractor(1000, max_size=(W, H), max_batch=n)
    mt = pkg.ORBmatcher(0.7)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    cap = ex.cap
    ex.enqueue_device(arr, W, H, stride)
    ex.sync()
    res = ex.fetch_all()
    rng = np.random.default_rng(9)
    Q = [_queries(rng, res[i][1], res[i][2], 1500) for i in range(n)]
    rows = _Rows(pkg, n, 1500)
    rows.upload(Q)
    r = ex.result_device()
    gs = pkg.DeviceBuffer(n * 3073 * 4); gi = pkg.DeviceBuffer(n * cap * 4)
    dm = pkg.DeviceBuffer(n * cap * 4); dn = pkg.DeviceBuffer(n * 4)
    sf = ex.GetScaleFactors()

    def enqueue():
        ex.enqueue_device(arr, W, H, stride)
        assert L.orbm_grid_build_batch_async(mt.h, r["kps"], r["counts"], n, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0
        assert _call(L, mt, r, cap, gs, gi, 0, rows, sf, 10.0, 0.9, dm, dn) == 0, L.orbm_last_error()

    enqueue()
    ex.sync()
    eager_m = dm.download(np.int32, n * cap); eager_n = dn.download(np.int32, n)
    assert eager_n.sum() > 200
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    dm.upload(np.full(n * cap, -7, np.int32)); dn.upload(np.full(n, -7, np.int32))
    assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
    ex.sync()
    assert np.array_equal(dm.download(np.int32, n * cap), eager_m) and np.array_equal(dn.download(np.int32, n), eager_n)
    ex.close(); mt.close()


def test_refusals_enqueue_nothing(pkg):
    """Oversized cap / q_stride, more than 12 levels and NULL arrays are refused with the documented codes; nothing runs."""
    m = pkg.ORBmatcher()
    L = m.L
    one = pkg.DeviceBuffer(4096)
    dm = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))
    sf = np.ones(16, np.float32)
    p = one.ptr

    def call(cap=4, qs=4, nlev=8, in_view=p, nframes=1):
        return L.orbm_search_by_projection_points_batch_async(m.h, p, p, p, cap, p, p, 0.0, 0.0, INV_W, INV_H, 0, nframes, None, None, p, qs,
                                                              in_view, p, p, p, p, p, None, 0.0, p, p, 0, 1.0, 0.8, _vp(sf), nlev, dm.ptr, dm.ptr)
    assert call(cap=70000) == -3 and b"65535" in L.orbm_last_error()
    assert call(qs=(1 << 20) + 1) == -3
    assert call(nlev=13) == -3
    assert call(in_view=None) == -2
    assert call(nframes=0) == -2 and call(cap=0) == -2 and call(qs=0) == -2
    m.sync()
    assert np.all(dm.download(np.int32, 16) == 12345)
