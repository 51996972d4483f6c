"""Batched SearchByProjection(CurrentFrame, LastFrame) -- M4, Tracking::TrackWithMotionModel -- on the device
(orbm_search_by_projection_frame_batch_async, fed by orbm_project_last_frame_batch_async): for every pair the final match row and
count equal, entry for entry, the single-frame host entry point (ORBmatcher.SearchByProjectionFrame) AND the oracle's
SearchByProjectionFrame on the same inputs, ORBM_MATCH_PRUNED and the ORBM_NO_MATCH padding included."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_extract import _device_batch
from test_motion_projection_cpu import project_last_frame_np, random_pose

pytestmark = pytest.mark.gpu

W, H = 752, 480
INV_W, INV_H = float(np.float32(64) / np.float32(W)), float(np.float32(48) / np.float32(H))
EUROC_K = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
MBF = 47.90639384423901
MB = MBF / 435.2046959714599
NLEV = 8


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class _Rows:
    """The per-query device arrays of one call, [npairs][q_stride], and the per-pair dir."""
    FIELDS = (("valid", np.uint8), ("u", np.float32), ("v", np.float32), ("invzc", np.float32), ("octave", np.int32), ("angle", np.float32),
              ("mp_obs", np.uint8))

    def __init__(self, pkg, npairs, qs):
        self.npairs, self.qs = npairs, qs
        n = npairs * qs
        self.nq = pkg.DeviceBuffer(4 * npairs)
        for name, dt in self.FIELDS:
            setattr(self, name, pkg.DeviceBuffer(np.dtype(dt).itemsize * n))
        self.qdesc = pkg.DeviceBuffer(32 * n)
        self.dir = pkg.DeviceBuffer(max(npairs, 4))

    def upload(self, Q, dirs=None):
        """Q: per pair a dict of host arrays (length nq <= q_stride); padding rows hold garbage (never read)."""
        self.nq.upload(np.array([len(q["u"]) for q in Q], np.int32))
        for name, dt in self.FIELDS:
            a = np.full((self.npairs, self.qs), 77, dt)
            for p, q in enumerate(Q):
                a[p, :len(q[name])] = q[name]
            getattr(self, name).upload(a)
        d = np.full((self.npairs, self.qs, 32), 0xA5, np.uint8)
        for p, q in enumerate(Q):
            d[p, :len(q["qdesc"])] = q["qdesc"]
        self.qdesc.upload(d)
        self.dir.upload(np.zeros(max(self.npairs, 4), np.uint8) if dirs is None else np.asarray(dirs, np.uint8))


def _call(L, m, r, cap, gs, gi, t_first, rows, sf, th, match, nm, uright=None, mbf=MBF, blocked=None, use_dir=True, retry_below=0,
          retried=None, check_ori=True, inv_w=INV_W, inv_h=INV_H, nlev=NLEV, npairs=None):
    return L.orbm_search_by_projection_frame_batch_async(
        m.h, r["kps"], r["desc"], r["counts"], cap, gs.ptr, gi.ptr, 0.0, 0.0, inv_w, inv_h, t_first, rows.npairs if npairs is None else npairs,
        None if uright is None else uright.ptr, float(mbf), None if blocked is None else blocked.ptr, rows.dir.ptr if use_dir else None,
        rows.nq.ptr, rows.qs, rows.valid.ptr, rows.u.ptr, rows.v.ptr, rows.invzc.ptr, rows.octave.ptr, rows.angle.ptr, rows.qdesc.ptr,
        rows.mp_obs.ptr, float(th), int(retry_below), _vp(sf), nlev, int(check_ori), match.ptr, nm.ptr, None if retried is None else retried.ptr)


def _check_pair(pkg, m, OM, sf, kt, dt, q, row, n_dev, th, d=0, check_ori=True, ur=None, blocked=None, mbf=MBF, w=W, h=H, nlev=NLEV):
    """Device row + count of one pair vs the host entry point and the oracle; returns (nmatches, pruned slots).  A valid row whose octave
    lies outside [0, nlev) is skipped by the batched call; the host entry point and the oracle see it as not valid."""
    nt = len(kt)
    if nt == 0 or len(q["u"]) == 0:
        assert n_dev == 0 and np.all(row == -1)
        return 0, 0
    octv = np.asarray(q["octave"], np.int32)
    valid = ((np.asarray(q["valid"]) != 0) & (octv >= 0) & (octv < nlev)).astype(np.uint8)
    octv = np.where(valid != 0, octv, 0).astype(np.int32)                  # skipped rows are never read; keep garbage out of the host index
    args = dict(cur_blocked=np.zeros(nt, np.uint8) if blocked is None else blocked[:nt], scale_factors=sf, valid=valid, u=q["u"], v=q["v"],
                invzc=q["invzc"], octave=octv, angle=q["angle"], qdesc=q["qdesc"], mp_obs=q["mp_obs"], th=th,
                forward=d == 1, backward=d == 2, mbf=mbf if ur is not None else 0.0, check_ori=check_ori)
    u = None if ur is None else np.ascontiguousarray(ur[:nt], np.float32)
    n_h, m_h = m.SearchByProjectionFrame(pkg.FrameView(kt, dt, w, h, uright=u, backend=m), **args)
    n_o, m_o = OM.SearchByProjectionFrame(pkg.FrameView(kt, dt, w, h, uright=u, backend=OM), **args)
    assert n_h == n_o and np.array_equal(m_h, m_o)
    assert n_dev == n_o, (n_dev, n_o)
    assert np.array_equal(row[:nt], m_o), np.flatnonzero(row[:nt] != m_o)[:10]
    assert np.all(row[nt:] == -1)
    return n_o, int((m_o == -2).sum())


def _queries(rng, kps, desc, nq, jitter=1.5, flips=6, own=False, nlev=NLEV, shift=0.0):
    """LastFrame MapPoints seen near keypoints of the searched frame: a few flipped descriptor bits, the octave sometimes one off,
    angles mostly consistent (one rotation bin) with some strays for the histogram cull."""
    n = len(kps)
    src = np.arange(nq) % n if own else rng.integers(0, n, nq)
    u = kps["x"][src].astype(np.float32); v = kps["y"][src].astype(np.float32)
    d = desc[src].copy()
    ang = kps["angle"][src].astype(np.float32)
    octv = kps["octave"][src].astype(np.int32)
    if not own:
        u = (u + rng.normal(0, jitter, nq) + shift).astype(np.float32); v = (v + rng.normal(0, jitter, nq)).astype(np.float32)
        nflip = rng.integers(0, flips + 1, nq)
        for j in range(flips):
            sel = np.flatnonzero(nflip > j); b = rng.integers(0, 256, len(sel))
            d[sel, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
        ang = np.mod(ang + 14.0 + rng.normal(0, 2, nq), 360).astype(np.float32)
        stray = rng.random(nq) < 0.15
        ang[stray] = rng.uniform(0, 360, stray.sum()).astype(np.float32)
        up = rng.random(nq) < 0.2
        octv[up] = np.minimum(octv[up] + 1, nlev - 1)
        dn = rng.random(nq) < 0.1
        octv[dn] = np.maximum(octv[dn] - 1, 0)
    return dict(valid=(rng.random(nq) < 0.85).astype(np.uint8), u=u, v=v, invzc=rng.uniform(0.02, 0.9, nq).astype(np.float32),
                octave=octv, angle=ang, qdesc=d, mp_obs=np.ones(nq, np.uint8))


def _uright(rng, kps, cap):
    ur = np.full(cap, -1, np.float32)
    ur[:len(kps)] = np.where(rng.random(len(kps)) < 0.6, kps["x"] - rng.uniform(1, 43, len(kps)), -1)
    return ur


@pytest.fixture(scope="module")
def batch(pkg, oracle, synth):
    NB = 10
    imgs = [synth.gen_image(W, H, 4000 + i) for i in range(NB)]
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
    return dict(NB=NB, ex=ex, res=res, m=m, OM=OM, L=L, r=r, cap=cap, gs=gs, gi=gi, sf=ex.GetScaleFactors())


_MATRIX = [(th, dm, st) for th in (7.0, 15.0, 30.0) for dm in ("0", "1", "2", "mix") for st in (False, True)]


@pytest.mark.parametrize("th,dmode,stereo", _MATRIX)
def test_parity_matrix(pkg, batch, th, dmode, stereo):
    """Pairs 1..9 of the block (t_first = 1).  Frame 3 is empty (searched); pair 4's query source is empty (nq = 0); slots blocked
    at 35 % (frame 2) and 97 % (frame 6: lists run dry, device rescan); mp_obs half set (frame 5) and none set (frame 7: slots taken
    again, overwrites counted and culled twice); frame 8's queries are its own keypoints and descriptors (distance-0 ties); frames 1
    and 9 hold valid rows whose octave lies outside the scale table (skipped).  Within each (th, dir) row one of the two stereo
    settings runs without the rotation check, alternating from row to row."""
    B = batch
    L, m, OM, res, cap, sf = B["L"], B["m"], B["OM"], B["res"], B["cap"], B["sf"]
    ix = _MATRIX.index((th, dmode, stereo))
    check_ori = (ix // 2 + ix) % 2 == 0                                       # stereo off / on take opposite settings; rows alternate
    rng = np.random.default_rng(1000 + ix)
    T0, NP = 1, B["NB"] - 1
    frames = list(range(T0, T0 + NP))
    Q = []
    for f in frames:
        kt, dt = res[f][1], res[f][2]
        if f == 4:
            q = _queries(rng, kt, dt, 0)
        elif f == 3:
            q = _queries(rng, res[2][1], res[2][2], 800)                     # the empty frame is searched with its neighbour's points
        else:
            q = _queries(rng, kt, dt, int(rng.integers(700, 1300)), own=(f == 8))
        if f == 5:
            q["mp_obs"] = (rng.random(len(q["u"])) < 0.5).astype(np.uint8)
        if f == 7:
            q["mp_obs"][:] = 0
        if f in (1, 9):                                                       # octave outside [0, nlevels): the row is skipped
            bad = rng.choice(len(q["u"]), 40, replace=False)
            q["valid"][bad] = 1
            q["octave"][bad] = rng.choice(np.array([-1, NLEV, NLEV + 3, -100], np.int32), 40)
        Q.append(q)
    dirs = np.full(NP, int(dmode) if dmode != "mix" else 0, np.uint8)
    if dmode == "mix":
        dirs = np.array([0, 1, 2, 7, 1, 2, 0, 1, 2][:NP], np.uint8)           # 7 reads as 0
    qs = max(len(q["u"]) for q in Q) + 5
    rows = _Rows(pkg, NP, qs)
    rows.upload(Q, dirs)
    blocked = np.zeros((NP, cap), np.uint8)
    blocked[2 - T0] = rng.random(cap) < 0.35
    blocked[6 - T0] = rng.random(cap) < 0.97
    dblk = pkg.DeviceBuffer(NP * cap).upload(blocked)
    ur_h, dur = None, None
    if stereo:
        ur_h = np.stack([_uright(rng, res[f][1], cap) for f in frames])
        dur = pkg.DeviceBuffer(NP * cap * 4).upload(ur_h)
    dm = pkg.DeviceBuffer(NP * cap * 4); dn = pkg.DeviceBuffer(NP * 4)
    assert _call(L, m, B["r"], cap, B["gs"], B["gi"], T0, rows, sf, th, dm, dn, uright=dur, blocked=dblk, check_ori=check_ori) == 0, L.orbm_last_error()
    m.sync()
    match = dm.download(np.int32, NP * cap).reshape(NP, cap); nm = dn.download(np.int32, NP)
    total, pruned = 0, 0
    for i, f in enumerate(frames):
        dd = int(dirs[i]) if dirs[i] in (1, 2) else 0
        n_ref, npr = _check_pair(pkg, m, OM, sf, res[f][1], res[f][2], Q[i], match[i], nm[i], th, d=dd, check_ori=check_ori,
                                 ur=None if ur_h is None else ur_h[i], blocked=blocked[i])
        total += n_ref; pruned += npr
    assert total > 1500
    assert nm[3 - T0] == 0 and nm[4 - T0] == 0
    if check_ori:
        assert pruned > 0


def test_parity_12_levels(pkg, oracle, synth):
    """A 12-level, scale-1.1 extractor: the scale table's upper half and forward / backward windows on it."""
    NB = 4
    imgs = [synth.gen_image(W, H, 4100 + i) for i in range(NB)]
    ex = pkg.ORBextractor(1000, 1.1, 12, max_size=(W, H), max_batch=NB)
    res = ex.extract_batch(imgs, [(0, 1000)] * NB)
    m = pkg.ORBmatcher(0.9); OM = oracle._oracle_matcher_class()(); L = pkg.lib()
    r = ex.result_device(); cap = r["cap"]; sf = ex.GetScaleFactors()
    assert len(sf) == 12
    gs = pkg.DeviceBuffer(NB * 3073 * 4); gi = pkg.DeviceBuffer(NB * cap * 4)
    assert L.orbm_grid_build_batch_async(m.h, r["kps"], r["counts"], NB, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0
    rng = np.random.default_rng(12)
    Q = [_queries(rng, res[f][1], res[f][2], 1000, nlev=12) for f in range(NB)]
    assert max(q["octave"].max() for q in Q) >= 9
    dirs = np.array([0, 1, 2, 1], np.uint8)
    rows = _Rows(pkg, NB, 1000); rows.upload(Q, dirs)
    ur_h = np.stack([_uright(rng, res[f][1], cap) for f in range(NB)])
    dur = pkg.DeviceBuffer(ur_h.nbytes).upload(ur_h)
    dm = pkg.DeviceBuffer(NB * cap * 4); dn = pkg.DeviceBuffer(NB * 4)
    assert _call(L, m, r, cap, gs, gi, 0, rows, sf, 15.0, dm, dn, uright=dur, nlev=12) == 0, L.orbm_last_error()
    m.sync()
    match = dm.download(np.int32, NB * cap).reshape(NB, cap); nm = dn.download(np.int32, NB)
    total = sum(_check_pair(pkg, m, OM, sf, res[f][1], res[f][2], Q[f], match[f], nm[f], 15.0, d=int(dirs[f]), ur=ur_h[f],
                            nlev=12)[0] for f in range(NB))
    assert total > 500


def test_large_cap(pkg, oracle):
    """A result block of 20 000 keypoints per frame at 1920x1080 (the extractor's quadtree cannot hold that many per level, so the
    block is laid out by hand: random keypoints on 8 levels, random descriptors).  More than 16 384 slots per frame: the shift form
    refuses that shape; this call runs it."""
    w, h, NB, cap = 1920, 1080, 2, 20480
    inv_w, inv_h = float(np.float32(64) / np.float32(w)), float(np.float32(48) / np.float32(h))
    rng = np.random.default_rng(13)
    m = pkg.ORBmatcher(0.9); OM = oracle._oracle_matcher_class()(); L = m.L
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    kps = np.zeros((NB, cap), pkg.KP_DTYPE); desc = np.zeros((NB, cap, 32), np.uint8)
    counts = np.array([20000, 19000], np.int32)
    for f in range(NB):
        n = counts[f]
        kps[f, :n]["x"] = rng.uniform(0, w - 1, n); kps[f, :n]["y"] = rng.uniform(0, h - 1, n)
        kps[f, :n]["angle"] = rng.uniform(0, 360, n); kps[f, :n]["octave"] = rng.integers(0, 8, n)
        kps[f, :n]["size"] = 31 * sf[kps[f, :n]["octave"]]; kps[f, :n]["class_id"] = -1
        desc[f, :n] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    dk, dd, dc = pkg.DeviceBuffer(kps.nbytes).upload(kps), pkg.DeviceBuffer(desc.nbytes).upload(desc), pkg.DeviceBuffer(8).upload(counts)
    r = dict(kps=dk.ptr, desc=dd.ptr, counts=dc.ptr)
    gs = pkg.DeviceBuffer(NB * 3073 * 4); gi = pkg.DeviceBuffer(NB * cap * 4)
    assert L.orbm_grid_build_batch_async(m.h, r["kps"], r["counts"], NB, cap, 0.0, 0.0, inv_w, inv_h, gs.ptr, gi.ptr) == 0, L.orbm_last_error()
    dm = pkg.DeviceBuffer(NB * cap * 4); dn = pkg.DeviceBuffer(NB * 4)
    assert L.orbm_search_by_projection_batch_async(m.h, r["kps"], r["desc"], r["counts"], cap, gs.ptr, gi.ptr, 0.0, 0.0, inv_w, inv_h, 1, 0, 1, 15.0,
                                                   _vp(sf), 8, 0.0, 0.0, None, None, 1, dm.ptr, dn.ptr) < 0
    res = [(None, kps[f, :counts[f]], desc[f, :counts[f]]) for f in range(NB)]
    Q = [_queries(rng, res[f][1], res[f][2], 6000) for f in range(NB)]
    rows = _Rows(pkg, NB, 6000); rows.upload(Q, [0, 1])
    blocked = (rng.random((NB, cap)) < 0.35).astype(np.uint8)
    dblk = pkg.DeviceBuffer(blocked.nbytes).upload(blocked)
    assert _call(L, m, r, cap, gs, gi, 0, rows, sf, 15.0, dm, dn, blocked=dblk, inv_w=inv_w, inv_h=inv_h) == 0, L.orbm_last_error()
    m.sync()
    match = dm.download(np.int32, NB * cap).reshape(NB, cap); nm = dn.download(np.int32, NB)
    total = 0
    for f in range(NB):
        total += _check_pair(pkg, m, OM, sf, res[f][1], res[f][2], Q[f], match[f], nm[f], 15.0, d=f, blocked=blocked[f], w=w, h=h)[0]
    assert total > 3000
    m.close()


def test_stereo_chain(pkg, oracle, synth):
    """mvuRight from orbm_stereo_batch_async (first_l == t_first) feeds the stereo gate of the batched search directly, with no host copy
    in between; each pair equals the host entry point and the oracle fed with the downloaded uright rows."""
    P = 3
    pairs = [synth.gen_stereo_pair(W, H, 4400 + i) for i in range(P)]
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
    rng = np.random.default_rng(44)
    Q = []
    for p in range(P):
        k, d = res[p][1], res[p][2]
        Q.append(_queries(rng, k, d, 2000))                                    # mbf * invzc spread over 1-43 px: the gate passes and rejects
    rows = _Rows(pkg, P, 2000)
    rows.upload(Q, [0, 1, 2])
    sf = ex.GetScaleFactors()
    dm = pkg.DeviceBuffer(P * cap * 4); dn = pkg.DeviceBuffer(P * 4)
    assert _call(L, mt, r, cap, gs, gi, 0, rows, sf, 7.0, dm, dn, uright=ur) == 0, L.orbm_last_error()
    mt.sync()
    match = dm.download(np.int32, P * cap).reshape(P, cap); nm = dn.download(np.int32, P)
    ur_h = ur.download(np.float32, P * cap).reshape(P, cap)
    total, differ = 0, 0
    for p in range(P):
        nt = len(res[p][1])
        assert (ur_h[p, :nt] > 0).sum() > 300
        total += _check_pair(pkg, mt, OM, sf, res[p][1], res[p][2], Q[p], match[p], nm[p], 7.0, d=p, ur=ur_h[p])[0]
        # the gate decides: without it the same pair gives another row
        _, m_free = mt.SearchByProjectionFrame(pkg.FrameView(res[p][1], res[p][2], W, H, backend=mt), cur_blocked=np.zeros(nt, np.uint8),
                                               scale_factors=sf, valid=Q[p]["valid"], u=Q[p]["u"], v=Q[p]["v"], invzc=Q[p]["invzc"],
                                               octave=Q[p]["octave"], angle=Q[p]["angle"], qdesc=Q[p]["qdesc"], mp_obs=Q[p]["mp_obs"], th=7.0,
                                               forward=p == 1, backward=p == 2)
        differ += int(not np.array_equal(m_free, match[p, :nt]))
    assert total > 300 and differ == P
    ex.close(); mt.close()


def _map_points(rng, kps, desc, T, k):
    """MapPoints that the camera at pose T (3x4) sees at the frame's keypoints: back-projected at random depths into the world."""
    n = len(kps)
    fx, fy, cx, cy = (float(a) for a in k)
    z = rng.uniform(1.0, 12.0, n)
    Pc = np.stack([(kps["x"] - cx) * z / fx, (kps["y"] - cy) * z / fy, z], 1)
    R, t = T.reshape(3, 4)[:, :3].astype(np.float64), T.reshape(3, 4)[:, 3].astype(np.float64)
    return ((Pc - t) @ R).astype(np.float32)                                   # Xw = R^T (Xc - t)


def test_projection_chain(pkg, batch):
    """orbm_project_last_frame_batch_async against the numpy restatement, bit for bit (valid, u, v, invzc, dir), with points behind the
    camera and just outside each bound and poses for all three directions; the search then reads those device rows directly, stereo
    gate on, and equals the oracle fed with the downloaded rows."""
    B = batch
    L, m, OM, res, cap, sf = B["L"], B["m"], B["OM"], B["res"], B["cap"], B["sf"]
    rng = np.random.default_rng(21)
    T0, NP = 0, 8
    k = EUROC_K; bounds = np.array([0.0, W, 0.0, H], np.float32)
    cur = np.zeros((NP, 12), np.float32); last = np.zeros((NP, 12), np.float32)
    Q = []
    qs = 0
    X3 = []
    for p in range(NP):
        f = T0 + p
        kt, dt = res[f][1], res[f][2]
        cur[p] = random_pose(rng, ang=0.01, trans=0.03)
        step = np.array([0.0, 0.0, (0.0, 0.3, -0.3)[p % 3]], np.float32)       # along the optical axis: dir 0, 1 (forward), 2 (backward)
        last[p] = cur[p]; last[p, [3, 7, 11]] = cur[p, [3, 7, 11]] - cur[p].reshape(3, 4)[:, :3] @ step
        X = _map_points(rng, kt, dt, cur[p], k) if len(kt) else np.zeros((0, 3), np.float32)
        n = len(X)
        if n:
            behind = rng.random(n) < 0.05
            X[behind] = X[behind] * np.float32(-1)
        X3.append(X)
        q = _queries(rng, kt, dt, n, own=True) if n else _queries(rng, kt, dt, 0)
        q["has_mp"] = (rng.random(n) < 0.9).astype(np.uint8)
        Q.append(q)
        qs = max(qs, n)
    # points just outside / on each bound of pair 0's camera
    e = 40
    z = rng.uniform(1, 10, e).astype(np.float32)
    bu = np.array([0, W, k[2], k[2]], np.float32)[np.arange(e) % 4]; bv = np.array([k[3], k[3], 0, H], np.float32)[np.arange(e) % 4]
    eps = np.float32(1e-3) * np.array([-1, 1, -1, 1, 0], np.float32)[np.arange(e) % 5]
    Pc = np.stack([(bu + eps - k[2]) * z / k[0], (bv + eps - k[3]) * z / k[1], z], 1).astype(np.float64)
    R0, t0 = cur[0].reshape(3, 4)[:, :3].astype(np.float64), cur[0].reshape(3, 4)[:, 3].astype(np.float64)
    X3[0] = np.concatenate([X3[0], ((Pc - t0) @ R0).astype(np.float32)])
    Q[0] = {key: np.concatenate([a, a[:e]]) if len(a) else a for key, a in Q[0].items()}
    qs = max(qs, len(X3[0])) + 3
    x3 = np.zeros((NP, qs, 3), np.float32); has = np.zeros((NP, qs), np.uint8)
    for p in range(NP):
        x3[p, :len(X3[p])] = X3[p]; has[p, :len(X3[p])] = Q[p]["has_mp"][:len(X3[p])]
    rows = _Rows(pkg, NP, qs)
    rows.upload(Q)                                                            # octave, angle, qdesc, mp_obs; valid / u / v / invzc / dir come next
    dcur, dlast, dx3, dhas = (pkg.DeviceBuffer(a.nbytes).upload(a) for a in (cur, last, x3, has))
    for mono in (True, False):
        assert L.orbm_project_last_frame_batch_async(m.h, NP, dcur.ptr, dlast.ptr, rows.nq.ptr, qs, dx3.ptr, dhas.ptr, _vp(k), _vp(bounds), MB, int(mono),
                                                     rows.valid.ptr, rows.u.ptr, rows.v.ptr, rows.invzc.ptr, rows.dir.ptr) == 0, L.orbm_last_error()
        m.sync()
        got = [b.download(dt, NP * qs).reshape(NP, qs) for b, dt in ((rows.valid, np.uint8), (rows.u, np.float32), (rows.v, np.float32),
                                                                        (rows.invzc, np.float32))]
        gdir = rows.dir.download(np.uint8, NP)
        ref = project_last_frame_np(cur, last, x3, has, k, bounds, MB, mono)
        for p in range(NP):
            n = len(X3[p])
            for g, rr in zip(got, ref[:4]):
                assert np.array_equal(g[p, :n].view(np.uint8), rr[p, :n].view(np.uint8))
        assert np.array_equal(gdir, ref[4])
        if mono:
            assert np.all(gdir == 0)
        else:
            assert set(gdir.tolist()) == {0, 1, 2}
    valid = got[0]
    assert (valid[0, len(X3[0]) - e:len(X3[0])] == 0).any() and (valid[0, len(X3[0]) - e:len(X3[0])] == 1).any()
    assert ((has != 0) & (valid == 0)).sum() > 50                             # behind the camera
    # the search on the device rows (stereo gate on), no host copy in between
    ur_h = np.stack([_uright(rng, res[T0 + p][1], cap) for p in range(NP)])
    dur = pkg.DeviceBuffer(ur_h.nbytes).upload(ur_h)
    dm = pkg.DeviceBuffer(NP * cap * 4); dn = pkg.DeviceBuffer(NP * 4)
    assert _call(L, m, B["r"], cap, B["gs"], B["gi"], T0, rows, sf, 7.0, dm, dn, uright=dur) == 0, L.orbm_last_error()
    m.sync()
    match = dm.download(np.int32, NP * cap).reshape(NP, cap); nm = dn.download(np.int32, NP)
    u, v, iz = got[1], got[2], got[3]
    total = 0
    for p in range(NP):
        n = len(X3[p])
        q = dict(Q[p]); q.update(valid=valid[p, :n], u=u[p, :n], v=v[p, :n], invzc=iz[p, :n])
        total += _check_pair(pkg, m, OM, sf, res[T0 + p][1], res[T0 + p][2], q, match[p], nm[p], 7.0, d=int(gdir[p]), ur=ur_h[p])[0]
    assert total > 1000


def test_retry(pkg, batch):
    """Tracking.cc:3213-3221 on the device (t_first = 0: pair p searches block frame p).  Pairs 0-2 have every query displaced by 1.5
    windows at th, so they land below retry_below = 20 at th but not at 2 * th: they retry from an empty frame (their blocked slots do
    not apply).  Pair 3 (the empty frame) retries and stays at 0.  Pairs 4-7 match well and keep their first rows.  retry_below = 0
    never retries."""
    B = batch
    L, m, OM, res, cap, sf = B["L"], B["m"], B["OM"], B["res"], B["cap"], B["sf"]
    rng = np.random.default_rng(31)
    NP, th, rb = 8, 7.0, 20
    Q = []
    for p in range(NP):
        kt, dt = res[p][1], res[p][2]
        if p == 3:
            Q.append(_queries(rng, kt, dt, 0))
            continue
        q = _queries(rng, kt, dt, 150 if p < 3 else 900, jitter=0.3)
        q["valid"][:] = 1
        if p < 3:
            q["u"] = (q["u"] + np.float32(1.5 * th) * sf[q["octave"]]).astype(np.float32)
        Q.append(q)
    rows = _Rows(pkg, NP, 900); rows.upload(Q)
    blocked = (rng.random((NP, cap)) < 0.3).astype(np.uint8)
    dblk = pkg.DeviceBuffer(blocked.nbytes).upload(blocked)
    dm = pkg.DeviceBuffer(NP * cap * 4); dn = pkg.DeviceBuffer(NP * 4); dr = pkg.DeviceBuffer(NP)
    for below in (rb, 0):
        dr.upload(np.full(NP, 9, np.uint8))
        assert _call(L, m, B["r"], cap, B["gs"], B["gi"], 0, rows, sf, th, dm, dn, blocked=dblk, retry_below=below, retried=dr) == 0, L.orbm_last_error()
        m.sync()
        match = dm.download(np.int32, NP * cap).reshape(NP, cap); nm = dn.download(np.int32, NP); rt = dr.download(np.uint8, NP)
        if below:
            assert rt.tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
        else:
            assert not rt.any()
        for p in range(NP):
            kt, dt = res[p][1], res[p][2]
            if rt[p]:
                n2, _ = _check_pair(pkg, m, OM, sf, kt, dt, Q[p], match[p], nm[p], 2 * th, blocked=None)
                if p < 3:
                    n1, _ = m.SearchByProjectionFrame(pkg.FrameView(kt, dt, W, H, backend=m), cur_blocked=blocked[p, :len(kt)], scale_factors=sf,
                                                      valid=Q[p]["valid"], u=Q[p]["u"], v=Q[p]["v"], invzc=Q[p]["invzc"], octave=Q[p]["octave"],
                                                      angle=Q[p]["angle"], qdesc=Q[p]["qdesc"], mp_obs=Q[p]["mp_obs"], th=th)
                    assert n1 < rb <= n2, (n1, n2)
            else:
                n1, _ = _check_pair(pkg, m, OM, sf, kt, dt, Q[p], match[p], nm[p], th, blocked=blocked[p])
                assert p >= 4 or not below
                if p >= 4:
                    assert n1 >= rb


def test_capture_replay(pkg, synth):
    """The matcher on the extractor's stream; extract + grid + project + search (with retry) captured into a slot after one eager
    run: the replay's rows equal the eager rows."""
    n = 4
    imgs, dev, arr, stride = _device_batch(pkg, synth, W, H, n, 4300)
    L = pkg.lib()
    ex = pkg.ORBextractor(1000, max_size=(W, H), max_batch=n)
    mt = pkg.ORBmatcher(0.7)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    cap = ex.cap
    ex.enqueue_device(arr, W, H, stride)
    ex.sync()
    res = ex.fetch_all()
    rng = np.random.default_rng(41)
    Q = [_queries(rng, res[i][1], res[i][2], len(res[i][1]), own=True) for i in range(n)]
    qs = max(len(q["u"]) for q in Q)
    rows = _Rows(pkg, n, qs); rows.upload(Q)
    cur = np.stack([random_pose(rng, 0.01, 0.03) for _ in range(n)]); last = cur.copy(); last[:, 11] -= np.float32(0.3)
    x3 = np.zeros((n, qs, 3), np.float32); has = np.zeros((n, qs), np.uint8)
    for i in range(n):
        X = _map_points(rng, res[i][1], res[i][2], cur[i], EUROC_K)
        x3[i, :len(X)] = X; has[i, :len(X)] = 1
    dcur, dlast, dx3, dhas = (pkg.DeviceBuffer(a.nbytes).upload(a) for a in (cur, last, x3, has))
    bounds = np.array([0.0, W, 0.0, H], np.float32)
    r = ex.result_device()
    gs = pkg.DeviceBuffer(n * 3073 * 4); gi = pkg.DeviceBuffer(n * cap * 4)
    dm = pkg.DeviceBuffer(n * cap * 4); dn = pkg.DeviceBuffer(n * 4); dr = pkg.DeviceBuffer(n)
    sf = ex.GetScaleFactors()

    def enqueue():
        ex.enqueue_device(arr, W, H, stride)
        assert L.orbm_grid_build_batch_async(mt.h, r["kps"], r["counts"], n, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0
        assert L.orbm_project_last_frame_batch_async(mt.h, n, dcur.ptr, dlast.ptr, rows.nq.ptr, qs, dx3.ptr, dhas.ptr, _vp(EUROC_K), _vp(bounds), MB, 0,
                                                     rows.valid.ptr, rows.u.ptr, rows.v.ptr, rows.invzc.ptr, rows.dir.ptr) == 0, L.orbm_last_error()
        assert _call(L, mt, r, cap, gs, gi, 0, rows, sf, 15.0, dm, dn, retry_below=20, retried=dr) == 0, L.orbm_last_error()

    enqueue()
    ex.sync()
    eager_m = dm.download(np.int32, n * cap); eager_n = dn.download(np.int32, n); eager_r = dr.download(np.uint8, n)
    assert eager_n.sum() > 200
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    dm.upload(np.full(n * cap, -7, np.int32)); dn.upload(np.full(n, -7, np.int32)); dr.upload(np.full(n, 9, np.uint8))
    assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
    ex.sync()
    assert np.array_equal(dm.download(np.int32, n * cap), eager_m) and np.array_equal(dn.download(np.int32, n), eager_n)
    assert np.array_equal(dr.download(np.uint8, n), eager_r)
    ex.close(); mt.close()


def test_refusals_enqueue_nothing(pkg):
    """A NULL required array, cap > 65535, nlevels > 12, npairs < 1 and q_stride over the limit are refused with the documented codes;
    nothing runs."""
    m = pkg.ORBmatcher()
    L = m.L
    one = pkg.DeviceBuffer(4096)
    dm = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))
    sf = np.ones(16, np.float32)
    p = one.ptr

    def call(cap=4, qs=4, nlev=8, valid=p, npairs=1):
        return L.orbm_search_by_projection_frame_batch_async(m.h, p, p, p, cap, p, p, 0.0, 0.0, INV_W, INV_H, 0, npairs, None, 0.0, None, None,
                                                             p, qs, valid, p, p, p, p, p, p, p, 15.0, 0, _vp(sf), nlev, 1, dm.ptr, dm.ptr, None)
    assert call(cap=65536) == -3 and b"65535" in L.orbm_last_error()
    assert call(qs=(1 << 20) + 1) == -3
    assert call(nlev=13) == -3
    assert call(valid=None) == -2
    assert call(npairs=0) == -2 and call(cap=0) == -2 and call(qs=0) == -2
    k = np.ones(4, np.float32)
    proj = lambda npairs=1, qs=4, x3=p: L.orbm_project_last_frame_batch_async(m.h, npairs, p, p, p, qs, x3, p, _vp(k), _vp(k), 0.1, 0,
                                                                             dm.ptr, dm.ptr, dm.ptr, dm.ptr, dm.ptr)
    assert proj(x3=None) == -2 and proj(npairs=0) == -2 and proj(qs=(1 << 20) + 1) == -3
    m.sync()
    assert np.all(dm.download(np.int32, 16) == 12345)
