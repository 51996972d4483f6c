"""M5 relocalisation SearchByProjection batched on the device (orbm_search_by_projection_kf_batch_async): for every (frame row, candidate
KeyFrame, pose) triple, the match row and nmatches equal, entry for entry, (a) the host entry point ORBmatcher.SearchByProjectionKF on a
FrameView of that frame row and (b) the oracle's SearchByProjectionKF, both fed by reloc_project_np (tests/test_reloc_projection_cpu.py,
pinned bit for bit to the facade's M5 lines).

The frame pools are laid out by hand (random keypoints, uniform octaves, descriptors drawn around a few dozen base descriptors so that
windows hold many near candidates) or come from the extractor.  A KeyFrame's MapPoints are frame keypoints back-projected at random depth
through the KeyFrame pose; the candidate pose is that pose slightly perturbed, so the projections land near their keypoints.
Queries whose log(ratio) / logScaleFactor lies within 1e-4 of an integer (the documented PredictScale caveat) are cleared from valid."""
import ctypes as C

import numpy as np
import pytest

from test_fuse_projection_cpu import F32, camera_centre_np, edge_points, near_integer_level, random_pose
from test_reloc_projection_cpu import behind_points, reloc_project_np

pytestmark = pytest.mark.gpu

W, H = 752, 480
KCAM = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
LOG_SF = F32(np.log(F32(1.2)))
E_INV, E_CAP = -2, -3


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(pkg, a):
    a = np.ascontiguousarray(a)
    return pkg.DeviceBuffer(max(a.nbytes, 4)).upload(a)


def _inv(n, d):
    return float(np.float32(n) / np.float32(d))


class Pool:
    """A frame pool on the device (kps, desc, counts [rows][cap] and its grid) and the host copies the reference reads."""

    def __init__(self, pkg, kps, desc, counts, sf, w=W, h=H):
        self.pkg, self.L = pkg, pkg.lib()
        self.kps, self.desc, self.counts = kps, desc, np.asarray(counts, np.int32)
        self.R, self.cap = kps.shape
        self.sf = np.ascontiguousarray(sf, np.float32); self.nlev = len(self.sf)
        self.w, self.h = w, h
        self.inv_w, self.inv_h = _inv(64, w), _inv(48, h)
        self.bounds = np.array([0, w, 0, h], np.float32)
        self.m = pkg.ORBmatcher(0.9)
        self.dk, self.dd, self.dc = _dev(pkg, kps), _dev(pkg, desc), _dev(pkg, self.counts)
        self.gs = pkg.DeviceBuffer(self.R * 3073 * 4); self.gi = pkg.DeviceBuffer(self.R * self.cap * 4)
        self.grid()
        self.m.sync()

    def grid(self):
        assert self.L.orbm_grid_build_batch_async(self.m.h, self.dk.ptr, self.dc.ptr, self.R, self.cap, 0.0, 0.0, self.inv_w, self.inv_h,
                                                  self.gs.ptr, self.gi.ptr) == 0, self.L.orbm_last_error()

    def row(self, r):
        n = int(self.counts[r])
        return self.kps[r, :n], self.desc[r, :n]


def synth_pool(pkg, rng, counts, cap, w=W, h=H, nlev=8, nbase=48, maxflip=40):
    """Random keypoints on nlev levels (uniform octaves), angles uniform; descriptor = one of nbase base descriptors with up to maxflip
    bits flipped."""
    R = len(counts)
    sf = (np.float32(1.2) ** np.arange(nlev)).astype(np.float32)
    kps = np.zeros((R, cap), pkg.KP_DTYPE); desc = np.zeros((R, cap, 32), np.uint8)
    base = rng.integers(0, 256, (nbase, 32), dtype=np.uint8)
    for f in range(R):
        n = int(counts[f])
        kps[f, :n]["x"] = rng.uniform(0, w - 1, n); kps[f, :n]["y"] = rng.uniform(0, h - 1, n)
        kps[f, :n]["angle"] = rng.uniform(0, 360, n); kps[f, :n]["octave"] = rng.integers(0, nlev, n)
        kps[f, :n]["size"] = 31 * sf[kps[f, :n]["octave"]]; kps[f, :n]["class_id"] = -1
        desc[f, :n] = flip(rng, base[rng.integers(0, nbase, n)], maxflip)
    return Pool(pkg, kps, desc, counts, sf, w, h)


def flip(rng, d, maxflip):
    d = d.copy()
    nflip = rng.integers(0, maxflip + 1, len(d))
    for j in range(maxflip):
        sel = np.flatnonzero(nflip > j); b = rng.integers(0, 256, len(sel))
        d[sel, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return d


def keyframe(rng, pool, row, nq, found=0.0, maxflip=30, src=None):
    """A candidate KeyFrame for frame row `row`: nq MapPoints (its slots) back-projected from frame keypoints at depth 2 .. 20 through a
    random KeyFrame pose, and the candidate pose (that pose perturbed).  mfMaxDistance puts the predicted level at the keypoint's octave
    (sometimes one off); angles mostly one rotation bin off the keypoint's, 15 % strays.  `found` of the valid slots are in sAlreadyFound.
    Returns dict(tcw, ow, pw, mn, mx, angle, qdesc, valid)."""
    kt, dt = pool.row(row)
    tkf = random_pose(rng, 0.5, 1.0)
    tcw = perturb(rng, tkf)
    ow = camera_centre_np(tcw[None])[0]
    if src is None:
        src = rng.integers(0, len(kt), nq)
    k = kt[src]
    z = rng.uniform(2, 20, nq)
    pc = np.stack([(k["x"] - KCAM[2]) * z / KCAM[0], (k["y"] - KCAM[3]) * z / KCAM[1], z], 1)
    T = tkf.reshape(3, 4).astype(np.float64)
    pw = ((pc - T[:, 3]) @ T[:, :3]).astype(F32)
    d = np.linalg.norm(pw.astype(np.float64) - ow.astype(np.float64), axis=1)
    off = rng.choice([0, 0, 0, 0, 0, 0, 0, 1, -1, 0], nq)
    mx = (d * pool.sf[np.clip(k["octave"] + off, 0, pool.nlev - 1)] * 1.2 ** (-rng.uniform(0.2, 0.8, nq))).astype(F32)
    mn = (mx / pool.sf[-1]).astype(F32)
    ang = np.mod(k["angle"] + 14.0 + rng.normal(0, 2, nq), 360).astype(F32)
    stray = rng.random(nq) < 0.15
    ang[stray] = rng.uniform(0, 360, stray.sum()).astype(F32)
    qdesc = flip(rng, dt[src], maxflip) if len(dt) else rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    valid = (rng.random(nq) < 0.9).astype(np.uint8)
    valid[rng.random(nq) < found] = 0                                        # sAlreadyFound
    near = near_integer_level(pw[None], mn[None], mx[None], tcw[None], ow[None], LOG_SF, pool.nlev)[0]
    valid[near] = 0
    return dict(tcw=tcw, ow=ow, pw=pw, mn=mn, mx=mx, angle=ang, qdesc=qdesc, valid=valid)


def perturb(rng, tcw, ang=0.002, trans=0.005):
    D = random_pose(rng, ang, trans).reshape(3, 4).astype(np.float64)
    T = np.asarray(tcw, F32).reshape(3, 4).astype(np.float64)
    return np.concatenate([D[:, :3] @ T[:, :3], (D[:, :3] @ T[:, 3] + D[:, 3])[:, None]], 1).astype(F32).reshape(12)


class Call:
    """The device buffers of one call.  pairs: list of dict(row, blocked [cap] or None, and keyframe()'s fields)."""

    def __init__(self, pool, pairs, qs=None, f_row_null=False, blocked_null=False, rng=None):
        pkg = pool.pkg
        rng = rng or np.random.default_rng(0)
        self.pool, self.pairs, self.P = pool, pairs, len(pairs)
        nq = np.array([len(p["valid"]) for p in pairs], np.int32)
        self.qs = qs or max(int(nq.max()), 1) + 5
        P, qs, cap = self.P, self.qs, pool.cap
        # padding holds garbage (valid set, huge coordinates): the call must not read it
        pw = rng.normal(0, 1e6, (P, qs, 3)).astype(F32); mn = np.zeros((P, qs), F32); mx = np.full((P, qs), 1e9, F32)
        ang = rng.uniform(0, 360, (P, qs)).astype(F32); qd = rng.integers(0, 256, (P, qs, 32), dtype=np.uint8)
        valid = np.ones((P, qs), np.uint8); blk = np.zeros((P, cap), np.uint8)
        for i, p in enumerate(pairs):
            n = nq[i]
            pw[i, :n] = p["pw"]; mn[i, :n] = p["mn"]; mx[i, :n] = p["mx"]; ang[i, :n] = p["angle"]; qd[i, :n] = p["qdesc"]
            valid[i, :n] = p["valid"]
            if p.get("blocked") is not None:
                blk[i] = p["blocked"]
        self.f_row = None if f_row_null else _dev(pkg, np.array([p["row"] for p in pairs], np.int32))
        self.blk = None if blocked_null else _dev(pkg, blk)
        self.tcw = _dev(pkg, np.stack([p["tcw"] for p in pairs]).astype(F32)); self.ow = _dev(pkg, np.stack([p["ow"] for p in pairs]).astype(F32))
        self.nq, self.valid, self.pw = _dev(pkg, nq), _dev(pkg, valid), _dev(pkg, pw)
        self.mn, self.mx, self.ang, self.qd = _dev(pkg, mn), _dev(pkg, mx), _dev(pkg, ang), _dev(pkg, qd)
        self.match = pkg.DeviceBuffer(4 * P * cap); self.nm = pkg.DeviceBuffer(4 * P)

    def enqueue(self, th, orb_dist, check_ori, **over):
        S = self.pool
        a = dict(npairs=self.P, nf_rows=S.R, cap=S.cap, kps=S.dk.ptr, desc=S.dd.ptr, counts=S.dc.ptr, gs=S.gs.ptr, gi=S.gi.ptr,
                 f_row=None if self.f_row is None else self.f_row.ptr, blk=None if self.blk is None else self.blk.ptr,
                 tcw=self.tcw.ptr, ow=self.ow.ptr, nq=self.nq.ptr, qs=self.qs, valid=self.valid.ptr, pw=self.pw.ptr, mn=self.mn.ptr,
                 mx=self.mx.ptr, angle=self.ang.ptr, qdesc=self.qd.ptr, k=_vp(KCAM), bounds=_vp(S.bounds), th=th, orb_dist=orb_dist,
                 sf=_vp(S.sf), nlev=S.nlev, match=self.match.ptr, nm=self.nm.ptr)
        a.update(over)
        return S.L.orbm_search_by_projection_kf_batch_async(
            S.m.h, a["npairs"], a["nf_rows"], a["cap"], a["kps"], a["desc"], a["counts"], a["gs"], a["gi"], 0.0, 0.0, S.inv_w, S.inv_h,
            a["f_row"], a["blk"], a["tcw"], a["ow"], a["nq"], a["qs"], a["valid"], a["pw"], a["mn"], a["mx"], a["angle"], a["qdesc"],
            a["k"], a["bounds"], float(a["th"]), int(a["orb_dist"]), a["sf"], float(LOG_SF), a["nlev"], int(check_ori), a["match"], a["nm"])

    def run(self, th, orb_dist, check_ori):
        rc = self.enqueue(th, orb_dist, check_ori)
        assert rc == 0, self.pool.L.orbm_last_error()
        assert self.pool.L.orbm_sync(self.pool.m.h) == 0
        return self.download()

    def download(self):
        cap = self.pool.cap
        return self.match.download(np.int32, self.P * cap).reshape(self.P, cap), self.nm.download(np.int32, self.P)


def proj_of(pool, p):
    return [a[0] for a in reloc_project_np(p["tcw"][None], p["ow"][None], p["pw"][None], p["mn"][None], p["mx"][None], p["valid"][None],
                                           KCAM, pool.bounds, LOG_SF, pool.nlev)]


def check(pkg, OM, pool, call, got, th, orb_dist, check_ori):
    """Every pair's row and count against the host entry point and the oracle; returns (total matches, pruned, rescans) where a
    rescan is a match preceded in (distance, grid position) rank by at least TK_K window candidates: the eight listed ones were all
    blocked, so the claim kernel had to sweep the window again."""
    match, nm = got
    total = pruned = rescans = 0
    for i, p in enumerate(call.pairs):
        row = match[i]
        r = p["row"]
        if not (0 <= r < pool.R) or len(p["valid"]) == 0 or pool.counts[r] == 0:
            assert nm[i] == 0 and np.all(row == -1), i
            continue
        kt, dt = pool.row(r)
        nt = len(kt)
        ok, u, v, lvl = proj_of(pool, p)
        blocked = np.zeros(nt, np.uint8) if p.get("blocked") is None else p["blocked"][:nt]
        args = dict(blocked=blocked, scale_factors=pool.sf, valid=ok, u=u, v=v, level=np.maximum(lvl, 0), angle=p["angle"], qdesc=p["qdesc"],
                    th=th, orb_dist=orb_dist, check_ori=check_ori)
        n_h, m_h = pool.m.SearchByProjectionKF(pkg.FrameView(kt, dt, pool.w, pool.h, backend=pool.m), **args)
        fo = pkg.FrameView(kt, dt, pool.w, pool.h, backend=OM)
        n_o, m_o = OM.SearchByProjectionKF(fo, **args)
        assert n_h == n_o and np.array_equal(m_h, m_o), i
        assert nm[i] == n_o, (i, nm[i], n_o)
        assert np.array_equal(row[:nt], m_o), (i, np.flatnonzero(row[:nt] != m_o)[:10])
        assert np.all(row[nt:] == -1), i
        total += n_o; pruned += int((m_o == -2).sum())
        pos = np.full(nt, 1 << 30, np.int64)                                 # grid position: the visiting order of the window scan
        pos[fo.grid_idx[:int(fo.grid_start[-1])]] = np.arange(int(fo.grid_start[-1]))
        for k in np.flatnonzero(m_o >= 0):
            q = int(m_o[k])
            rad = F32(th) * pool.sf[lvl[q]]
            inwin = ((np.abs(kt["x"] - u[q]) < rad) & (np.abs(kt["y"] - v[q]) < rad) & (kt["octave"] >= lvl[q] - 1) & (kt["octave"] <= lvl[q] + 1))
            dists = np.unpackbits(dt[inwin] ^ p["qdesc"][q], axis=1).sum(1)
            dk = np.unpackbits(dt[k] ^ p["qdesc"][q]).sum()
            pw_ = pos[inwin]
            rescans += int(((dists < dk) | ((dists == dk) & (pw_ < pos[k]))).sum() >= 8)
    return total, pruned, rescans


@pytest.fixture(scope="module")
def dense(pkg):
    """Four 752x480 frame rows of 4000 - 6000 keypoints (th 10 windows on the upper levels hold dozens) and one empty row; two base
    descriptors, so that a window holds many candidates within ORBdist and one blocked 97 % still yields matches far down its rank."""
    return synth_pool(pkg, np.random.default_rng(500), [6000, 5500, 0, 6000, 4000], 6144, nbase=2)


@pytest.fixture(scope="module")
def OM(oracle):
    return oracle._oracle_matcher_class()()


@pytest.mark.parametrize("passno", [1, 2])
@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("blocked", [0.0, 0.35, 0.97])
def test_relocalization_shape(pkg, OM, dense, passno, check_ori, blocked):
    """One frame row against nine candidates (different KeyFrames, poses, blocked rows and sAlreadyFound none / half / all), at
    th 10 / ORBdist 100 or th 3 / ORBdist 64; a tenth pair with f_row out of range, an eleventh with nq = 0."""
    th, orb_dist = (10.0, 100) if passno == 1 else (3.0, 64)
    rng = np.random.default_rng(passno * 100 + check_ori * 10 + int(blocked * 100))
    pairs = []
    for c in range(9):
        p = keyframe(rng, dense, 0, int(rng.integers(600, 1200)), found=(0.0, 0.5, 1.0)[c % 3])
        p.update(row=0, blocked=(rng.random(dense.cap) < blocked).astype(np.uint8))
        pairs.append(p)
    p = keyframe(rng, dense, 0, 50); p.update(row=dense.R, blocked=None); pairs.append(p)
    p = keyframe(rng, dense, 0, 0); p.update(row=0, blocked=None); pairs.append(p)
    call = Call(dense, pairs, rng=rng)
    got = call.run(th, orb_dist, check_ori)
    total, pruned, rescans = check(pkg, OM, dense, call, got, th, orb_dist, check_ori)
    assert got[1][2::3][:3].max() == 0                                      # sAlreadyFound = all: nothing to match
    if blocked < 0.5:
        assert total > 1000
    if check_ori and blocked < 0.5:
        assert pruned > 0
    if blocked > 0.9 and passno == 1:
        assert total > 20
        if not check_ori:                                                   # (a culled slot no longer names its query)
            assert rescans > 0, (total, rescans)


def test_many_trackers_shape(pkg, OM, dense):
    """Distinct frame rows (one empty, one out of range, -1), each with its own KeyFrame; then f_row = NULL (pair p reads row p) and
    f_blocked = NULL (nothing blocked)."""
    rng = np.random.default_rng(11)
    rows = [0, 1, 2, 3, 4, 1, -1, 7]
    pairs = []
    for r in rows:
        p = keyframe(rng, dense, r if 0 <= r < dense.R and dense.counts[r] else 0, 900, found=0.2)
        p.update(row=r, blocked=(rng.random(dense.cap) < 0.2).astype(np.uint8))
        pairs.append(p)
    call = Call(dense, pairs, rng=rng)
    got = call.run(10.0, 100, True)
    total = check(pkg, OM, dense, call, got, 10.0, 100, True)[0]
    assert total > 1500
    assert got[1][2] == 0 and got[1][6] == 0 and got[1][7] == 0
    for p, r in zip(pairs[:5], range(5)):
        p["row"] = r
        p["blocked"] = None
    c2 = Call(dense, pairs[:5], f_row_null=True, blocked_null=True, rng=rng)
    got2 = c2.run(10.0, 100, True)
    assert check(pkg, OM, dense, c2, got2, 10.0, 100, True)[0] > 1000


def test_colliding_claims(pkg, OM, dense):
    """Each keypoint feeds several slots of the KeyFrame (its MapPoint seen twice), so later queries find their best slot taken by an
    earlier claim: strict blocking (every claim blocks) gives another row than M4's rule, where only the caller's blocked set and
    observed MapPoints block -- computed here with the M4 host entry point on the same windows."""
    rng = np.random.default_rng(21)
    n = 800
    src = np.repeat(rng.integers(0, int(dense.counts[3]), n // 4), 4)
    p = keyframe(rng, dense, 3, n, src=src, maxflip=8)
    p.update(row=3, blocked=None)
    call = Call(dense, [p], rng=rng)
    got = call.run(10.0, 100, False)
    assert check(pkg, OM, dense, call, got, 10.0, 100, False)[0] > 150
    ok, u, v, lvl = proj_of(dense, p)
    kt, dt = dense.row(3)
    n4, m4 = dense.m.SearchByProjectionFrame(pkg.FrameView(kt, dt, W, H, backend=dense.m), cur_blocked=np.zeros(len(kt), np.uint8),
                                             scale_factors=dense.sf, valid=ok, u=u, v=v, invzc=np.zeros(n, F32), octave=np.maximum(lvl, 0),
                                             angle=p["angle"], qdesc=p["qdesc"], mp_obs=np.zeros(n, np.uint8), th=10.0, check_ori=False)
    assert n4 > 0 and not np.array_equal(got[0][0, :len(kt)], m4)


def test_gate_edges(pkg, OM, dense):
    """One pair per case, each with its own pose: points behind the camera whose projection lands in the image (M5 has no depth test),
    projections exactly on minX / maxX / minY / maxY (closed bounds: all accepted), and ordinary points."""
    rng = np.random.default_rng(31)
    pairs = []
    S_id = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    Xe, hit, _ = edge_points(rng, S_id, KCAM, dense.bounds, 80)
    assert hit.mean() > 0.8
    for i in range(240):
        row = [0, 1, 3, 4][i % 4]
        kt, dt = dense.row(row)
        if i < 80:
            tcw, X = S_id, Xe[i]
        else:
            tcw = random_pose(rng, 0.5, 1.0)
            X = behind_points(rng, tcw, KCAM, dense.bounds, 1)[0] if i < 160 else keyframe(rng, dense, row, 1)["pw"][0]
        ow = camera_centre_np(tcw[None])[0]
        d = np.linalg.norm(X.astype(np.float64) - ow)
        mx = np.array([d * 1.2 ** rng.uniform(0.2, 6.8)], F32)
        valid = np.ones(1, np.uint8)
        valid[near_integer_level(X[None, None], np.zeros((1, 1), F32), mx[None], tcw[None], ow[None], LOG_SF, dense.nlev)[0]] = 0
        pairs.append(dict(row=row, blocked=None, tcw=tcw, ow=ow, pw=X[None].astype(F32), mn=(mx / F32(10)).astype(F32), mx=mx,
                          angle=rng.uniform(0, 360, 1).astype(F32), qdesc=dt[rng.integers(0, len(dt), 1)], valid=valid))
    call = Call(dense, pairs, rng=rng)
    got = call.run(10.0, 100, False)
    check(pkg, OM, dense, call, got, 10.0, 100, False)
    oks = np.array([proj_of(dense, p)[0][0] for p in pairs])
    assert oks[:80].sum() > 50 and oks[80:160].sum() > 50                   # edges and points behind the camera pass the gates
    assert got[1][80:160].sum() > 0                                         # and some of them match


def test_12_levels_and_large_cap(pkg, OM):
    """A 12-level pyramid (levels up to 11 predicted and searched), and a 1920x1080 pool of 20 480 slots (20 000 / 19 000 keypoints)."""
    rng = np.random.default_rng(41)
    p12 = synth_pool(pkg, rng, [3000, 3000], 3072, nlev=12)
    pairs = []
    for r in (0, 1, 0):
        p = keyframe(rng, p12, r, 1000, found=0.1)
        p.update(row=r, blocked=(rng.random(p12.cap) < 0.3).astype(np.uint8))
        pairs.append(p)
    call = Call(p12, pairs, rng=rng)
    got = call.run(10.0, 100, True)
    assert check(pkg, OM, p12, call, got, 10.0, 100, True)[0] > 800
    assert max(proj_of(p12, p)[3].max() for p in pairs) == 11
    big = synth_pool(pkg, rng, [20000, 19000], 20480, w=1920, h=1080)
    pairs = []
    for r in (0, 1):
        p = keyframe(rng, big, r, 3000)
        p.update(row=r, blocked=(rng.random(big.cap) < 0.35).astype(np.uint8))
        pairs.append(p)
    call = Call(big, pairs, rng=rng)
    for th, od in ((10.0, 100), (3.0, 64)):
        got = call.run(th, od, True)
        assert check(pkg, OM, big, call, got, th, od, True)[0] > 1000
        assert np.all(got[0][1, 19000:] == -1)


def test_extractor_pool_both_passes(pkg, OM, synth):
    """Frame rows from the extractor (synthetic images): the th 10 / ORBdist 100 pass, then the th 3 / ORBdist 64 pass with the first
    pass's matches blocked and sAlreadyFound rebuilt from its row, as Tracking::Relocalization chains them."""
    NB = 3
    ex = pkg.ORBextractor(1500, max_size=(W, H), max_batch=NB)
    res = ex.extract_batch([synth.gen_image(W, H, 5100 + i) for i in range(NB)], [(0, 1000)] * NB)
    cap = max(len(res[f][1]) for f in range(NB))
    kps = np.zeros((NB, cap), pkg.KP_DTYPE); desc = np.zeros((NB, cap, 32), np.uint8)
    counts = [len(res[f][1]) for f in range(NB)]
    for f in range(NB):
        kps[f, :counts[f]] = res[f][1]; desc[f, :counts[f]] = res[f][2]
    pool = Pool(pkg, kps, desc, counts, ex.GetScaleFactors())
    rng = np.random.default_rng(51)
    pairs = []
    for c in range(8):
        p = keyframe(rng, pool, 0 if c < 6 else c - 5, 700, found=0.3, maxflip=40)
        p.update(row=0 if c < 6 else c - 5, blocked=(rng.random(cap) < 0.3).astype(np.uint8))
        pairs.append(p)
    call = Call(pool, pairs, rng=rng)
    got = call.run(10.0, 100, True)
    assert check(pkg, OM, pool, call, got, 10.0, 100, True)[0] > 1500
    for i, p in enumerate(pairs):                                           # pass 2 state
        row = got[0][i]
        p["blocked"] = (p["blocked"] | (row >= 0)).astype(np.uint8)
        found = np.zeros(len(p["valid"]), bool); found[row[row >= 0]] = True
        p["valid"] = (p["valid"] & ~found).astype(np.uint8)
        p["tcw"] = perturb(rng, p["tcw"], 0.0005, 0.001); p["ow"] = camera_centre_np(p["tcw"][None])[0]
        p["valid"][near_integer_level(p["pw"][None], p["mn"][None], p["mx"][None], p["tcw"][None], p["ow"][None], LOG_SF, pool.nlev)[0]] = 0
    call2 = Call(pool, pairs, rng=rng)
    got2 = call2.run(3.0, 64, True)
    assert check(pkg, OM, pool, call2, got2, 3.0, 64, True)[0] > 10


def test_capture_replay_equals_eager(pkg, synth, dense):
    """A step (an extraction, the pool's grid build and the batched search) captured into a graph and replayed gives the eager rows and
    counts."""
    L = dense.L
    rng = np.random.default_rng(61)
    pairs = []
    for c in range(8):
        p = keyframe(rng, dense, 0, 900, found=0.1)
        p.update(row=0, blocked=(rng.random(dense.cap) < 0.3).astype(np.uint8))
        pairs.append(p)
    call = Call(dense, pairs, rng=rng)
    ex = pkg.ORBextractor(1000, max_size=(W, H), max_batch=1)
    stride = (W + 63) // 64 * 64
    dimg = pkg.DeviceBuffer(stride * H)
    pad = np.zeros((H, stride), np.uint8); pad[:, :W] = synth.gen_image(W, H, 61)
    dimg.upload(pad)
    arr = (C.c_void_p * 1)(dimg.ptr)
    assert L.orbm_set_stream(dense.m.h, L.orbx_stream(ex.h)) == 0
    try:
        def enqueue():
            ex.enqueue_device(arr, W, H, stride, np.zeros(4, np.int32))
            dense.grid()
            assert call.enqueue(10.0, 100, True) == 0, L.orbm_last_error()

        enqueue()
        assert L.orbm_sync(dense.m.h) == 0
        eager = call.download()
        assert eager[1].sum() > 1000
        assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
        enqueue()
        assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
        call.match.upload(np.full(call.P * dense.cap, -7, np.int32)); call.nm.upload(np.full(call.P, -7, np.int32))
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        replay = call.download()
        for a, b in zip(eager, replay):
            assert np.array_equal(a, b)
    finally:
        assert L.orbm_set_stream(dense.m.h, None) == 0


def test_refusals_enqueue_nothing(pkg, dense):
    """Each refusal returns its documented code; the outputs keep their sentinel."""
    L = dense.L
    rng = np.random.default_rng(71)
    p = keyframe(rng, dense, 0, 64); p.update(row=0, blocked=None)
    call = Call(dense, [p, dict(p)], rng=rng)
    call.match.upload(np.full(2 * dense.cap, 12345, np.int32)); call.nm.upload(np.full(2, 12345, np.int32))
    for over in (dict(kps=None), dict(desc=None), dict(counts=None), dict(gs=None), dict(gi=None), dict(tcw=None), dict(ow=None),
                 dict(nq=None), dict(valid=None), dict(pw=None), dict(mn=None), dict(mx=None), dict(angle=None), dict(qdesc=None),
                 dict(k=None), dict(bounds=None), dict(sf=None), dict(match=None), dict(nm=None),
                 dict(npairs=0), dict(nf_rows=0), dict(cap=0), dict(qs=0), dict(nlev=0)):
        assert call.enqueue(10.0, 100, True, **over) == E_INV, over
    assert call.enqueue(10.0, 256, True) == E_INV
    assert call.enqueue(float("nan"), 100, True) == E_INV and call.enqueue(float("inf"), 64, False) == E_INV
    for over in (dict(cap=65536), dict(qs=(1 << 20) + 1), dict(nlev=13), dict(npairs=65536)):
        assert call.enqueue(10.0, 100, True, **over) == E_CAP, over
    assert L.orbm_sync(dense.m.h) == 0
    match, nm = call.download()
    assert np.all(match == 12345) and np.all(nm == 12345)
    # a negative ORBdist is accepted and matches nothing
    got = call.run(10.0, -1, True)
    assert np.all(got[0] == -1) and np.all(got[1] == 0)
