"""M6 Sim3 SearchByProjection batched on the device (orbm_search_by_projection_sim3_batch_async): for every (KeyFrame row, Sim3 pose,
MapPoint row) triple, the match row and nmatches equal, entry for entry, (a) the host entry point ORBmatcher.SearchByProjectionSim3 on a
FrameView of that row and (b) the oracle's SearchByProjectionSim3, both fed by sim3_project_np (tests/test_sim3_projection_cpu.py, pinned
bit for bit to the facade's sim3_gates lines) in the call's projection form.  Pools and MapPoints are laid out as in
tests/test_gpu_reloc_batch.py; normals point along the viewing ray, a tenth of them at random (the 60 degree gate rejects most of those)."""
import ctypes as C

import numpy as np
import pytest

from test_fuse_projection_cpu import F32, camera_centre_np, near_integer_level, random_pose
from test_gpu_reloc_batch import KCAM, LOG_SF, H, W, Pool, _dev, _vp, flip, keyframe, synth_pool
from test_sim3_projection_cpu import S_ID, edge_points_form, forms_differ_point, sim3_project_np

pytestmark = pytest.mark.gpu
E_INV, E_CAP = -2, -3


def mappoints(rng, pool, row, nq, found=0.0, maxflip=30, src=None):
    p = keyframe(rng, pool, row, nq, found=found, maxflip=maxflip, src=src)
    PO = p["pw"].astype(np.float64) - p["ow"].astype(np.float64)
    nrm = PO / np.maximum(np.linalg.norm(PO, axis=1, keepdims=True), 1e-30)
    stray = rng.random(nq) < 0.1
    r = rng.normal(0, 1, (int(stray.sum()), 3)); nrm[stray] = r / np.linalg.norm(r, axis=1, keepdims=True)
    p["normal"] = nrm.astype(F32)
    return p


class Call:
    """The device buffers of one call.  pairs: list of dict(row, matched [cap] or None, and mappoints()'s fields)."""

    def __init__(self, pool, pairs, row_null=False, matched_null=False, rng=None):
        pkg = pool.pkg
        rng = rng or np.random.default_rng(0)
        self.pool, self.pairs, self.P = pool, pairs, len(pairs)
        nq = np.array([len(p["valid"]) for p in pairs], np.int32)
        self.qs = max(int(nq.max()), 1) + 5
        P, qs, cap = self.P, self.qs, pool.cap
        pw = rng.normal(0, 1e6, (P, qs, 3)).astype(F32); nr = rng.normal(0, 1, (P, qs, 3)).astype(F32)     # padding: garbage nobody may read
        mn = np.zeros((P, qs), F32); mx = np.full((P, qs), 1e9, F32)
        qd = rng.integers(0, 256, (P, qs, 32), dtype=np.uint8); valid = np.ones((P, qs), np.uint8); mt = np.zeros((P, cap), np.uint8)
        for i, p in enumerate(pairs):
            n = nq[i]
            pw[i, :n] = p["pw"]; nr[i, :n] = p["normal"]; mn[i, :n] = p["mn"]; mx[i, :n] = p["mx"]; qd[i, :n] = p["qdesc"]; valid[i, :n] = p["valid"]
            if p.get("matched") is not None:
                mt[i] = p["matched"]
        self.kf_row = None if row_null else _dev(pkg, np.array([p["row"] for p in pairs], np.int32))
        self.mt = None if matched_null else _dev(pkg, mt)
        self.tcw = _dev(pkg, np.stack([p["tcw"] for p in pairs]).astype(F32)); self.ow = _dev(pkg, np.stack([p["ow"] for p in pairs]).astype(F32))
        self.nq, self.valid, self.pw, self.nr = _dev(pkg, nq), _dev(pkg, valid), _dev(pkg, pw), _dev(pkg, nr)
        self.mn, self.mx, self.qd = _dev(pkg, mn), _dev(pkg, mx), _dev(pkg, qd)
        self.match = pkg.DeviceBuffer(4 * P * cap); self.nm = pkg.DeviceBuffer(4 * P)

    def enqueue(self, th, ratio, form, **over):
        S = self.pool
        a = dict(npairs=self.P, rows=S.R, cap=S.cap, kps=S.dk.ptr, desc=S.dd.ptr, counts=S.dc.ptr, gs=S.gs.ptr, gi=S.gi.ptr,
                 kf_row=None if self.kf_row is None else self.kf_row.ptr, mt=None if self.mt is None else self.mt.ptr,
                 tcw=self.tcw.ptr, ow=self.ow.ptr, nq=self.nq.ptr, qs=self.qs, valid=self.valid.ptr, pw=self.pw.ptr, normal=self.nr.ptr,
                 mn=self.mn.ptr, mx=self.mx.ptr, qdesc=self.qd.ptr, k=_vp(KCAM), bounds=_vp(S.bounds), sf=_vp(S.sf), nlev=S.nlev,
                 match=self.match.ptr, nm=self.nm.ptr)
        a.update(over)
        return S.L.orbm_search_by_projection_sim3_batch_async(
            S.m.h, a["npairs"], a["rows"], a["cap"], a["kps"], a["desc"], a["counts"], a["gs"], a["gi"], 0.0, 0.0, S.inv_w, S.inv_h,
            a["kf_row"], a["mt"], a["tcw"], a["ow"], a["nq"], a["qs"], a["valid"], a["pw"], a["normal"], a["mn"], a["mx"], a["qdesc"],
            a["k"], a["bounds"], int(th), float(ratio), int(form), a["sf"], float(LOG_SF), a["nlev"], a["match"], a["nm"])

    def run(self, th, ratio, form):
        rc = self.enqueue(th, ratio, form)
        assert rc == 0, self.pool.L.orbm_last_error()
        assert self.pool.L.orbm_sync(self.pool.m.h) == 0
        return self.download()

    def download(self):
        cap = self.pool.cap
        return self.match.download(np.int32, self.P * cap).reshape(self.P, cap), self.nm.download(np.int32, self.P)


def proj_of(pool, p, form):
    return [a[0] for a in sim3_project_np(p["tcw"][None], p["ow"][None], p["pw"][None], p["normal"][None], p["mn"][None], p["mx"][None],
                                          p["valid"][None], KCAM, pool.bounds, LOG_SF, pool.nlev, form)]


def check(pkg, OM, pool, call, got, th, ratio, form):
    """Every pair's row and count against the host entry point and the oracle.  Returns, all from the ORACLE's rows: matches per pair,
    and the numbers of rescans (a match ranked behind >= 8 window candidates: the listed eight were all blocked), of queries refused only
    because of matched_in (the oracle matches more with an empty matched_in) and only because of the level band (an unmatched query whose
    window holds a free slot within the distance bound one level outside [level-1, level] and none inside)."""
    match, nm = got
    per = []
    rescans = only_matched = only_band = 0
    for i, p in enumerate(call.pairs):
        row = match[i]
        r = p["row"]
        if not (0 <= r < pool.R) or len(p["valid"]) == 0 or pool.counts[r] == 0:
            assert nm[i] == 0 and np.all(row == -1), i
            per.append(-1)
            continue
        kt, dt = pool.row(r)
        nt = len(kt)
        ok, u, v, lvl = proj_of(pool, p, form)
        mt_in = np.zeros(nt, np.uint8) if p.get("matched") is None else p["matched"][:nt]
        args = dict(scale_factors=pool.sf, valid=ok, u=u, v=v, level=np.maximum(lvl, 0), qdesc=p["qdesc"], th=th, ratio_hamming=ratio)
        n_h, m_h = pool.m.SearchByProjectionSim3(pkg.FrameView(kt, dt, pool.w, pool.h, backend=pool.m), matched_in=mt_in, **args)
        fo = pkg.FrameView(kt, dt, pool.w, pool.h, backend=OM)
        n_o, m_o = OM.SearchByProjectionSim3(fo, matched_in=mt_in, **args)
        assert n_h == n_o and np.array_equal(m_h, m_o), i
        assert nm[i] == n_o, (i, nm[i], n_o)
        assert np.array_equal(row[:nt], m_o), (i, np.flatnonzero(row[:nt] != m_o)[:10])
        assert np.all(row[nt:] == -1), i
        per.append(n_o)
        if mt_in.any():
            only_matched += max(0, OM.SearchByProjectionSim3(fo, matched_in=np.zeros(nt, np.uint8), **args)[0] - n_o)
        pos = np.full(nt, 1 << 30, np.int64)
        pos[fo.grid_idx[:int(fo.grid_start[-1])]] = np.arange(int(fo.grid_start[-1]))
        taken = mt_in.astype(bool) | (m_o >= 0)
        matched_q = np.zeros(len(ok), bool); matched_q[m_o[m_o >= 0]] = True
        for k in np.flatnonzero(m_o >= 0)[:400]:
            q = int(m_o[k])
            rad = F32(th) * pool.sf[lvl[q]]
            inwin = (np.abs(kt["x"] - u[q]) < rad) & (np.abs(kt["y"] - v[q]) < rad) & (kt["octave"] >= lvl[q] - 1) & (kt["octave"] <= lvl[q])
            dists = np.unpackbits(dt[inwin] ^ p["qdesc"][q], axis=1).sum(1)
            dk = np.unpackbits(dt[k] ^ p["qdesc"][q]).sum()
            rescans += int(((dists < dk) | ((dists == dk) & (pos[inwin] < pos[k]))).sum() >= 8)
        for q in np.flatnonzero(ok.astype(bool) & ~matched_q)[:400]:
            rad = F32(th) * pool.sf[lvl[q]]
            near = (np.abs(kt["x"] - u[q]) < rad) & (np.abs(kt["y"] - v[q]) < rad) & ~taken
            if not near.any():
                continue
            d = np.unpackbits(dt[near] ^ p["qdesc"][q], axis=1).sum(1).astype(np.float32)
            band = (kt["octave"][near] >= lvl[q] - 1) & (kt["octave"][near] <= lvl[q])
            good = d <= np.float32(50) * np.float32(ratio)
            only_band += int(np.any(good & ~band) and not np.any(good & band))
    return np.array(per), rescans, only_matched, only_band


@pytest.fixture(scope="module")
def dense(pkg):
    return synth_pool(pkg, np.random.default_rng(600), [6000, 5500, 0, 6000, 4000], 6144, nbase=2)


@pytest.fixture(scope="module")
def crowded(pkg):
    """One row of 32 000 keypoints on a 480x360 image (the batched grid build sorts at most 32 768 slots per row) and an empty one: at
    th 5 and th 3 a window on the upper levels (radius 3 * 1.2^7 = 10.7 px) still holds ~20 candidates of the level band, so a list of
    eight can be blocked entirely while the window holds more.  On the 6000-keypoint 752x480 rows of `dense` such a window holds about
    two and the rescan could never be taken."""
    return synth_pool(pkg, np.random.default_rng(601), [32000, 0], 32768, w=480, h=360, nbase=2)


@pytest.fixture(scope="module")
def OM(oracle):
    return oracle._oracle_matcher_class()()


@pytest.mark.parametrize("form,th,ratio", [(1, 8, 1.5), (0, 5, 1.0), (0, 3, 1.5)])
@pytest.mark.parametrize("matched", [0.0, 0.35, 0.97])
def test_place_recognition_shape(pkg, OM, dense, crowded, form, th, ratio, matched):
    """One KeyFrame row under nine poses (valid none / half / all by threes), a pair with kf_row out of range, one with nq = 0 and one
    on an empty row; LoopClosing's three parameter sets.  th 8 runs on the 6000-keypoint row, th 5 and th 3 on the crowded 32 000-keypoint row,
    so that at every radius the all-8-blocked rescan is taken at 97 % matched_in -- asserted from the oracle's replay."""
    pool = dense if th == 8 else crowded
    empty = 2 if th == 8 else 1
    rng = np.random.default_rng(form * 1000 + th * 10 + int(matched * 100))
    pairs = []
    for c in range(9):
        p = mappoints(rng, pool, 0, int(rng.integers(600, 1200)), found=(0.0, 0.5, 1.0)[c % 3])
        p.update(row=0, matched=(rng.random(pool.cap) < matched).astype(np.uint8))
        pairs.append(p)
    p = mappoints(rng, pool, 0, 50); p.update(row=pool.R, matched=None); pairs.append(p)
    p = mappoints(rng, pool, 0, 0); p.update(row=0, matched=None); pairs.append(p)
    p = mappoints(rng, pool, 0, 50); p.update(row=empty, matched=None); pairs.append(p)
    call = Call(pool, pairs, rng=rng)
    got = call.run(th, ratio, form)
    per, rescans, only_matched, only_band = check(pkg, OM, pool, call, got, th, ratio, form)
    assert np.all(per[2:9:3] == 0)                                          # valid none
    live = np.array([0, 1, 3, 4, 6, 7])
    if matched < 0.5:
        assert (per[live] > 0).sum() > len(live) / 2 and per[live].sum() > 300, per
        assert only_band > 0, only_band
    if matched > 0.0:
        assert only_matched > 0
    if matched > 0.9:
        assert per[live].sum() > 10 and rescans > 0, (th, per, rescans)


def test_distinct_rows_and_null_arrays(pkg, OM, dense):
    rng = np.random.default_rng(12)
    rows = [0, 1, 2, 3, 4, 1, -1, 7]
    pairs = []
    for r in rows:
        p = mappoints(rng, dense, r if 0 <= r < dense.R and dense.counts[r] else 0, 900, found=0.2)
        p.update(row=r, matched=(rng.random(dense.cap) < 0.2).astype(np.uint8))
        pairs.append(p)
    call = Call(dense, pairs, rng=rng)
    per = check(pkg, OM, dense, call, call.run(8, 1.5, 1), 8, 1.5, 1)[0]
    assert per[[0, 1, 3, 4, 5]].min() > 50, per
    for p, r in zip(pairs[:5], range(5)):
        p["row"] = r; p["matched"] = None
    c2 = Call(dense, pairs[:5], row_null=True, matched_null=True, rng=rng)
    assert check(pkg, OM, dense, c2, c2.run(8, 1.5, 0), 8, 1.5, 0)[0][[0, 1, 3, 4]].min() > 50


def test_colliding_queries(pkg, OM, dense):
    """Each keypoint is the source of four MapPoints: later queries find their best slot claimed and take another or nothing."""
    rng = np.random.default_rng(22)
    n = 800
    src = np.repeat(rng.integers(0, int(dense.counts[3]), n // 4), 4)
    p = mappoints(rng, dense, 3, n, src=src, maxflip=8)
    p.update(row=3, matched=None)
    call = Call(dense, [p], rng=rng)
    got = call.run(8, 1.5, 1)
    assert check(pkg, OM, dense, call, got, 8, 1.5, 1)[0][0] > 150
    row = got[0][0]; q = row[row >= 0]
    assert len(np.unique(q)) == len(q) and len(np.unique(src[q])) < len(q)   # several MapPoints of one source keypoint matched different slots


@pytest.mark.parametrize("ratio,at,above", [(1.5, 75, 76), (1.0, 50, 51)])
def test_distance_bound_is_inclusive(pkg, OM, ratio, at, above):
    """Hand-built descriptors: a slot at Hamming distance exactly 50 * ratio matches, one above does not."""
    rng = np.random.default_rng(33)
    n = 40
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    kps = np.zeros((1, 64), pkg.KP_DTYPE); desc = np.zeros((1, 64, 32), np.uint8)
    kps[0, :n]["x"] = 60 + 70 * (np.arange(n) % 9); kps[0, :n]["y"] = 60 + 80 * (np.arange(n) // 9); kps[0, :n]["octave"] = 2
    desc[0, :n] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pool = Pool(pkg, kps, desc, [n], sf)
    tcw = S_ID.copy(); ow = np.zeros(3, F32)
    z = 5.0
    pw = np.stack([(kps[0, :n]["x"] - KCAM[2]) * z / KCAM[0], (kps[0, :n]["y"] - KCAM[3]) * z / KCAM[1], np.full(n, z)], 1).astype(F32)
    d = np.linalg.norm(pw.astype(np.float64), axis=1)
    mx = (d * 1.2 ** 1.5).astype(F32); mn = (mx / F32(4)).astype(F32)       # predicted level 2
    qd = desc[0, :n].copy()
    nflip = np.where(np.arange(n) % 2 == 0, at, above)
    for i in range(n):
        for b in range(nflip[i]):
            qd[i, b >> 3] ^= np.uint8(1 << (b & 7))
    p = dict(row=0, matched=None, tcw=tcw, ow=ow, pw=pw, normal=(pw / d[:, None]).astype(F32), mn=mn, mx=mx, qdesc=qd, valid=np.ones(n, np.uint8))
    call = Call(pool, [p], rng=rng)
    got = call.run(3, ratio, 0)
    per = check(pkg, OM, pool, call, got, 3, ratio, 0)[0]
    row = got[0][0, :n]
    assert per[0] == n // 2 and np.all(row[0::2] == np.arange(0, n, 2)) and np.all(row[1::2] == -1)


@pytest.mark.parametrize("form", [0, 1])
def test_gate_edges(pkg, OM, dense, form):
    """One pair per point: projections exactly on each bound in the call's form (min accepted, max rejected), points just behind and
    just in front of the camera, points where the two forms round differently, ordinary points."""
    rng = np.random.default_rng(34 + form)
    Xe, hit, which = edge_points_form(rng, KCAM, dense.bounds, 80, form)
    assert hit.mean() > 0.8
    df = forms_differ_point(KCAM)[:40]
    pairs = []
    for i in range(200):
        row = [0, 1, 3, 4][i % 4]
        kt, dt = dense.row(row)
        if i < 80:
            X = Xe[i]
        elif i < 120:
            X = df[i - 80]
        elif i < 160:
            X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.choice([-3.0, -1e-3, 1e-3, 3.0])], F32)
        else:
            X = None
        if X is None:
            p = mappoints(rng, dense, row, 1)
        else:
            d = float(np.linalg.norm(X.astype(np.float64)))
            mx = np.array([d * 1.2 ** rng.uniform(0.2, 6.8)], F32)
            valid = np.ones(1, np.uint8)
            valid[near_integer_level(X[None, None], np.zeros((1, 1), F32), mx[None], S_ID[None], np.zeros((1, 3), F32), LOG_SF, dense.nlev)[0]] = 0
            p = dict(tcw=S_ID.copy(), ow=np.zeros(3, F32), pw=X[None].astype(F32), normal=(X[None] / max(d, 1e-30)).astype(F32),
                     mn=(mx / F32(10)).astype(F32), mx=mx, qdesc=dt[rng.integers(0, len(dt), 1)], valid=valid)
        p.update(row=row, matched=None)
        pairs.append(p)
    call = Call(dense, pairs, rng=rng)
    got = call.run(8, 1.5, form)
    check(pkg, OM, dense, call, got, 8, 1.5, form)
    oks = np.array([proj_of(dense, p, form)[0][0] for p in pairs])
    lo = np.flatnonzero(hit & (which % 2 == 0)); hi = np.flatnonzero(hit & (which % 2 == 1))
    assert oks[lo].sum() > 0.8 * len(lo) and oks[hi].sum() == 0
    zs = np.array([p["pw"][0, 2] for p in pairs[120:160]])
    assert np.all(oks[120:160][zs < 0] == 0) and oks[120:160][zs > 0].sum() > 0
    assert got[1][:80].sum() + got[1][160:].sum() > 0


def test_12_levels_and_large_cap(pkg, OM):
    rng = np.random.default_rng(42)
    p12 = synth_pool(pkg, rng, [3000, 3000], 3072, nlev=12)
    pairs = []
    for r in (0, 1, 0):
        p = mappoints(rng, p12, r, 1000, found=0.1)
        p.update(row=r, matched=(rng.random(p12.cap) < 0.3).astype(np.uint8))
        pairs.append(p)
    call = Call(p12, pairs, rng=rng)
    assert check(pkg, OM, p12, call, call.run(8, 1.5, 1), 8, 1.5, 1)[0].sum() > 300
    assert max(proj_of(p12, p, 1)[3].max() for p in pairs) == 11
    big = synth_pool(pkg, rng, [20000, 19000], 20480, w=1920, h=1080)
    pairs = []
    for r in (0, 1):
        p = mappoints(rng, big, r, 3000)
        p.update(row=r, matched=(rng.random(big.cap) < 0.35).astype(np.uint8))
        pairs.append(p)
    call = Call(big, pairs, rng=rng)
    for th, ratio, form in ((8, 1.5, 1), (5, 1.0, 0)):
        got = call.run(th, ratio, form)
        assert check(pkg, OM, big, call, got, th, ratio, form)[0].sum() > 300
        assert np.all(got[0][1, 19000:] == -1)


def test_capture_replay_equals_eager(pkg, synth, dense):
    L = dense.L
    rng = np.random.default_rng(62)
    pairs = []
    for c in range(6):
        p = mappoints(rng, dense, 0, 900, found=0.1)
        p.update(row=0, matched=(rng.random(dense.cap) < 0.3).astype(np.uint8))
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
            assert call.enqueue(8, 1.5, 1) == 0, L.orbm_last_error()

        enqueue()
        assert L.orbm_sync(dense.m.h) == 0
        eager = call.download()
        assert eager[1].sum() > 500
        assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
        enqueue()
        assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
        call.match.upload(np.full(call.P * dense.cap, -7, np.int32)); call.nm.upload(np.full(call.P, -7, np.int32))
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        for a, b in zip(eager, call.download()):
            assert np.array_equal(a, b)
    finally:
        assert L.orbm_set_stream(dense.m.h, None) == 0


def test_refusals_enqueue_nothing(pkg, dense):
    L = dense.L
    rng = np.random.default_rng(72)
    p = mappoints(rng, dense, 0, 64); p.update(row=0, matched=None)
    call = Call(dense, [p, dict(p)], rng=rng)
    call.match.upload(np.full(2 * dense.cap, 12345, np.int32)); call.nm.upload(np.full(2, 12345, np.int32))
    for over in (dict(kps=None), dict(desc=None), dict(counts=None), dict(gs=None), dict(gi=None), dict(tcw=None), dict(ow=None),
                 dict(nq=None), dict(valid=None), dict(pw=None), dict(normal=None), dict(mn=None), dict(mx=None), dict(qdesc=None),
                 dict(k=None), dict(bounds=None), dict(sf=None), dict(match=None), dict(nm=None),
                 dict(npairs=0), dict(rows=0), dict(cap=0), dict(qs=0), dict(nlev=0)):
        assert call.enqueue(8, 1.5, 1, **over) == E_INV, over
    for ratio in (float("nan"), float("inf"), 5.12, 6.0):                   # 50 * ratio >= 256: the reference would write vpMatched[-1]
        assert call.enqueue(8, ratio, 1) == E_INV, ratio
    assert call.enqueue(8, 1.5, 2) == E_INV and call.enqueue(8, 1.5, -1) == E_INV
    for over in (dict(cap=65536), dict(qs=(1 << 20) + 1), dict(nlev=13), dict(npairs=65536)):
        assert call.enqueue(8, 1.5, 1, **over) == E_CAP, over
    assert L.orbm_sync(dense.m.h) == 0
    match, nm = call.download()
    assert np.all(match == 12345) and np.all(nm == 12345)
    got = call.run(8, 5.1, 1)                                               # a large legal ratio: every free window candidate is accepted
    assert got[1].sum() > 0
