"""The routes of the batched SearchByProjection(Frame, Frame) list kernel (k_track_topk16), each forced by a constructed input:
windows of <= 8, 9-16 and 17-32 grid entries (one to two entries per lane), windows of more than 64 entries (feed-back passes),
rows with more than 16 candidates that pass the level and window tests (more than one round of 16 per pass, in the first pass and in
a later one), exactly 8 and exactly 9 such candidates, empty windows and an empty frame, frame counts that are no multiple of 8, 16
or 32, and query frames whose levels mix inside one 16-query workgroup.  The frames are synthetic keypoint / descriptor arrays (no
extraction): that each scene has its properties is checked on the CPU with the oracle's grid and GetFeaturesInArea
(test_scenes_have_their_routes, no GPU), and on the GPU every pair's match row and count must equal the oracle's
SearchByProjectionFrame entry for entry."""
import ctypes as C

import numpy as np
import pytest

W, H = 752, 480
F32 = np.float32
SF = np.ones(8, F32)
for _i in range(1, 8):
    SF[_i] = F32(SF[_i - 1] * F32(1.2))

# blob sizes of the cluster frames: same-level keypoints within +-3 px of a lattice point 150 px from the next one
BLOBS = [8, 9, 16, 17, 20, 33, 40, 70, 100, 7, 1, 15, 8, 9, 130]
BLOB_LEVEL = 2


def _flip(rng, base, nbits):
    d = base.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _kps(pkg, x, y, octave, angle):
    k = np.zeros(len(x), pkg.KP_DTYPE)
    k["x"] = x; k["y"] = y; k["octave"] = octave; k["angle"] = angle
    k["size"] = F32(31.0) * SF[np.asarray(octave, np.int64)] if len(x) else 0
    k["response"] = 50.0; k["class_id"] = -1
    return k


def _scatter_pair(pkg, rng, n, levels, shuffle_queries=False, n_far=0):
    """A searched frame of n keypoints spread over the image on the given levels (ascending), and a query frame: the same points
    moved by up to 2 px with a few descriptor bits flipped, plus n_far queries in a corner the searched frame leaves empty."""
    octave = np.sort(rng.choice(levels, n)).astype(np.int32)
    x = rng.uniform(20, W - 20, n).astype(F32); y = rng.uniform(20, H - 160 if n_far else H - 20, n).astype(F32)
    ang = rng.uniform(0, 360, n).astype(F32)
    dt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kt = _kps(pkg, x, y, octave, ang)
    qx = (x + rng.uniform(-2, 2, n)).astype(F32); qy = (y + rng.uniform(-2, 2, n)).astype(F32)
    qang = ((ang + rng.normal(0, 4, n)) % 360).astype(F32)
    qang[rng.random(n) < 0.15] = F32(rng.uniform(0, 360))                    # some against the rotation consensus
    dq = np.stack([_flip(rng, dt[i], int(rng.integers(0, 40))) for i in range(n)]) if n else dt.copy()
    qoct = octave.copy()
    if n_far:
        qx = np.concatenate([qx, rng.uniform(30, W - 30, n_far).astype(F32)]); qy = np.concatenate([qy, rng.uniform(H - 90, H - 25, n_far).astype(F32)])
        qang = np.concatenate([qang, rng.uniform(0, 360, n_far).astype(F32)]); qoct = np.concatenate([qoct, np.zeros(n_far, np.int32)])
        dq = np.concatenate([dq, rng.integers(0, 256, (n_far, 32), dtype=np.uint8)])
    if shuffle_queries:
        p = rng.permutation(len(qx))
        qx, qy, qang, qoct, dq = qx[p], qy[p], qang[p], qoct[p], dq[p]
    return (kt, dt), (_kps(pkg, qx, qy, qoct, qang), dq)


def _blob_pair(pkg, rng):
    """A searched frame that holds only blobs of BLOBS[i] same-level keypoints with near-equal descriptors, and queries at each blob's
    centre on the blob's level, one level up and down (the blob passes the level test) and two levels up (every entry fails it)."""
    tx, ty, tang, td, qx, qy, qoct, qang, qd = [], [], [], [], [], [], [], [], []
    for i, nb in enumerate(BLOBS):
        cx, cy = 80 + 150 * (i % 5), 80 + 160 * (i // 5)
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        a0 = float(rng.uniform(0, 360))
        for _ in range(nb):
            tx.append(cx + rng.uniform(-3, 3)); ty.append(cy + rng.uniform(-3, 3)); tang.append((a0 + rng.normal(0, 3)) % 360)
            td.append(_flip(rng, base, int(rng.integers(8, 30))))
        for lvl in (BLOB_LEVEL, BLOB_LEVEL, BLOB_LEVEL - 1, BLOB_LEVEL + 1, BLOB_LEVEL + 2, BLOB_LEVEL):
            qx.append(cx + rng.uniform(-1, 1)); qy.append(cy + rng.uniform(-1, 1)); qoct.append(lvl); qang.append((a0 + rng.normal(0, 3)) % 360)
            qd.append(_flip(rng, base, int(rng.integers(3, 12))))
    kt = _kps(pkg, np.array(tx, F32), np.array(ty, F32), np.full(len(tx), BLOB_LEVEL, np.int32), np.array(tang, F32))
    kq = _kps(pkg, np.array(qx, F32), np.array(qy, F32), np.array(qoct, np.int32), np.array(qang, F32))
    return (kt, np.stack(td)), (kq, np.stack(qd))


def _empty(pkg):
    return _kps(pkg, np.zeros(0, F32), np.zeros(0, F32), np.zeros(0, np.int32), np.zeros(0, F32)), np.zeros((0, 32), np.uint8)


def _scene(pkg, name):
    """(th, check_ori, [(searched frame, query frame), ...]); a frame is (keypoints, descriptors)."""
    rng = np.random.default_rng({"small": 1, "mono": 2, "wide": 3}[name])
    if name == "small":       # th 7: windows of a few entries, many of them empty; an empty frame on either side; a single query
        one = _scatter_pair(pkg, rng, 1, [0])
        return 7.0, True, [_scatter_pair(pkg, rng, 403, [0, 1], n_far=30), (_empty(pkg), _scatter_pair(pkg, rng, 37, [0])[1]),
                           (_scatter_pair(pkg, rng, 250, [0, 1, 2])[0], _empty(pkg)), one]
    if name == "mono":        # th 15, 1000 features over eight levels: the benchmark's shape; shuffled queries; the blobs
        lv = [0] * 22 + [1] * 18 + [2] * 15 + [3] * 13 + [4] * 10 + [5] * 9 + [6] * 7 + [7] * 6
        return 15.0, True, [_scatter_pair(pkg, rng, 1003, lv), _scatter_pair(pkg, rng, 1001, lv, shuffle_queries=True, n_far=12), _blob_pair(pkg, rng),
                            _scatter_pair(pkg, rng, 2507, lv)]
    lv = [0, 1, 2, 3, 4, 5, 6, 7]   # th 45: windows of more than 64 entries (feed-back passes), shuffled levels, the blobs again
    return 45.0, False, [_scatter_pair(pkg, rng, 3001, lv), _scatter_pair(pkg, rng, 1501, lv, shuffle_queries=True), _blob_pair(pkg, rng)]


def _window_profile(OM, view, kq, q, th):
    """The window of query q over view: its grid entries in the order a pass visits them (columns, then cells, then the grid's own
    order) and, for each, whether GetFeaturesInArea (levels octave +- 1) returns it."""
    x, y, o = F32(kq["x"][q]), F32(kq["y"][q]), int(kq["octave"][q])
    r = F32(th) * SF[o]
    c0 = max(0, int(np.floor((x - view.min_x - r) * view.inv_w))); c1 = min(63, int(np.ceil((x - view.min_x + r) * view.inv_w)))
    r0 = max(0, int(np.floor((y - view.min_y - r) * view.inv_h))); r1 = min(47, int(np.ceil((y - view.min_y + r) * view.inv_h)))
    gs, gi = view.grid_start, view.grid_idx
    ent = [int(k) for ix in range(c0, c1 + 1) for k in gi[gs[ix * 48 + r0]:gs[ix * 48 + r1 + 1]]] if (c0 < 64 and c1 >= 0 and r0 < 48 and r1 >= 0) else []
    surv = set(int(k) for k in OM.features_in_area(view, x, y, r, o - 1, o + 1)) if view.n else set()
    assert surv <= set(ent), "grid layout misread"
    return ent, [k in surv for k in ent]


def _profiles(pkg, OM, scene):
    th, _, pairs = scene
    out = []
    for (kt, dt), (kq, _) in pairs:
        view = pkg.FrameView(kt, dt, W, H, backend=OM) if len(kt) else None
        rows = []
        for q in range(len(kq)):
            ent, ok = _window_profile(OM, view, kq, q, th) if view is not None else ([], [])
            rows.append((len(ent), sum(ok), [sum(ok[b:b + 64]) for b in range(0, len(ent), 64)]))
        out.append(rows)
    return out


def test_scenes_have_their_routes(pkg, oracle):
    """CPU only: the properties the scenes were built for, read from the oracle's grid and GetFeaturesInArea."""
    OM = oracle._oracle_matcher_class()()
    prof = {name: _profiles(pkg, OM, _scene(pkg, name)) for name in ("small", "mono", "wide")}
    allrows = [r for p in prof.values() for rows in p for r in rows]
    ent = np.array([r[0] for r in allrows]); surv = np.array([r[1] for r in allrows])
    for lo, hi in [(1, 8), (9, 16), (17, 32), (33, 48), (49, 64)]:               # one to four entries per lane in the first pass
        assert np.count_nonzero((ent >= lo) & (ent <= hi)) >= 10, (lo, hi)
    assert np.count_nonzero(ent == 0) >= 10                                      # empty windows (no pass at all)
    assert np.count_nonzero((ent > 0) & (surv == 0)) >= 10                       # entries, none of which passes
    assert np.count_nonzero(ent > 64) >= 100 and np.count_nonzero(ent > 128) >= 10   # one and more feed-back passes
    for n in (8, 9, 15, 16, 17):
        assert np.count_nonzero(surv == n) >= 2, n
    first = np.array([r[2][0] if r[2] else 0 for r in allrows]); later = np.array([max(r[2][1:]) if len(r[2]) > 1 else 0 for r in allrows])
    assert np.count_nonzero(first > 16) >= 10 and np.count_nonzero(first > 48) >= 2      # two and four rounds in the first pass
    assert np.count_nonzero(later > 16) >= 4                                              # and in a feed-back pass
    # the same routes per scene where the scene is what forces them
    small = np.array([r[0] for rows in prof["small"] for r in rows])
    assert small.max() <= 16 and np.count_nonzero(small == 0) >= 30
    wide = np.array([r[0] for r in prof["wide"][0]])
    assert np.count_nonzero(wide > 64) >= 1000
    for name in ("small", "mono", "wide"):
        _, _, pairs = _scene(pkg, name)
        counts = [len(f[0]) for pr in pairs for f in pr]
        assert any(c % 8 for c in counts) and any(c % 16 for c in counts) and any(c % 32 for c in counts)
    for name, p in (("mono", 1), ("wide", 1)):                                   # levels mix inside the 16-query workgroups
        kq = _scene(pkg, name)[2][p][1][0]
        o = kq["octave"][:len(kq) // 16 * 16].reshape(-1, 16)
        assert np.count_nonzero(o.max(1) - o.min(1) >= 3) >= 0.9 * len(o)
    lv = _scene(pkg, "mono")[2][0][1][0]["octave"]
    assert np.all(np.diff(lv) >= 0)                                             # and the level-ordered frames are level-ordered


@pytest.mark.gpu
@pytest.mark.parametrize("blocked_rate", [0.0, 0.5])
@pytest.mark.parametrize("name", ["small", "mono", "wide"])
def test_batched_search_matches_oracle_on_every_route(pkg, oracle, name, blocked_rate):
    """Every pair's match row and count from orbm_search_by_projection_batch_async equal the oracle's SearchByProjectionFrame, entry
    for entry.  blocked_rate 0.5: half of the searched slots are taken, so the claims walk down the eight-entry lists."""
    th, check_ori, pairs = _scene(pkg, name)
    OM = oracle._oracle_matcher_class()()
    L = pkg.lib()
    m = pkg.ORBmatcher(0.9)
    NP = len(pairs)
    NB = 2 * NP                                                                  # frames 0 .. NP-1 are searched, NP .. 2 NP-1 search
    frames = [pr[0] for pr in pairs] + [pr[1] for pr in pairs]
    cap = max(len(f[0]) for f in frames) + 5
    kps = np.zeros((NB, cap), pkg.KP_DTYPE); desc = np.zeros((NB, cap, 32), np.uint8)
    counts = np.array([len(f[0]) for f in frames], np.int32)
    for i, (k, d) in enumerate(frames):
        kps[i, :len(k)] = k; desc[i, :len(k)] = d
    rng = np.random.default_rng(17)
    blocked = (rng.random((NB, cap)) < blocked_rate).astype(np.uint8)
    obs = (rng.random((NB, cap)) < 0.9).astype(np.uint8)
    dk, dd, dc = pkg.DeviceBuffer(kps.nbytes), pkg.DeviceBuffer(desc.nbytes), pkg.DeviceBuffer(counts.nbytes)
    dk.upload(kps); dd.upload(desc); dc.upload(counts)
    dblk, dobs = pkg.DeviceBuffer(blocked.nbytes), pkg.DeviceBuffer(obs.nbytes)
    dblk.upload(blocked); dobs.upload(obs)
    gs, gi = pkg.DeviceBuffer(NB * 3073 * 4), pkg.DeviceBuffer(NB * cap * 4)
    inv_w, inv_h = float(F32(64) / F32(W)), float(F32(48) / F32(H))
    assert L.orbm_grid_build_batch_async(m.h, dk.ptr, dc.ptr, NB, cap, 0.0, 0.0, inv_w, inv_h, gs.ptr, gi.ptr) == 0
    dm, dn = pkg.DeviceBuffer(NP * cap * 4), pkg.DeviceBuffer(NP * 4)
    rc = L.orbm_search_by_projection_batch_async(m.h, dk.ptr, dd.ptr, dc.ptr, cap, gs.ptr, gi.ptr, 0.0, 0.0, inv_w, inv_h, NP, 0, NP, th,
                                                 SF.ctypes.data_as(C.c_void_p), 8, 0.0, 0.0, dblk.ptr, dobs.ptr, int(check_ori), dm.ptr, dn.ptr)
    assert rc == 0, L.orbm_last_error()
    m.sync()
    match = dm.download(np.int32, NP * cap).reshape(NP, cap); nm = dn.download(np.int32, NP)
    total = 0
    for p, ((kt, dt), (kq, dq)) in enumerate(pairs):
        nq, nt = len(kq), len(kt)
        if nt == 0 or nq == 0:
            assert nm[p] == 0 and np.all(match[p] == -1), p
            continue
        n_ref, m_ref = OM.SearchByProjectionFrame(pkg.FrameView(kt, dt, W, H, backend=OM), cur_blocked=blocked[p, :nt], scale_factors=SF,
                                                  valid=np.ones(nq, np.uint8), u=kq["x"], v=kq["y"], invzc=np.zeros(nq, np.float32),
                                                  octave=kq["octave"], angle=kq["angle"], qdesc=dq, mp_obs=obs[NP + p, :nq], th=th, check_ori=check_ori)
        assert nm[p] == n_ref, (p, nm[p], n_ref)
        assert np.array_equal(match[p, :nt], m_ref), (p, np.flatnonzero(match[p, :nt] != m_ref)[:10])
        assert np.all(match[p, nt:] == -1), p
        total += n_ref
    assert total > 100                                                           # the comparison is not one of empty rows
