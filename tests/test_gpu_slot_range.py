"""The batched searches at the top of their accepted slot range, and the grid builders over all of theirs.

Searches (M3, M4 and their two-camera forms, M5, M6, M13, M10): one call each on the pools of tests/slot_range_cases.py at cap = 65535
and cap = 32769, the searched grid taken from GridFrame.csr() and uploaded (no device grid build is involved), every row compared entry for entry with the second reading:
count, row up to n, -1 beyond n.  tests/test_slot_range_cpu.py proves that these cases reach slots 65534 / 32768, the last bitmap word,
word 1024, grid position 32768, the rescan path and contended slots >= 32768.  The row-mapped searches also run 65535 pairs once.

Grid builders: orbm_grid_build and orbm_grid_build_batch_async against GridFrame.csr() directly (grid_start and grid_idx[:placed]) at
n / cap of 1, 8192, 8193, 20000, 32768, 32769, 50000 and 65535 -- every form of the build and both sides of each threshold between
them -- and orbm_frame_create, whose grid stays on the device, through a resident search over it."""
import numpy as np
import pytest

import second_reading as sr
import slot_range_cases as sc
import test_gpu_fuse_batch as fu
import test_gpu_local_points_batch as lp
import test_gpu_motion_model_batch as mm
import test_gpu_reloc_batch as rl
import test_gpu_sim3_projection_batch as s3
import test_gpu_triangulation_batch as tr

pytestmark = pytest.mark.gpu

CAPS = [sc.CAP_HALF, sc.CAP_TOP]                                               # the largest shape last


class DevPool:
    """A HostPool on the device with the grid of GridFrame.csr(): the fields rl.Call / s3.Call read from an rl.Pool."""

    def __init__(self, pkg, hp):
        self.pkg, self.L, self.hp = pkg, pkg.lib(), hp
        self.kps, self.desc, self.counts = hp.kps.view(pkg.KP_DTYPE), hp.desc, hp.counts
        self.R, self.cap, self.sf, self.nlev = hp.R, hp.cap, hp.sf, hp.nlev
        self.w, self.h, self.inv_w, self.inv_h, self.bounds = hp.w, hp.h, hp.inv_w, hp.inv_h, hp.bounds
        self.m = pkg.ORBmatcher(0.9)
        self.dk, self.dd, self.dc = rl._dev(pkg, self.kps), rl._dev(pkg, self.desc), rl._dev(pkg, self.counts)
        gs, gi, _ = hp.csr()
        self.gs, self.gi = rl._dev(pkg, gs), rl._dev(pkg, gi)
        self.r = dict(kps=self.dk.ptr, desc=self.dd.ptr, counts=self.dc.ptr)


_POOLS = {}


def _pool(pkg, cap, nlev=8):
    if (cap, nlev) not in _POOLS:
        _POOLS.clear()                                                        # one pool on the device at a time
        _POOLS[(cap, nlev)] = DevPool(pkg, sc.pool(cap, nlev))
    return _POOLS[(cap, nlev)]


def _same_pair(row_l, row_r, count, want, nl, nr, what):
    """A two-camera search: count, the left row and the right row up to their counts, -1 beyond."""
    assert int(count) == int(want[0]), (what, int(count), int(want[0]))
    assert np.array_equal(row_l[:nl], want[1]), (what, "left", np.flatnonzero(row_l[:nl] != want[1])[:8])
    assert np.array_equal(row_r[:nr], want[2]), (what, "right", np.flatnonzero(row_r[:nr] != want[2])[:8])
    assert np.all(row_l[nl:] == -1) and np.all(row_r[nr:] == -1), (what, "padding")


def _same_row(row, count, want, n, what):
    if want is None:
        assert int(count) == 0 and np.all(row == -1), what
        return
    assert int(count) == int(want[0]), (what, int(count), int(want[0]))
    assert np.array_equal(row[:n], want[1][:n]), (what, np.flatnonzero(row[:n] != want[1][:n])[:8])
    assert np.all(row[n:] == -1), what


# ---- searches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_m3_points(pkg, cap):
    case = sc.m3_case(cap)
    P = _pool(pkg, cap)
    Q = [dict(in_view=q["valid"], px=q["u"], py=q["v"], pxr=np.zeros(sc.NQ, np.float32), view_cos=q["view_cos"], level=q["level"], qdesc=q["desc"],
              mp_obs=q["mp_obs"]) for q in case["Q"]]
    R_ = lp._Rows(pkg, P.R, sc.NQ + 3); R_.upload(Q)
    dm = pkg.DeviceBuffer(P.R * P.cap * 4); dn = pkg.DeviceBuffer(P.R * 4)
    rc = lp._call(P.L, P.m, P.r, P.cap, P.gs, P.gi, 0, R_, P.sf, sc.M3_TH, sc.M3_NNRATIO, dm, dn, blocked=rl._dev(pkg, case["blocked"]),
                  inv_w=P.inv_w, inv_h=P.inv_h, nlev=P.nlev)
    assert rc == 0, P.L.orbm_last_error()
    P.m.sync()
    match = dm.download(np.int32, P.R * P.cap).reshape(P.R, P.cap); nm = dn.download(np.int32, P.R)
    for f, (r, _) in enumerate(case["frames"]):
        _same_row(match[f], nm[f], case["want"][f], P.hp.n(r), "M3 cap %d row %d" % (cap, r))


@pytest.mark.parametrize("cap", CAPS)
def test_m4_frame(pkg, cap):
    case = sc.m4_case(cap)
    P = _pool(pkg, cap)
    Q = [dict(valid=q["valid"], u=q["u"], v=q["v"], invzc=q["invzc"], octave=q["level"], angle=q["angle"], qdesc=q["desc"], mp_obs=q["mp_obs"])
         for q in case["Q"]]
    R_ = mm._Rows(pkg, P.R, sc.NQ + 3); R_.upload(Q)
    dm = pkg.DeviceBuffer(P.R * P.cap * 4); dn = pkg.DeviceBuffer(P.R * 4)
    rc = mm._call(P.L, P.m, P.r, P.cap, P.gs, P.gi, 0, R_, P.sf, sc.M4_TH, dm, dn, blocked=rl._dev(pkg, case["blocked"]), check_ori=True,
                  inv_w=P.inv_w, inv_h=P.inv_h, nlev=P.nlev)
    assert rc == 0, P.L.orbm_last_error()
    P.m.sync()
    match = dm.download(np.int32, P.R * P.cap).reshape(P.R, P.cap); nm = dn.download(np.int32, P.R)
    for f, (r, _) in enumerate(case["frames"]):
        _same_row(match[f], nm[f], case["want"][f], P.hp.n(r), "M4 cap %d row %d" % (cap, r))


@pytest.mark.parametrize("cap,nlev", [(sc.CAP_HALF, 8), (sc.CAP_TOP, 8), (sc.CAP_TOP, 12)])
def test_m5_kf(pkg, cap, nlev):
    case = sc.m5_case(cap, nlev)
    P = _pool(pkg, cap, nlev)
    match, nm = rl.Call(P, case["pairs"]).run(sc.M5_TH, sc.M5_ORB_DIST, True)
    for i, p in enumerate(case["pairs"]):
        _same_row(match[i], nm[i], case["want"][i], P.hp.n(p["row"]), "M5 cap %d pair %d" % (cap, i))


@pytest.mark.parametrize("cap", CAPS)
def test_m6_sim3(pkg, cap):
    case = sc.m6_case(cap)
    P = _pool(pkg, cap)
    match, nm = s3.Call(P, case["pairs"]).run(sc.M6_TH, sc.M6_RATIO, case["form"])
    for i, p in enumerate(case["pairs"]):
        _same_row(match[i], nm[i], case["want"][i], P.hp.n(p["row"]), "M6 cap %d pair %d" % (cap, i))


def _fuse(P, pairs, isg, th, chi2):
    """orbm_fuse_batch_async on pool P (no uright) for pairs of equal query counts: best [npairs][nq] and nfused."""
    st = lambda key: np.stack([p[key] for p in pairs])
    nq = len(pairs[0]["valid"])
    c = fu.Call(P, [p["row"] for p in pairs], st("tcw"), st("ow"), np.full(len(pairs), nq, np.int32), st("valid"), st("pw"), st("normal"), st("mn"),
                st("mx"), st("qdesc"), False)
    rc = P.L.orbm_fuse_batch_async(P.m.h, c.P, P.R, P.cap, P.dk.ptr, P.dd.ptr, None, P.gs.ptr, P.gi.ptr, 0.0, 0.0, P.inv_w, P.inv_h,
                                   c.kf_row.ptr, c.tcw.ptr, c.ow.ptr, c.nq.ptr, c.qs, c.valid.ptr, c.pw.ptr, c.normal.ptr, c.mn.ptr, c.mx.ptr,
                                   c.qdesc.ptr, 0, rl._vp(rl.KCAM), rl._vp(P.bounds), float(sc.BF), float(th), int(chi2), rl._vp(P.sf),
                                   rl._vp(isg), float(rl.LOG_SF), P.nlev, c.best.ptr, c.nf.ptr, c.lvl.ptr)
    assert rc == 0, P.L.orbm_last_error()
    assert P.L.orbm_sync(P.m.h) == 0
    best, nf, _ = c.download()
    return best, nf


@pytest.mark.parametrize("cap", CAPS)
def test_m13_fuse(pkg, cap):
    case = sc.m13_case(cap)
    P = _pool(pkg, cap)
    best, nf = _fuse(P, case["pairs"], case["isg"], sc.M13_TH, 1)
    for i, p in enumerate(case["pairs"]):
        want = case["want"][i]
        if want is None:
            assert nf[i] == 0 and np.all(best[i] == -1)
        else:
            assert int(nf[i]) == want[0] and np.array_equal(best[i], want[1]), ("M13 cap %d pair %d" % (cap, i), np.flatnonzero(best[i] != want[1])[:8])


@pytest.mark.parametrize("cap", CAPS)
def test_m4_frame_fisheye(pkg, cap):
    case = sc.m4_fisheye_case(cap)
    P = _pool(pkg, cap)
    first_l, first_r, npairs = case["layout"]
    qs = 2 * sc.NQ + 3
    up = {}
    for key, dt in (("valid", np.uint8), ("u", np.float32), ("v", np.float32), ("ur", np.float32), ("vr", np.float32), ("octave", np.int32),
                    ("angle", np.float32), ("mp_obs", np.uint8)):
        a = np.full((npairs, qs), 77, dt)                                     # padding: garbage nobody may read
        a[:, :2 * sc.NQ] = np.stack([q[key] for q in case["Q"]])
        up[key] = rl._dev(pkg, a)
    d = np.full((npairs, qs, 32), 0xA5, np.uint8); d[:, :2 * sc.NQ] = np.stack([q["qdesc"] for q in case["Q"]])
    nq = rl._dev(pkg, np.full(npairs, 2 * sc.NQ, np.int32)); dd = rl._dev(pkg, d); dirs = rl._dev(pkg, np.zeros(max(npairs, 4), np.uint8))
    bl, br = rl._dev(pkg, case["blocked_l"]), rl._dev(pkg, case["blocked_r"])
    ml = pkg.DeviceBuffer(npairs * cap * 4); mr = pkg.DeviceBuffer(npairs * cap * 4); nm = pkg.DeviceBuffer(npairs * 4); rt = pkg.DeviceBuffer(max(npairs, 4))
    rc = P.L.orbm_search_by_projection_frame_fisheye_batch_async(
        P.m.h, P.dk.ptr, P.dd.ptr, P.dc.ptr, cap, P.gs.ptr, P.gi.ptr, 0.0, 0.0, P.inv_w, P.inv_h, first_l, first_r, npairs, bl.ptr, br.ptr, dirs.ptr,
        nq.ptr, qs, up["valid"].ptr, up["u"].ptr, up["v"].ptr, up["ur"].ptr, up["vr"].ptr, up["octave"].ptr, up["angle"].ptr, dd.ptr, up["mp_obs"].ptr,
        float(sc.M4_TH), 0, rl._vp(P.sf), P.nlev, 1, ml.ptr, mr.ptr, nm.ptr, rt.ptr)
    assert rc == 0, P.L.orbm_last_error()
    P.m.sync()
    gl = ml.download(np.int32, npairs * cap).reshape(npairs, cap); gr = mr.download(np.int32, npairs * cap).reshape(npairs, cap)
    gn = nm.download(np.int32, npairs)
    for p in range(npairs):
        _same_pair(gl[p], gr[p], gn[p], case["want"][p], P.hp.n(first_l + p), P.hp.n(first_r + p), "M4 fisheye cap %d pair %d" % (cap, p))


@pytest.mark.parametrize("cap", CAPS)
def test_m3_points_fisheye(pkg, cap):
    case = sc.m3_fisheye_case(cap)
    P = _pool(pkg, cap)
    first_l, first_r, npairs = case["layout"]
    qs = 2 * sc.NQ + 3
    up = {}
    for key, dt in (("in_view", np.uint8), ("px", np.float32), ("py", np.float32), ("view_cos", np.float32), ("level", np.int32), ("in_view_r", np.uint8),
                    ("pxr", np.float32), ("pyr", np.float32), ("view_cos_r", np.float32), ("level_r", np.int32), ("mp_obs", np.uint8)):
        a = np.zeros((npairs, qs), dt)
        a[:, :2 * sc.NQ] = np.stack([q[key] for q in case["Q"]])
        up[key] = rl._dev(pkg, a)
    d = np.full((npairs, qs, 32), 0xA5, np.uint8); d[:, :2 * sc.NQ] = np.stack([q["qdesc"] for q in case["Q"]])
    nq = rl._dev(pkg, np.full(npairs, 2 * sc.NQ, np.int32)); dd = rl._dev(pkg, d)
    bl, br = rl._dev(pkg, case["blocked_l"]), rl._dev(pkg, case["blocked_r"])
    ml = pkg.DeviceBuffer(npairs * cap * 4); mr = pkg.DeviceBuffer(npairs * cap * 4); nm = pkg.DeviceBuffer(npairs * 4)
    rc = P.L.orbm_search_by_projection_points_fisheye_batch_async(
        P.m.h, P.dk.ptr, P.dd.ptr, P.dc.ptr, cap, P.gs.ptr, P.gi.ptr, 0.0, 0.0, P.inv_w, P.inv_h, first_l, first_r, npairs, bl.ptr, br.ptr, None, None,
        nq.ptr, qs, up["in_view"].ptr, up["px"].ptr, up["py"].ptr, up["view_cos"].ptr, up["level"].ptr, up["in_view_r"].ptr, up["pxr"].ptr,
        up["pyr"].ptr, up["view_cos_r"].ptr, up["level_r"].ptr, None, 0.0, dd.ptr, up["mp_obs"].ptr, 0, float(sc.M3_TH), float(sc.M3_NNRATIO),
        rl._vp(P.sf), P.nlev, ml.ptr, mr.ptr, nm.ptr)
    assert rc == 0, P.L.orbm_last_error()
    P.m.sync()
    gl = ml.download(np.int32, npairs * cap).reshape(npairs, cap); gr = mr.download(np.int32, npairs * cap).reshape(npairs, cap)
    gn = nm.download(np.int32, npairs)
    for p in range(npairs):
        _same_pair(gl[p], gr[p], gn[p], case["want"][p], P.hp.n(first_l + p), P.hp.n(first_r + p), "M3 fisheye cap %d pair %d" % (cap, p))


@pytest.mark.parametrize("cap", CAPS)
def test_m10_triangulation(pkg, cap):
    """cap1 = cap2 = cap, every slot a keypoint; the pairs: the two full rows, and each against the other pool's empty row."""
    c = sc.m10_case(cap)
    mt = pkg.ORBmatcher(0.6)
    none = (_kp(pkg, c["k1"][:0]), c["d1"][:0])
    A = tr.Pool(pkg, [(_kp(pkg, c["k1"]), c["d1"]), none], cap, 8, mp=[c["mp1"], c["mp1"][:0]])
    B = tr.Pool(pkg, [(_kp(pkg, c["k2"]), c["d2"]), none], cap, 8, mp=[c["mp2"], c["mp2"][:0]])
    A.node[0] = c["node"]; B.node[0] = c["node"]
    A.upload(); B.upload()
    got, nm = tr.run(pkg, mt, A, B, [0, 0, 1], [0, 1, 0], np.stack([sc.M10_F12] * 3), np.array([sc.M10_EP] * 3, np.float32), c["sf"], c["sigma2"],
                     check_ori=1)
    _same_row(got[0], nm[0], c["want"], cap, "M10 cap %d" % cap)
    assert nm[1] == 0 and nm[2] == 0 and np.all(got[1:] == -1)


# ---- npairs = 65535 -------------------------------------------------------------------------------------------------------------------
def _tiny(pkg):
    hp, kinds = sc.tiny_kinds()
    P = DevPool(pkg, hp)
    return hp, kinds, P, [kinds[i % 4] for i in range(sc.NPAIRS_TOP)]


def _each_kind(match, nm, wants, n_of, what):
    for j, want in enumerate(wants):
        rows, cnt = match[j::4], nm[j::4]
        assert np.all(rows == rows[0]) and np.all(cnt == cnt[0]), (what, j, np.flatnonzero((rows != rows[0]).any(1))[:4] * 4 + j)
        _same_row(rows[0], cnt[0], want, n_of(j), "%s kind %d" % (what, j))


def test_m5_65535_pairs(pkg):
    hp, kinds, P, pairs = _tiny(pkg)
    match, nm = rl.Call(P, pairs).run(sc.M5_TH, sc.M5_ORB_DIST, True)
    wants = []
    for p in kinds:
        ok, u, v, lvl = sc.proj_m5(hp, p)
        n = hp.n(p["row"])
        wants.append(sr.search_by_projection_kf(hp.grid(p["row"]), p["blocked"][:n], hp.sf, ok, u, v, np.maximum(lvl, 0), p["angle"], p["qdesc"],
                                                sc.M5_TH, sc.M5_ORB_DIST, True) if n else None)
    assert sum(w[0] for w in wants if w) > 10
    _each_kind(match, nm, wants, lambda j: hp.n(kinds[j]["row"]), "M5")


def test_m6_65535_pairs(pkg):
    hp, kinds, P, pairs = _tiny(pkg)
    match, nm = s3.Call(P, pairs).run(sc.M6_TH, sc.M6_RATIO, 0)
    wants = []
    for p in kinds:
        ok, u, v, lvl = sc.proj_m6(hp, p, 0)
        n = hp.n(p["row"])
        wants.append(sr.search_by_projection_sim3(hp.grid(p["row"]), p["matched"][:n], hp.sf, ok, u, v, np.maximum(lvl, 0), p["qdesc"], sc.M6_TH,
                                                  sc.M6_RATIO) if n else None)
    assert sum(w[0] for w in wants if w) > 10
    _each_kind(match, nm, wants, lambda j: hp.n(kinds[j]["row"]), "M6")


def test_m13_65535_pairs(pkg):
    hp, kinds, P, pairs = _tiny(pkg)
    isg = (np.float32(1) / (hp.sf * hp.sf)).astype(np.float32)
    best, nf = _fuse(P, pairs, isg, sc.M13_TH, 1)
    total = 0
    for j, p in enumerate(kinds):
        ok, u, v, ur, lvl = sc.proj_m13(hp, p)
        rows, cnt = best[j::4], nf[j::4]
        assert np.all(rows == rows[0]) and np.all(cnt == cnt[0]), j
        if hp.n(p["row"]) == 0:
            assert cnt[0] == 0 and np.all(rows[0] == -1)
            continue
        want = sr.fuse(hp.grid(p["row"]), hp.sf, isg, ok, u, v, ur, np.maximum(lvl, 0), p["qdesc"], sc.M13_TH, True)
        assert int(cnt[0]) == want[0] and np.array_equal(rows[0], want[1]), j
        total += want[0]
    assert total > 10


# ---- grid builders --------------------------------------------------------------------------------------------------------------------
def _kp(pkg, k):
    return np.ascontiguousarray(k).view(pkg.KP_DTYPE)


def _check_single(pkg, m, k):
    fv = pkg.FrameView(_kp(pkg, k), np.zeros((len(k), 32), np.uint8), sc.W, sc.H, backend=m)
    s, i, _ = sc.grid_want(k)
    assert fv.placed == len(i), (fv.placed, len(i))
    assert np.array_equal(fv.grid_start, s), np.flatnonzero(fv.grid_start != s)[:8]
    assert np.array_equal(fv.grid_idx[:len(i)], i), np.flatnonzero(fv.grid_idx[:len(i)] != i)[:8]


@pytest.mark.parametrize("n", sc.GRID_SIZES)
def test_grid_build(pkg, n):
    _check_single(pkg, pkg.ORBmatcher(0.9), sc.grid_points(n))


@pytest.mark.parametrize("n", [8192, 20000, 65535])
def test_grid_build_one_crowded_cell(pkg, n):
    """2048 keypoints of the highest slots in one cell, the rest sparse: the counting forms' per-cell order restore at its longest list."""
    _check_single(pkg, pkg.ORBmatcher(0.9), sc.grid_points(n, crowded=True))


@pytest.mark.parametrize("n", [8192, 32769, 50000, 65535])
def test_grid_build_several_long_cells(pkg, n):
    """Cells of exactly 64, 65, 100 and 700 keypoints: above 32768 keypoints the 64 stay with one lane and the three others go, one after
    the other, through the workgroup-wide sort."""
    _check_single(pkg, pkg.ORBmatcher(0.9), sc.grid_points(n, crowded="several"))


@pytest.mark.parametrize("cap", sc.GRID_SIZES)
def test_grid_build_batch(pkg, cap):
    """Rows with count == cap, count < cap, 0, count > cap and (from 4096 slots on) a row with one crowded cell and a row with cells of
    64, 65, 100 and 700 keypoints; the slots past a count hold keypoints that must not be placed."""
    L = pkg.lib(); m = pkg.ORBmatcher(0.9)
    counts = [cap, cap // 2, 0, cap + 1000] + ([cap, cap] if cap >= 4096 else [])
    R = len(counts)
    kps = np.zeros((R, cap), sc.KP_DTYPE)
    for r in range(R):
        kps[r] = np.roll(sc.grid_points(65535), -7 * r)[:cap] if r < 4 else sc.grid_points(cap, crowded=(True, "several")[r - 4])
    dk, dc = rl._dev(pkg, _kp(pkg, kps)), rl._dev(pkg, np.asarray(counts, np.int32))
    gs = pkg.DeviceBuffer(R * 3073 * 4).upload(np.full(R * 3073, -9, np.int32)); gi = pkg.DeviceBuffer(R * cap * 4).upload(np.full(R * cap, -9, np.int32))
    assert L.orbm_grid_build_batch_async(m.h, dk.ptr, dc.ptr, R, cap, 0.0, 0.0, sc.INV_W, sc.INV_H, gs.ptr, gi.ptr) == 0, L.orbm_last_error()
    m.sync()
    got_s = gs.download(np.int32, R * 3073).reshape(R, 3073); got_i = gi.download(np.int32, R * cap).reshape(R, cap)
    for r in range(R):
        s, i, _ = sc.grid_want(kps[r, :min(counts[r], cap)])
        assert np.array_equal(got_s[r], s), (r, np.flatnonzero(got_s[r] != s)[:8])
        assert np.array_equal(got_i[r, :len(i)], i), (r, np.flatnonzero(got_i[r, :len(i)] != i)[:8])


@pytest.mark.parametrize("n,crowded", [(n, False) for n in sc.GRID_SIZES] + [(8192, True), (65535, True), (65535, "several")])
def test_frame_create_grid(pkg, n, crowded):
    """orbm_frame_create keeps its grid on the device and nothing reads it back: a resident M4 search over it equals the second reading's
    search over GridFrame's grid.  The keypoints are those of the other builders' tests (negative cells, column 64 / row 48, half-way
    cells, crowded cells); 2000 queries sit on them all over the frame, and with crowded cells a quarter of the queries sit there, where
    the descriptors are nearly equal and the grid's visiting order decides between equal distances."""
    rng = np.random.default_rng(n)
    m = pkg.ORBmatcher(0.9)
    k = sc.grid_points(n, crowded); d = sc.grid_descriptors(k, crowded)
    sf = sc.pool(sc.CAP_HALF).sf
    rf = pkg.ResidentFrame(m, view=pkg.FrameView(_kp(pkg, k), d, sc.W, sc.H))
    NQ = 2000
    src = rng.integers(0, n, NQ)
    if crowded:
        cells = [c for c, _ in sc.LONG_CELLS] if crowded == "several" else [(50, 40)]
        inside = np.flatnonzero(np.any([(np.abs(k["x"] - 30.0 * cx) < 15.01) & (np.abs(k["y"] - 22.5 * cy) < 11.25) for cx, cy in cells], axis=0))
        src[:NQ // 4] = rng.choice(inside, NQ // 4)
    u = (k["x"][src] + rng.normal(0, 1, NQ)).astype(np.float32); v = (k["y"][src] + rng.normal(0, 1, NQ)).astype(np.float32)
    a = dict(cur_blocked=(rng.random(n) < 0.2).astype(np.uint8), scale_factors=sf, valid=np.ones(NQ, np.uint8), u=u, v=v,
             invzc=np.zeros(NQ, np.float32), octave=k["octave"][src].astype(np.int32), angle=k["angle"][src],
             qdesc=rl.flip(rng, d[src], 2 if crowded else 30),
             mp_obs=np.ones(NQ, np.uint8), th=7.0, check_ori=True)
    got = m.SearchByProjectionFrameResident(rf, **a)
    g = sr.GridFrame(k, d, 0.0, 0.0, sc.INV_W, sc.INV_H)
    want = sr.search_by_projection_frame(g, **a)
    rf.close()
    # the floor: of min(n, 2000) distinct keypoints asked for about 4 in 5 are placed and 4 in 5 of those free; a quarter is well below that
    assert want[0] + int((want[1] == sr.PRUNED).sum()) >= (min(n, NQ) // 4 if n > 1 else g.placed)
    if crowded:
        assert int(np.isin(np.flatnonzero(want[1] >= 0), inside).sum()) > 50                 # matches inside the crowded cells ...
        assert n < sc.CAP_TOP or want[2]["tie_kept_first_not_lowest_index"] > 0              # ... some won by visiting order against a lower index
    assert got[0] == want[0] and np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:8]


def test_grid_builders_refuse_above_65535(pkg):
    """One keypoint more than the header's limit: ORBM_E_CAPACITY from the two single-frame builders, ORBM_E_INVALID from the batched one."""
    m = pkg.ORBmatcher(0.9); L = pkg.lib()
    k = np.zeros(65536, pkg.KP_DTYPE); d = np.zeros((65536, 32), np.uint8)
    with pytest.raises(pkg.OrbError, match="code -3"):
        pkg.FrameView(k, d, sc.W, sc.H, backend=m)
    assert b"65535" in L.orbm_last_error()
    with pytest.raises(pkg.OrbError, match="code -3"):
        pkg.ResidentFrame(m, view=pkg.FrameView(k, d, sc.W, sc.H))
    assert b"a resident frame holds at most 65535" in L.orbm_last_error()
    dk, dc = rl._dev(pkg, k[:4]), rl._dev(pkg, np.zeros(1, np.int32))
    gs = pkg.DeviceBuffer(3073 * 4).upload(np.full(3073, -9, np.int32)); gi = pkg.DeviceBuffer(16)
    assert L.orbm_grid_build_batch_async(m.h, dk.ptr, dc.ptr, 1, 65536, 0.0, 0.0, sc.INV_W, sc.INV_H, gs.ptr, gi.ptr) == -2
    m.sync()
    assert np.all(gs.download(np.int32, 3073) == -9)                          # nothing was enqueued
