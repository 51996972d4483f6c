"""Batched two-camera SearchByProjection(Frame, vector<MapPoint*>) -- M3 with Nleft != -1, Tracking::SearchLocalPoints on a fisheye rig --
on the device (orbm_search_by_projection_points_fisheye_batch_async).  For every case of tests/points_fisheye_cases.py and every pair
the two match rows (ORBM_NO_MATCH padding included) and the count equal, entry for entry, the second reading of
tests/second_reading_points_fisheye.py and, where the host form is defined, the product's host entry point
(ORBmatcher.SearchByProjectionPointsFisheye); tests/test_second_reading_points_fisheye_cpu.py ties both to the oracle."""
import copy
import ctypes as C

import numpy as np
import pytest

import fisheye_cases as fc
import points_fisheye_cases as pc
from test_second_reading_points_fisheye_cpu import NAMES, second_reading_pair, single_pair

pytestmark = pytest.mark.gpu

ROW_KEYS = tuple(k for k, _ in pc.FIELDS) + ("qdesc",)
_want = {}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def reading(P, case, p, key=None):
    """The second reading of one pair, computed once per (case, pair) for the tests that share it."""
    if key is None:
        return second_reading_pair(P, case, p)
    if (key, p) not in _want:
        _want[(key, p)] = second_reading_pair(P, case, p)
    return _want[(key, p)]


class _Rows:
    """The per-pair device arrays of one call for pairs [p0, p0 + npairs) of a case; blocked and partner rows re-laid to the pool's cap."""

    def __init__(self, pkg, case, cap, p0=0, npairs=pc.NPAIRS):
        self.npairs, self.qs, self.cap, self.shared = npairs, case.q_stride, cap, int(case.q_shared)
        sel = slice(p0, p0 + npairs)
        h = case.rows()
        pick = lambda k: h[k] if case.q_shared and k in ("qdesc", "mp_obs") else h[k][sel]
        self.buf = {k: pkg.DeviceBuffer(max(pick(k).nbytes, 4)).upload(np.ascontiguousarray(pick(k))) for k in ROW_KEYS + ("nq",)}
        self.bl = pkg.DeviceBuffer(npairs * cap).upload(self.relaid(case.blocked_l[sel], 0))
        self.br = pkg.DeviceBuffer(npairs * cap).upload(self.relaid(case.blocked_r[sel], 0))
        self.l2r = pkg.DeviceBuffer(npairs * cap * 4).upload(self.relaid(case.l2r[sel], -1))
        self.r2l = pkg.DeviceBuffer(npairs * cap * 4).upload(self.relaid(case.r2l[sel], -1))
        self.ml = pkg.DeviceBuffer(npairs * cap * 4); self.mr = pkg.DeviceBuffer(npairs * cap * 4)
        self.nm = pkg.DeviceBuffer(npairs * 4)

    def relaid(self, b, fill):
        out = np.full((len(b), self.cap), fill, b.dtype)
        w = min(self.cap, b.shape[1])
        out[:, :w] = b[:, :w]
        return out

    def poison(self):
        n = self.npairs * self.cap
        self.ml.upload(np.full(n, -7, np.int32)); self.mr.upload(np.full(n, -7, np.int32))
        self.nm.upload(np.full(self.npairs, -7, np.int32))

    def results(self):
        n = self.npairs * self.cap
        return (self.ml.download(np.int32, n).reshape(self.npairs, self.cap), self.mr.download(np.int32, n).reshape(self.npairs, self.cap),
                self.nm.download(np.int32, self.npairs))


def _call(L, m, r, cap, gs, gi, rows, case, first_l=pc.FIRST_L, first_r=pc.FIRST_R, blocked=True, partners=True, depth=None):
    b = rows.buf
    use_depth = (case.th_far is not None) if depth is None else depth
    return L.orbm_search_by_projection_points_fisheye_batch_async(
        m.h, r["kps"], r["desc"], r["counts"], cap, gs.ptr, gi.ptr, 0.0, 0.0, pc.INV_W, pc.INV_H, first_l, first_r, rows.npairs,
        rows.bl.ptr if blocked else None, rows.br.ptr if blocked else None, rows.l2r.ptr if partners else None, rows.r2l.ptr if partners else None,
        b["nq"].ptr, rows.qs, b["in_view"].ptr, b["px"].ptr, b["py"].ptr, b["view_cos"].ptr, b["level"].ptr,
        b["in_view_r"].ptr, b["pxr"].ptr, b["pyr"].ptr, b["view_cos_r"].ptr, b["level_r"].ptr,
        b["depth"].ptr if use_depth else None, float(case.th_far if case.th_far is not None else 0.0), b["qdesc"].ptr, b["mp_obs"].ptr, rows.shared,
        float(case.th), float(case.nnratio), _vp(pc.SF), pc.NLEV, rows.ml.ptr, rows.mr.ptr, rows.nm.ptr)


def _same(row_l, row_r, n_dev, want, nl, nr, what):
    n, ml, mr = want[0], want[1], want[2]
    assert int(n_dev) == int(n), (what, int(n_dev), int(n))
    assert np.array_equal(row_l[:nl], ml), (what, "left", np.flatnonzero(row_l[:nl] != ml)[:8])
    assert np.array_equal(row_r[:nr], mr), (what, "right", np.flatnonzero(row_r[:nr] != mr)[:8])
    assert np.all(row_l[nl:] == -1) and np.all(row_r[nr:] == -1), (what, "padding")


def _on_device(pkg, m, L, P):
    cap = P["cap"]
    dk = pkg.DeviceBuffer(P["kps"].nbytes).upload(P["kps"]); dd = pkg.DeviceBuffer(P["desc"].nbytes).upload(P["desc"])
    dc = pkg.DeviceBuffer(P["counts"].nbytes).upload(P["counts"])
    r = dict(kps=dk.ptr, desc=dd.ptr, counts=dc.ptr)
    gs = pkg.DeviceBuffer(pc.NROWS * 3073 * 4); gi = pkg.DeviceBuffer(pc.NROWS * cap * 4)
    assert L.orbm_grid_build_batch_async(m.h, r["kps"], r["counts"], pc.NROWS, cap, 0.0, 0.0, pc.INV_W, pc.INV_H, gs.ptr, gi.ptr) == 0, L.orbm_last_error()
    return dict(P=P, r=r, cap=cap, gs=gs, gi=gi, keep=(dk, dd, dc))


@pytest.fixture(scope="module")
def dev(pkg, oracle, synth):
    """Both pools on the device, each with its grid."""
    m = pkg.ORBmatcher(0.9); L = pkg.lib()
    pools = {name: _on_device(pkg, m, L, P) for name, P in pc.pools(oracle, synth).items()}
    m.sync()
    return dict(pools=pools, CASES=pc.cases(oracle, synth), m=m, L=L)


@pytest.mark.parametrize("name", NAMES)
def test_parity(pkg, dev, name):
    case = dev["CASES"][name]
    D = dev["pools"][case.pool_name]
    P, cap = D["P"], D["cap"]
    rows = _Rows(pkg, case, cap)
    rows.poison()
    assert _call(dev["L"], dev["m"], D["r"], cap, D["gs"], D["gi"], rows, case) == 0, dev["L"].orbm_last_error()
    dev["m"].sync()
    ml, mr, nm = rows.results()
    for p in range(pc.NPAIRS):
        nl, nr = int(P["counts"][pc.FIRST_L + p]), int(P["counts"][pc.FIRST_R + p])
        _same(ml[p], mr[p], nm[p], reading(P, case, p, name), nl, nr, (name, p, "second reading"))
        if case.host_defined:
            _same(ml[p], mr[p], nm[p], single_pair(pkg, dev["m"], P, case, p), nl, nr, (name, p, "host entry point"))
    if case.pool_name == "scene":
        assert nm[0] > 100 and nm[1] > 100 and nm[2] >= 4 and nm[3] >= 4       # an empty row on either side does not empty the pair
    elif name not in ("ratio_reject_skips_right", "both_rows_empty", "nq0"):
        assert nm[case.rule_pair] >= 1 and nm.sum() == nm[case.rule_pair]


def test_null_optionals(pkg, dev):
    """blocked_l / blocked_r, l2r / r2l and depth NULL: none blocked, no partners, bFarPoints off."""
    case = dev["CASES"]["scene_th3_far"]
    D = dev["pools"]["scene"]
    P, cap = D["P"], D["cap"]
    bare = copy.copy(case)
    bare.blocked_l, bare.blocked_r = np.zeros_like(case.blocked_l), np.zeros_like(case.blocked_r)
    bare.l2r, bare.r2l = np.full_like(case.l2r, -1), np.full_like(case.r2l, -1)
    bare.th_far = None                                                         # (the far points' own fields are NaN: they stay out of view)
    bare.Q = []
    for q in case.Q:
        q = {k: v.copy() for k, v in q.items()}
        far = q["depth"] > np.float32(case.th_far)
        q["in_view"][far] = 0; q["in_view_r"][far] = 0
        bare.Q.append(q)
    rows = _Rows(pkg, bare, cap)
    rows.poison()
    assert _call(dev["L"], dev["m"], D["r"], cap, D["gs"], D["gi"], rows, bare, blocked=False, partners=False, depth=False) == 0, dev["L"].orbm_last_error()
    dev["m"].sync()
    ml, mr, nm = rows.results()
    for p in range(pc.NPAIRS):
        nl, nr = int(P["counts"][pc.FIRST_L + p]), int(P["counts"][pc.FIRST_R + p])
        want = reading(P, bare, p)
        assert want[3]["l2r_cross_writes"] == 0 and want[3]["r2l_cross_writes"] == 0
        _same(ml[p], mr[p], nm[p], want, nl, nr, (p, "second reading"))
    assert nm[:2].sum() > 200


def test_first_rows_and_fewer_pairs(pkg, dev):
    """first_l = 1, first_r = 5, npairs = 2 (pairs 1 and 2 of the pool); and left row 3 with right row 6: both rows empty."""
    case = dev["CASES"]["scene_th1"]
    D = dev["pools"]["scene"]
    P, cap = D["P"], D["cap"]
    rows = _Rows(pkg, case, cap, p0=1, npairs=2)
    rows.poison()
    assert _call(dev["L"], dev["m"], D["r"], cap, D["gs"], D["gi"], rows, case, first_l=1, first_r=5) == 0, dev["L"].orbm_last_error()
    dev["m"].sync()
    ml, mr, nm = rows.results()
    for i, p in enumerate((1, 2)):
        nl, nr = int(P["counts"][pc.FIRST_L + p]), int(P["counts"][pc.FIRST_R + p])
        _same(ml[i], mr[i], nm[i], reading(P, case, p, "scene_th1"), nl, nr, (p, "second reading"))
    assert nm[0] > 100 and nm[1] > 10
    assert P["counts"][3] == 0 and P["counts"][6] == 0
    rows = _Rows(pkg, case, cap, p0=0, npairs=1)                               # pair 0's queries over two empty rows
    rows.poison()
    assert _call(dev["L"], dev["m"], D["r"], cap, D["gs"], D["gi"], rows, case, first_l=3, first_r=6) == 0, dev["L"].orbm_last_error()
    dev["m"].sync()
    ml, mr, nm = rows.results()
    assert nm[0] == 0 and np.all(ml == -1) and np.all(mr == -1)


@pytest.fixture(scope="module")
def block(pkg, oracle, synth):
    """The scene pool's 8 images through the product extractor in one batch: its result block, the matcher on the extractor's stream."""
    imgs = fc.images(synth)
    stride = (pc.W + 63) // 64 * 64
    dimg = pkg.DeviceBuffer(pc.NROWS * stride * pc.H)
    for i, im in enumerate(imgs):
        pad = np.zeros((pc.H, stride), np.uint8); pad[:, :pc.W] = im
        dimg.upload(pad, offset=i * stride * pc.H)
    arr = (C.c_void_p * pc.NROWS)(*[dimg.ptr + i * stride * pc.H for i in range(pc.NROWS)])
    L = pkg.lib()
    ex = pkg.ORBextractor(fc.NF, 1.2, pc.NLEV, 20, 7, max_size=(pc.W, pc.H), max_batch=pc.NROWS)
    mt = pkg.ORBmatcher(0.9)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    lap = np.zeros(2 * pc.NROWS, np.int32)
    ex.enqueue_device(arr, pc.W, pc.H, stride, lap)
    ex.sync()
    res = ex.fetch_all()
    rows = [(np.ascontiguousarray(k).view(pc.KP_DTYPE).reshape(-1), np.ascontiguousarray(d, np.uint8).reshape(-1, 32)) for _, k, d in res]
    cap = ex.cap
    P = dict(rows=rows, cap=cap, counts=np.array([len(k) for k, _ in rows], np.int32))
    assert P["counts"][pc.FIRST_L + 3] == 0 and P["counts"][pc.FIRST_R + 2] == 0 and P["counts"].max() <= cap
    gs = pkg.DeviceBuffer(pc.NROWS * 3073 * 4); gi = pkg.DeviceBuffer(pc.NROWS * cap * 4)

    def extract_and_grid():
        ex.enqueue_device(arr, pc.W, pc.H, stride, lap)
        r = ex.result_device()
        assert L.orbm_grid_build_batch_async(mt.h, r["kps"], r["counts"], pc.NROWS, cap, 0.0, 0.0, pc.INV_W, pc.INV_H, gs.ptr, gi.ptr) == 0, L.orbm_last_error()
        return r

    def on_block(case):
        """The case with the block's counts: partner entries are honoured against the rows that are searched."""
        c = copy.copy(case)
        c.counts = P["counts"]
        return c

    yield dict(P=P, CASES=pc.cases(oracle, synth), ex=ex, mt=mt, L=L, cap=cap, gs=gs, gi=gi, extract_and_grid=extract_and_grid, on_block=on_block,
               keep=(dimg, arr))
    ex.close(); mt.close()


def test_result_block(pkg, block):
    """Pairs 1..3 of a scene case on an extractor result block with orbm_grid_build_batch_async over it: first_l = 1, first_r = 5, npairs = 3."""
    B = block
    case, P, cap, mt = B["on_block"](B["CASES"]["scene_th3_far"]), B["P"], B["cap"], B["mt"]
    r = B["extract_and_grid"]()
    rows = _Rows(pkg, case, cap, p0=1, npairs=3)
    rows.poison()
    assert _call(B["L"], mt, r, cap, B["gs"], B["gi"], rows, case, first_l=1, first_r=5) == 0, B["L"].orbm_last_error()
    B["ex"].sync()
    ml, mr, nm = rows.results()
    for i, p in enumerate((1, 2, 3)):
        nl, nr = int(P["counts"][pc.FIRST_L + p]), int(P["counts"][pc.FIRST_R + p])
        _same(ml[i], mr[i], nm[i], reading(P, case, p), nl, nr, (p, "second reading"))
        _same(ml[i], mr[i], nm[i], single_pair(pkg, mt, P, case, p), nl, nr, (p, "host entry point"))
    assert nm[0] > 100 and nm[1] > 10 and nm[2] > 10


def test_capture_replay(pkg, block):
    """Extraction + grid + the two-camera search captured after one eager run: two replays give the eager rows; after the right
    projections, the blocked arrays and the partner arrays are rewritten on the device a replay gives what a fresh eager call gives."""
    B = block
    case, cap, mt, ex, L = B["on_block"](B["CASES"]["scene_th3"]), B["cap"], B["mt"], B["ex"], B["L"]
    rows = _Rows(pkg, case, cap)

    def enqueue():
        r = B["extract_and_grid"]()
        assert _call(L, mt, r, cap, B["gs"], B["gi"], rows, case) == 0, L.orbm_last_error()

    rows.poison()
    enqueue()
    ex.sync()
    eager = rows.results()
    assert eager[2].sum() > 300
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    for _ in range(2):
        rows.poison()
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        for got, want in zip(rows.results(), eager):
            assert np.array_equal(got, want)
    # other right projections, other blocked slots and no partners on the left side, same buffers
    h = case.rows()
    rng = np.random.default_rng(5)
    live = np.isfinite(h["pxr"])
    rows.buf["pxr"].upload(np.where(live, h["pxr"] + rng.normal(0, 2, h["pxr"].shape), h["pxr"]).astype(np.float32))
    rows.buf["pyr"].upload(np.where(live, h["pyr"] + rng.normal(0, 2, h["pyr"].shape), h["pyr"]).astype(np.float32))
    rows.bl.upload((rng.random((pc.NPAIRS, cap)) < 0.5).astype(np.uint8)); rows.br.upload((rng.random((pc.NPAIRS, cap)) < 0.5).astype(np.uint8))
    rows.l2r.upload(np.full((pc.NPAIRS, cap), -1, np.int32))
    rows.poison()
    assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
    ex.sync()
    replay = rows.results()
    rows.poison()
    enqueue()
    ex.sync()
    fresh = rows.results()
    for got, want in zip(replay, fresh):
        assert np.array_equal(got, want)
    assert not np.array_equal(fresh[1], eager[1]) and not np.array_equal(fresh[0], eager[0])   # the rewritten inputs do change both rows


def test_refusals_enqueue_nothing(pkg):
    """Every refusal of the header comment, with the documented code; the output buffers stay as they were."""
    m = pkg.ORBmatcher()
    L = m.L
    one = pkg.DeviceBuffer(4096)
    dm = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))
    sf = np.ones(16, np.float32)
    p, o = one.ptr, dm.ptr
    names = ["kps", "desc", "counts", "grid_start", "grid_idx", "nq", "in_view", "px", "py", "view_cos", "level", "in_view_r", "pxr", "pyr",
             "view_cos_r", "level_r", "qdesc", "mp_obs", "match_l", "match_r", "nmatches", "sf"]

    def call(cap=4, qs=4, nlev=8, npairs=1, first_l=0, first_r=1, null=None, optional=p):
        a = {n: p for n in names}
        a.update(match_l=o, match_r=o, nmatches=o, sf=_vp(sf))
        if null:
            a[null] = None
        return L.orbm_search_by_projection_points_fisheye_batch_async(
            m.h, a["kps"], a["desc"], a["counts"], cap, a["grid_start"], a["grid_idx"], 0.0, 0.0, pc.INV_W, pc.INV_H, first_l, first_r, npairs,
            optional, optional, optional, optional, a["nq"], qs, a["in_view"], a["px"], a["py"], a["view_cos"], a["level"],
            a["in_view_r"], a["pxr"], a["pyr"], a["view_cos_r"], a["level_r"], optional, 20.0, a["qdesc"], a["mp_obs"], 0,
            1.0, 0.8, a["sf"], nlev, a["match_l"], a["match_r"], a["nmatches"])

    for n in names:
        assert call(null=n) == -2, n
    assert call(npairs=0) == -2 and call(cap=0) == -2 and call(qs=0) == -2 and call(nlev=0) == -2
    assert call(first_l=-1) == -2 and call(first_r=-1) == -2
    assert call(cap=65536) == -3 and b"65535" in L.orbm_last_error()
    assert call(qs=(1 << 20) + 1) == -3
    assert call(nlev=13) == -3
    assert call(npairs=65536) == -3
    m.sync()
    assert np.all(dm.download(np.int32, 16) == 12345)
    m.close()
