"""Depth point selection on the device: orbm_select_depth_points(_batch_async) -- the sorted walk of Tracking::UpdateLastFrame /
CreateNewKeyFrame and NeedNewKeyFrame's close counts -- against tests/second_reading_depth_select.py, entry for entry: device form ==
host form == second reading.  orbm_adopt_new_points_batch_async against numpy, byte for byte.  The chain test runs the INTEGRATION
recipe "RGB-D frames on the device" through unproject -> select -> adopt up to the M4 search and compares its match rows with the same
M4 call fed with rows patched on the host from the second reading."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import second_reading_depth_select as R
import second_reading_rgbd as RG
from test_gpu_rgbd import CDIST, CFACTOR, CH, CK, CMB, CW, MBF, TH, _ChainBuffers, _upload_rows, chain  # noqa: F401  (chain is a fixture)
from test_second_reading_depth_select_cpu import CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN, INF = float("nan"), float("inf")
SENT_I, SENT_B = -12345, 0x5A


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def M(pkg):
    m = pkg.ORBmatcher(0.9)
    return dict(m=m, L=m.L)


class _Rows:
    """Inputs and outputs of one device call: [nrows][cap] rows, the outputs with one sentinel row (entry) before and after."""

    def __init__(self, pkg, counts, first, nrows, cap, depth, keeps, tracked):
        self.pkg, self.first, self.nrows, self.cap = pkg, first, nrows, cap
        self.counts = np.asarray(counts, np.int32)
        self.depth = np.ascontiguousarray(depth, F); self.keeps = keeps; self.tracked = tracked
        assert self.depth.shape == (nrows, cap)
        self.dc = pkg.DeviceBuffer(self.counts.nbytes).upload(self.counts)
        self.dd = pkg.DeviceBuffer(self.depth.nbytes).upload(self.depth)
        self.dk = None if keeps is None else pkg.DeviceBuffer(nrows * cap).upload(np.ascontiguousarray(keeps, np.uint8))
        self.dt = None if tracked is None else pkg.DeviceBuffer(nrows * cap).upload(np.ascontiguousarray(tracked, np.uint8))
        self.order = pkg.DeviceBuffer((nrows + 2) * cap * 4); self.cn = pkg.DeviceBuffer((nrows + 2) * cap)
        self.cnt = [pkg.DeviceBuffer((nrows + 2) * 4) for _ in range(4)]       # nvisit, ncreate, nclose_tracked, nclose_untracked
        self.reset()

    def reset(self):
        n2 = self.nrows + 2
        self.order.upload(np.full(n2 * self.cap, SENT_I, np.int32)); self.cn.upload(np.full(n2 * self.cap, SENT_B, np.uint8))
        for b in self.cnt:
            b.upload(np.full(n2, SENT_I, np.int32))

    def call(self, M, th, max_points, close=True, **kw):
        a = dict(nrows=self.nrows, first=self.first, cap=self.cap, counts=self.dc.ptr, depth=self.dd.ptr, keeps=self.dk.ptr if self.dk else None,
                 tracked=self.dt.ptr if self.dt else None, th=th, mp=max_points, order=self.order.ptr + self.cap * 4, cn=self.cn.ptr + self.cap,
                 nv=self.cnt[0].ptr + 4, nc=self.cnt[1].ptr + 4, ct=self.cnt[2].ptr + 4 if close else None, cu=self.cnt[3].ptr + 4 if close else None)
        a.update(kw)
        return M["L"].orbm_select_depth_points_batch_async(M["m"].h, a["nrows"], a["first"], a["cap"], a["counts"], a["depth"], a["keeps"], a["tracked"],
                                                           a["th"], a["mp"], a["order"], a["cn"], a["nv"], a["nc"], a["ct"], a["cu"])

    def fetch(self):
        n2, cap = self.nrows + 2, self.cap
        order = self.order.download(np.int32, n2 * cap).reshape(n2, cap); cn = self.cn.download(np.uint8, n2 * cap).reshape(n2, cap)
        cnt = [b.download(np.int32, n2) for b in self.cnt]
        assert np.all(order[[0, -1]] == SENT_I) and np.all(cn[[0, -1]] == SENT_B), "a row outside the call was written"
        assert all(c[0] == SENT_I and c[-1] == SENT_I for c in cnt), "a count outside the call was written"
        return order[1:-1], cn[1:-1], [c[1:-1] for c in cnt]

    def untouched(self):
        n2, cap = self.nrows + 2, self.cap
        return (np.all(self.order.download(np.int32, n2 * cap) == SENT_I) and np.all(self.cn.download(np.uint8, n2 * cap) == SENT_B)
                and all(np.all(b.download(np.int32, n2) == SENT_I) for b in self.cnt))

    def expect(self, r, th, max_points):
        n = min(max(int(self.counts[self.first + r]), 0), self.cap)
        k = None if self.keeps is None else self.keeps[r, :n]; t = None if self.tracked is None else self.tracked[r, :n]
        nv, order, create, ncreate = R.select(self.depth[r, :n], k, th, max_points)
        return n, nv, order, create, ncreate, R.close_counts(self.depth[r, :n], t, th)


def _check(M, rows, th, max_points, close=True, host=True):
    """device form == second reading == host form for every row of the call; returns the nvisit row"""
    rows.reset()
    assert rows.call(M, th, max_points, close=close) == 0, M["L"].orbm_last_error()
    M["m"].sync()
    order, cn, cnt = rows.fetch()
    for r in range(rows.nrows):
        n, nv, eorder, ecreate, encreate, eclose = rows.expect(r, th, max_points)
        print("row %d: n %d, nvisit device %d reading %d; ncreate %d / %d; close %s / %s" % (r, n, cnt[0][r], nv, cnt[1][r], encreate, (cnt[2][r], cnt[3][r]), eclose))
        assert cnt[0][r] == nv and cnt[1][r] == encreate
        assert np.array_equal(order[r, :nv], eorder) and np.all(order[r, nv:] == -1), np.flatnonzero(order[r, :nv] != eorder)[:8]
        assert np.array_equal(cn[r, :n], ecreate) and not cn[r, n:].any()
        if close:
            assert (cnt[2][r], cnt[3][r]) == eclose
        else:
            assert cnt[2][r] == SENT_I and cnt[3][r] == SENT_I
        if host:
            k = None if rows.keeps is None else rows.keeps[r, :n]; t = None if rows.tracked is None else rows.tracked[r, :n]
            hnv, horder, hcn, hnc, hct, hcu = M["m"].SelectDepthPoints(rows.depth[r, :n], k, t, th, max_points)
            assert hnv == nv and np.array_equal(horder[:nv], eorder) and np.all(horder[nv:] == -1) and np.array_equal(hcn, ecreate)
            assert hnc == encreate and (hct, hcu) == eclose
    return cnt[0]


def _random_depth(rng, shape):
    """metres with ties (a quarter of the slots share eight values) and holes: -1 (no depth), 0, NaN, a negative, +inf"""
    d = rng.uniform(0.3, 8.0, shape).astype(F)
    tie = rng.random(shape) < 0.25
    d[tie] = rng.choice(np.array([0.5, 1.0, 2.0, 3.0, 3.5, 4.0, 6.0, 7.5], F), int(tie.sum()))
    for p, v in ((0.15, -1.0), (0.03, 0.0), (0.03, NAN), (0.02, -2.0), (0.02, INF)):
        d[rng.random(shape) < p] = v
    return d


@pytest.mark.parametrize("cap", [1, 63, 64, 65, 130, 257, 1000])
def test_device_host_and_reading_agree(pkg, M, cap):
    """Counts 0, 1, cap and one in between in one call with first = 1 (block frame 0, with a large count, is never in the call); beyond a
    row's count lie NaNs, positive depths and keeps_mp = 1, which must not be visited."""
    rng = np.random.default_rng(500 + cap)
    counts = [cap, 0, 1, cap, max(1, cap * 2 // 3)]
    depth = _random_depth(rng, (4, cap))
    keeps = (rng.random((4, cap)) < 0.4).astype(np.uint8); tracked = (rng.random((4, cap)) < 0.5).astype(np.uint8)
    for r in range(4):
        n = counts[1 + r]
        depth[r, n:] = np.where(rng.random(cap - n) < 0.5, NAN, rng.uniform(0.01, 0.2, cap - n)).astype(F)   # closer than any slot of the row
        keeps[r, n:] = 1
    depth[1, 0] = 2.0                                                       # the row of count 1 has its depth point
    rows = _Rows(pkg, counts, 1, 4, cap, depth, keeps, tracked)
    seen = set()
    for th, mp in ((3.0, 100), (3.0, 7), (NAN, 100), (INF, 0), (0.4, 0), (3.5, 20)):
        seen.update(_check(M, rows, th, mp).tolist())
    assert len(seen) > (1 if cap == 1 else 3)                               # 0, 1 and several bounds were exercised
    bare = _Rows(pkg, counts, 1, 4, cap, depth, None, None)                 # the NULL optionals: no MapPoints, no close counts
    _check(M, bare, 3.0, 7, close=False, host=False)
    _check(M, bare, 3.0, 7)


def _group_key(c):
    return (repr(float(c["th"])), c["max_points"])


def test_hand_worked_cases_in_rows(pkg, M):
    """The cases of tests/test_second_reading_depth_select_cpu.py laid into rows of 152 slots, one call per (th_depth, max_points), and
    compared with the HAND-WORKED answers, not only with the reading."""
    cap = 152
    groups = {}
    for c in CASES:
        groups.setdefault(_group_key(c), []).append(c)
    for cases in groups.values():
        nrows = len(cases)
        depth = np.full((nrows, cap), 0.001, F); keeps = np.ones((nrows, cap), np.uint8); tracked = np.ones((nrows, cap), np.uint8)   # beyond the count: garbage
        counts = np.zeros(nrows, np.int32)
        for r, c in enumerate(cases):
            n = len(c["depth"]); counts[r] = n
            depth[r, :n] = c["depth"]
            keeps[r, :n] = 0 if c["keeps"] is None else c["keeps"]; tracked[r, :n] = 0 if c["tracked"] is None else c["tracked"]
        rows = _Rows(pkg, counts, 0, nrows, cap, depth, keeps, tracked)
        _check(M, rows, cases[0]["th"], cases[0]["max_points"])
        order, cn, cnt = rows.fetch()
        for r, c in enumerate(cases):
            nv = c["nvisit"]
            assert cnt[0][r] == nv and np.array_equal(order[r, :nv], c["order"]) and np.array_equal(cn[r, :counts[r]], c["create"]), c["name"]
            assert (cnt[2][r], cnt[3][r]) == c["close"], c["name"]


def test_u16_like_row_and_denormals(pkg, M):
    """A row as a 16-bit depth camera gives it: 90 % of the depths share four values (ties by slot decide).  And a row of positive
    denormals beside 0, -0.0 and small normals, against a denormal threshold: nothing is flushed to zero."""
    rng = np.random.default_rng(41)
    cap = 1000
    raw = rng.integers(500, 30000, cap).astype(np.uint16)
    shared = rng.random(cap) < 0.9
    raw[shared] = rng.choice(np.array([5000, 5001, 12500, 20000], np.uint16), int(shared.sum()))
    raw[rng.random(cap) < 0.05] = 0
    d16 = (raw.astype(F) * (F(1.0) / F(5000.0))).astype(F)
    d16[d16 <= 0] = -1.0
    rows = _Rows(pkg, [cap], 0, 1, cap, d16[None], (rng.random((1, cap)) < 0.3).astype(np.uint8), (rng.random((1, cap)) < 0.3).astype(np.uint8))
    for th, mp in ((float(F(5000) * (F(1.0) / F(5000.0))), 100), (2.5, 100), (0.05, 100), (4.0, 600)):
        _check(M, rows, th, mp)
    den = np.array([1e-40, 0.0, 1e-45, -0.0, 2e-38, 1e-41, -1e-40, 1e-40, 3e-41, 1.0, 1e-45, NAN], F)
    assert den[2] > 0 and den[2].view(np.uint32) == 1                       # the smallest positive denormal
    rows = _Rows(pkg, [len(den)], 0, 1, len(den), den[None], None, None)
    nv = _check(M, rows, 1e-41, 0)                                          # close: the two 1e-45; 1e-41 == th is not; walk: 2 + the equal one + 1
    assert nv[0] == 4 and rows.fetch()[0][0, :4].tolist() == [2, 10, 5, 8]
    assert rows.fetch()[2][3][0] == 2
    assert _check(M, rows, 0.0, 100)[0] == 8                                # every positive depth, the denormals included


def test_largest_row_descending(pkg, M):
    """cap = ORBM_DEPTH_SELECT_MAX_CAP, every slot valid, depths descending (the sort's worst input order), with a tie every 16 slots."""
    cap = 16384
    d = (cap - np.arange(cap)).astype(F) / F(4.0)                          # 4096 m down to 0.25 m in quarter metres
    d[15::16] = d[14::16]                                                   # slot 16k + 15 ties with slot 16k + 14
    keeps = (np.arange(cap) % 3 == 0).astype(np.uint8)
    rows = _Rows(pkg, [cap], 0, 1, cap, d[None], keeps[None], keeps[None])
    nv = _check(M, rows, 2000.25, 100)
    assert 7000 < nv[0] < 9000
    assert _check(M, rows, NAN, 100, host=False)[0] == cap


def test_refused_arguments_enqueue_nothing(pkg, M):
    L, m = M["L"], M["m"]
    cap = 64
    rng = np.random.default_rng(3)
    rows = _Rows(pkg, [cap, cap], 0, 2, cap, _random_depth(rng, (2, cap)), np.zeros((2, cap), np.uint8), np.zeros((2, cap), np.uint8))
    for kw in (dict(counts=None), dict(depth=None), dict(order=None), dict(cn=None), dict(nv=None), dict(nc=None), dict(nrows=0), dict(cap=0), dict(cap=-5),
               dict(first=-1), dict(mp=-1)):
        assert rows.call(M, 3.0, 100, **kw) == -2, kw
    assert rows.call(M, 3.0, 100, cap=pkg.DEPTH_SELECT_MAX_CAP + 1) == -3 and rows.call(M, 3.0, 100, nrows=65536) == -3
    assert L.orbm_select_depth_points_batch_async(None, 2, 0, cap, rows.dc.ptr, rows.dd.ptr, None, None, 3.0, 100, rows.order.ptr, rows.cn.ptr,
                                                  rows.cnt[0].ptr, rows.cnt[1].ptr, None, None) == -2
    d = np.ones(4, F); order = np.full(4, SENT_I, np.int32); cn = np.full(4, SENT_B, np.uint8); one = np.full(3, SENT_I, np.int32)
    host = lambda **kw: L.orbm_select_depth_points(m.h, kw.get("n", 4), kw.get("depth", _vp(d)), None, None, 3.0, kw.get("mp", 100), kw.get("order", _vp(order)),
                                                   kw.get("cn", _vp(cn)), one.ctypes.data, one.ctypes.data + 4, one.ctypes.data + 8)
    assert host(n=-1) == -2 and host(depth=None) == -2 and host(order=None) == -2 and host(cn=None) == -2 and host(mp=-1) == -2
    assert host(n=pkg.DEPTH_SELECT_MAX_CAP + 1) == -3
    assert np.all(order == SENT_I) and np.all(cn == SENT_B) and np.all(one == SENT_I)
    assert host(n=0) == 0 and one.tolist() == [0, 0, 0]                     # an empty frame is no error
    a = _Adopt(pkg, rng, 2, 0, cap, [cap, cap], None)
    for kw in (dict(counts=None), dict(cn=None), dict(x3n=None), dict(desc=None), dict(x3=None), dict(has=None), dict(obs=None), dict(qd=None), dict(nrows=0),
               dict(cap=0), dict(first=-1)):
        assert a.call(M, **kw) == -2, kw
    assert a.call(M, nrows=65536) == -3
    m.sync()
    assert rows.untouched() and a.untouched()


class _Adopt:
    """A block of `first + nrows` frames' descriptors and counts, the call's input rows and its four in/out rows with a sentinel row
    before and after."""

    def __init__(self, pkg, rng, nrows, first, cap, counts, outlier_p):
        self.nrows, self.first, self.cap = nrows, first, cap
        self.counts = np.asarray(counts, np.int32); nb = len(self.counts)
        self.desc = rng.integers(0, 256, (nb, cap, 32)).astype(np.uint8)
        self.cn = (rng.random((nrows, cap)) < 0.4).astype(np.uint8)         # set beyond the count as well: those slots must stay untouched
        self.x3n = rng.uniform(-5, 5, (nrows, cap, 3)).astype(F)
        self.outlier = None if outlier_p is None else (rng.random((nrows, cap)) < outlier_p).astype(np.uint8)
        self.x3 = rng.uniform(-5, 5, (nrows + 2, cap, 3)).astype(F); self.has = rng.integers(0, 2, (nrows + 2, cap)).astype(np.uint8)
        self.obs = rng.integers(0, 4, (nrows + 2, cap)).astype(np.uint8); self.qd = rng.integers(0, 256, (nrows + 2, cap, 32)).astype(np.uint8)
        up = lambda a: pkg.DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a))
        self.dc, self.ddesc, self.dcn, self.dx3n = up(self.counts), up(self.desc), up(self.cn), up(self.x3n)
        self.dout = None if self.outlier is None else up(self.outlier)
        self.dx3, self.dhas, self.dobs, self.dqd = up(self.x3), up(self.has), up(self.obs), up(self.qd)

    def call(self, M, **kw):
        cap = self.cap
        a = dict(nrows=self.nrows, first=self.first, cap=cap, counts=self.dc.ptr, cn=self.dcn.ptr, x3n=self.dx3n.ptr, desc=self.ddesc.ptr,
                 out=self.dout.ptr if self.dout else None, x3=self.dx3.ptr + cap * 12, has=self.dhas.ptr + cap, obs=self.dobs.ptr + cap, qd=self.dqd.ptr + cap * 32)
        a.update(kw)
        return M["L"].orbm_adopt_new_points_batch_async(M["m"].h, a["nrows"], a["first"], a["cap"], a["counts"], a["cn"], a["x3n"], a["desc"], a["out"],
                                                        a["x3"], a["has"], a["obs"], a["qd"])

    def fetch(self):
        n2, cap = self.nrows + 2, self.cap
        return (self.dx3.download(F, n2 * cap * 3).reshape(n2, cap, 3), self.dhas.download(np.uint8, n2 * cap).reshape(n2, cap),
                self.dobs.download(np.uint8, n2 * cap).reshape(n2, cap), self.dqd.download(np.uint8, n2 * cap * 32).reshape(n2, cap, 32))

    def untouched(self):
        x3, has, obs, qd = self.fetch()
        return x3.tobytes() == self.x3.tobytes() and np.array_equal(has, self.has) and np.array_equal(obs, self.obs) and np.array_equal(qd, self.qd)

    def expect(self):
        x3, has, obs, qd = self.x3.copy(), self.has.copy(), self.obs.copy(), self.qd.copy()
        for r in range(self.nrows):
            n = min(max(int(self.counts[self.first + r]), 0), self.cap)
            sel = np.flatnonzero(self.cn[r, :n])
            x3[1 + r, sel] = self.x3n[r, sel]
            has[1 + r, sel] = 1 if self.outlier is None else 1 - self.outlier[r, sel]
            obs[1 + r, sel] = 0
            qd[1 + r, sel] = self.desc[self.first + r, sel]
        return x3, has, obs, qd


@pytest.mark.parametrize("outlier_p", [None, 0.3])
def test_adopt_against_numpy(pkg, M, outlier_p):
    """first = 2 of a block of five frames, counts 0, cap and one in between; every slot the call must not write is compared byte for
    byte with what was there, the rows before and after the call's included."""
    rng = np.random.default_rng(9)
    cap = 130
    a = _Adopt(pkg, rng, 3, 2, cap, [cap, cap, 0, cap, 77], outlier_p)
    assert a.call(M) == 0, M["L"].orbm_last_error()
    M["m"].sync()
    got, want = a.fetch(), a.expect()
    assert got[0].tobytes() == want[0].tobytes()
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(g, w)
    assert not np.array_equal(want[3], a.qd) and (outlier_p is None or (want[1][1:-1][a.cn == 1] == 0).any())


# ---------------------------------------------------------------------------------------------------------------------------
# INTEGRATION.md "RGB-D frames on the device" on 3 synthetic frames: ... unproject -> select -> adopt -> project -> M4
# ---------------------------------------------------------------------------------------------------------------------------
SEL_TH, SEL_MAX = 2.7, 30


class _Sel:
    """The caller's side of the last frames' MapPoints (pair p: last frame p) and the rows the three new calls write."""

    def __init__(self, pkg, Cn):
        cap = Cn["cap"]; rng = np.random.default_rng(19)
        self.keeps = (rng.random((2, cap)) < 0.35).astype(np.uint8)         # pMP && Observations() >= 1
        stale = (rng.random((2, cap)) < 0.15) & (self.keeps == 0)           # pMP with Observations() < 1: replaced when visited, kept otherwise
        self.outlier = (rng.random((2, cap)) < 0.2).astype(np.uint8)
        self.has = ((self.keeps == 1) | stale).astype(np.uint8)
        self.obs = self.keeps.copy()
        self.x3 = rng.uniform(-0.6, 0.6, (2, cap, 3)).astype(F); self.x3[:, :, 2] += F(2.6)   # in front of the cameras
        self.qd = rng.integers(0, 256, (2, cap, 32)).astype(np.uint8)
        for p in range(2):                                                  # a kept MapPoint carries its keypoint's descriptor
            n = Cn["counts"][p]
            self.qd[p, :n][self.keeps[p, :n] == 1] = Cn["res"][p][2][self.keeps[p, :n] == 1]
        up = lambda a: pkg.DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a))
        self.dkeeps, self.dout = up(self.keeps), up(self.outlier)
        self.dhas, self.dobs, self.dx3, self.dqd = up(self.has), up(self.obs), up(self.x3), up(self.qd)
        self.order = pkg.DeviceBuffer(2 * cap * 4); self.cn = pkg.DeviceBuffer(2 * cap); self.cnt = pkg.DeviceBuffer(4 * 2 * 4)

    def upload_rows(self, x3, has, obs, qd):
        self.dx3.upload(np.ascontiguousarray(x3)); self.dhas.upload(np.ascontiguousarray(has)); self.dobs.upload(np.ascontiguousarray(obs))
        self.dqd.upload(np.ascontiguousarray(qd))


def _enqueue_front(pkg, Cn, B, S, with_extract=True):
    """extract, undistort (DEVICE), rgbd, grid, unproject, select, adopt: pair p = last frame p, current frame p + 1"""
    L, ex, mt, cap = Cn["L"], Cn["ex"], Cn["mt"], Cn["cap"]
    r = ex.result_device()
    if with_extract:
        ex.enqueue_device(Cn["arr"], CW, CH, Cn["stride"])
    assert L.orbm_undistort_keypoints(mt.h, pkg.DEVICE, r["kps"], 3 * cap, _vp(CK), _vp(CDIST), 4, _vp(CK), B.un.ptr) >= 0, L.orbm_last_error()
    assert L.orbm_stereo_from_rgbd_batch_async(mt.h, 3, 0, cap, r["kps"], B.un.ptr, r["counts"], Cn["dtab"].ptr, pkg.DEPTH_U16, CW, CH, Cn["dstride"] * 2,
                                               float(CFACTOR), MBF, B.ur.ptr, B.dp.ptr, B.nv.ptr) == 0, L.orbm_last_error()
    b = Cn["bounds"]
    assert L.orbm_grid_build_batch_async(mt.h, B.un.ptr, r["counts"], 3, cap, float(b[0]), float(b[2]), Cn["inv_w"], Cn["inv_h"], B.gs.ptr, B.gi.ptr) == 0
    assert L.orbm_unproject_stereo_batch_async(mt.h, 2, 0, cap, B.un.ptr, r["counts"], B.dp.ptr, B.twc.ptr, _vp(CK), B.x3.ptr, B.has.ptr) == 0, L.orbm_last_error()
    c = S.cnt.ptr
    assert L.orbm_select_depth_points_batch_async(mt.h, 2, 0, cap, r["counts"], B.dp.ptr, S.dkeeps.ptr, None, SEL_TH, SEL_MAX, S.order.ptr, S.cn.ptr,
                                                  c, c + 8, None, None) == 0, L.orbm_last_error()
    assert L.orbm_adopt_new_points_batch_async(mt.h, 2, 0, cap, r["counts"], S.cn.ptr, B.x3.ptr, r["desc"], S.dout.ptr, S.dx3.ptr, S.dhas.ptr, S.dobs.ptr,
                                               S.dqd.ptr) == 0, L.orbm_last_error()


def _enqueue_search(pkg, Cn, B, S):
    """project_last_frame + M4 over the four query rows as they stand"""
    L, mt, cap, b = Cn["L"], Cn["mt"], Cn["cap"], Cn["bounds"]
    r = Cn["ex"].result_device()
    assert L.orbm_project_last_frame_batch_async(mt.h, 2, B.tcur.ptr, B.tlast.ptr, r["counts"], cap, S.dx3.ptr, S.dhas.ptr, _vp(CK), _vp(b), CMB, 0,
                                                 B.valid.ptr, B.u.ptr, B.v.ptr, B.iz.ptr, B.dir.ptr) == 0, L.orbm_last_error()
    rc = L.orbm_search_by_projection_frame_batch_async(
        mt.h, B.un.ptr, r["desc"], r["counts"], cap, B.gs.ptr, B.gi.ptr, float(b[0]), float(b[2]), Cn["inv_w"], Cn["inv_h"], 1, 2,
        B.ur.ptr + cap * 4, MBF, None, B.dir.ptr, r["counts"], cap, B.valid.ptr, B.u.ptr, B.v.ptr, B.iz.ptr, B.octave.ptr, B.angle.ptr, S.dqd.ptr,
        S.dobs.ptr, TH, 0, _vp(Cn["sf"]), 8, 1, B.match.ptr, B.nm.ptr, None)
    assert rc == 0, L.orbm_last_error()


def _host_patched_rows(Cn, S):
    """The four query rows patched on the host from the second readings alone; also the selection's evidence per pair."""
    mt, res, cap = Cn["mt"], Cn["res"], Cn["cap"]
    x3, has, obs, qd = S.x3.copy(), S.has.copy(), S.obs.copy(), S.qd.copy()
    ev = []
    for p in range(2):
        n = Cn["counts"][p]
        un = mt.UndistortKeyPoints(res[p][1], CK, CDIST)
        _, depth, nd = RG.compute_stereo_from_rgbd(res[p][1], un, Cn["depth"][p], CFACTOR, MBF)
        x3n, _ = RG.unproject_stereo(un, depth, Cn["twc"][p], CK)
        nv, order, create, ncreate = R.select(depth, S.keeps[p, :n], SEL_TH, SEL_MAX)
        sel = np.flatnonzero(create)
        x3[p, sel] = x3n[sel]; has[p, sel] = 1 - S.outlier[p, sel]; obs[p, sel] = 0; qd[p, sel] = res[p][2][sel]
        ev.append(dict(nd=nd, nv=nv, order=order, create=create, ncreate=ncreate, visited_kept=int(S.keeps[p, order].sum())))
    return (x3, has, obs, qd), ev


def test_chain_extract_to_m4(pkg, chain):
    Cn = chain
    cap = Cn["cap"]
    B = _ChainBuffers(pkg, cap); S = _Sel(pkg, Cn)
    _upload_rows(Cn, B)
    want, ev = _host_patched_rows(Cn, S)
    for p, e in enumerate(ev):                                              # cannot pass vacuously
        print("pair %d: %d depth points, %d visited, %d created, %d visited slots keep their MapPoint" % (p, e["nd"], e["nv"], e["ncreate"], e["visited_kept"]))
        assert SEL_MAX + 1 < e["nv"] < e["nd"] and e["ncreate"] > 10 and e["visited_kept"] > 5
    _enqueue_front(pkg, Cn, B, S)
    _enqueue_search(pkg, Cn, B, S)
    Cn["ex"].sync()
    order = S.order.download(np.int32, 2 * cap).reshape(2, cap); cn = S.cn.download(np.uint8, 2 * cap).reshape(2, cap)
    cnt = S.cnt.download(np.int32, 4)
    for p, e in enumerate(ev):
        n = Cn["counts"][p]
        assert cnt[p] == e["nv"] and cnt[2 + p] == e["ncreate"]
        assert np.array_equal(order[p, :e["nv"]], e["order"]) and np.all(order[p, e["nv"]:] == -1)
        assert np.array_equal(cn[p, :n], e["create"]) and not cn[p, n:].any()
    got = (S.dx3.download(F, 2 * cap * 3).reshape(2, cap, 3), S.dhas.download(np.uint8, 2 * cap).reshape(2, cap),
           S.dobs.download(np.uint8, 2 * cap).reshape(2, cap), S.dqd.download(np.uint8, 2 * cap * 32).reshape(2, cap, 32))
    assert got[0].tobytes() == want[0].tobytes() and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
    match = B.match.download(np.int32, 2 * cap).reshape(2, cap).copy(); nm = B.nm.download(np.int32, 2).copy()
    # the same M4 call fed with the rows patched on the host
    S.upload_rows(*want)
    B.match.upload(np.full(2 * cap, SENT_I, np.int32)); B.nm.upload(np.full(2, SENT_I, np.int32))
    _enqueue_search(pkg, Cn, B, S)
    Cn["ex"].sync()
    match_h = B.match.download(np.int32, 2 * cap).reshape(2, cap); nm_h = B.nm.download(np.int32, 2)
    print("matches: device-adopted rows %s, host-patched rows %s" % (nm.tolist(), nm_h.tolist()))
    assert np.array_equal(nm, nm_h) and np.array_equal(match, match_h) and nm.min() > 5
    # and the selection matters: the rows before adoption give another result
    S.upload_rows(S.x3, S.has, S.obs, S.qd)
    _enqueue_search(pkg, Cn, B, S)
    Cn["ex"].sync()
    assert not np.array_equal(B.match.download(np.int32, 2 * cap).reshape(2, cap), match)


def test_capture_replay_follows_depth_and_keeps(pkg, chain):
    """After one eager run, extraction + select + adopt are captured; the depth and keeps_mp rows are then rewritten and the graph
    replayed: the new selection appears, and the counts after a second replay are the same (nothing accumulates)."""
    Cn = chain
    L, ex, mt, cap = Cn["L"], Cn["ex"], Cn["mt"], Cn["cap"]
    rng = np.random.default_rng(23)
    r = ex.result_device()
    counts = Cn["counts"]
    depth = _random_depth(rng, (2, cap)); keeps = (rng.random((2, cap)) < 0.4).astype(np.uint8)
    dd = pkg.DeviceBuffer(depth.nbytes).upload(depth); dk = pkg.DeviceBuffer(keeps.nbytes).upload(keeps)
    order = pkg.DeviceBuffer(2 * cap * 4); cn = pkg.DeviceBuffer(2 * cap); cnt = pkg.DeviceBuffer(4 * 2 * 4)
    a = _Adopt(pkg, rng, 2, 1, cap, [0, 0, 0], None)                        # its own in/out rows; counts and desc come from the block

    def enqueue():
        ex.enqueue_device(Cn["arr"], CW, CH, Cn["stride"])
        c = cnt.ptr
        assert L.orbm_select_depth_points_batch_async(mt.h, 2, 1, cap, r["counts"], dd.ptr, dk.ptr, dk.ptr, 3.0, 40, order.ptr, cn.ptr, c, c + 8, c + 16,
                                                      c + 24) == 0, L.orbm_last_error()
        assert a.call(dict(L=L, m=mt), counts=r["counts"], cn=cn.ptr, desc=r["desc"]) == 0, L.orbm_last_error()

    def expect(depth, keeps):
        out = []
        for p in range(2):
            n = counts[1 + p]
            nv, o, c, nc = R.select(depth[p, :n], keeps[p, :n], 3.0, 40)
            out.append((nv, o, c, nc) + R.close_counts(depth[p, :n], keeps[p, :n], 3.0))
        return out

    def check(want):
        go = order.download(np.int32, 2 * cap).reshape(2, cap); gc = cn.download(np.uint8, 2 * cap).reshape(2, cap); gn = cnt.download(np.int32, 8)
        for p, (nv, o, c, nc, ct, cu) in enumerate(want):
            n = counts[1 + p]
            assert gn[[p, 2 + p, 4 + p, 6 + p]].tolist() == [nv, nc, ct, cu]
            assert np.array_equal(go[p, :nv], o) and np.all(go[p, nv:] == -1) and np.array_equal(gc[p, :n], c) and not gc[p, n:].any()
        return gn.copy(), gc.copy()

    enqueue()
    ex.sync()
    eager_n, _ = check(expect(depth, keeps))
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    depth2 = _random_depth(rng, (2, cap)); keeps2 = (rng.random((2, cap)) < 0.7).astype(np.uint8)
    dd.upload(depth2); dk.upload(keeps2)
    want = expect(depth2, keeps2)
    got = []
    for _ in range(2):
        a.dx3.upload(a.x3); a.dhas.upload(a.has); a.dobs.upload(a.obs); a.dqd.upload(a.qd)
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        gn, gc = check(want)
        got.append(gn)
        x3, has, obs, qd = a.fetch()                                        # the adopt step of the graph followed the new create_new rows
        for p in range(2):
            sel = gc[p] == 1
            assert sel.any() and not obs[1 + p][sel].any() and has[1 + p][sel].all() and np.array_equal(obs[1 + p][~sel], a.obs[1 + p][~sel])
            assert x3[1 + p][sel].tobytes() == a.x3n[p][sel].tobytes() and x3[1 + p][~sel].tobytes() == a.x3[1 + p][~sel].tobytes()
    assert np.array_equal(got[0], got[1]) and not np.array_equal(got[0], eager_n)


def test_cpp_facade_select_depth_points(pkg, tmp_path):
    """facade/FrameGeometry.h's SelectDepthPoints on mock vectors against the walk written out in plain C++ in the same file."""
    pkg.build()
    exe = str(tmp_path / "facade_depth_select_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "facade_depth_select_smoke.cpp"),
                           "-L", os.path.join(ROOT, "orb-slam3_amd"), "-lorbslam3_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "orb-slam3_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "need-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "facade_depth_select_smoke ok" in out.stdout, out.stdout + out.stderr
