"""Batched two-camera SearchByProjection(CurrentFrame, LastFrame) -- M4 with Nleft != -1, Tracking::TrackWithMotionModel on a fisheye
rig -- on the device (orbm_search_by_projection_frame_fisheye_batch_async).  For every case of tests/fisheye_cases.py and every pair
the two match rows (ORBM_NO_MATCH padding included) and the count equal, entry for entry, (a) the product's host entry point
(ORBmatcher.SearchByProjectionFrameFisheye), (b) the oracle's and (c) the second reading of tests/second_reading_fisheye.py."""
import ctypes as C

import numpy as np
import pytest

import fisheye_cases as fc
from test_second_reading_fisheye_cpu import NAMES, second_reading_pair, single_pair

pytestmark = pytest.mark.gpu

ROW_KEYS = ("valid", "u", "v", "ur", "vr", "octave", "angle", "qdesc", "mp_obs")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class _Rows:
    """The per-pair device arrays of one call for pairs [p0, p0 + npairs) of a case; blocked rows re-laid to the pool's cap."""

    def __init__(self, pkg, case, cap, p0=0, npairs=fc.NPAIRS):
        self.npairs, self.qs, self.cap = npairs, case.q_stride, cap
        sel = slice(p0, p0 + npairs)
        h = case.rows()
        self.buf = {k: pkg.DeviceBuffer(h[k][sel].nbytes).upload(h[k][sel]) for k in ROW_KEYS + ("nq",)}
        self.dir = pkg.DeviceBuffer(max(npairs, 4)).upload(np.resize(case.dirs[sel], max(npairs, 4)))
        self.bl = pkg.DeviceBuffer(npairs * cap).upload(self.relaid(case.blocked_l[sel]))
        self.br = pkg.DeviceBuffer(npairs * cap).upload(self.relaid(case.blocked_r[sel]))
        self.ml = pkg.DeviceBuffer(npairs * cap * 4); self.mr = pkg.DeviceBuffer(npairs * cap * 4)
        self.nm = pkg.DeviceBuffer(npairs * 4); self.rt = pkg.DeviceBuffer(max(npairs, 4))

    def relaid(self, b):
        out = np.zeros((len(b), self.cap), np.uint8)
        w = min(self.cap, b.shape[1])
        out[:, :w] = b[:, :w]
        return out

    def poison(self):
        n = self.npairs * self.cap
        self.ml.upload(np.full(n, -7, np.int32)); self.mr.upload(np.full(n, -7, np.int32))
        self.nm.upload(np.full(self.npairs, -7, np.int32)); self.rt.upload(np.full(max(self.npairs, 4), 9, np.uint8))

    def results(self):
        n = self.npairs * self.cap
        return (self.ml.download(np.int32, n).reshape(self.npairs, self.cap), self.mr.download(np.int32, n).reshape(self.npairs, self.cap),
                self.nm.download(np.int32, self.npairs), self.rt.download(np.uint8, self.npairs))


def _call(L, m, r, cap, gs, gi, rows, case, first_l=fc.FIRST_L, first_r=fc.FIRST_R, retry_below=0, blocked=True, th=None):
    b = rows.buf
    return L.orbm_search_by_projection_frame_fisheye_batch_async(
        m.h, r["kps"], r["desc"], r["counts"], cap, gs.ptr, gi.ptr, 0.0, 0.0, fc.INV_W, fc.INV_H, first_l, first_r, rows.npairs,
        rows.bl.ptr if blocked else None, rows.br.ptr if blocked else None, rows.dir.ptr, b["nq"].ptr, rows.qs, b["valid"].ptr,
        b["u"].ptr, b["v"].ptr, b["ur"].ptr, b["vr"].ptr, b["octave"].ptr, b["angle"].ptr, b["qdesc"].ptr, b["mp_obs"].ptr,
        float(case.th if th is None else th), int(retry_below), _vp(fc.SF), fc.NLEV, int(case.check_ori), rows.ml.ptr, rows.mr.ptr, rows.nm.ptr, rows.rt.ptr)


def _same(row_l, row_r, n_dev, want, nl, nr, what):
    n, ml, mr = want[0], want[1], want[2]
    assert int(n_dev) == int(n), (what, int(n_dev), int(n))
    assert np.array_equal(row_l[:nl], ml), (what, "left", np.flatnonzero(row_l[:nl] != ml)[:8])
    assert np.array_equal(row_r[:nr], mr), (what, "right", np.flatnonzero(row_r[:nr] != mr)[:8])
    assert np.all(row_l[nl:] == -1) and np.all(row_r[nr:] == -1), (what, "padding")


@pytest.fixture(scope="module")
def dev(pkg, oracle, synth):
    """The cases' pool on the device with its grid."""
    P = fc.pool(oracle, synth)
    m = pkg.ORBmatcher(0.9); L = pkg.lib()
    cap = P["cap"]
    dk = pkg.DeviceBuffer(P["kps"].nbytes).upload(P["kps"]); dd = pkg.DeviceBuffer(P["desc"].nbytes).upload(P["desc"])
    dc = pkg.DeviceBuffer(P["counts"].nbytes).upload(P["counts"])
    r = dict(kps=dk.ptr, desc=dd.ptr, counts=dc.ptr)
    gs = pkg.DeviceBuffer(fc.NROWS * 3073 * 4); gi = pkg.DeviceBuffer(fc.NROWS * cap * 4)
    assert L.orbm_grid_build_batch_async(m.h, r["kps"], r["counts"], fc.NROWS, cap, 0.0, 0.0, fc.INV_W, fc.INV_H, gs.ptr, gi.ptr) == 0, L.orbm_last_error()
    m.sync()
    return dict(P=P, CASES=fc.cases(oracle, synth), m=m, OM=oracle._oracle_matcher_class()(), L=L, r=r, cap=cap, gs=gs, gi=gi, keep=(dk, dd, dc))


@pytest.mark.parametrize("name", NAMES)
def test_parity(pkg, dev, name):
    D = dev
    case, P, cap = D["CASES"][name], D["P"], D["cap"]
    rows = _Rows(pkg, case, cap)
    rows.poison()
    assert _call(D["L"], D["m"], D["r"], cap, D["gs"], D["gi"], rows, case) == 0, D["L"].orbm_last_error()
    D["m"].sync()
    ml, mr, nm, rt = rows.results()
    assert not rt.any()
    for p in range(fc.NPAIRS):
        nl, nr = int(P["counts"][fc.FIRST_L + p]), int(P["counts"][fc.FIRST_R + p])
        _same(ml[p], mr[p], nm[p], single_pair(pkg, D["m"], P, case, p), nl, nr, (name, p, "host entry point"))
        _same(ml[p], mr[p], nm[p], single_pair(pkg, D["OM"], P, case, p), nl, nr, (name, p, "oracle"))
        _same(ml[p], mr[p], nm[p], second_reading_pair(P, case, p), nl, nr, (name, p, "second reading"))
    assert nm[3] == 0 and np.all(ml[3] == -1) and np.all(mr[3] == -1)          # the empty left row
    if name != "retry":
        assert nm[:3].sum() > 300


def test_retry(pkg, dev):
    """retry_below = 20 on the device against the second reading's retry form and against the host entry point called twice."""
    D = dev
    case, P, cap, m = D["CASES"]["retry"], D["P"], D["cap"], D["m"]
    rows = _Rows(pkg, case, cap)
    for below in (case.retry_below, 0):
        rows.poison()
        assert _call(D["L"], m, D["r"], cap, D["gs"], D["gi"], rows, case, retry_below=below) == 0, D["L"].orbm_last_error()
        m.sync()
        ml, mr, nm, rt = rows.results()
        if not below:
            assert not rt.any()
            continue
        assert rt.tolist() == [1, 0, 0, 1]                                     # pair 0 is displaced, pair 3 has an empty left row
        for p in range(fc.NPAIRS):
            nl, nr = int(P["counts"][fc.FIRST_L + p]), int(P["counts"][fc.FIRST_R + p])
            want = second_reading_pair(P, case, p, retry=True)
            assert bool(rt[p]) == want[4]
            _same(ml[p], mr[p], nm[p], want, nl, nr, (p, "second reading, retry form"))
            host = single_pair(pkg, m, P, case, p)
            assert (host[0] < below) == bool(rt[p])
            if host[0] < below:
                host = single_pair(pkg, m, P, case, p, th=2 * case.th, use_blocked=False)
            _same(ml[p], mr[p], nm[p], host, nl, nr, (p, "host entry point called twice"))
        assert nm[0] >= below


@pytest.fixture(scope="module")
def block(pkg, oracle, synth):
    """The pool's 8 images through the product extractor in one batch: its result block, the matcher on the extractor's stream."""
    imgs = fc.images(synth)
    stride = (fc.W + 63) // 64 * 64
    dimg = pkg.DeviceBuffer(fc.NROWS * stride * fc.H)
    for i, im in enumerate(imgs):
        pad = np.zeros((fc.H, stride), np.uint8); pad[:, :fc.W] = im
        dimg.upload(pad, offset=i * stride * fc.H)
    arr = (C.c_void_p * fc.NROWS)(*[dimg.ptr + i * stride * fc.H for i in range(fc.NROWS)])
    L = pkg.lib()
    ex = pkg.ORBextractor(fc.NF, 1.2, fc.NLEV, 20, 7, max_size=(fc.W, fc.H), max_batch=fc.NROWS)
    mt = pkg.ORBmatcher(0.9)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    lap = np.zeros(2 * fc.NROWS, np.int32)
    ex.enqueue_device(arr, fc.W, fc.H, stride, lap)
    ex.sync()
    res = ex.fetch_all()
    rows = [(np.ascontiguousarray(k).view(fc.KP_DTYPE).reshape(-1), np.ascontiguousarray(d, np.uint8).reshape(-1, 32)) for _, k, d in res]
    cap = ex.cap
    P = dict(rows=rows, cap=cap, counts=np.array([len(k) for k, _ in rows], np.int32))
    assert P["counts"][fc.FIRST_L + 3] == 0 and P["counts"][fc.FIRST_R + 2] == 0 and P["counts"].max() <= cap
    gs = pkg.DeviceBuffer(fc.NROWS * 3073 * 4); gi = pkg.DeviceBuffer(fc.NROWS * cap * 4)

    def extract_and_grid():
        ex.enqueue_device(arr, fc.W, fc.H, stride, lap)
        r = ex.result_device()
        assert L.orbm_grid_build_batch_async(mt.h, r["kps"], r["counts"], fc.NROWS, cap, 0.0, 0.0, fc.INV_W, fc.INV_H, gs.ptr, gi.ptr) == 0, L.orbm_last_error()
        return r

    yield dict(P=P, CASES=fc.cases(oracle, synth), ex=ex, mt=mt, L=L, cap=cap, gs=gs, gi=gi, OM=oracle._oracle_matcher_class()(),
               extract_and_grid=extract_and_grid, keep=(dimg, arr))
    ex.close(); mt.close()


def test_result_block(pkg, block):
    """Pairs 1..3 of the blocked case on an extractor result block: first_l = 1, first_r = 5, npairs = 3."""
    B = block
    case, P, cap, mt = B["CASES"]["blocked"], B["P"], B["cap"], B["mt"]
    r = B["extract_and_grid"]()
    rows = _Rows(pkg, case, cap, p0=1, npairs=3)
    rows.poison()
    assert _call(B["L"], mt, r, cap, B["gs"], B["gi"], rows, case, first_l=1, first_r=5) == 0, B["L"].orbm_last_error()
    B["ex"].sync()
    ml, mr, nm, _ = rows.results()
    total = 0
    for i, p in enumerate((1, 2, 3)):
        nl, nr = int(P["counts"][fc.FIRST_L + p]), int(P["counts"][fc.FIRST_R + p])
        _same(ml[i], mr[i], nm[i], single_pair(pkg, mt, P, case, p), nl, nr, (p, "host entry point"))
        _same(ml[i], mr[i], nm[i], single_pair(pkg, B["OM"], P, case, p), nl, nr, (p, "oracle"))
        _same(ml[i], mr[i], nm[i], second_reading_pair(P, case, p), nl, nr, (p, "second reading"))
        total += int(nm[i])
    assert total > 100 and nm[2] == 0


def test_capture_replay(pkg, block):
    """Extraction + grid + the two-camera search (with retry) captured after one eager run: two replays give the eager rows; after ur /
    vr and the blocked arrays are rewritten on the device a replay gives what a fresh eager call gives."""
    B = block
    case, cap, mt, ex, L = B["CASES"]["retry"], B["cap"], B["mt"], B["ex"], B["L"]
    rows = _Rows(pkg, case, cap)

    def enqueue():
        r = B["extract_and_grid"]()
        assert _call(L, mt, r, cap, B["gs"], B["gi"], rows, case, retry_below=case.retry_below) == 0, L.orbm_last_error()

    rows.poison()
    enqueue()
    ex.sync()
    eager = rows.results()
    assert eager[2].sum() > 100 and eager[3].any() and not eager[3].all()
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    for _ in range(2):
        rows.poison()
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        for got, want in zip(rows.results(), eager):
            assert np.array_equal(got, want)
    # other right projections and other blocked slots, same buffers
    h = case.rows()
    rng = np.random.default_rng(5)
    rows.buf["ur"].upload((h["ur"] + rng.normal(0, 4, h["ur"].shape)).astype(np.float32))
    rows.buf["vr"].upload((h["vr"] + rng.normal(0, 4, h["vr"].shape)).astype(np.float32))
    rows.bl.upload((rng.random((fc.NPAIRS, cap)) < 0.5).astype(np.uint8)); rows.br.upload((rng.random((fc.NPAIRS, cap)) < 0.5).astype(np.uint8))
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
    assert not np.array_equal(fresh[1], eager[1])                              # the rewritten inputs do change the right rows


def test_refusals_enqueue_nothing(pkg):
    """Every refusal of the header comment, with the documented code; the output buffers stay as they were."""
    m = pkg.ORBmatcher()
    L = m.L
    one = pkg.DeviceBuffer(4096)
    dm = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))
    sf = np.ones(16, np.float32)
    p, o = one.ptr, dm.ptr
    names = ["kps", "desc", "counts", "grid_start", "grid_idx", "nq", "valid", "u", "v", "ur", "vr", "octave", "angle", "qdesc", "mp_obs",
             "match_l", "match_r", "nmatches", "sf"]

    def call(cap=4, qs=4, nlev=8, npairs=1, first_l=0, first_r=1, retry_below=0, null=None, optional=p):
        a = {n: p for n in names}
        a.update(match_l=o, match_r=o, nmatches=o, sf=_vp(sf))
        if null:
            a[null] = None
        return L.orbm_search_by_projection_frame_fisheye_batch_async(
            m.h, a["kps"], a["desc"], a["counts"], cap, a["grid_start"], a["grid_idx"], 0.0, 0.0, fc.INV_W, fc.INV_H, first_l, first_r, npairs,
            optional, optional, optional, a["nq"], qs, a["valid"], a["u"], a["v"], a["ur"], a["vr"], a["octave"], a["angle"], a["qdesc"], a["mp_obs"],
            15.0, retry_below, a["sf"], nlev, 1, a["match_l"], a["match_r"], a["nmatches"], None)

    for n in names:
        assert call(null=n) == -2, n
    assert call(npairs=0) == -2 and call(cap=0) == -2 and call(qs=0) == -2 and call(nlev=0) == -2
    assert call(first_l=-1) == -2 and call(first_r=-1) == -2 and call(retry_below=-1) == -2
    assert call(cap=65536) == -3 and b"65535" in L.orbm_last_error()
    assert call(qs=(1 << 20) + 1) == -3
    assert call(nlev=13) == -3
    assert call(npairs=65536) == -3
    m.sync()
    assert np.all(dm.download(np.int32, 16) == 12345)
    m.close()
