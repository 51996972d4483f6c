"""MapPoint refresh on the device: orbm_distinctive_descriptors(_batch_async) -- MapPoint::ComputeDistinctiveDescriptors -- and
orbm_update_normal_and_depth(_batch_async) -- MapPoint::UpdateNormalAndDepth -- against tests/second_reading_mappoint.py, bit for bit
(floats compared as uint32, no tolerance): host form == device form == second reading.  Outputs are pre-filled with sentinels, so a row
that must stay untouched is seen to stay.  The chain test feeds the rows straight into orbm_is_in_frustum(ORBM_DEVICE) and the M3 batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mappoint_cases as MC
import second_reading_mappoint as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SENT_D, SENT_I, SENT_F, SENT_U = 0xCD, -777, F(-777.25), 0x5A


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class _Dev:
    """The call's inputs on the device."""

    def __init__(self, pkg, P, M):
        up = lambda a: pkg.DeviceBuffer(max(a.nbytes, 4)).upload(np.ascontiguousarray(a))
        self.desc, self.kps, self.counts, self.ow_l, self.ow_r = up(P["desc"]), up(P["kps"]), up(P["counts"]), up(P["ow_l"]), up(P["ow_r"])
        self.off, self.row, self.slot, self.flags, self.valid = up(M["off"]), up(M["row"]), up(M["slot"]), up(M["flags"]), up(M["valid"])
        self.pw, self.ref_row, self.ref_slot = up(M["pw"]), up(M["ref_row"]), up(M["ref_slot"])


class _Out:
    """Outputs of nmp MapPoints with one sentinel MapPoint before and after."""

    def __init__(self, pkg, nmp):
        self.n = nmp
        n2 = nmp + 2
        self.mp_desc, self.best, self.med = pkg.DeviceBuffer(n2 * 32), pkg.DeviceBuffer(n2 * 4), pkg.DeviceBuffer(n2 * 4)
        self.normal, self.mn, self.mx, self.up = pkg.DeviceBuffer(n2 * 12), pkg.DeviceBuffer(n2 * 4), pkg.DeviceBuffer(n2 * 4), pkg.DeviceBuffer(n2)
        self.reset()

    def reset(self):
        n2 = self.n + 2
        self.mp_desc.upload(np.full(n2 * 32, SENT_D, np.uint8)); self.best.upload(np.full(n2, SENT_I, np.int32)); self.med.upload(np.full(n2, SENT_I, np.int32))
        self.normal.upload(np.full(n2 * 3, SENT_F, F)); self.mn.upload(np.full(n2, SENT_F, F)); self.mx.upload(np.full(n2, SENT_F, F))
        self.up.upload(np.full(n2, SENT_U, np.uint8))

    def fetch(self):
        n2 = self.n + 2
        d = self.mp_desc.download(np.uint8, n2 * 32).reshape(n2, 32); b = self.best.download(np.int32, n2); md = self.med.download(np.int32, n2)
        nv = self.normal.download(F, n2 * 3).reshape(n2, 3); mn = self.mn.download(F, n2); mx = self.mx.download(F, n2); up = self.up.download(np.uint8, n2)
        assert np.all(d[[0, -1]] == SENT_D) and b[0] == b[-1] == SENT_I and md[0] == md[-1] == SENT_I, "a MapPoint outside the call was written"
        assert np.all(nv[[0, -1]] == SENT_F) and mn[0] == mn[-1] == SENT_F and mx[0] == mx[-1] == SENT_F and up[0] == up[-1] == SENT_U
        return dict(desc=d[1:-1], best=b[1:-1], med=md[1:-1], normal=nv[1:-1], mn=mn[1:-1], mx=mx[1:-1], up=up[1:-1])

    def untouched(self):
        n2 = self.n + 2
        return (np.all(self.mp_desc.download(np.uint8, n2 * 32) == SENT_D) and np.all(self.best.download(np.int32, n2) == SENT_I) and
                np.all(self.med.download(np.int32, n2) == SENT_I) and np.all(self.normal.download(F, n2 * 3) == SENT_F) and
                np.all(self.mn.download(F, n2) == SENT_F) and np.all(self.mx.download(F, n2) == SENT_F) and np.all(self.up.download(np.uint8, n2) == SENT_U))


def _expect(P, M, lo=0, hi=None):
    """The second reading's rows for MapPoints [lo, hi) of the call, over sentinel-filled outputs."""
    hi = M["nmp"] if hi is None else hi
    n = hi - lo
    off = M["off"][lo:hi + 1]
    d, b, md = R.distinctive_batch(P["desc"], P["counts"], off, M["row"], M["slot"], M["flags"], M["valid"][lo:hi], np.full((n, 32), SENT_D, np.uint8))
    nv, mn, mx, up = R.normal_depth_batch(P["kps"], P["counts"], P["ow_l"], P["ow_r"], off, M["row"], M["slot"], M["flags"], M["valid"][lo:hi],
                                          M["pw"][lo:hi], M["ref_row"][lo:hi], M["ref_slot"][lo:hi], MC.SCALE,
                                          np.full((n, 3), SENT_F, F), np.full(n, SENT_F, F), np.full(n, SENT_F, F))
    return dict(desc=d, best=b, med=md, normal=nv, mn=mn, mx=mx, up=up)


def _same(got, want, what=("desc", "best", "med", "normal", "mn", "mx", "up")):
    for k in what:
        g, w = got[k], want[k]
        if g.dtype == F:
            g, w = _bits(g), _bits(w)
        assert np.array_equal(g, w), (k, np.argwhere(g != w)[:8].tolist())


def _enqueue(S, out, lo=0, hi=None, valid=True, which="dn", **kw):
    """The device calls (d: descriptors, n: normals) for MapPoints [lo, hi); kw overrides single arguments (the refused-argument test)."""
    M, D, m, L = S["M"], S["D"], S["m"], S["L"]
    hi = M["nmp"] if hi is None else hi
    a = dict(nmp=hi - lo, nrows=MC.NROWS, cap=MC.CAP, desc=D.desc.ptr, kps=D.kps.ptr, counts=D.counts.ptr, ow_l=D.ow_l.ptr, ow_r=D.ow_r.ptr,
             nobs=len(M["row"]), off=D.off.ptr + 4 * lo, row=D.row.ptr, slot=D.slot.ptr, flags=D.flags.ptr, valid=D.valid.ptr + lo if valid else None,
             pw=D.pw.ptr + 12 * lo, ref_row=D.ref_row.ptr + 4 * lo, ref_slot=D.ref_slot.ptr + 4 * lo, sf=_vp(MC.SCALE), nlev=MC.NLEV,
             mp_desc=out.mp_desc.ptr + 32, best=out.best.ptr + 4, med=out.med.ptr + 4, normal=out.normal.ptr + 12, mn=out.mn.ptr + 4, mx=out.mx.ptr + 4,
             up=out.up.ptr + 1, h=m.h)
    a.update(kw)
    rc1 = None if "d" not in which else L.orbm_distinctive_descriptors_batch_async(a["h"], a["nmp"], a["nrows"], a["cap"], a["desc"], a["counts"], a["nobs"], a["off"], a["row"], a["slot"],
                                                     a["flags"], a["valid"], a["mp_desc"], a["best"], a["med"])
    rc2 = None if "n" not in which else L.orbm_update_normal_and_depth_batch_async(a["h"], a["nmp"], a["nrows"], a["cap"], a["kps"], a["counts"], a["ow_l"], a["ow_r"], a["nobs"], a["off"],
                                                     a["row"], a["slot"], a["flags"], a["valid"], a["pw"], a["ref_row"], a["ref_slot"], a["sf"], a["nlev"],
                                                     a["normal"], a["mn"], a["mx"], a["up"])
    return rc1, rc2


@pytest.fixture(scope="module")
def S(pkg):
    P = MC.pool(); M = MC.mappoints(P)
    m = pkg.ORBmatcher(0.9)
    want = _expect(P, M)
    return dict(P=P, M=M, m=m, L=m.L, D=_Dev(pkg, P, M), want=want)


def test_fixture_holds_what_it_promises(S):
    """Ties, the value 256, every list size, the malformed lists and every gate occur in the inputs (no GPU work here)."""
    P, M, want = S["P"], S["M"], S["want"]
    assert 190 <= M["nmp"] <= 230 and len(M["row"]) < 6000 and M["off"][0] > 0
    assert set(MC.NS) - {-1} <= set(M["ns"].tolist())
    sp = M["special"]
    base = P["base"]
    assert R.descriptor_distance(base, P["desc"][MC.CROW, 42]) == 256
    assert (want["best"][sp["complement"]], want["med"][sp["complement"]]) == (1, 0)          # A, ~A, ~A: an 8-bit distance would answer 0
    assert (want["best"][sp["equal"]], want["med"][sp["equal"]]) == (0, 0)                    # a three-way tie
    assert (want["best"][sp["clusters"]], want["med"][sp["clusters"]]) == (2, 2)              # the earlier of two tied rows
    assert (want["best"][sp["lower_median"]], want["med"][sp["lower_median"]]) == (1, 10)
    assert (want["best"][sp["complement_pair"]], want["med"][sp["complement_pair"]]) == (0, 0)
    assert want["med"].max() > 100 and (want["best"] > 64).any()                              # a winner beyond the first chunk of 64 rows
    dec = M["dec"]
    assert M["off"][dec + 1] < M["off"][dec] and want["best"][dec] == -1 and want["up"][dec] == 0 and want["best"][dec + 1] >= 0
    assert all(want["up"][mp] == 0 for mp in M["gated"]) and all(want["best"][mp] >= 0 for mp in M["gated"])
    inval = np.flatnonzero(M["valid"] == 0)
    assert np.all(want["best"][inval] == -1) and np.all(want["up"][inval] == 0) and np.all(want["desc"][inval] == SENT_D)
    # 0 after skipping: bad KeyFrames give no descriptor but a normal; junk entries give neither
    no_desc = (want["best"] == -1) & (M["valid"] == 1)
    assert (no_desc & (want["up"] == 1)).any() and (no_desc & (want["up"] == 0)).sum() > 5
    # positions count skipped entries: some winner sits behind a skipped entry of its own list
    behind = 0
    for mp in np.flatnonzero(want["best"] > 0):
        e0 = M["off"][mp]
        behind += any((M["flags"][e] & MC.BAD_KF) or not R._in_pool(int(M["row"][e]), int(M["slot"][e]), P["counts"], MC.CAP) for e in range(e0, e0 + want["best"][mp]))
    assert behind > 5
    assert np.isfinite(want["normal"][want["up"] == 1]).all()
    assert (M["flags"] & MC.RIGHT).sum() > 100 and (M["flags"] & MC.BAD_KF).sum() > 30


def test_device_form_equals_second_reading(pkg, S):
    out = _Out(pkg, S["M"]["nmp"])
    assert _enqueue(S, out) == (0, 0), S["L"].orbm_last_error()
    S["m"].sync()
    got = out.fetch()
    print("MapPoints %d, entries %d: %d descriptors, %d normals" % (S["M"]["nmp"], len(S["M"]["row"]), (got["best"] >= 0).sum(), got["up"].sum()))
    _same(got, S["want"])
    # best_median is optional; valid == NULL means all valid
    out.reset()
    assert _enqueue(S, out, med=None, valid=False) == (0, 0)
    S["m"].sync()
    got = out.fetch()
    M2 = dict(S["M"], valid=np.ones(S["M"]["nmp"], np.uint8))
    _same(got, _expect(S["P"], M2), what=("desc", "best", "normal", "mn", "mx", "up"))
    assert np.all(got["med"] == SENT_I)


@pytest.mark.parametrize("nmp,lo", [(1, 17), (63, 2), (64, 40), (65, 101), (1, 19)])
def test_slices_of_the_call(pkg, S, nmp, lo):
    """nmp at the workgroup and wave edges; the offsets are absolute, so a slice of obs_off is a call of its own."""
    out = _Out(pkg, nmp)
    assert _enqueue(S, out, lo, lo + nmp) == (0, 0), S["L"].orbm_last_error()
    S["m"].sync()
    want = {k: v[lo:lo + nmp] for k, v in S["want"].items()}
    _same(out.fetch(), want)


def test_host_form_equals_second_reading(pkg, S):
    P, M, m = S["P"], S["M"], S["m"]
    n = M["nmp"]
    rc, d, b, md = m.ComputeDistinctiveDescriptors(P["desc"], P["counts"], M["off"], M["row"], M["slot"], M["flags"], M["valid"], np.full((n, 32), SENT_D, np.uint8))
    assert rc == (S["want"]["best"] >= 0).sum()
    rc2, nv, mn, mx, up = m.UpdateNormalAndDepth(P["kps"], P["counts"], P["ow_l"], P["ow_r"], M["off"], M["row"], M["slot"], M["flags"], M["valid"], M["pw"],
                                                 M["ref_row"], M["ref_slot"], MC.SCALE, np.full((n, 3), SENT_F, F), np.full(n, SENT_F, F), np.full(n, SENT_F, F))
    assert rc2 == S["want"]["up"].sum()
    _same(dict(desc=d, best=b, med=md, normal=nv, mn=mn, mx=mx, up=up), S["want"])
    # no right centres: the entries that name the right camera are skipped
    lo, hi = 20, 40
    off = M["off"][lo:hi + 1]
    got = m.UpdateNormalAndDepth(P["kps"], P["counts"], P["ow_l"], None, off, M["row"], M["slot"], M["flags"], None, M["pw"][lo:hi], M["ref_row"][lo:hi],
                                 M["ref_slot"][lo:hi], MC.SCALE)
    want = R.normal_depth_batch(P["kps"], P["counts"], P["ow_l"], None, off, M["row"], M["slot"], M["flags"], None, M["pw"][lo:hi], M["ref_row"][lo:hi],
                                M["ref_slot"][lo:hi], MC.SCALE, np.zeros((hi - lo, 3), F), np.zeros(hi - lo, F), np.zeros(hi - lo, F))
    assert np.array_equal(_bits(got[1]), _bits(want[0])) and np.array_equal(got[4], want[3]) and not np.array_equal(_bits(want[0]), _bits(S["want"]["normal"][lo:hi]))


def test_refused_arguments_enqueue_nothing(pkg, S):
    L = S["L"]
    out = _Out(pkg, S["M"]["nmp"])
    shared = [dict(counts=None), dict(off=None), dict(row=None), dict(slot=None), dict(flags=None), dict(nmp=0), dict(nmp=-1), dict(nrows=0), dict(cap=0),
              dict(nobs=-1), dict(h=None)]
    for kw in shared:
        assert _enqueue(S, out, **kw) == (-2, -2), kw
    for kw in (dict(desc=None), dict(mp_desc=None), dict(best=None)):
        assert _enqueue(S, out, which="d", **kw)[0] == -2, kw
    for kw in (dict(kps=None), dict(ow_l=None), dict(pw=None), dict(ref_row=None), dict(ref_slot=None), dict(sf=None), dict(normal=None), dict(mn=None),
               dict(mx=None), dict(up=None), dict(nlev=0), dict(nlev=-3)):
        assert _enqueue(S, out, which="n", **kw)[1] == -2, kw
    assert _enqueue(S, out, which="n", nlev=13)[1] == -3 and b"12" in L.orbm_last_error()
    assert _enqueue(S, out, nmp=(1 << 20) + 1) == (-3, -3)
    assert _enqueue(S, out, nrows=1 << 16, cap=1 << 16) == (-3, -3)
    S["m"].sync()
    assert out.untouched()                                                  # nothing was enqueued: every sentinel is intact
    P, M, m = S["P"], S["M"], S["m"]
    keep = np.full((M["nmp"], 32), SENT_D, np.uint8)
    bo = np.full(M["nmp"], SENT_I, np.int32)
    rc = L.orbm_distinctive_descriptors(m.h, M["nmp"], MC.NROWS, MC.CAP, _vp(P["desc"]), None, len(M["row"]), _vp(M["off"]), _vp(M["row"]), _vp(M["slot"]),
                                        _vp(M["flags"]), None, _vp(keep), _vp(bo), None)
    assert rc == -2 and np.all(keep == SENT_D) and np.all(bo == SENT_I)


def test_captured_replay_follows_new_contents(pkg, S, synth):
    """After one eager run both calls are captured behind an extraction (a step graph holds one); the descriptor pool, pw and ow_l are
    then rewritten and the graph replayed: the outputs follow the new contents, and a second replay is identical (nothing accumulates)."""
    L, M, D = S["L"], S["M"], S["D"]
    cw = ch = 239; stride = 256                                             # the smallest size the (1.2, 8) extractor accepts
    pad = np.zeros((ch, stride), np.uint8); pad[:, :cw] = synth.gen_image(cw, ch, 9100)
    dimg = pkg.DeviceBuffer(pad.nbytes).upload(pad)
    arr = (C.c_void_p * 1)(dimg.ptr)
    ex = pkg.ORBextractor(500, max_size=(cw, ch), max_batch=1)
    m = pkg.ORBmatcher(0.9)
    assert L.orbm_set_stream(m.h, L.orbx_stream(ex.h)) == 0
    S2 = dict(S, m=m)
    out = _Out(pkg, M["nmp"])
    ex.enqueue_device(arr, cw, ch, stride)
    assert _enqueue(S2, out) == (0, 0)
    ex.sync()
    _same(out.fetch(), S["want"])
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    ex.enqueue_device(arr, cw, ch, stride)
    assert _enqueue(S2, out) == (0, 0), L.orbm_last_error()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    rng = np.random.default_rng(77)
    P2 = dict(S["P"])
    P2["desc"] = S["P"]["desc"].copy(); P2["desc"][:MC.CROW] = rng.integers(0, 256, (MC.CROW, MC.CAP, 32)).astype(np.uint8)
    P2["ow_l"] = rng.uniform(-2, 2, (MC.NROWS, 3)).astype(F)
    M2 = dict(M, pw=rng.uniform(-5, 5, M["pw"].shape).astype(F))
    try:
        D.desc.upload(P2["desc"]); D.ow_l.upload(P2["ow_l"]); D.pw.upload(M2["pw"])
        want2 = _expect(P2, M2)
        assert not np.array_equal(want2["best"], S["want"]["best"]) and not np.array_equal(_bits(want2["normal"]), _bits(S["want"]["normal"]))
        got = []
        for _ in range(2):
            out.reset()
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            ex.sync()
            got.append(out.fetch())
            _same(got[-1], want2)
        _same(got[0], got[1])
    finally:
        D.desc.upload(S["P"]["desc"]); D.ow_l.upload(S["P"]["ow_l"]); D.pw.upload(M["pw"])


# ---------------------------------------------------------------------------------------------------------------------------
# the chain: mp_desc / normal / min_dist / max_dist go straight into orbm_is_in_frustum(ORBM_DEVICE) and the M3 batch
# ---------------------------------------------------------------------------------------------------------------------------
W, H = 640, 480
K = np.array([500.0, 500.0, 320.0, 240.0], F)
BOUNDS = np.array([0.0, W, 0.0, H], F)


def _chain_inputs(pkg):
    """One frame of 300 keypoints seen by an identity camera; MapPoint i sits on the ray of keypoint i and was observed by 2 to 9
    KeyFrames near the origin whose descriptors are the keypoint's with a few bits flipped."""
    rng = np.random.default_rng(41)
    nkp, fcap, nmp = 300, 320, 260
    kps = np.zeros((1, fcap), pkg.KP_DTYPE)
    kps["x"][0, :nkp] = rng.uniform(20, W - 20, nkp); kps["y"][0, :nkp] = rng.uniform(20, H - 20, nkp)
    kps["octave"][0, :nkp] = rng.integers(0, MC.NLEV, nkp); kps["angle"][0, :nkp] = rng.uniform(0, 360, nkp)
    fdesc = rng.integers(0, 256, (1, fcap, 32)).astype(np.uint8)
    nrows, cap = 10, 192                                                    # 1 920 slots for about 1 430 observations
    P = dict(desc=rng.integers(0, 256, (nrows, cap, 32)).astype(np.uint8), kps=np.zeros((nrows, cap), pkg.KP_DTYPE),
             counts=np.full(nrows, cap, np.int32), ow_l=rng.uniform(-0.2, 0.2, (nrows, 3)).astype(F), ow_r=None)
    z = rng.uniform(2, 8, nmp).astype(F)
    pw = np.stack([(kps["x"][0, :nmp] - K[2]) * z / K[0], (kps["y"][0, :nmp] - K[3]) * z / K[1], z], 1).astype(F)
    off, row, slot, nxt = [0], [], [], np.zeros(nrows, int)
    ref_row, ref_slot = [], []
    for i in range(nmp):
        n = int(rng.integers(2, 10))
        rows = rng.choice(nrows, n, replace=False)
        rows = rows[nxt[rows] < cap]
        for r in rows:
            s = nxt[r]; nxt[r] += 1
            P["desc"][r, s] = MC.flip(fdesc[0, i], rng.choice(256, rng.integers(0, 25), replace=False))
            P["kps"]["octave"][r, s] = kps["octave"][0, i]
            row.append(r); slot.append(s)
        off.append(len(row))
        ref_row.append(rows[0] if len(rows) else -1); ref_slot.append(nxt[rows[0]] - 1 if len(rows) else -1)
    M = dict(nmp=nmp, off=np.array(off, np.int32), row=np.array(row, np.int32), slot=np.array(slot, np.int32), flags=np.zeros(len(row), np.uint8),
             valid=np.ones(nmp, np.uint8), pw=pw, ref_row=np.array(ref_row, np.int32), ref_slot=np.array(ref_slot, np.int32))
    return kps, fdesc, np.array([nkp], np.int32), fcap, P, M


def test_chain_rows_feed_frustum_and_local_points_search(pkg):
    m = pkg.ORBmatcher(0.9); L = m.L
    kps, fdesc, fcount, fcap, P, M = _chain_inputs(pkg)
    nmp = M["nmp"]
    Pd = dict(P, ow_r=np.zeros_like(P["ow_l"]))
    S = dict(P=P, M=M, m=m, L=L, D=_Dev(pkg, Pd, M))
    d, b, md = R.distinctive_batch(P["desc"], P["counts"], M["off"], M["row"], M["slot"], M["flags"], None, np.zeros((nmp, 32), np.uint8))
    nv, mn, mx, up = R.normal_depth_batch(P["kps"], P["counts"], P["ow_l"], None, M["off"], M["row"], M["slot"], M["flags"], None, M["pw"], M["ref_row"],
                                          M["ref_slot"], MC.SCALE, np.zeros((nmp, 3), F), np.zeros(nmp, F), np.zeros(nmp, F))
    assert (b >= 0).sum() > 240 and up.sum() > 240
    up_ = lambda a: pkg.DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a))
    dk, dd, dc = up_(kps), up_(fdesc), up_(fcount)
    gs, gi = pkg.DeviceBuffer(3073 * 4), pkg.DeviceBuffer(fcap * 4)
    inv_w, inv_h = float(F(64) / F(W)), float(F(48) / F(H))
    assert L.orbm_grid_build_batch_async(m.h, dk.ptr, dc.ptr, 1, fcap, 0.0, 0.0, inv_w, inv_h, gs.ptr, gi.ptr) == 0
    Rcw = np.eye(3, dtype=F).reshape(9); tcw = np.zeros(3, F); Ow = np.zeros(3, F)
    lsf = float(np.log(F(1.2)))
    nq = up_(np.array([nmp], np.int32)); obs = up_(np.ones(nmp, np.uint8))

    def search(p_desc, p_normal, p_mn, p_mx):
        iv = pkg.DeviceBuffer(nmp); bufs = [pkg.DeviceBuffer(nmp * 4) for _ in range(6)]
        px, py, pxr, dep, lev, vc = bufs
        assert L.orbm_is_in_frustum(m.h, pkg.DEVICE, nmp, S["D"].pw.ptr, p_normal, p_mn, p_mx, _vp(Rcw), _vp(tcw), _vp(Ow), _vp(K), _vp(BOUNDS), 40.0, 0.5, lsf,
                                    MC.NLEV, iv.ptr, px.ptr, py.ptr, pxr.ptr, dep.ptr, lev.ptr, vc.ptr) == 0, L.orbm_last_error()
        match = pkg.DeviceBuffer(fcap * 4).upload(np.full(fcap, -5, np.int32)); nm = pkg.DeviceBuffer(4)
        rc = L.orbm_search_by_projection_points_batch_async(m.h, dk.ptr, dd.ptr, dc.ptr, fcap, gs.ptr, gi.ptr, 0.0, 0.0, inv_w, inv_h, 0, 1, None, None, nq.ptr, nmp,
                                                            iv.ptr, px.ptr, py.ptr, pxr.ptr, vc.ptr, lev.ptr, None, 0.0, p_desc, obs.ptr, 0, 3.0, 0.8,
                                                            _vp(MC.SCALE), MC.NLEV, match.ptr, nm.ptr)
        assert rc == 0, L.orbm_last_error()
        m.sync()
        return match.download(np.int32, fcap), int(nm.download(np.int32, 1)[0]), iv.download(np.uint8, nmp)

    out = _Out(pkg, nmp)
    out.mp_desc.upload(np.zeros((nmp + 2) * 32, np.uint8)); out.normal.upload(np.zeros((nmp + 2) * 3, F)); out.mn.upload(np.zeros(nmp + 2, F)); out.mx.upload(np.zeros(nmp + 2, F))
    assert _enqueue(S, out, ow_r=None, valid=False, nrows=P["desc"].shape[0], cap=P["desc"].shape[1]) == (0, 0), L.orbm_last_error()
    got = search(out.mp_desc.ptr + 32, out.normal.ptr + 12, out.mn.ptr + 4, out.mx.ptr + 4)       # the new calls' rows, never leaving the device
    rd, rn, rmn, rmx = up_(d), up_(nv), up_(mn), up_(mx)
    want = search(rd.ptr, rn.ptr, rmn.ptr, rmx.ptr)                                                # the second reading's rows
    print("chain: %d of %d MapPoints in view, %d matches" % (want[2].sum(), nmp, want[1]))
    assert want[2].sum() > 200 and want[1] > 150
    assert got[1] == want[1] and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


def test_cpp_facade_mappoint_refresh(pkg, tmp_path):
    """facade/MapPointRefresh.h's templates on mock MapPoint / KeyFrame types against plain C++ in the same file."""
    pkg.build()
    exe = str(tmp_path / "facade_mappoint_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "facade_mappoint_smoke.cpp"),
                           "-L", os.path.join(ROOT, "orb-slam3_amd"), "-lorbslam3_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "orb-slam3_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "need-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "facade_mappoint_smoke ok" in out.stdout, out.stdout + out.stderr
