"""Batched Frame::isInFrustum on the device (orbm_is_in_frustum_batch_async, k_frustum_batch): one launch for all frames of a call, poses,
counts and skip flags read from device rows, the query rows of the batched SearchLocalPoints search (M3) written in place.  Checked against
the second reading of the reference (tests/second_reading_frame.py) on the constructed cases of tests/frame_cases.py, bit for bit against
the single-frame form orbm_is_in_frustum(ORBM_DEVICE), and inside a captured {extraction -> grid -> frustum -> M3} step that is replayed
under new poses.
Every output buffer starts from sentinels and carries guard entries on both sides of its rows."""
import ctypes as C

import numpy as np
import pytest

import frame_cases as fc
from test_gpu_frame_second_reading import _KEYS, _device_form
from test_gpu_local_points_batch import EUROC_K, H, INV_H, INV_W, MBF, NLEV, W, _Rows, _call, _pose, batch  # noqa: F401  (batch: the extractor fixture)
from test_second_reading_frame_cpu import check_frustum_expectations, compare_frustum

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_CAPACITY = -2, -3
G = 4                                                                        # guard entries on either side of every output buffer
SENT_N = -4321                                                               # n_in_view before the call
# random_scene(2000, seed) per frame of the reading comparison: the reading alone marks 0 of 2000 levels ambiguous on each (checked on the CPU)
BIG_SEEDS = (2100, 2101, 2102)


@pytest.fixture(scope="module")
def m(pkg):
    return pkg.ORBmatcher(0.7)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _up(pkg, a):
    a = np.ascontiguousarray(a)
    return pkg.DeviceBuffer(max(a.nbytes, 4)).upload(a)


class _Out:
    """The seven output rows [nframes][qs] and n_in_view [nframes] on the device, filled with sentinels, G guard entries on either side."""

    def __init__(self, pkg, nframes, qs):
        self.nframes, self.qs = nframes, qs
        self.bufs = {key: _up(pkg, np.full(nframes * qs + 2 * G, v, dt)) for key, dt, v in _KEYS}
        self.cnt = _up(pkg, np.full(nframes + 2 * G, SENT_N, np.int32))

    def reset(self):
        for key, dt, v in _KEYS:
            self.bufs[key].upload(np.full(self.nframes * self.qs + 2 * G, v, dt))
        self.cnt.upload(np.full(self.nframes + 2 * G, SENT_N, np.int32))

    def ptr(self, key):
        return self.bufs[key].ptr + G * np.dtype(dict((k, dt) for k, dt, _ in _KEYS)[key]).itemsize

    def ptrs(self):
        return [self.ptr(key) for key, _, _ in _KEYS]

    def cnt_ptr(self):
        return self.cnt.ptr + 4 * G

    def rows(self, what):
        """Downloads; the guards must hold their sentinels.  Returns {key: [nframes][qs]}, n_in_view [nframes]."""
        out = {}
        for key, dt, v in _KEYS:
            a = self.bufs[key].download(dt, self.nframes * self.qs + 2 * G)
            assert np.all(a[:G] == v) and np.all(a[-G:] == v), (what, key, "an entry outside the rows was written")
            out[key] = a[G:-G].reshape(self.nframes, self.qs)
        c = self.cnt.download(np.int32, self.nframes + 2 * G)
        assert np.all(c[:G] == SENT_N) and np.all(c[-G:] == SENT_N), (what, "n_in_view: an entry outside the row was written")
        return out, c[G:-G]


class _In:
    """The input rows of one call: per frame pose rows, nq, and the MapPoint rows ([nframes][qs], or one row when shared) padded with zeros."""

    def __init__(self, pkg, cases, nqs, qs, shared=False, skip=None):
        nf = len(cases)
        self.nframes, self.qs, self.shared = nf, qs, shared
        self.tcw = _up(pkg, np.stack([self.pose_row(c.scene)[0] for c in cases]))
        self.ow = _up(pkg, np.stack([self.pose_row(c.scene)[1] for c in cases]))
        self.nq = _up(pkg, np.asarray(nqs, np.int32))
        nrows = 1 if shared else nf
        pw = np.zeros((nrows, qs, 3), F); nm = np.zeros((nrows, qs, 3), F); mn = np.zeros((nrows, qs), F); mx = np.zeros((nrows, qs), F)
        for f in range(nrows):
            s = cases[f].scene
            k = min(len(s["pw"]), qs)
            pw[f, :k] = s["pw"][:k]; nm[f, :k] = s["normal"][:k]; mn[f, :k] = s["min_dist"][:k]; mx[f, :k] = s["max_dist"][:k]
        self.pw, self.nm, self.mn, self.mx = _up(pkg, pw), _up(pkg, nm), _up(pkg, mn), _up(pkg, mx)
        self.skip = None if skip is None else _up(pkg, np.asarray(skip, np.uint8).reshape(nf, qs))

    @staticmethod
    def pose_row(scene):
        """tcw[12] = row-major 3x4 [Rcw | tcw], ow[3]: the layout the header documents."""
        R = np.asarray(scene["rcw"], F).reshape(3, 3); t = np.asarray(scene["tcw"], F).reshape(3, 1)
        return np.concatenate([R, t], 1).reshape(12), np.asarray(scene["ow"], F).reshape(3)


def _run(pkg, m, cases, nqs, qs, shared=False, skip=None, count=True, what=""):
    """One call on fresh sentinel-filled outputs; every frame uses cases[0]'s camera and gate parameters."""
    c0 = cases[0]
    i = _In(pkg, cases, nqs, qs, shared, skip)
    o = _Out(pkg, len(cases), qs)
    rc = m.L.orbm_is_in_frustum_batch_async(m.h, len(cases), i.tcw.ptr, i.ow.ptr, i.nq.ptr, qs, None if i.skip is None else i.skip.ptr,
                                            i.pw.ptr, i.nm.ptr, i.mn.ptr, i.mx.ptr, int(shared), _vp(np.ascontiguousarray(c0.k, F)),
                                            _vp(np.ascontiguousarray(c0.bounds, F)), float(c0.bf), float(c0.cos_limit), float(c0.lsf), int(c0.nlevels),
                                            *o.ptrs(), o.cnt_ptr() if count else None)
    assert rc == 0, m.L.orbm_last_error()
    m.sync()
    rows, cnt = o.rows(what)
    if not count:
        assert np.all(cnt == SENT_N)
    return rows, cnt


def _sentinel_rows(nframes, qs):
    return {key: np.full((nframes, qs), v, dt) for key, dt, v in _KEYS}


def _expected(cases, nqs, qs, skip=None):
    """The second reading's rows under the call's contract.  Entry i of frame f with n = min(max(nq, 0), qs):
         i >= n or skip[f][i]   in_view = 0, the six other fields keep the sentinel
         otherwise              what the reading writes, the fields it leaves alone keeping the sentinel (init)
    Returns (rows {key: [nframes][qs]}, ambiguous [nframes][qs], n_in_view [nframes], the readings' branch counters per frame)."""
    nf = len(cases)
    want = _sentinel_rows(nf, qs); amb = np.zeros((nf, qs), bool); cnt = np.zeros(nf, np.int32); ts = []
    want["in_view"][:] = 0
    for f, c in enumerate(cases):
        n = min(max(int(nqs[f]), 0), qs)
        out, a, t = c.reading(n, init={key: np.full(n, v, dt) for key, dt, v in _KEYS})
        ts.append(t)
        live = np.ones(n, bool) if skip is None else (np.asarray(skip).reshape(nf, qs)[f, :n] == 0)
        for key in want:
            want[key][f, :n][live] = out[key][live]
        amb[f, :n] = a & live
        cnt[f] = int(out["in_view"][live].sum())
    return want, amb, cnt, ts


def _same_params(case, scene, name):
    return fc.FrustumCase(name, scene, k=case.k, bounds=case.bounds, bf=case.bf, cos_limit=case.cos_limit, lsf=case.lsf, nlevels=case.nlevels)


def _single_rows(pkg, m, cases, nqs, qs):
    """orbm_is_in_frustum(ORBM_DEVICE) per frame on sentinel rows, laid out as the batch lays them out (tail: in_view = 0)."""
    rows = _sentinel_rows(len(cases), qs)
    rows["in_view"][:] = 0
    for f, c in enumerate(cases):
        n = min(max(int(nqs[f]), 0), qs)
        if n:
            one = _device_form(pkg, m, c, n)
            for key in rows:
                rows[key][f, :n] = one[key]
    return rows


def _assert_rows_equal(what, got, want):
    for key, _, _ in _KEYS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.tobytes() == b.tobytes(), (what, key, np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))[:6])


@pytest.mark.parametrize("name", fc.FRUSTUM_NAMES)
def test_constructed_case_between_two_random_frames(pkg, m, name):
    """The constructed case as frame 1 of three; frames 0 (a full row) and 2 are random scenes under other poses.  All seven rows of all
    three frames equal the second reading and, level of ambiguous points included, the single-frame form."""
    case = fc.frustum_case(name)
    n = len(case.scene["pw"])
    qs = n + 3
    cases = [_same_params(case, fc.random_scene(qs, 31), "random before " + name), case,
             _same_params(case, fc.random_scene(max(1, n // 2), 32), "random after " + name)]
    nqs = [qs, n, max(1, n // 2)]
    got, cnt = _run(pkg, m, cases, nqs, qs, what=name)
    want, amb, wcnt, ts = _expected(cases, nqs, qs)
    for f in range(3):
        compare_frustum("%s, frame %d" % (name, f), {k: v[f] for k, v in got.items()}, {k: v[f] for k, v in want.items()}, amb[f])
    assert np.array_equal(cnt, wcnt)
    check_frustum_expectations(case, {k: v[1, :n] for k, v in got.items()}, amb[1, :n], ts[1])
    _assert_rows_equal(name + " against the single-frame form", got, _single_rows(pkg, m, cases, nqs, qs))


def test_equals_the_single_frame_form_bit_for_bit(pkg, m):
    """Five frames of 700 random points each under five poses, per-frame rows and then one shared row: every row equals
    orbm_is_in_frustum(ORBM_DEVICE) called once per frame, the level of every point included (both forms run one device function)."""
    n, qs = 700, 701
    scenes = [fc.random_scene(n, 500 + f) for f in range(5)]
    cases = [fc.FrustumCase("random %d" % f, s) for f, s in enumerate(scenes)]
    got, cnt = _run(pkg, m, cases, [n] * 5, qs, what="per-frame rows")
    single = _single_rows(pkg, m, cases, [n] * 5, qs)
    _assert_rows_equal("per-frame rows", got, single)
    assert np.array_equal(cnt, single["in_view"].sum(1)) and cnt.min() > 50
    shared = [fc.FrustumCase("shared %d" % f, dict(scenes[0], rcw=s["rcw"], tcw=s["tcw"], ow=s["ow"])) for f, s in enumerate(scenes)]
    got, cnt = _run(pkg, m, shared, [n] * 5, qs, shared=True, what="shared row")
    single = _single_rows(pkg, m, shared, [n] * 5, qs)
    _assert_rows_equal("shared row", got, single)
    assert np.array_equal(cnt, single["in_view"].sum(1))


@pytest.mark.parametrize("shared", (0, 1))
@pytest.mark.parametrize("nqs", (fc.POINT_COUNTS, (0, 300, 257, 1)))
def test_shapes_tail_and_clamp(pkg, m, nqs, shared):
    """q_stride = 260 (two point blocks, the second partly dead); counts on either side of a workgroup; an empty frame; a count above
    q_stride, which is clamped.  Tail entries: in_view = 0 and the sentinel in the other six rows."""
    qs = 260
    assert fc.POINT_COUNTS == (1, 255, 256, 257)
    scenes = [fc.random_scene(qs, 700 + f) for f in range(4)]
    if shared:
        scenes = [dict(scenes[0], rcw=s["rcw"], tcw=s["tcw"], ow=s["ow"]) for s in scenes]
    cases = [fc.FrustumCase("shape %d" % f, s) for f, s in enumerate(scenes)]
    got, cnt = _run(pkg, m, cases, nqs, qs, shared=bool(shared), what="shapes")
    want, amb, wcnt, _ = _expected(cases, nqs, qs)
    for f in range(4):
        n = min(max(nqs[f], 0), qs)
        compare_frustum("shapes, frame %d" % f, {k: v[f] for k, v in got.items()}, {k: v[f] for k, v in want.items()}, amb[f])
        assert np.all(got["in_view"][f, n:] == 0)
        for key, dt, v in _KEYS:
            if key != "in_view":
                assert np.all(got[key][f, n:] == v), (f, key)
    assert np.array_equal(cnt, wcnt)
    assert wcnt[nqs.index(257)] > 20 and (0 not in nqs or cnt[nqs.index(0)] == 0)


def test_skip_rows_and_the_count(pkg, m):
    """A third of the entries skipped at random: in_view = 0 and six sentinels there, the others as without a skip row; n_in_view counts
    the reading's in-view points among the entries not skipped; n_in_view = NULL is accepted and changes no row."""
    n, qs = 500, 503
    cases = [fc.FrustumCase("skip %d" % f, fc.random_scene(n, 900 + f)) for f in range(3)]
    nqs = [n, n - 7, n]
    skip = (np.random.default_rng(12).random((3, qs)) < 1 / 3).astype(np.uint8)
    plain, pcnt = _run(pkg, m, cases, nqs, qs, what="no skip row")
    got, cnt = _run(pkg, m, cases, nqs, qs, skip=skip, what="skip row")
    want, amb, wcnt, _ = _expected(cases, nqs, qs, skip=skip)
    for f in range(3):
        compare_frustum("skip, frame %d" % f, {k: v[f] for k, v in got.items()}, {k: v[f] for k, v in want.items()}, amb[f])
        s = skip[f] != 0
        assert np.all(got["in_view"][f][s] == 0)
        for key, dt, v in _KEYS:
            if key != "in_view":
                assert np.all(got[key][f][s] == v), (f, key)
            assert got[key][f][~s].tobytes() == plain[key][f][~s].tobytes(), (f, key)
        assert cnt[f] == got["in_view"][f].sum() == wcnt[f]
    assert np.all(wcnt > 20) and np.all(wcnt < pcnt)
    again, none = _run(pkg, m, cases, nqs, qs, skip=skip, count=False, what="n_in_view = NULL")
    _assert_rows_equal("n_in_view = NULL", again, got)


def test_reading_on_2000_random_points_per_frame(pkg, m):
    """random_scene(2000, seed) per frame: everything equals the second reading except, at most, the level of points the reading marks
    ambiguous -- at most 0.001 of the points, the share tests/test_second_reading_frame_cpu.py asserts for this generator."""
    n, qs = fc.BIG, fc.BIG + 1
    cases = [fc.FrustumCase("random %d" % s, fc.random_scene(n, s)) for s in BIG_SEEDS]
    got, cnt = _run(pkg, m, cases, [n] * len(cases), qs, what="2000 points")
    want, amb, wcnt, _ = _expected(cases, [n] * len(cases), qs)
    for f in range(len(cases)):
        assert amb[f].sum() <= 0.001 * n, (BIG_SEEDS[f], amb[f].sum())
        compare_frustum("2000 points, frame %d" % f, {k: v[f] for k, v in got.items()}, {k: v[f] for k, v in want.items()}, amb[f])
    assert np.array_equal(cnt, wcnt) and wcnt.min() > 0.1 * n


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


def test_capture_and_replay_follow_new_poses(pkg, synth, batch):
    """{extraction -> grid -> frustum batch -> M3 batch} captured once on the extractor block (the graph slot wants an extraction in it;
    the images are the fixture's, now on the device), frames 0..2 searched, then replayed under poses, counts and skip rows uploaded
    between the launches.  After every replay the frustum rows and n_in_view equal eager single-frame calls under the same poses (the
    skip and tail rules applied to them), and M3's rows equal an eager M3 fed with those rows; the first state again gives the first
    result, so the count starts from zero on every replay."""
    B = batch
    L, ex, sf, NB = B["L"], B["ex"], B["sf"], B["NB"]
    imgs = [synth.gen_image(W, H, 40 * B["seed"] + i) for i in range(NB)]
    imgs[3] = np.full((H, W), 128, np.uint8)
    stride = (W + 63) // 64 * 64
    dimg = pkg.DeviceBuffer(NB * stride * H)
    for i, im in enumerate(imgs):
        pad = np.zeros((H, stride), np.uint8); pad[:, :W] = im
        dimg.upload(pad, offset=i * stride * H)
    arr = (C.c_void_p * NB)(*[dimg.ptr + i * stride * H for i in range(NB)])
    lap = np.array([(0, 1000)] * NB, np.int32)
    mt = pkg.ORBmatcher(0.9)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    ex.enqueue_device(arr, W, H, stride, lap)
    ex.sync()
    res = ex.fetch_all()
    assert all(np.array_equal(res[i][1], B["res"][i][1]) for i in range(NB))  # the block the fixture extracted
    r = ex.result_device(); cap = r["cap"]
    gs = pkg.DeviceBuffer(NB * 3073 * 4); gi = pkg.DeviceBuffer(NB * cap * 4)

    def grid():
        assert L.orbm_grid_build_batch_async(mt.h, r["kps"], r["counts"], NB, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0, L.orbm_last_error()

    grid()
    rng = np.random.default_rng(B["seed"] + 77)
    NF = 3
    fx, fy, cx, cy = EUROC_K
    maps = []
    for f in range(NF):                                                      # the local maps of test_frustum_chain: the frame's keypoints at two depths
        k, d = res[f][1], res[f][2]
        n = len(k)
        z = np.concatenate([rng.uniform(1.0, 4.0, n), rng.uniform(4.0, 14.0, n)]).astype(F)
        u = np.concatenate([k["x"], k["x"]]); v = np.concatenate([k["y"], k["y"]]); octv = np.concatenate([k["octave"], k["octave"]])
        Pw = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1).astype(F)
        dist = np.linalg.norm(Pw, axis=1).astype(F)
        mx = (dist * sf[octv]).astype(F)
        maps.append(dict(pw=Pw, normal=(Pw / dist[:, None]).astype(F), min_dist=(mx / sf[NLEV - 1]).astype(F), max_dist=mx,
                         qdesc=np.concatenate([d, d]), mp_obs=(rng.random(2 * n) < 0.9).astype(np.uint8)))
    nmax = [len(mp["pw"]) for mp in maps]
    qs = max(nmax) + 3
    bounds = np.array([0.0, W, 0.0, H], F)
    lsf = float(np.log(F(1.2)))

    def state(i):
        poses = [_pose(rng) for _ in range(NF)]
        nqs = list(nmax) if i == 0 else [int(rng.integers(n // 2, n)) for n in nmax]
        skip = np.zeros((NF, qs), np.uint8) if i == 0 else (rng.random((NF, qs)) < 0.3).astype(np.uint8)
        cases = [fc.FrustumCase("state %d frame %d" % (i, f), dict(maps[f], rcw=R.reshape(9), tcw=t, ow=Ow), k=EUROC_K, bounds=bounds, bf=MBF,
                                cos_limit=0.5, lsf=lsf, nlevels=NLEV) for f, (R, t, Ow) in enumerate(poses)]
        return dict(cases=cases, nqs=nqs, skip=skip)

    states = [state(i) for i in range(4)]
    inp = _In(pkg, states[0]["cases"], states[0]["nqs"], qs, skip=states[0]["skip"])
    out = _Out(pkg, NF, qs)
    # M3's view of the rows: the frustum's outputs in place, descriptors and observation flags per frame
    rows = _Rows(pkg, NF, qs)
    rows.upload([dict(px=np.zeros(len(mp["pw"]), F), qdesc=mp["qdesc"], mp_obs=mp["mp_obs"]) for mp in maps])
    ref = _Rows(pkg, NF, qs)
    ref.upload([dict(px=np.zeros(len(mp["pw"]), F), qdesc=mp["qdesc"], mp_obs=mp["mp_obs"]) for mp in maps])
    rows.nq = inp.nq
    for attr, key in (("in_view", "in_view"), ("px", "proj_x"), ("py", "proj_y"), ("pxr", "proj_xr"), ("view_cos", "view_cos"),
                      ("level", "level"), ("depth", "depth")):
        setattr(rows, attr, _At(out.ptr(key)))
    dm = pkg.DeviceBuffer(NF * cap * 4); dn = pkg.DeviceBuffer(NF * 4)
    dm_ref = pkg.DeviceBuffer(NF * cap * 4); dn_ref = pkg.DeviceBuffer(NF * 4)
    th, th_far = 3.0, 9.0

    def enqueue():
        ex.enqueue_device(arr, W, H, stride, lap)
        grid()
        rc = L.orbm_is_in_frustum_batch_async(mt.h, NF, inp.tcw.ptr, inp.ow.ptr, inp.nq.ptr, qs, inp.skip.ptr, inp.pw.ptr, inp.nm.ptr, inp.mn.ptr,
                                              inp.mx.ptr, 0, _vp(EUROC_K), _vp(bounds), MBF, 0.5, lsf, NLEV, *out.ptrs(), out.cnt_ptr())
        assert rc == 0, L.orbm_last_error()
        assert _call(L, mt, r, cap, gs, gi, 0, rows, sf, th, 0.8, dm, dn, depth=True, th_far=th_far) == 0, L.orbm_last_error()

    def eager(s):
        """Single-frame calls under the state's poses, its skip and tail rules applied; then an eager M3 on those rows."""
        want = _single_rows(pkg, mt, s["cases"], s["nqs"], qs)
        for f in range(NF):
            sk = s["skip"][f] != 0
            sk[s["nqs"][f]:] = False
            want["in_view"][f][sk] = 0
            for key, dt, v in _KEYS:
                if key != "in_view":
                    want[key][f][sk] = v
        ref.nq.upload(np.asarray(s["nqs"], np.int32))
        for attr, key in (("in_view", "in_view"), ("px", "proj_x"), ("py", "proj_y"), ("pxr", "proj_xr"), ("view_cos", "view_cos"),
                          ("level", "level"), ("depth", "depth")):
            getattr(ref, attr).upload(want[key])
        assert _call(L, mt, r, cap, gs, gi, 0, ref, sf, th, 0.8, dm_ref, dn_ref, depth=True, th_far=th_far) == 0, L.orbm_last_error()
        mt.sync()
        return want, dm_ref.download(np.int32, NF * cap), dn_ref.download(np.int32, NF)

    want = [eager(s) for s in states]                                        # also M3's one eager run ahead of the capture
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    first = None
    for i in (0, 1, 2, 3, 0):
        s = states[i]
        out.reset()
        dm.upload(np.full(NF * cap, -7, np.int32)); dn.upload(np.full(NF, -7, np.int32))
        inp.tcw.upload(np.stack([_In.pose_row(c.scene)[0] for c in s["cases"]])); inp.ow.upload(np.stack([_In.pose_row(c.scene)[1] for c in s["cases"]]))
        inp.nq.upload(np.asarray(s["nqs"], np.int32)); inp.skip.upload(s["skip"])
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        got, cnt = out.rows("replay under state %d" % i)
        w_rows, w_match, w_nm = want[i]
        _assert_rows_equal("replay under state %d" % i, got, w_rows)
        assert np.array_equal(cnt, w_rows["in_view"].sum(1)), (i, cnt)
        match, nm = dm.download(np.int32, NF * cap), dn.download(np.int32, NF)
        assert np.array_equal(match, w_match) and np.array_equal(nm, w_nm), i
        assert cnt.min() > 100 and nm.sum() > 100
        if first is None:
            first = (got, cnt, match, nm)
    _assert_rows_equal("the first state again", got, first[0])
    assert np.array_equal(cnt, first[1]) and np.array_equal(match, first[2]) and np.array_equal(nm, first[3])
    assert not np.array_equal(want[1][0]["proj_x"], want[0][0]["proj_x"])     # the states do differ
    mt.close()


def test_refusals_enqueue_nothing(pkg, m):
    """Every ORBM_E_INVALID / ORBM_E_CAPACITY case: the documented code, the argument named, and sentinel-filled outputs unchanged."""
    L = m.L
    qs = 8
    case = fc.FrustumCase("refused", fc.random_scene(qs, 5))
    inp = _In(pkg, [case, case], [qs, qs], qs, skip=np.zeros((2, qs), np.uint8))
    out = _Out(pkg, 2, qs)
    k, b = np.ascontiguousarray(case.k, F), np.ascontiguousarray(case.bounds, F)
    names = ["nframes", "tcw", "ow", "nq", "q_stride", "skip", "pw", "normal", "min_dist", "max_dist", "q_shared", "k_host", "bounds_host", "bf",
             "viewing_cos_limit", "log_scale_factor", "n_scale_levels", "in_view", "proj_x", "proj_y", "proj_xr", "depth", "level", "view_cos", "n_in_view"]

    def call(**kw):
        a = dict(zip(names, [2, inp.tcw.ptr, inp.ow.ptr, inp.nq.ptr, qs, inp.skip.ptr, inp.pw.ptr, inp.nm.ptr, inp.mn.ptr, inp.mx.ptr, 0, _vp(k), _vp(b),
                             float(case.bf), 0.5, float(case.lsf), 8] + out.ptrs() + [out.cnt_ptr()]))
        a.update(kw)
        return L.orbm_is_in_frustum_batch_async(m.h, *[a[n] for n in names])

    required =[n for n in names if n not in ("skip", "n_in_view", "nframes", "q_stride", "q_shared", "bf", "viewing_cos_limit", "log_scale_factor", "n_scale_levels")]
    for name in required:
        assert call(**{name: None}) == E_INVALID, name
        assert name.encode() in L.orbm_last_error(), (name, L.orbm_last_error())
    for name, bad in (("nframes", 0), ("nframes", -1), ("q_stride", 0), ("n_scale_levels", 0), ("viewing_cos_limit", float("nan")),
                      ("viewing_cos_limit", float("inf")), ("log_scale_factor", float("nan")), ("log_scale_factor", float("-inf"))):
        assert call(**{name: bad}) == E_INVALID, (name, bad)
        assert name.encode() in L.orbm_last_error(), (name, L.orbm_last_error())
    for name, bad in (("nframes", 65536), ("q_stride", (1 << 20) + 1)):
        assert call(**{name: bad}) == E_CAPACITY, (name, bad)
        assert name.encode() in L.orbm_last_error(), (name, L.orbm_last_error())
    m.sync()
    rows, cnt = out.rows("refused calls")
    for key, dt, v in _KEYS:
        assert np.all(rows[key] == v), key
    assert np.all(cnt == SENT_N)
    assert call() == 0, L.orbm_last_error()                                  # the same arguments, none of them bad, do run
    m.sync()
    rows, cnt = out.rows("accepted call")
    assert np.all(rows["in_view"] <= 1) and np.all(cnt >= 0)
