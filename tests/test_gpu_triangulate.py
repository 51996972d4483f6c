"""CreateNewMapPoints behind M10 on the device (orbm_triangulate_new_points / orbm_triangulate_new_points_batch_async).  The device form,
the host form (both spaces) and the g++ build of csrc/orbm_triangulate.h (tests/triangulate_header.cpp) give the same bits for every
output, x3d included; the header's answer is held to the second reading by the rule of tests/test_triangulate_header_cpu.py (flags,
winners, counts and order exact with no match excluded, unprojected points bit for bit, x3D_h within C eps32 s1 / (s3 - s4)).  Shapes:
the committed scenes, row counts 1 .. 300 at cap1 320 as eight groups of one call, groups of 1, 3 and 64 pairs, two groups over one
aliased pool; garbage match entries and rows out of range; every refusal; {M10, triangulate} captured on a 376 x 240 extractor block
and replayed under new poses and new matches; the C++ facade."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_reading_triangulate as sr   # noqa: E402
import triangulate_cases as tc            # noqa: E402
import triangulate_io as io               # noqa: E402
import triangulate_results as res         # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_CAPACITY = -2, -3
NAME = "orbm_triangulate_new_points_batch_async"


@pytest.fixture(scope="module")
def m(pkg):
    mt = pkg.ORBmatcher(0.6)
    yield mt
    mt.close()


@pytest.fixture(scope="module")
def header_exe(tmp_path_factory):
    return io.build_program(tmp_path_factory.mktemp("triangulate_gpu"))


def _up(pkg, a, t=None):
    a = np.ascontiguousarray(a, t)
    return pkg.DeviceBuffer(max(a.nbytes, 4)).upload(a)


class DevPool:
    def __init__(self, pkg, p):
        self.rows, self.cap = p["kps_un"].shape
        self.b = {k: _up(pkg, p[k]) for k in ("kps_un", "kps", "counts", "uright", "depth", "tcw", "ow") if p.get(k) is not None}

    def args(self):
        g = lambda k: self.b[k].ptr if k in self.b else None
        return (self.rows, self.cap, g("kps_un"), g("kps"), g("counts"), g("uright"), g("depth"), g("tcw"), g("ow"))


class Outs:
    """Device outputs, poisoned: every slot of every row is written by every call."""
    KEYS = (("won_pair", np.int32, 1), ("won_idx2", np.int32, 1), ("x3d", np.float32, 3), ("order", np.int32, 1))

    def __init__(self, pkg, ng, npairs, cap1):
        self.ng, self.npairs, self.cap1 = ng, npairs, cap1
        self.b = {k: _up(pkg, np.full(ng * cap1 * w, -77, t)) for k, t, w in self.KEYS}
        self.b["reason"] = _up(pkg, np.full(npairs * cap1, 0xCD, np.uint8))
        self.b["ncreated"] = _up(pkg, np.full(npairs, -77, np.int32)); self.b["ntotal"] = _up(pkg, np.full(ng, -77, np.int32))

    def ptrs(self):
        return tuple(self.b[k].ptr for k in ("won_pair", "won_idx2", "x3d", "reason", "ncreated", "order", "ntotal"))

    def fetch(self):
        ng, npairs, cap1 = self.ng, self.npairs, self.cap1
        return {"won_pair": self.b["won_pair"].download(np.int32, ng * cap1).reshape(ng, cap1),
                "won_idx2": self.b["won_idx2"].download(np.int32, ng * cap1).reshape(ng, cap1),
                "x3d": self.b["x3d"].download(np.float32, ng * cap1 * 3).reshape(ng, cap1, 3),
                "reason": self.b["reason"].download(np.uint8, npairs * cap1).reshape(npairs, cap1),
                "ncreated": self.b["ncreated"].download(np.int32, npairs), "order": self.b["order"].download(np.int32, ng * cap1).reshape(ng, cap1),
                "ntotal": self.b["ntotal"].download(np.int32, ng)}


def run_device(pkg, m, c):
    p1 = DevPool(pkg, c["pool1"]); p2 = p1 if c["pool2"] is c["pool1"] else DevPool(pkg, c["pool2"])
    npairs, cap1 = c["matches12"].shape; ng = len(c["group_start"]) - 1
    d1, d2, dm = _up(pkg, c["row1"], np.int32), _up(pkg, c["row2"], np.int32), _up(pkg, c["matches12"], np.int32)
    o = Outs(pkg, ng, npairs, cap1)
    m.TriangulateNewPointsBatchAsync(c["group_start"], npairs, p1.args(), p2.args(), d1.ptr, d2.ptr, dm.ptr, c["k1"], c["k2"], c["mb1"], c["mbf1"], c["mb2"],
                                     c["sf1"], c["ls1"], c["sf2"], c["ls2"], c["ratio_factor"], c["th_far"], *o.ptrs())
    m.sync()
    return o.fetch()


def run_host(m, c):
    return m.TriangulateNewPoints(c["group_start"], c["pool1"], c["pool2"], c["row1"], c["row2"], c["matches12"], c["k1"], c["k2"], c["mb1"], c["mbf1"],
                                  c["mb2"], c["sf1"], c["ls1"], c["sf2"], c["ls2"], c["ratio_factor"], c["th_far"])


def same(a, b, who):
    for k in io.OUT_KEYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (who, k)


def all_forms(pkg, m, exe, tmp, c, tag, r=None):
    h = io.run_program(exe, c, tmp, tag)
    d = run_device(pkg, m, c)
    same(d, h, "device vs header"); same(run_host(m, c), h, "host vs header")
    r = r or sr.read_case(c)
    worst = res.check_against_reading(c, r, h, "header", xh=h["xh"])
    res.check_against_reading(c, r, d, "device")
    print("%s: %s MapPoints, largest x3D_h distance / bound %.3f" % (tag, list(d["ntotal"]), worst))
    return d, r


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_device_host_header_and_reading(pkg, m, header_exe, tmp_path, name):
    d, r = all_forms(pkg, m, header_exe, tmp_path, res.cases()[name], name, res.reading(name))
    assert d["ntotal"].sum() >= 15


def test_row_counts_around_the_wave_and_the_workgroup(pkg, m, header_exe, tmp_path):
    """Row counts 1, 63, 64, 65, 255, 256, 257 and 300 at cap1 320: eight groups of three pairs in one call."""
    c = res.cases()["row_counts"]
    assert tuple(c["pool1"]["counts"][:8]) == tc.ROW_COUNTS and c["matches12"].shape == (24, 320)
    d, r = all_forms(pkg, m, header_exe, tmp_path, c, "row_counts", res.reading("row_counts"))
    assert np.all(d["ntotal"][1:] >= 20)
    assert {sr.OK_TRI, sr.OK_ST1, sr.OK_ST2, sr.TAKEN, sr.BEHIND_1, sr.BEHIND_2, sr.CHI2_1, sr.CHI2_2, sr.SCALE, sr.LOW_PARALLAX, sr.BAD_OCTAVE} <= set(np.unique(r["reason"]))


@pytest.mark.parametrize("name", ["one_pair", "pairs_64"])
def test_groups_of_1_and_64_pairs(pkg, m, header_exe, tmp_path, name):
    c = res.cases()[name]
    assert len(c["row1"]) == (1 if name == "one_pair" else 64)
    d, r = all_forms(pkg, m, header_exe, tmp_path, c, name, res.reading(name))
    if name == "pairs_64":
        assert np.count_nonzero(d["ncreated"]) >= 5 and np.any(d["won_pair"] >= 32)      # late pairs create points too


def test_two_groups_over_one_aliased_pool_and_the_device_space(pkg, m, header_exe, tmp_path):
    """Pool 1 and pool 2 are the same arrays; the host form with ORBM_DEVICE arrays equals the async form."""
    c = res.cases()["two_groups_one_pool"]
    assert c["pool2"] is c["pool1"] and len(c["group_start"]) == 3
    d = run_device(pkg, m, c)
    L = pkg.lib()
    p = DevPool(pkg, c["pool1"])
    npairs, cap1 = c["matches12"].shape
    d1, d2, dm = _up(pkg, c["row1"], np.int32), _up(pkg, c["row2"], np.int32), _up(pkg, c["matches12"], np.int32)
    o = Outs(pkg, 2, npairs, cap1)
    f = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.c_void_p)
    gs = np.ascontiguousarray(c["group_start"], np.int32)
    rc = L.orbm_triangulate_new_points(m.h, pkg.DEVICE, 2, gs.ctypes.data_as(C.c_void_p), npairs, *p.args(), *p.args(), d1.ptr, d2.ptr, dm.ptr, f(c["k1"]), f(c["k2"]),
                                       float(c["mb1"]), float(c["mbf1"]), float(c["mb2"]), f(c["sf1"]), f(c["ls1"]), f(c["sf2"]), f(c["ls2"]), len(c["sf1"]),
                                       float(c["ratio_factor"]), float(c["th_far"]), *o.ptrs())
    assert rc == 0, L.orbm_last_error()
    same(o.fetch(), d, "ORBM_DEVICE space vs async")


def test_garbage_matches_rows_out_of_range_and_null_optionals(pkg, m, header_exe, tmp_path):
    c = dict(res.cases()["mono_3"])
    mm = c["matches12"].copy(); n2 = int(c["pool2"]["counts"][1]); cap2 = c["pool2"]["kps_un"].shape[1]
    mm[1, :6] = [-2, -(2 ** 31), 2 ** 31 - 1, n2, cap2, 10 ** 6]
    c["matches12"] = mm; c["row2"] = c["row2"].copy(); c["row2"][2] = 99
    d, _ = all_forms(pkg, m, header_exe, tmp_path, c, "garbage")
    assert np.all(d["reason"][1, :6] == sr.NO_MATCH) and np.all(d["reason"][2] == sr.NO_MATCH) and d["ncreated"][2] == 0
    c["row1"] = np.full(3, -1, np.int32)                                     # the group's current KeyFrame is out of range: nothing is created
    d, _ = all_forms(pkg, m, header_exe, tmp_path, c, "row1_out")
    assert d["ntotal"][0] == 0 and np.all(d["won_pair"] == -1) and np.all(d["order"] == -1) and np.all(d["reason"] == sr.NO_MATCH)
    # uright / depth / kps NULL: every feature mono, UnprojectStereo_ never runs; equals the same case with explicit -1 rows
    c = dict(res.cases()["stereo1_2"])
    mono = {k: dict(c[k], uright=None, depth=None, kps=None) for k in ("pool1", "pool2")}
    expl = {k: dict(c[k], uright=np.full_like(c[k]["uright"], -1), depth=np.full_like(c[k]["depth"], -1)) for k in ("pool1", "pool2")}
    same(run_device(pkg, m, dict(c, **mono)), run_device(pkg, m, dict(c, **expl)), "NULL optionals")
    # a group of mixed row1 creates nothing on the device and is refused where row1 is readable
    c = dict(res.cases()["mono_3"]); c["row1"] = np.array([0, 0, 1], np.int32)
    c["pool1"] = {k: (np.concatenate([v, v]) if isinstance(v, np.ndarray) else v) for k, v in c["pool1"].items()}
    d = run_device(pkg, m, c)
    assert d["ntotal"][0] == 0 and np.all(d["reason"] == sr.MIXED) and np.all(d["won_pair"] == -1)
    same(d, io.run_program(header_exe, c, tmp_path, "mixed"), "mixed row1")
    with pytest.raises(pkg.OrbError):
        run_host(m, c)


def test_refusals_enqueue_nothing(pkg, m):
    L = pkg.lib()
    c = res.cases()["mono_2"]
    p1, p2 = DevPool(pkg, c["pool1"]), DevPool(pkg, c["pool2"])
    npairs, cap1 = c["matches12"].shape
    d1, d2, dm = _up(pkg, c["row1"], np.int32), _up(pkg, c["row2"], np.int32), _up(pkg, c["matches12"], np.int32)
    o = Outs(pkg, 1, npairs, cap1)
    before = o.fetch()
    f = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.c_void_p)
    keep = []

    def call(ngroups=1, gs=(0, 2), npairs_=npairs, a=None, b=None, nlevels=8, ratio=float(c["ratio_factor"]), null=(), space=None):
        g = np.ascontiguousarray(gs, np.int32); keep.append(g)
        a = list(a or p1.args()); b = list(b or p2.args())
        args = [ngroups, g.ctypes.data_as(C.c_void_p), npairs_, *a, *b, d1.ptr, d2.ptr, dm.ptr, f(c["k1"]), f(c["k2"]), float(c["mb1"]), float(c["mbf1"]),
                float(c["mb2"]), f(c["sf1"]), f(c["ls1"]), f(c["sf2"]), f(c["ls2"]), nlevels, ratio, 0.0, *o.ptrs()]
        for i in null:
            args[i] = None
        if space is not None:
            return L.orbm_triangulate_new_points(m.h, space, *args)
        return getattr(L, NAME)(m.h, *args)

    assert call() == 0
    m.sync()
    good = o.fetch()
    o2 = Outs(pkg, 1, npairs, cap1); o.b = o2.b                               # fresh poison for the refused calls
    # required arrays: group_start, kps_un1, counts1, tcw1, ow1, kps_un2, counts2, tcw2, ow2, row1, row2, matches12, k1, k2, the four tables, six outputs
    required = [1, 5, 7, 10, 11, 14, 16, 19, 20, 21, 22, 23, 24, 25, 29, 30, 31, 32, 36, 37, 38, 40, 41, 42]
    for i in required:
        assert call(null=(i,)) == E_INVALID, i
    for i in (6, 8, 9, 15, 17, 18, 39):                                       # kps, uright, depth of both pools and reason may be NULL
        assert call(null=(i,)) == 0, i
    m.sync()
    o3 = Outs(pkg, 1, npairs, cap1); o.b = o3.b
    a = list(p1.args())
    for kw in (dict(ngroups=0), dict(npairs_=0), dict(nlevels=0), dict(a=[0] + a[1:]), dict(a=[a[0], 0] + a[2:]), dict(gs=(1, 2)), dict(gs=(0, 1)),
               dict(ngroups=2, gs=(0, 3, 2)), dict(ngroups=2, gs=(0, -1, 2)), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(space=7)):
        assert call(**kw) == E_INVALID, kw
    for kw in (dict(a=[a[0], 65536] + a[2:]), dict(b=[p2.args()[0], 65536] + list(p2.args()[2:])), dict(npairs_=65536, gs=(0, 65536)), dict(nlevels=33),
               dict(npairs_=65, gs=(0, 65))):
        assert call(**kw) == E_CAPACITY, kw
    assert b"at most" in L.orbm_last_error()
    m.sync()
    after = o.fetch()
    for k in io.OUT_KEYS:
        assert after[k].tobytes() == before[k].tobytes(), k                  # the poison stands: nothing was enqueued
    assert good["ntotal"][0] == res.reading("mono_2")["ntotal"][0]


def test_captured_with_m10_and_replayed(pkg, synth, header_exe, tmp_path):
    """Extractor block (376 x 240) -> BoW -> M10 -> triangulate, captured once; has_mp1 (so matches12) and the poses are rewritten and the
    graph replayed: every output equals a fresh eager run into other buffers, the first state gives the first bits again (nothing
    accumulates), and an eager state equals the g++ build of the header on the fetched rows."""
    from test_triangulation_batch_rule_cpu import fundamental
    L = pkg.lib()
    W, H, NF, P = 376, 240, 600, 3
    Kc = (217.6, 217.6, 183.6, 126.1)
    base = [0.11 * (1 + i / 10.0) for i in range(P)]
    imgs = [synth.gen_stereo_pair(W, H, 100)[0]] + [synth.gen_stereo_pair(W, H, 100, dmin=2 + i, dmax=30 + 2 * i)[1] for i in range(P)]
    stride = (W + 63) // 64 * 64
    dev = pkg.DeviceBuffer((P + 1) * stride * H)
    for i, im in enumerate(imgs):
        pad = np.zeros((H, stride), np.uint8); pad[:, :W] = im
        dev.upload(pad, offset=i * stride * H)
    arr = (C.c_void_p * (P + 1))(*[dev.ptr + i * stride * H for i in range(P + 1)])
    ex = pkg.ORBextractor(NF, max_size=(W, H), max_batch=P + 1)
    mt = pkg.ORBmatcher(0.6)
    voc = pkg.ORBVocabulary(mt, synth.gen_vocabulary(10, 3, seed=7))
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    cap, rows = ex.cap, P + 1
    lap = np.zeros(4 * rows, np.int32)
    sf = ex.GetScaleFactors(); sig = ex.GetScaleSigmaSquares(); nl = ex.GetLevels()
    k6 = np.array([Kc[0], Kc[1], Kc[2], Kc[3], np.float32(1) / np.float32(Kc[0]), np.float32(1) / np.float32(Kc[1])], np.float32)
    F = np.stack([fundamental(Kc, Kc, np.eye(3), (b, 0, 0)) for b in base]); ep = np.array([[1e4, Kc[3]]] * P, np.float32)
    node = pkg.DeviceBuffer(4 * rows * cap); weight = pkg.DeviceBuffer(8 * rows * cap)
    rng = np.random.default_rng(4)

    def state(share, scale):
        mp = np.zeros((rows, cap), np.uint8); mp[0] = rng.random(cap) < share
        tcw = np.zeros((rows, 12), np.float32); ow = np.zeros((rows, 3), np.float32)
        tcw[:, [0, 5, 10]] = 1
        for i, b in enumerate(base):
            tcw[1 + i, 3] = -b * scale; ow[1 + i, 0] = b * scale
        return mp, tcw, ow
    states = [state(0.0, 1.0), state(0.4, 1.0), state(0.2, 2.0)]
    dmp, dtcw, dow = _up(pkg, states[0][0]), _up(pkg, states[0][1]), _up(pkg, states[0][2])
    d1, d2 = _up(pkg, np.zeros(P, np.int32)), _up(pkg, np.arange(1, P + 1, dtype=np.int32))
    dF, de = _up(pkg, F), _up(pkg, ep)
    gs = np.array([0, P], np.int32)
    fp = lambda a: a.ctypes.data_as(C.c_void_p)

    class Run:
        def __init__(self):
            self.mm = pkg.DeviceBuffer(4 * P * cap); self.nm = pkg.DeviceBuffer(4 * P); self.o = Outs(pkg, 1, P, cap)

        def enqueue(self):
            ex.enqueue_device(arr, W, H, stride, lap)
            r = ex.result_device()
            assert L.orbm_bow_transform_batch_async(mt.h, voc.h, r["desc"], rows * cap, 2, None, node.ptr, weight.ptr) == 0, L.orbm_last_error()
            side = (rows, cap, r["kps"], r["desc"], r["counts"], node.ptr, weight.ptr, dmp.ptr, None)
            assert L.orbm_search_for_triangulation_batch_async(mt.h, P, *side, *side, d1.ptr, d2.ptr, dF.ptr, de.ptr, fp(sf), fp(sig), nl, 0, 0, 0,
                                                               self.mm.ptr, self.nm.ptr) == 0, L.orbm_last_error()
            pool = (rows, cap, r["kps"], None, r["counts"], None, None, dtcw.ptr, dow.ptr)
            mt.TriangulateNewPointsBatchAsync(gs, P, pool, pool, d1.ptr, d2.ptr, self.mm.ptr, k6, k6, 0.11, 0.11 * Kc[0], 0.11, sf, sig, sf, sig,
                                              1.5 * float(sf[1]), 0.0, *self.o.ptrs())

        def fetch(self):
            ex.sync()
            return dict(self.o.fetch(), matches12=self.mm.download(np.int32, P * cap).reshape(P, cap))

    def upload(s):
        dmp.upload(s[0]); dtcw.upload(s[1]); dow.upload(s[2])
    try:
        A, B = Run(), Run()
        want = []
        for s in states:                                                     # the eager runs, ahead of the capture
            upload(s)
            B.enqueue()
            want.append(B.fetch())
        assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
        A.enqueue()
        assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
        for i in (0, 1, 2, 0, 0):
            upload(states[i])
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            got = A.fetch()
            for k, w in want[i].items():
                assert got[k].tobytes() == w.tobytes(), (i, k)
        # the states differ where they should, and the device equals the header and the reading on the fetched rows
        assert want[0]["ntotal"][0] >= 20 and want[1]["ntotal"][0] < want[0]["ntotal"][0]
        assert not np.array_equal(want[0]["matches12"], want[1]["matches12"]) and want[2]["x3d"].tobytes() != want[0]["x3d"].tobytes()
        upload(states[2]); B.enqueue(); ex.sync()
        fetched = ex.fetch_all()
        kp = np.zeros((rows, cap), pkg.KP_DTYPE); counts = np.zeros(rows, np.int32)
        for i in range(rows):
            n = len(fetched[i][1]); kp[i, :n] = fetched[i][1]; counts[i] = n
        pool = {"kps_un": kp, "kps": None, "counts": counts, "uright": None, "depth": None, "tcw": states[2][1], "ow": states[2][2]}
        c = {"pool1": pool, "pool2": pool, "group_start": gs, "row1": np.zeros(P, np.int32), "row2": np.arange(1, P + 1, dtype=np.int32),
             "matches12": want[2]["matches12"], "k1": k6, "k2": k6, "mb1": np.float32(0.11), "mbf1": np.float32(0.11 * Kc[0]), "mb2": np.float32(0.11),
             "sf1": sf, "ls1": sig, "sf2": sf, "ls2": sig, "ratio_factor": np.float32(1.5 * float(sf[1])), "th_far": np.float32(0)}
        h = io.run_program(header_exe, c, tmp_path, "chain")
        same(want[2], h, "chain vs header")
        res.check_against_reading(c, sr.read_case(c), h, "header", xh=h["xh"])
    finally:
        assert L.orbm_set_stream(mt.h, None) == 0
        ex.close(); mt.close()


def test_cpp_facade_create_new_map_points(pkg, tmp_path):
    """facade/CreateNewMapPoints.h on mock KeyFrame types: the flattened calls give the points of the array form, in the reference's order."""
    pkg.build()
    exe = str(tmp_path / "facade_triangulate_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "facade_triangulate_smoke.cpp"),
                           "-L", os.path.join(ROOT, "orb-slam3_amd"), "-lorbslam3_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "orb-slam3_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "need-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "facade_triangulate_smoke ok" in out.stdout, out.stdout + out.stderr
