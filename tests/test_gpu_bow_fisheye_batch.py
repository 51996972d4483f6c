"""Batched two-camera SearchByBoW(KeyFrame, Frame) -- M7 with F.Nleft != -1, Tracking::TrackReferenceKeyFrame and Relocalization on a
fisheye rig -- on the device (orbm_search_by_bow_fisheye_batch_async).  For every batch of tests/bow_fisheye_cases.py and every pair the
two match rows (the -1 padding included) and the count equal, entry for entry, (a) the second reading of
tests/second_reading_bow_fisheye.py, (b) the product's host entry point orbm_search_by_bow_fisheye and (c) the oracle's."""
import ctypes as C

import numpy as np
import pytest

import bow_fisheye_cases as bc
import second_reading_bow_fisheye as srb

pytestmark = pytest.mark.gpu

MAX_CAP_KF, MAX_CAP_F = 24576, 12288                                          # ORBM_BOW_MAX_CAP, ORBM_BOW_FISHEYE_MAX_CAP_F
POOL_KEYS = ("kps", "desc", "counts", "node", "weight")


class DevPool:
    """One pool of a Batch on the device."""

    def __init__(self, pkg, P):
        self.rows, self.cap = P["rows"], P["cap"]
        self.buf = {k: pkg.DeviceBuffer(P[k].nbytes).upload(np.ascontiguousarray(P[k])) for k in POOL_KEYS + (("good",) if "good" in P else ())}

    def ptr(self, k):
        return self.buf[k].ptr


_DEV = {}                                                                     # batch name -> its two pools on the device


def _pools(pkg, b):
    """The pools of a batch of bow_fisheye_cases.py (hand, scene_l1, scene_l2: with_params() shares the arrays under one name)."""
    if b.name not in _DEV:
        _DEV[b.name] = (DevPool(pkg, b.K), DevPool(pkg, b.F))
    return _DEV[b.name]


def _run(pkg, mt, b, K=None, Fp=None):
    """Enqueue batch b and download the two rows and the counts; the outputs are poisoned beforehand."""
    L = pkg.lib()
    if K is None:
        K, Fp = _pools(pkg, b)
    P, cap = b.npairs, Fp.cap
    rows = [pkg.DeviceBuffer(4 * P).upload(a) for a in (b.kf_row, b.fl_row, b.fr_row)]
    ml = pkg.DeviceBuffer(4 * P * cap).upload(np.full(P * cap, -7, np.int32)); mr = pkg.DeviceBuffer(4 * P * cap).upload(np.full(P * cap, -7, np.int32))
    nm = pkg.DeviceBuffer(4 * P).upload(np.full(P, -7, np.int32))
    rc = L.orbm_search_by_bow_fisheye_batch_async(mt.h, P, K.rows, K.cap, K.ptr("kps"), K.ptr("desc"), K.ptr("counts"), K.ptr("node"),
                                                  K.ptr("weight") if b.weights else None, K.ptr("good"),
                                                  Fp.rows, Fp.cap, Fp.ptr("kps"), Fp.ptr("desc"), Fp.ptr("counts"), Fp.ptr("node"),
                                                  Fp.ptr("weight") if b.weights else None,
                                                  rows[0].ptr, rows[1].ptr, rows[2].ptr, b.nnratio, b.check_ori, ml.ptr, mr.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()
    assert L.orbm_sync(mt.h) == 0, L.orbm_last_error()
    return ml.download(np.int32, P * cap).reshape(P, cap), mr.download(np.int32, P * cap).reshape(P, cap), nm.download(np.int32, P)


def _check(b, ml, mr, nm, mt, OM):
    """Every pair against the three comparators, each directly; returns the counts."""
    for p in range(b.npairs):
        a = bc.single_args(b, p)
        if a is None:
            assert nm[p] == 0 and np.all(ml[p] == -1) and np.all(mr[p] == -1), (b.names[p], "out of range")
            continue
        nl, nr = a[6], len(a[4]) - a[6]
        for what, (n, fm) in (("second reading", srb.search_by_bow_fisheye(*a)[:2]), ("host entry point", mt.SearchByBoWFisheye(*a)),
                              ("oracle", OM.SearchByBoWFisheye(*a))):
            assert int(nm[p]) == int(n), (b.name, b.names[p], what, int(nm[p]), int(n))
            assert np.array_equal(ml[p, :nl], fm[:nl]), (b.name, b.names[p], what, "left", np.flatnonzero(ml[p, :nl] != fm[:nl])[:8])
            assert np.array_equal(mr[p, :nr], fm[nl:]), (b.name, b.names[p], what, "right", np.flatnonzero(mr[p, :nr] != fm[nl:])[:8])
        assert np.all(ml[p, nl:] == -1) and np.all(mr[p, nr:] == -1), (b.name, b.names[p], "padding")
    return nm


@pytest.fixture(scope="module")
def env(pkg, oracle):
    mt = pkg.ORBmatcher(0.7)
    yield mt, oracle._oracle_matcher_class()()
    mt.close()


@pytest.mark.parametrize("nnratio,check_ori,weights", bc.HAND_PARAMS)
def test_hand_pairs(pkg, env, nnratio, check_ori, weights):
    mt, OM = env
    b = bc.hand(nnratio, check_ori, weights)
    ml, mr, nm = _run(pkg, mt, b)
    _check(b, ml, mr, nm, mt, OM)
    assert nm[b.names.index("th_50")] == 2 and nm[b.names.index("th_51")] == 0 and np.all(nm[-6:] == 0)


@pytest.mark.parametrize("levelsup,nnratio,check_ori,weights", bc.SCENE_PARAMS)
def test_scene_pairs(pkg, oracle, synth, env, levelsup, nnratio, check_ori, weights):
    mt, OM = env
    b = bc.scene(oracle, synth, levelsup, nnratio, check_ori, weights)
    ml, mr, nm = _run(pkg, mt, b)
    _check(b, ml, mr, nm, mt, OM)
    assert nm[:3].min() > 80 and nm[3] < nm[:3].min() // 4 and nm[5] == 0 and nm[6] == 0 and nm[8] == 0, nm


@pytest.mark.parametrize("which", ["hand", "scene"])
def test_empty_right_row_equals_one_camera_batch(pkg, oracle, synth, env, which):
    """Every pair with its right row replaced by an empty one: the left rows and the counts are those of orbm_search_by_bow_batch_async
    on (kf_row, fl_row), and the right rows are all -1."""
    mt, OM = env
    L = pkg.lib()
    b = bc.hand(0.7, 1) if which == "hand" else bc.scene(oracle, synth, 2, 0.75, 1)
    empty = 2 * b.names.index("empty_right") + 1 if which == "hand" else 6
    assert b.F["counts"][empty] == 0
    keep = [p for p in range(b.npairs) if b.in_range(p)]
    e = bc.Batch(b.name, b.K, b.F, b.kf_row[keep], b.fl_row[keep], np.full(len(keep), empty, np.int32), b.nnratio, b.check_ori,
                 True, [b.names[p] for p in keep])
    ml, mr, nm = _run(pkg, mt, e)
    _check(e, ml, mr, nm, mt, OM)
    K, Fp = _pools(pkg, b)
    P = e.npairs
    dk = pkg.DeviceBuffer(4 * P).upload(e.kf_row); df = pkg.DeviceBuffer(4 * P).upload(e.fl_row)
    fm = pkg.DeviceBuffer(4 * P * Fp.cap).upload(np.full(P * Fp.cap, -7, np.int32)); n1 = pkg.DeviceBuffer(4 * P).upload(np.full(P, -7, np.int32))
    rc = L.orbm_search_by_bow_batch_async(mt.h, P, K.rows, K.cap, K.ptr("kps"), K.ptr("desc"), K.ptr("counts"), K.ptr("node"), K.ptr("weight"), K.ptr("good"),
                                          Fp.rows, Fp.cap, Fp.ptr("kps"), Fp.ptr("desc"), Fp.ptr("counts"), Fp.ptr("node"), Fp.ptr("weight"),
                                          dk.ptr, df.ptr, e.nnratio, e.check_ori, fm.ptr, n1.ptr)
    assert rc == 0, L.orbm_last_error()
    mt.sync()
    assert np.array_equal(fm.download(np.int32, P * Fp.cap).reshape(P, Fp.cap), ml) and np.array_equal(n1.download(np.int32, P), nm)
    assert np.all(mr == -1) and nm.sum() > (5 if which == "hand" else 300)


def test_relocalization_shape(pkg, oracle, synth, env):
    """Relocalization: ONE (left, right) frame against nine KeyFrame rows -- its own, two other rigs', the same three with other MapPoint
    masks, the frame's own features stacked as a KeyFrame, its cameras in the other order, and an empty one; nnratio 0.75."""
    mt, OM = env
    s = bc.scene(oracle, synth, 1, 0.75, 1)
    rng = np.random.default_rng(8)

    def kf(r, good=None):
        c = int(s.K["counts"][r])
        return tuple(s.K[k][r, :c] for k in ("kps", "desc", "node", "weight")) + (s.K["good"][r, :c] if good is None else good(c),)

    def stacked(rows):
        c = [int(s.F["counts"][r]) for r in rows]
        return tuple(np.concatenate([s.F[k][r, :n] for r, n in zip(rows, c)]) for k in ("kps", "desc", "node", "weight")) + (np.ones(sum(c), np.uint8),)
    rows = [kf(0), kf(1), kf(2)] + [kf(r, lambda c: (rng.random(c) < 0.5).astype(np.uint8)) for r in (0, 1, 2)] + [stacked((1, 4)), stacked((4, 1)), kf(3)]
    K9 = bc.make_pool(rows, max(len(r[0]) for r in rows) + 1, True)
    b = bc.Batch("reloc", K9, s.F, list(range(9)), [1] * 9, [4] * 9, 0.75, 1)
    ml, mr, nm = _run(pkg, mt, b)
    _check(b, ml, mr, nm, mt, OM)
    assert nm[1] > 100 and min(nm[6], nm[7]) > 300 and max(nm[0], nm[2]) < nm[1] // 4 and nm[4] < nm[1] and nm[8] == 0, nm


@pytest.fixture(scope="module")
def chain(pkg, oracle, synth):
    """The scene's frame images (three rigs: rows 0-2 left, 3-5 right, 6 flat) through the product extractor in one batch; the matcher and
    the vocabulary on the extractor's stream; the scene's stacked KeyFrame pool on the device."""
    _, f_imgs = bc.scene_images(synth)
    imgs = [p[0] for p in f_imgs] + [p[1] for p in f_imgs] + [np.full((bc.H, bc.W), 128, np.uint8)]
    n = len(imgs)
    stride = (bc.W + 63) // 64 * 64
    dimg = pkg.DeviceBuffer(n * stride * bc.H)
    for i, im in enumerate(imgs):
        pad = np.zeros((bc.H, stride), np.uint8); pad[:, :bc.W] = im
        dimg.upload(pad, offset=i * stride * bc.H)
    arr = (C.c_void_p * n)(*[dimg.ptr + i * stride * bc.H for i in range(n)])
    L = pkg.lib()
    ex = pkg.ORBextractor(bc.NF, 1.2, 8, 20, 7, max_size=(bc.W, bc.H), max_batch=n)
    mt = pkg.ORBmatcher(0.7)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    voc = pkg.ORBVocabulary(mt, bc.scene_tree(synth))
    yield dict(ex=ex, mt=mt, L=L, voc=voc, arr=arr, stride=stride, n=n, OM=oracle._oracle_matcher_class()(), keep=dimg)
    ex.close(); mt.close()


def test_chain_and_capture_replay(pkg, oracle, synth, chain):
    """On one handle and one stream: extraction (two rows per rig) -> orbm_bow_transform_batch_async over the result block -> the search.
    The eager result equals the three comparators on the downloaded block; the captured step replayed equals the eager result; two more
    replays on changed inputs (another good_kf mask, then other pair rows) equal fresh eager calls on those inputs, so nothing
    accumulates across replays."""
    D = chain
    ex, mt, L, n = D["ex"], D["mt"], D["L"], D["n"]
    s = bc.scene(oracle, synth, 1, 0.7, 1)
    K = DevPool(pkg, s.K)
    cap = ex.cap
    node = pkg.DeviceBuffer(4 * n * cap); weight = pkg.DeviceBuffer(8 * n * cap)
    kf_row = np.array([0, 1, 2, 1, 2, 0, 3], np.int32); fl_row = np.array([0, 1, 2, 1, 6, 5, 0], np.int32); fr_row = np.array([3, 4, 5, 6, 5, 2, 3], np.int32)
    P = len(kf_row)
    rows = [pkg.DeviceBuffer(4 * P).upload(a) for a in (kf_row, fl_row, fr_row)]
    ml = pkg.DeviceBuffer(4 * P * cap); mr = pkg.DeviceBuffer(4 * P * cap); nm = pkg.DeviceBuffer(4 * P)
    lap = np.zeros(2 * n, np.int32)

    def enqueue():
        ex.enqueue_device(D["arr"], bc.W, bc.H, D["stride"], lap)
        r = ex.result_device()
        assert L.orbm_bow_transform_batch_async(mt.h, D["voc"].h, r["desc"], n * cap, 1, None, node.ptr, weight.ptr) == 0, L.orbm_last_error()
        assert L.orbm_search_by_bow_fisheye_batch_async(mt.h, P, K.rows, K.cap, K.ptr("kps"), K.ptr("desc"), K.ptr("counts"), K.ptr("node"), K.ptr("weight"),
                                                        K.ptr("good"), n, cap, r["kps"], r["desc"], r["counts"], node.ptr, weight.ptr,
                                                        rows[0].ptr, rows[1].ptr, rows[2].ptr, 0.7, 1, ml.ptr, mr.ptr, nm.ptr) == 0, L.orbm_last_error()

    def poison():
        ml.upload(np.full(P * cap, -7, np.int32)); mr.upload(np.full(P * cap, -7, np.int32)); nm.upload(np.full(P, -7, np.int32))

    def results():
        return ml.download(np.int32, P * cap).reshape(P, cap), mr.download(np.int32, P * cap).reshape(P, cap), nm.download(np.int32, P)

    poison(); enqueue(); ex.sync()
    eager = results()
    # the block as a Batch for the comparators: keypoints and descriptors as fetched, node ids and weights as the device transform left them
    res = ex.fetch_all()
    h_node = node.download(np.int32, n * cap).reshape(n, cap); h_weight = weight.download(np.float64, n * cap).reshape(n, cap)
    frows = [(np.ascontiguousarray(k).view(bc.KP_DTYPE).reshape(-1), np.ascontiguousarray(dsc, np.uint8).reshape(-1, 32), h_node[i, :len(k)], h_weight[i, :len(k)])
             for i, (_, k, dsc) in enumerate(res)]
    assert len(frows[6][0]) == 0 and min(len(r[0]) for r in frows[:6]) > 200
    b = bc.Batch("chain", s.K, bc.make_pool(frows, cap, False), kf_row, fl_row, fr_row, 0.7, 1)
    _check(b, eager[0], eager[1], eager[2], mt, D["OM"])
    assert eager[2][:3].min() > 80 and eager[2][6] == 0, eager[2]

    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    poison()
    assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
    ex.sync()
    for got, want in zip(results(), eager):
        assert np.array_equal(got, want)
    rng = np.random.default_rng(3)
    changes = [lambda: K.buf["good"].upload((rng.random(s.K["good"].shape) < 0.4).astype(np.uint8)),
               lambda: (rows[0].upload(kf_row[::-1].copy()), rows[2].upload(np.roll(fr_row, 1)))]
    last = eager
    for change in changes:
        change()
        poison()
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        replay = results()
        poison(); enqueue(); ex.sync()
        fresh = results()
        for got, want in zip(replay, fresh):
            assert np.array_equal(got, want)
        assert not np.array_equal(fresh[2], last[2])                          # the changed inputs do change the counts
        last = fresh
    assert L.orbm_set_stream(mt.h, None) == 0


def test_capacity_limit(pkg, oracle, synth, env):
    """cap_kf = 24576 and cap_f = 12288 per camera (the largest LDS shape, 157 864 bytes) with sparse counts: accepted and exact; a
    smaller call afterwards still launches."""
    mt, OM = env
    s = bc.scene(oracle, synth, 1, 0.7, 1)

    def relaid(P, rows, cap):
        c = [int(P["counts"][r]) for r in rows]
        return bc.make_pool([tuple(P[k][r, :n] for k in ("kps", "desc", "node", "weight") + (("good",) if "good" in P else ())) for r, n in zip(rows, c)],
                            cap, "good" in P)
    b = bc.Batch("capacity", relaid(s.K, [0, 3], MAX_CAP_KF), relaid(s.F, [0, 3, 6], MAX_CAP_F), [0, 0, 1, 0], [0, 1, 0, 2], [1, 0, 1, 1], 0.7, 1)
    ml, mr, nm = _run(pkg, mt, b)
    _check(b, ml, mr, nm, mt, OM)
    assert ml.shape == (4, MAX_CAP_F) and nm[0] > 80 and nm[2] == 0 and nm[3] == 0
    h = bc.hand(0.7, 1)
    _check(h, *_run(pkg, mt, h), mt, OM)


def test_refusals_enqueue_nothing(pkg):
    """Each refusal code with the documented reason on a live handle; the outputs keep their sentinel."""
    m = pkg.ORBmatcher()
    L = m.L
    buf = pkg.DeviceBuffer(1 << 16)
    p = buf.ptr
    fm = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))
    o = fm.ptr

    def call(npairs=1, nkr=1, capk=4, nfr=1, capf=4, nn=0.7, node_kf=p, good=p, fl=p, fr=p, out_r=o):
        return L.orbm_search_by_bow_fisheye_batch_async(m.h, npairs, nkr, capk, p, p, p, node_kf, None, good, nfr, capf, p, p, p, p, None,
                                                        None, fl, fr, nn, 1, o, out_r, o)
    assert call(node_kf=None) == -2 and call(good=None) == -2 and call(fl=None) == -2 and call(fr=None) == -2 and call(out_r=None) == -2
    assert call(npairs=0) == -2 and call(nkr=0) == -2 and call(nfr=0) == -2 and call(capk=0) == -2 and call(capf=0) == -2
    assert call(nn=float("nan")) == -2 and call(nn=float("inf")) == -2
    assert call(capk=MAX_CAP_KF + 1) == -3 and b"24576" in L.orbm_last_error()
    assert call(capf=MAX_CAP_F + 1) == -3 and b"12288" in L.orbm_last_error()
    assert call(npairs=65536) == -3
    m.sync()
    assert np.all(fm.download(np.int32, 16) == 12345)
    m.close()
