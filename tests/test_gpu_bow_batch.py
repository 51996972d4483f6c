"""M7 SearchByBoW(KeyFrame, Frame) batched on the device (orbm_search_by_bow_batch_async) and the device vocabulary transform that feeds
it (orbm_bow_transform_batch_async).  Frames and KeyFrames come from orbx_extract_batch_async on device images; node ids and weights
from the new transform call.  Every pair's row and count must equal the host entry point orbm_search_by_bow AND the oracle's
SearchByBoW, both given FeatureVectors built as DBoW2 builds them (weight > 0)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 752, 480
MAX_CAP = 24576                           # ORBM_BOW_MAX_CAP
NKF_IMG, NF_IMG = 16, 8                   # KeyFrame pool: 16 left images + a black one; frame pool: 8 right images, 2 unrelated, a black one


def _fv(nodes, keep):
    """FeatureVector CSR of DBoW2 (std::map<node, vector<idx>>) over the features with keep set: nodes ascending, indices ascending."""
    idx = np.flatnonzero(keep).astype(np.int32)
    order = idx[np.argsort(nodes[idx], kind="stable")]
    un, start = np.unique(nodes[order], return_index=True)
    return un.astype(np.int32), np.append(start, len(order)).astype(np.int32), order.astype(np.int32)


def _upload_images(pkg, imgs):
    stride = (W + 63) // 64 * 64
    dev = pkg.DeviceBuffer(len(imgs) * stride * H)
    for i, im in enumerate(imgs):
        pad = np.zeros((H, stride), np.uint8); pad[:, :W] = im
        dev.upload(pad, offset=i * stride * H)
    arr = (C.c_void_p * len(imgs))(*[dev.ptr + i * stride * H for i in range(len(imgs))])
    return dev, arr, stride


class Pool:
    """Rows of one extractor result block, with node ids / words / weights from orbm_bow_transform_batch_async."""

    def __init__(self, pkg, mt, imgs, nfeatures):
        self.L = pkg.lib()
        self.ex = pkg.ORBextractor(nfeatures, max_size=(W, H), max_batch=len(imgs))
        self.dev, self.arr, self.stride = _upload_images(pkg, imgs)
        self.ex.enqueue_device(self.arr, W, H, self.stride, np.zeros(4 * len(imgs), np.int32))
        self.ex.sync()
        self.r = self.ex.result_device()
        self.cap, self.rows = self.ex.cap, len(imgs)
        self.res = self.ex.fetch_all()
        n = self.rows * self.cap
        self.word, self.node, self.weight = pkg.DeviceBuffer(4 * n), pkg.DeviceBuffer(4 * n), pkg.DeviceBuffer(8 * n)
        self.mt = mt

    def transform(self, voc, levelsup):
        n = self.rows * self.cap
        rc = self.L.orbm_bow_transform_batch_async(self.mt.h, voc.h, self.r["desc"], n, levelsup, self.word.ptr, self.node.ptr, self.weight.ptr)
        assert rc == 0, self.L.orbm_last_error()
        self.mt.sync()
        self.h_node = self.node.download(np.int32, n).reshape(self.rows, self.cap)
        self.h_weight = self.weight.download(np.float64, n).reshape(self.rows, self.cap)
        self.h_word = self.word.download(np.int32, n).reshape(self.rows, self.cap)
        for r in range(self.rows):                                          # the node ids and weights the search reads, pinned by the oracle
            nr = len(self.kps(r))
            if nr:
                _, _, w, nd, wt = voc.oracle.transform(self.desc(r), levelsup)
                assert np.array_equal(self.h_word[r, :nr], w) and np.array_equal(self.h_node[r, :nr], nd), r
                assert self.h_weight[r, :nr].tobytes() == wt.tobytes(), r

    def kps(self, r):
        return self.res[r][1]

    def desc(self, r):
        return self.res[r][2]


@pytest.fixture(scope="module")
def pools(pkg, synth):
    pairs = [synth.gen_stereo_pair(W, H, 900 + i) for i in range(NKF_IMG)]
    black = np.zeros((H, W), np.uint8)
    kf_imgs = [p[0] for p in pairs] + [black]
    f_imgs = [pairs[i][1] for i in range(NF_IMG)] + [synth.gen_image(W, H, 77), synth.gen_image(W, H, 78), black]
    mt = pkg.ORBmatcher(0.7)
    K = Pool(pkg, mt, kf_imgs, 1500)                                        # more features: cap_kf != cap_f
    F = Pool(pkg, mt, f_imgs, 1000)
    assert K.cap != F.cap and len(K.res[-1][1]) == 0 and len(F.res[-1][1]) == 0
    yield mt, K, F
    K.ex.close(); F.ex.close()


_VOCABS = {}


def _vocab(pkg, synth, mt, k, L, stop_frac=0.0, seed=7):
    key = (id(mt), k, L, stop_frac, seed)
    if key not in _VOCABS:
        _VOCABS[key] = _make_vocab(pkg, synth, mt, k, L, stop_frac, seed)
    return _VOCABS[key]


def _make_vocab(pkg, synth, mt, k, L, stop_frac, seed):
    tree = synth.gen_vocabulary(k, L, seed=seed)
    if stop_frac:
        rng = np.random.default_rng(seed)
        leaves = np.flatnonzero(tree["is_leaf"])
        tree["weight"][rng.choice(leaves, int(len(leaves) * stop_frac), replace=False)] = 0.0
    import orbref
    voc = pkg.ORBVocabulary(mt, tree)
    voc.oracle = orbref.Vocabulary(tree)                                    # the oracle's DBoW2 restatement of the same tree
    return voc


def _run(pkg, mt, K, F, kf_row, f_row, good, nnratio, check_ori, weights=True, kf_pool=None):
    """Enqueue the batch for the pairs (kf_row, f_row) and download rows and counts."""
    L = pkg.lib()
    kp = kf_pool or K
    P = len(kf_row)
    dk = pkg.DeviceBuffer(4 * P).upload(np.asarray(kf_row, np.int32)); df = pkg.DeviceBuffer(4 * P).upload(np.asarray(f_row, np.int32))
    dg = pkg.DeviceBuffer(good.nbytes).upload(good)
    fm = pkg.DeviceBuffer(4 * P * F.cap).upload(np.full(P * F.cap, -7, np.int32)); nm = pkg.DeviceBuffer(4 * P).upload(np.full(P, -7, np.int32))
    rc = L.orbm_search_by_bow_batch_async(mt.h, P, kp.rows, kp.cap, kp.r["kps"], kp.r["desc"], kp.r["counts"], kp.node.ptr,
                                          kp.weight.ptr if weights else None, dg.ptr,
                                          F.rows, F.cap, F.r["kps"], F.r["desc"], F.r["counts"], F.node.ptr, F.weight.ptr if weights else None,
                                          dk.ptr, df.ptr, float(nnratio), int(check_ori), fm.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()
    assert L.orbm_sync(mt.h) == 0, L.orbm_last_error()
    return fm.download(np.int32, P * F.cap).reshape(P, F.cap), nm.download(np.int32, P)


def _check(pkg, oracle, mt, K, F, kf_row, f_row, good, nnratio, check_ori, rows, counts, weights=True):
    """Every pair against orbm_search_by_bow and the oracle; returns the counts."""
    OM = oracle._oracle_matcher_class()()
    for p, (kr, fr) in enumerate(zip(kf_row, f_row)):
        if not (0 <= kr < K.rows and 0 <= fr < F.rows):
            assert counts[p] == 0 and np.all(rows[p] == -1), p
            continue
        kk, dkk = K.kps(kr), K.desc(kr); kf_, df_ = F.kps(fr), F.desc(fr)
        nk, nf = len(kk), len(kf_)
        g = np.ascontiguousarray(good[kr * K.cap: kr * K.cap + nk])
        keep_k = K.h_weight[kr, :nk] > 0 if weights else np.ones(nk, bool)
        keep_f = F.h_weight[fr, :nf] > 0 if weights else np.ones(nf, bool)
        fvk, fvf = _fv(K.h_node[kr, :nk], keep_k), _fv(F.h_node[fr, :nf], keep_f)
        a = mt.SearchByBoW(kk, dkk, g, fvk, kf_, df_, fvf, nnratio, check_ori)
        b = OM.SearchByBoW(kk, dkk, g, fvk, kf_, df_, fvf, nnratio, check_ori)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), ("host vs oracle", p)
        assert counts[p] == b[0], ("count", p, counts[p], b[0])
        assert np.array_equal(rows[p, :nf], b[1]), ("row", p, np.flatnonzero(rows[p, :nf] != b[1])[:8])
        assert np.all(rows[p, nf:] == -1), p
    return counts


TRACK_KF = list(range(NF_IMG)) + [0, 1, 5, NKF_IMG, 3, -1, 2, 40, 0]          # overlapping pairs, unrelated, KF count 0, frame count 0, out of range
TRACK_F = list(range(NF_IMG)) + [NF_IMG, NF_IMG + 1, 2, 0, NF_IMG + 2, 0, 99, 1, -3]


@pytest.mark.parametrize("nnratio,check_ori", [(0.6, 1), (0.7, 1), (0.75, 0), (1.0, 1), (0.7, 0)])
def test_track_reference_pairs(pkg, oracle, synth, pools, nnratio, check_ori):
    """TrackReferenceKeyFrame shape: frames against overlapping KeyFrames (claims contend), unrelated pairs, empty rows, rows out of range;
    ORBvoc-sized vocabulary at levelsup 4 with all KF MapPoints good."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 6)
    K.transform(voc, 4); F.transform(voc, 4)
    good = np.ones(K.rows * K.cap, np.uint8)
    rows, counts = _run(pkg, mt, K, F, TRACK_KF, TRACK_F, good, nnratio, check_ori)
    _check(pkg, oracle, mt, K, F, TRACK_KF, TRACK_F, good, nnratio, check_ori, rows, counts)
    assert counts[:NF_IMG].min() > 100 and counts[NF_IMG:NF_IMG + 2].max() < 40, counts   # overlapping content matches, unrelated hardly
    assert np.all(counts[11:] == 0)


def test_relocalization_shape(pkg, oracle, synth, pools):
    """Relocalization: one frame against every KeyFrame of the pool through f_row (cap_kf != cap_f), nnratio 0.75, orientation on."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 6)
    K.transform(voc, 4); F.transform(voc, 4)
    kf_row = list(range(K.rows)); f_row = [3] * K.rows
    good = np.ones(K.rows * K.cap, np.uint8)
    rows, counts = _run(pkg, mt, K, F, kf_row, f_row, good, 0.75, 1)
    _check(pkg, oracle, mt, K, F, kf_row, f_row, good, 0.75, 1, rows, counts)
    assert len(kf_row) >= 16 and counts[3] > 100 and np.delete(counts, 3).max() < counts[3] // 2, counts


@pytest.mark.parametrize("mode", ["half", "zero"])
def test_good_masks(pkg, oracle, synth, pools, mode):
    """good_kf about 50 % random, and all zero (every count 0)."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 3)
    K.transform(voc, 1); F.transform(voc, 1)
    good = (np.random.default_rng(3).random(K.rows * K.cap) < 0.5).astype(np.uint8) if mode == "half" else np.zeros(K.rows * K.cap, np.uint8)
    rows, counts = _run(pkg, mt, K, F, TRACK_KF, TRACK_F, good, 0.7, 1)
    _check(pkg, oracle, mt, K, F, TRACK_KF, TRACK_F, good, 0.7, 1, rows, counts)
    if mode == "zero":
        assert counts.max() == 0 and np.all(rows == -1)
    else:
        assert counts[:NF_IMG].min() > 30


@pytest.mark.parametrize("weights", [True, False])
def test_stopped_words(pkg, oracle, synth, pools, weights):
    """A vocabulary with many stopped words: with the weights the stopped features are in no bucket; with NULL weights every feature is."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 3, stop_frac=0.2, seed=11)
    K.transform(voc, 1); F.transform(voc, 1)
    nstop = sum(int((K.h_weight[r, :len(K.kps(r))] <= 0).sum()) for r in range(NF_IMG))
    assert nstop > 200, nstop                                               # the rows really hold stopped features
    good = np.ones(K.rows * K.cap, np.uint8)
    rows, counts = _run(pkg, mt, K, F, TRACK_KF, TRACK_F, good, 0.7, 1, weights=weights)
    _check(pkg, oracle, mt, K, F, TRACK_KF, TRACK_F, good, 0.7, 1, rows, counts, weights=weights)
    if weights:                                                             # no match lands on a stopped frame feature
        for p in range(NF_IMG):
            nf = len(F.kps(p))
            assert np.all(F.h_weight[p, :nf][rows[p, :nf] >= 0] > 0)


@pytest.mark.parametrize("levelsup", [1, 2, 3])
def test_levelsup_and_long_buckets(pkg, oracle, synth, pools, levelsup):
    """(10, 3) vocabulary: levelsup 1, 2 (buckets of ~100 > 64) and 3 (the root: one bucket holding every feature, > 256)."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 3)
    K.transform(voc, levelsup); F.transform(voc, levelsup)
    good = np.ones(K.rows * K.cap, np.uint8)
    rows, counts = _run(pkg, mt, K, F, TRACK_KF, TRACK_F, good, 0.7, 1)
    _check(pkg, oracle, mt, K, F, TRACK_KF, TRACK_F, good, 0.7, 1, rows, counts)
    longest = max(np.bincount(F.h_node[0, :len(F.kps(0))] - F.h_node[0, :len(F.kps(0))].min()).max(),
                  np.bincount(K.h_node[0, :len(K.kps(0))] - K.h_node[0, :len(K.kps(0))].min()).max())
    if levelsup == 2:
        assert longest > 64
    if levelsup == 3:
        assert longest > 256 and len(np.unique(F.h_node[0, :len(F.kps(0))])) == 1


def test_self_pair(pkg, oracle, synth, pools):
    """The frame pool used as its own KeyFrame pool: KF row == frame row."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 6)
    F.transform(voc, 4)
    rows_ = list(range(F.rows))
    good = np.ones(F.rows * F.cap, np.uint8)
    rows, counts = _run(pkg, mt, F, F, rows_, rows_, good, 0.7, 1, kf_pool=F)
    _check(pkg, oracle, mt, F, F, rows_, rows_, good, 0.7, 1, rows, counts)
    assert counts[0] > 300


def test_transform_batch_matches_host(pkg, synth, pools):
    """orbm_bow_transform_batch_async word / node / weight equal orbm_bow_transform on the same rows; NULL word / weight are accepted."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 3, stop_frac=0.1)
    K.transform(voc, 2)
    for r in (0, 5, NKF_IMG - 1):
        n = len(K.kps(r))
        (_, _), (_, _, _), w, nd, wt = voc.transform(K.desc(r), 2)
        assert np.array_equal(K.h_word[r, :n], w) and np.array_equal(K.h_node[r, :n], nd) and K.h_weight[r, :n].tobytes() == wt.tobytes()
    L = pkg.lib()
    node2 = pkg.DeviceBuffer(4 * K.rows * K.cap)
    assert L.orbm_bow_transform_batch_async(mt.h, voc.h, K.r["desc"], K.rows * K.cap, 2, None, node2.ptr, None) == 0
    mt.sync()
    assert np.array_equal(node2.download(np.int32, K.rows * K.cap).reshape(K.rows, K.cap), K.h_node)


def test_capture_replay_equals_eager(pkg, oracle, synth, pools):
    """The step (frame extraction, transform of both pools, search) captured into a graph and replayed gives the eager rows and counts."""
    mt, K, F = pools
    L = pkg.lib()
    voc = _vocab(pkg, synth, mt, 10, 6)
    P = len(TRACK_KF)
    dk = pkg.DeviceBuffer(4 * P).upload(np.asarray(TRACK_KF, np.int32)); df = pkg.DeviceBuffer(4 * P).upload(np.asarray(TRACK_F, np.int32))
    good = np.ones(K.rows * K.cap, np.uint8); dg = pkg.DeviceBuffer(good.nbytes).upload(good)
    fm = pkg.DeviceBuffer(4 * P * F.cap); nm = pkg.DeviceBuffer(4 * P)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(F.ex.h)) == 0

    def enqueue():
        F.ex.enqueue_device(F.arr, W, H, F.stride, np.zeros(4 * F.rows, np.int32))    # the step: extraction, transform, search
        for pool in (K, F):
            assert L.orbm_bow_transform_batch_async(mt.h, voc.h, pool.r["desc"], pool.rows * pool.cap, 4, None, pool.node.ptr, pool.weight.ptr) == 0
        assert L.orbm_search_by_bow_batch_async(mt.h, P, K.rows, K.cap, K.r["kps"], K.r["desc"], K.r["counts"], K.node.ptr, K.weight.ptr, dg.ptr,
                                                F.rows, F.cap, F.r["kps"], F.r["desc"], F.r["counts"], F.node.ptr, F.weight.ptr,
                                                dk.ptr, df.ptr, 0.7, 1, fm.ptr, nm.ptr) == 0, L.orbm_last_error()

    enqueue()
    assert L.orbm_sync(mt.h) == 0
    eager_m = fm.download(np.int32, P * F.cap); eager_n = nm.download(np.int32, P)
    assert eager_n[:NF_IMG].min() > 100
    assert L.orbx_capture_begin(F.ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(F.ex.h) == 0, L.orbx_last_error()
    fm.upload(np.full(P * F.cap, -7, np.int32)); nm.upload(np.full(P, -7, np.int32))
    assert L.orbx_graph_launch(F.ex.h, 0) == 0, L.orbx_last_error()
    F.ex.sync()
    assert np.array_equal(fm.download(np.int32, P * F.cap), eager_m) and np.array_equal(nm.download(np.int32, P), eager_n)
    assert L.orbm_set_stream(mt.h, None) == 0


@pytest.mark.parametrize("capk,capf", [(20480, MAX_CAP), (MAX_CAP, MAX_CAP)])
def test_capacity_limit(pkg, oracle, synth, capk, capf):
    """cap_kf = 20480 (a 5 x 4000-feature initialiser KeyFrame) and both capacities at the documented limit (the largest LDS shape) are
    accepted and exact; the KF rows are a caller-gathered pool of that layout."""
    L = pkg.lib()
    mt = pkg.ORBmatcher(0.7)
    l, r = synth.gen_stereo_pair(W, H, 321)
    exk = pkg.ORBextractor(4000, max_size=(W, H)); exf = pkg.ORBextractor(1000, max_size=(W, H))
    _, kk, dk = exk(l, (0, 0)); _, kf_, df_ = exf(r, (0, 0))
    voc = _vocab(pkg, synth, mt, 10, 6)
    (_, _), (fvk_n, fvk_s, fvk_i), _, ndk, wk = voc.oracle.transform(dk, 4)
    (_, _), (fvf_n, fvf_s, fvf_i), _, ndf, wf = voc.oracle.transform(df_, 4)

    def pool(kps, desc, nd, wt, cap):
        k = np.zeros(cap, kps.dtype); k[:len(kps)] = kps
        d = np.zeros((cap, 32), np.uint8); d[:len(desc)] = desc
        n = np.zeros(cap, np.int32); n[:len(nd)] = nd
        w = np.zeros(cap, np.float64); w[:len(wt)] = wt
        return [pkg.DeviceBuffer(a.nbytes).upload(a) for a in (k, d, np.array([len(kps)], np.int32), n, w)]

    K = pool(kk, dk, ndk, wk, capk); F = pool(kf_, df_, ndf, wf, capf)
    good = np.ones(capk, np.uint8); dg = pkg.DeviceBuffer(capk).upload(good)
    fm = pkg.DeviceBuffer(4 * capf); nm = pkg.DeviceBuffer(4)
    rc = L.orbm_search_by_bow_batch_async(mt.h, 1, 1, capk, K[0].ptr, K[1].ptr, K[2].ptr, K[3].ptr, K[4].ptr, dg.ptr,
                                          1, capf, F[0].ptr, F[1].ptr, F[2].ptr, F[3].ptr, F[4].ptr, None, None, 0.7, 1, fm.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()
    assert L.orbm_sync(mt.h) == 0
    OM = oracle._oracle_matcher_class()()
    n_ref, row_ref = OM.SearchByBoW(kk, dk, good[:len(kk)], (fvk_n, fvk_s, fvk_i), kf_, df_, (fvf_n, fvf_s, fvf_i), 0.7, True)
    row = fm.download(np.int32, capf)
    assert int(nm.download(np.int32, 1)[0]) == n_ref and np.array_equal(row[:len(kf_)], row_ref) and np.all(row[len(kf_):] == -1)
    assert len(kk) > 3000 and n_ref > 100


def test_refusals_enqueue_nothing(pkg):
    """Each refusal code with the documented reason; the outputs keep their sentinel."""
    m = pkg.ORBmatcher()
    L = m.L
    buf = pkg.DeviceBuffer(1 << 16)
    p = buf.ptr
    fm = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))

    def call(npairs=1, nkr=1, capk=4, nfr=1, capf=4, nn=0.7, node_kf=p, good=p, f_match=None):
        return L.orbm_search_by_bow_batch_async(m.h, npairs, nkr, capk, p, p, p, node_kf, None, good, nfr, capf, p, p, p, p, None,
                                                None, None, nn, 1, f_match or fm.ptr, fm.ptr)
    assert call(node_kf=None) == -2 and call(good=None) == -2
    assert call(npairs=0) == -2 and call(nkr=0) == -2 and call(nfr=0) == -2 and call(capk=0) == -2 and call(capf=0) == -2
    assert call(nn=float("nan")) == -2 and call(nn=float("inf")) == -2
    assert call(capk=MAX_CAP + 1) == -3 and b"24576" in L.orbm_last_error()
    assert call(capf=MAX_CAP + 1) == -3
    assert call(npairs=65536) == -3
    assert L.orbm_bow_transform_batch_async(m.h, None, p, 4, 4, None, p, None) == -2
    m.sync()
    assert np.all(fm.download(np.int32, 16) == 12345)
