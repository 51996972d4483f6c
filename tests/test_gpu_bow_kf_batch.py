"""M8 SearchByBoW(KeyFrame, KeyFrame) batched on the device (orbm_search_by_bow_kf_batch_async).  Every pair's row and count must equal the
host entry point orbm_search_by_bow_kf AND the oracle's SearchByBoWKF, both given FeatureVectors built as DBoW2 builds them (weight > 0).
Pools are extractor result blocks (stereo pairs, unrelated images, a black image; cap1 != cap2) with node ids and weights from
orbm_bow_transform_batch_async, or rows laid out by hand for the threshold, tie, contention and bucket cases."""
import numpy as np
import pytest

from test_gpu_bow_batch import MAX_CAP, NF_IMG, NKF_IMG, Pool, _fv, _vocab, pools  # noqa: F401  (fixture + helpers)

pytestmark = pytest.mark.gpu


def _goods(mode, n, seed):
    if mode == "all":
        return np.ones(n, np.uint8)
    if mode == "none":
        return np.zeros(n, np.uint8)
    return (np.random.default_rng(seed).random(n) < 0.5).astype(np.uint8)


def _run(pkg, mt, A, B, row1, row2, good1, good2, nnratio, check_ori, weights=True, null_rows=False):
    L = pkg.lib()
    P = len(row1)
    d1 = pkg.DeviceBuffer(4 * P).upload(np.asarray(row1, np.int32)); d2 = pkg.DeviceBuffer(4 * P).upload(np.asarray(row2, np.int32))
    g1 = pkg.DeviceBuffer(good1.nbytes).upload(good1); g2 = pkg.DeviceBuffer(good2.nbytes).upload(good2)
    mm = pkg.DeviceBuffer(4 * P * A.cap).upload(np.full(P * A.cap, -7, np.int32)); nm = pkg.DeviceBuffer(4 * P).upload(np.full(P, -7, np.int32))
    rc = L.orbm_search_by_bow_kf_batch_async(mt.h, P, A.rows, A.cap, A.r["kps"], A.r["desc"], A.r["counts"], A.node.ptr,
                                             A.weight.ptr if weights else None, g1.ptr,
                                             B.rows, B.cap, B.r["kps"], B.r["desc"], B.r["counts"], B.node.ptr, B.weight.ptr if weights else None, g2.ptr,
                                             None if null_rows else d1.ptr, None if null_rows else d2.ptr, float(nnratio), int(check_ori), mm.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()
    assert L.orbm_sync(mt.h) == 0, L.orbm_last_error()
    return mm.download(np.int32, P * A.cap).reshape(P, A.cap), nm.download(np.int32, P)


def _check(oracle, mt, A, B, row1, row2, good1, good2, nnratio, check_ori, rows, counts, weights=True):
    """Every pair against orbm_search_by_bow_kf and the oracle.  Returns per pair the oracle's count with and without the rotation cull."""
    OM = oracle._oracle_matcher_class()()
    with_ori, without = [], []
    for p, (r1, r2) in enumerate(zip(row1, row2)):
        if not (0 <= r1 < A.rows and 0 <= r2 < B.rows):
            assert counts[p] == 0 and np.all(rows[p] == -1), p
            with_ori.append(0); without.append(0)
            continue
        k1, dd1 = A.kps(r1), A.desc(r1); k2, dd2 = B.kps(r2), B.desc(r2)
        n1, n2 = len(k1), len(k2)
        ga = np.ascontiguousarray(good1[r1 * A.cap: r1 * A.cap + n1]); gb = np.ascontiguousarray(good2[r2 * B.cap: r2 * B.cap + n2])
        keep1 = A.h_weight[r1, :n1] > 0 if weights else np.ones(n1, bool)
        keep2 = B.h_weight[r2, :n2] > 0 if weights else np.ones(n2, bool)
        args = dict(k1=k1, d1=dd1, good1=ga, fv1=_fv(A.h_node[r1, :n1], keep1), k2=k2, d2=dd2, good2=gb, fv2=_fv(B.h_node[r2, :n2], keep2),
                    nnratio=nnratio)
        if n1 == 0 or n2 == 0:
            assert counts[p] == 0 and np.all(rows[p] == -1), p
            with_ori.append(0); without.append(0)
            continue
        a = mt.SearchByBoWKF(check_ori=check_ori, **args)
        b = OM.SearchByBoWKF(check_ori=check_ori, **args)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), ("host vs oracle", p)
        assert counts[p] == b[0], ("count", p, counts[p], b[0])
        assert np.array_equal(rows[p, :n1], b[1]), ("row", p, np.flatnonzero(rows[p, :n1] != b[1])[:8])
        assert np.all(rows[p, n1:] == -1), p
        with_ori.append(b[0]); without.append(OM.SearchByBoWKF(check_ori=False, **args)[0] if check_ori else b[0])
    return np.array(with_ori), np.array(without)


# pool K: 16 left images + black (cap 1500-ish); pool F: 8 right images, 2 unrelated, black
PLACE_ROW1 = [3] * 36                                                       # the place-recognition shape: one current KeyFrame, 36 candidates
PLACE_ROW2 = [(i * 5) % 11 for i in range(36)]
DISTINCT_1 = list(range(NF_IMG)) + [0, 1, 5, NKF_IMG, 3, -1, 2, 40, 0]      # overlapping, unrelated, empty rows, out of range
DISTINCT_2 = list(range(NF_IMG)) + [NF_IMG, NF_IMG + 1, 2, 0, NF_IMG + 2, 0, 99, 1, -3]


@pytest.mark.parametrize("nnratio,check_ori", [(0.9, 1), (0.6, 1), (0.9, 0), (0.6, 0)])
@pytest.mark.parametrize("shape", ["place", "distinct"])
def test_extractor_pools(pkg, oracle, synth, pools, shape, nnratio, check_ori):
    """cap1 != cap2; one row against 36 (K row 3 as pKF1 against the frame pool's rows) and distinct rows with empty and out-of-range ones."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 6)
    K.transform(voc, 4); F.transform(voc, 4)
    r1, r2 = (PLACE_ROW1, PLACE_ROW2) if shape == "place" else (DISTINCT_1, DISTINCT_2)
    g1, g2 = _goods("all", K.rows * K.cap, 0), _goods("all", F.rows * F.cap, 0)
    rows, counts = _run(pkg, mt, K, F, r1, r2, g1, g2, nnratio, check_ori)
    w, wo = _check(oracle, mt, K, F, r1, r2, g1, g2, nnratio, check_ori, rows, counts)
    nonempty = [p for p, (a, b) in enumerate(zip(r1, r2)) if 0 <= a < K.rows and 0 <= b < F.rows and len(K.kps(a)) and len(F.kps(b))]
    assert (w[nonempty] > 0).sum() > len(nonempty) / 2, w                   # vacuity: the oracle matches in most non-empty pairs
    if check_ori:
        assert np.any(wo > w), (w, wo)                                      # and the rotation cull removes matches somewhere


@pytest.mark.parametrize("m1,m2", [("all", "half"), ("half", "all"), ("half", "half"), ("none", "all"), ("all", "none")])
def test_good_masks(pkg, oracle, synth, pools, m1, m2):
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 3)
    K.transform(voc, 1); F.transform(voc, 1)
    g1, g2 = _goods(m1, K.rows * K.cap, 3), _goods(m2, F.rows * F.cap, 4)
    rows, counts = _run(pkg, mt, K, F, DISTINCT_1, DISTINCT_2, g1, g2, 0.9, 1)
    w, _ = _check(oracle, mt, K, F, DISTINCT_1, DISTINCT_2, g1, g2, 0.9, 1, rows, counts)
    if "none" in (m1, m2):
        assert counts.max() == 0 and np.all(rows == -1)
    else:
        assert w[:NF_IMG].min() > 20
        for p in range(NF_IMG):                                             # no match names a pKF2 feature without a good MapPoint
            m = rows[p][rows[p] >= 0]
            assert np.all(g2[DISTINCT_2[p] * F.cap + m] == 1) and np.all(g1[DISTINCT_1[p] * K.cap + np.flatnonzero(rows[p] >= 0)] == 1)


@pytest.mark.parametrize("weights", [True, False])
def test_stopped_words(pkg, oracle, synth, pools, weights):
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 3, stop_frac=0.2, seed=11)
    K.transform(voc, 1); F.transform(voc, 1)
    g1, g2 = _goods("all", K.rows * K.cap, 0), _goods("all", F.rows * F.cap, 0)
    rows, counts = _run(pkg, mt, K, F, DISTINCT_1, DISTINCT_2, g1, g2, 0.9, 1, weights=weights)
    w, _ = _check(oracle, mt, K, F, DISTINCT_1, DISTINCT_2, g1, g2, 0.9, 1, rows, counts, weights=weights)
    assert w[:NF_IMG].min() > 50
    if weights:
        for p in range(NF_IMG):
            n1 = len(K.kps(p))
            assert np.all(K.h_weight[p, :n1][rows[p, :n1] >= 0] > 0)


@pytest.mark.parametrize("levelsup", [2, 3])
def test_long_buckets_self_and_swapped(pkg, oracle, synth, pools, levelsup):
    """Buckets longer than 64 (levelsup 2) and the root bucket (3) on both sides; a row against itself through one pool passed twice and
    NULL row arrays; the pools swapped: the result is not the transpose."""
    mt, K, F = pools
    voc = _vocab(pkg, synth, mt, 10, 3)
    K.transform(voc, levelsup); F.transform(voc, levelsup)
    gk, gf = _goods("all", K.rows * K.cap, 0), _goods("all", F.rows * F.cap, 0)
    ident = list(range(F.rows))
    rows, counts = _run(pkg, mt, F, F, ident, ident, gf, gf, 0.9, 1, null_rows=True)
    w, _ = _check(oracle, mt, F, F, ident, ident, gf, gf, 0.9, 1, rows, counts)
    assert w[0] > 300 and w[-1] == 0                                        # the black image: an empty row
    a, b = list(range(NF_IMG)), list(range(NF_IMG))
    r12, c12 = _run(pkg, mt, K, F, a, b, gk, gf, 0.9, 1)
    r21, c21 = _run(pkg, mt, F, K, b, a, gf, gk, 0.9, 1)
    _check(oracle, mt, K, F, a, b, gk, gf, 0.9, 1, r12, c12)
    _check(oracle, mt, F, K, b, a, gf, gk, 0.9, 1, r21, c21)
    differs = 0
    for p in range(NF_IMG):
        t = np.full(K.cap, -1, np.int32); j = np.flatnonzero(r21[p] >= 0); t[r21[p][j]] = j
        differs += not np.array_equal(t, r12[p])
    assert differs > 0


def test_capture_replay_equals_eager(pkg, synth, pools):
    mt, K, F = pools
    L = pkg.lib()
    voc = _vocab(pkg, synth, mt, 10, 6)
    P = len(PLACE_ROW1)
    d1 = pkg.DeviceBuffer(4 * P).upload(np.asarray(PLACE_ROW1, np.int32)); d2 = pkg.DeviceBuffer(4 * P).upload(np.asarray(PLACE_ROW2, np.int32))
    g1 = pkg.DeviceBuffer(K.rows * K.cap).upload(np.ones(K.rows * K.cap, np.uint8)); g2 = pkg.DeviceBuffer(F.rows * F.cap).upload(np.ones(F.rows * F.cap, np.uint8))
    mm = pkg.DeviceBuffer(4 * P * K.cap); nm = pkg.DeviceBuffer(4 * P)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(F.ex.h)) == 0
    try:
        def enqueue():
            F.ex.enqueue_device(F.arr, 752, 480, F.stride, np.zeros(4 * F.rows, np.int32))
            for pool in (K, F):
                assert L.orbm_bow_transform_batch_async(mt.h, voc.h, pool.r["desc"], pool.rows * pool.cap, 4, None, pool.node.ptr, pool.weight.ptr) == 0
            assert L.orbm_search_by_bow_kf_batch_async(mt.h, P, K.rows, K.cap, K.r["kps"], K.r["desc"], K.r["counts"], K.node.ptr, K.weight.ptr, g1.ptr,
                                                       F.rows, F.cap, F.r["kps"], F.r["desc"], F.r["counts"], F.node.ptr, F.weight.ptr, g2.ptr,
                                                       d1.ptr, d2.ptr, 0.9, 1, mm.ptr, nm.ptr) == 0, L.orbm_last_error()
        enqueue()
        assert L.orbm_sync(mt.h) == 0
        eager_m = mm.download(np.int32, P * K.cap); eager_n = nm.download(np.int32, P)
        assert eager_n.max() > 100
        assert L.orbx_capture_begin(F.ex.h, 0) == 0, L.orbx_last_error()
        enqueue()
        assert L.orbx_capture_end(F.ex.h) == 0, L.orbx_last_error()
        mm.upload(np.full(P * K.cap, -7, np.int32)); nm.upload(np.full(P, -7, np.int32))
        assert L.orbx_graph_launch(F.ex.h, 0) == 0, L.orbx_last_error()
        F.ex.sync()
        assert np.array_equal(mm.download(np.int32, P * K.cap), eager_m) and np.array_equal(nm.download(np.int32, P), eager_n)
    finally:
        assert L.orbm_set_stream(mt.h, None) == 0


# ---- hand-built rows -------------------------------------------------------------------------------------------------------------------
def _bits(base, n):
    """base with its first n bits flipped: Hamming distance exactly n."""
    d = base.copy()
    for b in range(n):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _hand(pkg, oracle, d1, n1, d2, n2, nnratio=0.9, cap1=None, cap2=None, check_ori=0):
    """One pair of rows uploaded by the test (node ids given, all weights 1, all good); returns the device row, checked against the host
    entry point and the oracle."""
    L = pkg.lib(); mt = pkg.ORBmatcher(0.9)
    c1, c2 = cap1 or len(d1) + 3, cap2 or len(d2) + 5

    def pool(desc, nodes, cap):
        k = np.zeros(cap, pkg.KP_DTYPE); k["angle"][:len(desc)] = 10.0
        d = np.full((cap, 32), 0xAA, np.uint8); d[:len(desc)] = desc         # padding: identical garbage that would match if read
        n = np.zeros(cap, np.int32); n[:len(desc)] = nodes
        return k, d, n, [pkg.DeviceBuffer(a.nbytes).upload(a) for a in (k, d, np.array([len(desc)], np.int32), n, np.ones(cap, np.uint8))]
    ka, da, na, A = pool(np.asarray(d1, np.uint8), np.asarray(n1, np.int32), c1)
    kb, db, nb, B = pool(np.asarray(d2, np.uint8), np.asarray(n2, np.int32), c2)
    mm = pkg.DeviceBuffer(4 * c1); nm = pkg.DeviceBuffer(4)
    rc = L.orbm_search_by_bow_kf_batch_async(mt.h, 1, 1, c1, A[0].ptr, A[1].ptr, A[2].ptr, A[3].ptr, None, A[4].ptr,
                                             1, c2, B[0].ptr, B[1].ptr, B[2].ptr, B[3].ptr, None, B[4].ptr, None, None, float(nnratio), check_ori, mm.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()
    assert L.orbm_sync(mt.h) == 0
    row = mm.download(np.int32, c1); cnt = int(nm.download(np.int32, 1)[0])
    m1, m2 = len(d1), len(d2)
    args = dict(k1=ka[:m1], d1=da[:m1], good1=np.ones(m1, np.uint8), fv1=_fv(na[:m1], np.ones(m1, bool)),
                k2=kb[:m2], d2=db[:m2], good2=np.ones(m2, np.uint8), fv2=_fv(nb[:m2], np.ones(m2, bool)), nnratio=nnratio, check_ori=bool(check_ori))
    a = mt.SearchByBoWKF(**args); b = oracle._oracle_matcher_class()().SearchByBoWKF(**args)
    assert a[0] == b[0] == cnt and np.array_equal(a[1], b[1]) and np.array_equal(row[:m1], b[1]) and np.all(row[m1:] == -1)
    return row[:m1]


def test_th_low_is_strict(pkg, oracle):
    """Best distance 49 matches, 50 and 51 do not: M7 would accept 50."""
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    d2 = [_bits(base[0], 49), _bits(base[1], 50), _bits(base[2], 51)]
    row = _hand(pkg, oracle, list(base), [5, 6, 7], d2, [5, 6, 7], nnratio=1.0)
    assert list(row) == [0, -1, -1]


def test_tie_and_contention(pkg, oracle):
    """Two equal best distances: the ratio test fails for nnratio <= 1.  Two pKF1 features wanting one pKF2 feature: the second takes its
    next best (inside TH_LOW) or nothing."""
    rng = np.random.default_rng(2)
    b = rng.integers(0, 256, 32, dtype=np.uint8)
    far = b ^ np.uint8(0xFF)
    row = _hand(pkg, oracle, [b], [9], [_bits(b, 10), far, _bits(b, 10)], [9, 9, 9], nnratio=1.0)
    # candidates 0 and 2 are the same descriptor at distance 10 (candidate 1 is far): a tie
    assert list(row) == [-1]
    row = _hand(pkg, oracle, [b, _bits(b, 1)], [4, 4], [_bits(b, 2), _bits(b, 30), far], [4, 4, 4], nnratio=0.9)
    assert list(row) == [0, 1]                                              # the second feature falls back to its next best
    row = _hand(pkg, oracle, [b, _bits(b, 1)], [4, 4], [_bits(b, 2), _bits(b, 60), far], [4, 4, 4], nnratio=0.9)
    assert list(row) == [0, -1]                                             # ... or to nothing


def test_hash_collision_and_long_buckets(pkg, oracle):
    """Nodes 3 and 259 share the hash bucket (node & 255) but never meet; buckets of 150 features on both sides."""
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    n = 150
    d1 = np.stack([_bits(base[i % 2], int(rng.integers(0, 12))) for i in range(2 * n)])
    d2 = np.stack([_bits(base[(i + 1) % 2], int(rng.integers(0, 12))) for i in range(2 * n)])
    n1 = np.where(np.arange(2 * n) % 2 == 0, 3, 259); n2 = np.where((np.arange(2 * n) + 1) % 2 == 0, 3, 259)
    # identical descriptors under DIFFERENT nodes: pKF1's node-3 features look like pKF2's node-259 features and vice versa
    d2x = d2.copy(); n2x = np.where(n2 == 3, 259, 3)
    row = _hand(pkg, oracle, d1, n1, d2x, n2x, nnratio=1.0)
    got = np.flatnonzero(row >= 0)
    assert np.all(n1[got] == n2x[row[got]])                                 # a match never crosses nodes
    row = _hand(pkg, oracle, d1, n1, d2, n2, nnratio=1.0)
    assert np.all(n1[np.flatnonzero(row >= 0)] == n2[row[row >= 0]])


def test_refusals_enqueue_nothing(pkg):
    m = pkg.ORBmatcher()
    L = m.L
    buf = pkg.DeviceBuffer(1 << 16)
    p = buf.ptr
    out = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))
    names = ["kps1", "desc1", "counts1", "node1", "good1", "kps2", "desc2", "counts2", "node2", "good2", "matches12", "nmatches"]

    def call(npairs=1, n1=1, c1=4, n2=1, c2=4, nn=0.9, **null):
        a = {k: (None if k in null else (out.ptr if k in ("matches12", "nmatches") else p)) for k in names}
        return L.orbm_search_by_bow_kf_batch_async(m.h, npairs, n1, c1, a["kps1"], a["desc1"], a["counts1"], a["node1"], None, a["good1"],
                                                   n2, c2, a["kps2"], a["desc2"], a["counts2"], a["node2"], None, a["good2"],
                                                   None, None, nn, 1, a["matches12"], a["nmatches"])
    for k in names:
        assert call(**{k: 1}) == -2, k
    for kw in (dict(npairs=0), dict(n1=0), dict(n2=0), dict(c1=0), dict(c2=0), dict(nn=float("nan")), dict(nn=float("inf"))):
        assert call(**kw) == -2, kw
    assert call(c1=MAX_CAP + 1) == -3 and b"24576" in L.orbm_last_error()
    assert call(c2=MAX_CAP + 1) == -3 and call(npairs=65536) == -3
    m.sync()
    assert np.all(out.download(np.int32, 16) == 12345)
