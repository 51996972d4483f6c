"""Inputs shared by the two-camera SearchByBoW tests (M7 with F.Nleft != -1, ORBmatcher.cc:314-547).

A Batch is what one orbm_search_by_bow_fisheye_batch_async call takes, as numpy arrays: a KeyFrame pool (one STACKED row per two-camera
KeyFrame), a frame pool (one row per camera image), the pair lists kf_row / fl_row / fr_row and the two parameters.  single_args()
turns one pair of it into the arguments of the single-pair forms (the oracle's and the product's SearchByBoWFisheye, the second
reading): stacked frame arrays, Nleft and FeatureVectors built as DBoW2 builds them (nodes ascending, indices ascending, weight > 0).

  hand(nnratio, check_ori, weights)   hand-laid pairs: descriptors are bit patterns at chosen Hamming distances from an all-zero
                                      KeyFrame descriptor, node ids are assigned directly; each pair is built to reach one rule
  scene(oracle, synth, levelsup, ...) 376 x 240 synthetic rigs, 500 features per camera, a seeded (10, 3) vocabulary tree; 9 pairs

This file only makes arrays: the extractor and the vocabulary are handed in, and no matcher of the oracle, the product or a second
reading is imported."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
W, H, NF = 376, 240, 500

# the (nnratio, check_ori, weights) of the hand batch and the (levelsup, nnratio, check_ori, weights) of the scene batch every test file runs
HAND_PARAMS = [(0.7, 1, True), (0.7, 0, True), (0.75, 1, True), (1.0, 1, True), (1.0, 0, True), (1.25, 1, True), (0.7, 1, False)]
SCENE_PARAMS = [(1, 0.7, 1, True), (1, 0.75, 1, True), (1, 1.0, 0, True), (2, 0.7, 1, True), (2, 0.75, 0, True), (2, 1.0, 1, True), (2, 0.7, 1, False)]

_cache = {}


class Batch:
    def __init__(self, name, K, Fp, kf_row, fl_row, fr_row, nnratio, check_ori, weights=True, names=None):
        self.name, self.K, self.F = name, K, Fp
        self.kf_row, self.fl_row, self.fr_row = [np.asarray(a, np.int32) for a in (kf_row, fl_row, fr_row)]
        self.nnratio, self.check_ori, self.weights = float(nnratio), int(check_ori), bool(weights)
        self.names = names or ["pair%d" % p for p in range(len(kf_row))]

    @property
    def npairs(self):
        return len(self.kf_row)

    def in_range(self, p):
        return 0 <= self.kf_row[p] < self.K["rows"] and 0 <= self.fl_row[p] < self.F["rows"] and 0 <= self.fr_row[p] < self.F["rows"]

    def with_params(self, nnratio, check_ori, weights=True):
        return Batch(self.name, self.K, self.F, self.kf_row, self.fl_row, self.fr_row, nnratio, check_ori, weights, self.names)


def make_pool(rows, cap, with_good):
    """rows: [(kps, desc, node, weight[, good])] -> the block arrays of one pool; slots past a count hold zeros (good: ones, so that
    only the count keeps them out)."""
    n = len(rows)
    P = dict(rows=n, cap=cap, kps=np.zeros((n, cap), KP_DTYPE), desc=np.zeros((n, cap, 32), np.uint8), counts=np.zeros(n, np.int32),
             node=np.zeros((n, cap), np.int32), weight=np.ones((n, cap), np.float64))
    if with_good:
        P["good"] = np.ones((n, cap), np.uint8)
    for r, row in enumerate(rows):
        c = len(row[0])
        assert c <= cap
        P["counts"][r] = c
        P["kps"][r, :c] = row[0]; P["desc"][r, :c] = row[1]; P["node"][r, :c] = row[2]; P["weight"][r, :c] = row[3]
        if with_good:
            P["good"][r, :c] = row[4]
    return P


def feature_vector(nodes, keep):
    """FeatureVector CSR of DBoW2 (std::map<node, vector<idx>>) over the features with keep set: nodes ascending, indices ascending."""
    idx = np.flatnonzero(keep).astype(np.int32)
    order = idx[np.argsort(nodes[idx], kind="stable")]
    un, start = np.unique(nodes[order], return_index=True)
    return un.astype(np.int32), np.append(start, len(order)).astype(np.int32), order.astype(np.int32)


def single_args(b, p):
    """Pair p as (kps_kf, desc_kf, kf_good, fv_kf, kps_f, desc_f, nleft, fv_f, nnratio, check_ori) for a single-pair SearchByBoWFisheye,
    the frame stacked left then right.  None for a pair with a row out of range."""
    if not b.in_range(p):
        return None
    K, Fp = b.K, b.F
    kr, fl, fr = int(b.kf_row[p]), int(b.fl_row[p]), int(b.fr_row[p])
    nk, nl, nr = int(K["counts"][kr]), int(Fp["counts"][fl]), int(Fp["counts"][fr])
    kps_f = np.concatenate([Fp["kps"][fl, :nl], Fp["kps"][fr, :nr]])
    desc_f = np.concatenate([Fp["desc"][fl, :nl], Fp["desc"][fr, :nr]])
    node_f = np.concatenate([Fp["node"][fl, :nl], Fp["node"][fr, :nr]])
    wt_f = np.concatenate([Fp["weight"][fl, :nl], Fp["weight"][fr, :nr]])
    keep_k = K["weight"][kr, :nk] > 0 if b.weights else np.ones(nk, bool)
    keep_f = wt_f > 0 if b.weights else np.ones(nl + nr, bool)
    return (np.ascontiguousarray(K["kps"][kr, :nk]), np.ascontiguousarray(K["desc"][kr, :nk]), np.ascontiguousarray(K["good"][kr, :nk]),
            feature_vector(K["node"][kr, :nk], keep_k), kps_f, desc_f, nl, feature_vector(node_f, keep_f), b.nnratio, b.check_ori)


# ---------------------------------------------------------------------------------------------------------------------------
# hand-laid pairs
# ---------------------------------------------------------------------------------------------------------------------------
def d(k, start=0):
    """A descriptor with bits [start, start + k) set: Hamming distance k from the all-zero descriptor."""
    bits = np.zeros(256, np.uint8); bits[start:start + k] = 1
    return np.packbits(bits, bitorder="little")


FAR = d(120, 130)                                                  # 120 bits away from zero, and from every d(k <= 60) at least 120 - k


def _rows(feats, with_good=False):
    """feats: [(node, desc, angle, weight[, good])] -> the row tuple of make_pool."""
    n = len(feats)
    kps = np.zeros(n, KP_DTYPE)
    kps["angle"] = [f[2] for f in feats]
    kps["x"] = np.arange(n); kps["octave"] = 0
    out = (kps, np.array([f[1] for f in feats], np.uint8).reshape(n, 32), np.array([f[0] for f in feats], np.int32),
           np.array([f[3] for f in feats], np.float64))
    return out + (np.array([f[4] for f in feats], np.uint8),) if with_good else out


def _k(node=7, desc=None, angle=0.0, weight=1.0, good=1):
    return (node, d(0) if desc is None else desc, angle, weight, good)


def _f(desc, node=7, angle=0.0, weight=1.0):
    return (node, desc, angle, weight)


def _long_bucket(rng, nl, nr, nkf, node=7):
    """nl left and nr right candidates of one node among features of other nodes, in shuffled slot order; nkf KeyFrame features with
    random descriptors, each with one near copy (3 + i flipped bits) in each camera that has candidates, placed late in the list where
    it can be, and a second copy at 30 flips as the runner-up."""
    def flip(desc, k):
        out = np.unpackbits(desc).copy()
        out[rng.choice(256, k, replace=False)] ^= 1
        return np.packbits(out)

    kdesc = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(nkf)]
    kf = [_k(node, kdesc[i], angle=float(rng.uniform(0, 360))) for i in range(nkf)]
    kf += [_k(node + 1 + i, rng.integers(0, 256, 32, dtype=np.uint8)) for i in range(5)]
    sides = []
    for n in (nl, nr):
        cand = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(n)]
        if n:
            late = list(range(n - 1, -1, -1))
            for i in range(nkf):
                if n >= 2 * nkf:
                    cand[late[2 * i]] = flip(kdesc[i], 3 + i)
                    cand[late[2 * i + 1]] = flip(kdesc[i], 30)
                elif i < n:                                                     # a short side: the near copy alone
                    cand[i] = flip(kdesc[i], 3 + i)
        feats = [(True, _f(c, node, angle=float(rng.uniform(0, 360)))) for c in cand]
        feats += [(False, _f(rng.integers(0, 256, 32, dtype=np.uint8), node + 1 + int(rng.integers(0, 5)))) for _ in range(20)]
        # a stable shuffle of which slots hold the node's candidates: their relative order stays as laid out above
        mask = rng.permutation(np.array([f[0] for f in feats]))
        inn = iter([f[1] for f in feats if f[0]]); out = iter([f[1] for f in feats if not f[0]])
        sides.append([next(inn) if m else next(out) for m in mask])
    return kf, sides[0], sides[1]


def _hand_pairs():
    rng = np.random.default_rng(4242)
    P = {}
    # bestDist1 on / just above TH_LOW with a right candidate at 10
    P["th_50"] = ([_k()], [_f(d(50)), _f(d(80))], [_f(d(10))])
    P["th_51"] = ([_k()], [_f(d(51)), _f(d(90))], [_f(d(10))])
    # no left candidate in the node (the left row holds another node): the right candidate at 10 is never looked at
    P["no_left_in_node"] = ([_k()], [_f(d(5), node=8)], [_f(d(10))])
    # the left ratio test fails at every nnratio <= 1 (two left candidates at 20 on different bits); the right slot is claimed
    P["left_ratio_fails"] = ([_k()], [_f(d(20)), _f(d(20, 20)), _f(FAR)], [_f(FAR), _f(d(10))])
    # right ties (bestDist1R == bestDist2R, claimed: first index) and left ties (claimed only with nnratio > 1: first index)
    P["right_tie"] = ([_k()], [_f(d(5)), _f(d(60))], [_f(FAR), _f(d(10, 40)), _f(d(10))])
    P["left_tie"] = ([_k()], [_f(FAR), _f(d(30, 30)), _f(d(30)), _f(d(60))], [_f(d(12))])
    # a later KeyFrame feature takes the second-best slot after the best was claimed, in each camera; each claims one slot per camera
    P["second_best"] = ([_k(), _k()], [_f(d(40)), _f(d(8)), _f(d(5))], [_f(d(9)), _f(FAR), _f(d(6))])
    # the right camera's only candidate is claimed by the first KeyFrame feature: the second one finds none there
    P["right_exhausted"] = ([_k(), _k()], [_f(d(5)), _f(d(8)), _f(d(40))], [_f(d(6))])
    # node ids 7 and 263 share a hash bucket of 256: features of different nodes never meet
    P["hash_collision"] = ([_k(7), _k(263), _k(519, d(2))],
                           [_f(d(5), 263), _f(d(6), 7), _f(d(60), 7), _f(d(60), 263), _f(d(1), 519 + 256)],
                           [_f(d(3), 263), _f(d(4), 7), _f(d(1), 775)])
    # stopped words on each side and good_kf holes: the nearest KeyFrame feature, left and right candidates are out
    P["stopped_and_holes"] = ([_k(weight=0.0, angle=10.0), _k(good=0, angle=20.0), _k(angle=30.0)],
                              [_f(d(2), weight=0.0), _f(d(7)), _f(d(45))], [_f(d(1), weight=0.0), _f(d(9))])
    # culls that clear entries of both rows: every KeyFrame feature claims one slot per camera in its own node; bins 0 (12 entries),
    # 5 (7) and 10 (4) survive, bin 15 (one left entry) and bin 20 (one entry in each row) are cleared
    kf, le, ri = [], [], []
    for i, (ak, al, ar) in enumerate([(0, 0, 0)] * 6 + [(60, 0, 0)] * 3 + [(120, 0, 0)] * 2 + [(180, 0, 120), (240, 0, 0)]):
        kf.append(_k(100 + i, angle=float(ak))); le.append(_f(d(3), 100 + i, angle=float(al))); ri.append(_f(d(2), 100 + i, angle=float(ar)))
    P["cull_both_rows"] = (kf, le, ri)
    # buckets longer than 64: left only, right only (six left candidates open the node), the boundary inside a 64-entry pass, > 128
    for nl, nr in ((70, 0), (6, 70), (60, 10), (64, 1), (63, 2), (100, 60), (130, 5)):
        P["long_%d_%d" % (nl, nr)] = _long_bucket(rng, nl, nr, 6)
    # empty rows
    P["empty_right"] = ([_k(), _k()], [_f(d(5)), _f(d(8)), _f(d(40))], [])
    P["empty_left"] = ([_k()], [], [_f(d(3))])
    P["empty_kf"] = ([], [_f(d(5))], [_f(d(3))])
    return P


def hand(nnratio=0.7, check_ori=1, weights=True):
    """All hand-laid pairs in one batch (pair p: KeyFrame row p, left row 2p, right row 2p + 1), then pairs with a row out of range."""
    if "hand" not in _cache:
        P = _hand_pairs()
        names = list(P)
        krows = [_rows(P[n][0], True) for n in names]
        frows = [r for n in names for r in (_rows(P[n][1]), _rows(P[n][2]))]
        K = make_pool(krows, max(len(r[0]) for r in krows) + 3, True)
        Fp = make_pool(frows, max(len(r[0]) for r in frows) + 5, False)
        n = len(names)
        kf_row = list(range(n)) + [-1, n, 0, 0, 0, 0]
        fl_row = [2 * p for p in range(n)] + [0, 0, -1, 2 * n, 0, 0]
        fr_row = [2 * p + 1 for p in range(n)] + [1, 1, 1, 1, -5, 2 * n]
        _cache["hand"] = Batch("hand", K, Fp, kf_row, fl_row, fr_row, 0.7, 1, True, names + ["out_of_range_%d" % i for i in range(6)])
    return _cache["hand"].with_params(nnratio, check_ori, weights)


# ---------------------------------------------------------------------------------------------------------------------------
# scene pairs
# ---------------------------------------------------------------------------------------------------------------------------
def scene_tree(synth, stop_frac=0.15, seed=31):
    """A (10, 3) tree with 15 % of its words stopped."""
    tree = synth.gen_vocabulary(10, 3, seed=seed)
    rng = np.random.default_rng(seed)
    leaves = np.flatnonzero(tree["is_leaf"])
    tree["weight"][rng.choice(leaves, int(len(leaves) * stop_frac), replace=False)] = 0.0
    return tree


def scene_images(synth):
    """Three rigs: KeyFrame images (left, right) and the frame images of the same rig a little later (shifted, with new noise)."""
    rng = np.random.default_rng(99)
    kf, fr = [], []
    for s in range(3):
        l, r = synth.gen_stereo_pair(W, H, 5200 + s)
        kf.append((l, r))
        fr.append(tuple(np.clip(np.roll(im, 2 + s, axis=1).astype(np.float64) + rng.normal(0, 3.0, im.shape), 0, 255).astype(np.uint8) for im in (l, r)))
    return kf, fr


def scene(oracle, synth, levelsup=1, nnratio=0.7, check_ori=1, weights=True):
    """9 pairs over 3 rigs: each frame against its own KeyFrame, an unrelated KeyFrame, an empty right row, an empty left row, an empty
    KeyFrame row, the two cameras swapped, a row out of range.  levelsup 1: about 100 nodes; levelsup 2: 10 nodes, buckets of about 100."""
    key = ("scene", levelsup)
    if key not in _cache:
        if "extracted" not in _cache:
            ex = oracle.Extractor(NF, 1.2, 8, 20, 7)
            voc = oracle.Vocabulary(scene_tree(synth))

            def feats(img):
                _, k, dsc, _ = ex(img, (0, 0))
                return np.ascontiguousarray(k).view(KP_DTYPE).reshape(-1).copy(), np.ascontiguousarray(dsc, np.uint8).reshape(-1, 32).copy()
            kf_imgs, f_imgs = scene_images(synth)
            flat = np.full((H, W), 128, np.uint8)
            _cache["extracted"] = (voc, [(feats(l), feats(r)) for l, r in kf_imgs], [feats(im) for im in [p[0] for p in f_imgs] + [p[1] for p in f_imgs] + [flat]])
        voc, kf_feats, f_feats = _cache["extracted"]
        rng = np.random.default_rng(17 + levelsup)

        def nodes(dsc):
            if len(dsc) == 0:
                return np.zeros(0, np.int32), np.zeros(0, np.float64)
            t = voc.transform(dsc, levelsup)
            return t[3].copy(), t[4].copy()
        krows = []
        for (kl, dl), (kr, dr) in kf_feats:                                     # one stacked row: left features then right
            k = np.concatenate([kl, kr]); dsc = np.concatenate([dl, dr])
            nd, wt = nodes(dsc)
            krows.append((k, dsc, nd, wt, (rng.random(len(k)) < 0.8).astype(np.uint8)))
        krows.append((np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), np.zeros(0, np.int32), np.zeros(0, np.float64), np.zeros(0, np.uint8)))
        frows = [(k, dsc) + nodes(dsc) for k, dsc in f_feats]
        K = make_pool(krows, max(len(r[0]) for r in krows) + 3, True)
        Fp = make_pool(frows, max(len(r[0]) for r in frows) + 5, False)
        assert Fp["counts"][6] == 0 and Fp["counts"][:6].min() > 200 and Fp["counts"].max() <= 600
        #          own KeyFrame    unrelated  empty right  empty left  empty KF  swapped  out of range
        kf_row = [0, 1, 2,         0,         1,           1,          3,        2,       7]
        fl_row = [0, 1, 2,         1,         1,           6,          0,        5,       0]
        fr_row = [3, 4, 5,         4,         6,           4,          3,        2,       3]
        _cache[key] = Batch("scene_l%d" % levelsup, K, Fp, kf_row, fl_row, fr_row, 0.7, 1, True,
                            ["own0", "own1", "own2", "unrelated", "empty_right", "empty_left", "empty_kf", "swapped", "out_of_range"])
    return _cache[key].with_params(nnratio, check_ori, weights)
