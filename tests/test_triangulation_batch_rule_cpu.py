"""The cross-pair rule of INTEGRATION.md for the batched SearchForTriangulation (orbm_search_for_triangulation_batch_async), on the
oracle alone (no GPU): LocalMapping::CreateNewMapPoints searches neighbour after neighbour and the current KeyFrame gains MapPoints in
between, so neighbour i + 1 skips the features that neighbour 0..i triangulated.  Features are independent in M10 (vbMatched2 is not kept,
ORBmatcher.cc:1567) and LocalMapping runs without the orientation check, so ONE search of every neighbour from the has_mp1 state at the
start, followed by a walk over the pairs in order that drops every match whose idx1 an earlier pair triangulated, gives the same rows.
With the orientation check on the rule is not exact: the histogram of a later pair would have been built without the dropped matches.

The module also holds what the GPU tests of the batch share with this one: the scene (one KeyFrame, N neighbour views with their own
F12 / epipole), the per-pair oracle call and the rule itself."""
import numpy as np
import pytest

W, H, NF = 752, 480, 1200
K_CAM = (435.2, 435.2, 367.2, 252.2)                                         # fx, fy, cx, cy
SHIFTS = [0, 3, -4, 7, -2, 5, -6, 1, 9, -8, 4, -1]                           # rows each neighbour view is shifted by (cy2 = cy + shift)


def fundamental(k1, k2, R12, t12):
    """F12 = K1^-T [t12]x R12 K2^-1 (the facade's ComputeF12 product), row-major float32 [9]."""
    def kinv(k):
        fx, fy, cx, cy = k
        return np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], np.float64)
    t = np.asarray(t12, np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)
    return (kinv(k1).T @ tx @ np.asarray(R12, np.float64) @ kinv(k2)).astype(np.float32).reshape(9)


def fv(nodes, keep):
    """FeatureVector CSR as DBoW2 builds it: nodes ascending, indices ascending, only the features with keep set."""
    idx = np.flatnonzero(keep).astype(np.int32)
    order = idx[np.argsort(nodes[idx], kind="stable")]
    un, start = np.unique(nodes[order], return_index=True)
    return un.astype(np.int32), np.append(start, len(order)).astype(np.int32), order.astype(np.int32)


def levels(n=8, f=1.2):
    sf = np.cumprod(np.concatenate([[np.float32(1)], np.full(n - 1, np.float32(f))]).astype(np.float32)).astype(np.float32)
    return sf, (sf * sf).astype(np.float32)


def make_scene(oracle, synth, seed, nneigh, nf=NF):
    """One KeyFrame (the left image of a rectified synthetic stereo pair) and nneigh neighbour views of the same scene: right images of
    growing disparity (a pure sideways motion t12 = (0.11 * (1 + i / 10), 0, 0), R12 = I) whose keypoints are moved down by SHIFTS[i]
    rows, i.e. seen by a camera with cy2 = cy + shift.  Every neighbour has its own F12 (the epipolar line of (x1, y1) is the row y1 +
    shift: a neighbour searched with another neighbour's F12 finds next to nothing) and its own epipole."""
    left, _ = synth.gen_stereo_pair(W, H, seed)
    _, k1, d1, _ = oracle.Extractor(nf)(left, (0, 0))
    neigh, F, ep = [], [], []
    for i in range(nneigh):
        s = SHIFTS[i % len(SHIFTS)]
        _, k2, d2, _ = oracle.Extractor(nf)(synth.gen_stereo_pair(W, H, seed, dmin=2 + i, dmax=40 + 2 * i)[1], (0, 0))
        k2 = k2.copy(); k2["y"] += np.float32(s)
        neigh.append((k2, d2))
        k2cam = (K_CAM[0], K_CAM[1], K_CAM[2], K_CAM[3] + s)
        F.append(fundamental(K_CAM, k2cam, np.eye(3), (0.11 * (1 + i / 10.0), 0, 0)))
        ep.append((1e4 + 500.0 * i, K_CAM[3] + s))
    return dict(k1=k1, d1=d1, neigh=neigh, F=np.stack(F), ep=np.asarray(ep, np.float32))


def nodes_of(desc, bits):
    return (desc[:, 0].astype(np.int32) & ((1 << bits) - 1)).astype(np.int32)


def ref_pair(M, k1, d1, nd1, keep1, mp1, ur1, k2, d2, nd2, keep2, mp2, ur2, F, ep, sf, sig, only_stereo=False, coarse=False, check_ori=False):
    """One pair through a matcher with the host signature (the oracle's or the product's SearchForTriangulation)."""
    return M.SearchForTriangulation(k1, d1, np.ascontiguousarray(mp1, np.uint8), ur1, fv(nd1, keep1), k2, d2, np.ascontiguousarray(mp2, np.uint8), ur2,
                                    fv(nd2, keep2), F, (float(ep[0]), float(ep[1])), sf, sig, only_stereo=bool(only_stereo), coarse=bool(coarse),
                                    check_ori=bool(check_ori))


def apply_cross_pair_rule(rows, succeeded):
    """INTEGRATION.md, CreateNewMapPoints: rows [npairs][n1] from ONE batched call on the initial has_mp1; succeeded(p, idx1) says whether
    the caller's triangulation of that match succeeded (the feature then holds a MapPoint).  Returns the rows the reference's
    neighbour-by-neighbour loop produces."""
    rows = rows.copy()
    taken = np.zeros(rows.shape[1], bool)
    for p in range(rows.shape[0]):
        rows[p, taken] = -1
        for i1 in np.flatnonzero(rows[p] >= 0):
            if succeeded(p, i1):
                taken[i1] = True
    return rows


def sequential(M, sc, bits, mp1, mp2s, sf, sig, succeeded, check_ori):
    """The reference's order: neighbour after neighbour, has_mp1 updated in between."""
    k1, d1 = sc["k1"], sc["d1"]
    nd1 = nodes_of(d1, bits); mp1 = mp1.copy()
    out = []
    for p, (k2, d2) in enumerate(sc["neigh"]):
        _, row = ref_pair(M, k1, d1, nd1, np.ones(len(k1), bool), mp1, None, k2, d2, nodes_of(d2, bits), np.ones(len(k2), bool), mp2s[p], None,
                          sc["F"][p], sc["ep"][p], sf, sig, check_ori=check_ori)
        out.append(row)
        for i1 in np.flatnonzero(row >= 0):
            if succeeded(p, i1):
                mp1[i1] = 1
    return np.stack(out)


def batched_on_oracle(M, sc, bits, mp1, mp2s, sf, sig, check_ori):
    k1, d1 = sc["k1"], sc["d1"]
    nd1 = nodes_of(d1, bits)
    return np.stack([ref_pair(M, k1, d1, nd1, np.ones(len(k1), bool), mp1, None, k2, d2, nodes_of(d2, bits), np.ones(len(k2), bool), mp2s[p], None,
                              sc["F"][p], sc["ep"][p], sf, sig, check_ori=check_ori)[1] for p, (k2, d2) in enumerate(sc["neigh"])])


def rule_case(seed, sc, share):
    rng = np.random.default_rng(seed)
    mp1 = (rng.random(len(sc["k1"])) < share).astype(np.uint8)
    mp2s = [(rng.random(len(k2)) < share).astype(np.uint8) for k2, _ in sc["neigh"]]
    coin = rng.random((len(sc["neigh"]), len(sc["k1"]))) < 0.5
    return mp1, mp2s, (lambda p, i1: bool(coin[p, i1]))


@pytest.fixture(scope="module")
def scene(oracle, synth):
    return make_scene(oracle, synth, 100, 6)


@pytest.mark.parametrize("bits,share", [(4, 0.0), (6, 0.3), (8, 0.3)])
def test_rule_equals_the_sequential_loop(oracle, scene, bits, share):
    OM = oracle._oracle_matcher_class()()
    sf, sig = levels()
    mp1, mp2s, ok = rule_case(11 + bits, scene, share)
    seq = sequential(OM, scene, bits, mp1, mp2s, sf, sig, ok, check_ori=False)
    bat = batched_on_oracle(OM, scene, bits, mp1, mp2s, sf, sig, check_ori=False)
    assert (bat >= 0).sum(1).min() >= 80                                     # every neighbour matches (the issue's floor for shares <= 0.5)
    ruled = apply_cross_pair_rule(bat, ok)
    assert np.array_equal(ruled, seq)
    assert (ruled != bat).sum() > 50                                         # and the rule does drop matches: later pairs repeat earlier idx1


def test_rule_is_not_exact_with_the_orientation_check(oracle, scene):
    """The counter-example.  On the scenes as generated (seeds 100-104, bits 4 / 6 / 8) none was found: nearly every match has rot ~ 0, two
    bins hold them all and the cull never changes.  So the neighbours' keypoint angles are spread over four rotation bins of similar
    size (+60 degrees x (index mod 4)); then which three bins survive depends on which features earlier pairs took away, and masking the
    batch's rows is no longer the sequential result.  The same scene without the check stays exact."""
    OM = oracle._oracle_matcher_class()()
    sf, sig = levels()
    sc = dict(scene)
    sc["neigh"] = []
    for k, d in scene["neigh"]:
        k = k.copy()
        k["angle"] = np.mod(k["angle"] + np.float32(60.0) * (np.arange(len(k)) % 4), np.float32(360.0)).astype(np.float32)
        sc["neigh"].append((k, d))
    mp1, mp2s, ok = rule_case(11 + 4, sc, 0.0)
    seq = sequential(OM, sc, 4, mp1, mp2s, sf, sig, ok, check_ori=True)
    ruled = apply_cross_pair_rule(batched_on_oracle(OM, sc, 4, mp1, mp2s, sf, sig, check_ori=True), ok)
    assert (ruled != seq).sum() > 0
    seq0 = sequential(OM, sc, 4, mp1, mp2s, sf, sig, ok, check_ori=False)
    assert np.array_equal(apply_cross_pair_rule(batched_on_oracle(OM, sc, 4, mp1, mp2s, sf, sig, check_ori=False), ok), seq0)
