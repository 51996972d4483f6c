"""M10 SearchForTriangulation_ batched on the device (orbm_search_for_triangulation_batch_async).  Every pair's row and count must equal the
host entry point orbm_search_for_triangulation AND the oracle's SearchForTriangulation; everything compared is integer and index work,
so bit-exact.  The scene is the suite's rectified synthetic stereo pair at the CreateNewMapPoints shape (752 x 480, 1200 features): one
KeyFrame against N neighbour views, each with its own F12 and epipole (tests/test_triangulation_batch_rule_cpu.py: make_scene).  Buckets
come from desc[:, 0] & (2^bits - 1).

Conditions asserted on the oracle alone keep the cases from being vacuous: >= 80 matches per pair in every gate-on case with a has_mp
share <= 0.5 (read as: cases that search all features, only_stereo off -- with only_stereo on and no stereo feature the search matches
nothing by definition, and that case asserts exactly that), >= 1 match at share 0.95, an epipole gate that changes a result, an epipolar
gate that rejects a best-distance candidate whose idx1 still matches, and a tie won by the higher idx2."""
import ctypes as C

import numpy as np
import pytest

from test_triangulation_batch_rule_cpu import (H, NF, W, apply_cross_pair_rule, fv, levels, make_scene, nodes_of, ref_pair, rule_case,
                                               sequential)

pytestmark = pytest.mark.gpu

NNEIGH = 12
NAME = "orbm_search_for_triangulation_batch_async"


class Pool:
    """Rows of cap slots laid out by the test: the arrays of one pool on the device and their host copies.  Slots beyond a row's count
    hold garbage that would match if it were read (the descriptor of slot 0, node of slot 0, no MapPoint)."""

    def __init__(self, pkg, rows, cap, bits, mp=None, ur=None, weight=None):
        self.pkg, self.rows, self.cap, self.n = pkg, len(rows), cap, [len(k) for k, _ in rows]
        self.k = np.zeros((self.rows, cap), pkg.KP_DTYPE); self.d = np.zeros((self.rows, cap, 32), np.uint8)
        self.node = np.zeros((self.rows, cap), np.int32); self.mp = np.zeros((self.rows, cap), np.uint8)
        self.ur = None if ur is None else np.full((self.rows, cap), 5.0, np.float32)
        self.w = None if weight is None else np.ones((self.rows, cap), np.float64)
        for r, (k, d) in enumerate(rows):
            n = len(k)
            if n:
                self.k[r, :] = k[0]; self.d[r, :] = d[0]
                self.k[r, :n] = k; self.d[r, :n] = d
                self.node[r] = nodes_of(self.d[r], bits)
            if mp is not None:
                self.mp[r, :n] = mp[r]
            if ur is not None:
                self.ur[r, :n] = ur[r]
            if weight is not None:
                self.w[r, :n] = weight[r]
        self.upload()

    def upload(self):
        up = lambda a: self.pkg.DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a))
        self.dk, self.dd, self.dn, self.dm = up(self.k), up(self.d), up(self.node), up(self.mp)
        self.dc = up(np.asarray(self.n, np.int32))
        self.du = None if self.ur is None else up(self.ur)
        self.dw = None if self.w is None else up(self.w)

    def args(self):
        return (self.rows, self.cap, self.dk.ptr, self.dd.ptr, self.dc.ptr, self.dn.ptr, None if self.dw is None else self.dw.ptr, self.dm.ptr,
                None if self.du is None else self.du.ptr)

    def host(self, r):
        """(kps, desc, nodes, keep, has_mp, uright) of row r as the host entry point takes them."""
        n = self.n[r]
        keep = np.ones(n, bool) if self.w is None else self.w[r, :n] > 0
        return (np.ascontiguousarray(self.k[r, :n]), np.ascontiguousarray(self.d[r, :n]), self.node[r, :n], keep, self.mp[r, :n],
                None if self.ur is None else np.ascontiguousarray(self.ur[r, :n]))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(pkg, mt, A, B, row1, row2, F, ep, sf, sig, nlevels=8, only_stereo=0, coarse=0, check_ori=0, out=None):
    L = pkg.lib()
    P = len(F)
    d1 = None if row1 is None else pkg.DeviceBuffer(4 * P).upload(np.asarray(row1, np.int32))
    d2 = None if row2 is None else pkg.DeviceBuffer(4 * P).upload(np.asarray(row2, np.int32))
    dF = pkg.DeviceBuffer(36 * P).upload(np.ascontiguousarray(F, np.float32)); de = pkg.DeviceBuffer(8 * P).upload(np.ascontiguousarray(ep, np.float32))
    mm, nm = out or (pkg.DeviceBuffer(4 * P * A.cap).upload(np.full(P * A.cap, -7, np.int32)), pkg.DeviceBuffer(4 * P).upload(np.full(P, -7, np.int32)))
    rc = getattr(L, NAME)(mt.h, P, *A.args(), *B.args(), None if d1 is None else d1.ptr, None if d2 is None else d2.ptr, dF.ptr, de.ptr,
                          _p(sf), _p(sig), nlevels, int(only_stereo), int(coarse), int(check_ori), mm.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()
    assert L.orbm_sync(mt.h) == 0, L.orbm_last_error()
    return mm.download(np.int32, P * A.cap).reshape(P, A.cap), nm.download(np.int32, P)


def check(oracle, mt, A, B, row1, row2, F, ep, sf, sig, rows, counts, only_stereo=0, coarse=0, check_ori=0, mp2_extra=None, host=True):
    """Every pair against orbm_search_for_triangulation and the oracle; returns the oracle's count per pair."""
    OM = oracle._oracle_matcher_class()()
    got = []
    for p in range(len(F)):
        r1 = p if row1 is None else row1[p]; r2 = p if row2 is None else row2[p]
        if not (0 <= r1 < A.rows and 0 <= r2 < B.rows) or A.n[r1] == 0 or B.n[r2] == 0:
            assert counts[p] == 0 and np.all(rows[p] == -1), p
            got.append(0)
            continue
        k1, d1, nd1, keep1, mp1, ur1 = A.host(r1); k2, d2, nd2, keep2, mp2, ur2 = B.host(r2)
        if mp2_extra is not None:
            mp2 = mp2 | mp2_extra[r2][:len(mp2)]
        a = (k1, d1, nd1, keep1, mp1, ur1, k2, d2, nd2, keep2, mp2, ur2, F[p], ep[p], sf, sig, only_stereo, coarse, check_ori)
        n_ref, m_ref = ref_pair(OM, *a)
        if host:
            n_h, m_h = ref_pair(mt, *a)
            assert n_h == n_ref and np.array_equal(m_h, m_ref), ("host vs oracle", p)
        assert counts[p] == n_ref, ("count", p, counts[p], n_ref)
        assert np.array_equal(rows[p, :len(k1)], m_ref), ("row", p, np.flatnonzero(rows[p, :len(k1)] != m_ref)[:8])
        assert np.all(rows[p, len(k1):] == -1), p
        got.append(n_ref)
    return np.array(got)


@pytest.fixture(scope="module")
def sc(oracle, synth):
    return make_scene(oracle, synth, 100, NNEIGH)


@pytest.fixture(scope="module")
def mt(pkg):
    m = pkg.ORBmatcher(0.6)
    yield m
    m.close()


def _masks(sc, s1, s2, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(len(sc["k1"])) < s1).astype(np.uint8), [(rng.random(len(k)) < s2).astype(np.uint8) for k, _ in sc["neigh"]]


def _pools(pkg, sc, bits, mp1=None, mp2s=None, ur1=None, ur2s=None, w1=None, w2s=None, cap1=1500, cap2=1400):
    """Pool 1: the KeyFrame (row 0) and neighbour 0 (row 1, never named); pool 2: the neighbours.  cap1 != cap2."""
    k1, d1 = sc["k1"], sc["d1"]; n0 = sc["neigh"][0]
    z = lambda n: np.zeros(n, np.uint8)
    A = Pool(pkg, [(k1, d1), n0], cap1, bits, mp=[z(len(k1)) if mp1 is None else mp1, z(len(n0[0]))],
             ur=None if ur1 is None else [ur1, np.full(len(n0[0]), -1, np.float32)], weight=None if w1 is None else [w1, np.ones(len(n0[0]))])
    B = Pool(pkg, sc["neigh"], cap2, bits, mp=mp2s, ur=ur2s, weight=w2s)
    return A, B


PERM = [(7 * i + 3) % NNEIGH for i in range(NNEIGH)]                         # row2: a permutation of the neighbours


@pytest.mark.parametrize("s1,s2", [(0.0, 0.0), (0.5, 0.5), (0.95, 0.95), (0.0, 0.5), (0.95, 0.0)])
@pytest.mark.parametrize("bits", [4, 6, 8])
def test_one_keyframe_against_its_neighbours(pkg, oracle, sc, mt, bits, s1, s2):
    """The CreateNewMapPoints shape: row1 repeated, row2 a permutation, cap1 != cap2, a different F12 and epipole per pair."""
    mp1, mp2s = _masks(sc, s1, s2, 5000 + bits)                              # masks under which the oracle keeps its floor of 80 (bits 8, 0.5 / 0.5: 88)
    A, B = _pools(pkg, sc, bits, mp1, mp2s)
    sf, sig = levels()
    F, ep = sc["F"][PERM], sc["ep"][PERM]
    for coarse in (0, 1):
        rows, counts = run(pkg, mt, A, B, [0] * NNEIGH, PERM, F, ep, sf, sig, coarse=coarse)
        n = check(oracle, mt, A, B, [0] * NNEIGH, PERM, F, ep, sf, sig, rows, counts, coarse=coarse)
        print("bits %d shares %.2f/%.2f coarse %d: oracle matches per pair %s" % (bits, s1, s2, coarse, n.tolist()))
        if max(s1, s2) <= 0.5 and not coarse:
            assert n.min() >= 80, n
        if max(s1, s2) > 0.5:
            assert n.sum() >= 1, n
        m = rows[rows >= 0]
        assert not np.any(mp1[np.nonzero(rows[:, :len(mp1)] >= 0)[1]]) and m.size == counts.sum()
    # a neighbour searched with another neighbour's geometry finds next to nothing: the per-pair F12 matters in this scene
    if s1 == 0.0 and s2 == 0.0:
        OM = oracle._oracle_matcher_class()()
        k2, d2 = sc["neigh"][8]                                               # shifted by 9 rows, searched with the F12 of the -8 rows view
        wrong = ref_pair(OM, sc["k1"], sc["d1"], nodes_of(sc["d1"], bits), np.ones(len(sc["k1"]), bool), mp1, None, k2, d2, nodes_of(d2, bits),
                         np.ones(len(k2), bool), mp2s[8], None, sc["F"][9], sc["ep"][9], sf, sig)[0]
        assert wrong < 40, wrong


@pytest.mark.parametrize("check_ori", [0, 1])
@pytest.mark.parametrize("coarse", [0, 1])
@pytest.mark.parametrize("only_stereo", [0, 1])
@pytest.mark.parametrize("stereo_share", [0.0, 0.5])
def test_stereo_flags_and_orientation(pkg, oracle, sc, mt, stereo_share, only_stereo, coarse, check_ori):
    rng = np.random.default_rng(77)
    ur1 = np.where(rng.random(len(sc["k1"])) < stereo_share, 5.0, -1.0).astype(np.float32)
    ur2s = [np.where(rng.random(len(k)) < stereo_share, 5.0, -1.0).astype(np.float32) for k, _ in sc["neigh"]]
    A, B = _pools(pkg, sc, 4, ur1=ur1, ur2s=ur2s)
    sf, sig = levels()
    kw = dict(only_stereo=only_stereo, coarse=coarse, check_ori=check_ori)
    rows, counts = run(pkg, mt, A, B, [0] * NNEIGH, PERM, sc["F"][PERM], sc["ep"][PERM], sf, sig, **kw)
    n = check(oracle, mt, A, B, [0] * NNEIGH, PERM, sc["F"][PERM], sc["ep"][PERM], sf, sig, rows, counts, **kw)
    print("stereo %.1f only_stereo %d coarse %d ori %d: oracle matches per pair %s" % (stereo_share, only_stereo, coarse, check_ori, n.tolist()))
    if only_stereo and stereo_share == 0.0:
        assert n.max() == 0 and np.all(rows == -1)                           # bOnlyStereo on monocular KeyFrames: every feature skipped (:1464-1466)
    elif not coarse:
        assert n.min() >= 80, n
    if check_ori and not only_stereo:
        n0 = check(oracle, mt, A, B, [0] * NNEIGH, PERM, sc["F"][PERM], sc["ep"][PERM], sf, sig,
                   *run(pkg, mt, A, B, [0] * NNEIGH, PERM, sc["F"][PERM], sc["ep"][PERM], sf, sig, only_stereo=only_stereo, coarse=coarse),
                   only_stereo=only_stereo, coarse=coarse, host=False)
        assert np.any(n0 > n), (n0, n)                                       # the three-maxima cull removes matches somewhere


@pytest.mark.parametrize("null_weights", [False, True])
def test_stopped_words(pkg, oracle, sc, mt, null_weights):
    """~10 % of the features carry a stopped word (weight 0): in no bucket on either side.  NULL weights: none stopped."""
    rng = np.random.default_rng(5)
    w1 = np.where(rng.random(len(sc["k1"])) < 0.1, 0.0, rng.uniform(0.1, 9.0, len(sc["k1"])))
    w2s = [np.where(rng.random(len(k)) < 0.1, 0.0, 1.5) for k, _ in sc["neigh"]]
    A, B = _pools(pkg, sc, 6, w1=None if null_weights else w1, w2s=None if null_weights else w2s)
    sf, sig = levels()
    rows, counts = run(pkg, mt, A, B, [0] * NNEIGH, PERM, sc["F"][PERM], sc["ep"][PERM], sf, sig)
    n = check(oracle, mt, A, B, [0] * NNEIGH, PERM, sc["F"][PERM], sc["ep"][PERM], sf, sig, rows, counts)
    assert n.min() >= 80, n
    if not null_weights:
        for p in range(NNEIGH):
            i1 = np.flatnonzero(rows[p] >= 0)
            assert np.all(w1[i1] > 0) and np.all(w2s[PERM[p]][rows[p][i1]] > 0)


def test_rows_out_of_range_empty_rows_null_rows_and_one_pair(pkg, oracle, sc, mt):
    k0 = sc["k1"][:0], sc["d1"][:0]
    A = Pool(pkg, [(sc["k1"], sc["d1"]), k0, sc["neigh"][2]], 1300, 6)
    B = Pool(pkg, [sc["neigh"][0], sc["neigh"][1], k0], 1250, 6)
    sf, sig = levels()
    row1 = [0, -1, 0, 3, 1, 0, 2, 0]; row2 = [0, 0, 3, 1, 0, 2, -5, 1]
    sel = [0, 0, 0, 1, 0, 0, 0, 1]
    F, ep = sc["F"][sel], sc["ep"][sel]
    rows, counts = run(pkg, mt, A, B, row1, row2, F, ep, sf, sig)
    n = check(oracle, mt, A, B, row1, row2, F, ep, sf, sig, rows, counts)
    assert n[0] >= 80 and n[7] >= 80 and list(n[1:7]) == [0] * 6, n
    # NULL row arrays: pair p = row p of both pools; and a single pair
    rows, counts = run(pkg, mt, A, B, None, None, sc["F"][[0, 1, 2]], sc["ep"][[0, 1, 2]], sf, sig)
    n = check(oracle, mt, A, B, None, None, sc["F"][[0, 1, 2]], sc["ep"][[0, 1, 2]], sf, sig, rows, counts)
    assert n[0] >= 80 and n[1] == 0 and n[2] == 0
    rows, counts = run(pkg, mt, A, B, [0], [1], sc["F"][[1]], sc["ep"][[1]], sf, sig)
    assert check(oracle, mt, A, B, [0], [1], sc["F"][[1]], sc["ep"][[1]], sf, sig, rows, counts)[0] >= 80


def test_epipole_gate_and_non_finite_epipole(pkg, oracle, sc, mt):
    """An epipole placed exactly on kp2 of a known match (no stereo features) takes that match away; +inf and NaN epipoles compare as
    IEEE does (nothing is closer than the bound) and equal the far epipole's result."""
    A, B = _pools(pkg, sc, 4)
    sf, sig = levels()
    OM = oracle._oracle_matcher_class()()
    k1, d1, nd1, keep1, mp1, _ = A.host(0); k2, d2, nd2, keep2, mp2, _ = B.host(0)
    far = ref_pair(OM, k1, d1, nd1, keep1, mp1, None, k2, d2, nd2, keep2, mp2, None, sc["F"][0], sc["ep"][0], sf, sig)[1]
    i1 = int(np.flatnonzero(far >= 0)[10]); j = int(far[i1])
    on = np.array([k2["x"][j], k2["y"][j]], np.float32)
    near = ref_pair(OM, k1, d1, nd1, keep1, mp1, None, k2, d2, nd2, keep2, mp2, None, sc["F"][0], on, sf, sig)[1]
    assert near[i1] != far[i1]                                               # the gate changes the result (oracle alone)
    ep = np.array([sc["ep"][0], on, [np.inf, np.inf], [np.nan, 240.0], [-np.inf, 3.0]], np.float32)
    F = sc["F"][[0] * 5]
    rows, counts = run(pkg, mt, A, B, [0] * 5, [0] * 5, F, ep, sf, sig)
    n = check(oracle, mt, A, B, [0] * 5, [0] * 5, F, ep, sf, sig, rows, counts)
    assert n.min() >= 80 and rows[1, i1] != rows[0, i1]
    assert np.array_equal(rows[2], rows[0]) and np.array_equal(rows[3], rows[0]) and np.array_equal(rows[4], rows[0])


def test_epipolar_gate_rejects_a_best_candidate_that_then_matches_elsewhere(pkg, oracle, sc, mt):
    A, B = _pools(pkg, sc, 4)
    sf, sig = levels()
    F, ep = sc["F"][[0, 0]], sc["ep"][[0, 0]]
    gate, _ = run(pkg, mt, A, B, [0], [0], F[:1], ep[:1], sf, sig)
    coarse, _ = run(pkg, mt, A, B, [0], [0], F[:1], ep[:1], sf, sig, coarse=1)
    OM = oracle._oracle_matcher_class()()
    k1, d1, nd1, keep1, mp1, _ = A.host(0); k2, d2, nd2, keep2, mp2, _ = B.host(0)
    g = ref_pair(OM, k1, d1, nd1, keep1, mp1, None, k2, d2, nd2, keep2, mp2, None, F[0], ep[0], sf, sig)[1]
    c = ref_pair(OM, k1, d1, nd1, keep1, mp1, None, k2, d2, nd2, keep2, mp2, None, F[0], ep[0], sf, sig, coarse=True)[1]
    moved = np.flatnonzero((g >= 0) & (c >= 0) & (g != c))
    ham = lambda a, b: int(np.unpackbits(a ^ b).sum())
    # the coarse winner is the best distance overall; where the gated run names someone else, that winner failed the epipolar gate
    assert len(moved) >= 1 and all(ham(d1[i], d2[c[i]]) <= ham(d1[i], d2[g[i]]) for i in moved)
    assert np.array_equal(gate[0, :len(g)], g) and np.array_equal(coarse[0, :len(c)], c)


def test_tie_goes_to_the_higher_idx2(pkg, oracle, sc, mt):
    """A pKF2 feature duplicated at a higher index: two gate-passing candidates at the minimum distance, the LAST one wins."""
    sf, sig = levels()
    OM = oracle._oracle_matcher_class()()
    k2, d2 = sc["neigh"][0]
    base = ref_pair(OM, sc["k1"], sc["d1"], nodes_of(sc["d1"], 6), np.ones(len(sc["k1"]), bool), np.zeros(len(sc["k1"]), np.uint8), None, k2, d2,
                    nodes_of(d2, 6), np.ones(len(k2), bool), np.zeros(len(k2), np.uint8), None, sc["F"][0], sc["ep"][0], sf, sig)[1]
    hit = np.flatnonzero(base >= 0)[[3, 50, 90]]
    k2d = np.concatenate([k2, k2[base[hit]]]); d2d = np.concatenate([d2, d2[base[hit]]])
    A = Pool(pkg, [(sc["k1"], sc["d1"])], 1300, 6); B = Pool(pkg, [(k2d, d2d)], 1300, 6)
    rows, counts = run(pkg, mt, A, B, [0], [0], sc["F"][[0]], sc["ep"][[0]], sf, sig)
    n = check(oracle, mt, A, B, [0], [0], sc["F"][[0]], sc["ep"][[0]], sf, sig, rows, counts)
    assert n[0] >= 80
    assert list(rows[0, hit]) == [len(k2), len(k2) + 1, len(k2) + 2]         # the duplicates, not the originals


def test_octave_outside_nlevels_never_matches(pkg, oracle, sc, mt):
    """A few pKF2 features claim octave 9 / -1 while nlevels is 8: they match nothing (the kernels do not index the level tables with
    them).  The expectation is the host result with those features taken out of the search (has_mp2 set)."""
    sf12, sig12 = levels(12)
    A, B = _pools(pkg, sc, 6)
    rows0, _ = run(pkg, mt, A, B, [0] * 3, [0, 1, 2], sc["F"][:3], sc["ep"][:3], sf12[:8].copy(), sig12[:8].copy())
    bad = [np.zeros(B.cap, np.uint8) for _ in range(B.rows)]
    for r in range(3):
        j = rows0[r][rows0[r] >= 0][:12]                                    # features that DO match with their true octave
        B.k["octave"][r, j[:6]] = 9; B.k["octave"][r, j[6:]] = -1
        bad[r][j] = 1
    B.upload()
    rows, counts = run(pkg, mt, A, B, [0] * 3, [0, 1, 2], sc["F"][:3], sc["ep"][:3], sf12[:8].copy(), sig12[:8].copy())
    n = check(oracle, mt, A, B, [0] * 3, [0, 1, 2], sc["F"][:3], sc["ep"][:3], sf12, sig12, rows, counts, mp2_extra=bad)
    assert n.min() >= 80
    for r in range(3):
        assert not np.any(np.isin(rows[r], np.flatnonzero(bad[r])))


def test_equals_the_benchmark_entry_on_its_own_shape(pkg, sc, mt):
    """One F12, no MapPoints, row p against row p, NULL weights: orbm_triangulation_batch_async's rows, entry for entry."""
    L = pkg.lib()
    P, cap = 6, 1300
    rng = np.random.default_rng(3)
    A = Pool(pkg, [(sc["k1"], sc["d1"])] * P, cap, 6, ur=[np.where(rng.random(len(sc["k1"])) < 0.5, 5.0, -1.0).astype(np.float32)] * P)
    B = Pool(pkg, sc["neigh"][:P], cap, 6)
    sf, sig = levels()
    F = np.stack([sc["F"][0]] * P); ep = np.stack([sc["ep"][0]] * P)
    for only_stereo, coarse in ((0, 0), (0, 1)):
        rows, counts = run(pkg, mt, A, B, None, None, F, ep, sf, sig, only_stereo=only_stereo, coarse=coarse)
        mm = pkg.DeviceBuffer(4 * P * cap).upload(np.full(P * cap, -1, np.int32)); nm = pkg.DeviceBuffer(4 * P)
        rc = L.orbm_triangulation_batch_async(mt.h, P, cap, A.dk.ptr, A.dd.ptr, A.dc.ptr, A.dn.ptr, A.du.ptr, B.dk.ptr, B.dd.ptr, B.dc.ptr, B.dn.ptr, None,
                                              _p(F[0]), float(ep[0][0]), float(ep[0][1]), _p(sf), _p(sig), 8, only_stereo, coarse, mm.ptr, nm.ptr)
        assert rc == 0 and L.orbm_sync(mt.h) == 0
        old = mm.download(np.int32, P * cap).reshape(P, cap)
        assert np.array_equal(old, rows) and np.array_equal(nm.download(np.int32, P), counts)
        assert counts[0] >= 80 and counts.sum() > counts[0]                  # pair 0 has the right geometry, the others little


def test_capture_replays_follow_changed_contents(pkg, oracle, synth, sc):
    """One eager call, then a captured graph replayed twice after has_mp1, F12 and row2 changed IN PLACE: the rows follow the new
    contents and nmatches does not accumulate."""
    L = pkg.lib()
    mt = pkg.ORBmatcher(0.6)
    img = synth.gen_image(W, H, 1)
    stride = (W + 63) // 64 * 64
    dev = pkg.DeviceBuffer(stride * H); pad = np.zeros((H, stride), np.uint8); pad[:, :W] = img; dev.upload(pad)
    arr = (C.c_void_p * 1)(dev.ptr)
    ex = pkg.ORBextractor(500, max_size=(W, H), max_batch=1)
    mp1, mp2s = _masks(sc, 0.3, 0.3, 9)
    A, B = _pools(pkg, sc, 6, mp1, mp2s)
    sf, sig = levels()
    P = NNEIGH
    d1 = pkg.DeviceBuffer(4 * P).upload(np.zeros(P, np.int32)); d2 = pkg.DeviceBuffer(4 * P).upload(np.asarray(PERM, np.int32))
    dF = pkg.DeviceBuffer(36 * P).upload(sc["F"][PERM]); de = pkg.DeviceBuffer(8 * P).upload(sc["ep"][PERM])
    mm = pkg.DeviceBuffer(4 * P * A.cap); nm = pkg.DeviceBuffer(4 * P)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    try:
        def enqueue():
            ex.enqueue_device(arr, W, H, stride, np.zeros(4, np.int32))
            assert getattr(L, NAME)(mt.h, P, *A.args(), *B.args(), d1.ptr, d2.ptr, dF.ptr, de.ptr, _p(sf), _p(sig), 8, 0, 0, 1, mm.ptr, nm.ptr) == 0, L.orbm_last_error()

        def fetch():
            ex.sync()
            return mm.download(np.int32, P * A.cap).reshape(P, A.cap), nm.download(np.int32, P)
        enqueue()
        rows_a, counts_a = fetch()
        check(oracle, mt, A, B, [0] * P, PERM, sc["F"][PERM], sc["ep"][PERM], sf, sig, rows_a, counts_a, check_ori=1, host=False)
        assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
        enqueue()
        assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
        # new contents, same buffers: another MapPoint mask, the neighbours in another order with their geometry
        perm2 = PERM[::-1]
        A.mp[0, :len(mp1)] = _masks(sc, 0.6, 0.0, 10)[0]; A.dm.upload(A.mp)
        d2.upload(np.asarray(perm2, np.int32)); dF.upload(sc["F"][perm2]); de.upload(sc["ep"][perm2])
        for _ in range(2):
            mm.upload(np.full(P * A.cap, -7, np.int32))
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            rows_b, counts_b = fetch()
            n = check(oracle, mt, A, B, [0] * P, perm2, sc["F"][perm2], sc["ep"][perm2], sf, sig, rows_b, counts_b, check_ori=1, host=False)
            assert n.min() >= 20 and not np.array_equal(rows_b, rows_a)
    finally:
        assert L.orbm_set_stream(mt.h, None) == 0
        ex.close(); mt.close()


def test_chain_from_the_extractor_block(pkg, oracle, synth):
    """Extractor result block -> orbm_bow_transform_batch_async -> the batched search, on one handle; the rows equal the host path on
    the fetched data.  One pool passed twice: rows [0, P) are the left images, [P, 2P) the right ones."""
    L = pkg.lib()
    P = 3
    pairs = [synth.gen_stereo_pair(W, H, 100 + i) for i in range(P)]
    imgs = [p[0] for p in pairs] + [p[1] for p in pairs]
    stride = (W + 63) // 64 * 64
    dev = pkg.DeviceBuffer(2 * P * stride * H)
    for i, im in enumerate(imgs):
        pad = np.zeros((H, stride), np.uint8); pad[:, :W] = im
        dev.upload(pad, offset=i * stride * H)
    arr = (C.c_void_p * (2 * P))(*[dev.ptr + i * stride * H for i in range(2 * P)])
    ex = pkg.ORBextractor(NF, max_size=(W, H), max_batch=2 * P)
    mt = pkg.ORBmatcher(0.6)
    voc = pkg.ORBVocabulary(mt, synth.gen_vocabulary(10, 3, seed=7))
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    cap = ex.cap
    ex.enqueue_device(arr, W, H, stride, np.zeros(4 * 2 * P, np.int32))
    r = ex.result_device()
    node = pkg.DeviceBuffer(4 * 2 * P * cap); weight = pkg.DeviceBuffer(8 * 2 * P * cap)
    assert L.orbm_bow_transform_batch_async(mt.h, voc.h, r["desc"], 2 * P * cap, 2, None, node.ptr, weight.ptr) == 0, L.orbm_last_error()
    rng = np.random.default_rng(4)
    mp = (rng.random((2 * P, cap)) < 0.5).astype(np.uint8); dmp = pkg.DeviceBuffer(mp.nbytes).upload(mp)
    sf = ex.GetScaleFactors(); sig = ex.GetScaleSigmaSquares()
    F = np.stack([np.array([0, 0, 0, 0, 0, -0.11 * (1 + p), 0, 0.11 * (1 + p), 0], np.float32) for p in range(P)])
    ep = np.array([[1e4, 240.0 + p] for p in range(P)], np.float32)
    row1 = list(range(P)); row2 = [P + p for p in range(P)]
    d1 = pkg.DeviceBuffer(4 * P).upload(np.asarray(row1, np.int32)); d2 = pkg.DeviceBuffer(4 * P).upload(np.asarray(row2, np.int32))
    dF = pkg.DeviceBuffer(36 * P).upload(F); de = pkg.DeviceBuffer(8 * P).upload(ep)
    mm = pkg.DeviceBuffer(4 * P * cap); nm = pkg.DeviceBuffer(4 * P)
    side = (2 * P, cap, r["kps"], r["desc"], r["counts"], node.ptr, weight.ptr, dmp.ptr, None)
    rc = getattr(L, NAME)(mt.h, P, *side, *side, d1.ptr, d2.ptr, dF.ptr, de.ptr, _p(sf), _p(sig), ex.GetLevels(), 0, 0, 0, mm.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()
    ex.sync()
    res = ex.fetch_all()
    rows = mm.download(np.int32, P * cap).reshape(P, cap); counts = nm.download(np.int32, P)
    nd = node.download(np.int32, 2 * P * cap).reshape(2 * P, cap); wt = weight.download(np.float64, 2 * P * cap).reshape(2 * P, cap)
    assert L.orbm_set_stream(mt.h, None) == 0
    OM = oracle._oracle_matcher_class()()
    for p in range(P):
        k1, dd1 = res[p][1], res[p][2]; k2, dd2 = res[P + p][1], res[P + p][2]
        n1, n2 = len(k1), len(k2)
        a = (k1, dd1, nd[p, :n1], wt[p, :n1] > 0, mp[p, :n1], None, k2, dd2, nd[P + p, :n2], wt[P + p, :n2] > 0, mp[P + p, :n2], None, F[p], ep[p], sf, sig)
        n_h, m_h = ref_pair(mt, *a); n_o, m_o = ref_pair(OM, *a)
        assert n_h == n_o == counts[p] and np.array_equal(m_h, m_o) and np.array_equal(rows[p, :n1], m_o) and np.all(rows[p, n1:] == -1), p
        assert n_o >= 80, n_o
    ex.close(); mt.close()


@pytest.mark.parametrize("bits,share", [(4, 0.0), (8, 0.3)])
def test_cross_pair_rule(pkg, oracle, sc, mt, bits, share):
    """one batched call from the initial has_mp1 plus the masking walk equals the neighbour-by-neighbour loop of the
    host entry point and of the oracle, with has_mp1 updated after each pair by a random half of its matches."""
    sf, sig = levels()
    mp1, mp2s, ok = rule_case(50 + bits, sc, share)
    A, B = _pools(pkg, sc, bits, mp1, mp2s)
    ident = list(range(NNEIGH))
    rows, counts = run(pkg, mt, A, B, [0] * NNEIGH, ident, sc["F"], sc["ep"], sf, sig)
    assert counts.min() >= 80
    ruled = apply_cross_pair_rule(rows[:, :len(sc["k1"])], ok)
    OM = oracle._oracle_matcher_class()()
    assert np.array_equal(ruled, sequential(OM, sc, bits, mp1, mp2s, sf, sig, ok, check_ori=False))
    assert np.array_equal(ruled, sequential(mt, sc, bits, mp1, mp2s, sf, sig, ok, check_ori=False))
    assert (ruled != rows[:, :len(sc["k1"])]).sum() > 100


def test_refusals_enqueue_nothing(pkg):
    m = pkg.ORBmatcher()
    L = m.L
    buf = pkg.DeviceBuffer(1 << 16)
    p = buf.ptr
    out = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))
    sf, sig = levels()
    names = ["kps1", "desc1", "counts1", "node1", "has_mp1", "kps2", "desc2", "counts2", "node2", "has_mp2", "F12", "ep", "sf", "sig", "matches12", "nmatches"]

    def call(npairs=1, n1=1, c1=4, n2=1, c2=4, nlevels=8, **null):
        a = {k: (None if k in null else (out.ptr if k in ("matches12", "nmatches") else p)) for k in names}
        a["sf"] = None if "sf" in null else _p(sf); a["sig"] = None if "sig" in null else _p(sig)
        return getattr(L, NAME)(m.h, npairs, n1, c1, a["kps1"], a["desc1"], a["counts1"], a["node1"], None, a["has_mp1"], None,
                                n2, c2, a["kps2"], a["desc2"], a["counts2"], a["node2"], None, a["has_mp2"], None,
                                None, None, a["F12"], a["ep"], a["sf"], a["sig"], nlevels, 0, 0, 1, a["matches12"], a["nmatches"])
    for k in names:
        assert call(**{k: 1}) == -2, k
    for kw in (dict(npairs=0), dict(n1=0), dict(n2=0), dict(c1=0), dict(c2=0), dict(nlevels=0)):
        assert call(**kw) == -2, kw
    assert call(c1=65536) == -3 and b"65535" in L.orbm_last_error()
    assert call(c2=65536) == -3 and call(nlevels=13) == -3 and call(npairs=65536) == -3
    m.sync()
    assert np.all(out.download(np.int32, 16) == 12345)
