"""Case sets for the second reading of Frame::ComputeBoW and Frame::isInFrustum (tests/second_reading_frame.py), shared by
tests/test_second_reading_frame_cpu.py (oracle against reading) and tests/test_gpu_frame_second_reading.py (device against reading).
Plain numpy / mpmath; edges are found by stepping in float ulps through the reading's own arithmetic, or by setting an input of the call
(a bound, the cosine limit) to the value the reading computed for a chosen point.  Imports no product code and no oracle."""
import mpmath
import numpy as np

import second_reading_frame as srf

F = np.float32
INF = F(np.inf)

# ---------------------------------------------------------------------------------------------------------------------------
# DBoW2 trees: dicts of k, L, parent, is_leaf, desc, weight (node 0 = the root, parent[i] < i), the arrays orbm_vocab_create takes
# ---------------------------------------------------------------------------------------------------------------------------
TIES = ((3, 17), (15, 16), (0, 30))              # child positions given one descriptor: the earlier one must win
COUNTS = (1, 3, 5, 15, 16, 17, 67)               # descriptor counts: the last wave (4 descriptors) and workgroup (16) partly dead


def _flipped(rng, d, nbits):
    out = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


class _Builder:
    """Nodes are appended in the order the caller walks the tree; a child's descriptor is its parent's with a few bits flipped, so that a
    row near a node is nearer to that node's ancestors than to their siblings and descends to it."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.parent, self.leaf, self.desc, self.weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]

    def add(self, pid, leaf, depth, weight=None):
        rng = self.rng
        d = rng.integers(0, 256, 32, dtype=np.uint8) if depth == 1 else _flipped(rng, self.desc[pid], 24 if depth == 2 else 10)
        self.parent.append(pid); self.leaf.append(1 if leaf else 0); self.desc.append(d)
        self.weight.append(float(rng.uniform(0.1, 9.0)) if weight is None else weight)
        return len(self.parent) - 1

    def children_of(self, pid):
        return [i for i in range(1, len(self.parent)) if self.parent[i] == pid]

    def duplicate(self, pid):
        ch = self.children_of(pid)
        for a, b in TIES:
            if b < len(ch):
                self.desc[ch[b]] = self.desc[ch[a]].copy()

    def tree(self, name, k, L):
        return dict(name=name, k=k, L=L, parent=np.array(self.parent, np.int32), is_leaf=np.array(self.leaf, np.uint8),
                    desc=np.array(self.desc, np.uint8), weight=np.array(self.weight, np.float64))


def regular_tree(k, L, seed):
    """A full k-ary tree of L levels in breadth-first order.  The root, its first child and that child's first child carry the TIES
    duplicates (where they have that many children); a few words are stopped with weight 0 and a few with a negative weight."""
    b = _Builder(seed)
    level = [0]
    for depth in range(1, L + 1):
        nxt = []
        for pid in level:
            for _ in range(k):
                w = None
                if depth == L:
                    r = b.rng.random()
                    w = 0.0 if r < 0.04 else (-float(b.rng.uniform(0.1, 2.0)) if r < 0.07 else None)
                nxt.append(b.add(pid, depth == L, depth, w))
        level = nxt
    pid = 0
    for depth in range(L):
        b.duplicate(pid)
        pid = b.children_of(pid)[0]
    return b.tree("k%d_L%d" % (k, L), k, L)


def hand_tree(all_stopped=False):
    """L = 3, emitted depth-first (a node's subtree before its next sibling: children are NOT contiguous ids).
       root: 31 children -- 0 = A, 1 = B, 2 = C, 3..30 leaves at depth 1; TIES duplicates, so child 30 (a leaf) repeats A's descriptor
       A:    16 children -- 0 = A0 (20 leaves at depth 3), 1..15 leaves at depth 2
       B:    1 child, a leaf at depth 2
       C:    31 leaves at depth 2 with the TIES duplicates
    Leaves at depths 1, 2 and 3 lie side by side under the root."""
    b = _Builder(77)
    w = (lambda: 0.0 if b.rng.random() < 0.7 else -1.5) if all_stopped else (lambda: None)
    for pos in range(31):
        if pos == 0:
            a = b.add(0, False, 1)
            for p2 in range(16):
                if p2 == 0:
                    a0 = b.add(a, False, 2)
                    for _ in range(20):
                        b.add(a0, True, 3, w())
                else:
                    b.add(a, True, 2, w())
        elif pos == 1:
            bb = b.add(0, False, 1)
            b.add(bb, True, 2, w())
        elif pos == 2:
            c = b.add(0, False, 1)
            for _ in range(31):
                b.add(c, True, 2, w())
            b.duplicate(c)
        else:
            b.add(0, True, 1, w())
    b.duplicate(0)
    return b.tree("hand_stopped" if all_stopped else "hand", 31, 3)


def identical_children_tree():
    """L = 1: three leaves with ONE descriptor.  The complement of it is at distance 256 from all three: the first must win."""
    b = _Builder(5)
    first = b.add(0, True, 1)
    for _ in range(2):
        i = b.add(0, True, 1); b.desc[i] = b.desc[first].copy()
    return b.tree("identical", 3, 1)


def magnitudes_tree():
    """L = 1, 20 words whose weights span 18 decades: the order of BowVector::normalize's sum (ascending word id) decides its last bits.
    The 40 rows that bow_features adds on word 2 all carry that word's ONE weight, 0.1: they show addWeight's repeated sum (not 40 * 0.1),
    not its order.  Weights of very different magnitude on one word cannot come out of a tree -- a word has one weight -- so that order
    is pinned on arrays, through orbm_bow_vectors directly (bow_arrays in tests/test_second_reading_frame_cpu.py); the device forms'
    per-feature weights are compared bit for bit, which is all the transform contributes to the sum."""
    b = _Builder(6)
    ws = [1e-9, 1e9, 0.1, 3e-7, 7.0, 1e-3, 123456.789, 5e-9, 2.5e8, 1.0 / 3.0, 1e-9, 9e8, 0.7, 1e-5, 4e4, 6e-8, 3.0, 1e7, 2e-2, 8e-9]
    for wgt in ws:
        b.add(0, True, 1, wgt)
    return b.tree("magnitudes", 20, 1)


def too_many_children_tree():
    b = _Builder(8)
    for _ in range(32):
        b.add(0, True, 1)
    return b.tree("children32", 32, 1)


_TREE_MAKERS = {"k17_L2": lambda: regular_tree(17, 2, 172), "k17_L3": lambda: regular_tree(17, 3, 173), "k20_L2": lambda: regular_tree(20, 2, 202),
                 "k20_L3": lambda: regular_tree(20, 3, 203), "hand": hand_tree, "hand_stopped": lambda: hand_tree(all_stopped=True),
                 "identical": identical_children_tree, "magnitudes": magnitudes_tree}
TREE_NAMES = tuple(_TREE_MAKERS)                 # known when the tests are collected; a tree is built when a test first asks for it
_TREES = {}


def bow_tree(name):
    if name not in _TREES:
        _TREES[name] = _TREE_MAKERS[name]()
        assert _TREES[name]["name"] == name
    return _TREES[name]


def levelsups(L):
    return sorted({0, 1, L - 1, L, L + 2})


def tree_text(tree):
    """The DBoW2 text form of a tree (TemplatedVocabulary.h:1338-1424: `k L scoring weighting`, then `parent isLeaf d0 .. d31 weight`)."""
    lines = ["%d %d 0 0" % (tree["k"], tree["L"])]
    for i in range(1, len(tree["parent"])):
        lines.append("%d %d %s %r" % (tree["parent"][i], tree["is_leaf"][i], " ".join(str(int(x)) for x in tree["desc"][i]), float(tree["weight"][i])))
    return "\n".join(lines) + "\n"


def bow_features(tree, voc):
    """The constructed descriptor rows of one tree (voc = its second reading).  For the root, its first three inner children and the
    first inner child below each of those: an exact copy of every child (distance 0; at the TIES positions two children tie at 0), the copy with one
    bit flipped (ties at 1), and the bitwise complement of every child (distance 256 to it).  Then 24 random rows, and for the magnitudes
    tree 40 copies of word 2.  The rows are dealt round-robin by the depth at which their descent ends, so that the four rows of a wave
    leave at different depths wherever the tree has leaves at different depths."""
    rng = np.random.default_rng(len(tree["parent"]))
    picked, frontier = [0], [0]
    while frontier:
        nxt = []
        for pid in frontier:
            inner = [c for c in voc.nodes[pid].children if not voc.nodes[c].is_leaf()]
            nxt += inner[:3] if pid == 0 else inner[:1]
        picked += nxt
        frontier = nxt
    rows = []
    for pid in picked:
        for c in voc.nodes[pid].children:
            d = voc.nodes[c].descriptor
            rows += [d.copy(), _flipped(rng, d, 1), np.bitwise_not(d)]
    rows += [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(24)]
    if tree["name"] == "magnitudes":
        rows += [tree["desc"][3].copy() for _ in range(40)]                  # node 3 = word 2, weight 0.1
    by_depth = {}
    for r in rows:
        t = srf.transform_one(voc, r, 0)[3]
        depth = [key[1] for key in t if isinstance(key, tuple) and key[0] == "leaf_depth"][0]
        by_depth.setdefault(depth, []).append(r)
    out, lists = [], [by_depth[d] for d in sorted(by_depth)]
    while any(lists):
        for l in lists:
            if l:
                out.append(l.pop(0))
    return np.array(out, np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# isInFrustum
# ---------------------------------------------------------------------------------------------------------------------------
EUROC_K = [458.654, 457.296, 367.215, 248.375]                       # Examples/Monocular/EuRoC.yaml
BOUNDS = [-20.0, 770.0, -15.0, 495.0]
BF = 47.90639384423901
LSF = float(np.log(F(1.2)))
LSF_SMALL = float(np.log(F(1.1)))                                    # mfLogScaleFactor of a pyramid with scale factor 1.1
NLEVELS = 8
POINT_COUNTS = (1, 255, 256, 257)
BIG = 2000


def random_scene(n, seed):
    """The generator of tests/test_gpu_geometry.py: points around a mildly rotated camera, normals scattered about the viewing ray,
    distance ranges that put some points outside on either side."""
    rng = np.random.default_rng(seed)
    Pw = rng.uniform(-6, 6, (n, 3)).astype(F); Pw[:, 2] += 5.0
    ang = rng.uniform(-0.3, 0.3, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).astype(F)
    t = rng.uniform(-0.5, 0.5, 3).astype(F)
    Ow = (-R.T @ t).astype(F)
    d = Pw - Ow
    nm = d / np.linalg.norm(d, axis=1, keepdims=True)
    nm = (nm + rng.normal(0, 0.6, (n, 3))).astype(F)
    nm /= np.linalg.norm(nm, axis=1, keepdims=True)
    dist = np.linalg.norm(d, axis=1).astype(F)
    mx = (dist * rng.uniform(0.6, 4.0, n)).astype(F); mn = (mx / 1.2 ** 7 * rng.uniform(0.5, 1.5, n)).astype(F)
    return dict(pw=Pw, normal=nm.astype(F), min_dist=mn, max_dist=mx, rcw=R.reshape(9), tcw=t, ow=Ow)


class FrustumCase:
    """One call: name, the per-point arrays + camera (`scene`), the call's parameters, and what it must show: expect = minimum counts
    of the reading's branch counters, points = {index: {"in_view": 0 / 1, "proj_set": bool, "level": int, "ambiguous": bool}}."""

    def __init__(self, name, scene, k=EUROC_K, bounds=BOUNDS, bf=BF, cos_limit=0.5, lsf=LSF, nlevels=NLEVELS, expect=None, points=None):
        self.name, self.scene, self.k, self.bounds, self.bf, self.cos_limit, self.lsf, self.nlevels = name, scene, k, bounds, bf, cos_limit, lsf, nlevels
        self.expect, self.points = expect or {}, points or {}

    def args(self, n=None):
        s = self.scene
        n = len(s["pw"]) if n is None else n
        return (s["pw"][:n], s["normal"][:n], s["min_dist"][:n], s["max_dist"][:n], s["rcw"], s["tcw"], s["ow"], self.k, self.bounds, self.bf,
                self.cos_limit, self.lsf, self.nlevels)

    def reading(self, n=None, init=None):
        return srf.is_in_frustum(*self.args(n), init=init)


def _step(x, ulps):
    x = F(x)
    for _ in range(abs(ulps)):
        x = np.nextafter(x, INF if ulps > 0 else -INF)
    return x


def _solve(fn, target, x0, reach=24):
    """The float nearest x0 (within `reach` ulps) with fn(x) == target, or None."""
    for k in range(reach + 1):
        for s in ((0,) if k == 0 else (k, -k)):
            x = _step(x0, s)
            if fn(x) == target:
                return x
    return None


def _point_dists(scene):
    """Each point's `dist` as the reading computes it (Frame.cc:651-653)."""
    return np.array([srf._cv_norm31([F(p[c] - scene["ow"][c]) for c in range(3)]) for p in scene["pw"]], F)


def band(q):
    return srf.AMBIGUITY_FACTOR * srf.AMBIGUITY_UNIT * max(abs(float(q)), 1.0)


def ratios_around(m, lsf=LSF):
    """Float ratios next to q = m: (the nearest below the ambiguous band, those inside it, the nearest above it), by stepping in ulps,
    starting at exp(m * logScaleFactor)."""
    r0 = F(np.exp(m * float(F(lsf))))
    q = lambda r: srf.scale_quotient(r, lsf) - m
    inside, lo, hi = [], None, None
    r = r0
    while lo is None:
        d = q(r)
        if d < -band(d + m): lo = r
        elif abs(d) <= band(d + m): inside.append(r)
        r = _step(r, -1)
    r = _step(r0, 1)
    while hi is None:
        d = q(r)
        if d > band(d + m): hi = r
        elif abs(d) <= band(d + m): inside.append(r)
        r = _step(r, 1)
    return lo, sorted(set(inside)), hi


FRUSTUM_NAMES = ("on_the_four_bounds", "one_ulp_outside_each_bound", "viewCos_on_the_limit", "viewCos_one_ulp_below_the_limit",
                 "distance_and_level_gates", "one_scale_level", "low_clamp_with_a_smaller_scale_factor", "PcZ_around_zero",
                 "PcZ_minus_zero_unreachable")
_FRUSTUM = {}


def frustum_case(name):
    """The constructed case of that name; all of them are built when a test first asks for one, not when the tests are collected."""
    if not _FRUSTUM:
        _FRUSTUM.update((c.name, c) for c in frustum_cases())
        assert tuple(_FRUSTUM) == FRUSTUM_NAMES
    return _FRUSTUM[name]


def frustum_cases():
    base = random_scene(400, 2024)
    out0, _, _ = FrustumCase("base", base).reading()
    acc = [int(i) for i in np.nonzero(out0["in_view"])[0]]
    dists = _point_dists(base)
    cases = []

    # ---- u / v exactly on each of the four bounds (accepted), then every bound moved one ulp inward (the same points rejected) ----
    u, v = out0["proj_x"], out0["proj_y"]
    on = [acc[int(np.argmin(u[acc]))], acc[int(np.argmax(u[acc]))], acc[int(np.argmin(v[acc]))], acc[int(np.argmax(v[acc]))]]
    assert len(set(on)) == 4
    exact = [u[on[0]], u[on[1]], v[on[2]], v[on[3]]]
    cases.append(FrustumCase("on_the_four_bounds", base, bounds=exact,
                             expect={"u_on_minX": 1, "u_on_maxX": 1, "v_on_minY": 1, "v_on_maxY": 1},
                             points={i: {"in_view": 1} for i in on}))
    inward = [_step(exact[0], 1), _step(exact[1], -1), _step(exact[2], 1), _step(exact[3], -1)]
    cases.append(FrustumCase("one_ulp_outside_each_bound", base, bounds=inward,
                             expect={"u_below_minX": 1, "u_above_maxX": 1, "v_below_minY": 1, "v_above_maxY": 1},
                             points={i: {"in_view": 0, "proj_set": False} for i in on}))

    # ---- viewCos equal to the limit (accepted) and one ulp below it ----
    vc = out0["view_cos"]
    j = acc[int(np.argsort(vc[acc])[len(acc) // 2])]
    cases.append(FrustumCase("viewCos_on_the_limit", base, cos_limit=float(vc[j]), expect={"viewCos_on_limit": 1}, points={j: {"in_view": 1}}))
    cases.append(FrustumCase("viewCos_one_ulp_below_the_limit", base, cos_limit=float(_step(vc[j], 1)), expect={"viewCos_below_limit": 1},
                             points={j: {"in_view": 0, "proj_set": True}}))

    # ---- per-point gates on copies of accepted points: the distance range and PredictScale ----
    rows, points = [], {}
    pool = iter(acc * 50)

    def add(i, mn, mx, **want):
        rows.append((base["pw"][i], base["normal"][i], F(mn), F(mx)))
        points[len(rows) - 1] = want

    def place(make, want):
        """Tries accepted points in turn until make(i, dist) finds its (min_dist, max_dist)."""
        for _ in range(200):
            i = next(pool)
            got = make(i, dists[i])
            if got is not None:
                add(i, got[0], got[1], **want)
                return
        raise AssertionError("no accepted point admits " + repr(want))

    def min_for(target):
        return lambda i, d: (lambda m: None if m is None else (m, F(2) * d))(_solve(lambda x: F(F(0.8) * x), target(d), F(d / F(0.8))))

    def max_for(target):
        return lambda i, d: (lambda m: None if m is None else (F(0), m))(_solve(lambda x: F(F(1.2) * x), target(d), F(d / F(1.2))))

    place(min_for(lambda d: d), {"in_view": 1, "tag": "dist_on_min"})
    place(min_for(lambda d: _step(d, 1)), {"in_view": 0, "proj_set": True, "tag": "dist_below_min"})
    place(max_for(lambda d: d), {"in_view": 1, "level": 0, "tag": "dist_on_max"})
    place(max_for(lambda d: _step(d, -1)), {"in_view": 0, "proj_set": True, "tag": "dist_above_max"})

    def ratio_is(r):
        return lambda i, d: (lambda m: None if m is None else (F(0), m))(_solve(lambda x: F(x / d), r, F(r * d)))

    n_amb = 0
    for m in range(NLEVELS):
        lo, inside, hi = ratios_around(m)
        # just outside the band: compared.  Below m the level is m (clamped at 0), above it m + 1 (clamped at the top)
        place(ratio_is(lo), {"in_view": 1, "level": max(m, 0), "ambiguous": False, "tag": "below_band_%d" % m})
        place(ratio_is(hi), {"in_view": 1, "level": min(m + 1, NLEVELS - 1), "ambiguous": False, "tag": "above_band_%d" % m})
        for r in inside:
            if float(r) != 1.0:
                place(ratio_is(r), {"in_view": 1, "ambiguous": m <= NLEVELS - 2, "tag": "inside_band_%d" % m})
                n_amb += m <= NLEVELS - 2
    place(ratio_is(F(1.0)), {"in_view": 1, "level": 0, "ambiguous": False, "tag": "ratio_one"})
    place(ratio_is(F(0.9)), {"in_view": 1, "level": 0, "ambiguous": False, "tag": "below_one"})
    place(ratio_is(F(1.2 ** 9)), {"in_view": 1, "level": NLEVELS - 1, "ambiguous": False, "tag": "clamped_high"})
    place(ratio_is(F(1e6)), {"in_view": 1, "level": NLEVELS - 1, "ambiguous": False, "tag": "clamped_high_far"})
    gates = dict(base, pw=np.array([r[0] for r in rows], F), normal=np.array([r[1] for r in rows], F),
                 min_dist=np.array([r[2] for r in rows], F), max_dist=np.array([r[3] for r in rows], F))
    cases.append(FrustumCase("distance_and_level_gates", gates, points=points,
                             expect={"dist_on_min": 1, "dist_on_max": 1, "dist_below_min": 1, "dist_above_max": 1, "proj_kept_after_reject": 2,
                                     "ambiguous_level": n_amb, "ratio_one_exact": 1, "clamped_high": 3}))
    # (with logScaleFactor = log(1.2f) the low clamp is out of reach here: it needs ceil(q) < 0, q <= -1, ratio <= 1 / 1.2, the distance
    # gate's own edge, and `dist_on_max` lands at q = -0.99999985, whose ceil is -0.  The case after the next one reaches it.)
    one = {i: dict(w, **({"level": 0, "ambiguous": False} if w["in_view"] else {})) for i, w in points.items()}
    cases.append(FrustumCase("one_scale_level", gates, nlevels=1, points=one, expect={"clamped_high": 10}))

    # ---- the low clamp (MapPoint.cc:734).  logScaleFactor is a parameter of the call: with log(1.1f) the ratios between 1 / 1.2 (the
    # distance gate) and 1 / 1.1 have q in (-1.92, -1], ceil(q) = -1, and only the clamp makes the level 0.  Around m = -1 no case is
    # ambiguous: both neighbours of q clamp or round to 0.
    rows, points = [], {}
    lo, inside, hi = ratios_around(-1, LSF_SMALL)
    place(ratio_is(F(0.87)), {"in_view": 1, "level": 0, "ambiguous": False, "tag": "q_near_-1.46"})
    place(ratio_is(F(0.84)), {"in_view": 1, "level": 0, "ambiguous": False, "tag": "q_near_-1.83"})
    place(ratio_is(lo), {"in_view": 1, "level": 0, "ambiguous": False, "tag": "below_band_-1"})
    place(ratio_is(hi), {"in_view": 1, "level": 0, "ambiguous": False, "tag": "above_band_-1"})
    for r in inside:
        place(ratio_is(r), {"in_view": 1, "level": 0, "ambiguous": False, "tag": "inside_band_-1"})
    place(ratio_is(F(1.5)), {"in_view": 1, "level": 5, "ambiguous": False, "tag": "q_near_4.25"})
    place(ratio_is(F(2.0)), {"in_view": 1, "level": NLEVELS - 1, "ambiguous": False, "tag": "q_near_7.27"})
    small = dict(base, pw=np.array([r[0] for r in rows], F), normal=np.array([r[1] for r in rows], F),
                 min_dist=np.array([r[2] for r in rows], F), max_dist=np.array([r[3] for r in rows], F))
    cases.append(FrustumCase("low_clamp_with_a_smaller_scale_factor", small, lsf=LSF_SMALL, points=points, expect={"clamped_low": 3, "clamped_high": 1}))

    # ---- PcZ around zero, under the identity pose: Pc = Pw exactly ----
    den = F(1e-45)                                                           # the smallest subnormal, 2**-149
    assert float(den) == 2.0 ** -149
    z = [  # pw, min_dist, max_dist, expectation
        ((1.0, 0.5, -float(den)), 0.0, 8.0, {"in_view": 0, "proj_set": False}),          # one ulp below 0: rejected at :628
        ((0.0, 0.0, -0.0), 1.0, 8.0, {"in_view": 0, "proj_set": True, "nan": True}),     # the Matx sum from +0 turns -0 into +0; 0 / 0: NaN passes :635-638
        ((0.0, 0.0, 0.0), 1.0, 8.0, {"in_view": 0, "proj_set": True, "nan": True}),
        ((1.0, 0.0, 0.0), 0.0, 8.0, {"in_view": 0, "proj_set": False}),                  # x / +0 = +inf > maxX
        ((-1.0, 0.0, -0.0), 0.0, 8.0, {"in_view": 0, "proj_set": False}),                # PcZ is +0: -inf < minX
        ((0.0, 0.0, float(den)), 0.0, float(den), {"in_view": 1, "level": 0, "ambiguous": False}),      # in view at the principal point, invz = +inf
        ((0.0, 0.0, 1e-40), 0.0, 1e-40, {"in_view": 1, "level": 0, "ambiguous": False}),
        ((1.0, 0.0, 1e-40), 0.0, 8.0, {"in_view": 0, "proj_set": False}),                # fx * 1 / 1e-40 overflows to +inf
        ((0.0, 0.0, 1.0), 0.0, 1.0, {"in_view": 1, "level": 0, "ambiguous": False}),
    ]
    zs = dict(pw=np.array([p[0] for p in z], F), normal=np.tile(np.array([0, 0, 1], F), (len(z), 1)), min_dist=np.array([p[1] for p in z], F),
              max_dist=np.array([p[2] for p in z], F), rcw=np.eye(3, dtype=F).reshape(9), tcw=np.zeros(3, F), ow=np.zeros(3, F))
    cases.append(FrustumCase("PcZ_around_zero", zs, points={i: p[3] for i, p in enumerate(z)},
                             expect={"PcZ_negative": 1, "PcZ_zero": 4, "PcZ_subnormal": 4, "projection_non_finite": 5, "ratio_one_exact": 3}))
    # -0 cannot come out of the Matx rule at all: even a third row and a translation of -0 give PcZ = +0 (s starts at +0)
    neg = dict(zs, rcw=np.array([1, 0, 0, 0, 1, 0, -0.0, -0.0, -0.0], F), tcw=np.array([0, 0, -0.0], F))
    cases.append(FrustumCase("PcZ_minus_zero_unreachable", neg, expect={"PcZ_zero": len(z)}))
    return cases


def exact_projection(case, n=None):
    """The projective value fx * Xc / Zc + cx (and v) in exact arithmetic from the float inputs, and the rounding margin of the float
    expression Frame.cc:621 + Pinhole.cpp:35 around it.  With eps = 2**-24 and to first order:
        Xc: three products, two roundings in the sum (the first add to 0 is exact) and the add of t    |dX| <= 4 eps SX,
            SX = sum |r_0k P_k| + |t_0|  (every partial sum is bounded by SX); dZ likewise
        fx * Xc, / Zc, + cx: one rounding each                                   |du| <= 2 eps |fx Xc / Zc| + eps |u|
        the input errors pass through the quotient                               fx / |Zc| (dX + |Xc / Zc| dZ)
    The sum, times 1.01 for the second-order terms (valid while dZ < |Zc| / 1000; other points get margin = inf), is returned as
    margin_u / margin_v.  Returns (u, v, margin_u, margin_v) as float64 arrays."""
    pw, _, _, _, rcw, tcw, _, k, *_ = case.args(n)
    eps = 2.0 ** -24
    fx, fy, cx, cy = (float(F(x)) for x in k)
    R = [float(x) for x in np.asarray(rcw, F)]; T = [float(x) for x in np.asarray(tcw, F)]
    us, vs, mu, mv = [], [], [], []
    with mpmath.workdps(50):
        for p in np.asarray(pw, F).reshape(-1, 3):
            P = [mpmath.mpf(float(x)) for x in p]
            c = [sum(mpmath.mpf(R[3 * r + i]) * P[i] for i in range(3)) + mpmath.mpf(T[r]) for r in range(3)]
            S = [sum(abs(mpmath.mpf(R[3 * r + i]) * P[i]) for i in range(3)) + abs(mpmath.mpf(T[r])) for r in range(3)]
            d = [4 * eps * s for s in S]
            if c[2] == 0 or d[2] >= abs(c[2]) / 1000:
                us.append(np.nan); vs.append(np.nan); mu.append(np.inf); mv.append(np.inf)
                continue
            u = fx * c[0] / c[2] + cx; v = fy * c[1] / c[2] + cy
            eu = 2 * eps * abs(fx * c[0] / c[2]) + eps * abs(u) + fx / abs(c[2]) * (d[0] + abs(c[0] / c[2]) * d[2])
            ev = 2 * eps * abs(fy * c[1] / c[2]) + eps * abs(v) + fy / abs(c[2]) * (d[1] + abs(c[1] / c[2]) * d[2])
            us.append(float(u)); vs.append(float(v)); mu.append(float(eu * 1.01)); mv.append(float(ev * 1.01))
    return np.array(us), np.array(vs), np.array(mu), np.array(mv)
