"""Inputs shared by the two-camera SearchLocalPoints tests (M3 with Nleft != -1, ORBmatcher.cc:45-239).  Arrays only: the extractor is
handed in, and no matcher of the oracle, the product or a second reading is imported.

Two pools of 8 rows each, 4 left rows then 4 right rows; pair p is left row p and right row 4 + p.
  scene   the pool of tests/fisheye_cases.py (512 x 512 synthetic stereo pairs, at most 1000 features a row): pairs 0 and 1 a stereo
          pair each, pair 2 has an EMPTY right row, pair 3 an EMPTY left row.  l2r / r2l (mvLeftToRightMatch / mvRightToLeftMatch)
          are the mutual nearest descriptors of a pair.
  hand    a few dozen handmade keypoints per camera: every constructed case owns a site of the image (60 px apart, windows are at
          most 12 px wide) with keypoints whose descriptors lie at chosen distances from the case's query.  Pair 0 is (left, right),
          pair 1 (EMPTY, right), pair 2 (left, EMPTY), pair 3 (EMPTY, EMPTY).
A query that the search must skip, and the fields of a camera block it must skip, carry NaN (levels: GARBAGE), so a read of them shows.
"""
import numpy as np

from fisheye_cases import F, FIRST_L, FIRST_R, H, INV_H, INV_W, KP_DTYPE, NLEV, NPAIRS, NROWS, SF, W, _hamming_matrix, pool  # noqa: F401

GARBAGE = 1 << 20                                                              # a level that would index far outside the scale table
LEFT = ("in_view", "px", "py", "view_cos", "level")
RIGHT = ("in_view_r", "pxr", "pyr", "view_cos_r", "level_r")
FIELDS = (("in_view", np.uint8), ("px", np.float32), ("py", np.float32), ("view_cos", np.float32), ("level", np.int32),
          ("in_view_r", np.uint8), ("pxr", np.float32), ("pyr", np.float32), ("view_cos_r", np.float32), ("level_r", np.int32),
          ("depth", np.float32), ("mp_obs", np.uint8))

_cache = {}


def _empty_q(n=0):
    q = {name: np.zeros(n, dt) for name, dt in FIELDS}
    q["qdesc"] = np.zeros((n, 32), np.uint8)
    return q


def mask_skipped(q, th_far=None):
    """NaN / GARBAGE into every field the search must not read: the fields of a camera block that is not in view, the right fields
    other than level_r where level_r == -1 (:172), and everything but in_view* and depth of a far point (:59-60)."""
    q = {k: v.copy() for k, v in q.items()}
    far = np.zeros(len(q["px"]), bool) if th_far is None else (q["depth"] > F(th_far))
    offl = (q["in_view"] == 0) | far; offr = (q["in_view_r"] == 0) | far
    for k in ("px", "py", "view_cos"):
        q[k][offl] = np.nan
    q["level"][offl] = GARBAGE
    for k in ("pxr", "pyr", "view_cos_r"):
        q[k][offr | (q["level_r"] == -1)] = np.nan
    q["level_r"][offr] = GARBAGE
    q["depth"][(q["in_view"] == 0) & (q["in_view_r"] == 0)] = np.nan
    return q


class Case:
    """One search over the 4 pairs of a pool.  Q[p]: the query arrays of pair p (or, with q_shared, one set of qdesc / mp_obs rows
    for every pair: Q[p]["qdesc"] and ["mp_obs"] are then the same arrays, and nq is the same for every pair)."""

    def __init__(self, name, pool_name, Q, cap, counts, th=1.0, nnratio=0.8, th_far=None, q_shared=False, blocked_l=None, blocked_r=None,
                 l2r=None, r2l=None, rule=None, rule_pair=0, host_defined=True):
        self.name, self.pool_name, self.th, self.nnratio, self.th_far = name, pool_name, float(th), float(nnratio), th_far
        self.Q = [mask_skipped(q, th_far) for q in Q]
        self.q_shared, self.cap, self.counts = bool(q_shared), cap, counts
        self.blocked_l = np.zeros((NPAIRS, cap), np.uint8) if blocked_l is None else blocked_l
        self.blocked_r = np.zeros((NPAIRS, cap), np.uint8) if blocked_r is None else blocked_r
        self.l2r = np.full((NPAIRS, cap), -1, np.int32) if l2r is None else l2r
        self.r2l = np.full((NPAIRS, cap), -1, np.int32) if r2l is None else r2l
        self.rule, self.rule_pair, self.host_defined = rule, rule_pair, host_defined
        self.q_stride = max(len(q["px"]) for q in Q) + 5

    def rows(self):
        """The per-query block arrays [NPAIRS][q_stride] (padding rows hold garbage that is never read), nq [NPAIRS]; qdesc and mp_obs
        are [q_stride] rows when q_shared."""
        out = {"nq": np.array([len(q["px"]) for q in self.Q], np.int32)}
        for name, dt in FIELDS:
            a = np.full((NPAIRS, self.q_stride), 77, dt)
            for p, q in enumerate(self.Q):
                a[p, :len(q[name])] = q[name]
            out[name] = a
        d = np.full((NPAIRS, self.q_stride, 32), 0xA5, np.uint8)
        for p, q in enumerate(self.Q):
            d[p, :len(q["qdesc"])] = q["qdesc"]
        out["qdesc"] = d
        if self.q_shared:
            out["qdesc"] = np.ascontiguousarray(d[0]); out["mp_obs"] = np.ascontiguousarray(out["mp_obs"][0])
        return out

    def partners(self, p):
        """(l2r, r2l) of pair p as the search honours them: an entry outside [0, count of the other row) reads as -1."""
        nl, nr = int(self.counts[FIRST_L + p]), int(self.counts[FIRST_R + p])
        a, b = self.l2r[p, :nl].copy(), self.r2l[p, :nr].copy()
        a[(a < 0) | (a >= nr)] = -1; b[(b < 0) | (b >= nl)] = -1
        return a, b


def reference_args(case, p):
    """One pair for a single-pair search that has no depth argument and no level test (host entry point, oracle): the depth gate and a
    level outside [0, NLEV) (-1 on the right is the reference's own) are folded into in_view*; skipped levels are handed over as 0."""
    q = case.Q[p]
    far = np.zeros(len(q["px"]), bool) if case.th_far is None else (q["depth"] > F(case.th_far))
    out = {}
    for names in (LEFT, RIGHT):
        iv, _, _, _, lv = names
        lvl = q[lv].astype(np.int64)
        ok = (q[iv] != 0) & ~far & (((lvl >= 0) & (lvl < NLEV)) | ((lvl == -1) & (lv == "level_r")))
        d = {k2: q[k] for k, k2 in zip(names, LEFT)}
        d["in_view"] = ok.astype(np.uint8); d["level"] = np.where(ok, lvl, 0).astype(np.int32)
        out["left" if names is LEFT else "right"] = d
    l2r, r2l = case.partners(p)
    nl, nr = len(l2r), len(r2l)
    return dict(blocked_l=case.blocked_l[p, :nl], blocked_r=case.blocked_r[p, :nr], l2r=l2r, r2l=r2l, scale_factors=SF, left=out["left"],
                right=out["right"], qdesc=q["qdesc"], mp_obs=q["mp_obs"], th=case.th, nnratio=case.nnratio)


# ------------------------------------------------------------------------------------------------------------------------------
# scene cases
# ------------------------------------------------------------------------------------------------------------------------------
def mutual_nearest(dl, dr, max_dist=60):
    """mvLeftToRightMatch / mvRightToLeftMatch stand-ins: left k and right j name each other when each is the other's nearest descriptor."""
    l2r = np.full(len(dl), -1, np.int32); r2l = np.full(len(dr), -1, np.int32)
    if len(dl) and len(dr):
        hm = _hamming_matrix(dl, dr)
        j = hm.argmin(1); k = hm.argmin(0)
        for a in range(len(dl)):
            if k[j[a]] == a and hm[a, j[a]] <= max_dist:
                l2r[a] = j[a]; r2l[j[a]] = a
    return l2r, r2l


def _scene_queries(rng, kl, dl, kr, dr, nq, obs, flips=6):
    """nq local map points seen near keypoints of the pair: (px, py) near a left keypoint, (pxr, pyr) near the right keypoint whose
    descriptor is nearest to it; levels mostly the keypoint's octave; some points in one camera only, some in neither."""
    ks, ds = (kl, dl) if len(kl) else (kr, dr)
    src = rng.integers(0, len(ks), nq)
    q = _empty_q(nq)
    d = ds[src].copy()
    nflip = rng.integers(0, flips + 1, nq)
    for b in range(flips):
        sel = np.flatnonzero(nflip > b); bit = rng.integers(0, 256, len(sel))
        d[sel, bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)
    q["qdesc"] = d
    if len(kl):
        x, y, lv = kl["x"][src], kl["y"][src], kl["octave"][src]
    else:                                                                      # an empty left row: windows over nothing
        x, y, lv = kr["x"][src] + F(20), kr["y"][src], kr["octave"][src]
    if len(kr):
        if len(kl):
            hm = _hamming_matrix(ds[src], dr)
            j = hm.argmin(1)
            far = hm[np.arange(nq), j] > 80                                    # no counterpart: somewhere else in the right image
            j[far] = rng.integers(0, len(kr), int(far.sum()))
        else:
            j = src
        xr, yr, lvr = kr["x"][j], kr["y"][j], kr["octave"][j]
    else:
        xr, yr, lvr = x - F(20), y, lv
    jit = lambda a, s: (a.astype(np.float32) + rng.normal(0, s, nq)).astype(np.float32)
    q["px"], q["py"], q["pxr"], q["pyr"] = jit(x, 1.0), jit(y, 1.0), jit(xr, 0.7), jit(yr, 0.7)
    up = rng.random(nq) < 0.25
    q["level"] = np.where(up, np.minimum(lv + 1, NLEV - 1), lv).astype(np.int32)
    up = rng.random(nq) < 0.25
    q["level_r"] = np.where(up, np.minimum(lvr + 1, NLEV - 1), lvr).astype(np.int32)
    q["level_r"][rng.random(nq) < 0.05] = -1
    bad = rng.random(nq) < 0.03                                                # levels outside the scale table: the block is skipped
    q["level"][bad] = rng.choice(np.array([-1, NLEV, NLEV + 3, -100], np.int32), int(bad.sum()))
    bad = rng.random(nq) < 0.03
    q["level_r"][bad] = rng.choice(np.array([NLEV, NLEV + 3, -100], np.int32), int(bad.sum()))
    q["view_cos"] = rng.uniform(0.99, 1.0, nq).astype(np.float32); q["view_cos_r"] = rng.uniform(0.99, 1.0, nq).astype(np.float32)
    q["in_view"] = (rng.random(nq) < 0.8).astype(np.uint8); q["in_view_r"] = (rng.random(nq) < 0.7).astype(np.uint8)
    q["depth"] = rng.uniform(1.0, 30.0, nq).astype(np.float32)
    q["mp_obs"] = (rng.random(nq) < obs).astype(np.uint8)
    return q


def _scene_cases(P):
    rows, cap, counts = P["rows"], P["cap"], P["counts"]
    L = [rows[FIRST_L + p] for p in range(NPAIRS)]; R = [rows[FIRST_R + p] for p in range(NPAIRS)]
    l2r = np.full((NPAIRS, cap), -1, np.int32); r2l = np.full((NPAIRS, cap), -1, np.int32)
    for p in range(NPAIRS):
        a, b = mutual_nearest(L[p][1], R[p][1])
        l2r[p, :len(a)] = a; r2l[p, :len(b)] = b

    def base(rng, obs, nq=(420, 380, 300, 250)):
        return [_scene_queries(rng, L[p][0], L[p][1], R[p][0], R[p][1], nq[p], obs) for p in range(NPAIRS)]

    def shared(rng, obs, n_each=150):
        """One map for every pair: n_each points seen by each pair, in view only in the pair that sees them."""
        parts = base(rng, obs, nq=(n_each,) * NPAIRS)
        Q = []
        for p in range(NPAIRS):
            q = {k: np.concatenate([parts[s][k] for s in range(NPAIRS)]) for k in parts[0]}
            other = np.ones(NPAIRS * n_each, bool); other[p * n_each:(p + 1) * n_each] = False
            q["in_view"][other] = 0; q["in_view_r"][other] = 0
            Q.append(q)
        for q in Q[1:]:
            q["qdesc"], q["mp_obs"] = Q[0]["qdesc"], Q[0]["mp_obs"]
        return Q

    def blocked(rng, fracs):
        return np.stack([(rng.random(cap) < f).astype(np.uint8) for f in fracs])

    kw = dict(cap=cap, counts=counts, l2r=l2r, r2l=r2l)
    out = {}
    rng = np.random.default_rng(7301)
    out["scene_th1"] = Case("scene_th1", "scene", base(rng, 0.5), th=1.0, nnratio=0.8, blocked_l=blocked(rng, (0.35,) * 4),
                            blocked_r=blocked(rng, (0.35,) * 4), **kw)
    rng = np.random.default_rng(7302)
    out["scene_th3"] = Case("scene_th3", "scene", base(rng, 1.0), th=3.0, nnratio=0.9, **kw)
    rng = np.random.default_rng(7303)
    out["scene_th1_far"] = Case("scene_th1_far", "scene", base(rng, 1.0), th=1.0, nnratio=0.8, th_far=20.0, **kw)
    rng = np.random.default_rng(7304)
    out["scene_th3_far"] = Case("scene_th3_far", "scene", base(rng, 0.5), th=3.0, nnratio=0.9, th_far=12.5, blocked_l=blocked(rng, (0.35,) * 4),
                                blocked_r=blocked(rng, (0.35,) * 4), **kw)
    # th 10: left windows of a few dozen candidates; with 97 % of a row blocked the TK_K = 8 listed ones run dry
    rng = np.random.default_rng(7305)
    out["scene_th10_blocked"] = Case("scene_th10_blocked", "scene", base(rng, 1.0), th=10.0, nnratio=0.9, blocked_l=blocked(rng, (0.97, 0.35, 0.97, 0.0)),
                                     blocked_r=blocked(rng, (0.35, 0.97, 0.0, 0.97)), **kw)
    # no query has observations: nothing is blocked, slots are taken again and counted again
    rng = np.random.default_rng(7306)
    out["scene_no_obs"] = Case("scene_no_obs", "scene", base(rng, 0.0, nq=(1400, 1200, 300, 250)), th=3.0, nnratio=0.9, **kw)
    rng = np.random.default_rng(7307)
    out["scene_shared"] = Case("scene_shared", "scene", shared(rng, 0.5), th=3.0, nnratio=0.9, q_shared=True, th_far=25.0,
                               blocked_l=blocked(rng, (0.35,) * 4), blocked_r=blocked(rng, (0.35,) * 4), **kw)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the handmade pool and its constructed cases
# ------------------------------------------------------------------------------------------------------------------------------
def _flip(desc, bits):
    """desc with the given bit positions flipped: Hamming distance len(bits) from desc."""
    d = desc.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


class _Hand:
    """Collects the handmade keypoints (left / right) and the constructed cases over them."""

    def __init__(self):
        self.rng = np.random.default_rng(7400)
        self.k = ([], []); self.d = ([], [])
        self.specs = []
        self.nsite = 0

    def site(self):
        """Centre of a fresh site; 60 px from its neighbours."""
        s = self.nsite; self.nsite += 1
        return F(40 + 60 * (s % 8)), F(45 + 60 * (s // 8))

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def kp(self, cam, x, y, qdesc, dist, octave=0, first_bit=0):
        """A keypoint of camera cam (0 left, 1 right) at (x, y) whose descriptor is `dist` bits from qdesc; returns its slot."""
        rec = np.zeros(1, KP_DTYPE)
        rec["x"], rec["y"], rec["size"], rec["octave"], rec["class_id"] = x, y, 31.0, octave, -1
        self.k[cam].append(rec); self.d[cam].append(_flip(qdesc, range(first_bit, first_bit + dist)))
        return len(self.k[cam]) - 1

    def query(self, qdesc, left=None, right=None, obs=1, view_cos=0.5, level_r=0):
        """left / right: the projection (x, y) in that camera, or None = not in view there.  view_cos 0.5: radius 4 at level 0."""
        q = _empty_q(1)
        q["qdesc"][0] = qdesc; q["mp_obs"][0] = obs; q["depth"][0] = 5.0
        if left is not None:
            q["in_view"][0] = 1; q["px"][0], q["py"][0] = left; q["view_cos"][0] = view_cos
        if right is not None:
            q["in_view_r"][0] = 1; q["pxr"][0], q["pyr"][0] = right; q["view_cos_r"][0] = view_cos; q["level_r"][0] = level_r
        return q

    def case(self, name, rule, queries, pair=0, th=1.0, nnratio=0.8, bl=(), br=(), l2r=None, r2l=None, host_defined=True, th_far=None):
        self.specs.append(dict(name=name, rule=rule, queries=queries, pair=pair, th=th, nnratio=nnratio, bl=bl, br=br, l2r=l2r or {}, r2l=r2l or {},
                               host_defined=host_defined, th_far=th_far))

    def finish(self):
        kl = np.concatenate(self.k[0]); kr = np.concatenate(self.k[1])
        dl = np.stack(self.d[0]); dr = np.stack(self.d[1])
        e = (np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8))
        rows = [(kl, dl), e, (kl, dl), e, (kr, dr), (kr, dr), e, e]
        counts = np.array([len(k) for k, _ in rows], np.int32)
        cap = int(counts.max()) + 3
        kps = np.zeros((NROWS, cap), KP_DTYPE); desc = np.zeros((NROWS, cap, 32), np.uint8)
        for r, (k, d) in enumerate(rows):
            kps[r, :len(k)] = k; desc[r, :len(k)] = d
        P = dict(rows=rows, cap=cap, kps=kps, desc=desc, counts=counts)
        out = {}
        for s in self.specs:
            Q = [_empty_q() for _ in range(NPAIRS)]
            if s["queries"]:
                Q[s["pair"]] = {k: np.concatenate([q[k] for q in s["queries"]]) for k in s["queries"][0]}
            bl = np.zeros((NPAIRS, cap), np.uint8); br = np.zeros((NPAIRS, cap), np.uint8)
            bl[:, list(s["bl"])] = 1; br[:, list(s["br"])] = 1
            l2r = np.full((NPAIRS, cap), -1, np.int32); r2l = np.full((NPAIRS, cap), -1, np.int32)
            for k, v in s["l2r"].items():
                l2r[:, k] = v
            for k, v in s["r2l"].items():
                r2l[:, k] = v
            out[s["name"]] = Case(s["name"], "hand", Q, cap, counts, th=s["th"], nnratio=s["nnratio"], blocked_l=bl, blocked_r=br, l2r=l2r, r2l=r2l,
                                  rule=s["rule"], rule_pair=s["pair"], host_defined=s["host_defined"], th_far=s["th_far"])
        return P, out


def _hand():
    h = _Hand()
    # 1. a same-level ratio rejection in the left block (40 > 0.8 * 45) ends the query: the right keypoint 10 bits away stays free
    (x, y), d = h.site(), h.desc()
    h.kp(0, x + 1, y, d, 40); h.kp(0, x - 1, y + 1, d, 45, first_bit=100); h.kp(1, x, y, d, 10)
    h.case("ratio_reject_skips_right", "left_ratio_rejected_right_in_view", [h.query(d, (x, y), (x, y))])
    # 2. an empty left window: the right block still runs
    (x, y), d = h.site(), h.desc()
    h.kp(1, x, y, d, 10)
    h.case("left_empty", "left_empty_right_searched", [h.query(d, (x, y), (x, y)), h.query(d, (-300.0, 2000.0), (x, y), obs=0)])
    # 3. a left best above TH_HIGH
    (x, y), d = h.site(), h.desc()
    h.kp(0, x, y, d, 120); h.kp(1, x, y, d, 10)
    h.case("left_above_th_high", "left_above_th_high_right_searched", [h.query(d, (x, y), (x, y))])
    # 4. a left window whose candidates are all blocked
    (x, y), d = h.site(), h.desc()
    a = h.kp(0, x, y, d, 5); b = h.kp(0, x + 2, y, d, 7); h.kp(1, x, y, d, 10)
    h.case("left_all_blocked", "left_all_blocked_right_searched", [h.query(d, (x, y), (x, y))], bl=(a, b))
    # 5. / 6. / 7. one camera only, neither
    (x, y), d = h.site(), h.desc()
    h.kp(0, x, y, d, 5); h.kp(1, x, y, d, 5)
    h.case("left_only", "left_only", [h.query(d, (x, y), None)])
    h.case("right_only", "right_only", [h.query(d, None, (x, y))])
    h.case("neither", "neither_in_view", [h.query(d, None, None), h.query(d, (x, y), (x, y)), h.query(d, None, None)])
    # 8. level_r == -1: the reference's own skip of the right block
    h.case("level_r_minus_1", "level_r_minus_1", [h.query(d, (x, y), (x, y), level_r=-1)])
    # 9. th 3: the left radius is 12, the right one stays 4 -- a right keypoint 6 px away with the query's own descriptor is not matched
    (x, y), d = h.site(), h.desc()
    h.kp(0, x + 9, y, d, 5); h.kp(1, x + 6, y, d, 0)
    h.case("right_radius_without_th", "right_between_r_and_th_r", [h.query(d, (x, y), (x, y))], th=3.0, nnratio=0.9)
    # 10. an l2r cross write with observations blocks the right slot: for the same query's right block (it takes the other keypoint) and
    # for a later query whose descriptor is that slot's own
    (x, y), d = h.site(), h.desc()
    a = h.kp(0, x, y, d, 5); b = h.kp(1, x, y, d, 3); h.kp(1, x + 2, y, d, 20, octave=1)
    h.case("l2r_blocks", "l2r_cross_blocks", [h.query(d, (x, y), (x, y), level_r=1), h.query(_flip(d, range(3)), None, (x, y), level_r=1)], l2r={a: b})
    # 11. an l2r cross write without observations: the same query's right block claims that same right slot; the query counts 3
    (x, y), d = h.site(), h.desc()
    a = h.kp(0, x, y, d, 5); b = h.kp(1, x, y, d, 3)
    h.case("l2r_open_counts_3", "right_claims_own_cross_slot", [h.query(d, (x, y), (x, y), obs=0)], l2r={a: b})
    # 12. a cross write overwrites the slot an earlier query WITH observations holds
    (x, y), d = h.site(), h.desc()
    a = h.kp(0, x, y, d, 5); b = h.kp(1, x, y, d, 3)
    h.case("cross_overwrites_observed", "cross_overwrote_observed", [h.query(d, None, (x, y)), h.query(d, (x, y), None)], l2r={a: b})
    # 13. r2l cross writes: from a right-only query, and onto the left slot the same query has just claimed
    (x, y), d = h.site(), h.desc()
    a = h.kp(0, x, y, d, 5); b = h.kp(1, x, y, d, 3)
    (x2, y2), d2 = h.site(), h.desc()
    a2 = h.kp(0, x2, y2, d2, 5); b2 = h.kp(1, x2, y2, d2, 3)
    h.case("r2l_cross", "r2l_onto_own_left_claim", [h.query(d, None, (x, y)), h.query(d2, (x2, y2), (x2, y2))], r2l={b: a, b2: a2})
    # 14. - 16. empty rows (pairs 1, 2, 3 of the pool)
    for name, rule, pair in (("empty_left_row", "left_row_empty", 1), ("empty_right_row", "right_row_empty", 2), ("both_rows_empty", "left_row_empty", 3)):
        h.case(name, rule, [h.query(d, (x, y), (x, y)), h.query(d2, (x2, y2), (x2, y2), obs=0)], pair=pair, l2r={a: b, a2: b2}, r2l={b: a, b2: a2})
    # 17. no queries
    h.case("nq0", "no_queries", [])
    # 19. / 20. lists of TK_K = 8 that run dry in a window of 12: one unblocked entry listed (left), none (right)
    (x, y), d = h.site(), h.desc()
    sl = [h.kp(0, x - 2.25 + 1.5 * (i % 4), y - 1.5 + 1.5 * (i // 4), d, i + 1) for i in range(12)]
    (xr, yr), dr = h.site(), h.desc()
    sr_ = [h.kp(1, xr - 2.25 + 1.5 * (i % 4), yr - 1.5 + 1.5 * (i // 4), dr, (i + 1) if i < 11 else 30) for i in range(12)]
    h.case("rescan_left", "left_claims", [h.query(d, (x, y), None)], bl=[s for i, s in enumerate(sl) if i < 8 and i != 4])
    h.case("rescan_right", "right_claims", [h.query(dr, None, (xr, yr))], br=sr_[:10])
    # 18. partner entries in [count, cap): read as -1.  Compared with the reading only (the host form would write past its row).
    (x, y), d = h.site(), h.desc()
    a = h.kp(0, x, y, d, 5); b = h.kp(1, x, y, d, 3)
    h.case("partner_out_of_range", "left_claims", [h.query(d, (x, y), (x, y))], l2r={a: 0}, r2l={b: 0}, host_defined=False)       # (the entries are set below, once the counts are known)
    P, cases = h.finish()
    c = cases["partner_out_of_range"]
    nl, nr = int(P["counts"][FIRST_L]), int(P["counts"][FIRST_R])
    c.l2r[:, a] = nr + 1; c.r2l[:, b] = nl                                     # both < cap = count + 3
    return P, cases


def hand_pool():
    if "hand" not in _cache:
        _cache["hand"] = _hand()
    return _cache["hand"][0]


def pools(oracle, synth):
    return {"scene": pool(oracle, synth), "hand": hand_pool()}


def cases(oracle, synth):
    """name -> Case, in a fixed order: the scene cases, then the constructed ones."""
    if "cases" not in _cache:
        out = _scene_cases(pool(oracle, synth))
        hand_pool()
        out.update(_cache["hand"][1])
        _cache["cases"] = out
    return _cache["cases"]


SCENE_NAMES = ["scene_th1", "scene_th3", "scene_th1_far", "scene_th3_far", "scene_th10_blocked", "scene_no_obs", "scene_shared"]
HAND_NAMES = ["ratio_reject_skips_right", "left_empty", "left_above_th_high", "left_all_blocked", "left_only", "right_only", "neither",
              "level_r_minus_1", "right_radius_without_th", "l2r_blocks", "l2r_open_counts_3", "cross_overwrites_observed", "r2l_cross",
              "empty_left_row", "empty_right_row", "both_rows_empty", "nq0", "rescan_left", "rescan_right", "partner_out_of_range"]
NAMES = SCENE_NAMES + HAND_NAMES
