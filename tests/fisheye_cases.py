"""Inputs shared by the two-camera motion-model tests (M4 with Nleft != -1, ORBmatcher.cc:2469-2711): one pool of 8 rows -- 4 left rows
then 4 right rows -- from the CPU oracle extractor on 512 x 512 synthetic images (at most 1000 features a row), and a set of
constructed cases over it, each built to reach one rule of the search.  Pair p is left row p and right row 4 + p:
    pair 0, 1   a synthetic stereo pair each (the right image is the left one under a disparity field)
    pair 2      a left image with an EMPTY right row
    pair 3      an EMPTY left row with a right image
Query rows are built around keypoints as _queries of tests/test_gpu_motion_model_batch.py builds them: (u, v) near a left keypoint,
(ur, vr) near the right keypoint whose descriptor is nearest to it.  This file only makes arrays: the extractor is handed in, and no
matcher of the oracle, the product or a second reading is imported."""
import numpy as np

F = np.float32
W = H = 512
NF, NLEV, NROWS, NPAIRS = 900, 8, 8, 4                            # nfeatures 900: the quadtree may return a few more, never above 1000
FIRST_L, FIRST_R = 0, 4
INV_W, INV_H = float(F(64) / F(W)), float(F(48) / F(H))
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
SF = np.cumprod(np.concatenate([[F(1)], np.full(NLEV - 1, F(1.2))]).astype(np.float32)).astype(np.float32)
FIELDS = (("valid", np.uint8), ("u", np.float32), ("v", np.float32), ("ur", np.float32), ("vr", np.float32), ("octave", np.int32),
          ("angle", np.float32), ("mp_obs", np.uint8))

_cache = {}


def images(synth):
    """The 8 images of the pool, in row order."""
    l0, r0 = synth.gen_stereo_pair(W, H, 7100)
    l1, r1 = synth.gen_stereo_pair(W, H, 7101)
    flat = np.full((H, W), 128, np.uint8)                                      # no corner anywhere: an empty row
    return [l0, l1, synth.gen_image(W, H, 7102), flat, r0, r1, flat.copy(), synth.gen_image(W, H, 7103)]


def pool(oracle, synth):
    """rows: [(kps, desc)] * 8; cap; and the block arrays kps [8][cap], desc [8][cap][32], counts [8] (slots past a count hold zeros)."""
    if "pool" not in _cache:
        ex = oracle.Extractor(NF, 1.2, NLEV, 20, 7)
        rows = []
        for img in images(synth):
            _, k, d, _ = ex(img, (0, 0))
            rows.append((np.ascontiguousarray(k).view(KP_DTYPE).reshape(-1).copy(), np.ascontiguousarray(d, np.uint8).reshape(-1, 32).copy()))
        counts = np.array([len(k) for k, _ in rows], np.int32)
        cap = int(counts.max()) + 3                                            # not a multiple of 32: the last blocked word is partial
        kps = np.zeros((NROWS, cap), KP_DTYPE); desc = np.zeros((NROWS, cap, 32), np.uint8)
        for r, (k, d) in enumerate(rows):
            kps[r, :len(k)] = k; desc[r, :len(k)] = d
        _cache["pool"] = dict(rows=rows, cap=cap, kps=kps, desc=desc, counts=counts)
    return _cache["pool"]


def _hamming_matrix(a, b):
    ba = np.unpackbits(a, axis=1).astype(np.float32); bb = np.unpackbits(b, axis=1).astype(np.float32)
    return (ba @ (1 - bb).T + (1 - ba) @ bb.T).astype(np.int32)


def _pair_queries(rng, kl, dl, kr, dr, nq, jitter=1.5, flips=6, own=False):
    """nq LastFrame MapPoints seen near keypoints of the pair: a few flipped descriptor bits, the octave sometimes one off, angles mostly
    consistent (one rotation bin) with strays for the histogram cull.  own: the queries are the left keypoints themselves."""
    if len(kl) == 0:                                                           # an empty left row: the queries sit on the right keypoints
        ks, ds = kr, dr
    else:
        ks, ds = kl, dl
    n = len(ks)
    src = np.arange(nq) % n if own else rng.integers(0, n, nq)
    u = ks["x"][src].astype(np.float32); v = ks["y"][src].astype(np.float32)
    d = ds[src].copy()
    ang = ks["angle"][src].astype(np.float32)
    octv = ks["octave"][src].astype(np.int32)
    if len(kr) and nq:
        if len(kl):
            hm = _hamming_matrix(ds[src], dr)
            j = hm.argmin(1)
            far = hm[np.arange(nq), j] > 80                                    # no counterpart: somewhere else in the right image
            j[far] = rng.integers(0, len(kr), int(far.sum()))
        else:
            j = src
        ur = kr["x"][j].astype(np.float32); vr = kr["y"][j].astype(np.float32)
    else:
        ur = (u - F(20)).astype(np.float32); vr = v.copy()
    if not own:
        u = (u + rng.normal(0, jitter, nq)).astype(np.float32); v = (v + rng.normal(0, jitter, nq)).astype(np.float32)
        ur = (ur + rng.normal(0, jitter, nq)).astype(np.float32); vr = (vr + rng.normal(0, jitter, nq)).astype(np.float32)
        nflip = rng.integers(0, flips + 1, nq)
        for b in range(flips):
            sel = np.flatnonzero(nflip > b); bit = rng.integers(0, 256, len(sel))
            d[sel, bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)
        ang = np.mod(ang + 14.0 + rng.normal(0, 2, nq), 360).astype(np.float32)
        stray = rng.random(nq) < 0.15
        ang[stray] = rng.uniform(0, 360, int(stray.sum())).astype(np.float32)
        up = rng.random(nq) < 0.2
        octv[up] = np.minimum(octv[up] + 1, NLEV - 1)
        dn = rng.random(nq) < 0.1
        octv[dn] = np.maximum(octv[dn] - 1, 0)
    return dict(valid=(rng.random(nq) < 0.85).astype(np.uint8), u=u, v=v, ur=ur, vr=vr, octave=octv, angle=ang, qdesc=d,
                mp_obs=np.ones(nq, np.uint8))


def _free_spots(rng, k, r, n, lo=-40.0, hi=W + 40.0):
    """n points more than r + 1 px (in x or in y) away from every keypoint of k, inside or just outside the image."""
    out = []
    while len(out) < n:
        x, y = rng.uniform(lo, hi, 2)
        if len(k) == 0 or np.all(np.maximum(np.abs(k["x"] - x), np.abs(k["y"] - y)) > r + 1):
            out.append((x, y))
    return np.array(out, np.float32)


def _append(q, extra, rng):
    """q with the rows of `extra` mixed in at random places; returns the merged rows and the new indices of the extra ones."""
    n0, n1 = len(q["u"]), len(extra["u"])
    perm = rng.permutation(n0 + n1)
    out = {key: np.concatenate([q[key], extra[key]])[perm] for key in q}
    where = np.empty(n0 + n1, np.int64); where[perm] = np.arange(n0 + n1)
    return out, np.sort(where[n0:])


class Case:
    def __init__(self, name, Q, th=15.0, dirs=(0, 0, 0, 0), check_ori=True, retry_below=0, blocked_l=None, blocked_r=None, cap=0, meta=None):
        self.name, self.Q, self.th, self.check_ori, self.retry_below = name, Q, float(th), bool(check_ori), int(retry_below)
        self.dirs = np.asarray(dirs, np.uint8)
        self.blocked_l = np.zeros((NPAIRS, cap), np.uint8) if blocked_l is None else blocked_l
        self.blocked_r = np.zeros((NPAIRS, cap), np.uint8) if blocked_r is None else blocked_r
        self.q_stride = max(len(q["u"]) for q in Q) + 5
        self.meta = meta or {}

    def direction(self, p):
        """(forward, backward) of pair p: dir 1 / 2, any other value reads as neither."""
        return int(self.dirs[p]) == 1, int(self.dirs[p]) == 2

    def rows(self):
        """The per-query block arrays [NPAIRS][q_stride] (padding rows hold garbage that is never read) and nq [NPAIRS]."""
        out = {"nq": np.array([len(q["u"]) for q in self.Q], np.int32)}
        for name, dt in FIELDS:
            a = np.full((NPAIRS, self.q_stride), 77, dt)
            for p, q in enumerate(self.Q):
                a[p, :len(q[name])] = q[name]
            out[name] = a
        d = np.full((NPAIRS, self.q_stride, 32), 0xA5, np.uint8)
        for p, q in enumerate(self.Q):
            d[p, :len(q["qdesc"])] = q["qdesc"]
        out["qdesc"] = d
        return out


def cases(oracle, synth):
    """name -> Case, in a fixed order."""
    if "cases" in _cache:
        return _cache["cases"]
    P = pool(oracle, synth)
    rows, cap = P["rows"], P["cap"]
    L = [rows[FIRST_L + p] for p in range(NPAIRS)]; R = [rows[FIRST_R + p] for p in range(NPAIRS)]

    def base(rng, nq=(420, 380, 300, 250), **kw):
        return [_pair_queries(rng, L[p][0], L[p][1], R[p][0], R[p][1], nq[p], **kw) for p in range(NPAIRS)]

    def blocked(rng, fracs):
        return np.stack([(rng.random(cap) < f).astype(np.uint8) for f in fracs])

    out = {}
    # a left window without candidates ends the query: its right window, which holds the query's own descriptor, is never searched
    rng = np.random.default_rng(7201)
    Q = base(rng)
    n_e = 40
    kr0, dr0 = R[0]
    low = np.flatnonzero(kr0["octave"] <= 1)
    j = rng.choice(low, n_e, replace=False)
    spots = _free_spots(rng, L[0][0], 7.0, n_e)
    spots[:6] = [(-300.0, 100.0), (1900.0, 40.0), (250.0, -900.0), (100.0, 1500.0), (-1999.0, -1999.0), (2000.0, 2000.0)]   # left windows off the grid
    extra = dict(valid=np.ones(n_e, np.uint8), u=spots[:, 0].copy(), v=spots[:, 1].copy(), ur=kr0["x"][j].astype(np.float32),
                 vr=kr0["y"][j].astype(np.float32), octave=np.zeros(n_e, np.int32), angle=kr0["angle"][j].astype(np.float32), qdesc=dr0[j].copy(),
                 mp_obs=np.ones(n_e, np.uint8))
    Q[0], idx = _append(Q[0], extra, rng)
    out["empty_left"] = Case("empty_left", Q, th=7.0, cap=cap, meta={"pair": 0, "queries": idx})
    # the mirror: the query's own left keypoint, and a right window without candidates (some of them off the grid)
    rng = np.random.default_rng(7202)
    Q = base(rng)
    kl1, dl1 = L[1]
    low = np.flatnonzero(kl1["octave"] <= 1)
    j = rng.choice(low, n_e, replace=False)
    spots = _free_spots(rng, R[1][0], 7.0, n_e)
    spots[:6] = [(-300.0, 100.0), (1900.0, 40.0), (250.0, -900.0), (100.0, 1500.0), (-1999.0, -1999.0), (2000.0, 2000.0)]
    extra = dict(valid=np.ones(n_e, np.uint8), u=kl1["x"][j].astype(np.float32), v=kl1["y"][j].astype(np.float32), ur=spots[:, 0].copy(),
                 vr=spots[:, 1].copy(), octave=np.zeros(n_e, np.int32), angle=kl1["angle"][j].astype(np.float32), qdesc=dl1[j].copy(),
                 mp_obs=np.ones(n_e, np.uint8))
    Q[1], idx = _append(Q[1], extra, rng)
    out["empty_right"] = Case("empty_right", Q, th=7.0, cap=cap, meta={"pair": 1, "queries": idx})
    # a slot in each camera for one query
    rng = np.random.default_rng(7203)
    out["both"] = Case("both", base(rng), th=15.0, dirs=(1, 2, 0, 0), cap=cap)
    # blocked slots: 97 % of one camera and 35 % of the other; lists of TK_K = 8 run dry in windows that hold more
    rng = np.random.default_rng(7204)
    out["blocked"] = Case("blocked", base(rng), th=30.0, cap=cap, blocked_l=blocked(rng, (0.97, 0.35, 0.35, 0.0)),
                          blocked_r=blocked(rng, (0.35, 0.97, 0.0, 0.97)))
    # queries without observations leave their slot open: it is taken again, and counted again
    rng = np.random.default_rng(7205)
    Q = base(rng, nq=(1400, 1200, 300, 250))
    Q[0]["mp_obs"][:] = 0
    Q[1]["mp_obs"] = (rng.random(len(Q[1]["u"])) < 0.5).astype(np.uint8)
    out["overwrite"] = Case("overwrite", Q, th=15.0, check_ori=False, cap=cap)
    # the rotation check prunes entries of both rows
    rng = np.random.default_rng(7206)
    out["cull"] = Case("cull", base(rng), th=15.0, check_ori=True, cap=cap)
    # Tracking's retry: pair 0 displaced by 1.5 windows at th (few matches at th, many at 2 * th), pair 1 matches at once
    rng = np.random.default_rng(7207)
    Q = base(rng, nq=(150, 380, 300, 250), jitter=0.3)
    for q in Q:
        q["valid"][:] = 1
    shift = (F(1.5 * 7.0) * SF[Q[0]["octave"]]).astype(np.float32)
    Q[0]["u"] = (Q[0]["u"] + shift).astype(np.float32); Q[0]["ur"] = (Q[0]["ur"] + shift).astype(np.float32)
    out["retry"] = Case("retry", Q, th=7.0, retry_below=20, cap=cap, blocked_l=blocked(rng, (0.3,) * 4), blocked_r=blocked(rng, (0.3,) * 4))
    # the level band of each direction, both cameras (7 reads as 0)
    rng = np.random.default_rng(7208)
    out["dir"] = Case("dir", base(rng), th=15.0, dirs=(2, 1, 0, 7), cap=cap)
    # valid rows whose octave lies outside the scale table are skipped
    rng = np.random.default_rng(7209)
    Q = base(rng)
    bad = {}
    for p in (0, 1):
        bad[p] = np.sort(rng.choice(len(Q[p]["u"]), 40, replace=False))
        Q[p]["valid"][bad[p]] = 1
        Q[p]["octave"][bad[p]] = rng.choice(np.array([-1, NLEV, NLEV + 3, -100], np.int32), 40)
    out["octave"] = Case("octave", Q, th=15.0, dirs=(0, 1, 0, 0), cap=cap, meta={"bad": bad})
    # a pair without queries
    rng = np.random.default_rng(7210)
    out["nq0"] = Case("nq0", base(rng, nq=(420, 0, 300, 250)), th=15.0, cap=cap)
    _cache["cases"] = out
    return out


def reference_args(case, p):
    """The keyword arguments of one pair for a single-pair search (host entry point, oracle): a valid row whose octave lies outside
    [0, NLEV) is what the batched call skips, so it is handed over as not valid, with its octave set to 0."""
    q = case.Q[p]
    octv = np.asarray(q["octave"], np.int32)
    valid = ((np.asarray(q["valid"]) != 0) & (octv >= 0) & (octv < NLEV)).astype(np.uint8)
    fwd, bwd = case.direction(p)
    return dict(scale_factors=SF, valid=valid, u=q["u"], v=q["v"], ur=q["ur"], vr=q["vr"], octave=np.where(valid != 0, octv, 0).astype(np.int32),
                angle=q["angle"], qdesc=q["qdesc"], mp_obs=q["mp_obs"], forward=fwd, backward=bwd, check_ori=case.check_ori)
