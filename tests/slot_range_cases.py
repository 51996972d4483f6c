"""Cases at the top of the batched searches' accepted slot range (cap <= 65535 keypoint slots per row): numpy only, no GPU, no oracle, no
product import.  tests/test_slot_range_cpu.py proves from the second reading that the cases are what they claim;
tests/test_gpu_slot_range.py runs the device calls on them with the grid of GridFrame.csr() handed in.

A pool is kps / desc / counts in the [rows][cap] layout of the C ABI on a 1920 x 1080 frame: keypoints uniform, octaves uniform,
descriptors a few base descriptors with up to 40 bits flipped (as synth_pool draws them), slots at and past a row's count filled with
keypoints and descriptors that look just as good (a kernel that reads them matches them).  On top of that a row gets PLANTED keypoints
(plant): their slots, positions, octaves and descriptors are set by hand so that a query has a known outcome on a slot at the top of the
range, in the last word of a (cap + 31) >> 5 word bitmap, in word 1024, or on either side of grid position 32768.

Every planted query sits exactly on a keypoint (`src`), so the searches that project on the device (M5, M6, M13) get it as that
keypoint back-projected (test_gpu_reloc_batch.keyframe with src given) and the others as its coordinates."""
import functools

import numpy as np

import second_reading as sr
import test_gpu_reloc_batch as rl                     # keyframe(), flip(), KCAM, LOG_SF: numpy only
import test_gpu_sim3_projection_batch as s3           # mappoints(): numpy only
from test_fuse_projection_cpu import F32, fuse_project_np, near_integer_level

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
W, H = 1920, 1080
HALF = 32768
CAP_TOP, CAP_HALF = 65535, 32769
PLANT_OCTAVE = 4
TK_K = 8                                               # candidates a *_topk kernel lists per query (orbm_kernels.hip.h)
NQ = 1500
BF = F32(47.90639384423901)


def _inv(n, d):
    return float(np.float32(n) / np.float32(d))


INV_W, INV_H = _inv(64, W), _inv(48, H)
BOUNDS = np.array([0, W, 0, H], np.float32)


class HostPool:
    """kps / desc [R][cap], counts [R] (a count may exceed cap: the calls read min(count, cap)), the scale table, and per row the
    second reading's GridFrame."""

    def __init__(self, kps, desc, counts, nlev, plants):
        self.kps, self.desc, self.counts = kps, desc, np.asarray(counts, np.int32)
        self.R, self.cap = kps.shape
        self.nlev = nlev
        self.sf = (np.float32(1.2) ** np.arange(nlev)).astype(np.float32)
        self.w, self.h, self.inv_w, self.inv_h, self.bounds = W, H, INV_W, INV_H, BOUNDS
        self.plants = plants                                               # row -> plant() dict
        self._grids = {}

    def n(self, r):
        return min(int(self.counts[r]), self.cap)

    def row(self, r):
        n = self.n(r)
        return self.kps[r, :n], self.desc[r, :n]

    def grid(self, r):
        if r not in self._grids:
            k, d = self.row(r)
            self._grids[r] = sr.GridFrame(k, d, 0.0, 0.0, INV_W, INV_H)
        return self._grids[r]

    def csr(self):
        """grid_start [R][3073], grid_idx [R][cap] (zero past the placed entries) and placed [R], from GridFrame.csr()."""
        gs = np.zeros((self.R, 3073), np.int32); gi = np.zeros((self.R, self.cap), np.int32); placed = np.zeros(self.R, np.int32)
        for r in range(self.R):
            s, i = self.grid(r).csr()
            gs[r] = s; gi[r, :len(i)] = i; placed[r] = len(i)
        return gs, gi, placed


def _fresh(rng, n=1):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flipped(d, bits):
    d = np.array(d, np.uint8).copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _draw_row(rng, k, d, n, sf, base, maxflip=40):
    nlev = len(sf)
    k["x"][:n] = rng.uniform(0, W - 1, n); k["y"][:n] = rng.uniform(0, H - 1, n)
    k["angle"][:n] = rng.uniform(0, 360, n); k["octave"][:n] = rng.integers(0, nlev, n)
    k["size"][:n] = 31 * sf[k["octave"][:n]]; k["class_id"][:n] = -1
    d[:n] = rl.flip(rng, base[rng.integers(0, len(base), n)], maxflip)


def _set_kp(k, d, sf, slot, x, y, octave, desc, angle=None):
    k["x"][slot] = x; k["y"][slot] = y; k["octave"][slot] = octave; k["size"][slot] = 31 * sf[octave]
    d[slot] = desc
    if angle is not None:
        k["angle"][slot] = angle


def plant(rng, k, d, n, sf, tie):
    """Lay the planted keypoints into one row of n keypoints (k, d: its kps and desc, changed in place).  Returns the situations:
      top      slots whose keypoint carries a descriptor of its own far from every other: n-1, n-2, 32768, 32767, 0
      runner   the slot one pixel from n-1 whose descriptor is 6 bits from n-1's
      cluster  ten slots on one spot at distances 1 .. 9 and 40 from the descriptor `cluster_q` (more than TK_K of them: with the
               eight best blocked the listed candidates are all blocked and the survivor is cluster[8])
      word1024 two ordinary slots in bitmap word 1024 that the blocked variant blocks
      shared   two slots >= 32768 (where n allows) each wanted by two queries
      tie      (a, b, q): two keypoints of one cell a quarter pixel apart at grid positions 32767 and 32768, each 2 bits from q
    and `blocked`, the slots the blocked variant of a search sets in its blocked / matched array, and `queries`, a list of
    dict(src, desc, what): a query on keypoint src (its coordinates and octave) with descriptor desc."""
    # planted keypoints lie around the principal point of rl.KCAM, where the perturbed pose of keyframe() moves a projection least
    box = lambda: (rng.uniform(200, 560), rng.uniform(120, 380))
    P = dict(n=n, queries=[])
    top = []
    for s in (n - 1, n - 2, HALF, HALF - 1, 0):
        if 0 <= s < n and s not in top:
            top.append(s)
    for s in top:
        _set_kp(k, d, sf, s, *box(), PLANT_OCTAVE, _fresh(rng)[0])
        P["queries"].append(dict(src=s, desc=d[s].copy(), what="top"))
    P["top"] = top
    runner = n - 9
    _set_kp(k, d, sf, runner, k["x"][n - 1] + F32(1.0), k["y"][n - 1] + F32(0.5), PLANT_OCTAVE, _flipped(d[n - 1], range(0, 60, 10)),
            angle=k["angle"][n - 1])
    P["runner"] = runner
    cluster = list(range(n - 20, n - 10))
    cq = _fresh(rng)[0]; cx, cy = box(); perm = rng.permutation(256)
    for j, s in enumerate(cluster):
        _set_kp(k, d, sf, s, cx + 0.1 * j, cy, PLANT_OCTAVE, _flipped(cq, perm[:j + 1] if j < 9 else perm[:40]), angle=k["angle"][cluster[0]])
    P["cluster"], P["cluster_q"] = cluster, cq
    P["queries"].append(dict(src=cluster[0], desc=cq, what="cluster"))
    word1024 = [s for s in (HALF + 2, HALF + 22) if s < n - 40]
    for s in word1024:
        _set_kp(k, d, sf, s, *box(), PLANT_OCTAVE, _fresh(rng)[0])
        P["queries"].append(dict(src=s, desc=d[s].copy(), what="word1024"))
    P["word1024"] = word1024
    shared = [n - 35, n - 36] if n - 36 >= HALF else [n - 1, n - 1]
    for s in set(shared) - set(top):
        _set_kp(k, d, sf, s, *box(), PLANT_OCTAVE, _fresh(rng)[0])
    # same group of 8: two queries side by side on shared[0], the second one closer; different groups of 64: shared[1], the later one closer
    P["queries"].append(dict(src=shared[0], desc=_flipped(d[shared[0]], (1, 2, 3)), what="shared8"))
    P["queries"].append(dict(src=shared[0], desc=_flipped(d[shared[0]], (4,)), what="shared8"))
    P["queries"].append(dict(src=shared[1], desc=_flipped(d[shared[1]], (5, 6)), what="shared64a"))
    P["queries"].append(dict(src=shared[1], desc=d[shared[1]].copy() if shared[1] not in top else _flipped(d[shared[1]], (7,)), what="shared64b"))
    P["shared"] = shared
    P["blocked"] = [n - 1] + cluster[:TK_K] + word1024
    P["tie"] = None
    if tie:
        taken = set(top + [runner] + cluster + word1024 + shared)
        g = sr.GridFrame(k[:n], d[:n], 0.0, 0.0, INV_W, INV_H)
        start, idx = g.csr()
        assert len(idx) > HALF + 1
        cell = int(np.searchsorted(start, HALF, side="right")) - 1           # the cell that holds grid position 32768
        assert start[cell] <= HALF - 1 and start[cell + 1] >= HALF + 1, "grid position 32768 opens a cell: draw the row with another seed"
        a, b = int(idx[HALF - 1]), int(idx[HALF])
        assert a not in taken and b not in taken
        q = _fresh(rng)[0]
        _set_kp(k, d, sf, a, k["x"][a], k["y"][a], PLANT_OCTAVE, _flipped(q, (0, 1)))
        # b moves next to a, towards the middle of their cell, and so stays in it
        gx, gy = float(F32(k["x"][a]) * F32(INV_W)), float(F32(k["y"][a]) * F32(INV_H))
        dx = F32(0.25) if gx < round(gx) else F32(-0.25); dy = F32(0.25) if gy < round(gy) else F32(-0.25)
        _set_kp(k, d, sf, b, k["x"][a] + dx, k["y"][a] + dy, PLANT_OCTAVE - 1, _flipped(q, (2, 3)), angle=k["angle"][a])
        s2, i2 = sr.GridFrame(k[:n], d[:n], 0.0, 0.0, INV_W, INV_H).csr()
        assert np.array_equal(s2, start) and int(i2[HALF - 1]) == a and int(i2[HALF]) == b
        P["tie"] = (a, b, q)
        P["queries"].append(dict(src=a, desc=q, what="tie"))
    return P


@functools.lru_cache(maxsize=None)
def pool(cap, nlev=8):
    """cap 65535: rows of 65535, 32769, 32768, 0 and 70000 (> cap) keypoints and row 0 again; cap 32769: rows of 32769, 32768, 0 and
    row 0 again.  Rows 0 and 1 of the first and row 0 of the second carry plants; the 12-level variant is rows 0 and 3 of the first."""
    rng = np.random.default_rng(cap * 100 + nlev)
    counts = [65535, 32769, 32768, 0, 70000, 65535] if cap == CAP_TOP else [32769, 32768, 0, 32769]
    if nlev != 8:
        counts = [cap, 0]
    R = len(counts)
    sf = (np.float32(1.2) ** np.arange(nlev)).astype(np.float32)
    base = _fresh(rng, 48)
    kps = np.zeros((R, cap), KP_DTYPE); desc = np.zeros((R, cap, 32), np.uint8)
    plants = {}
    for r in range(R):
        _draw_row(rng, kps[r], desc[r], cap, sf, base)                     # every slot, so that the ones past the count look like keypoints
    planted_rows = {CAP_TOP: (0, 1), CAP_HALF: (0,)}[cap] if nlev == 8 else (0,)
    for r in planted_rows:
        n = min(counts[r], cap)
        plants[r] = plant(rng, kps[r], desc[r], n, sf, tie=(n == CAP_TOP))
    if nlev == 8:
        kps[R - 1] = kps[0]; desc[R - 1] = desc[0]; plants[R - 1] = plants[0]
    return HostPool(kps, desc, counts, nlev, plants)


# ---- queries -----------------------------------------------------------------------------------------------------------------------
def _sources(rng, n, nq):
    """Half of the queries on any keypoint, half on the upper half of the slots."""
    return np.concatenate([rng.integers(0, n, nq - nq // 2), rng.integers(n // 2, n, nq // 2)])


def _slots(P, first=8, far=3 * 64):
    """Where the planted queries go in the query row: in order from `first`, the two `shared8` ones in one group of 8, and shared64b
    `far` queries after shared64a (another group of 64)."""
    at, i = [], first
    for q in P["queries"]:
        if q["what"] == "shared64b":
            at.append(at[-1] + far)
        else:
            at.append(i); i += 1
    return at


def planted(P, at, what):
    """The query indices of the planted queries named `what`."""
    return [a for a, q in zip(at, P["queries"]) if q["what"] == what]


def blocked_rows(rng, hp, r, frac, variant):
    """The blocked / matched array of row r [cap]: `frac` of the slots at random, never a planted slot; in the blocked variant the
    plant's `blocked` slots on top."""
    b = (rng.random(hp.cap) < frac).astype(np.uint8)
    P = hp.plants.get(r)
    if P is not None:
        keep = set(P["top"] + [P["runner"]] + P["cluster"] + P["word1024"] + P["shared"]) | (set(P["tie"][:2]) if P["tie"] else set())
        b[sorted(keep)] = 0
        if variant:
            b[P["blocked"]] = 1
    return b


def direct_queries(rng, hp, r, nq=NQ, jitter=1.0, flips=30):
    """Post-projection query arrays of row r, for the searches that are handed them (M3, M4): dict(valid, u, v, level, angle, desc,
    planted_at).  An empty row gets queries on row 0's keypoints."""
    k, d = hp.row(r if hp.n(r) else 0)
    n = len(k)
    src = _sources(rng, n, nq)
    u = (k["x"][src] + rng.normal(0, jitter, nq)).astype(np.float32); v = (k["y"][src] + rng.normal(0, jitter, nq)).astype(np.float32)
    lvl = k["octave"][src].astype(np.int32)
    up = rng.random(nq) < 0.2
    lvl[up] = np.minimum(lvl[up] + 1, hp.nlev - 1)
    ang = np.mod(k["angle"][src] + 14.0 + rng.normal(0, 2, nq), 360).astype(np.float32)
    stray = rng.random(nq) < 0.15
    ang[stray] = rng.uniform(0, 360, int(stray.sum())).astype(np.float32)
    desc = rl.flip(rng, d[src], flips)
    valid = (rng.random(nq) < 0.9).astype(np.uint8)
    at = []
    P = hp.plants.get(r)
    if P is not None and hp.n(r):
        at = _slots(P)
        for i, q in zip(at, P["queries"]):
            s = q["src"]
            u[i], v[i], lvl[i], desc[i], valid[i] = k["x"][s], k["y"][s], PLANT_OCTAVE, q["desc"], 1
            ang[i] = np.float32(np.mod(k["angle"][s] + 14.0, 360))
    return dict(valid=valid, u=u, v=v, level=lvl, angle=ang, desc=desc, planted_at=at)


def projected_queries(rng, hp, r, nq=NQ, maxflip=30):
    """MapPoints for the searches that project on the device (M5, M6, M13): rl.keyframe / s3.mappoints on row r's keypoints (an empty
    row: row 0's), the planted ones among them with mfMaxDistance putting the predicted level at PLANT_OCTAVE.  `excluded` counts the
    queries keyframe() cleared for the PredictScale caveat (near_integer_level)."""
    rr = r if hp.n(r) else 0
    k, d = hp.row(rr)
    src = _sources(rng, len(k), nq)
    P = hp.plants.get(r) if hp.n(r) else None
    at = _slots(P) if P is not None else []
    for i, q in zip(at, P["queries"] if P else []):
        src[i] = q["src"]
    p = s3.mappoints(rng, hp, rr, nq, maxflip=maxflip, src=src)
    for i, q in zip(at, P["queries"] if P else []):
        PO = p["pw"][i].astype(np.float64) - p["ow"].astype(np.float64)
        dist = np.linalg.norm(PO)
        p["mx"][i] = F32(dist * hp.sf[PLANT_OCTAVE] * 1.2 ** -0.5); p["mn"][i] = p["mx"][i] / hp.sf[-1]
        p["normal"][i] = (PO / dist).astype(F32)
        p["qdesc"][i] = q["desc"]; p["valid"][i] = 1
        p["angle"][i] = np.float32(np.mod(k["angle"][q["src"]] + 14.0, 360))
    near = near_integer_level(p["pw"][None], p["mn"][None], p["mx"][None], p["tcw"][None], p["ow"][None], rl.LOG_SF, hp.nlev)[0]
    assert not near[at].any()
    p["excluded"] = int(near.sum()); p["planted_at"] = at
    return p


def proj_m5(hp, p):
    return rl.proj_of(hp, p)


def proj_m6(hp, p, form):
    return s3.proj_of(hp, p, form)


def proj_m13(hp, p):
    return [a[0] for a in fuse_project_np(p["tcw"][None], p["ow"][None], p["pw"][None], p["normal"][None], p["mn"][None], p["mx"][None],
                                          p["valid"][None], rl.KCAM, hp.bounds, BF, rl.LOG_SF, hp.nlev)]


# ---- the calls: what each search is run on, and the second reading's rows ---------------------------------------------------------
def _frames(hp):
    """(row, blocked variant) per frame of the frame-indexed calls (M3, M4): every row of the pool, the repeated last row blocked."""
    return [(r, r == hp.R - 1) for r in range(hp.R)]


def _pairs(hp):
    """(row, blocked variant) per pair of the row-mapped calls (M5, M6, M13)."""
    out = [(0, False), (hp.R - 1, True), (1, False), (hp.R - 2 if hp.cap == CAP_TOP else 2, False), (2, False)]
    if hp.cap == CAP_TOP:
        out += [(3, False), (1, True)]
    return out


M3_TH, M3_NNRATIO = 1.0, 0.9
M4_TH = 7.0
M5_TH, M5_ORB_DIST = 10.0, 100
M6_TH, M6_RATIO = 8, 1.5
M13_TH = 3.0


@functools.lru_cache(maxsize=None)
def m3_case(cap):
    hp = pool(cap)
    rng = np.random.default_rng(300 + cap)
    Q, B, want = [], [], []
    for r, variant in _frames(hp):
        q = direct_queries(rng, hp, r)
        q["view_cos"] = np.full(NQ, 0.9, np.float32)                        # the 4.0 radius
        q["mp_obs"] = (rng.random(NQ) < 0.6).astype(np.uint8)
        q["mp_obs"][q["planted_at"]] = 1
        if q["planted_at"]:                                                 # the first of the two side by side holds no observations: overwritten
            q["mp_obs"][planted(hp.plants[r], q["planted_at"], "shared8")[0]] = 0
        b = blocked_rows(rng, hp, r, 0.2, variant)
        Q.append(q); B.append(b)
        n = hp.n(r)
        want.append(sr.search_by_projection_points(hp.grid(r), b[:n], hp.sf, q["valid"], q["u"], q["v"], np.zeros(NQ, np.float32), q["view_cos"],
                                                   q["level"], q["desc"], q["mp_obs"], M3_TH, M3_NNRATIO) if n else None)
    return dict(hp=hp, frames=_frames(hp), Q=Q, blocked=np.stack(B), want=want)


@functools.lru_cache(maxsize=None)
def m4_case(cap):
    hp = pool(cap)
    rng = np.random.default_rng(400 + cap)
    Q, B, want = [], [], []
    for r, variant in _frames(hp):
        q = direct_queries(rng, hp, r)
        q["invzc"] = rng.uniform(0.02, 0.9, NQ).astype(np.float32)
        q["mp_obs"] = (rng.random(NQ) < 0.6).astype(np.uint8)
        q["mp_obs"][q["planted_at"]] = 1
        if q["planted_at"]:                                                 # the first of the two side by side holds no observations: overwritten
            q["mp_obs"][planted(hp.plants[r], q["planted_at"], "shared8")[0]] = 0
        b = blocked_rows(rng, hp, r, 0.2, variant)
        Q.append(q); B.append(b)
        n = hp.n(r)
        want.append(sr.search_by_projection_frame(hp.grid(r), b[:n], hp.sf, q["valid"], q["u"], q["v"], q["invzc"], q["level"], q["angle"],
                                                  q["desc"], q["mp_obs"], M4_TH, check_ori=True) if n else None)
    return dict(hp=hp, frames=_frames(hp), Q=Q, blocked=np.stack(B), want=want)


def _projected_case(cap, seed, key, nlev=8):
    hp = pool(cap, nlev)
    rng = np.random.default_rng(seed + cap)
    pairs = []
    for r, variant in (_pairs(hp) if nlev == 8 else [(0, False), (1, False), (0, True)]):
        p = projected_queries(rng, hp, r)
        p["row"] = r
        p[key] = blocked_rows(rng, hp, r, 0.2, variant)
        pairs.append(p)
    return hp, pairs


@functools.lru_cache(maxsize=None)
def m5_case(cap, nlev=8):
    hp, pairs = _projected_case(cap, 500, "blocked", nlev)
    want = []
    for p in pairs:
        n = hp.n(p["row"])
        ok, u, v, lvl = proj_m5(hp, p)
        want.append(sr.search_by_projection_kf(hp.grid(p["row"]), p["blocked"][:n], hp.sf, ok, u, v, np.maximum(lvl, 0), p["angle"], p["qdesc"],
                                               M5_TH, M5_ORB_DIST, True) if n else None)
    return dict(hp=hp, pairs=pairs, want=want)


@functools.lru_cache(maxsize=None)
def m6_case(cap, form=0):
    hp, pairs = _projected_case(cap, 600, "matched")
    want = []
    for p in pairs:
        n = hp.n(p["row"])
        ok, u, v, lvl = proj_m6(hp, p, form)
        want.append(sr.search_by_projection_sim3(hp.grid(p["row"]), p["matched"][:n], hp.sf, ok, u, v, np.maximum(lvl, 0), p["qdesc"], M6_TH, M6_RATIO)
                    if n else None)
    return dict(hp=hp, pairs=pairs, want=want, form=form)


@functools.lru_cache(maxsize=None)
def m13_case(cap):
    hp, pairs = _projected_case(cap, 1300, "unused")
    isg = (F32(1) / (hp.sf * hp.sf)).astype(np.float32)
    want = []
    for p in pairs:
        ok, u, v, ur, lvl = proj_m13(hp, p)
        want.append(sr.fuse(hp.grid(p["row"]), hp.sf, isg, ok, u, v, ur, np.maximum(lvl, 0), p["qdesc"], M13_TH, True) if hp.n(p["row"]) else None)
    return dict(hp=hp, pairs=pairs, want=want, isg=isg)


# ---- the batch-count edge: 65535 pairs over a tiny pool -----------------------------------------------------------------------------
NPAIRS_TOP = 65535


@functools.lru_cache(maxsize=None)
def tiny_pool():
    """Four rows of 64 slots (50, 64, 0 and 33 keypoints) on a 1920 x 1080 frame, the keypoints of a row within a few pixels of each
    other so that a handful of queries meets them."""
    rng = np.random.default_rng(77)
    counts = [50, 64, 0, 33]
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    base = _fresh(rng, 4)
    kps = np.zeros((4, 64), KP_DTYPE); desc = np.zeros((4, 64, 32), np.uint8)
    for r in range(4):
        _draw_row(rng, kps[r], desc[r], 64, sf, base, maxflip=20)
        cx, cy = rng.uniform(300, W - 300), rng.uniform(300, H - 300)
        kps[r]["x"] = (cx + rng.uniform(-40, 40, 64)).astype(np.float32); kps[r]["y"] = (cy + rng.uniform(-40, 40, 64)).astype(np.float32)
    return HostPool(kps, desc, counts, 8, {})


@functools.lru_cache(maxsize=None)
def tiny_kinds():
    """Four distinct pair contents (rows 0, 1, 2 = empty, 3; 24 MapPoints each) that the 65535 pairs repeat in turn."""
    hp = tiny_pool()
    rng = np.random.default_rng(78)
    kinds = []
    for r in range(4):
        p = projected_queries(rng, hp, r, nq=24, maxflip=10)
        p["row"] = r
        p["blocked"] = p["matched"] = (rng.random(hp.cap) < 0.2).astype(np.uint8)
        kinds.append(p)
    return hp, kinds


# ---- keypoint sets for the grid builders ------------------------------------------------------------------------------------------
GRID_SIZES = (1, 8192, 8193, 20000, 32768, 32769, 50000, 65535)


LONG_CELLS = (((10, 10), 64), ((20, 30), 65), ((40, 5), 100), ((55, 44), 700))


def grid_descriptors(k, crowded=False):
    """Descriptors for grid_points(n, crowded): one of 48 base descriptors with up to 40 bits flipped; in a crowded cell one base with up
    to 2 bits flipped, so that a window there holds many candidates at equal distance and the grid's visiting order decides."""
    rng = np.random.default_rng(len(k) + 17)
    base = _fresh(rng, 48)
    d = rl.flip(rng, base[rng.integers(0, 48, len(k))], 40)
    if crowded:
        cells = [c for c, _ in LONG_CELLS] if crowded == "several" else [(50, 40)]
        for cx, cy in cells:
            at = np.flatnonzero((np.abs(k["x"] - 30.0 * cx) < 15.01) & (np.abs(k["y"] - 22.5 * cy) < 11.25))
            d[at] = rl.flip(rng, np.repeat(base[:1], len(at), 0), 2)
    return d


@functools.lru_cache(maxsize=None)
def grid_points(n, crowded=False):
    """n keypoints for a grid build on the 1920 x 1080 frame: uniform over a box 40 px wider than the image (negative cells, cells past
    column 63 / row 47: not placed), one in eight on the far edge (x in [1905, 1920) rounds onto column 64, y in [1068.75, 1080) onto
    row 48: not placed), one in eight with x = 15 + 30 c or y = 11.25 + 22.5 c (half-way between two cells: rounds away from zero).
    crowded = True: 2048 of them, on high slots, in one cell.  crowded = "several": cells (10, 10), (20, 30), (40, 5) and (55, 44) hold
    exactly 64, 65, 100 and 700 keypoints (LONG_CELLS), on slots of the upper half: either side of the list length from which the
    build above 32768 keypoints sorts a cell with the whole workgroup, and more than one such cell in a row."""
    rng = np.random.default_rng(9000 + n + (2 if crowded == "several" else int(crowded)))
    k = np.zeros(n, KP_DTYPE)
    x = rng.uniform(-40, W + 40, n); y = rng.uniform(-40, H + 40, n)
    e = rng.random(n) < 0.125
    x[e] = np.where(rng.random(int(e.sum())) < 0.5, rng.uniform(1905, 1920, int(e.sum())), x[e])
    y[e] = np.where(x[e] < 1905, rng.uniform(1068.75, 1080, int(e.sum())), y[e])
    hw = rng.random(n) < 0.125
    x[hw] = 15 + 30 * rng.integers(-1, 65, int(hw.sum()))
    hh = rng.random(n) < 0.0625
    y[hh] = 11.25 + 22.5 * rng.integers(-1, 49, int(hh.sum()))
    if crowded == "several":
        assert n >= 4096
        gx = np.floor(x.astype(np.float32).astype(np.float64) * float(np.float32(INV_W)) + 0.5)
        gy = np.floor(y.astype(np.float32).astype(np.float64) * float(np.float32(INV_H)) + 0.5)
        for (cx, cy), _ in LONG_CELLS:                                        # empty the cells, then fill them to the count
            x[(gx == cx) & (gy == cy)] += 60.0
        slots = n // 2 + rng.permutation(n - n // 2)[:sum(c for _, c in LONG_CELLS)]
        for (cx, cy), c in LONG_CELLS:
            at, slots = slots[:c], slots[c:]
            x[at] = 30.0 * cx + rng.uniform(-10, 10, c); y[at] = 22.5 * cy + rng.uniform(-8, 8, c)
    elif crowded:
        assert n >= 4096
        x[n - 3000:n - 952] = rng.uniform(1500, 1515, 2048); y[n - 3000:n - 952] = rng.uniform(900, 910, 2048)   # cell (50, 40), high slots
    k["x"] = x; k["y"] = y; k["octave"] = rng.integers(0, 8, n); k["angle"] = rng.uniform(0, 360, n); k["class_id"] = -1
    return k


def grid_want(k):
    """(grid_start, grid_idx[:placed], trace) of GridFrame.csr() for keypoints k."""
    g = sr.GridFrame(k, np.zeros((len(k), 32), np.uint8), 0.0, 0.0, INV_W, INV_H)
    s, i = g.csr()
    return s, i, g.trace


# ---- M10: SearchForTriangulation between two pools of cap slots ----------------------------------------------------------------------
M10_F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)       # the epipolar line of (x1, y1) is the row y2 = y1
M10_EP = (W * 0.5, H * 0.5)
M10_NODES = 300                                                          # node ids 0 .. 299: 44 pairs of them share their low byte


def _fv(nodes):
    """FeatureVector CSR as DBoW2 builds it: nodes ascending, indices ascending inside."""
    order = np.argsort(nodes, kind="stable").astype(np.int32)
    un, start = np.unique(nodes[order], return_index=True)
    return un.astype(np.int32), np.append(start, len(order)).astype(np.int32), order


@functools.lru_cache(maxsize=None)
def m10_case(cap):
    """KeyFrame 1 and KeyFrame 2 rows of n = cap keypoints (and an empty row each): feature i of KeyFrame 2 is feature i of KeyFrame 1
    three quarters of a pixel lower with up to 20 descriptor bits flipped and its angle turned (M10_ROTATIONS' shares), both in node
    i's bucket, so the bucket lists run over the whole slot range and node ids above 255 share their low byte with others.  Most
    KeyFrame 1 slots carry a MapPoint: the active ones are about 2000, nine in ten of them on the upper half.  Planted on top:
      own      features n-1, n-2, 32768, 32767 and 0 are active and their partner free: each ends on its own index
      tie      feature n-35 (its partner taken) finds slots 3 and n-1 at equal distance on its row: the last listed, n-1, wins
      taken    features n-15 (last bitmap word) and 32770 (word 1024; the lower one where n is 32769) whose partner carries a MapPoint."""
    n = cap
    rng = np.random.default_rng(1000 + cap)
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    base = _fresh(rng, 48)
    k1 = np.zeros(n, KP_DTYPE); d1 = np.zeros((n, 32), np.uint8)
    _draw_row(rng, k1, d1, n, sf, base)
    k2 = k1.copy(); k2["y"] += F32(0.75)
    k2["angle"] = np.mod(k2["angle"] + rng.choice([0.0, 10.0, 40.0, 100.0, 200.0], n, p=[0.5, 0.2, 0.12, 0.1, 0.08]), 360).astype(np.float32)
    d2 = rl.flip(rng, d1, 20)
    node = rng.integers(0, M10_NODES, n).astype(np.int32)
    mp1 = np.ones(n, np.uint8)
    act = np.concatenate([rng.choice(np.arange(n // 2, n), 1800, replace=False), rng.choice(n // 2, 200, replace=False)])
    mp1[act] = 0
    mp2 = (rng.random(n) < 0.3).astype(np.uint8)
    own = [s for s in (n - 1, n - 2, HALF, HALF - 1, 0) if s < n]
    t = n - 35
    taken = [n - 15, HALF + 2 if HALF + 2 < n - 40 else HALF - 30]
    for s in own + [t] + taken:
        mp1[s] = 0; mp2[s] = 0
        k1["x"][s] = rng.uniform(100, 800); k2["x"][s] = k1["x"][s]        # away from the epipole
    mp1[3] = 1; mp2[3] = 0
    mp2[t] = 1
    for s in taken:
        mp2[s] = 1
    q = d1[t]
    d2[3] = _flipped(q, range(0, 6)); d2[n - 1] = _flipped(q, range(6, 12)); d1[n - 1] = _flipped(d2[n - 1], (20, 21))
    for a in (k1, k2):
        a["y"][n - 1] = a["y"][t]
    k2["y"][3] = k2["y"][t]; k2["x"][3] = 300.0
    k2["octave"][3] = k2["octave"][n - 1] = 0
    node[[3, n - 1]] = node[t]
    for s in own + [t]:                                                    # no turn: the planted matches fall into the kept bin 0
        k2["angle"][s] = k1["angle"][s]
    k1["angle"][n - 1] = k2["angle"][n - 1] = k2["angle"][3] = k1["angle"][t]
    want = sr.search_for_triangulation(k1, d1, mp1, None, _fv(node), k2, d2, mp2, None, _fv(node), M10_F12, M10_EP, sf, (sf * sf).astype(np.float32),
                                       False, False, True)
    return dict(n=n, k1=k1, d1=d1, mp1=mp1, k2=k2, d2=d2, mp2=mp2, node=node, sf=sf, sigma2=(sf * sf).astype(np.float32), want=want,
                own=own, tie=(t, 3, n - 1), taken=taken)


# ---- the two-camera (fisheye) forms of M3 and M4: pair p searches left row p and right row first_r + p of one pool -------------------
import second_reading_fisheye as srf                     # noqa: E402
import second_reading_points_fisheye as srpf             # noqa: E402


def fisheye_layout(hp):
    """(first_l, first_r, npairs): cap 65535: left rows 0, 1, 2 against right rows 3 (empty), 4 (count > cap), 5 (row 0 again, the blocked
    variant); cap 32769: left rows 0, 1 against right rows 2 (empty), 3 (row 0 again, the blocked variant)."""
    npairs = hp.R // 2
    return 0, hp.R - npairs, npairs


def _two_camera_queries(rng, hp, rl_, rr_):
    """2 NQ queries of a pair: the first NQ drawn on the left row's keypoints (direct_queries) with a keypoint of the right row as their
    right projection, the last NQ drawn on the right row's with a left keypoint of their octave as left projection (an empty left
    window ends an M4 query before its right search).  Returns the left-drawn and right-drawn query dicts and the right / left
    coordinates that go with them."""
    ql, qr = direct_queries(rng, hp, rl_), direct_queries(rng, hp, rr_)
    kl, _ = hp.row(rl_ if hp.n(rl_) else 0); kr, _ = hp.row(rr_ if hp.n(rr_) else 0)
    jr = rng.integers(0, len(kr), NQ)
    by_octave = [np.flatnonzero(kl["octave"] == o) for o in range(hp.nlev)]
    jl = np.array([rng.choice(by_octave[o]) for o in qr["level"]])
    return ql, qr, (kr["x"][jr], kr["y"][jr]), (kl["x"][jl], kl["y"][jl])


@functools.lru_cache(maxsize=None)
def m4_fisheye_case(cap):
    hp = pool(cap)
    rng = np.random.default_rng(4400 + cap)
    first_l, first_r, npairs = fisheye_layout(hp)
    Q, BL, BR, want = [], [], [], []
    cat = lambda a, b: np.concatenate([a, b])
    for p in range(npairs):
        rl_, rr_ = first_l + p, first_r + p
        ql, qr, right_of_l, left_of_r = _two_camera_queries(rng, hp, rl_, rr_)
        q = dict(valid=cat(ql["valid"], qr["valid"]), u=cat(ql["u"], left_of_r[0]), v=cat(ql["v"], left_of_r[1]), ur=cat(right_of_l[0], qr["u"]),
                 vr=cat(right_of_l[1], qr["v"]), octave=cat(ql["level"], qr["level"]), angle=cat(ql["angle"], qr["angle"]),
                 qdesc=cat(ql["desc"], qr["desc"]), planted_l=ql["planted_at"], planted_r=[NQ + a for a in qr["planted_at"]])
        q["mp_obs"] = (rng.random(2 * NQ) < 0.6).astype(np.uint8)
        for r, at in ((rl_, q["planted_l"]), (rr_, q["planted_r"])):
            if at:
                q["mp_obs"][at] = 1
                q["mp_obs"][planted(hp.plants[r], at, "shared8")[0]] = 0
        bl = blocked_rows(rng, hp, rl_, 0.2, False); br = blocked_rows(rng, hp, rr_, 0.2, rr_ == hp.R - 1)
        Q.append(q); BL.append(bl); BR.append(br)
        want.append(srf.search_by_projection_frame_fisheye(hp.grid(rl_), hp.grid(rr_), bl[:hp.n(rl_)], br[:hp.n(rr_)], hp.sf, q["valid"], q["u"], q["v"],
                                                           q["ur"], q["vr"], q["octave"], q["angle"], q["qdesc"], q["mp_obs"], M4_TH, check_ori=True))
    return dict(hp=hp, layout=(first_l, first_r, npairs), Q=Q, blocked_l=np.stack(BL), blocked_r=np.stack(BR), want=want)


@functools.lru_cache(maxsize=None)
def m3_fisheye_case(cap):
    """As m4_fisheye_case; a left-drawn query is in view on the left (a third of them on the right as well), a right-drawn one on the
    right alone."""
    hp = pool(cap)
    rng = np.random.default_rng(3300 + cap)
    first_l, first_r, npairs = fisheye_layout(hp)
    Q, BL, BR, want = [], [], [], []
    cat = lambda a, b: np.concatenate([a, b])
    z = np.zeros(NQ, np.uint8)
    for p in range(npairs):
        rl_, rr_ = first_l + p, first_r + p
        ql, qr, right_of_l, left_of_r = _two_camera_queries(rng, hp, rl_, rr_)
        both = (rng.random(NQ) < 0.33).astype(np.uint8) & ql["valid"]
        both[ql["planted_at"]] = 0
        q = dict(in_view=cat(ql["valid"], z), px=cat(ql["u"], left_of_r[0]), py=cat(ql["v"], left_of_r[1]), view_cos=np.full(2 * NQ, 0.9, np.float32),
                 level=cat(ql["level"], qr["level"]), in_view_r=cat(both, qr["valid"]), pxr=cat(right_of_l[0], qr["u"]), pyr=cat(right_of_l[1], qr["v"]),
                 view_cos_r=np.full(2 * NQ, 0.9, np.float32), level_r=cat(ql["level"], qr["level"]), qdesc=cat(ql["desc"], qr["desc"]),
                 planted_l=ql["planted_at"], planted_r=[NQ + a for a in qr["planted_at"]])
        q["mp_obs"] = (rng.random(2 * NQ) < 0.6).astype(np.uint8)
        for r, at in ((rl_, q["planted_l"]), (rr_, q["planted_r"])):
            if at:
                q["mp_obs"][at] = 1
                q["mp_obs"][planted(hp.plants[r], at, "shared8")[0]] = 0
        bl = blocked_rows(rng, hp, rl_, 0.2, False); br = blocked_rows(rng, hp, rr_, 0.2, rr_ == hp.R - 1)
        Q.append(q); BL.append(bl); BR.append(br)
        want.append(srpf.search_by_projection_points_fisheye(hp.grid(rl_), hp.grid(rr_), bl[:hp.n(rl_)], br[:hp.n(rr_)], None, None, hp.sf, q["in_view"],
                                                             q["px"], q["py"], q["view_cos"], q["level"], q["in_view_r"], q["pxr"], q["pyr"],
                                                             q["view_cos_r"], q["level_r"], q["qdesc"], q["mp_obs"], M3_TH, M3_NNRATIO))
    return dict(hp=hp, layout=(first_l, first_r, npairs), Q=Q, blocked_l=np.stack(BL), blocked_r=np.stack(BR), want=want)
