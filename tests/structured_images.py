"""Structured test images: saturated, periodic and tie-heavy frames that the value-noise generator (orb-slam3_amd/synth.py)
never produces.  gen(kind, w, h, seed, **params) -> uint8 (h, w); pure numpy, deterministic for a given argument list.

kind        parameters (defaults)              what it is for
binary      --                                 every pixel 0 or 255 at random: 9/16 of the pixels pass FAST's 4-point quick test (~770 of a 36 x 38
                                               cell: under level 0's queue of ~900-1000 entries, over it on levels 1-3 once the resize has
                                               spread the values: k_fast_fix there), every 16-bit lane at its extreme on level 0
blocks      block (4; 2..6)                    random 0/255 blocks: plateaus of equal FAST score on level 0 (no strict maximum), corners on level 1
dots        pitch (8)                          white dots on black, one every `pitch` px: thousands of candidates with one response, symmetric
                                               orientation patches (m01 == m10 == 0)
holes       pitch (10)                         the negative: black holes on white, at a pitch that does not divide the FAST cell size
clipped     gain (4.0)                         synth's textured frame with `gain` times its contrast about its mean, clipped: most pixels 0 or 255
checker     period (16), contrast (255),       checkerboard about 128; contrast 15 sits between minTh (7) and iniTh (20): the per-cell threshold retry;
            flip (0)                           period 3 with a fraction `flip` of the pixels inverted: nearly every pixel passes the quick test, so
                                               the level-0 cells overflow the wave's queue too, and the inverted pixels give them corners
ramp_dots   pitch (8)                          horizontal ramp under a dot lattice: m01 == 0 < m10, angle exactly 0
halves      left ("binary"), right ("constant") left half one kind, right half another: overflowing and empty cells in one strip
border      pitch (3), base (255)              structure only 19..22 px from the image edges (the EDGE_THRESHOLD band; the blur's reflect-101 border
                                               is read under it), all-`base` elsewhere
constant    value (128)                        no corner at all
textured / sparse / lowcontrast               synth.gen_image, unchanged
"""
import importlib

import numpy as np

KINDS = ("binary", "blocks", "dots", "holes", "clipped", "checker", "ramp_dots", "halves", "border")
SYNTH_KINDS = ("textured", "sparse", "lowcontrast")
DENSE = ("checker", {"period": 3, "contrast": 255, "flip": 0.05})      # the kind that overflows the queue on level 0 as well

# (kind, parameters) of every structured case the CPU and GPU suites and the tools walk through
STRUCTURED = [("binary", {}), ("blocks", {"block": 4}), ("blocks", {"block": 3}), ("dots", {"pitch": 8}), ("dots", {"pitch": 7}),
              ("holes", {"pitch": 10}), ("clipped", {"gain": 4.0}), ("checker", {"period": 16, "contrast": 255}),
              ("checker", {"period": 16, "contrast": 15}), ("checker", {"period": 3, "contrast": 255, "flip": 0.05}), ("ramp_dots", {"pitch": 8}),
              ("halves", {"left": "binary", "right": "constant"}), ("halves", {"left": "dots", "right": "binary"}),
              ("border", {"base": 255}), ("border", {"base": 0})]


def case_id(v):
    """pytest id of a parameter dictionary."""
    if isinstance(v, dict):
        return "-".join("%s%s" % kv for kv in sorted(v.items())) or "default"
    return None


def _synth():
    return importlib.import_module("orb-slam3_amd.synth")


def _lattice(w, h, pitch, seed):
    """Boolean mask of one pixel every `pitch` px in both directions; the seed moves the lattice's phase."""
    m = np.zeros((h, w), bool)
    m[(pitch // 2 + seed) % pitch::pitch, (pitch // 2 + 3 * seed) % pitch::pitch] = True
    return m


def gen(kind, w, h, seed, **p):
    rng = np.random.default_rng(seed)
    if kind in SYNTH_KINDS:
        return _synth().gen_image(w, h, seed, kind)
    if kind == "constant":
        return np.full((h, w), p.get("value", 128), np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w), dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "blocks":
        b = int(p.get("block", 4))
        assert 2 <= b <= 6
        cells = rng.integers(0, 2, ((h + b - 1) // b, (w + b - 1) // b), dtype=np.uint8) * 255
        return np.ascontiguousarray(np.kron(cells, np.ones((b, b), np.uint8))[:h, :w]).astype(np.uint8)
    if kind == "dots":
        return np.where(_lattice(w, h, int(p.get("pitch", 8)), seed), 255, 0).astype(np.uint8)
    if kind == "holes":
        return np.where(_lattice(w, h, int(p.get("pitch", 10)), seed), 0, 255).astype(np.uint8)
    if kind == "clipped":
        img = _synth().gen_image(w, h, seed, "textured").astype(np.float64)
        m = img.mean()
        return np.clip(np.rint(m + float(p.get("gain", 4.0)) * (img - m)), 0, 255).astype(np.uint8)
    if kind == "checker":
        period = int(p.get("period", 16)); c = int(p.get("contrast", 255))
        lo = 128 - (c + 1) // 2; hi = lo + c
        yy, xx = np.mgrid[0:h, 0:w]
        on = ((((yy + seed) // period) + ((xx + 3 * seed) // period)) & 1).astype(bool)
        if p.get("flip"):                                            # a fraction of the pixels inverted at random: corners on a board that has none
            on ^= rng.random((h, w)) < float(p["flip"])
        return np.where(on, hi, lo).astype(np.uint8)
    if kind == "ramp_dots":
        ramp = (np.arange(w, dtype=np.int64) * 255 // max(w - 1, 1)).astype(np.uint8)
        img = np.broadcast_to(ramp, (h, w)).copy()
        dot = _lattice(w, h, int(p.get("pitch", 8)), seed)
        img[dot] = np.where(img[dot] < 128, 255, 0)               # every dot at full contrast against its half of the ramp
        return img
    if kind == "halves":
        left = gen(p.get("left", "binary"), w, h, seed); right = gen(p.get("right", "constant"), w, h, seed + 1)
        img = left.copy()
        img[:, w // 2:] = right[:, w // 2:]
        return img
    if kind == "border":
        base = int(p.get("base", 255))
        yy, xx = np.mgrid[0:h, 0:w]
        d = np.minimum(np.minimum(xx, w - 1 - xx), np.minimum(yy, h - 1 - yy))       # distance to the nearest image edge
        band = (d >= 19) & (d <= 22)
        noise = rng.integers(0, 2, (h, w), dtype=np.uint8) * 255
        return np.where(band, noise, base).astype(np.uint8)
    raise ValueError("unknown kind %r" % (kind,))


def fast_bruteforce(img, thr):
    """FAST-9/16 + strict 3x3 maximum, score = max(A, B) - 1, straight from the definition: A (B) is the largest over the 16 arcs of
    nine contiguous ring pixels of the smallest amount by which the centre is brighter (darker) than the arc; a corner has
    max(A, B) > thr.  Returns [[x, y, score], ...] in row-major order, as oracle.fast does."""
    dx = [0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1]
    dy = [3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3]
    h, w = img.shape
    S = np.zeros((h, w), np.int64)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            v = int(img[y, x]); d = [v - int(img[y + dy[k], x + dx[k]]) for k in range(16)]
            A = max(min(d[(s + t) % 16] for t in range(9)) for s in range(16))
            B = max(min(-d[(s + t) % 16] for t in range(9)) for s in range(16))
            if max(A, B) > thr:
                S[y, x] = max(A, B) - 1
    exp = []
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            if S[y, x] > 0:
                nb = S[y - 1:y + 2, x - 1:x + 2].copy(); nb[1, 1] = -1
                if S[y, x] > nb.max():
                    exp.append([x, y, int(S[y, x])])
    return exp


def quick_test_fraction(img, thr):
    """Fraction of the pixels (3 px inside the frame) that pass the 4-point test at radius 3:
    v - max(min(up, down), min(left, right)) > thr  or  min(max(up, down), max(left, right)) - v > thr."""
    a = img.astype(np.int64)
    v = a[3:-3, 3:-3]; up = a[:-6, 3:-3]; dn = a[6:, 3:-3]; lf = a[3:-3, :-6]; rt = a[3:-3, 6:]
    bright = v - np.maximum(np.minimum(up, dn), np.minimum(lf, rt)) > thr
    dark = np.minimum(np.maximum(up, dn), np.maximum(lf, rt)) - v > thr
    return float((bright | dark).mean())


MBF = 47.90639384423901
MB = MBF / 435.2046959714599            # Examples/Stereo/EuRoC.yaml:9,28
PAIRS = [("dots", 12, {"pitch": 8}), ("binary", 20, {})]           # (kind, disparity, parameters) of the stereo cases


def shifted_pair(kind, w, h, seed, d, **params):
    """Rectified stereo pair at constant disparity d: right(x) = left(x + d), so uL - uR = d."""
    big = gen(kind, w + d, h, seed, **params)
    return np.ascontiguousarray(big[:, :w]), np.ascontiguousarray(big[:, d:d + w])


# ---- which FAST route a cell takes in the product (restated from the host code, for the conditions the suites assert) ----
def fast_cells(w, h):
    """The reference's FAST cell grid of a w x h level (ORBextractor.cc:1085-1110): [(x0, y0, cw, ch, row, col)], cell size (wc, hc).
    A cell evaluates the pixels [x0 + 3, x0 + cw - 3) x [y0 + 3, y0 + ch - 3); these ranges tile the level."""
    width, height = w - 32, h - 32
    ncols, nrows = width // 35, height // 35
    wc, hc = -(-width // ncols), -(-height // nrows)
    cells = []
    for i in range(nrows):
        y0 = 16 + i * hc
        if y0 >= h - 16 - 3:
            continue
        for j in range(ncols):
            x0 = 16 + j * wc
            if x0 >= w - 16 - 6:
                continue
            cells.append((x0, y0, min(x0 + wc + 6, w - 16) - x0, min(y0 + hc + 6, h - 16) - y0, i, j))
    return cells, (wc, hc)


def fast_queue_caps(level_sizes):
    """Entries of the survivor queue a wave of k_fast4 has for a cell, per level: a restatement of the host code that sizes it
    (orb-slam3_amd/csrc/orbx_plan.h, "strips for k_fast3" and "FAST launch groups"; 256 threads = 4 waves per workgroup).  A cell whose
    quick-test survivors outnumber it is redone by k_fast_fix.  Level 0 and the fine levels get max(512, what lets 7 workgroups share a
    CU's 160 KB), never more than the worst case of their cells; the coarse levels keep the worst case unless 5 workgroups fit at
    >= 3/4 of it.  This is derived from the code, not read from the device: nothing in the product's ABI reports it."""
    up = lambda v, a: (v + a - 1) // a * a
    waves = 4
    strips = []                                                     # (level, lp, rows, worst case)
    ncells = []
    for l, (w, h) in enumerate(level_sizes):
        cells, _ = fast_cells(w, h)
        ncells.append(len(cells))
        ci = 0
        while ci < len(cells):
            f = cells[ci]
            xal = (f[0] - 4) & ~15
            n = needed = 0
            while ci + n < len(cells) and n < waves:
                c = cells[ci + n]
                nd = c[0] + c[2] - 3 - xal + 8
                if c[1] != f[1] or nd > 512:
                    break
                needed = nd; n += 1
            assert n > 0
            worst = max([64] + [up(max(0, c[2] - 6) * max(0, c[3] - 6), 64) for c in cells[ci:ci + n]])
            strips.append((l, up(needed, 16), f[3], worst))
            ci += n
    L = len(level_sizes)
    after = [sum(ncells[l:]) for l in range(L + 1)]
    k = L - 1
    while k > 0 and after[k] * 100 <= 15 * after[0]:
        k -= 1
    caps = [0] * L
    for gi, levels in enumerate(([0], list(range(1, k + 1)), list(range(max(k, 0) + 1, L)))):
        grp = [s for s in strips if s[0] in levels]
        if not grp:
            continue
        tile = max(s[1] * s[2] for s in grp); worst = max(s[3] for s in grp)
        lp = max(s[1] for s in grp); rows = max(s[2] for s in grp)
        pitch = 176 if lp <= 176 else 208 if lp <= 208 else 0
        if pitch:
            tile = pitch * rows
        tile = up(tile, 16)
        cap = worst
        if gi < 2:
            budget = int((160 * 1024 // 7 - 2 * tile) / (2 * waves))
            cap = min(worst, max(512, budget // 64 * 64))
        else:
            q5 = int((160 * 1024 // 5 - 2 * tile) / (2 * waves)) // 64 * 64
            if q5 < worst and q5 * 4 >= worst * 3:
                cap = q5
        for l in levels:
            caps[l] = cap
    return caps


def quick_test_mask(img, thr):
    """Per pixel: does it pass the 4-point test at radius 3 (False within 3 px of the frame)?"""
    a = img.astype(np.int64)
    q = np.zeros(a.shape, bool)
    v = a[3:-3, 3:-3]; up = a[:-6, 3:-3]; dn = a[6:, 3:-3]; lf = a[3:-3, :-6]; rt = a[3:-3, 6:]
    q[3:-3, 3:-3] = (v - np.maximum(np.minimum(up, dn), np.minimum(lf, rt)) > thr) | (np.minimum(np.maximum(up, dn), np.maximum(lf, rt)) - v > thr)
    return q


def cell_routes(ref, nlevels=8, ini_th=20, min_th=7):
    """Per level of the oracle extractor `ref` (after a call): (cells, cells redone by k_fast_fix, cells retried at minTh, queue entries).
    A cell overflows when its quick-test survivors at iniTh outnumber the queue, or -- it being empty at iniTh -- those at minTh do."""
    sizes = [ref.level_size(l) for l in range(nlevels)]
    caps = fast_queue_caps(sizes)
    out = []
    for l in range(nlevels):
        img = ref.level_image(l)
        cells, (wc, hc) = fast_cells(*sizes[l])
        qi, qm = quick_test_mask(img, ini_th), quick_test_mask(img, min_th)
        c = ref.level_candidates(l)                                 # x, y relative to (16, 16): a cell returns x in [3, wc + 3) of its origin
        s = c[c[:, 2] >= ini_th]                                    # score = max(A, B) - 1 >= iniTh: found by the iniTh pass
        strong = set(zip(((s[:, 1] - 3) // hc).tolist(), ((s[:, 0] - 3) // wc).tolist()))
        over = retry = 0
        for x0, y0, cw, ch, i, j in cells:
            box = (slice(y0 + 3, y0 + ch - 3), slice(x0 + 3, x0 + cw - 3))
            again = (i, j) not in strong and min_th < ini_th
            retry += again
            over += bool(qi[box].sum() > caps[l] or (again and qm[box].sum() > caps[l]))
        out.append((len(cells), over, retry, caps[l]))
    return out
