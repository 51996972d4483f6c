"""Inputs shared by the ComputeStereoMatches tests: constructed stereo pairs, each built to reach one branch of Frame.cc:1027-1276.
A case is an image pair plus hand-laid keypoint and descriptor rows -- not extractor output.  Level 0 of a pyramid is the caller's image,
so octave-0 cases have exact pixel control: both images are independent noise in [64, 191], and a SITE paints into the right image the
left image's texture around a left keypoint, shifted, and then adds increments of at most 60 to pixels of the right keypoint's central
11 x 11 window, so that the SAD at the matching shift is exactly the number asked for (every other shift compares unrelated noise: about
5000).  One camera: 376 x 240 (no level's width is a multiple of 64, the pitch of the device pyramids), the nominal 1.2 / 8-level
extractor.  No oracle, product or second-reading import: this file only makes arrays."""
import numpy as np

F = np.float32
W, H, NLEVELS = 376, 240, 8
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
MB, MBF = 1.0, 40.0                              # maxD = mbf / mb = 40 px, so that [minU, maxU] has both ends inside the image
MAXD = 40.0


def scale_tables(scale_factor=1.2, nlevels=NLEVELS):
    """mvScaleFactor / mvInvScaleFactor as ORBextractor.cc:484-499 fills them: a float vector times the double member scaleFactor."""
    sf = np.ones(nlevels, F)
    for i in range(1, nlevels):
        sf[i] = F(np.float64(sf[i - 1]) * np.float64(F(scale_factor)))
    return sf, (F(1.0) / sf).astype(F)


SF, ISF = scale_tables()
LEVEL_W = [int(np.rint(F(W) * ISF[l])) for l in range(NLEVELS)]             # ORBextractor.cc:1669, cvRound of a float product
LEVEL_H = [int(np.rint(F(H) * ISF[l])) for l in range(NLEVELS)]


def bits(*ranges):
    """A 32-byte descriptor with the bits of the given [lo, hi) ranges set."""
    b = np.zeros(256, np.uint8)
    for lo, hi in ranges:
        b[lo:hi] = 1
    return np.packbits(b, bitorder="little")


def band(y, octave):
    """(minr, maxr) of Frame.cc:1071-1073 for a right keypoint."""
    r = F(F(2.0) * SF[octave])
    return int(np.floor(F(F(y) - r))), int(np.ceil(F(F(y) + r)))


def cut_threshold(median):
    """Frame.cc:1263 in float."""
    return F(F(F(1.5) * F(1.4)) * F(median))


def survives(s, median):
    return bool(F(s) < cut_threshold(median))


def _sad(a, b):
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())


class Case:
    """One constructed pair.  expect: counter of the second reading -> least count that proves the branch was reached (0 = must be 0,
    ("==", n) = exactly n); valid: left keypoint -> whether it holds a stereo point at the end; sad: left keypoint -> its best SAD."""

    def __init__(self, name, seed, mb=MB, mbf=MBF):
        self.name, self.mb, self.mbf = name, mb, mbf
        self.rng = np.random.default_rng(seed)
        self.img_l = self.rng.integers(64, 192, (H, W)).astype(np.uint8)
        self.img_r = self.rng.integers(64, 192, (H, W)).astype(np.uint8)
        self._kl, self._dl, self._kr, self._dr = [], [], [], []
        self.expect, self.valid, self.sad = {}, {}, {}
        self.clamped = []                                                    # left keypoints that end on the clamp of :1243-1247

    def left(self, x, y, desc, octave=0):
        self._kl.append((x, y, 31.0, 0.0, 1.0, octave, -1)); self._dl.append(desc)
        return len(self._kl) - 1

    def right(self, x, y, desc, octave=0):
        self._kr.append((x, y, 31.0, 0.0, 1.0, octave, -1)); self._dr.append(desc)
        return len(self._kr) - 1

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def paint(self, x, y, shift, sad=120, half=16):
        """Right image, rows y-5..y+5: the columns around c = x - shift take the left image's texture around x (clipped to the image), then
        increments summing to `sad` go onto pixels of the 11 x 11 window centred on (c, y): SAD(left window at x, right window at c) == sad."""
        c = x - shift
        k0 = max(-half, -c, -x); k1 = min(half, W - 1 - c, W - 1 - x)
        assert k0 <= -5 and k1 >= 5 and 5 <= y < H - 5
        self.img_r[y - 5:y + 6, c + k0:c + k1 + 1] = self.img_l[y - 5:y + 6, x + k0:x + k1 + 1]
        cells = [(yy, xx) for yy in range(y - 5, y + 6) for xx in range(c - 5, c + 6)]
        order = self.rng.permutation(len(cells))
        left = sad
        for j in order:
            if left == 0:
                break
            inc = min(60, left)
            self.img_r[cells[j]] += inc                                      # texture <= 191: no overflow
            left -= inc
        assert left == 0 and _sad(self.img_l[y - 5:y + 6, x - 5:x + 6], self.img_r[y - 5:y + 6, c - 5:c + 6]) == sad
        return c

    def site(self, x, y, shift=8, e=0, sad=120, dl=None, dr=None, valid=True):
        """A left keypoint at (x, y), its texture in the right image at x - shift, the right keypoint `e` columns right of it: the slide's
        best shift is -e.  Returns (left index, right index)."""
        c = self.paint(x, y, shift, sad)
        lo = max(c + e - 10, 0)
        win = self.img_l[y - 5:y + 6, x - 5:x + 6]
        for inc in range(-5, 6):                                             # the builder's own check: -e is the strict minimum
            c0 = c + e + inc - 5
            if inc != -e and c0 >= lo and c0 + 11 <= W:
                assert _sad(win, self.img_r[y - 5:y + 6, c0:c0 + 11]) > sad, (self.name, x, y, inc)
        d = self.desc() if dl is None else dl
        il = self.left(float(x), float(y), d)
        ir = self.right(float(c + e), float(y), d if dr is None else dr)
        if valid is not None:
            self.valid[il] = valid
        if valid:
            self.sad[il] = sad
        return il, ir

    def fillers(self, n=5, y0=200, sad=120):
        """n plain matches (SAD 120) on the rows from y0 down, so that the pair's median does not depend on the case's own points."""
        for i in range(n):
            self.site(60 + 50 * i, y0 + 12 * (i % 3), sad=sad)

    def arrays(self):
        return (np.array(self._kl, KP_DTYPE), np.array(self._dl, np.uint8).reshape(-1, 32),
                np.array(self._kr, KP_DTYPE), np.array(self._dr, np.uint8).reshape(-1, 32))


def _row_band():
    c = Case("row_band", 11)
    c.fillers()
    n_out = 0
    # right keypoints with integer and fractional y at octaves 0 and 3; left keypoints on rows minr-1, minr, maxr, maxr+1 of each
    for x, y, o in ((60, 30.0, 0), (140, 70.3, 0), (220, 110.0, 3), (300, 160.5, 3)):
        minr, maxr = band(y, o)
        d = c.desc()
        c.right(float(x - 8), y, d, octave=o)
        if o == 0:                                                           # exact pixels: every in-band row is a match with SAD 0
            c.img_r[minr - 6:maxr + 7, x - 24:x + 9] = c.img_l[minr - 6:maxr + 7, x - 16:x + 17]
        for j, row in enumerate((minr - 1, minr, maxr, maxr + 1)):
            inside = minr <= row <= maxr
            il = c.left(float(x), float(row) + 0.25 * j, d, octave=o)        # (int)vL decides the row
            if o == 0 or not inside:
                c.valid[il] = inside
            if o == 0 and inside:
                c.sad[il] = 0
            n_out += not inside
    assert band(30.0, 0) == (28, 32) and band(70.3, 0) == (68, 73)
    # bands that leave the image at the top and at the bottom (:1077 would index rows -4.. and ..242): those rows are dropped
    c.right(20.0, 2.0, c.desc(), octave=3); c.right(20.0, 238.5, c.desc(), octave=3)
    assert band(2.0, 3)[0] < 0 and band(238.5, 3)[1] >= H
    c.expect = {"empty_row_list": ("==", n_out), "row_on_minr": 4, "row_on_maxr": 4, "row_outside_image_dropped": 4}
    return c


def _octave_band():
    c = Case("octave_band", 12)
    c.fillers()
    x = 100
    for j, o in enumerate((0, 1, 2, 3, 4)):                                  # levelL = 2 against levelL - 2 .. levelL + 2
        y = 20 + 30 * j
        d = c.desc()
        il = c.left(float(x), float(y), d, octave=2)
        c.right(float(x - 8), float(y), d, octave=o)
        if o in (0, 4):
            c.valid[il] = False
    c.expect = {"octave_band_reject": ("==", 2), "bestDist_ge_thOrbDist": ("==", 2)}
    return c


def _u_range():
    c = Case("u_range", 13)
    c.fillers()
    x = 200
    # uR exactly minU: the texture two columns right of the keypoint, disparity about 38
    a, ra = c.site(x, 20, shift=38, e=-2)
    assert c._kr[ra][0] == x - MAXD
    # one float step below minU
    b, rb = c.site(x, 40, shift=38, e=-2, valid=False)
    c._kr[rb] = (float(np.nextafter(F(x - MAXD), F(-1e9))),) + c._kr[rb][1:]
    # uR exactly uL = maxU: the texture two columns left of the keypoint, disparity about 2
    d_, rd = c.site(x, 60, shift=2, e=2)
    assert c._kr[rd][0] == x
    # one float step above maxU
    e_, re_ = c.site(x, 80, shift=2, e=2, valid=False)
    c._kr[re_] = (float(np.nextafter(F(x), F(1e9))),) + c._kr[re_][1:]
    # a left keypoint with x < 0 on a row that has candidates: maxU < 0
    d = c.desc()
    g = c.left(-3.0, 100.0, d); c.right(20.0, 100.0, d)
    c.valid[g] = False
    c.expect = {"uR_on_minU": 1, "uR_on_maxU": 1, "u_range_reject": 2, "maxU_negative": ("==", 1)}
    return c


def _hamming():
    c = Case("hamming", 14)
    c.fillers()
    a, _ = c.site(100, 20, dl=bits(), dr=bits((0, 74)))                      # 74 < thOrbDist: goes on
    b, _ = c.site(100, 40, dl=bits(), dr=bits((0, 75)), valid=False)         # 75: stops
    g, _ = c.site(100, 60, dl=bits(), dr=bits((0, 100)), valid=False)        # only candidates at >= TH_HIGH: bestDist keeps its initial 100
    c.right(95.0, 60.0, bits((0, 120)))
    c.expect = {"bestDist_on_thOrbDist_minus_1": 1, "bestDist_ge_thOrbDist": ("==", 2)}
    return c


def _hamming_ties():
    """One row whose list holds 140 right keypoints.  Left keypoint A: the winner is right keypoint 70 (second trip of a 64-lane scan,
    fifth of a 16-lane one); 75 (another lane) and 134 (the same lane of 64, a later trip) tie with it at distance 30, and keypoint 3
    holds a larger distance at a lower index.  Only 70 sits on the painted texture: any other winner gives another uright."""
    c = Case("hamming_ties", 15)
    c.fillers(y0=150)
    x, y = 300, 40
    q = bits()
    c.paint(x, y, 8)
    special = {3: (x - 30.0, bits((0, 40))), 70: (x - 8.0, bits((0, 30))), 75: (x - 20.0, bits((10, 40))), 134: (x - 14.0, bits((100, 130)))}
    for i in range(140):
        if i in special:
            c.right(special[i][0], float(y), special[i][1])
        else:
            c.right(float(10 + 2 * i), float(y + (i % 5) - 2), c.desc())      # random rows of the band: about 128 bits from every query
    a = c.left(float(x), float(y), q)
    c.valid[a] = True; c.sad[a] = 120
    # left keypoint B on the same row: two exact ties at a distance that goes on, the lower index (20, at the texture) wins over 21
    x2 = 120
    c.paint(x2, y, 8)
    q2 = bits((128, 256))
    c._kr[20] = (x2 - 8.0, float(y), 31.0, 0.0, 1.0, 0, -1); c._dr[20] = bits((128, 256), (0, 12))
    c._kr[21] = (x2 - 16.0, float(y), 31.0, 0.0, 1.0, 0, -1); c._dr[21] = bits((128, 256), (20, 32))
    b = c.left(float(x2), float(y), q2)
    c.valid[b] = True; c.sad[b] = 120
    c.expect = {"distance_tie": 3, "candidates_over_64": 2}
    return c


def _sad_window():
    c = Case("sad_window", 16)
    c.fillers()
    w0 = LEVEL_W[0]
    # octave 0: round(uR0) + 11 == width is skipped, == width - 1 runs (its last shift reads column width - 2)
    a, _ = c.site(369, 20, shift=4, e=0, valid=False)                        # right keypoint at 365
    assert c._kr[-1][0] + 11 == w0
    b, _ = c.site(369, 40, shift=4, e=-1)                                    # right keypoint at 364, texture one column right of it
    assert c._kr[-1][0] + 11 == w0 - 1
    # iniu == 0: the right keypoint on column 0; only the last shift lies inside the level, it wins (SAD 60) and is rejected as +L
    g, _ = c.site(13, 60, shift=8, e=-5, sad=60, valid=False)
    assert c._kr[-1][0] == 0.0
    # iniu == -1
    d = c.desc()
    h = c.left(20.0, 80.0, d); c.right(-1.0, 80.0, d)
    c.valid[h] = False
    # a coarse octave: the same two bounds against level 3's width
    o = 3
    for j, sc in enumerate((LEVEL_W[o] - 11, LEVEL_W[o] - 12)):
        ur0 = F(F(sc) * SF[o])
        assert int(np.floor(float(F(ur0 * ISF[o])) + 0.5)) == sc
        d = c.desc()
        y = 110.0 + 30 * j
        il = c.left(float(ur0) + 4.0, y, d, octave=o); c.right(float(ur0), y, d, octave=o)
        assert int(np.floor(float(F(F(float(ur0) + 4.0) * ISF[o])) + 0.5)) + 5 < LEVEL_W[o]
        if j == 0:
            c.valid[il] = False
    c.expect = {"endu_ge_cols": ("==", 2), "endu_cols_minus_1": ("==", 2), "iniu_zero": ("==", 1), "iniu_negative": ("==", 1),
                "slide_left_of_level": 10, "bestincR_at_plus_L": 1}
    return c


def _slide():
    c = Case("slide", 17)
    c.fillers()
    a, _ = c.site(100, 20, e=5, valid=False)                                 # best shift -5
    b, _ = c.site(100, 40, e=-5, valid=False)                                # best shift +5
    # a texture of period 6 along the row: shifts -3 and +3 both give SAD 0, the first one wins
    x, y = 200, 60
    u0 = x - 8
    per = c.rng.integers(64, 192, (11, 6)).astype(np.uint8)
    for col in range(x - 5, x + 6):
        c.img_l[y - 5:y + 6, col] = per[:, col % 6]
    for col in range(u0 - 10, u0 + 11):
        c.img_r[y - 5:y + 6, col] = per[:, (col - u0 + 3 + x) % 6]
    win = c.img_l[y - 5:y + 6, x - 5:x + 6]
    sads = [_sad(win, c.img_r[y - 5:y + 6, u0 + i - 5:u0 + i + 6]) for i in range(-5, 6)]
    assert sads[2] == 0 and sads[8] == 0 and sorted(sads)[2] > 0
    d = c.desc()
    p = c.left(float(x), float(y), d); c.right(float(u0), float(y), d)
    c.valid[p] = True; c.sad[p] = 0
    # rows that are constant over the window and one column more on the right: SAD(0) == SAD(+1) == 0 < SAD(-1), deltaR == 0.5 exactly
    x, y = 300, 80
    u0 = x - 8
    rowval = c.rng.integers(64, 192, (11, 1)).astype(np.uint8)
    c.img_l[y - 5:y + 6, x - 5:x + 6] = rowval
    c.img_r[y - 5:y + 6, u0 - 5:u0 + 7] = rowval
    d = c.desc()
    h = c.left(float(x), float(y), d); c.right(float(u0), float(y), d)
    c.valid[h] = True; c.sad[h] = 0
    c.expect = {"bestincR_at_minus_L": ("==", 1), "bestincR_at_plus_L": ("==", 1), "sad_tie_between_shifts": 2, "deltaR_half": ("==", 1)}
    return c


def _symmetric(c, x, y):
    """The same horizontally symmetric patch around column x of both images: SAD(0) == 0 and SAD(-1) == SAD(+1)."""
    half = c.rng.integers(64, 192, (11, 12)).astype(np.uint8)
    for k in range(-11, 12):
        c.img_l[y - 5:y + 6, x + k] = half[:, abs(k)]
        c.img_r[y - 5:y + 6, x + k] = half[:, abs(k)]


def _clamp_fraction(c, n, y):
    """A left keypoint at a FRACTIONAL x whose disparity is exactly 0.  Both images hold the same texture around column n; the right
    image's columns n - 6 and n + 6 -- each read by one neighbouring shift only -- are set so that the parabola's offset deltaR =
    (d1 - d3) / (2 (d1 + d3)) is positive, and the left keypoint is laid at uL = n + deltaR, the very float :1235 computes."""
    rows = slice(y - 5, y + 6)
    c.img_r[rows, n - 16:n + 17] = c.img_l[rows, n - 16:n + 17]
    win = c.img_l[rows, n - 5:n + 6]
    base1 = _sad(win[:, 1:], c.img_r[rows, n - 5:n + 5])                     # shift -1 without its column n - 6
    base3 = _sad(win[:, :-1], c.img_r[rows, n - 4:n + 6])                    # shift +1 without its column n + 6
    i1, i3 = 600 + max(base3 - base1, 0), 0

    def lay(col_r, col_l, total):                                            # |left - right| over the 11 rows sums to `total`
        for r in range(y - 5, y + 6):
            inc = min(60, total)
            c.img_r[r, col_r] = c.img_l[r, col_l] + inc
            total -= inc
        assert total == 0
    lay(n - 6, n - 5, i1); lay(n + 6, n + 5, i3)
    d1 = F(_sad(win, c.img_r[rows, n - 6:n + 5])); d3 = F(_sad(win, c.img_r[rows, n - 4:n + 7]))
    assert d1 == base1 + i1 and d3 == base3 + i3 and d1 > d3
    delta = F(F(d1 - d3) / F(F(2.0) * F(d1 + d3)))                           # d2 == 0
    ul = F(F(n) + delta)
    assert F(0) < delta < F(0.45) and float(ul) != round(float(ul))
    d = c.desc()
    il = c.left(float(ul), float(y), d); c.right(float(n), float(y), d)
    c.valid[il] = True; c.sad[il] = 0
    return il


def clamp_in_float_differs():
    """The binades [2^j, 2^(j+1)) of uL, 1/8 <= uL < 512, in which `(float)((double)uL - 0.01)` (:1246 as written) and `uL - 0.01f` can
    differ.  uL sits on its binade's grid, so the exact difference sits at a FIXED fraction of a grid step above a grid point -- the
    fraction of 0.01 / ulp -- in the binade of the result (uL's, or the one below it); the two forms differ only if a rounding boundary
    (fraction 1/2) lies within 0.01 - (double)0.01f = 2.2e-10 of it.  The list is EMPTY: no keypoint of an image this size can tell the two
    forms apart, so the clamp cases pin the value of :1246 and not the width of its subtraction."""
    out = []
    gap = 0.01 - float(F(0.01))
    for j in range(-3, 9):
        for ulp in (2.0 ** (j - 23), 2.0 ** (j - 24)):
            frac = (0.01 / ulp) % 1.0
            if abs(frac - 0.5) <= 2 * abs(gap) / ulp:
                out.append(j)
    return out


def _disparity():
    c = Case("disparity", 18)
    c.fillers()
    a, ra = c.site(100, 20, shift=-3, e=-3, valid=False)                     # uR == uL, the slide moves right of uL: disparity -3
    assert c._kr[ra][0] == 100.0
    x, y = 200, 40                                                           # exactly 0: symmetric patch, uR == uL on integers
    _symmetric(c, x, y)
    d = c.desc()
    z = c.left(float(x), float(y), d); c.right(float(x), float(y), d)
    c.valid[z] = True; c.sad[z] = 0
    c.clamped.append(z)
    g, rg = c.site(300, 60, shift=42, e=2, valid=False)                      # uR == minU, the slide moves left: disparity 42 >= maxD
    assert c._kr[rg][0] == 300 - MAXD
    c.clamped.append(_clamp_fraction(c, 24, 80))
    c.expect = {"disparity_negative": ("==", 1), "disparity_ge_maxD": ("==", 1), "clamp": ("==", 2)}
    return c


GRID = [(40 + 24 * i, 12 + 12 * j) for j in range(19) for i in range(14)]    # sites whose windows do not touch


def _cut(name, seed, sads, expect, extra=None):
    """A pair whose surviving points have exactly the SADs given, in the order given."""
    c = Case(name, seed)
    order = list(sads)
    med = sorted(order)[len(order) // 2] if order else None
    for (x, y), s in zip(GRID, order):
        il, _ = c.site(x, y, sad=s, valid=survives(s, med))
        c.sad[il] = s                                                        # stays set for a point the cut removes
    if extra:
        extra(c)
    n_cut = sum(not survives(s, med) for s in order)
    c.expect = dict(expect)
    c.expect["cut"] = ("==", n_cut); c.expect["kept"] = ("==", len(order) - n_cut)
    c.median = med
    return c


def _around(m):
    """Seven SADs whose rank-3 element is m, with m - 1 and m + 1 beside it, the largest survivor of the float threshold and the first
    value it cuts: a median read one place too low cuts the former, one place too high keeps the latter."""
    th = cut_threshold(m)
    k = int(np.ceil(float(th))) - 1
    assert survives(k, m) and not survives(k + 1, m) and not survives(k, m - 1) and survives(k + 1, m + 1)
    return [k + 1, m - 1, m + 1, m - 2, k, m, m - 1]


def float_and_double_thresholds_differ():
    """Every (median m, SAD s) for which `s < 1.5f*1.4f*m` in float and the same test in double -- with the product's constants taken as
    double literals, as one literal 2.1, or as the float constant promoted -- disagree.  SADs are integers below 121 * 255 and 2.1 m is a
    multiple of 0.1, far coarser than either rounding: the list is EMPTY, so no input can tell a float threshold from a double one.  The
    threshold case below therefore pins the strict `<` and the rounding of the product at m = 10 (20 survives, 21 does not) instead."""
    m = np.arange(0, 121 * 255 + 1, dtype=np.int64)
    th_f = (F(F(1.5) * F(1.4)) * m.astype(F)).astype(F)
    out = []
    for th_d in (1.5 * 1.4 * m.astype(np.float64), 2.1 * m.astype(np.float64), float(F(F(1.5) * F(1.4))) * m.astype(np.float64)):
        for ds in (-1, 0, 1):
            s = np.floor(2.1 * m).astype(np.int64) + ds
            differ = np.nonzero((s.astype(F) < th_f) != (s.astype(np.float64) < th_d))[0]
            out += [(int(m[i]), int(s[i])) for i in differ]
    return out


def _no_match(c):
    d = c.desc()
    il = c.left(100.0, 100.0, d); c.right(92.0, 100.0, bits((0, 256)) ^ d)
    c.valid[il] = False


def constructed_cases():
    out = [_row_band(), _octave_band(), _u_range(), _hamming(), _hamming_ties(), _sad_window(), _slide(), _disparity()]
    out.append(_cut("cut_none_survive", 30, [], {"empty_vDistIdx": 1}, extra=_no_match))
    out.append(_cut("cut_one", 31, [500], {}))
    out.append(_cut("cut_one_sad_zero", 32, [0], {}))                        # median 0: the threshold is 0 and nothing is below it
    out.append(_cut("cut_two", 33, [100, 300], {}))                          # rank 1 = 300; rank 0 would cut the 300
    out.append(_cut("cut_odd", 34, [700, 100, 300, 600, 200], {}))
    out.append(_cut("cut_even", 35, [280, 120, 100, 260, 130, 110], {}))     # rank 3 = 130 keeps 260; rank 2 = 120 would cut it
    out.append(_cut("cut_all_equal", 36, [77] * 6, {}))
    for m in (127, 128, 1279, 1280):                                         # last / first of a bin of 128, at two multiples
        out.append(_cut("cut_bin_%d" % m, 40 + m % 7, _around(m), {}))
    out.append(_cut("cut_ties_at_median", 37, [50] + [200] * 40 + [419, 420, 421] + [90] * 30, {}))
    out.append(_cut("cut_threshold_edge", 38, [10, 21, 10, 20, 10], {}))     # 1.5f * 1.4f * 10 rounds to 21: 20 < 21 survives, 21 does not
    assert survives(20, 10) and not survives(21, 10)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
