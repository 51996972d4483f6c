"""A second, independent reading of the front of the frame: image ingest (cvtColor *2GRAY, remap INTER_LINEAR, CLAHE) and
undistortion (cv::undistortPoints as Frame::UndistortKeyPoints / ComputeImageBounds call it), in plain Python.

Written from the arithmetic the ABI comments of include/orbx.h and include/orbm.h state and from OpenCV 4.x's published behaviour, not
from oracle/orbref_frame.cpp or the kernels: it imports no product code and no oracle, and it states every operation in another form
than they do -- a tensor product instead of a pixel loop, exact rationals instead of the 5-bit weight table, np.pad / np.bincount /
np.cumsum instead of index reflection and counting loops, 200-bit mpmath instead of double -- so that a shared misreading has to be made
twice.

Every function returns its result plus a collections.Counter of the branches it took; tests/test_second_reading_ingest_cpu.py wants
every branch in BRANCHES reached by the shared cases.

What is still taken on trust: that OpenCV 4.x is the version (3.x has other gray coefficients and another CLAHE residual rule); x86's
cvRound on out-of-range and non-finite values (INT_MIN, which saturate_cast<short> of `>> 5` sends outside every image); five
fixed-point passes of undistortPoints with no epsilon test (TermCriteria(MAX_ITER, 5, 0.01) on this call path).
"""
from collections import Counter
from fractions import Fraction

import mpmath
import numpy as np

F = np.float32

BRANCHES = {
    "gray": {"ch3", "ch4", "red_first", "blue_first", "bits14", "bits15"},
    "remap": {"inside", "partial", "all_out", "nonfinite", "far", "integer_phase", "map_tie", "value_tie", "negative", "neg_zero"},
    "clahe": {"divisible", "extended", "extended_divisible_dim", "area1", "single_tile", "no_clip", "clip_floor_1", "clip_above_tile",
              "nothing_clipped", "residual0", "step1", "step2", "step>=3", "clamp_low_x", "clamp_high_x", "clamp_low_y", "clamp_high_y"},
    "undistort": {"five_passes", "icdist_negative", "copy", "radial", "tangential", "rational", "thin_prism"},
}


# ----------------------------------------------------------------------------------------------------------------------------------
# cvtColor(COLOR_{RGB,BGR,RGBA,BGRA}2GRAY), 8 bit
# ----------------------------------------------------------------------------------------------------------------------------------
GRAY_COEF = {14: (4899, 9617, 1868), 15: (9798, 19235, 3735)}          # (RY, GY, BY) for OpenCV 3.x / 4.x


def gray_ideal(r, g, b):
    """round(0.299 R + 0.587 G + 0.114 B) in exact rationals (half up; the check below allows 1 anyway)."""
    v = Fraction(299, 1000) * int(r) + Fraction(587, 1000) * int(g) + Fraction(114, 1000) * int(b)
    return (v + Fraction(1, 2)).__floor__()


def gray_from_color(img, blue_first, bits):
    """img [h][w][3|4] uint8 -> ([h][w] uint8, Counter).  gray = (R*RY + G*GY + B*BY + 2^(bits-1)) >> bits; alpha is ignored;
    blue_first swaps the outer two coefficients."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (3, 4) and bits in GRAY_COEF
    taken = Counter()
    taken["ch%d" % img.shape[2]] += 1
    taken["blue_first" if blue_first else "red_first"] += 1
    taken["bits%d" % bits] += 1
    ry, gy, by = GRAY_COEF[bits]
    assert ry + gy + by == 1 << bits                                  # white stays 255, gray stays gray
    coef = np.array([by, gy, ry] if blue_first else [ry, gy, by], np.int64)
    acc = np.tensordot(img[..., :3].astype(np.int64), coef, axes=([2], [0]))
    out = (acc + (1 << (bits - 1))) >> bits
    assert out.min() >= 0 and out.max() <= 255
    # cross-check against the definition the coefficients approximate: exact integers, 2000 * (0.299 R + ...) = 2 * (299 R + ...)
    rgb = img[..., :3][..., ::-1] if blue_first else img[..., :3]
    ideal = (2 * np.tensordot(rgb.astype(np.int64), np.array([299, 587, 114], np.int64), axes=([2], [0])) + 1000) // 2000
    assert np.abs(out - ideal).max() <= 1
    return out.astype(np.uint8), taken


# ----------------------------------------------------------------------------------------------------------------------------------
# remap(INTER_LINEAR, BORDER_CONSTANT 0), 8 bit, CV_32F maps
# ----------------------------------------------------------------------------------------------------------------------------------
def map_coordinate(v, taken=None):
    """One map entry -> its source coordinate as a Fraction with denominator 32, or None where the entry is outside every image:
    s = round_half_even(float32(v) * float32(32)); not finite, or |s| >> 5 above 32767 (what saturate_cast<short> cannot hold) -> None."""
    taken = Counter() if taken is None else taken
    with np.errstate(all="ignore"):
        t = F(F(v) * F(32))
    if not np.isfinite(t):
        taken["nonfinite"] += 1
        return None
    exact = Fraction(float(t))
    if exact.denominator == 2:
        taken["map_tie"] += 1
    s = round(exact)                                                  # Python rounds a Fraction half to even
    if (abs(s) >> 5) > 32767:
        taken["far"] += 1
        return None
    if s < 0:
        taken["negative"] += 1
    if s == 0 and np.signbit(F(v)):
        taken["neg_zero"] += 1
    return Fraction(s, 32)


def remap_linear(img, mapx, mapy):
    """img [sh][sw] uint8, maps [dh][dw] float32 -> ([dh][dw] uint8, Counter): exact bilinear interpolation of the zero-extended
    source at the coordinate of map_coordinate, rounded as floor(exact + 1/2)."""
    img = np.asarray(img); mapx = np.asarray(mapx, F); mapy = np.asarray(mapy, F)
    assert img.dtype == np.uint8 and img.ndim == 2 and mapx.shape == mapy.shape and mapx.ndim == 2
    sh, sw = img.shape
    dh, dw = mapx.shape
    ext = np.pad(img.astype(np.int64), 2)                             # two zero columns / rows on every side
    out = np.zeros((dh, dw), np.uint8)
    taken = Counter()
    half = Fraction(1, 2)
    for j in range(dh):
        for i in range(dw):
            cx = map_coordinate(mapx[j, i], taken); cy = map_coordinate(mapy[j, i], taken)
            if cx is None or cy is None:
                continue                                              # border value 0
            ix = cx.__floor__(); iy = cy.__floor__()
            a = cx - ix; b = cy - iy
            if a == 0 and b == 0:
                taken["integer_phase"] += 1
            nin = sum(1 for x in (ix, ix + 1) for y in (iy, iy + 1) if 0 <= x < sw and 0 <= y < sh)
            taken["inside" if nin == 4 else "all_out" if nin == 0 else "partial"] += 1
            ex = min(max(ix, -2), sw) + 2; ey = min(max(iy, -2), sh) + 2       # beyond the zero band everything is zero anyway
            p = ext[ey:ey + 2, ex:ex + 2]
            exact = ((1 - a) * int(p[0, 0]) + a * int(p[0, 1])) * (1 - b) + ((1 - a) * int(p[1, 0]) + a * int(p[1, 1])) * b
            r = exact + half
            if r.denominator == 1:
                taken["value_tie"] += 1
            out[j, i] = r.__floor__()
    return out, taken


def prove_rounding():
    """floor(exact + 1/2) == (sum + 2^14) >> 15 for the integer weights 32 (32-fx)(32-fy) ..: for every one of the 32 x 32 phases the
    four integer weights are 2^15 times the exact bilinear weights, hence sum to 2^15, hence sum / 2^15 is the exact value."""
    for fy in range(32):
        for fx in range(32):
            a, b = Fraction(fx, 32), Fraction(fy, 32)
            exact = [(1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b]
            ints = [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
            if [e * (1 << 15) for e in exact] != ints or sum(ints) != 1 << 15:
                return False
    return True


# ----------------------------------------------------------------------------------------------------------------------------------
# CLAHE, OpenCV 4.x
# ----------------------------------------------------------------------------------------------------------------------------------
def clahe_geometry(w, h, tiles, taken=None):
    """-> (right extension, bottom extension, tile width, tile height).  As soon as ONE dimension is no multiple of its tile count BOTH
    are extended by tiles - size % tiles: the dimension that divides grows by a full tile count."""
    taken = Counter() if taken is None else taken
    tx, ty = tiles
    if w % tx == 0 and h % ty == 0:
        taken["divisible"] += 1
        return 0, 0, w // tx, h // ty
    taken["extended"] += 1
    if w % tx == 0 or h % ty == 0:
        taken["extended_divisible_dim"] += 1
    px, py = tx - w % tx, ty - h % ty
    return px, py, (w + px) // tx, (h + py) // ty


def clip_value(clip_limit, area, taken=None):
    """clip = max(int(clip_limit * area / 256), 1) when clip_limit > 0, else 0 = no clipping."""
    taken = Counter() if taken is None else taken
    if not clip_limit > 0:
        taken["no_clip"] += 1
        return 0
    c = int(float(clip_limit) * area / 256)
    if c < 1:
        taken["clip_floor_1"] += 1
        c = 1
    if c > area:
        taken["clip_above_tile"] += 1
    return c


def clip_and_spread(hist, clip, taken=None):
    """Steps 2 and 3 for one tile: clip, clipped // 256 to every bin, the residual as +1 on bins 0, step, 2 step, ..."""
    taken = Counter() if taken is None else taken
    hist = np.asarray(hist, np.int64).copy()
    assert hist.shape == (256,)
    if clip <= 0:
        return hist
    clipped = int(np.maximum(hist - clip, 0).sum())
    if clipped == 0:
        taken["nothing_clipped"] += 1
    hist = np.minimum(hist, clip) + clipped // 256
    residual = clipped % 256
    if residual == 0:
        taken["residual0"] += 1
        return hist
    step = max(256 // residual, 1)
    taken["step1" if step == 1 else "step2" if step == 2 else "step>=3"] += 1
    bins = np.arange(0, 256, step)[:residual]                          # residual * step <= 256: the residual is always spent
    assert len(bins) == residual
    hist[bins] += 1
    return hist


def _round_saturate(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)                # np.rint rounds half to even


def clahe(img, clip_limit, tiles):
    """img [h][w] uint8 -> ([h][w] uint8, Counter)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    tx, ty = tiles
    taken = Counter()
    px, py, tw, th = clahe_geometry(w, h, tiles, taken)
    ext = np.pad(img, ((0, py), (0, px)), mode="reflect") if (px or py) else img   # numpy's "reflect" is OpenCV's REFLECT_101
    area = tw * th
    if area == 1:
        taken["area1"] += 1
    if tx == 1 or ty == 1:
        taken["single_tile"] += 1
    clip = clip_value(clip_limit, area, taken)
    scale = F(255) / F(area)
    luts = np.zeros((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            tile = ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            hist = clip_and_spread(np.bincount(tile.ravel(), minlength=256), clip, taken)
            assert hist.sum() == area
            luts[j, i] = _round_saturate(np.cumsum(hist).astype(F) * scale)

    def axis(n, t, ntiles, name):
        f = np.arange(n).astype(F) * (F(1) / F(t)) - F(0.5)
        lo = np.floor(f)
        wa = (f - lo).astype(F); wa1 = (F(1) - wa).astype(F)
        lo = lo.astype(np.int64); hi = lo + 1                          # the weights are taken before the clamp
        if (lo < 0).any():
            taken["clamp_low_" + name] += 1
        if (hi > ntiles - 1).any():
            taken["clamp_high_" + name] += 1
        return np.maximum(lo, 0), np.minimum(hi, ntiles - 1), wa, wa1

    x1, x2, xa, xa1 = axis(w, tw, tx, "x")
    y1, y2, ya, ya1 = axis(h, th, ty, "y")
    v = img.astype(np.int64)
    Y1, Y2, X1, X2 = y1[:, None], y2[:, None], x1[None, :], x2[None, :]
    l11 = luts[Y1, X1, v].astype(F); l12 = luts[Y1, X2, v].astype(F)
    l21 = luts[Y2, X1, v].astype(F); l22 = luts[Y2, X2, v].astype(F)
    XA, XA1, YA, YA1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    top = l11 * XA1 + l12 * XA                                         # every numpy operation below is one float32 operation
    bot = l21 * XA1 + l22 * XA
    res = top * YA1 + bot * YA
    assert res.dtype == F
    return _round_saturate(res), taken


# ----------------------------------------------------------------------------------------------------------------------------------
# undistortPoints(K, D, R = I, P = newK) and the forward model
# ----------------------------------------------------------------------------------------------------------------------------------
def _coefficients(dist):
    """OpenCV's order (k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4[, tauX, tauY]) widened from float32."""
    d = [float(F(c)) for c in dist]
    if len(d) > 14:
        raise ValueError("at most 14 distortion coefficients")
    if any(c != 0 for c in d[12:]):
        raise NotImplementedError("the tilted sensor model is not part of this reading")
    d = (d + [0.0] * 12)[:12]
    return [mpmath.mpf(c) for c in d]


def _wide(values):
    return [mpmath.mpf(float(F(c))) for c in values]


def undistort_exact(u, v, K, dist, newK, iters=5, prec=200, taken=None):
    """One point at `prec` bits -> (u', v') as mpf.  x0 = (u - cx) / fx, then `iters` passes of the fixed-point step; a negative icdist
    returns the start point."""
    taken = Counter() if taken is None else taken
    with mpmath.workprec(prec):
        fx, fy, cx, cy = _wide(K)
        nfx, nfy, ncx, ncy = _wide(newK)
        k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coefficients(dist)
        x0 = (mpmath.mpf(float(F(u))) - cx) / fx
        y0 = (mpmath.mpf(float(F(v))) - cy) / fy
        x, y = x0, y0
        for _ in range(iters):
            r2 = x * x + y * y
            icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
            if icdist < 0:
                taken["icdist_negative"] += 1
                x, y = x0, y0
                break
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 * r2
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 * r2
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
        else:
            taken["five_passes" if iters == 5 else "other_passes"] += 1
        return nfx * x + ncx, nfy * y + ncy


def _to_float32(value, prec):
    """A `prec`-bit value -> (nearest float32, undecidable).  undecidable: the value lies within 2^-44 |value| of the midpoint between
    two float32 neighbours, where a double evaluation could round the other way."""
    with mpmath.workprec(prec):
        f = F(float(value))                                            # via double: exact wherever `undecidable` is False
        if not np.isfinite(f):
            return f, True
        margin = mpmath.ldexp(abs(value), -44)
        for other in (np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))):
            mid = (mpmath.mpf(float(f)) + mpmath.mpf(float(other))) / 2
            if abs(value - mid) <= margin:
                return f, True
        return f, False


def undistort(u, v, K, dist, newK, iters=5, prec=200):
    """u, v: float32 arrays -> ([n][2] float32, undecidable [n] bool, Counter).  This is cv::undistortPoints itself: the copy for
    dist[0] == 0 is Frame::UndistortKeyPoints' and lives in undistort_keypoints."""
    u = np.atleast_1d(np.asarray(u, F)); v = np.atleast_1d(np.asarray(v, F))
    taken = Counter()
    d = [float(F(c)) for c in dist] + [0.0] * 12
    for name, idx in (("radial", (0, 1, 4)), ("tangential", (2, 3)), ("rational", (5, 6, 7)), ("thin_prism", (8, 9, 10, 11))):
        if any(d[i] != 0 for i in idx):
            taken[name] += 1
    out = np.zeros((len(u), 2), F); und = np.zeros(len(u), bool)
    for i in range(len(u)):
        a, b = undistort_exact(u[i], v[i], K, dist, newK, iters, prec, taken)
        out[i, 0], ua = _to_float32(a, prec)
        out[i, 1], ub = _to_float32(b, prec)
        und[i] = ua or ub
    return out, und, taken


def undistort_keypoints(u, v, K, dist, newK):
    """Frame::UndistortKeyPoints: a first coefficient of zero (or none at all) copies the coordinates."""
    if len(dist) < 1 or float(F(dist[0])) == 0.0:
        u = np.atleast_1d(np.asarray(u, F)); v = np.atleast_1d(np.asarray(v, F))
        return np.stack([u, v], axis=1), np.zeros(len(u), bool), Counter({"copy": 1})
    return undistort(u, v, K, dist, newK)


def distort(x, y, K, dist, prec=200):
    """The forward Brown-Conrady model with rational and thin-prism terms: a normalised point -> its pixel, as mpf."""
    with mpmath.workprec(prec):
        fx, fy, cx, cy = _wide(K)
        k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coefficients(dist)
        x = mpmath.mpf(x); y = mpmath.mpf(y)
        r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
        radial = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
        xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r4
        yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r4
        return fx * xd + cx, fy * yd + cy


def round_trip_error(u, v, K, dist, iters=60, prec=200):
    """|distort(undistort(p)) - p| in pixels, the larger of the two coordinates, as a float."""
    with mpmath.workprec(prec):
        x, y = undistort_exact(u, v, K, dist, (1.0, 1.0, 0.0, 0.0), iters, prec)
        uu, vv = distort(x, y, K, dist, prec)
        return float(max(abs(uu - mpmath.mpf(float(F(u)))), abs(vv - mpmath.mpf(float(F(v))))))


def image_bounds(cols, rows, K, dist, newK):
    """Frame::ComputeImageBounds -> ((minX, maxX, minY, maxY) float32, undecidable, Counter): the corners (0,0), (cols,0), (0,rows),
    (cols,rows) undistorted; minX from the two left corners, maxX from the two right ones, minY from the two upper ones, maxY from the
    two lower ones (Frame.cc:1005-1008).  A first coefficient of zero gives the image rectangle."""
    if len(dist) < 1 or float(F(dist[0])) == 0.0:
        return np.array([0, cols, 0, rows], F), False, Counter({"copy": 1})
    p, und, taken = undistort(np.array([0, cols, 0, cols], F), np.array([0, 0, rows, rows], F), K, dist, newK)
    b = np.array([min(p[0, 0], p[2, 0]), max(p[1, 0], p[3, 0]), min(p[0, 1], p[1, 1]), max(p[2, 1], p[3, 1])], F)
    return b, bool(und.any()), taken
