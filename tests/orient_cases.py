"""cv::fastAtan2 stated in float32 numpy, and small frames chosen for k_orient_desc2's patch, lane-group and frame geometry.

fast_atan2_np is SURVEY A.4 word for word: every product and sum rounded to float32 on its own, `ax >= ay` takes the tie, eps is
float(DBL_EPSILON).  With umax_table / moments / descriptors of tests/test_oracle_structured_cpu.py it states IC_Angle and
computeOrbDescriptor (ORBextractor.cc:91-138, :150-202) without any code of the oracle or the product; this file imports neither.

The steered dot: a one-pixel dot on a flat background is a FAST corner whose 31-px disc is symmetric (both moments 0, angle 0).  A
half-plane painted inside the dot's 31 x 31 box, `dx u + dy v >= d0 (|dx| + |dy|)` clipped to u^2 + v^2 <= 17^2, tips the centroid
towards (dx, dy) and leaves FAST's ring (radius 3) flat for d0 >= 4.  The eight directions give the exact cases of fastAtan2: the
half-plane of an axis is symmetric about it (the other moment is 0), that of a diagonal under u <-> v or u <-> -v (|m01| == |m10|,
c == 1 exactly), as the umax disc is.

k_orient_desc2 packs four keypoints into a wave and sixteen into a workgroup, deals the workgroups of the first 8 * (frames / 8)
frames over the XCDs, fetches a 37-row blurred patch as 48-byte rows from (cx - 18) & ~7 out of 16 x 8-px tiles (40-byte rows from
(cx - 18) & ~3 on row-major levels), and reads rows cy - 18 .. cy + 18.  What decides which piece, which tile, which lane and which
frame meets which keypoint is: how close a keypoint is to each border (19 px at the least) and where its rotated pattern reaches;
(cx - 18) & 7 and (cy - 18) & 7; the level's width (w % 16, and w % 64 in {0, 62, 63}, where a patch row at x = w - 20 reaches into
the extra tile column btpr - 1) and height (h % 8); n % 4, n % 16 and n == 0; the batch size against 8.  FRAMES and batch_images list
frames that contain every such class; tests/test_orient_cases_cpu.py derives the classes from the oracle and fails if a frame stops
containing the class it is listed for."""
import numpy as np

INI_TH, MIN_TH = 20, 7
DIRECTIONS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))    # 0, 45, ..., 315 degrees (y points down)
REACH = 18                                                   # the rotated pattern's largest |row|, |column| (test_pattern_reach)
MOMENT_BOUND = 624240                                        # 255 * sum of u over the u > 0 half of the umax disc (test_moment_bound)


# ---- cv::fastAtan2 ----
def fast_atan2_np(y, x):
    """cv::fastAtan2(y, x) in degrees for float32 arrays (or scalars): float32 throughout, no contraction."""
    f = np.float32
    y = np.asarray(y, f); x = np.asarray(x, f)
    scalar = y.ndim == 0 and x.ndim == 0
    y, x = np.broadcast_arrays(np.atleast_1d(y), np.atleast_1d(x))
    s = f(180.0 / np.pi)
    p1, p3, p5, p7 = (f(f(c) * s) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    eps = f(np.finfo(np.float64).eps)
    ax, ay = np.abs(x), np.abs(y)
    xbig = ax >= ay
    num = np.where(xbig, ay, ax).astype(f)
    den = (np.where(xbig, ax, ay).astype(f) + eps).astype(f)
    c = (num / den).astype(f)
    c2 = (c * c).astype(f)
    a = ((p7 * c2).astype(f) + p5).astype(f)
    a = ((a * c2).astype(f) + p3).astype(f)
    a = ((a * c2).astype(f) + p1).astype(f)
    a = (a * c).astype(f)
    a = np.where(xbig, a, (f(90) - a).astype(f)).astype(f)
    a = np.where(x < 0, (f(180) - a).astype(f), a).astype(f)
    a = np.where(y < 0, (f(360) - a).astype(f), a).astype(f)
    return f(a[0]) if scalar else a


A45 = fast_atan2_np(1.0, 1.0)                                # |y| == |x|: the float32 sum of the four coefficients
EXACT_ANGLES = tuple(np.float32(v) for v in (0.0, A45, 90.0, np.float32(180) - A45, 180.0, np.float32(180) + A45, 270.0, np.float32(360) - A45))
# (180 + a45 is fastAtan2's 360 - (180 - a45); the two are the same float32: test_fast_atan2_np_exact_cases)


# ---- the steered dot ----
def half_plane(direction, d0):
    """[(u, v)] of the steered dot's half-plane inside its 31 x 31 box."""
    dx, dy = direction
    out = []
    for v in range(-15, 16):
        for u in range(-15, 16):
            if dx * u + dy * v >= d0 * (abs(dx) + abs(dy)) and u * u + v * v <= 17 * 17:
                out.append((u, v))
    return out


def paint(w, h, dots, bg=40, amp=200, d0=5):
    """uint8 (h, w): `bg` everywhere; every dot (x, y, direction index or None) is one pixel of 255 (0 where amp < bg) with its
    half-plane at value `amp`.  The boxes of two dots never overlap and every box lies inside the frame."""
    img = np.full((h, w), bg, np.uint8)
    for i, (x, y, d) in enumerate(dots):
        assert 15 <= x < w - 15 and 15 <= y < h - 15, (x, y)
        for a, b, _ in dots[:i]:
            assert max(abs(a - x), abs(b - y)) >= 31 or (d is None and max(abs(a - x), abs(b - y)) >= 8), (x, y, a, b)
        if d is not None:
            for u, v in half_plane(DIRECTIONS[d % 8], d0):
                img[y + v, x + u] = amp
        img[y, x] = 255 if amp >= bg else 0
    return img


def border_dots(w, h, turn=0):
    """14 steered dots 19 px from the borders: the corners, three each on the first and the last row FAST evaluates, two each on the
    first and the last column.  Along y = 19 they are steered to 45 degrees, along y = h - 20 to 225, along x = 19 to 315, along
    x = w - 20 to 135 (the pattern's point (-13, -13) then lands 18 px towards the border); `turn` rotates the direction table."""
    top, bottom, left, right = 1 + turn, 5 + turn, 7 + turn, 3 + turn
    xs_top = [19 + (w - 39) * k // 4 + k for k in (1, 2, 3)]
    xs_bot = [19 + (w - 39) * k // 4 - 2 * k - 1 for k in (1, 2, 3)]
    ys_l = [19 + (h - 39) * k // 3 + k for k in (1, 2)]
    ys_r = [19 + (h - 39) * k // 3 - 2 * k - 1 for k in (1, 2)]
    dots = [(19, 19, top), (w - 20, 19, right), (w - 20, h - 20, bottom), (19, h - 20, left)]
    dots += [(x, 19, top) for x in xs_top] + [(x, h - 20, bottom) for x in xs_bot]
    dots += [(19, y, left) for y in ys_l] + [(w - 20, y, right) for y in ys_r]
    return dots


def border_frame(w, h, turn=0, bg=40, amp=200, d0=5):
    return paint(w, h, border_dots(w, h, turn), bg, amp, d0)


def doubled(img):
    """Every pixel as a 2 x 2 block: at scale factor 2.0 the bilinear level 1 is `img` again, byte for byte."""
    return np.kron(img, np.ones((2, 2), np.uint8))


def lattice_dots(w, h, n, pitch=24, steer=False, first=0):
    """n dots `pitch` px apart in reading order from (24, 24), unsteered (isolated pixels) or steered with the direction table in turn."""
    if steer:
        pitch = max(pitch, 34)
    per_row = (w - 48) // pitch + 1
    assert n <= per_row * ((h - 48) // pitch + 1), (w, h, n)
    return [(24 + pitch * (i % per_row), 24 + pitch * (i // per_row), (first + i) % 8 if steer else None) for i in range(n)]


def spread_dots(n):
    """n <= 17 isolated dots inside COUNT_SIZE placed for the quadtree (inner area 128 x 112, split at 64 / 56, then 32 / 28, then
    16 / 14): dot i < 16 sits in cell i of the 4 x 4 grid taken quadrant by quadrant, so that every prefix spreads over the quadrants
    and no node ever hands all its dots to one child (DistributeOctTree stops at the first pass that does not grow its list:
    tests/extract_cases.py, two_close_dots_N5); the 17th shares cell 0 with dot 0, in another sixteenth."""
    assert 0 <= n <= 17
    out = []
    for i in range(min(n, 16)):
        qx, qy, sx, sy = i & 1, (i >> 1) & 1, (i >> 2) & 1, (i >> 3) & 1
        out.append((16 + 64 * qx + 32 * sx + 6, 16 + 56 * qy + 28 * sy + 6, None))
    if n == 17:
        out.append((16 + 24, 16 + 20, None))
    return out


def compass_frame(w, h, turn=0, bg=40, amp=200, d0=5):
    """As many steered dots as fit, 34 px apart, the eight directions in turn."""
    per_row, rows = (w - 48) // 34 + 1, (h - 48) // 34 + 1
    return paint(w, h, lattice_dots(w, h, per_row * rows, steer=True, first=turn), bg, amp, d0)


# ---- frames ----
# name -> dict(img, nf, sf, nl).  Level sizes and what each frame is listed for (test_frames_contain_the_classes holds them to it):
#  border_257x183   257 x 183, 214 x 153, 178 x 127, 149 x 106: samples on row 1, row h - 2, column 1, column w - 2 of level 0; w % 16 == 1, h % 8 == 7
#  border_256x200   w % 16 == 0 and w % 64 == 0 (a patch row at x = w - 20 ends in tile column btpr - 1), h % 8 == 0
#  border_247x185   w % 16 == 7, h % 8 == 1
#  border_255x193   w % 16 == 15 and w % 64 == 63 (tile column btpr - 1 again), h % 8 == 1
#  doubled_*        the same four at twice the size, sf 2.0, two levels: level 1 is the small frame, so the same border, width and
#                   height classes on a level the resize made, read from the pyramid and not from the caller's buffer
#  compass_240x200  every direction several times on one level: the eight exact angles
#  sat_*            bg 0 / amp 255 and bg 255 / amp 0 at d0 4: |m| >= 0.9 of the bound with every sign pair; bg 255 with dark dots
#                   and no half-plane: m01 == m10 == 0 at the largest a1 and a2
#  count_N          N isolated dots on one level, N in COUNTS (0: a flat frame); one more dot than a wave / a workgroup holds, one fewer, as many
SIZES = ((257, 183), (256, 200), (247, 185), (255, 193))
COUNTS = (0, 1, 3, 4, 5, 15, 16, 17)
COUNT_SIZE = (160, 144)


def _frames():
    out = {}
    for w, h in SIZES:
        out["border_%dx%d" % (w, h)] = dict(img=border_frame(w, h), nf=300, sf=1.2, nl=4)
    for i, (w, h) in enumerate(SIZES):
        out["doubled_%dx%d" % (w, h)] = dict(img=doubled(border_frame(w, h, turn=0 if i == 0 else 2 * i)), nf=300, sf=2.0, nl=2)
    out["compass_240x200"] = dict(img=compass_frame(240, 200), nf=300, sf=1.2, nl=3)
    out["sat_dark_bg"] = dict(img=compass_frame(240, 200, 1, bg=0, amp=255, d0=4), nf=300, sf=1.2, nl=3)
    out["sat_bright_bg"] = dict(img=compass_frame(240, 200, 2, bg=255, amp=0, d0=4), nf=300, sf=1.2, nl=3)
    out["sat_bright_dots"] = dict(img=paint(240, 200, lattice_dots(240, 200, 40), bg=255, amp=0), nf=300, sf=1.2, nl=3)
    for n in COUNTS:
        out["count_%d" % n] = dict(img=paint(COUNT_SIZE[0], COUNT_SIZE[1], spread_dots(n)), nf=100, sf=1.2, nl=1)
    for f in out.values():
        f["img"].setflags(write=False)
    return out


FRAMES = _frames()
BORDER = ["border_%dx%d" % s for s in SIZES]
DOUBLED = ["doubled_%dx%d" % s for s in SIZES]
SATURATED = ["sat_dark_bg", "sat_bright_bg", "sat_bright_dots"]
COUNT = ["count_%d" % n for n in COUNTS]

# ---- batches: frames of one size whose images all differ, with very different n (0 included) ----
BATCH_SIZES = (1, 7, 8, 9, 16, 17)
BATCH_W, BATCH_H = 160, 144
BATCH_PARAMS = dict(nf=100, sf=1.2, nl=2)
# dots per frame by position: 0 and 12 next to each other at the dealt positions (0 .. 8 * (B / 8) - 1) and at the undealt ones behind them
_BATCH_N = (5, 0, 12, 1, 9, 11, 3, 0, 12, 4, 0, 7, 2, 10, 6, 8, 0)


def batch_images(size):
    """The frames of the batch of `size`: frame i has its own number of steered dots (0: a flat frame of its own grey level), the
    direction table rotated by i."""
    imgs = []
    for i in range(size):
        n = _BATCH_N[(i + size) % len(_BATCH_N)] if size > 1 else 5
        img = paint(BATCH_W, BATCH_H, lattice_dots(BATCH_W, BATCH_H, n, steer=True, first=i), bg=40 + i, amp=200 - i)
        img.setflags(write=False)
        imgs.append(img)
    return imgs


# ---- the statement ----
def statement(level, blurred, xs, ys, pattern):
    """(angle float32 [n], descriptors uint8 [n, 32], m01, m10) of the keypoints (xs, ys) of one level: IC_Angle on the un-blurred
    level, computeOrbDescriptor on the blurred one."""
    from test_oracle_structured_cpu import descriptors, moments
    m01, m10 = moments(level, xs, ys)
    assert max(np.abs(m01).max(initial=0), np.abs(m10).max(initial=0)) <= MOMENT_BOUND < 2 ** 24      # the casts to float32 are exact
    angle = fast_atan2_np(m01.astype(np.float32), m10.astype(np.float32))
    return angle, descriptors(blurred, xs, ys, angle, pattern), m01, m10


def sample_offsets(angle, pattern):
    """(rows, columns) int64 [n, 512] of computeOrbDescriptor's samples about the keypoint (ORBextractor.cc:163-170)."""
    factor_pi = np.float32(np.pi / np.float64(np.float32(180.0)))
    rad = (np.asarray(angle, np.float32) * factor_pi).astype(np.float32)
    a = np.cos(rad.astype(np.float64)).astype(np.float32)[:, None]
    b = np.sin(rad.astype(np.float64)).astype(np.float32)[:, None]
    pat = pattern.astype(np.float32).reshape(512, 2)
    px = pat[None, :, 0]; py = pat[None, :, 1]
    row = np.rint(((px * b).astype(np.float32) + (py * a).astype(np.float32)).astype(np.float32)).astype(np.int64)
    col = np.rint(((px * a).astype(np.float32) - (py * b).astype(np.float32)).astype(np.float32)).astype(np.int64)
    return row, col
