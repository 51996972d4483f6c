"""tests/orient_cases.py on the CPU: hand-worked answers of the float32 statement of cv::fastAtan2 and of the steered dot, the oracle's
fastAtan2 held to the statement, the proof that no descriptor sample leaves the 37-row patch, and the condition that the frames contain
every class of k_orient_desc2's geometry they are listed for -- derived from the oracle's level_size and level_keypoints and the
statement, so that a later edit cannot quietly turn them into ordinary frames.  The oracle is then held to the statement on every frame."""
import numpy as np
import pytest

import orient_cases as oc
from blur_cases import gauss7_exact
from orient_cases import A45, FRAMES, MOMENT_BOUND, fast_atan2_np
from test_oracle_structured_cpu import GAUSS7, check_orientation_and_descriptors, moments, umax_table

_facts = {}


def facts(oracle, name):
    """Per level of a frame on the oracle: (w, h, xyr, angle, m01, m10, sample rows, sample columns); computed once."""
    if name not in _facts:
        f = FRAMES[name]
        ref = oracle.Extractor(f["nf"], f["sf"], f["nl"], oc.INI_TH, oc.MIN_TH)
        n = ref(f["img"], (0, 0))[0]
        assert n >= 0, name
        out = []
        for l in range(f["nl"]):
            w, h = ref.level_size(l)
            xyr, ang = ref.level_keypoints(l)
            if len(xyr):
                a, d, m01, m10 = oc.statement(ref.level_image(l), ref.level_image(l, blurred=True), xyr[:, 0], xyr[:, 1], oracle.pattern())
                assert a.tobytes() == ang.tobytes(), (name, l)
                r, c = oc.sample_offsets(a, oracle.pattern())
                out.append((w, h, xyr, a, m01, m10, xyr[:, 1][:, None] + r, xyr[:, 0][:, None] + c))
            else:
                z = np.zeros(0, np.int64)
                out.append((w, h, xyr, ang, z, z, np.zeros((0, 512), np.int64), np.zeros((0, 512), np.int64)))
        _facts[name] = (n, out, ref.level_image(1).copy() if f["nl"] > 1 else None)
    return _facts[name]


# ---- hand-worked answers ----
def test_fast_atan2_np_exact_cases():
    """Where no polynomial error is involved: the origin, the axes, and |y| == |x| (c == 1 exactly -- eps is below half an ulp of any
    non-zero moment -- and `ax >= ay` takes the tie), whose value is the float32 sum of the four coefficients."""
    f = np.float32
    assert fast_atan2_np(0.0, 0.0) == 0.0
    for y, x, want in [(0, 5, 0.0), (5, 0, 90.0), (0, -5, 180.0), (-5, 0, 270.0), (0, 1e6, 0.0), (3e5, 0, 90.0), (0, MOMENT_BOUND, 0.0),
                       (-MOMENT_BOUND, 0, 270.0)]:
        assert fast_atan2_np(float(y), float(x)) == f(want), (y, x)
    s = f(180.0 / np.pi)
    p1, p3, p5, p7 = (f(c) * s for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    a45 = f(f(f(p7 + p5) + p3) + p1)
    assert A45 == a45 and abs(float(a45) - 45.0) < 0.02
    for m in (1.0, 7.0, 255.0, 120000.0, float(MOMENT_BOUND)):
        assert fast_atan2_np(m, m) == a45 and fast_atan2_np(m, -m) == f(180) - a45
        assert fast_atan2_np(-m, -m) == f(360) - (f(180) - a45) and fast_atan2_np(-m, m) == f(360) - a45
    assert f(360) - (f(180) - a45) == f(180) + a45                    # EXACT_ANGLES names it 180 + a45
    assert len(set(float(a) for a in oc.EXACT_ANGLES)) == 8
    y = np.array([0, 5, -5, 3], f); x = np.array([0, 5, 0, -3], f)  # arrays as well
    assert fast_atan2_np(y, x).tolist() == [0.0, float(a45), 270.0, float(f(180) - a45)]


def test_moment_bound():
    um = umax_table()
    half = sum(sum(range(1, um[abs(v)] + 1)) for v in range(-15, 16))
    assert 255 * half == MOMENT_BOUND == 624240
    # the kernel's intermediate sums on an all-255 disc: a2 = sum of I, a1 = sum of (u + 16) I; m10 = a1 - 16 a2
    npx = sum(2 * um[abs(v)] + 1 for v in range(-15, 16))
    assert npx == 749 and 255 * 16 * npx < 2 ** 24


def test_the_angle_stays_below_360():
    """The smallest negative m01 against the largest m10: fastAtan2 stays below 360, so ar = angle * factorPI stays inside the domain
    od_sincos was checked on.  360.0 itself would need 360 - a to round up to 360, a < 2^-16 degrees: |m01| / m10 < 3e-7, and the
    smallest non-zero quotient of integer moments of an 8-bit disc is 1 / 624240 = 1.6e-6."""
    worst = fast_atan2_np(-1.0, float(MOMENT_BOUND))
    assert 359.99 < worst < 360.0
    assert fast_atan2_np(-1.0, float(MOMENT_BOUND)) == np.float32(360) - fast_atan2_np(1.0, float(MOMENT_BOUND))
    assert fast_atan2_np(1.0, float(MOMENT_BOUND)) > np.float32(2.0 ** -15)


def test_single_dot_by_hand(oracle):
    """A single dot: the disc is symmetric, both moments 0, angle 0; the pattern is read unrotated from the 7 x 7 impulse response."""
    img = oc.paint(120, 100, [(60, 50, None)], bg=0, amp=255)
    assert img.sum() == 255 and img[50, 60] == 255
    ang, desc, m01, m10 = oc.statement(img, gauss7_exact(img), np.array([60]), np.array([50]), oracle.pattern())
    assert m01[0] == 0 and m10[0] == 0 and ang[0] == 0.0
    g = np.zeros((41, 41), np.int64)
    g[17:24, 17:24] = (np.outer(GAUSS7, GAUSS7) * 255 + 32768) >> 16
    p = oracle.pattern().astype(np.int64).reshape(256, 4)
    bits = g[20 + p[:, 1], 20 + p[:, 0]] < g[20 + p[:, 3], 20 + p[:, 2]]
    assert np.array_equal(desc[0], np.packbits(bits, bitorder="little")) and 0 < int(bits.sum()) < 256


@pytest.mark.parametrize("d", range(8))
def test_steered_dot_moments_by_hand(d):
    """The half-plane's moment summed by hand from umax: the background and the centre pixel contribute nothing (the disc is symmetric,
    the centre has u = v = 0), every half-plane pixel inside the disc (amp - bg) times its coordinate."""
    bg, amp, d0 = 40, 200, 5
    dx, dy = oc.DIRECTIONS[d]
    img = oc.paint(80, 80, [(40, 40, d)], bg, amp, d0)
    um = umax_table()
    want10 = want01 = 0
    for v in range(-15, 16):
        for u in range(-um[abs(v)], um[abs(v)] + 1):
            if dx * u + dy * v >= d0 * (abs(dx) + abs(dy)):             # (the clip u^2 + v^2 <= 17^2 lies outside the disc)
                assert u * u + v * v <= 17 * 17
                want10 += u * (amp - bg); want01 += v * (amp - bg)
    m01, m10 = moments(img, np.array([40]), np.array([40]))
    assert (int(m01[0]), int(m10[0])) == (want01, want10)
    assert np.sign(want10) == dx and np.sign(want01) == dy
    if dx and dy:
        assert abs(want01) == abs(want10)
    if d == 0:        # u = 5 .. umax: 110 (v = 0) + 6 * 110 + 6 * 95 + 4 * 81 + 2 * (68 + 56 + 45 + 35 + 26 + 11 + 0) down the table
        assert want10 == 160 * sum(sum(range(5, um[abs(v)] + 1)) for v in range(-15, 16)) == 160 * 2146
    assert fast_atan2_np(float(want01), float(want10)) == oc.EXACT_ANGLES[d]


# ---- the oracle's fastAtan2 against the statement ----
def test_oracle_fast_atan2_equals_the_statement_on_a_lattice(oracle):
    f = oracle.lib().orbref_fast_atan2
    v = sorted(set(list(range(0, 34)) + [int(round(1.37 ** k)) for k in range(10, 43)] + [MOMENT_BOUND - k for k in (0, 1, 2, 255)] + [160 * 2146, 255 * 2146]))
    assert v[-1] == MOMENT_BOUND and len(v) > 60
    v = np.array([-x for x in v[:0:-1]] + v, np.float32)
    yy, xx = np.meshgrid(v, v, indexing="ij")
    want = fast_atan2_np(yy.ravel(), xx.ravel())
    got = np.array([f(float(y), float(x)) for y, x in zip(yy.ravel(), xx.ravel())], np.float32)
    assert got.tobytes() == want.tobytes()
    assert want.max() < 360.0 and want.min() == 0.0


def test_oracle_fast_atan2_equals_the_statement_on_every_case(oracle):
    f = oracle.lib().orbref_fast_atan2
    pairs = 0
    for name in FRAMES:
        for w, h, xyr, ang, m01, m10, rows, cols in facts(oracle, name)[1]:
            got = np.array([f(float(a), float(b)) for a, b in zip(m01, m10)], np.float32)
            assert got.tobytes() == ang.tobytes(), name
            pairs += len(m01)
    assert pairs > 1000


# ---- the patch holds every sample ----
def test_pattern_reach(oracle):
    """|row| = |x b + y a| <= |(x, y)| |(a, b)| <= sqrt(338 (1 + 1e-6)) = 18.385 (three float32 roundings move it by 3e-6 at the
    most), which rounds to 18 at the most: no sample leaves rows / columns -18 .. 18 of the patch, whatever the angle.  18 is attained
    in all four directions."""
    pat = oracle.pattern().astype(np.int64).reshape(512, 2)
    assert (pat ** 2).sum(1).max() == 338 and 338 * (1 + 1e-6) < 18.49 ** 2
    deg = np.concatenate([np.arange(0, 360 * 256, dtype=np.float64) / 256, np.array(oc.EXACT_ANGLES, np.float64)]).astype(np.float32)
    deg = np.concatenate([deg, np.nextafter(deg, np.float32(400)), np.float32([359.99997])])
    rad = (deg * np.float32(np.pi / np.float64(np.float32(180.0)))).astype(np.float32)
    a = np.cos(rad.astype(np.float64)).astype(np.float32).astype(np.float64)
    b = np.sin(rad.astype(np.float64)).astype(np.float32).astype(np.float64)
    assert (a * a + b * b).max() <= 1 + 1e-6
    lo_r = lo_c = hi_r = hi_c = 0
    for chunk in np.array_split(deg, 64):
        r, c = oc.sample_offsets(chunk, oracle.pattern())
        lo_r, hi_r, lo_c, hi_c = min(lo_r, r.min()), max(hi_r, r.max()), min(lo_c, c.min()), max(hi_c, c.max())
    assert (lo_r, hi_r, lo_c, hi_c) == (-oc.REACH, oc.REACH, -oc.REACH, oc.REACH)
    # the four steerings of the border dots send one sample 18 px towards their border
    r, c = oc.sample_offsets(np.array([oc.EXACT_ANGLES[i] for i in (1, 5, 7, 3)], np.float32), oracle.pattern())
    assert r[0].min() == -18 and r[1].max() == 18 and c[2].min() == -18 and c[3].max() == 18


# ---- the frames contain their classes ----
def _steered_found(level, dots):
    """How many of the dots are among the level's keypoints."""
    xy = set(map(tuple, level[2][:, :2].tolist()))
    return sum((x, y) in xy for x, y, _ in dots)


def test_frames_contain_the_classes(oracle):
    # every frame is one the product accepts: every level holds a 35-px cell inside its 16-px border, and a root for the quadtree
    for name in FRAMES:
        for w, h, *_ in facts(oracle, name)[1]:
            assert w >= 67 and h >= 67 and round((w - 32) / (h - 32)) >= 1, name
    # border frames: 14 of 14 dots on level 0, samples on row 1, row h - 2, column 1, column w - 2, keypoints 19 px from every border
    for name, (w, h) in zip(oc.BORDER, oc.SIZES):
        lv = facts(oracle, name)[1]
        assert (lv[0][0], lv[0][1]) == (w, h) and _steered_found(lv[0], oc.border_dots(w, h)) == 14, name
        assert (lv[0][6].min(), lv[0][6].max(), lv[0][7].min(), lv[0][7].max()) == (1, h - 2, 1, w - 2), name
        x, y = lv[0][2][:, 0], lv[0][2][:, 1]
        assert (x.min(), x.max(), y.min(), y.max()) == (19, w - 20, 19, h - 20), name
    # doubled frames: level 1 is the small frame byte for byte, with the same 14 dots and the same reach, on a level the resize made
    for i, (name, (w, h)) in enumerate(zip(oc.DOUBLED, oc.SIZES)):
        n, lv, level1 = facts(oracle, name)
        small = oc.border_frame(w, h, turn=0 if i == 0 else 2 * i)
        assert np.array_equal(level1, small) and (lv[1][0], lv[1][1]) == (w, h), name
        assert _steered_found(lv[1], oc.border_dots(w, h)) == 14, name
        x, y = lv[1][2][:, 0], lv[1][2][:, 1]
        assert (x.min(), x.max(), y.min(), y.max()) == (19, w - 20, 19, h - 20), name
        if i == 0:                                                       # (the turned ones are steered elsewhere)
            assert (lv[1][6].min(), lv[1][6].max(), lv[1][7].min(), lv[1][7].max()) == (1, h - 2, 1, w - 2), name
            assert np.array_equal(lv[1][2], facts(oracle, oc.BORDER[0])[1][0][2])
    # width and height classes, on level 0 and on a resized level, each with a keypoint at x = w - 20 / y = h - 20; the widths whose
    # patch row at x = w - 20 ends in the extra tile column: (w - 38) & ~7 + 40 >= align64(w)
    for names, l in ((oc.BORDER, 0), (oc.DOUBLED, 1)):
        wc, hc, extra = set(), set(), set()
        for name in names:
            w, h, xyr = facts(oracle, name)[1][l][:3]
            if (xyr[:, 0] == w - 20).any():
                wc.add(w % 16)
                if ((w - 38) & ~7) + 40 >= (w + 63) // 64 * 64:
                    extra.add(w % 64)
            if (xyr[:, 1] == h - 20).any():
                hc.add(h % 8)
        assert wc == {0, 1, 7, 15} and hc == {0, 1, 7} and extra == {0, 63}, (l, wc, hc, extra)
    # all eight column phases and row phases of the tiled fetch, on level 0 and on resized levels; of the row-major fetch, all four
    for resized in (False, True):
        cp, rp = set(), set()
        for name in FRAMES:
            for l, lvl in enumerate(facts(oracle, name)[1]):
                if (l > 0) == resized:
                    cp |= set(((lvl[2][:, 0] - 18) & 7).tolist()); rp |= set(((lvl[2][:, 1] - 18) & 7).tolist())
        assert cp == set(range(8)) and rp == set(range(8)), (resized, cp, rp)
    # the eight exact angles, several times each, with |m01| == |m10| on the diagonals
    lvl = facts(oracle, "compass_240x200")[1][0]
    for i, a in enumerate(oc.EXACT_ANGLES):
        hit = lvl[3] == a
        assert hit.sum() >= 3, (i, int(hit.sum()))
        if i % 2:
            assert np.all(np.abs(lvl[4][hit]) == np.abs(lvl[5][hit])) and np.all(lvl[4][hit] != 0)
        elif i % 4 == 0:
            assert np.all(lvl[4][hit] == 0) and np.all(np.sign(lvl[5][hit]) == (1 if i == 0 else -1))
        else:
            assert np.all(lvl[5][hit] == 0) and np.all(np.sign(lvl[4][hit]) == (1 if i == 2 else -1))
    # saturated: |m| >= 0.9 of the bound with both signs of both moments, every sign pair at large moments on the diagonals
    for name in ("sat_dark_bg", "sat_bright_bg"):
        lvl = facts(oracle, name)[1][0]
        m01, m10 = lvl[4], lvl[5]
        big = 0.9 * MOMENT_BOUND
        assert m10.max() >= big and m10.min() <= -big and m01.max() >= big and m01.min() <= -big, name
        assert max(m10.max(), m01.max()) == 576810 and 576810 / MOMENT_BOUND > 0.924
        pairs = {(int(np.sign(a)), int(np.sign(b))) for a, b in zip(m01, m10) if abs(a) == abs(b) and abs(a) >= 0.5 * MOMENT_BOUND}
        assert pairs == {(1, 1), (1, -1), (-1, 1), (-1, -1)}, (name, pairs)
    lvl = facts(oracle, "sat_bright_dots")[1][0]
    assert len(lvl[2]) == 40 and np.all(lvl[4] == 0) and np.all(lvl[5] == 0) and np.all(lvl[3] == 0.0)
    img = FRAMES["sat_bright_dots"]["img"]
    for x, y, _ in lvl[2]:                                               # the whole disc but its centre is 255: the largest a1 and a2
        box = img[y - 15:y + 16, x - 15:x + 16]
        assert box[15, 15] == 0 and (box == 255).sum() == 31 * 31 - 1
    # the counts around four per wave and sixteen per workgroup, on one level
    assert [facts(oracle, name)[0] for name in oc.COUNT] == list(oc.COUNTS) == [0, 1, 3, 4, 5, 15, 16, 17]
    assert np.all(FRAMES["count_0"]["img"] == 40)


def test_batches_differ_and_mix_counts(oracle):
    """Every batch: all images differ, every frame is accepted, the counts are very different with 0 among the frames the XCD deal
    covers (the first 8 * (B / 8)) and among those behind them, and next to a frame with many."""
    assert oc.BATCH_SIZES == (1, 7, 8, 9, 16, 17)
    p = oc.BATCH_PARAMS
    for size in oc.BATCH_SIZES:
        imgs = oc.batch_images(size)
        assert len(imgs) == size and len({im.tobytes() for im in imgs}) == size
        ns = []
        for im in imgs:
            assert im.shape == (oc.BATCH_H, oc.BATCH_W)
            ns.append(oracle.Extractor(p["nf"], p["sf"], p["nl"], oc.INI_TH, oc.MIN_TH)(im, (0, 0))[0])
        assert min(ns) >= 0
        if size == 1:
            assert ns[0] > 16
            continue
        dealt = size // 8 * 8
        assert max(ns) >= 40 and 0 in ns, (size, ns)                    # (a workgroup holds 16: three and more workgroups beside none)
        if dealt:
            assert 0 in ns[:dealt] and max(ns[:dealt]) >= 40, (size, ns)
        if size == 9:
            assert ns[8] > 16, ns                                        # the one frame behind the deal has keypoints,
        if size == 17:
            assert ns[16] == 0, ns                                       # or none
        assert len(set(ns)) >= min(size, 5)


# ---- the oracle against the statement, on every frame ----
@pytest.mark.parametrize("name", list(FRAMES))
def test_oracle_equals_the_statement(oracle, name):
    f = FRAMES[name]
    kps, m01, m10 = check_orientation_and_descriptors(oracle, f["img"], f["nf"], f["sf"], f["nl"], oc.INI_TH, oc.MIN_TH)
    assert kps["angle"].tobytes() == fast_atan2_np(m01.astype(np.float32), m10.astype(np.float32)).tobytes()
    n, lv, _ = facts(oracle, name)                                         # (facts asserts the oracle's per-level angles against the statement)
    assert n == len(kps) == sum(len(l[2]) for l in lv)


@pytest.mark.parametrize("size", oc.BATCH_SIZES)
def test_oracle_equals_the_statement_on_the_batches(oracle, size):
    p = oc.BATCH_PARAMS
    for im in oc.batch_images(size):
        kps, m01, m10 = check_orientation_and_descriptors(oracle, im, p["nf"], p["sf"], p["nl"], oc.INI_TH, oc.MIN_TH)
        assert kps["angle"].tobytes() == fast_atan2_np(m01.astype(np.float32), m10.astype(np.float32)).tobytes()
