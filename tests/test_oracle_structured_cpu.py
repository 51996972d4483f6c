"""The CPU oracle on saturated, periodic and tie-heavy images (tests/structured_images.py), held by statements that share no code with it:
an independent numpy statement of the orientation and descriptor stage (IC_Angle, ORBextractor.cc:91-138 with umax as :542-570;
computeOrbDescriptor, :150-202), the brute-force FAST definition on saturated crops, hand-derivable answers, and conditions on the
generators themselves (what each kind is there to provoke), so that a later edit cannot quietly turn them into ordinary images."""
import numpy as np
import pytest

import structured_images as si

HALF_PATCH = 15
GAUSS7 = np.array([18, 34, 48, 56, 48, 34, 18], np.int64)

STRUCTURED, _id = si.STRUCTURED, si.case_id


# ---- the numpy statement of E6 (orientation) and E8 (steered BRIEF) ----
def umax_table():
    """ORBextractor.cc:542-570: the half-width of every row of the 31-px disc."""
    hp = np.float32(HALF_PATCH)
    vmax = int(np.floor(hp * np.sqrt(np.float32(2)) / np.float32(2) + np.float32(1)))
    vmin = int(np.ceil(hp * np.sqrt(np.float32(2)) / np.float32(2)))
    um = [0] * (HALF_PATCH + 1)
    for v in range(vmax + 1):
        um[v] = int(np.rint(np.sqrt(float(HALF_PATCH * HALF_PATCH - v * v))))
    v0 = 0
    for v in range(HALF_PATCH, vmin - 1, -1):
        while um[v0] == um[v0 + 1]:
            v0 += 1
        um[v] = v0
        v0 += 1
    return um


def moments(img, xs, ys):
    """m01, m10 of the umax disc about every (x, y): plain integer sums of v * I and u * I (the reference pairs the rows v and -v;
    integer addition does not care)."""
    um = umax_table()
    uu, vv = [], []
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        for u in range(-um[abs(v)], um[abs(v)] + 1):
            uu.append(u); vv.append(v)
    uu = np.array(uu, np.int64); vv = np.array(vv, np.int64)
    patch = img.astype(np.int64)[np.asarray(ys, np.int64)[:, None] + vv[None, :], np.asarray(xs, np.int64)[:, None] + uu[None, :]]
    return (patch * vv).sum(1), (patch * uu).sum(1)


def angles(oracle, m01, m10):
    f = oracle.lib().orbref_fast_atan2                               # cv::fastAtan2 restated; its exact cases: test_fast_atan2_exact_cases
    return np.array([f(float(np.float32(a)), float(np.float32(b))) for a, b in zip(m01, m10)], np.float32)


def descriptors(blurred, xs, ys, angle, pattern):
    """computeOrbDescriptor: every float32 product and sum rounded on its own, cos/sin through double, cvRound = round half even."""
    factor_pi = np.float32(np.pi / np.float64(np.float32(180.0)))
    rad = (np.asarray(angle, np.float32) * factor_pi).astype(np.float32)
    a = np.cos(rad.astype(np.float64)).astype(np.float32)[:, None]
    b = np.sin(rad.astype(np.float64)).astype(np.float32)[:, None]
    pat = pattern.astype(np.float32).reshape(512, 2)
    px = pat[None, :, 0]; py = pat[None, :, 1]
    row = np.rint(((px * b).astype(np.float32) + (py * a).astype(np.float32)).astype(np.float32)).astype(np.int64)
    col = np.rint(((px * a).astype(np.float32) - (py * b).astype(np.float32)).astype(np.float32)).astype(np.int64)
    t = blurred[np.asarray(ys, np.int64)[:, None] + row, np.asarray(xs, np.int64)[:, None] + col].astype(np.int64)
    bits = t[:, 0::2] < t[:, 1::2]                                   # pair i: point 2i against point 2i + 1
    return np.packbits(bits, axis=1, bitorder="little")               # bit i of byte k = pair 8k + i


def check_orientation_and_descriptors(oracle, img, nf=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
    """Run the oracle on img (lapping (0, 0): the output is the levels in order) and restate every keypoint's angle, descriptor and
    the other five fields from the oracle's own level images and selected points.  Returns (keypoints, m01, m10) of the whole frame."""
    ref = oracle.Extractor(nf, scale_factor, nlevels, ini_th, min_th)
    n, kps, desc, mono = ref(img, (0, 0))
    assert n >= 0 and mono == n
    sf = ref.tables()["sf"]
    pattern = oracle.pattern()
    at = 0
    all01, all10 = [], []
    for l in range(nlevels):
        xyr, ang = ref.level_keypoints(l)
        k = len(xyr)
        if k == 0:
            continue
        xs, ys = xyr[:, 0], xyr[:, 1]
        m01, m10 = moments(ref.level_image(l), xs, ys)
        want_angle = angles(oracle, m01, m10)
        out = kps[at:at + k]
        assert want_angle.tobytes() == ang.tobytes() and out["angle"].tobytes() == want_angle.tobytes(), "angle, level %d" % l
        want_desc = descriptors(ref.level_image(l, blurred=True), xs, ys, want_angle, pattern)
        assert np.array_equal(desc[at:at + k], want_desc), "descriptor, level %d" % l
        scale = sf[l] if l else np.float32(1)
        assert np.array_equal(out["x"], xs.astype(np.float32) * scale) and np.array_equal(out["y"], ys.astype(np.float32) * scale)
        assert np.all(out["octave"] == l) and np.all(out["class_id"] == -1) and np.array_equal(out["response"], xyr[:, 2].astype(np.float32))
        assert np.all(out["size"] == np.float32(int(np.float32(31) * sf[l])))
        all01.append(m01); all10.append(m10)
        at += k
    assert at == n
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return kps, cat(all01), cat(all10)


CASES = [("textured", {}), ("sparse", {})] + STRUCTURED


@pytest.mark.parametrize("size", [(752, 480), (501, 397)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pyramid", [(1.2, 8), (1.5, 5)], ids=lambda p: "sf%.1f-L%d" % p)
@pytest.mark.parametrize("kind,params", CASES, ids=_id)
def test_orientation_and_descriptor_numpy_statement(oracle, kind, params, pyramid, size):
    img = si.gen(kind, size[0], size[1], 7, **params)
    check_orientation_and_descriptors(oracle, img, 1000, pyramid[0], pyramid[1])


def test_umax_table(oracle):
    assert umax_table() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert umax_table() == oracle.Extractor(100).tables()["umax"].tolist()


def test_fast_atan2_exact_cases(oracle):
    """cv::fastAtan2 where no polynomial error is involved: the origin, the axes, and |y| == |x| (c == 1 exactly; the `ax >= ay`
    branch takes the tie), whose value is the float32 sum of the four coefficients."""
    f = oracle.lib().orbref_fast_atan2
    assert f(0.0, 0.0) == 0.0
    for y, x, want in [(0, 5, 0.0), (5, 0, 90.0), (0, -5, 180.0), (-5, 0, 270.0), (0, 1e6, 0.0), (3e5, 0, 90.0)]:
        assert f(float(y), float(x)) == want, (y, x)
    s = np.float32(180.0 / np.pi)
    p1, p3, p5, p7 = (np.float32(c) * s for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
    a45 = np.float32(np.float32(np.float32(p7 + p5) + p3) + p1)
    assert abs(float(a45) - 45.0) < 0.02
    for m in (1.0, 7.0, 255.0, 120000.0):
        assert f(m, m) == a45 and f(m, -m) == np.float32(180) - a45
        assert f(-m, -m) == np.float32(360) - (np.float32(180) - a45) and f(-m, m) == np.float32(360) - a45


# ---- FAST on saturated input ----
@pytest.mark.parametrize("kind,params", [("binary", {}), ("blocks", {"block": 4}), ("blocks", {"block": 2}), ("clipped", {"gain": 4.0}),
                                         ("checker", {"period": 16, "contrast": 255}), ("checker", {"period": 5, "contrast": 255}),
                                         ("checker", {"period": 16, "contrast": 15})], ids=_id)
def test_fast_bruteforce_on_saturated_crops(oracle, kind, params):
    img = np.ascontiguousarray(si.gen(kind, 200, 160, 11, **params)[40:90, 70:130])      # 60 x 50
    found = 0
    for thr in (7, 20, 254):
        exp = si.fast_bruteforce(img, thr)
        assert oracle.fast(img, thr).tolist() == exp, thr
        for x, y, s in exp[:20]:
            assert oracle.fast_score(img, x, y) == s
        found += len(exp)
    if kind in ("binary", "clipped"):
        assert found > 0


# ---- hand-derivable answers ----
def test_two_by_two_block_has_no_strict_maximum(oracle):
    img = np.zeros((120, 140), np.uint8); img[60:62, 70:72] = 255
    for y in (60, 61):
        for x in (70, 71):
            assert oracle.fast_score(img, x, y) == 254                # the other three pixels lie inside the ring: all 16 are darker by 255
    assert len(oracle.fast(img, 20)) == 0 and len(oracle.fast(img, 7)) == 0
    n, kps, desc, mono = oracle.Extractor(100, 1.2, 1, 20, 7)(img)
    assert n == 0
    img[61, 71] = 254                                                 # three equal scores and a smaller one next to them: still none
    assert len(oracle.fast(img, 20)) == 0
    img[60:62, 70:72] = 0; img[60, 70] = 255                          # one pixel alone is a strict maximum
    assert oracle.fast(img, 20).tolist() == [[70, 60, 254]]


def test_single_dot_angle_and_descriptor(oracle):
    img = np.zeros((300, 300), np.uint8); img[150, 150] = 255
    kps, m01, m10 = check_orientation_and_descriptors(oracle, img, 100)
    ref = oracle.Extractor(100)
    n, kps, desc, mono = ref(img, (0, 0))
    assert n >= 1 and kps[0]["x"] == 150.0 and kps[0]["y"] == 150.0 and kps[0]["octave"] == 0
    assert kps[0]["angle"] == 0.0 and kps[0]["response"] == 254.0 and kps[0]["size"] == 31.0
    assert m01[0] == 0 and m10[0] == 0
    # angle 0: the pattern is read unrotated from the blurred dot, which is the 7 x 7 impulse response and 0 elsewhere
    g = np.zeros((41, 41), np.int64)
    g[17:24, 17:24] = (np.outer(GAUSS7, GAUSS7) * 255 + 32768) >> 16
    p = oracle.pattern().astype(np.int64).reshape(256, 4)
    bits = g[20 + p[:, 1], 20 + p[:, 0]] < g[20 + p[:, 3], 20 + p[:, 2]]
    assert np.array_equal(desc[0], np.packbits(bits, bitorder="little"))
    assert 0 < int(bits.sum()) < 256


@pytest.mark.parametrize("value", [0, 255])
def test_saturated_constant_frames_have_no_keypoint(oracle, value):
    n, kps, desc, mono = oracle.Extractor(1000)(np.full((480, 752), value, np.uint8), (0, 1000))
    assert n == 0 and mono == 0


def test_too_small_structured_frame_is_rejected(oracle):
    assert oracle.Extractor(1000)(si.gen("binary", 120, 100, 1))[0] < 0


# ---- the generators provoke what they are for (752 x 480, default parameters) ----
W, H = 752, 480


def _run(oracle, kind, **params):
    img = si.gen(kind, W, H, 7, **params)
    ref = oracle.Extractor(1000)
    n, kps, desc, mono = ref(img, (0, 0))
    return img, ref, n, kps


def _angle0_moments(oracle, ref, kps):
    """Recomputed (m01, m10) of the final keypoints whose angle is exactly 0.0."""
    m01s, m10s = [], []
    for l in range(8):
        xyr, ang = ref.level_keypoints(l)
        z = ang == 0.0
        if z.any():
            a, b = moments(ref.level_image(l), xyr[z, 0], xyr[z, 1])
            m01s.append(a); m10s.append(b)
    assert int((kps["angle"] == 0.0).sum()) == sum(len(a) for a in m01s)
    return np.concatenate(m01s), np.concatenate(m10s)


def test_generators_are_deterministic_and_uint8():
    for kind, params in STRUCTURED:
        a = si.gen(kind, 333, 222, 5, **params); b = si.gen(kind, 333, 222, 5, **params)
        assert a.dtype == np.uint8 and a.shape == (222, 333) and np.array_equal(a, b), kind
    assert not np.array_equal(si.gen("binary", 64, 64, 1), si.gen("binary", 64, 64, 2))


def test_binary_saturates_and_floods_the_quick_test(oracle):
    img, ref, n, kps = _run(oracle, "binary")
    assert np.isin(img, (0, 255)).mean() >= 0.99
    assert si.quick_test_fraction(img, 20) >= 0.50                    # theory 9/16
    assert n >= 300
    assert len(ref.level_candidates(1)) >= 3 * 4000                   # the noise images give ~4 000


def test_blocks_have_plateaus_on_level_0(oracle):
    img, ref, n, kps = _run(oracle, "blocks", block=4)
    assert 10 * len(ref.level_candidates(0)) < len(ref.level_candidates(1))
    assert n >= 300


@pytest.mark.parametrize("kind", ["dots", "ramp_dots"])
def test_dot_lattices_give_exact_zero_angles(oracle, kind):
    img, ref, n, kps = _run(oracle, kind, pitch=8)
    assert n >= 300 and int((kps["angle"] == 0.0).sum()) >= 100
    m01, m10 = _angle0_moments(oracle, ref, kps)
    # Angle 0.0 has two sources, and each kind is there for one of them: on an unbroken lattice the disc about a dot is symmetric, both
    # moments vanish and fastAtan2(0, 0) = 0; under the ramp m10 > 0 everywhere, so only m01 == 0 < m10 can occur.  Each is asked of
    # the kind that can give it.
    if kind == "dots":
        assert np.any((m01 == 0) & (m10 == 0))                        # a dot of an unbroken lattice, by symmetry
        c = ref.level_candidates(0)
        assert np.bincount(c[:, 2]).max() >= 1000                     # one response shared by the whole lattice
    else:
        assert np.any((m01 == 0) & (m10 > 0))                         # the ramp tips the centroid along +x only


def test_holes_pitch_does_not_divide_the_cell(oracle):
    img, ref, n, kps = _run(oracle, "holes", pitch=10)
    assert n >= 300
    w_cell = int(np.ceil((W - 32) / ((W - 32) // 35))); h_cell = int(np.ceil((H - 32) / ((H - 32) // 35)))
    assert w_cell % 10 and h_cell % 10
    assert np.bincount(ref.level_candidates(0)[:, 2]).max() >= 1000


def test_clipped_is_mostly_saturated(oracle):
    img, ref, n, kps = _run(oracle, "clipped", gain=4.0)
    assert np.isin(img, (0, 255)).mean() >= 0.50 and n >= 300


def test_checker_low_contrast_goes_through_the_retry(oracle):
    img, ref, n, kps = _run(oracle, "checker", period=16, contrast=15)
    assert 7 < int(img.max()) - int(img.min()) <= 20
    resp = np.concatenate([ref.level_candidates(l)[:, 2] for l in range(8)])
    assert len(np.unique(resp)) <= 4
    crop = np.ascontiguousarray(img[16:16 + 70, 16:16 + 90])
    assert si.fast_bruteforce(crop, 20) == []
    assert si.quick_test_fraction(img, 20) == 0.0                     # the 4-point test is necessary for a corner: none anywhere at iniTh,
    assert len(resp) > 300 and resp.max() < 20                        # so every candidate of every level came from the minTh pass
    assert n >= 300
    img, ref, n, kps = _run(oracle, "checker", period=16, contrast=255)
    assert n >= 300


def test_every_kind_gives_enough_keypoints(oracle):
    for kind, params in STRUCTURED:
        n = oracle.Extractor(1000)(si.gen(kind, W, H, 7, **params), (0, 0))[0]
        if kind == "halves" and "constant" in params.values():
            assert n > 0
        else:
            assert n >= 300, (kind, params, n)


def test_halves_share_overflowing_and_empty_cells(oracle):
    img, ref, n, kps = _run(oracle, "halves", left="binary", right="constant")
    c = ref.level_candidates(0)
    assert len(c) > 1000 and c[:, 0].max() + 16 <= W // 2 + 3 and n > 0
    assert np.all(img[:, W // 2:] == 128)


def test_border_structure_stays_in_the_edge_band(oracle):
    for base in (0, 255):
        img = si.gen("border", W, H, 7, base=base)
        assert np.all(img[23:-23, 23:-23] == base) and np.all(img[:19] == base) and np.all(img[:, :19] == base)
        assert np.all(img[-19:] == base) and np.all(img[:, -19:] == base)
        ring = img[19:23, 19:-19]
        assert 0.3 < (ring == 255).mean() < 0.7
        ref = oracle.Extractor(1000)
        n, kps, desc, mono = ref(img, (0, 0))
        c = ref.level_keypoints(0)[0]
        d = np.minimum(np.minimum(c[:, 0], W - 1 - c[:, 0]), np.minimum(c[:, 1], H - 1 - c[:, 1]))
        assert len(c) > 0 and d.min() == 19 and d.max() <= 25       # keypoints on the first row FAST may return, none in the interior


# ---- which FAST route the cells take under the product's queue capacity (structured_images.fast_queue_caps) ----
def test_queue_capacity_restatement():
    ref_sizes = [(752, 480), (627, 400), (522, 333), (435, 278), (363, 231), (302, 193), (252, 161), (210, 134)]
    caps = si.fast_queue_caps(ref_sizes)
    # 36 x 38-px cells, four to a strip of pitch 176: 7 workgroups per CU leave (160 KB / 7 - 2 * 176 * 44) / 8 = 989 -> 960 entries
    assert caps[0] == 960 and caps[1] == 960
    assert caps[7] >= 1368                                            # the coarse levels keep their worst case: never an overflow there
    for w, h in [(421, 307), (1241, 376), (1920, 1080)]:
        lv = [(int(np.rint(np.float32(w) / np.float32(1.2) ** l)), int(np.rint(np.float32(h) / np.float32(1.2) ** l))) for l in range(4)]
        assert all(512 <= c <= 1088 for c in si.fast_queue_caps(lv + ref_sizes[4:])[:1])


def test_overflow_and_retry_routes_are_walked(oracle):
    """binary: 9/16 of a 36 x 38 cell is ~770 survivors -- under level 0's 960 entries, over them on levels 1-3.  The dense checker
    (period 3, 5 % of the pixels inverted): nearly every pixel passes, so the full-size cells of level 0 overflow as well, and hold corners."""
    img, ref, n, kps = _run(oracle, "binary")
    r = si.cell_routes(ref)
    assert r[0][1] == 0 and r[1][1] * 2 >= r[1][0] and sum(x[1] for x in r[1:4]) >= 200 and sum(x[1] for x in r[4:]) == 0
    img, ref, n, kps = _run(oracle, *si.DENSE[:1], **si.DENSE[1])
    r = si.cell_routes(ref)
    assert np.isin(img, (0, 255)).all() and si.quick_test_fraction(img, 20) >= 0.80
    assert r[0][1] * 10 >= r[0][0] * 9 and r[1][1] * 10 >= r[1][0] * 9           # >= 90 % of the cells of levels 0 and 1 (the rest: ragged last cells)
    assert len(ref.level_candidates(0)) >= 2000 and n >= 900
    for w, h in [(421, 307), (1241, 376), (1920, 1080)]:                          # the sizes the GPU suite runs it at
        ref = oracle.Extractor(1000)
        ref(si.gen(si.DENSE[0], w, h, 13, **si.DENSE[1]), (0, 0))
        r = si.cell_routes(ref)
        assert r[0][1] * 10 >= r[0][0] * 8, (w, h, r[0])
    img, ref, n, kps = _run(oracle, "checker", period=16, contrast=15)
    r = si.cell_routes(ref)
    assert all(x[2] == x[0] and x[1] == 0 for x in r)                             # every cell retried, none overflows
    img, ref, n, kps = _run(oracle, "halves", left="binary", right="constant")
    r = si.cell_routes(ref)
    assert r[1][1] >= 40 and r[1][2] >= 40                                        # overflowing and retried (empty) cells on one level


# ---- the stereo pairs provoke what they are for ----
def _row_band_ties(kl, dl, kr, dr, sf):
    """Left keypoints whose best Hamming distance over the right keypoints of their row band (|vR - vL| <= 2 * sf[octave of R], the
    rows a right keypoint is filed under, Frame.cc:1127-1141; levels within one of each other, :1170) is taken by two or more."""
    ties = with_cand = 0
    bits = np.unpackbits(dl[:, None, :] ^ dr[None, :, :], axis=2).sum(2)
    for i in range(len(kl)):
        band = (np.abs(kr["y"] - kl["y"][i]) <= 2.0 * sf[kr["octave"]]) & (np.abs(kr["octave"] - kl["octave"][i]) <= 1) & (kr["x"] <= kl["x"][i])
        if band.any():
            d = bits[i][band]
            with_cand += 1
            ties += int((d == d.min()).sum() >= 2)
    return ties, with_cand


@pytest.mark.parametrize("kind,d,params", si.PAIRS, ids=["dots", "binary"])
def test_stereo_pairs_provoke_ties_and_rejections(oracle, pkg, kind, d, params):
    l, r = si.shifted_pair(kind, 752, 480, 51, d, **params)
    assert np.array_equal(l[:, d:], r[:, :752 - d])
    ol, orr = oracle.Extractor(1200), oracle.Extractor(1200)
    nl, kl, dl, _ = ol(l, (0, 0)); nr, kr, dr, _ = orr(r, (0, 0))
    ties, with_cand = _row_band_ties(kl, dl, kr, dr, ol.tables()["sf"])
    n, ur, dp = oracle._oracle_matcher_class()().ComputeStereoMatches(ol, orr, kl, dl, kr, dr, si.MB, si.MBF)
    assert n > 100 and with_cand >= 1000
    assert n * 2 < with_cand                                           # most left keypoints with a candidate end without a match (dots 451, binary 190 of ~1100; a value-noise pair keeps 760 of 1129)
    if kind == "dots":
        assert ties >= 100                                             # a lattice repeats along the row: equal best distances (measured 267; a value-noise pair: 17)
        disp = kl["x"][ur >= 0] - ur[ur >= 0]
        assert np.sum(np.abs(disp - d) > 1.0) >= 50                    # and many matches settle on another period of the lattice
