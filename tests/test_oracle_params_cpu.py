"""The CPU oracle at non-default ORB parameters against plain numpy restatements of the published algorithms (no GPU).

The oracle and the product share one author, and the GPU tests of the other scale factors, level counts and
thresholds (tests/test_gpu_extractor_params.py) compare the product with the oracle only.  This module pins the oracle itself there:
  * the constructor's tables (ORBextractor.cc:468-571): the scale recurrence in double stored as float, sigma^2 and the inverses,
    nfeaturesPerLevel with cvRound and the remainder on the last level, umax;
  * the pyramid: level sizes cvRound(w * invScale) from the original size, each level cv::resize(INTER_LINEAR) of the previous one
    (SURVEY.md Appendix A.2), at scale factors whose tap patterns the default 1.2 never produces (1.5, 1.6, 2.0 among them);
  * the "too small" rule: the reference's FAST grid needs an inner width and height of at least one 35-px cell on every level.
"""
import numpy as np
import pytest

# (scale_factor, nlevels): the defaults, the parameter sets of tests/test_gpu_extractor_params.py and a few neighbours
PARAMS = [(1.2, 8), (1.2, 1), (1.2, 2), (1.2, 12), (1.1, 12), (1.3, 7), (1.5, 5), (1.6, 4), (2.0, 4), (1.05, 3), (1.25, 9)]
NFEATURES = [1, 5, 17, 50, 500, 1000, 1200, 2000, 4000, 5000]


def _tables(nfeatures, scale_factor, nlevels):
    """ORBextractor::ORBextractor's tables restated: float members, a double scaleFactor built from the float argument."""
    f32 = np.float32
    sfd = float(f32(scale_factor))                       # the C ABI takes a float; the reference keeps it as a double member
    sf = np.zeros(nlevels, f32); s2 = np.zeros(nlevels, f32)
    sf[0] = 1.0; s2[0] = 1.0
    for i in range(1, nlevels):
        sf[i] = f32(float(sf[i - 1]) * sfd)              # float * double, stored as float
        s2[i] = sf[i] * sf[i]                            # float * float
    inv_sf = (f32(1.0) / sf).astype(f32); inv_s2 = (f32(1.0) / s2).astype(f32)
    factor = f32(1.0 / sfd)
    n_desired = f32(nfeatures) * (f32(1) - factor) / (f32(1) - f32(factor.astype(np.float64) ** nlevels))
    nfeat = np.zeros(nlevels, np.int32)
    total = 0
    for lv in range(nlevels - 1):
        nfeat[lv] = int(np.rint(n_desired))              # cvRound: half to even
        total += int(nfeat[lv])
        n_desired = f32(n_desired * factor)
    nfeat[nlevels - 1] = max(nfeatures - total, 0)
    # umax: the rows of the 31-px patch circle (HALF_PATCH_SIZE 15)
    hp = 15
    umax = np.zeros(16, np.int32)
    vmax = int(np.floor(f32(hp) * f32(np.sqrt(f32(2))) / f32(2) + f32(1)))
    vmin = int(np.ceil(f32(hp) * f32(np.sqrt(f32(2))) / f32(2)))
    for v in range(vmax + 1):
        umax[v] = int(np.rint(np.sqrt(float(hp * hp - v * v))))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return dict(sf=sf, inv_sf=inv_sf, sig2=s2, inv_sig2=inv_s2, nfeat=nfeat, umax=umax)


def _level_sizes(w, h, inv_sf):
    return [(int(np.rint(np.float32(w) * s)), int(np.rint(np.float32(h) * s))) for s in inv_sf]


def _resize_linear(src, dw, dh):
    """cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR) for CV_8UC1, vectorised."""
    sh, sw = src.shape
    f32 = np.float32

    def taps(dn, sn, clamp_right):
        scale = 1.0 / (dn / sn)
        f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(f32)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(f32)).astype(f32)
        if clamp_right:                                  # columns: clamp the tap and drop its fraction at both edges
            lo = s < 0; f[lo] = 0; s[lo] = 0
            hi = s >= sn - 1; f[hi] = 0; s[hi] = sn - 1
        a0 = np.clip(np.rint((f32(1) - f) * f32(2048)), -32768, 32767).astype(np.int64)
        a1 = np.clip(np.rint(f * f32(2048)), -32768, 32767).astype(np.int64)
        return s, a0, a1

    sx, a0, a1 = taps(dw, sw, True)
    sy, b0, b1 = taps(dh, sh, False)                     # rows: weights kept, the source row index clamped
    s = src.astype(np.int64)
    hz = s[:, sx] * a0 + s[:, np.minimum(sx + 1, sw - 1)] * a1
    h0 = hz[np.clip(sy, 0, sh - 1)]; h1 = hz[np.clip(sy + 1, 0, sh - 1)]
    v = (((b0[:, None] * (h0 >> 4)) >> 16) + ((b1[:, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("scale_factor,nlevels", PARAMS)
def test_constructor_tables(oracle, scale_factor, nlevels):
    for nf in NFEATURES:
        got = oracle.Extractor(nf, scale_factor, nlevels).tables()
        want = _tables(nf, scale_factor, nlevels)
        for key in ("sf", "inv_sf", "sig2", "inv_sig2"):
            assert got[key].tobytes() == want[key].tobytes(), (nf, key, got[key], want[key])
        assert np.array_equal(got["nfeat"], want["nfeat"]), (nf, got["nfeat"], want["nfeat"])
        assert int(got["nfeat"].sum()) == max(nf, int(want["nfeat"][:-1].sum()))
        assert np.array_equal(got["umax"], want["umax"]), (got["umax"], want["umax"])


def test_tables_restatement_spot_values():
    """Hand-checked values, so that the restatement above cannot drift along with the oracle."""
    t = _tables(1000, 1.2, 8)
    assert np.array_equal(t["nfeat"], [217, 181, 151, 126, 105, 87, 73, 60])
    assert np.array_equal(t["umax"], [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3])
    assert t["sf"][1] == np.float32(1.2) and abs(float(t["sf"][7]) - 1.2 ** 7) < 1e-5
    t1 = _tables(1, 1.2, 8)
    assert np.array_equal(t1["nfeat"], [0] * 7 + [1])   # every level but the last rounds to 0 features
    assert np.array_equal(_tables(1000, 1.2, 1)["nfeat"], [1000])


# (w, h, scale_factor, nlevels, seed, kind)
PYRAMIDS = [
    (752, 480, 1.2, 8, 1, "textured"),
    (752, 480, 1.5, 5, 2, "textured"),                 # k_resize2 and k_resize in one pyramid on the device
    (752, 480, 1.6, 4, 3, "textured"),                 # every level on k_resize
    (1920, 1080, 2.0, 4, 4, "sparse"),                 # exact halving: a 2x2 average up to rounding
    (752, 480, 1.3, 7, 5, "textured"),
    (752, 480, 1.1, 12, 6, "textured"),
    (1920, 1080, 1.2, 12, 7, "sparse"),
    (1241, 376, 1.2, 8, 8, "sparse"),                  # KITTI: odd widths on every level
    (480, 752, 1.2, 8, 9, "textured"),                 # portrait
    (337, 337, 1.5, 5, 10, "textured"),                # the smallest size (1.5, 5) accepts
    (239, 239, 1.2, 8, 11, "textured"),                # the smallest size (1.2, 8) accepts
    (640, 480, 1.2, 2, 12, "lowcontrast"),
]


@pytest.mark.parametrize("w,h,scale_factor,nlevels,seed,kind", PYRAMIDS)
def test_pyramid_levels_equal_resize_restatement(oracle, synth, w, h, scale_factor, nlevels, seed, kind):
    img = synth.gen_image(w, h, seed, kind)
    ref = oracle.Extractor(500, scale_factor, nlevels)
    n = ref(img, (0, 0))[0]
    assert n >= 0
    sizes = _level_sizes(w, h, _tables(500, scale_factor, nlevels)["inv_sf"])
    prev = img
    for lv in range(nlevels):
        assert ref.level_size(lv) == sizes[lv], (lv, ref.level_size(lv), sizes[lv])
        want = img if lv == 0 else _resize_linear(prev, *sizes[lv])
        got = ref.level_image(lv)
        assert got.shape == want.shape and np.array_equal(got, want), (lv, np.argwhere(got != want)[:5])
        prev = want


@pytest.mark.parametrize("sw,sh,dw,dh", [(752, 480, 501, 320), (752, 480, 470, 300), (960, 540, 480, 270), (101, 77, 37, 29),
                                         (1241, 376, 1034, 313), (64, 64, 63, 63), (40, 40, 13, 11)])
def test_resize_primitive_equals_restatement(oracle, sw, sh, dw, dh):
    """orbref_resize_linear directly, on random bytes (every intermediate value range), at downscales from ~1.0 to ~3.4."""
    src = np.random.default_rng(sw * 7 + dw).integers(0, 256, (sh, sw), dtype=np.uint8)
    assert np.array_equal(oracle.resize_linear(src, dw, dh), _resize_linear(src, dw, dh))


@pytest.mark.parametrize("scale_factor,nlevels", [(1.2, 8), (1.5, 5), (1.1, 12), (2.0, 4), (1.2, 1)])
def test_too_small_boundary(oracle, scale_factor, nlevels):
    """The oracle refuses (-3) exactly when some level's inner area (the level minus the 16-px FAST border on each side) is narrower
    or shorter than one 35-px cell; the restated level sizes predict the smallest accepted width and height."""
    inv_sf = _tables(10, scale_factor, nlevels)["inv_sf"]
    ok = lambda w, h: all(sw - 32 >= 35 and sh - 32 >= 35 for sw, sh in _level_sizes(w, h, inv_sf))
    wmin = next(w for w in range(30, 4000) if ok(w, 600))
    hmin = next(h for h in range(30, 4000) if ok(800, h))
    ex = oracle.Extractor(10, scale_factor, nlevels)
    flat = lambda w, h: np.full((h, w), 128, np.uint8)
    assert ex(flat(wmin, 600))[0] == 0 and ex(flat(wmin - 1, 600))[0] == -3
    assert ex(flat(800, hmin))[0] == 0 and ex(flat(800, hmin - 1))[0] == -3
    if (scale_factor, nlevels) == (1.2, 8):
        assert wmin == hmin == 239


def test_small_budgets_keep_four_nodes_per_root(oracle, synth):
    """nfeatures 1: every level but the last wants 0 features, yet DistributeOctTree still splits the root once (4 nodes per
    root), so each of the 8 levels of a 752x480 textured frame returns 4 * nIni = 8 keypoints (64 in all, not 1)."""
    img = synth.gen_image(752, 480, 1)
    n, kps, _, mono = oracle.Extractor(1)(img, (0, 0))
    assert n == 64 and mono == 64
    assert np.array_equal(np.bincount(kps["octave"], minlength=8), [8] * 8)
