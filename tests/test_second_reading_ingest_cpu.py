"""tests/second_reading_ingest.py held to hand-worked answers, then the oracle held to the reading bit for bit on every case of
tests/ingest_cases.py, then the reading's branch counters: every one reached.  The undistortion comparison is exact because no chosen
input is `undecidable` (a 200-bit value within 2^-44 relative of a float32 rounding boundary): that count is asserted to be zero.  No
GPU."""
import ctypes as C
import itertools
from collections import Counter

import numpy as np
import pytest

import ingest_cases as IC
import second_reading_ingest as R

F = np.float32
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the reading itself ---------------------------------------------------------------------------------------------------------
def test_residual_patterns_by_hand():
    """Bin 7 stands `residual` above the clip 10 and is cut back to 10; the excess is below 256, so no bin gets a whole share, and
    +1 goes to bins 0, step, 2 step, .. with step = max(256 // residual, 1):  3 -> step 85: 0, 85, 170;  200 -> step 1: 0..199;
    129 -> step 1 (256 // 129 = 1): 0..128;  128 -> step 2: every second bin 0..254."""
    for residual, bins in ((3, [0, 85, 170]), (200, range(200)), (129, range(129)), (128, range(0, 256, 2))):
        want = np.zeros(256, np.int64); want[7] = 10; want[100] = 3
        want[list(bins)] += 1
        taken = Counter()
        got = R.clip_and_spread(IC.one_tile_histogram(residual), 10, taken)
        assert np.array_equal(got, want), residual
        assert list(taken) == ["step>=3" if residual == 3 else "step2" if residual == 128 else "step1"]
    # an excess of 256 + 3: one whole share for every bin, then the residual 3
    h = np.zeros(256, np.int64); h[7] = 10 + 259
    got = R.clip_and_spread(h, 10)
    want = np.ones(256, np.int64); want[7] = 11; want[[0, 85, 170]] += 1
    assert np.array_equal(got, want)
    assert np.array_equal(R.clip_and_spread(h, 0), h)                    # no clipping


def test_tile_size_when_one_dimension_divides():
    """64 x 37 under 8 x 8 tiles: 37 % 8 = 5, so BOTH dimensions grow: 64 + (8 - 0) = 72 and 37 + 3 = 40; the tile is 9 x 5, not 8 x 5."""
    assert R.clahe_geometry(64, 37, (8, 8)) == (8, 3, 9, 5)
    assert R.clahe_geometry(37, 64, (8, 8)) == (3, 8, 5, 9)
    assert R.clahe_geometry(64, 40, (8, 8)) == (0, 0, 8, 5)
    assert R.clahe_geometry(33, 65, (2, 3)) == (1, 1, 17, 22)
    assert R.clip_value(3.0, 45) == 1 and R.clip_value(40.0, 45) == 7 and R.clip_value(0.0, 45) == 0 and R.clip_value(1e-9, 4096) == 1


def test_clahe_by_hand():
    """One tile holding every gray level once, unclipped: LUT[i] = round((i + 1) * 255 / 256); with a single tile every pixel blends
    that LUT with itself.  A constant image has its whole mass at or below its value: 255 everywhere."""
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    out, _ = R.clahe(img, 0.0, (1, 1))
    assert np.array_equal(out.ravel(), [int(np.rint(F(i + 1) * (F(255) / F(256)))) for i in range(256)])
    assert np.all(R.clahe(np.full((16, 16), 77, np.uint8), 0.0, (2, 2))[0] == 255)
    # tile area 1, clip 1: nothing to clip; a tile's LUT is 0 below its pixel's value and 255 from it on.  The pixel in the middle of
    # Pixel x lies half way between the centres of tiles x - 1 and x (x - 0.5: weights 1/2, 1/2; tile -1 clamps to 0).  Row (10, 20, 5):
    # pixel 0 reads its own LUT: 255; pixel 1 (20) reads tile 0 (10 <= 20: 255) and its own: 255; pixel 2 (5) reads tile 1 (20 > 5: 0)
    # and its own (255): 127.5, which rounds to the even 128
    out, taken = R.clahe(np.array([[10, 20, 5]], np.uint8), 3.0, (3, 1))
    assert out.tolist() == [[255, 255, 128]] and taken["area1"] == 1 and taken["nothing_clipped"] == 3


def test_remap_by_hand():
    """The half-pixel row of test_remap_linear_known_answers: (a + b + 1) >> 1, the last column blends with the border 0."""
    assert R.prove_rounding()
    img = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
    ys, xs = np.mgrid[0:2, 0:3].astype(F)
    assert np.array_equal(R.remap_linear(img, xs, ys)[0], img)
    half, taken = R.remap_linear(img, xs + F(0.5), ys)
    assert half.tolist() == [[15, 25, 15], [45, 55, 30]] and taken["partial"] == 4 and taken["inside"] == 2
    assert not R.remap_linear(img, xs - F(5), ys)[0].any()
    q, taken = R.remap_linear(img, xs + F(0.25), ys + F(0.5))             # (10 * 3 + 20) / 4 = 12.5, (40 * 3 + 50) / 4 = 42.5 -> 27.5 -> 28
    assert q[0, 0] == 28 and taken["value_tie"] >= 1                      # a tie of the VALUE goes up: floor(x + 1/2)
    # ties of v * 32 go to the even neighbour: 32.5 / 32 -> 32 / 32, 33.5 / 32 -> 34 / 32
    assert R.map_coordinate(F(32.5 / 32)) == 1 and R.map_coordinate(F(33.5 / 32)) * 32 == 34
    # outside every image: |s| >> 5 above 32767, the overflowed product, the non-finite entries
    for v in (32768.0, -32768.0, 2.0 ** 27, 3e38, np.inf, -np.inf, np.nan):
        assert R.map_coordinate(F(v)) is None, v
    assert R.map_coordinate(F(32767.98)) is not None and R.map_coordinate(F(-32767.0)) == -32767


def test_gray_by_hand():
    """255 * 9798 + 16384 = 2514874 -> >> 15 = 76 (red); 255 * 19235 + 16384 = 4921309 -> 150 (green); 255 * 3735 + 16384 = 968809 -> 29
    (blue); the sums give yellow 226, cyan 179, magenta 105; the 14-bit coefficients give the same eight values."""
    cube = IC.CUBE.reshape(1, 8, 3)
    for bits in (14, 15):
        assert R.gray_from_color(cube, False, bits)[0].ravel().tolist() == [0, 29, 150, 179, 76, 105, 226, 255]
        assert R.gray_from_color(cube, True, bits)[0].ravel().tolist() == [0, 76, 150, 226, 29, 105, 179, 255]
        rgba = np.concatenate([cube, np.full((1, 8, 1), 9, np.uint8)], axis=2)
        assert np.array_equal(R.gray_from_color(rgba, False, bits)[0], R.gray_from_color(cube, False, bits)[0])
    for c in IC.CUBE:
        assert abs(int(R.gray_from_color(c.reshape(1, 1, 3), False, 15)[0][0, 0]) - R.gray_ideal(*c)) <= 1


@pytest.mark.parametrize("name", ["euroc4", "rational8", "prism12"])
def test_distort_after_undistort_is_the_identity(name):
    """Iterated to convergence (60 passes) the reading's undistort inverts the forward model to 1e-12 px: a swapped p1 / p2, a
    misplaced k3 or a wrong thin-prism sign would leave a residual of the size of the term."""
    for u, v in ((0, 0), (752, 480), (751, 0), (300.25, 200.5), (367.215, 248.375), (10, 470)):
        assert R.round_trip_error(u, v, IC.EUROC_K, IC.DIST_SETS[name]) < 1e-12
    if name == "euroc4":                                                 # five passes are NOT converged at the corner: 0.010 px
        assert 0.005 < R.round_trip_error(0, 0, IC.EUROC_K, IC.DIST_SETS[name], iters=5) < 0.02
        assert R.round_trip_error(0, 0, IC.EUROC_K, IC.DIST_SETS[name], iters=20) < 1e-15


def test_tilt_is_not_part_of_the_reading():
    with pytest.raises(NotImplementedError):
        R.undistort([1.0], [2.0], IC.EUROC_K, IC.TILT, IC.EUROC_K)


# ---- the oracle held to the reading ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", IC.GRAY_SIZES)
def test_oracle_gray(oracle, size):
    w, h = size
    for ch, blue_first, bits in IC.GRAY_VARIANTS:
        for img, (want, taken) in zip(IC.gray_images(w, h, ch), IC.gray_reading(w, h, ch, blue_first, bits)):
            assert np.array_equal(oracle.gray_from_color(img, blue_first, bits), want), (ch, blue_first, bits)


@pytest.mark.parametrize("case", IC.REMAP_CASES, ids=lambda c: "%dx%d-%dx%d-%s" % (c[0] + c[1] + (c[2],)))
def test_oracle_remap(oracle, case):
    mx, my, far = IC.remap_maps(*case)
    for img, (want, taken) in zip(IC.remap_sources(*case[0]), IC.remap_reading(*case)):
        got = oracle.remap_linear(img, mx, my)
        assert not want[far].any()                                       # the far-outside entries read the border
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if case[2] == "lattice":
        assert taken["inside"] == 1024


@pytest.mark.parametrize("size,tiles", IC.CLAHE_SIZES + [IC.CLAHE_REFUSED])
def test_oracle_clahe(oracle, size, tiles):
    for clip in IC.CLAHE_CLIPS:
        for kind in IC.CLAHE_KINDS:
            want, taken = IC.clahe_reading(size, tiles, clip, kind)
            got = oracle.clahe(IC.clahe_image(size[0], size[1], kind), clip, tiles)
            assert np.array_equal(got, want), (clip, kind, np.argwhere(got != want)[:8])


def _oracle_undistort(oracle, u, v, dist, new_k):
    L = oracle.lib()
    L.orbref_undistort_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    kps = np.zeros(len(u), KP); kps["x"] = u; kps["y"] = v; kps["size"] = 31; kps["octave"] = np.arange(len(u)) % 8; kps["class_id"] = -1
    out = np.zeros(len(u), KP)
    k = np.array(IC.EUROC_K, F); nk = np.array(new_k, F); d = np.array(dist, F)
    rc = L.orbref_undistort_keypoints(_p(kps), len(u), _p(k), _p(d), len(d), _p(nk), _p(out))
    return rc, kps, out


@pytest.mark.parametrize("name,new_k", IC.UNDIST_CASES)
def test_oracle_undistort(oracle, name, new_k):
    want, undecidable, taken = IC.undistort_reading(name, new_k)
    assert int(undecidable.sum()) == 0                                   # otherwise: another UNDIST_SEED, never a tolerance
    u, v = IC.undistort_points(name)
    rc, kps, out = _oracle_undistort(oracle, u[:len(want)], v[:len(want)], IC.DIST_SETS[name], IC.NEW_K if new_k else IC.EUROC_K)
    assert rc == len(want)
    got = np.stack([out["x"], out["y"]], axis=1)
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8]
    for f in ("size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(out[f], kps[f])
    if len(want) > 1:                                                    # point 1, the principal point, goes to the new one
        nk = IC.NEW_K if new_k else IC.EUROC_K
        assert out["x"][1] == F(nk[2]) and out["y"][1] == F(nk[3])
    if name == "bailout":
        assert 300 < taken["icdist_negative"] < 1000                     # both outcomes of the bail-out well populated


def test_oracle_copies_when_the_first_coefficient_is_zero(oracle):
    u, v = IC.undistort_points("euroc4")
    dist = (0.0, 0.1, 0.01, 0.0)
    want, _, taken = R.undistort_keypoints(u[:10], v[:10], IC.EUROC_K, dist, IC.NEW_K)
    rc, kps, out = _oracle_undistort(oracle, u[:10], v[:10], dist, IC.NEW_K)
    assert rc == 10 and out.tobytes() == kps.tobytes() and np.array_equal(want[:, 0], u[:10]) and np.array_equal(want[:, 1], v[:10])
    assert taken["copy"] == 1


@pytest.mark.parametrize("size", IC.BOUNDS_SIZES)
def test_oracle_image_bounds(oracle, size):
    L = oracle.lib()
    L.orbref_image_bounds.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    k = np.array(IC.EUROC_K, F)
    for name in ("euroc4", "five", "rational8", "prism12"):
        want, undecidable, _ = IC.bounds_reading(name, size)
        assert not undecidable
        d = np.array(IC.DIST_SETS[name], F); b = np.zeros(4, F)
        assert L.orbref_image_bounds(size[0], size[1], _p(k), _p(d), len(d), _p(k), _p(b)) == 0
        assert b.tobytes() == want.tobytes(), (name, b, want)
    d = np.zeros(4, F); b = np.zeros(4, F)
    assert L.orbref_image_bounds(size[0], size[1], _p(k), _p(d), 4, _p(k), _p(b)) == 0
    assert b.tolist() == R.image_bounds(size[0], size[1], IC.EUROC_K, (0.0,) * 4, IC.EUROC_K)[0].tolist() == [0.0, size[0], 0.0, size[1]]
    if size == (752, 480):                                               # EuRoC's own size: barrel distortion, every corner moves outwards
        e = IC.bounds_reading("euroc4", size)[0]
        assert e[0] < 0 and e[2] < 0 and e[1] > size[0] and e[3] > size[1]


def test_oracle_refuses_tilt_and_oversized_remap_sources(oracle):
    u, v = IC.undistort_points("prism12")
    assert _oracle_undistort(oracle, u[:5], v[:5], IC.TILT, IC.EUROC_K)[0] == -2
    assert _oracle_undistort(oracle, u[:5], v[:5], IC.TILT[:13], IC.EUROC_K)[0] == -2
    assert _oracle_undistort(oracle, u[:5], v[:5], IC.TILT[:12] + (0.0, 0.0), IC.EUROC_K)[0] == 5
    L = oracle.lib()
    L.orbref_image_bounds.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    k = np.array(IC.EUROC_K, F); d = np.array(IC.TILT, F); b = np.zeros(4, F)
    assert L.orbref_image_bounds(752, 480, _p(k), _p(d), 14, _p(k), _p(b)) == -2
    L.orbref_remap_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    src = np.zeros((1, 32768), np.uint8); m = np.zeros((1, 1), F); o = np.zeros((1, 1), np.uint8)
    assert L.orbref_remap_linear(_p(src), 32768, 1, 32768, _p(m), _p(m), 1, 1, _p(o), 1) == -2
    assert L.orbref_remap_linear(_p(src), 32767, 1, 32768, _p(m), _p(m), 1, 1, _p(o), 1) == 0


def test_every_branch_of_the_reading_is_reached():
    """Over the shared cases (their readings are cached: after the tests above this costs nothing).  The grid the product refuses
    does not count."""
    reached = {k: Counter() for k in R.BRANCHES}
    for (w, h), (ch, blue_first, bits) in itertools.product(IC.GRAY_SIZES, IC.GRAY_VARIANTS):
        for _, taken in IC.gray_reading(w, h, ch, blue_first, bits):
            reached["gray"].update(taken)
    for case in IC.REMAP_CASES:
        for _, taken in IC.remap_reading(*case):
            reached["remap"].update(taken)
    for (size, tiles), clip, kind in itertools.product(IC.CLAHE_SIZES, IC.CLAHE_CLIPS, IC.CLAHE_KINDS):
        reached["clahe"].update(IC.clahe_reading(size, tiles, clip, kind)[1])
    for name, new_k in IC.UNDIST_CASES:
        reached["undistort"].update(IC.undistort_reading(name, new_k)[2])
    reached["undistort"].update(IC.undistort_reading("copy")[2])
    for part, names in R.BRANCHES.items():
        assert names - set(reached[part]) == set(), (part, sorted(names - set(reached[part])))
