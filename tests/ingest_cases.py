"""Deterministic inputs for the ingest / undistortion second reading, shared by tests/test_second_reading_ingest_cpu.py and
tests/test_gpu_ingest_second_reading.py: the smallest shapes at which k_gray, k_remap, k_clahe_lut / k_clahe_apply and k_undistort can
still go wrong (one thread makes 4 pixels, one workgroup 1024: widths around 1024 and 2048 reach blockIdx.x = 1 and 2).  The reading of
a case is computed once per process (functools.lru_cache) and must not be modified by a test."""
import functools
import itertools

import numpy as np

import second_reading_ingest as R

F = np.float32

# ---- cvtColor -------------------------------------------------------------------------------------------------------------------
GRAY_SIZES = [(1, 1), (3, 2), (4, 3), (1023, 2), (1024, 2), (1025, 3), (1027, 2), (2049, 2)]
GRAY_VARIANTS = list(itertools.product((3, 4), (False, True), (14, 15)))             # channels, blue_first, coefficient bits
CUBE = np.array(list(itertools.product((0, 255), repeat=3)), np.uint8)              # the eight corners of the colour cube


def gray_images(w, h, ch, nimg=3):
    """nimg random images [h][w][ch]; the cube corners fill the END of the last row of image 0 as far as they fit (the ragged tail of
    the last column block) and the start of the first row of image 1."""
    rng = np.random.default_rng(1000 * w + 10 * h + ch)
    imgs = [rng.integers(0, 256, (h, w, ch), dtype=np.uint8) for _ in range(nimg)]
    n = min(8, w)
    imgs[0][h - 1, w - n:, :3] = CUBE[:n]
    imgs[1][0, :n, :3] = CUBE[8 - n:]
    return imgs


@functools.lru_cache(maxsize=None)
def gray_reading(w, h, ch, blue_first, bits):
    return tuple(R.gray_from_color(im, blue_first, bits) for im in gray_images(w, h, ch))


# ---- remap ----------------------------------------------------------------------------------------------------------------------
REMAP_SOURCES = [(7, 5), (300, 4)]
REMAP_CASES = [(src, dst, kind) for src in REMAP_SOURCES
               for dst, kind in (((32, 32), "lattice"), ((32, 32), "mixed"), ((5, 3), "mixed"), ((1025, 2), "mixed"), ((1031, 3), "mixed"))]
FAR_OUTSIDE = [1e4, -1e4, 32768.0, -32768.0, 2.0 ** 27, 1e9, -1e9, 3e38, np.inf, -np.inf, np.nan]


def remap_sources(sw, sh, nimg=3):
    """Pixels in [1, 255]: a tap that wrongly lands on a pixel (pixel (0, 0) for a wrapped coordinate) can never read the border value."""
    rng = np.random.default_rng(77 * sw + sh)
    return [rng.integers(1, 256, (sh, sw), dtype=np.uint8) for _ in range(nimg)]


def _special_entries(sw, sh):
    """(mapx, mapy, far) triples: one coordinate special, the other one plainly inside."""
    xs = [(2 * k + 0.5) / 32 for k in (16, 17)] + [(k + 0.5) / 32 for k in (40, 41)]            # ties of v * 32, towards even k and odd k
    xs += [-1.5, -1.03125, -0.5, -0.03125, sw - 1.0, sw - 0.5, sw - 0.03125]                    # (-2,-1), (-1,0), [sw-1, sw)
    xs += [0.0, -0.0, 1.0, float(sw - 2), -1.0, -2.0, float(sw)]                                # exact integers and -0.0
    ys = [(2 * k + 0.5) / 32 for k in (16, 17)] + [-1.5, -0.5, sh - 1.0, sh - 0.5, 0.0, -0.0, float(sh), -1.0]
    out = [(x, 1.25, False) for x in xs] + [(1.25, y, False) for y in ys]
    out += [(v, 1.25, True) for v in FAR_OUTSIDE] + [(1.25, v, True) for v in FAR_OUTSIDE]
    return out


@functools.lru_cache(maxsize=None)
def remap_maps(src, dst, kind):
    """-> (mapx, mapy, far): far [dh][dw] bool marks the entries that must read the border."""
    sw, sh = src; dw, dh = dst
    if kind == "lattice":                                              # every one of the 32 x 32 weight pairs once
        assert dst == (32, 32)
        i = np.arange(32, dtype=np.float64)
        mx = np.broadcast_to(2 + i[None, :] / 32, (32, 32)); my = np.broadcast_to(1 + i[:, None] / 32, (32, 32))
        return mx.astype(F), my.astype(F), np.zeros((32, 32), bool)
    rng = np.random.default_rng(5 * sw + 3 * dw + dh)
    mx = (rng.integers(-64, 32 * sw + 64, (dh, dw)) / 32.0).astype(F)                          # -2 .. sw + 2 in steps of 1/32
    my = (rng.integers(-64, 32 * sh + 64, (dh, dw)) / 32.0).astype(F)
    odd = rng.random((dh, dw)) < 0.25                                  # a quarter off the 1/32 lattice: rounding of v * 32 matters
    mx[odd] += F(0.011); my[odd] -= F(0.007)
    far = np.zeros((dh, dw), bool)
    sp = _special_entries(sw, sh)
    fx, fy, ff = mx.reshape(-1), my.reshape(-1), far.reshape(-1)
    n = dw * dh
    both_ends = n > 4 * len(sp) + 8
    for k, (x, y, isfar) in enumerate(sp):                             # every second entry from the first one on, so that each has
        for pos in [2 * k] + ([n - 1 - 2 * k] if both_ends else []):   # an ordinary neighbour; in a large map again from the last
            if pos < n:                                                # entry back (the last column block of the last row)
                fx[pos], fy[pos], ff[pos] = F(x), F(y), isfar
    return mx, my, far


@functools.lru_cache(maxsize=None)
def remap_reading(src, dst, kind):
    mx, my, _ = remap_maps(src, dst, kind)
    return tuple(R.remap_linear(im, mx, my) for im in remap_sources(*src))


# ---- CLAHE ----------------------------------------------------------------------------------------------------------------------
CLAHE_SIZES = [((64, 37), (8, 8)), ((37, 64), (8, 8)), ((8, 8), (8, 8)), ((16, 16), (1, 1)), ((1030, 9), (2, 3)), ((33, 65), (2, 3))]
CLAHE_REFUSED = ((2, 16), (8, 8))                                      # w = 2 under 8 tiles: the extension exceeds what reflect-101 holds
CLAHE_CLIPS = [0.0, 1e-9, 1.5, 3.0, 40.0, 1e6]
CLAHE_KINDS = ["constant", "two_valued", "ramp", "random", "random_low", "random_few"]


def clahe_image(w, h, kind):
    rng = np.random.default_rng(13 * w + h)
    if kind == "constant":
        return np.full((h, w), 200, np.uint8)
    if kind == "two_valued":
        im = np.full((h, w), 17, np.uint8); im[h // 2, w // 3] = 230
        return im
    if kind == "ramp":
        return ((np.arange(w)[None, :] * 5 + np.arange(h)[:, None] * 3) % 256).astype(np.uint8)
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "random_low":                                           # low contrast: few occupied bins, large clipped excess
        return rng.integers(100, 116, (h, w), dtype=np.uint8)
    assert kind == "random_few"
    return rng.choice(np.array([3, 90, 91, 250], np.uint8), (h, w))


@functools.lru_cache(maxsize=None)
def clahe_reading(size, tiles, clip, kind):
    return R.clahe(clahe_image(size[0], size[1], kind), clip, tiles)


def one_tile_histogram(residual, clip=10):
    """A 256-bin histogram whose clipped excess is exactly `residual` (< 256): bin 7 stands `residual` above the clip."""
    h = np.zeros(256, np.int64); h[7] = clip + residual; h[100] = 3
    return h


# ---- undistortion ---------------------------------------------------------------------------------------------------------------
EUROC_K = (458.654, 457.296, 367.215, 248.375)
NEW_K = (400.0, 410.0, 320.5, 240.25)
DIST_SETS = {
    "euroc4": (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05),
    "five": (0.3, -0.2, 1e-3, -2e-3, 0.05),
    "rational8": (0.12, -0.05, 1e-3, -5e-4, 0.01, 0.08, -0.02, 0.005),
    "prism12": (0.12, -0.05, 1e-3, -5e-4, 0.01, 0.08, -0.02, 0.005, 1e-3, -2e-4, 5e-4, 1e-4),
    "bailout": (-0.9, 0.0, 0.0, 0.0),                                 # 1 - 0.9 r^2 turns negative from r = 1.054 on
    "copy": (0.0, 0.1, 0.01, 0.0),                                    # Frame.cc:928: a first coefficient of zero copies the input
}
UNDIST_CASES = [(n, False) for n in ("euroc4", "five", "rational8", "prism12", "bailout")] + [("five", True), ("prism12", True)]
UNDIST_COUNTS = [1, 255, 256, 257, 1000]                               # k_undistort: one thread per point, 256 per workgroup
UNDIST_SEED = 2024
BOUNDS_SIZES = [(752, 480), (1241, 376), (1920, 1080)]
TILT = (0.12, -0.05, 1e-3, -5e-4, 0.01, 0.08, -0.02, 0.005, 1e-3, -2e-4, 5e-4, 1e-4, 0.02, -0.01)


def undistort_points(name):
    """1000 float32 points: -100 .. +100 px around a 752 x 480 image (out to +-2000 px for the bail-out set); point 1 is the principal
    point itself."""
    rng = np.random.default_rng(UNDIST_SEED + sorted(DIST_SETS).index(name))
    if name == "bailout":
        u = rng.uniform(-2000, 2000, 1000); v = rng.uniform(-2000, 2000, 1000)
    else:
        u = rng.uniform(-100, 852, 1000); v = rng.uniform(-100, 580, 1000)
    u = u.astype(F); v = v.astype(F)
    u[1], v[1] = F(EUROC_K[2]), F(EUROC_K[3])
    return u, v


@functools.lru_cache(maxsize=None)
def undistort_reading(name, new_k=False):
    """The reading of all 1000 points of a set (prefixes serve the smaller counts); with new_k the first 257 under NEW_K."""
    u, v = undistort_points(name)
    if new_k:
        u, v = u[:257], v[:257]
    return R.undistort_keypoints(u, v, EUROC_K, DIST_SETS[name], NEW_K if new_k else EUROC_K)


@functools.lru_cache(maxsize=None)
def bounds_reading(name, size):
    return R.image_bounds(size[0], size[1], EUROC_K, DIST_SETS[name], EUROC_K)
