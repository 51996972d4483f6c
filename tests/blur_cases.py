"""The 7x7 blur stated in exact integers, and small frames chosen for k_blur3's strip, tile and walk geometry.

The statement is SURVEY A.3's wording of cv::GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) for CV_8UC1: the exact integer 2-D
convolution with outer(K, K), K = [18, 34, 48, 56, 48, 34, 18], over the reflect-101 extension of the image, rounded once,
(acc + 32768) >> 16.  It is numpy on int64 and shares nothing with the oracle or the product; this file imports neither (the value
noise generator and the oracle's level_size are handed in by the caller).  Every blurred-level comparison of tests/test_gpu_blur_tiles.py
and tests/ab/test_ab_blur_tiles.py is byte equality with gauss7_exact.

k_blur3 cuts a level into 32-px column strips (four to a 128-px workgroup; a wave whose strip starts past the right edge is not live)
and 26-row tiles (walked B3_CHUNK = 8 at a time in the walking form); its weight tables hold the reflect-101 folds, so what decides
which table entry, which staged piece and which output piece meets which pixel is w % 32, w % 128, w % 16, h % 26, h % 8 and the tile
count.  k_blur2 (the A/B library's VALU kernel) cuts a level into strips of 63 / 62 dwords and picks its right-edge byte selectors
from (w - 1) & 3.  GEOMS lists frames whose levels contain every such class; tests/test_blur_cases_cpu.py derives the classes from the
oracle's level_size and fails if a geometry stops containing the class it is listed for."""
import numpy as np

K = (18, 34, 48, 56, 48, 34, 18)
B3_ROWS, B3_CHUNK = 26, 8                                   # orbx_kernels.hip.h: rows of a tile, tiles of a walk task
NFEATURES, INI_TH, MIN_TH = 200, 20, 7


def gauss7_exact(img):
    """cv::GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) of a uint8 image, as SURVEY A.3 words it, in exact integers."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2 and min(img.shape) >= 4      # (np.pad "reflect" is reflect-101: gfedcb|abcdefgh|gfedcba)
    h, w = img.shape
    p = np.pad(img, 3, mode="reflect").astype(np.int64)
    k2 = np.outer(K, K).astype(np.int64)
    acc = np.zeros((h, w), np.int64)
    for dy in range(7):
        for dx in range(7):
            acc += k2[dy, dx] * p[dy:dy + h, dx:dx + w]
    out = (acc + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# name -> (w, h, nlevels, scale factor, frames); every level is >= 67 px both ways (a 35-px FAST cell inside a 16-px border).
# The comments give the level sizes and what each level is listed for (test_geometries_contain_the_classes holds them to it).
GEOMS = {
    # 129 x 183, 108 x 152, 90 x 127: w % 128 == 1 and w % 32 == 1 (two groups, the second one column wide: one live wave, and the right
    # fold reaches 3 px into the previous strip), w % 16 == 1; h % 26 == 1, ntile == 8 and h % 8 == 7 on level 0, h % 8 == 0 on level 1;
    # level 2: w <= 96 (a dead wave in the only group), h % 8 == 7
    "fold1": (129, 183, 3, 1.2, 6),
    # 415 x 97, 346 x 81, 288 x 67: w % 32 == 31 and w % 16 == 15 (level 0), w % 32 == 0 with w % 128 == 32 (level 2: one live wave in
    # the third group); h % 26 == 3 (level 1, the bottom fold reaches the previous tile), h % 8 == 1 (levels 0, 1), ntile < 8
    "wide31": (415, 97, 3, 1.2, 6),
    # 195 x 210, 162 x 175, 135 x 146: w % 32 == 3 (level 0), w % 32 == 2 (level 1), w % 128 == 7 (level 2: one live wave);
    # h % 26 == 2 (level 0), ntile == 9 (level 0: a full chunk and a chunk of one tile)
    "fold32": (195, 210, 3, 1.2, 6),
    # 256 x 442, 213 x 368, 178 x 307: h % 26 == 0 and ntile == 17 (level 0: two full chunks and a chunk of one tile), ntile == 15 and 12;
    # w % 128 == 0 with two groups; 256 px = 64 dwords, the last of them k_blur2's lane 63 of the first strip (as 752 px has in its
    # third).  The geometry with the most walk tasks per frame (6 + 4 + 4).  (A frame must be at least half as wide as high inside its
    # 16-px border -- the quadtree wants a root, round((w - 32) / (h - 32)) >= 1 -- so the tall frames are not narrow.)
    "tall": (256, 442, 3, 1.2, 6),
    # 240 x 415, 200 x 346, 167 x 288: h % 26 == 25 and ntile == 16 (level 0: two full chunks), h % 8 == 7; level 2: h % 26 == 2, h % 8 == 0
    "tall16": (240, 415, 3, 1.2, 6),
    # 160 x 208, 133 x 173, 111 x 144: ntile == 8 and h % 26 == 0 (level 0: exactly one full chunk, the last tile full), h % 8 == 0;
    # level 1: a level made by the resize chain (not the caller's buffer) with one live wave in its last group (w % 128 == 5);
    # level 2: w % 16 == 15, a single group of four live waves
    "chunk8": (160, 208, 3, 1.2, 6),
}
MOST_WALK_TASKS = "tall"


def level_sizes(oracle, name):
    """[(w, h)] of every level of a geometry, from the oracle's level_size."""
    w, h, nl, sf, _ = GEOMS[name]
    ref = oracle.Extractor(NFEATURES, sf, nl, INI_TH, MIN_TH)
    ref(np.zeros((h, w), np.uint8), (0, 0))
    return [tuple(ref.level_size(l)) for l in range(nl)]


def ntile(h):
    return (h + B3_ROWS - 1) // B3_ROWS


def walk_tasks(sizes):
    """k_blur3's walk tasks per frame: one per (128-px group, chunk of up to B3_CHUNK tiles) of every level."""
    return sum(((w + 127) // 128) * ((ntile(h) + B3_CHUNK - 1) // B3_CHUNK) for w, h in sizes)


def blur2_strips(w):
    """k_blur2's strips of a w-px level as (first dword, last stored dword, the strip's lane 63 is the level's last dword)."""
    gl, g0, out = (w - 1) >> 2, 0, []
    while g0 <= gl:
        lead = 1 if g0 > 0 else 0
        last, lane63 = g0 - lead + 62, False
        if g0 - lead + 63 == gl:
            last, lane63 = gl, True
        out.append((g0, min(last, gl), lane63))
        g0 = last + 1
    return out


IMPULSE_X = (31, 32, 127, 128)
IMPULSE_Y = (25, 26, 207, 208)


def impulse_points(w, h, inset=0):
    """Single pixels at least 8 px apart (Chebyshev), so that their 7 x 7 footprints stay apart and level 0 of the blur is the 2-D
    tap table around each of them, folds included.  inset 0: the four corners, and one pixel in each of the columns w-1, w-2, 31,
    32, 127, 128 and of the rows h-1, h-2, 25, 26, 207, 208 that the frame has (a wanted column gets the first free place down a ladder
    of rows, a wanted row along a ladder of columns).  inset 1: (1, 1) and the other three corners' diagonal neighbours -- (1, 1) is
    one pixel from (0, 0), so the two cannot share a frame under the 8-px rule -- with the ladders moved by four pixels."""
    pts = []

    def free(x, y):
        return 0 <= x < w and 0 <= y < h and all(max(abs(x - a), abs(y - b)) >= 8 for a, b in pts)

    for x, y in ((inset, inset), (w - 1 - inset, inset), (inset, h - 1 - inset), (w - 1 - inset, h - 1 - inset)):
        assert free(x, y), (x, y)
        pts.append((x, y))
    for x in (w - 1, w - 2) + IMPULSE_X:                    # (w - 1 and h - 1 away from the corners as well)
        if 0 <= x < w:
            pts.append((x, next(y for y in range(11 + 4 * inset, h, 9) if free(x, y))))
    for y in (h - 1, h - 2) + IMPULSE_Y:
        if 0 <= y < h:
            pts.append((next(x for x in range(13 + 4 * inset, w, 9) if free(x, y)), y))
    return pts


def impulse_image(w, h, inset=0):
    img = np.zeros((h, w), np.uint8)
    for x, y in impulse_points(w, h, inset):
        img[y, x] = 255
    return img


IMAGE_KINDS = ("noise", "binary", "zeros", "full", "impulse", "impulse1")
_images = {}


def image(synth, name, i):
    """Frame i of a geometry: value noise, random 0 / 255 pixels, all 0, all 255 (the accumulator extremes of the horizontal pass,
    H - 32768 = -32768 and 32512), the two impulse frames (level 0 of their blur is the 2-D tap table itself, folds included); further
    frames are value noise and random 0 / 255 pixels with other seeds."""
    w, h = GEOMS[name][:2]
    if (name, i) not in _images:
        seed = 900 + 137 * sorted(GEOMS).index(name) + i
        kind = IMAGE_KINDS[i] if i < len(IMAGE_KINDS) else ("noise", "binary")[i % 2]
        if kind == "noise":
            img = synth.gen_image(w, h, seed)
        elif kind == "binary":
            import structured_images
            img = structured_images.gen("binary", w, h, seed)
        elif kind in ("impulse", "impulse1"):
            img = impulse_image(w, h, int(kind == "impulse1"))
        else:
            img = np.full((h, w), 255 if kind == "full" else 0, np.uint8)
        img.setflags(write=False)
        _images[(name, i)] = img
    return _images[(name, i)]
