"""tests/blur_cases.py on the CPU: the frames contain the strip, tile and walk classes they are listed for, the numpy statement of
the 7x7 blur gives the hand-worked answers, the taps follow from the Gaussian, and the oracle's gauss7 equals the statement on every
level of every geometry and image kind (folds on all four sides, at sizes the 9 x 13 known-answer test never had)."""
import numpy as np
import pytest

import blur_cases as bc
from blur_cases import GEOMS, gauss7_exact


def test_statement_imports_neither_oracle_nor_product():
    src = open(bc.__file__).read()
    for word in ("import orbref", "orb-slam3_amd", "import_module", "ctypes"):
        assert word not in src, word


def _classes(oracle):
    return {k: bc.level_sizes(oracle, k) for k in GEOMS}


def test_geometries_contain_the_classes(oracle):
    c = _classes(oracle)
    lv = [s for k in c for s in c[k]]
    assert all(w >= 67 and h >= 67 for w, h in lv)
    assert all(int(np.floor((w - 32) / (h - 32) + 0.5)) >= 1 for w, h in lv)                  # the quadtree's nIni: orbx_create refuses 0
    ws, hs = [w for w, _ in lv], [h for _, h in lv]
    W = lambda k, l: c[k][l][0]
    H = lambda k, l: c[k][l][1]
    # ---- columns
    assert W("tall", 0) % 128 == 0 and W("tall", 0) > 128                                     # w % 128 == 0: the last group is full
    assert 1 <= W("fold1", 0) % 128 <= 32 and W("fold1", 0) > 128                            # one live wave in the last group: level 0,
    assert 1 <= W("chunk8", 1) % 128 <= 32 and W("chunk8", 1) > 128                          # a level the resize chain made,
    assert W("wide31", 2) % 128 == 32 and W("fold32", 2) % 128 < 32                          # a whole strip and a ragged one
    assert {W("wide31", 2) % 32, W("fold1", 0) % 32, W("fold32", 1) % 32, W("fold32", 0) % 32, W("wide31", 0) % 32} == {0, 1, 2, 3, 31}
    assert {0, 1, 2, 3, 31} <= {w % 32 for w in ws}
    assert W("fold1", 0) % 16 == 1 and W("wide31", 0) % 16 == 15 and W("chunk8", 2) % 16 == 15
    assert 96 < W("chunk8", 2) < 128 and 96 < W("fold1", 1) < 128                             # a single group, all four waves live
    assert W("fold1", 2) <= 96                                                                # a dead wave in the only group
    # ---- rows
    assert [H("tall", 0) % 26, H("fold1", 0) % 26, H("fold32", 0) % 26, H("wide31", 1) % 26, H("tall16", 0) % 26] == [0, 1, 2, 3, 25]
    assert H("chunk8", 0) % 26 == 0 and H("tall16", 2) % 26 == 2
    assert {0, 1, 2, 3, 25} <= {h % 26 for h in hs}
    assert H("fold1", 1) % 8 == 0 and H("wide31", 0) % 8 == 1 and H("wide31", 1) % 8 == 1 and H("fold1", 0) % 8 == 7 and H("tall16", 0) % 8 == 7
    assert {0, 1, 7} <= {h % 8 for h in hs}
    nt = lambda k, l: bc.ntile(H(k, l))
    assert nt("chunk8", 0) == 8 and nt("fold1", 0) == 8 and nt("fold32", 0) == 9              # a full chunk; a second chunk of one tile
    assert nt("tall16", 0) == 16 and nt("tall", 0) == 17                                      # ntile % 8 in {0, 1} beyond the first chunk
    assert all(bc.ntile(h) < 8 for _, h in c["wide31"])                                       # never a full chunk
    # ---- the walk: the listed geometry has the most walk tasks per frame among the tall ones, and the threshold is within reach
    wt = {k: bc.walk_tasks(c[k]) for k in c}
    assert wt[bc.MOST_WALK_TASKS] == max(wt.values()) == 14 and 6 * max(wt.values()) < 2048  # (a geometry's own frames: the one-tile form)
    # ---- k_blur2: the four right-edge selectors, a last dword in a strip's lane 63, a level narrower than one strip, and two strips
    assert {(w - 1) & 3 for w in ws} == {0, 1, 2, 3}
    assert [s[2] for s in bc.blur2_strips(W("tall", 0))] == [True]
    assert [s[2] for s in bc.blur2_strips(752)] == [False, False, True]                      # (the workload's own case)
    assert any(len(bc.blur2_strips(w)) == 1 and ((w - 1) >> 2) < 62 for w in ws)
    assert any(len(bc.blur2_strips(w)) == 2 for w in ws)
    for k in GEOMS:
        assert GEOMS[k][4] >= len(bc.IMAGE_KINDS)


def test_impulse_frames():
    for k, (w, h, *_) in GEOMS.items():
        for inset in (0, 1):
            pts = bc.impulse_points(w, h, inset)
            assert len(set(pts)) == len(pts)
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 8 for i, a in enumerate(pts) for b in pts[:i]), k
            xs, ys = {x for x, _ in pts}, {y for _, y in pts}
            assert {x for x in (w - 1, w - 2) + bc.IMPULSE_X if x < w} <= xs, k
            assert {y for y in (h - 1, h - 2) + bc.IMPULSE_Y if y < h} <= ys, k
            corners = {(inset, inset), (w - 1 - inset, inset), (inset, h - 1 - inset), (w - 1 - inset, h - 1 - inset)}
            assert corners <= set(pts)
            img = bc.impulse_image(w, h, inset)
            assert int(img.sum()) == 255 * len(pts)
            # level 0 of the blur is the 2-D tap table around every impulse, folds included: column x of the 1-D table of an n-long
            # line holds the summed taps that reach source pixel p from output x
            out = gauss7_exact(img)
            tab = lambda p, n: np.array([sum(K for i, K in enumerate(bc.K) if _r101(o + i - 3, n) == p) for o in range(n)])
            exp = np.zeros((h, w), np.int64)
            for x, y in pts:
                exp += np.outer(tab(y, h), tab(x, w)) * 255
            assert np.array_equal(out, (exp + 32768) >> 16), k


def _r101(q, n):
    q = -q if q < 0 else q
    return 2 * n - 2 - q if q >= n else q


def test_hand_worked_answers():
    img = np.zeros((40, 37), np.uint8); img[0, 0] = 255
    out = gauss7_exact(img)
    assert out[0, 0] == (56 * 56 * 255 + 32768) >> 16 == 12
    assert out[3, 3] == (18 * 18 * 255 + 32768) >> 16 == 1
    assert out[0, 3] == (56 * 18 * 255 + 32768) >> 16 == 4 and not out[4:, :].any() and not out[:, 4:].any()
    img = np.zeros((40, 37), np.uint8); img[1, 1] = 255
    out = gauss7_exact(img)
    assert out[0, 0] == ((48 + 48) * (48 + 48) * 255 + 32768) >> 16 == 36                  # the fold: taps -1 and +1 both land on pixel 1
    assert out[1, 1] == ((56 + 34) * (56 + 34) * 255 + 32768) >> 16 == 32                  # offset -2 lands on pixel 1 too (1 - 2 = -1 -> 1)
    assert out[4, 4] == (18 * 18 * 255 + 32768) >> 16 == 1
    img = np.zeros((40, 37), np.uint8); img[39, 36] = 255                                     # the far corner folds the same way
    assert np.array_equal(gauss7_exact(img)[::-1, ::-1], gauss7_exact(img[::-1, ::-1]))
    assert gauss7_exact(img)[39, 36] == 12
    for v in (0, 1, 77, 128, 254, 255):
        assert np.all(gauss7_exact(np.full((67, 71), v, np.uint8)) == v)
    # the horizontal pass's extremes: 256 * 255 = 65280 fits 16 bits, 65280 - 32768 = 32512, 0 - 32768 = -32768
    assert sum(bc.K) == 256 and sum(bc.K) * 255 - 32768 == 32512
    # separable: rows first (Q8.8, exact), then columns, one rounding
    rng = np.random.default_rng(5)
    im = rng.integers(0, 256, (31, 29), dtype=np.uint8)
    p = np.pad(im, 3, mode="reflect").astype(np.int64)
    hsum = sum(bc.K[i] * p[:, i:i + 29] for i in range(7))
    vsum = sum(bc.K[i] * hsum[i:i + 31, :] for i in range(7))
    assert hsum.max() <= 65280 and np.array_equal(gauss7_exact(im), (vsum + 32768) >> 16)


def test_taps_follow_from_the_gaussian():
    """SURVEY A.3's wording of OpenCV >= 4.3's fixed-point kernel: exp(-x^2 / (2 sigma^2)), sigma = 2, normalised, times 256, rounded
    with the rounding error carried from the outermost tap inwards, the centre tap taking what is left of 256.  OpenCV's source is not
    available to this repository, so that this IS what OpenCV does stays on trust; what the test pins is that the
    taps in the kernels, the oracle and the statement are the ones the wording yields, and that per-tap rounding would not be."""
    g = np.exp(-np.arange(-3, 4, dtype=np.float64) ** 2 / 8.0)
    g = g / g.sum() * 256.0
    assert [round(float(v), 2) for v in g[:4]] == [17.96, 33.56, 48.82, 55.32]
    taps, err, margin = [0] * 7, 0.0, 1.0
    for i in range(3):
        t = int(np.floor(g[i] + err + 0.5))
        margin = min(margin, abs(g[i] + err - t - 0.5), abs(g[i] + err - t + 0.5))
        err += g[i] - t
        taps[i] = taps[6 - i] = t
    taps[3] = 256 - sum(taps)
    assert tuple(taps) == bc.K == (18, 34, 48, 56, 48, 34, 18)
    each = [int(np.floor(v + 0.5)) for v in g]
    assert each == [18, 34, 49, 55, 49, 34, 18] and sum(each) == 257
    # the nearest rounding boundary is 0.016 away (33.516 after diffusion): far above any error of exp and the sums in double
    assert margin > 0.015


@pytest.mark.parametrize("name", list(GEOMS))
def test_oracle_gauss7_equals_the_statement(oracle, synth, name):
    w, h, nl, sf, frames = GEOMS[name]
    sizes = bc.level_sizes(oracle, name)
    for i in range(frames):
        ref = oracle.Extractor(bc.NFEATURES, sf, nl, bc.INI_TH, bc.MIN_TH)
        ref(bc.image(synth, name, i), (0, 0))
        for l in range(nl):
            lvl = ref.level_image(l)
            assert lvl.shape == sizes[l][::-1]
            exact = gauss7_exact(lvl)
            assert oracle.gauss7(lvl).tobytes() == exact.tobytes(), (name, i, l)
            bl = ref.level_image(l, blurred=True)              # the oracle blurs only levels on which it selected a keypoint
            assert bl is None or bl.tobytes() == exact.tobytes(), (name, i, l)
    # the extremes reach the output unchanged and the impulse frame stays an impulse response on level 0
    assert np.all(gauss7_exact(bc.image(synth, name, 3)) == 255) and not gauss7_exact(bc.image(synth, name, 2)).any()
