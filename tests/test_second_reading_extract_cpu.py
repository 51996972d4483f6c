"""The CPU oracle's extractor (oracle/orbref_extract.cpp) against the second reading of ORBextractor.cc's cell loop, quadtree and
epilogue (tests/second_reading_extract.py), entry for entry: hand-worked answers first, then the oracle's `distribute`, level
candidates, level keypoints and final output on the hand-laid frames of tests/extract_cases.py, on seeded random candidate sets and on
whole frames.  Every case proves from the reading's counters that it reached its branch; every counter the reading names is reached;
where the reading reports no cut inside a group of equal counts, the selected set is the same under every tie order.  No GPU."""
import os
import random
import re
from collections import Counter

import numpy as np
import pytest

import extract_cases as ec
import second_reading_extract as sr
import structured_images as si

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ec.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def test_second_reading_imports_neither_oracle_nor_product():
    src = open(os.path.join(HERE, "second_reading_extract.py")).read()
    mods = set(re.findall(r"^\s*(?:from|import)\s+([\w\.]+)", src, flags=re.M))
    assert mods == {"math", "random", "collections", "numpy"}, mods
    for word in ("orbref", "orb-slam3_amd", "importlib", "ctypes", "__import__", "liborb"):
        assert word not in src, word
    helper = open(os.path.join(HERE, "extract_cases.py")).read()
    assert set(re.findall(r"^\s*(?:from|import)\s+([\w\.]+)", helper, flags=re.M)) == {"numpy"}


def _read_levels(levels, c, tie="newest"):
    return sr.extract(levels, c["nf"], c["sf"], c["ini"], c["mn"], c["lap"], tie)


@pytest.fixture(scope="module")
def runs(oracle):
    """Every hand-laid frame through the oracle and -- on the oracle's level images -- through the reading, once."""
    out = {}
    for c in CASES:
        ref = oracle.Extractor(c["nf"], c["sf"], c["nl"], c["ini"], c["mn"])
        n, kps, desc, mono = ref(c["img"], c["lap"])
        assert n >= 0, (c["name"], n)
        levels = [ref.level_image(l) for l in range(c["nl"])]
        out[c["name"]] = dict(ref=ref, n=n, kps=kps, mono=mono, levels=levels, read=_read_levels(levels, c))
    return out


# ------------------------------------------------------------------------------------------------------------------ hand-worked answers
def _level0(name):
    c = BY_NAME[name]
    assert c["nl"] == 1
    return _read_levels([c["img"]], c)                      # level 0 is the image itself (:1711)


def test_hand_worked_one_two_three_dots():
    r = _level0("one_dot_N1")                               # (20, 30) value 140 on 40: response 99, one root with one key
    assert r["level_keypoints"][0].tolist() == [[36, 46, 99]] and r["mono"] == 1
    f = sr.fields_array(r["fields"])
    assert f.tolist() == [(36.0, 46.0, 31.0, 99.0, 0, -1)]
    # two dots, N = 1: the root [0, 64) x [0, 64) is cut at 32; n1 holds (10, 10), n4 (50, 50); both are pushed to the front, n4 last
    r = _level0("two_dots_N1")
    assert r["level_keypoints"][0].tolist() == [[66, 66, 109], [26, 26, 99]] and r["mono"] == 2
    # three dots in n1, n2, n3: pushed in that order, so the list reads n3, n2, n1
    for name in ("three_dots_N2", "three_dots_N3"):
        assert _level0(name)["level_keypoints"][0].tolist() == [[28, 66, 119], [66, 28, 109], [26, 26, 99]]
    # two dots 4 px apart and N = 5: the first split puts both into one child, the list does not grow, and the walk stops with one
    # node holding both (:889): the stronger, (14, 10) at 150, comes out
    assert _level0("two_close_dots_N5")["level_keypoints"][0].tolist() == [[30, 26, 109]]


def test_hand_worked_response_tie_follows_cell_order():
    # 70 x 70: cells evaluate x in [3, 38) | [38, 67), the root is cut at 35.  vToDistributeKeys = (10, 10), (36, 30) from cell (0, 0),
    # (44, 12) from cell (0, 1), (10, 60), (60, 60); n2 holds (36, 30) and (44, 12), both 99: the first in that order stays
    r = _level0("tie_cell_order_beats_raster")
    assert r["candidates"][0].tolist() == [[10, 10, 79], [36, 30, 99], [44, 12, 99], [10, 60, 79], [60, 60, 79]]
    assert r["level_keypoints"][0].tolist() == [[76, 76, 79], [26, 76, 79], [52, 46, 99], [26, 26, 79]]
    r = _level0("tie_cell_order_is_raster")
    assert r["candidates"][0].tolist() == [[10, 10, 79], [36, 12, 99], [44, 30, 99], [10, 60, 79], [60, 60, 79]]
    assert r["level_keypoints"][0].tolist() == [[76, 76, 79], [26, 76, 79], [52, 28, 99], [26, 26, 79]]
    assert _level0("tie_broken_by_response")["level_keypoints"][0].tolist() == [[76, 76, 79], [26, 76, 79], [60, 28, 100], [26, 26, 79]]


def test_hand_worked_break_on_a_group_boundary():
    # quadrants hold 9, 4, 4, 1 keys and N = 7: 4 + 3 * 3 > 7 opens the final phase; sorted (4, n2), (4, n3), (9, n1); the walk from
    # the back splits n1 at 32 into 4 | 2 | 2 | 1 keys -> 7 nodes -> break.  List: c4, c3, c2, c1, n4, n3, n2.
    # values 101 + (7x + 13y) % 111: (27,27) 197 (31,27) 114 (35,27) 142 (27,31) 138 (31,31) 166 (35,31) 194 (27,35) 190 (31,35) 107 (35,35) 135;
    # (30,94) 201 (34,94) 118 (30,98) 142 (34,98) 170; (94,30) 150 (98,30) 178 (94,34) 202 (98,34) 119
    r = _level0("break_on_group_boundary")
    assert r["level_keypoints"][0].tolist() == [[51, 51, 94], [43, 51, 149], [51, 47, 153], [43, 43, 156], [116, 116, 109], [46, 110, 160], [110, 50, 161]]
    assert r["counters"]["break_fired"] == 1 and not r["counters"]["cut_inside_tie_group"]
    # N = 8: the walk goes on to the newer of the two 4s, n3 (bottom left: {30, 34} x {94, 98}, cut at 32 | 96 into four single keys)
    r = _level0("break_inside_tie_group")
    assert r["level_keypoints"][0].tolist()[:4] == [[50, 114, 129], [46, 114, 101], [50, 110, 77], [46, 110, 160]]
    assert r["level_keypoints"][0].tolist()[4:] == [[51, 51, 94], [43, 51, 149], [51, 47, 153], [43, 43, 156], [116, 116, 109], [110, 50, 161]]
    assert r["counters"]["cut_inside_tie_group"] == 1


def test_hand_worked_cell_loop():
    for name in ("adjacent_equal_pair_inside_a_cell", "adjacent_unequal_pair_inside_a_cell", "strong_and_weak_cells", "level_edges"):
        assert set(map(tuple, _level0(name)["candidates"][0].tolist())) == BY_NAME[name]["cands"], name
    # an equal pair in columns 37 | 38: the last evaluated column of cell 0 and the first of cell 1; both are kept, cell 0's first
    assert _level0("equal_pair_across_a_cell_border_columns")["candidates"][0].tolist() == [[37, 20, 99], [38, 20, 99], [72, 60, 99], [73, 60, 99]]
    assert _level0("equal_pair_across_a_cell_border_rows")["candidates"][0].tolist() == [[20, 37, 99], [20, 38, 99], [90, 72, 99], [90, 73, 99]]
    # constructor: 1000 features over 8 levels at 1.2 (the reference's default), 752 x 480
    assert sr.features_per_level(1000, 1.2, 8) == [217, 181, 151, 126, 105, 87, 73, 60]
    assert sr.level_sizes(752, 480, 1.2, 8)[:3] == [(752, 480), (627, 400), (522, 333)]


def test_hand_worked_epilogue(runs):
    """Level-1 keypoints whose float32 product with the scale factor is a whole number, or one ulp beside one, against lapping bounds
    on that number: which side they end on, and that they are written from the back in the order met."""
    seen = 0
    for c in CASES:
        if "pins" not in c:
            continue
        r = runs[c["name"]]["read"]
        f = sr.fields_array(r["fields"])
        n, mono = len(f), r["mono"]
        for x, inside in c["pins"]:
            at = [i for i in range(n) if f["octave"][i] == 1 and f["x"][i] == x]
            assert at, (c["name"], x)
            assert all((i >= mono) == inside for i in at), (c["name"], x, at, mono)
            seen += 1
        lap = c["lap"]
        assert mono == sum(1 for i in range(n) if not (lap[0] <= float(f["x"][i]) <= lap[1]))
        # mono part in the order met, lapping part reversed
        assert r["perm"][:mono] == sorted(r["perm"][:mono]) and r["perm"][mono:] == sorted(r["perm"][mono:], reverse=True)
        if lap == (0, 176):
            assert mono == 0
        if lap in ((0, 0), (500, 600)):
            assert mono == n
    assert seen >= 25


# ------------------------------------------------------------------------------------------------------------------ oracle == reading
def test_cases_reach_their_branches_and_equal_the_oracle(oracle, runs):
    for c in CASES:
        r = runs[c["name"]]; rd = r["read"]; ref = r["ref"]
        t = rd["counters"]
        for k in c["want"]:
            assert t[k] > 0, (c["name"], k, dict(t))
        for k in c["never"]:
            assert t[k] == 0, (c["name"], k, dict(t))
        if c["cands"] is not None:
            assert set(map(tuple, rd["candidates"][0].tolist())) == c["cands"], c["name"]
        if c["n_out"] is not None:
            assert len(rd["fields"]) == c["n_out"], c["name"]
        for l in range(c["nl"]):
            assert np.array_equal(ref.level_candidates(l), rd["candidates"][l]), (c["name"], l)
            assert np.array_equal(ref.level_keypoints(l)[0], rd["level_keypoints"][l]), (c["name"], l)
            w, h = ref.level_size(l)
            got = oracle.distribute(ref.level_candidates(l), 16, w - 16, 16, h - 16, rd["budget"][l]).tolist()
            assert got == rd["selected"][l], (c["name"], l)
        f = sr.fields_array(rd["fields"])
        assert len(f) == r["n"] and rd["mono"] == r["mono"], c["name"]
        for name in sr.KEY_FIELDS:
            assert f[name].tobytes() == r["kps"][name].tobytes(), (c["name"], name)


def test_wide_frames_with_small_budgets_return_four_nodes_per_root(runs):
    """1241 x 376 (four roots) and 2400 x 420 (six) with budgets below 4 * nIni: 16 / 24 keypoints per level, not an error."""
    for name, per_level in (("wide_1241_nl1_N4", 16), ("wide_1241_nl1_N7", 16), ("wide_2400_nl1_N11", 24), ("wide_2400_nl1_N15", 24)):
        assert runs[name]["n"] == per_level
    seen_full = 0
    for name, n_ini in (("wide_1241_nl8_nf20", 4), ("wide_2400_nl8_nf50", 6)):
        r = runs[name]
        counts = np.bincount(r["kps"]["octave"], minlength=8)
        budget = r["read"]["budget"]
        for l in range(8):
            w, h = r["ref"].level_size(l)
            ini = sr.c_round(np.float32(w - 32) / np.float32(h - 32))
            assert ini >= n_ini
            assert budget[l] < 4 * ini - 3
            # every quadrant of every root holds a candidate (counted here from the candidates alone) -> exactly 4 * nIni nodes
            k = r["read"]["candidates"][l]
            hx = np.float32(w - 32) / np.float32(ini)
            root = (k[:, 0].astype(np.float32) / hx).astype(int)
            left = k[:, 0] < np.array([int(hx * np.float32(i)) for i in range(ini + 1)])[root] + \
                np.array([-(-(int(hx * np.float32(i + 1)) - int(hx * np.float32(i))) // 2) for i in range(ini)])[root]
            top = k[:, 1] < -(-(h - 32) // 2)
            full = len(set(zip(root.tolist(), left.tolist(), top.tolist()))) == 4 * ini
            assert counts[l] == 4 * ini if full else counts[l] < 4 * ini, (name, l)
            seen_full += full
    assert seen_full >= 14


def test_no_level_width_loses_a_column_to_the_minus_6_rule():
    """ORBextractor.cc:1102 skips a cell column when iniX >= maxBorderX - 6 where the row test (:1085) says 3.  The search: 104 level
    widths up to 2400 (the first is 1118) have a last column that the 6 skips and a 3 would not, i.e. (nCols - 1) * wCell in
    [W - 6, W - 3).  None of them loses a pixel by it: the skipped cell would be at most 6 px wide, under FAST's 7, and the column
    before it already reaches the border (iniX + wCell + 6 >= maxBorderX).  structured_images.fast_cells and the reading's grid agree on
    every such width, and the cells' evaluated columns tile [3, W - 3) exactly.  So no frame is added for it: a 1118-px-wide frame
    would run the same code as the 1241-px one above."""
    widths = ec.skipped_column_widths(2400)
    assert len(widths) == 104 and widths[0] == 1118
    for w in widths[:3] + widths[-3:]:
        cells, wc, hc = sr.cell_grid(w, 99)
        assert [(x0, y0, x1 - x0, y1 - y0, i, j) for x0, y0, x1, y1, i, j in cells] == si.fast_cells(w, 99)[0]
        n_cols = (w - 32) // 35
        assert max(c[5] for c in cells) == n_cols - 2                        # the last column is skipped
        cover = sorted((c[0] + 3, c[2] - 3) for c in cells if c[4] == 0)
        assert cover[0][0] == 19 and cover[-1][1] == w - 19
        assert all(a[1] == b[0] for a, b in zip(cover, cover[1:]))


def _random_set(rnd, it):
    W = rnd.choice([70, 100, 192, 320, 333, 576, 700]); H = rnd.choice([64, 128, 131])
    n = rnd.randint(1, 300)
    if it % 3 == 0:                                                          # an 8-px lattice: counts tie
        pts = {(rnd.randrange(0, W - 3, 8) + 3, rnd.randrange(0, H - 3, 8) + 3) for _ in range(n)}
    else:
        pts = {(rnd.randint(3, W - 4), rnd.randint(3, H - 4)) for _ in range(n)}
    pts = sorted(pts, key=lambda p: (p[1] // 35, p[0] // 35, p[1], p[0]))    # cell by cell, as the cell loop emits them
    keys = np.array([(x, y, rnd.choice([30, 30, 50, rnd.randint(7, 254)])) for x, y in pts], np.int32)
    N = rnd.choice([1, 2, 3, 5, 8, 13, 21, 40, 80, 150, 400])
    return keys, W, H, N


def test_distribute_on_random_sets_and_cut_free_sets_do_not_depend_on_the_tie_order(oracle):
    rnd = random.Random(5)
    total = Counter()
    free = cut = reordered = 0
    for it in range(300):
        keys, W, H, N = _random_set(rnd, it)
        idx, t = sr.distribute_oct_tree(keys, 16, 16 + W, 16, 16 + H, N, "newest")
        assert oracle.distribute(keys, 16, 16 + W, 16, 16 + H, N).tolist() == idx, (it, W, H, N)
        total.update(t)
        if t["cut_inside_tie_group"]:
            cut += 1
            continue
        free += 1
        for tie in ("oldest", 11, 12, 13):
            other, t2 = sr.distribute_oct_tree(keys, 16, 16 + W, 16, 16 + H, N, tie)
            assert sorted(other) == sorted(idx), (it, tie)
            reordered += other != idx
    assert free >= 100 and cut >= 30 and reordered > 0, (free, cut, reordered)
    for k in ("final_phase", "second_walk", "break_mid_walk", "roots_erased", "key_outside_root_rect", "finished_by_prev_size"):
        assert total[k] > 0, k


def test_hand_laid_cut_free_sets_do_not_depend_on_the_tie_order(runs):
    """The flag pins: the `boundary` cases are cut-free by construction, the `inside` ones are not; and every hand-laid level the reading
    reports cut-free selects the same set under the other orders."""
    assert not runs["break_on_group_boundary"]["read"]["counters"]["cut_inside_tie_group"]
    assert not runs["clusters_N9"]["read"]["counters"]["cut_inside_tie_group"]
    for name in ("break_inside_tie_group", "break_after_whole_group", "break_at_first_of_group", "four_equal_quadrants"):
        assert runs[name]["read"]["counters"]["cut_inside_tie_group"] == 1, name
    checked = differs = 0
    for c in CASES:
        rd = runs[c["name"]]["read"]
        for l, img in enumerate(runs[c["name"]]["levels"]):
            h, w = img.shape
            keys = rd["candidates"][l]
            idx, t = sr.distribute_oct_tree(keys, 16, w - 16, 16, h - 16, rd["budget"][l], "newest")
            assert idx == rd["selected"][l]
            for tie in ("oldest", 1, 2, 3):
                other, _ = sr.distribute_oct_tree(keys, 16, w - 16, 16, h - 16, rd["budget"][l], tie)
                if not t["cut_inside_tie_group"]:
                    assert sorted(other) == sorted(idx), (c["name"], l, tie)
                    checked += 1
                else:
                    differs += sorted(other) != sorted(idx)
    assert checked >= 100 and differs > 0                                    # and where the cut is inside a group, the rule does decide


def test_every_counter_was_reached(runs):
    total = Counter()
    for r in runs.values():
        total.update(r["read"]["counters"])
    for k in sr.COUNTERS + ("cell_retry_min_th", "cell_found_at_min_th"):
        assert total[k] > 0, k


# ------------------------------------------------------------------------------------------------------------------ whole frames
FRAMES = [("textured", {}), ("sparse", {}), ("lowcontrast", {}), ("dots", {"pitch": 8}), ("checker", {"period": 16, "contrast": 15}), ("blocks", {"block": 3})]


@pytest.mark.parametrize("w,h", [(376, 240), (421, 307)])
@pytest.mark.parametrize("sf,nl", [(1.2, 8), (1.5, 3)])
@pytest.mark.parametrize("kind,params", FRAMES, ids=[k for k, _ in FRAMES])
def test_whole_frames(oracle, kind, params, sf, nl, w, h):
    img = si.gen(kind, w, h, 7, **params)
    nf = 400
    ref = oracle.Extractor(nf, sf, nl, 20, 7)
    assert sr.features_per_level(nf, sf, nl) == ref.tables()["nfeat"].tolist()
    rd = None
    for lap in ((0, 0), (0, 1000)):
        n, kps, desc, mono = ref(img, lap)
        assert n >= 0
        if rd is None:
            levels = [ref.level_image(l) for l in range(nl)]
            assert sr.level_sizes(w, h, sf, nl) == [ref.level_size(l) for l in range(nl)]
            rd = sr.extract(levels, nf, sf, 20, 7, lap)
            for l in range(nl):
                assert np.array_equal(ref.level_candidates(l), rd["candidates"][l]), l
                assert np.array_equal(ref.level_keypoints(l)[0], rd["level_keypoints"][l]), l
            per_level = [sr.level_keypoints(rd["candidates"][l], rd["selected"][l], l, sr.scale_factors(sf, nl)[0]) for l in range(nl)]
            fields, mono_r = rd["fields"], rd["mono"]
        else:
            _, fields, mono_r = sr.assemble(per_level, lap, sr.scale_factors(sf, nl)[0])
        f = sr.fields_array(fields)
        assert len(f) == n and mono_r == mono, lap
        for name in sr.KEY_FIELDS:
            assert f[name].tobytes() == kps[name].tobytes(), (lap, name)


# ------------------------------------------------------------------------------------------------------------------ the vectorised FAST
def test_vectorised_fast_equals_the_bruteforce_definition():
    rng = np.random.default_rng(5)                                           # the crop of tests/test_oracle_kat.py
    base = rng.integers(0, 256, (8, 9)).astype(np.float64)
    img = np.kron(base, np.ones((5, 5)))[:38, :42] + rng.normal(0, 6, (38, 42))
    crops = [np.clip(np.rint(img), 0, 255).astype(np.uint8)]
    crops.append(rng.integers(0, 2, (21, 24), dtype=np.uint8) * 255)         # saturated
    crops.append(np.full((6, 30), 9, np.uint8)); crops.append(np.full((7, 7), 9, np.uint8))
    crops[-1][3, 3] = 200
    for name in ("equal_pair_across_a_cell_border_columns", "equal_pair_across_a_cell_border_rows", "equal_pair_across_a_cell_corner",
                 "unequal_pair_across_a_cell_border", "adjacent_equal_pair_inside_a_cell", "adjacent_unequal_pair_inside_a_cell"):
        im = BY_NAME[name]["img"]
        for x0, y0, x1, y1, i, j in sr.cell_grid(im.shape[1], im.shape[0])[0]:
            if (im[y0:y1, x0:x1] != ec.BG).any():
                crops.append(im[y0:y1, x0:x1])                                   # the cell's own sub-image
    assert len(crops) > 12
    for k, crop in enumerate(crops):
        for thr in (7, 20, 254):
            want = si.fast_bruteforce(crop, thr) if min(crop.shape) >= 7 else []
            assert [list(p) for p in sr.fast(crop, thr)] == want, (k, thr)
