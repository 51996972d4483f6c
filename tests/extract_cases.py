"""Hand-laid frames for the extractor's cell loop, quadtree and epilogue (tests/second_reading_extract.py is the reading they are
held to).  Pure numpy; imports neither the oracle nor the product.

paint(w, h, dots, bg) puts single pixels on a flat background.  An isolated pixel with value - bg > iniTh is a FAST corner with
response value - bg - 1 (all 16 ring pixels are darker by value - bg; no pixel near it sees more than one bright ring pixel), so the
candidates of level 0 and their responses -- ties included -- are known by construction.  Dots are given in the quadtree's
coordinates (relative to the 16-px border: image pixel (x + 16, y + 16)) and stay at least 4 px apart unless a case says otherwise.

With nlevels = 1 the budget N of level 0 is nfeatures itself (ORBextractor.cc:526).  A level must be at least 35 px wide and high
inside its border (tests/test_oracle_params_cpu.py::test_too_small_boundary), so the smallest frame is 67 x 67.

Every case is a dict: name, img, nf, nl, sf, ini, mn (the extractor's parameters), lap, want (counters of the reading that must be
non-zero on this frame: the proof that it reached its branch), never (counters that must stay zero), cands (level-0 candidates known
by construction, as a set of (x, y, response), or None), n_out (number of keypoints known by construction, or None).
"""
import numpy as np

BG = 40


def paint(w, h, dots, bg=BG):
    """uint8 (h, w): `bg` everywhere, dots = [(x, y, value)] in the quadtree's coordinates."""
    img = np.full((h, w), bg, np.uint8)
    for x, y, v in dots:
        assert 0 <= x + 16 < w and 0 <= y + 16 < h and 0 <= v <= 255
        img[y + 16, x + 16] = v
    return img


def case(name, W, H, dots, nf, want=(), never=(), nl=1, sf=1.2, ini=20, mn=7, lap=(0, 0), bg=BG, cands="all", n_out=None):
    """A frame whose inner area (inside the 16-px border) is W x H."""
    if cands == "all":                                                           # every dot is a candidate with response value - bg - 1
        cands = {(x, y, abs(v - bg) - 1) for x, y, v in dots}
    return dict(name=name, img=paint(W + 32, H + 32, dots, bg), nf=nf, nl=nl, sf=sf, ini=ini, mn=mn, lap=lap, want=tuple(want),
                never=tuple(never), cands=cands, n_out=n_out)


def lattice(x0, y0, x1, y1, pitch, value=lambda x, y: 140):
    return [(x, y, value(x, y)) for y in range(y0, y1, pitch) for x in range(x0, x1, pitch)]


def _varied(x, y):
    """Distinct-looking responses without a random generator: 101 .. 211."""
    return 101 + (x * 7 + y * 13) % 111


def cluster(cx, cy, n=3, pitch=4, value=_varied):
    """n x n dots `pitch` px apart with their corner at (cx, cy)."""
    return lattice(cx, cy, cx + n * pitch, cy + n * pitch, pitch, value)


def quadtree_cases():
    out = []
    # ---- one, two, three dots; budgets above and below the count
    out.append(case("one_dot_N1", 64, 64, [(20, 30, 140)], 1, want=["roots_single", "finished_in_full_pass"], n_out=1))
    out.append(case("one_dot_N5", 64, 64, [(20, 30, 140)], 5, want=["roots_single", "finished_by_prev_size"], n_out=1))
    out.append(case("two_dots_N1", 64, 64, [(10, 10, 140), (50, 50, 150)], 1, want=["stop_in_first_pass_above_N"], n_out=2))
    out.append(case("two_dots_N5", 64, 64, [(10, 10, 140), (50, 50, 150)], 5, want=["finished_by_prev_size"], n_out=2))
    out.append(case("two_close_dots_N5", 64, 64, [(10, 10, 140), (14, 10, 150)], 5, want=["zero_gain_split", "finished_by_prev_size"], n_out=1))
    out.append(case("three_dots_N2", 64, 64, [(10, 10, 140), (50, 12, 150), (12, 50, 160)], 2, want=["finished_in_full_pass"], n_out=3))
    out.append(case("three_dots_N3", 64, 64, [(10, 10, 140), (50, 12, 150), (12, 50, 160)], 3, want=["finished_in_full_pass"], n_out=3))
    # ---- a full lattice, N = 1..4: the first pass ends with 4 * nIni nodes, more than N
    for n in (1, 2, 3):
        out.append(case("lattice_N%d" % n, 64, 64, lattice(4, 4, 60, 60, 8, _varied), n, want=["stop_in_first_pass_above_N"], n_out=4))
    out.append(case("lattice_N4", 64, 64, lattice(4, 4, 60, 60, 8, _varied), 4, want=["finished_in_full_pass"], never=["stop_in_first_pass_above_N"], n_out=4))
    out.append(case("lattice_N5", 64, 64, lattice(4, 4, 60, 60, 8, _varied), 5, want=["final_phase", "break_fired"]))
    # ---- nIni = 1..6: ratio 1, 1.5 (round half away from zero -> 2), 2.5 (-> 3, hX = 106.67), 3.5 (-> 4), 4.5 (-> 5, hX = 115.2), 5.5 (-> 6, hX = 117.33)
    for n_ini, W in ((1, 128), (2, 192), (3, 320), (4, 448), (5, 576), (6, 704)):
        hx = np.float32(W) / np.float32(n_ini)
        dots = lattice(6, 6, W - 4, 124, 16, _varied)
        for i in range(1, n_ini):                                                # dots on the root boundary int(hX * i) and beside it
            c = int(hx * np.float32(i))
            for k, x in enumerate((c - 1, c, c + 1)):
                y = 14 + 32 * k + 4 * (i % 2)
                dots = [d for d in dots if max(abs(d[0] - x), abs(d[1] - y)) >= 4]
                dots.append((x, y, 150 + 10 * k + i))
        want = ["final_phase"] + (["key_outside_root_rect"] if n_ini in (3, 5, 6) else [])
        out.append(case("roots_%d" % n_ini, W, 128, dots, 12 * n_ini, want=want))
        out.append(case("roots_%d_small_budget" % n_ini, W, 128, dots, 2, want=["stop_in_first_pass_above_N"], n_out=4 * n_ini))
    # ---- an empty root and a root with one dot (nIni = 3): everything else in root 0
    out.append(case("empty_and_single_root", 320, 128, lattice(6, 6, 100, 124, 12, _varied) + [(300, 60, 200)], 20,
                    want=["roots_erased", "roots_single", "final_phase"]))
    out.append(case("only_the_last_root", 320, 128, [(300, 60, 200), (250, 20, 180)], 20, want=["roots_erased", "finished_by_prev_size"], n_out=2))
    # ---- fewer dots than N: stops when a pass no longer grows the list
    out.append(case("fewer_dots_than_N", 128, 128, lattice(10, 10, 120, 120, 24, _varied), 100, want=["finished_by_prev_size"], never=["final_phase"], n_out=25))
    # ---- tight clusters far apart, N between the number of clusters and the number of dots
    cl = cluster(6, 6) + cluster(100, 10) + cluster(20, 100) + cluster(96, 96, 4) + cluster(60, 50, 2)
    for n in (6, 9, 14, 22, 30):
        out.append(case("clusters_N%d" % n, 128, 128, cl, n, want=["zero_gain_split", "break_mid_walk"] + (["second_walk"] if n in (9, 14, 22) else []),
                        never=["cut_inside_tie_group"] if n == 9 else []))
    # ---- odd rectangles: pairs of dots 2 px apart (neither a 3 x 3 neighbour nor on the other's ring), N above the number of dots, so
    # every pair is separated: the deepest splits divide rectangles 2 and 3 px wide / high (ceil halves).  A 100 x 140 root halves to
    # 50 x 70, 25 x 35, 13|12 x 18|17, ... : two keys still share a rectangle 2 px wide only where it is higher than wide
    # A root twice as high as wide (70 x 140, nIni = round(0.5) = 1) still holds two keys in a rectangle ONE pixel wide, 149 x 100 in
    # one a pixel high: ceil(1 / 2) = 1, so the right-hand (lower) children have no width (height) at all
    for name, W, H in (("tall", 100, 140), ("wide", 140, 100), ("square", 100, 100), ("one_px_wide", 70, 140), ("one_px_high", 149, 100)):
        base = lattice(5, 5, W - 6, H - 6, 13, _varied)
        odd = list(base)
        for k, (x, y, v) in enumerate(base):
            dx, dy = ((2, 0), (0, 2), (1, 2), (2, 1))[k % 4]
            odd.append((x + dx, y + dy, v + 1 + k % 3))
        want = {"tall": ["split_w2", "split_w3", "split_h3"], "wide": ["split_h2", "split_h3", "split_w3"], "square": ["split_w3", "split_h3"],
                "one_px_wide": ["split_w1", "split_w2", "split_w3"], "one_px_high": ["split_h1", "split_h2", "split_h3"]}[name]
        out.append(case("odd_rectangles_" + name, W, H, odd, 600, want=want + ["finished_by_prev_size"], n_out=len(odd)))
    # ---- response ties inside a final node where cell order and raster order disagree: W = 70 has two cell columns, cell 0
    # evaluates x in [3, 38) and cell 1 [38, 67); the first pass cuts the root at x = 35, so (36, 30) and (44, 12) share quadrant n2.
    # (36, 30) comes first in vToDistributeKeys (cell 0) though it is lower in the image: it wins the tie.  Mirrored, the orders agree.
    out.append(case("tie_cell_order_beats_raster", 70, 70, [(36, 30, 140), (44, 12, 140), (10, 10, 120), (10, 60, 120), (60, 60, 120)], 2,
                    want=["response_tie_in_node", "stop_in_first_pass_above_N"], n_out=4))
    out.append(case("tie_cell_order_is_raster", 70, 70, [(36, 12, 140), (44, 30, 140), (10, 10, 120), (10, 60, 120), (60, 60, 120)], 2,
                    want=["response_tie_in_node", "stop_in_first_pass_above_N"], n_out=4))
    out.append(case("tie_broken_by_response", 70, 70, [(36, 30, 140), (44, 12, 141), (10, 10, 120), (10, 60, 120), (60, 60, 120)], 2,
                    never=["response_tie_in_node"], n_out=4))
    return out


def boundary_cases():
    """The final walk's `break`: on a boundary between groups of equal count (the selected set is the reference's own under any
    allocator) and inside such a group (the project's normative order decides).  128 x 128, N chosen so that the first pass (4 nodes)
    enters the final phase at once: 4 + 3 * nToExpand > N."""
    out = []
    # quadrant counts 9, 4, 4, 1: the walk splits the 9 (+3 nodes -> 7 >= N = 7) and stops before the two 4s
    # (every cluster straddles the centre of its 64 x 64 quadrant, so a split of it gains three nodes)
    q = cluster(27, 27) + cluster(94, 30, 2) + cluster(30, 94, 2) + [(100, 100, 150)]
    out.append(case("break_on_group_boundary", 128, 128, q, 7, want=["break_fired", "break_mid_walk"], never=["cut_inside_tie_group"]))
    # N = 8: the 9 is split (7 nodes), then the first of the two 4s (10 >= 8) and not the second
    out.append(case("break_inside_tie_group", 128, 128, q, 8, want=["break_fired", "cut_inside_tie_group"]))
    # counts 9, 9, 4, 1 and N = 10: both 9s are split (4 + 3 + 3 = 10), the break falls after the group of two
    q2 = cluster(27, 27) + cluster(91, 27) + cluster(30, 94, 2) + [(100, 100, 150)]
    out.append(case("break_after_whole_group", 128, 128, q2, 10, want=["break_fired", "cut_inside_tie_group"]))
    out.append(case("break_at_first_of_group", 128, 128, q2, 7, want=["break_fired", "cut_inside_tie_group"]))
    # all four quadrants alike, N = 5: the newest node (n4, bottom right) is the only one split
    q3 = cluster(30, 30, 2) + cluster(94, 30, 2) + cluster(30, 94, 2) + cluster(94, 94, 2)
    out.append(case("four_equal_quadrants", 128, 128, q3, 5, want=["break_fired", "cut_inside_tie_group"]))
    return out


def cell_cases():
    """140 x 105 inside the border: 4 x 3 cells of 35 x 35; cell (i, j) evaluates x in [35 j + 3, 35 j + 38), y in [35 i + 3, 35 i + 38)
    (the last column to 137, the last row to 102)."""
    W, H = 140, 105
    out = []
    out.append(case("adjacent_equal_pair_inside_a_cell", W, H, [(20, 20, 140), (21, 20, 140), (60, 50, 140), (60, 51, 140), (100, 80, 150)], 50,
                    cands={(100, 80, 109)}, n_out=1))
    out.append(case("adjacent_unequal_pair_inside_a_cell", W, H, [(20, 20, 140), (21, 20, 141), (100, 80, 150)], 50,
                    cands={(21, 20, 100), (100, 80, 109)}, n_out=2))
    # columns 37 | 38 and 72 | 73 belong to different cells, rows 37 | 38 likewise: neither sees the other's response
    out.append(case("equal_pair_across_a_cell_border_columns", W, H, [(37, 20, 140), (38, 20, 140), (72, 60, 140), (73, 60, 140)], 50))
    out.append(case("equal_pair_across_a_cell_border_rows", W, H, [(20, 37, 140), (20, 38, 140), (90, 72, 140), (90, 73, 140)], 50))
    out.append(case("equal_pair_across_a_cell_corner", W, H, [(37, 37, 140), (38, 38, 140)], 50))
    out.append(case("unequal_pair_across_a_cell_border", W, H, [(37, 20, 140), (38, 20, 190), (20, 37, 190), (20, 38, 140)], 50))
    # iniTh 20, minTh 7: a weak dot (response 9) is found only where its cell has nothing at iniTh
    out.append(case("strong_and_weak_cells", W, H, [(10, 10, 140), (20, 20, 50), (50, 10, 50), (60, 20, 52), (100, 50, 48), (100, 90, 46)], 50,
                    want=["cell_found_at_min_th"], cands={(10, 10, 99), (50, 10, 9), (60, 20, 11), (100, 50, 7)}, n_out=4))
    # first / last evaluated column and row of the level, and one pixel outside
    out.append(case("level_edges", W, H, [(3, 50, 140), (2, 60, 140), (136, 50, 140), (137, 60, 140), (50, 3, 140), (60, 2, 140), (70, 101, 140), (80, 102, 140)], 50,
                    cands={(3, 50, 99), (136, 50, 99), (50, 3, 99), (70, 101, 99)}, n_out=4))
    out.append(case("level_corners", W, H, [(3, 3, 140), (136, 3, 141), (3, 101, 142), (136, 101, 143)], 50, n_out=4))
    out.append(case("dark_dots", W, H, [(20, 20, 100), (60, 60, 90), (100, 30, 80)], 50, bg=200, n_out=3))
    return out


def skipped_column_widths(limit=2400):
    """Level widths (inner width + 32 <= limit) whose last cell column is skipped by `iniX >= maxBorderX - 6` (ORBextractor.cc:1102)
    though a row at the same distance would pass `iniY >= maxBorderY - 3` (:1085): (nCols - 1) * wCell in [W - 6, W - 3)."""
    out = []
    for W in range(35, limit - 32 + 1):
        n = W // 35
        wc = -(-W // n)
        if W - 6 <= (n - 1) * wc < W - 3:
            out.append(W + 32)
    return out


def wide_cases():
    """Wide frame x small budget: 4 * nIni nodes per level whatever N is."""
    out = []
    for W, H, n_ini, budgets in ((1241 - 32, 376 - 32, 4, (4, 7)), (2400 - 32, 420 - 32, 6, (11, 15))):
        dots = lattice(5, 5, W - 4, H - 4, 12, _varied)
        for nf in budgets:
            out.append(case("wide_%d_nl1_N%d" % (W + 32, nf), W, H, dots, nf, want=["stop_in_first_pass_above_N"], n_out=4 * n_ini))
    for n in (1, 2, 3, 4):
        out.append(case("wide_352x160_N%d" % n, 320, 128, lattice(5, 5, 316, 124, 10, _varied), n, want=["stop_in_first_pass_above_N"], n_out=12))
    return out


def wide_pyramid_cases():
    """The same wide frames through 8 levels with a budget below 4 * nIni on every level.  2 x 2 blobs survive the resizes as corners."""
    out = []
    for w, h, nf in ((1241, 376, 20), (2400, 420, 50)):
        img = np.full((h, w), BG, np.uint8)
        for y in range(22, h - 22, 14):
            for x in range(22, w - 22, 14):
                img[y:y + 2, x:x + 2] = _varied(x, y) + 25
                img[y, x] += 15                                                 # a strict maximum on level 0 too
        out.append(dict(name="wide_%d_nl8_nf%d" % (w, nf), img=img, nf=nf, nl=8, sf=1.2, ini=20, mn=7, lap=(0, 0),
                        want=("stop_in_first_pass_above_N",), never=(), cands=None, n_out=None))
    return out


def epilogue_frame(sf):
    """176 x 112, two levels: dots every 6 (sf 1.2) or 13 (sf 1.3) px of level 0 land on whole pixels of level 1, which the epilogue
    scales back by one float32 multiply: the products fall exactly on integers, or one ulp beside them."""
    w, h = 176, 112
    img = np.full((h, w), BG, np.uint8)
    step = 6 if sf == 1.2 else 13
    for y in range(step * 4, h - 20, step * 2):
        for x in range(step * 3, w - 19, step):
            img[y, x] = 250
    return img


def epilogue_cases():
    out = []
    # pins: (scaled x of a level-1 keypoint as float32, is it inside the lapping area): 90 * 1.2f = 108 + 1 ulp, 90 * 1.3f = 117 - 1 ulp,
    # 30 * 1.2f = 36, 60 * 1.2f = 72, 75 * 1.2f = 90, 80 * 1.3f = 104 and 100 * 1.3f = 130 exactly
    up, dn = np.nextafter(np.float32(108), np.float32(200)), np.nextafter(np.float32(117), np.float32(0))
    for sf, laps in ((1.2, (((0, 0), [(72.0, False)]), ((0, 176), [(72.0, True), (up, True)]), ((-5, 1000), [(36.0, True)]), ((500, 600), [(144.0, False)]),
                           ((36, 90), [(36.0, True), (90.0, True), (up, False)]), ((72, 108), [(72.0, True), (90.0, True), (up, False), (42.0, False)]),
                           ((72, 72), [(72.0, True), (90.0, False)]))),
                     (1.3, (((0, 0), [(dn, False)]), ((0, 176), [(dn, True)]), ((117, 130), [(dn, False), (130.0, True), (143.0, False)]),
                           ((104, 117), [(104.0, True), (dn, True), (91.0, False)]), ((52, 104), [(52.0, True), (104.0, True), (dn, False)])))):
        for lap, pins in laps:
            out.append(dict(name="epilogue_sf%s_lap_%d_%d" % (sf, lap[0], lap[1]), img=epilogue_frame(sf), nf=60, nl=2, sf=sf, ini=20, mn=7, lap=lap,
                            want=(), never=(), cands=None, n_out=None, pins=[(np.float32(x), b) for x, b in pins]))
    return out


def all_cases():
    return quadtree_cases() + boundary_cases() + cell_cases() + wide_cases() + epilogue_cases() + wide_pyramid_cases()


def key(c):
    """Frames with the same key can share an extractor and go through one batch."""
    return (c["img"].shape[1], c["img"].shape[0], c["nf"], c["nl"], c["sf"], c["ini"], c["mn"])
