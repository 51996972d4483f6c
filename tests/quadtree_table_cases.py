"""Hand-laid frames for k_quadtree2's table mode (path histograms instead of passes over the candidates) and its fallback, built with
tests/extract_cases.py's case / paint / lattice and held to tests/second_reading_extract.py like them.  Pure numpy; imports neither
the oracle nor the product.

The kernel refines a level on histograms of the candidates' paths through the first D subdivisions of their root and only walks the
candidates again when a node at depth D still holds two of them (orbx_plan.h picks D; table_depth() below restates the rule and
tests/test_quadtree_table_cases_cpu.py pins it to the planner).  What decides the mode of a level is therefore how deep two candidates
stay together.  node_path() and separating_depth() walk the reference's own halving (ExtractorNode::DivideNode, ceil halves, i.e.
(w + 1) >> 1) for given points, so a case's expectation -- falls back or not -- comes from the reference's geometry, not from the kernel.

Two dots alone never get deep: the first pass that does not grow the list ends DistributeOctTree (ORBextractor.cc:889), and a pair
that stays together splits with zero gain.  ladder(s) therefore gives a pair that separates at depth s one more dot per depth 1..s-1
that leaves the pair's node exactly there: every pass grows the list by one until the pair is apart.  With a budget above the number
of dots every dot ends in a node of its own (n_out = number of dots), so the level certainly runs an iteration with a two-key node at
every depth below s: it falls back if and only if s >= D + 1.

Extra fields of a case: area (inner W, H), deep (levels that must fall back: known by construction), D (table depth its geometry plans).
For frames that are not ladders levels_that_fall_back() decides: it walks the second reading's DistributeOctTree with DivideNode watched.
"""
import math

import numpy as np

import extract_cases as ec
import second_reading_extract as sr

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- the reference's halving
def roots(W, H):
    """(nIni, hX) of an inner area W x H (ORBextractor.cc:695-698)."""
    n_ini = int(math.floor(float(F(F(W) / F(H))) + 0.5))
    return n_ini, F(F(W) / F(n_ini))


def node_path(x, y, W, H, depth):
    """(root, q1, .., q_depth): the node that holds key (x, y) after `depth` subdivisions of its root."""
    n_ini, hx = roots(W, H)
    r = int(F(F(x) / hx))                                                        # :740
    ulx, urx, uly, bry = int(F(hx * F(r))), int(F(hx * F(r + 1))), 0, H           # :717-720
    path = [r]
    for _ in range(depth):
        mx, my = ulx + ((urx - ulx + 1) >> 1), uly + ((bry - uly + 1) >> 1)      # :608-609
        q = (0 if x < mx else 1) + (0 if y < my else 2)                          # :651-664
        ulx, urx = (ulx, mx) if x < mx else (mx, urx)
        uly, bry = (uly, my) if y < my else (my, bry)
        path.append(q)
    return tuple(path)


def separating_depth(p, q, W, H, limit=14):
    """Number of subdivisions after which p and q lie in different nodes (0: different roots); None if they never part."""
    for d in range(limit + 1):
        if node_path(p[0], p[1], W, H, d) != node_path(q[0], q[1], W, H, d):
            return d
    return None


def share_a_node(points, W, H, depth):
    """True when two of the points lie in one node after `depth` subdivisions."""
    seen = set()
    for x, y in points:
        p = node_path(int(x), int(y), W, H, depth)
        if p in seen:
            return True
        seen.add(p)
    return False


# ---------------------------------------------------------------------------------------------------------------- the planner's rule, restated
def table_depth(k):
    """D of orbx_plan.h for an extractor key (w, h, nf, nl, sf, ..): the largest of fuseD .. fuseD + 2 whose extra histogram levels fit
    on childPos / newPos (10 B per list entry), whose path table fits on the sort keys and whose paths fit 12 bits.
    Returns (fuseD, D, maxN, maxIni)."""
    w, h, nf, nl, sf = k[:5]
    sizes = sr.level_sizes(w, h, sf, nl)
    inis = [sr.c_round(F(lw - 32) / F(lh - 32)) for lw, lh in sizes]
    max_n = max(max(n, 4 * i) for n, i in zip(sr.features_per_level(nf, sf, nl), inis))
    max_ini = max(inis)
    cap = max_n + 8
    sort = 1 << (cap - 1).bit_length()
    fuse = 4 if max_n >= 512 and max_ini <= 4 else 3
    depth = fuse
    for d in (fuse + 2, fuse + 1):
        paths = max_ini << (2 * d)
        hist = 4 * sum(max_ini << (2 * e) for e in range(fuse + 1, d + 1))
        if paths <= 4096 and hist <= 10 * cap and 2 * paths <= 8 * sort:
            depth = d
            break
    return fuse, depth, max_n, max_ini


# ---------------------------------------------------------------------------------------------------------------- constructions
A = 128                                                                          # the ladders' inner area: halves stay even down to 2 px


def ladder(s, y0=9):
    """s + 1 dots in a 128 x 128 area: a pair 2 px apart that separates at depth s (2 <= s <= 6), and for d = 1 .. s - 1 one dot that
    shares the pair's node down to depth d - 1 and leaves it at depth d."""
    c = A >> s
    pair = [(64 + c - 1, y0), (64 + c + 1, y0)]
    assert separating_depth(pair[0], pair[1], A, A) == s
    dots = list(pair)
    for d in range(1, s):
        rung = next((x, y) for y in range(5, A - 6) for x in range(5, A - 6)
                    if separating_depth((x, y), pair[0], A, A) == d and all(max(abs(x - a), abs(y - b)) >= 5 for a, b in dots))
        dots.append(rung)
    for i, p in enumerate(dots):                                                 # the pair is the only couple that stays together to depth s - 1
        for q in dots[:i]:
            d = separating_depth(p, q, A, A)
            assert d == s if {p, q} == set(pair) else d < s
    return [(x, y, 120 + 7 * i) for i, (x, y) in enumerate(dots)]


def triple(s):
    """s + 2 dots in a 128 x 128 area: three dots around the centre of one node of depth s - 1 (2 <= s <= 6), in three of its quadrants
    and 2 px apart (offsets (2, 1), (0, 2), (-2, 1): none a 3 x 3 neighbour or on another's ring), and one dot per depth 1 .. s - 1 as
    in ladder()."""
    c = A >> s
    mx, my = 64 + c, (8 // (2 * c)) * 2 * c + c                                  # the node [64, 64 + 2c) x [my - c, my + c)
    three = [(mx - 2, my - 2), (mx, my - 1), (mx - 2, my)]
    dots = list(three)
    for d in range(1, s):
        dots.append(next((x, y) for y in range(5, A - 6) for x in range(5, A - 6)
                         if separating_depth((x, y), three[0], A, A) == d and all(max(abs(x - a), abs(y - b)) >= 5 for a, b in dots)))
    for i, p in enumerate(dots):                                                 # the three part from one another at depth s, every other couple earlier
        for q in dots[:i]:
            d = separating_depth(p, q, A, A)
            assert d == s if p in three and q in three else d < s
    return [(x, y, 120 + 7 * i) for i, (x, y) in enumerate(dots)]


def _case(name, W, H, dots, nf, deep=(), **kw):
    c = ec.case(name, W, H, dots, nf, cands=kw.pop("cands", None), **kw)
    c["area"] = (W, H)
    c["deep"] = tuple(deep)
    c["D"] = table_depth(ec.key(c))[1]
    return c


def ladder_cases():
    """For D = 3, 4, 5 (budgets 60, 400, 600 on one level of 160 x 160): pairs that separate at depth D - 1 (table mode to the end),
    D (the last iteration the tables can serve) and D + 1 (fallback, in state 0: the budget is far away)."""
    out = []
    for D, nf in ((3, 60), (4, 400), (5, 600)):
        for s in (D - 1, D, D + 1):
            dots = ladder(s)
            out.append(_case("ladder_D%d_s%d" % (D, s), A, A, dots, nf, deep=(0,) if s >= D + 1 else (), want=["finished_by_prev_size"],
                             never=["final_phase"], n_out=len(dots)))
            assert out[-1]["D"] == D
    # three dots that stay in one node down to depth s - 1 and go three ways at depth s: a node with three keys is served by the last
    # table iteration (s = D), or meets the fallback (s = D + 1).  (The node with three keys that splits 2 + 1 and hands a pair one
    # level down is in every ladder: the pair and the dot that leaves it last.)
    for D, nf in ((3, 60), (4, 400), (5, 600)):
        for s in (D - 1, D, D + 1):
            dots = triple(s)
            out.append(_case("triple_D%d_s%d" % (D, s), A, A, dots, nf, deep=(0,) if s >= D + 1 else (), want=["finished_by_prev_size"],
                             never=["final_phase"], n_out=len(dots)))
            assert out[-1]["D"] == D
    # ---- the final phase on the way down (D = 3): budget = number of dots, so the last passes are walks of the final phase
    d4, d3, d6 = ladder(4), ladder(3), ladder(6)
    out.append(_case("ladder_state1_s3", A, A, d3, 5, want=["final_phase"], n_out=len(d3)))                    # tables to the end
    out.append(_case("ladder_state1_s4", A, A, d4, 5, deep=(0,), want=["final_phase", "break_fired"], n_out=len(d4)))     # falls back inside the final phase
    out.append(_case("ladder_state0_then_1_s6", A, A, d6, 7, deep=(0,), want=["final_phase", "break_fired"], n_out=len(d6)))   # falls back before it, ends in it
    out.append(_case("ladder_state1_s2_shallow", A, A, ladder(2), 7, want=["finished_by_prev_size"], n_out=3))
    return out


def phase_cases():
    out = []
    full = ec.lattice(4, 4, A, A, 8, ec._varied)                                  # 16 x 16 dots: 4, 16, 64, 256 nodes after 1, 2, 3, 4 full passes
    for passes, nf in ((1, 10), (2, 40), (3, 150)):                              # 4 + 12 > 10; 16 <= 40 < 16 + 48; 64 <= 150 < 64 + 192
        out.append(_case("final_phase_after_%d" % passes, A, A, full, nf, want=["final_phase", "break_fired"], never=["second_walk"]))
    cl = ec.cluster(6, 6) + ec.cluster(100, 10) + ec.cluster(20, 100) + ec.cluster(96, 96, 4) + ec.cluster(60, 50, 2)
    out.append(_case("second_walk_falls_back", A, A, cl, 14, want=["final_phase", "second_walk", "zero_gain_split"]))   # (its second walk divides depth-3 nodes)
    # two walks that the tables serve (D = 3): two 2 x 2 clusters per quadrant, each across the centre of its 32 x 32 node.  Pass 1: 4 nodes,
    # 4 + 3 * 4 > 10; walk 1 parts the clusters (8 nodes < 10), walk 2 divides depth-2 nodes and stops at the first (11 >= 10)
    two = [d for qx in (0, 64) for qy in (0, 64) for k in (0, 32) for d in ec.cluster(qx + k + 14, qy + k + 14, 2)]
    out.append(_case("second_walk_on_tables", A, A, two, 10, want=["final_phase", "second_walk", "break_fired"]))
    # a pair without a ladder beside a ladder: its node splits with zero gain while the ladder keeps the passes growing.  The pass
    # that ends the level (no growth) still divides the pair's node, one level below the ladder's last: s = D - 1 = 2 keeps it on the tables
    out.append(_case("zero_gain_in_table_mode", A, A, ladder(2) + [(20, 100, 150), (22, 100, 160)], 60, want=["zero_gain_split", "finished_by_prev_size"]))
    # response tie inside a final node whose keys come from two cells (see extract_cases: tie_cell_order_beats_raster)
    out.append(_case("tie_through_path_table", 70, 70, [(36, 30, 140), (44, 12, 140), (10, 10, 120), (10, 60, 120), (60, 60, 120)], 2,
                     want=["response_tie_in_node", "stop_in_first_pass_above_N"], n_out=4))
    return out


def root_cases():
    """1 .. 4 roots (ratios 1, 1.5, 2.5, 3.5) with an erased root: the path table has rows no node owns.  The last root of the wider
    ones holds a single dot."""
    out = [_case("no_candidate", 64, 64, [], 5, want=["roots_erased"], n_out=0)]
    for n_ini, W, H, empty in ((2, 180, 120, 0), (3, 180, 72, 1), (4, 175, 50, 2)):
        assert roots(W, H)[0] == n_ini
        hx = roots(W, H)[1]
        dots = []
        for r in range(n_ini):
            x0, x1 = int(hx * F(r)), int(hx * F(r + 1))
            if r == empty:
                continue
            if r == n_ini - 1 and n_ini > 2:
                dots.append(((x0 + x1) // 2, H // 2, 200))                       # a root with one key
            else:
                dots += ec.lattice(x0 + 5, 5, x1 - 4, H - 4, 9, ec._varied)
        want = ["roots_erased", "final_phase"] + (["roots_single"] if n_ini > 2 else [])
        out.append(_case("roots_%d_one_erased" % n_ini, W, H, dots, 14, want=want))
    # a budget below 4 * nIni: every root is split once whatever N is
    out.append(_case("budget_below_4_roots", 175, 50, ec.lattice(5, 5, 171, 46, 9, ec._varied), 5, want=["stop_in_first_pass_above_N"], n_out=16))
    return out


def pyramid_cases():
    """Two and three levels: 2 x 2 blobs survive the resizes as corners.  weak_second_level: dots just above iniTh = minTh on level 0
    that the resize flattens, so level 1 has no candidate at all."""
    out = []
    for name, w, h, nl, nf in (("pyramid_2_levels", 176, 144, 2, 60), ("pyramid_3_levels", 180, 150, 3, 150)):
        img = np.full((h, w), ec.BG, np.uint8)
        for y in range(22, h - 22, 11):
            for x in range(22, w - 22, 11):
                img[y:y + 2, x:x + 2] = ec._varied(x, y) + 25
                img[y, x] += 15
        c = dict(name=name, img=img, nf=nf, nl=nl, sf=1.2, ini=20, mn=7, lap=(0, 0), want=("final_phase",), never=(), cands=None, n_out=None,
                 area=(w - 32, h - 32), deep=())
        c["D"] = table_depth(ec.key(c))[1]
        out.append(c)
    dots = [(x, y, ec.BG + 24) for x, y, _ in ec.lattice(7, 7, 100, 100, 13)]     # (odd positions at sf 1.5: no level-1 pixel samples a dot alone)
    c = ec.case("weak_second_level", 112, 112, dots, 40, nl=2, sf=1.5, ini=20, mn=20, cands=None)
    c.update(area=(112, 112), deep=())
    c["D"] = table_depth(ec.key(c))[1]
    out.append(c)
    return out


def all_cases():
    return ladder_cases() + phase_cases() + root_cases() + pyramid_cases()


def levels_sharing_a_node(c, candidates):
    """Levels of case c on which two candidates ((n, 3) arrays per level, as the reading returns them) lie in one node at depth D: the
    only levels that can leave table mode.  A level not listed runs on the tables whatever its budget."""
    out = []
    for l, (lw, lh) in enumerate(sr.level_sizes(c["img"].shape[1], c["img"].shape[0], c["sf"], c["nl"])):
        k = np.asarray(candidates[l]).reshape(-1, 3)
        if share_a_node([(int(x), int(y)) for x, y in k[:, :2]], lw - 32, lh - 32, c["D"]):
            out.append(l)
    return out


def levels_that_fall_back(c, rd, depth=None):
    """Levels of case c whose quadtree leaves table mode, from the reading rd of its level images: DistributeOctTree is walked again per
    level with DivideNode watched.  A node is never divided in the pass that made it (a full pass steps over the children it pushes, a
    walk of the final phase takes the previous pass's children), so the pass of a division is one more than the pass its node was born
    in.  The tables serve a pass as long as every node with more than one key is shallower than D; the level falls back when a pass
    runs after one that made a node with several keys at depth D -- whether or not that pass gets as far as dividing it."""
    D = c["D"] if depth is None else depth
    out = []
    inner = sr.divide_node
    for l, (lw, lh) in enumerate(sr.level_sizes(c["img"].shape[1], c["img"].shape[0], c["sf"], c["nl"])):
        born = {}                                                                # id(node) -> (node, depth, pass it was made in); roots: depth 0, pass 0
        made_deep, last_pass = [], [0]

        def watched(n, kx, ky, t=None):
            _, d, p = born.get(id(n), (n, 0, 0))
            last_pass[0] = max(last_pass[0], p + 1)
            children = inner(n, kx, ky, t)
            for ch in children:
                born[id(ch)] = (ch, d + 1, p + 1)
                if len(ch.keys) > 1 and d + 1 >= D:
                    made_deep.append(p + 1)
            return children

        sr.divide_node = watched
        try:
            sr.distribute_oct_tree(rd["candidates"][l], sr.BORDER, lw - sr.BORDER, sr.BORDER, lh - sr.BORDER, rd["budget"][l])
        finally:
            sr.divide_node = inner
        if made_deep and last_pass[0] > min(made_deep):
            out.append(l)
    return out
