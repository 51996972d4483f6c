"""A second, independent reading of the extractor between its numpy-pinned pieces, in plain Python / numpy.

Written from the reference's src/ORBextractor.cc alone: the constructor's split of nfeatures (:509-526), ComputePyramid's level sizes
(:1664-1672), ComputeKeyPointsOctTree's cell loop (:1038-1177), ExtractorNode::DivideNode (:602-674), DistributeOctTree (:688-1034)
and the epilogue of operator() (:1587-1658).  It imports no product code and no oracle.  The level images (mvImagePyramid without
its border) are data and are handed in; the resize, the Gaussian, IC_Angle and the descriptor have numpy statements of their own
(tests/test_oracle_params_cpu.py, tests/test_oracle_structured_cpu.py) and are not restated.

Arithmetic follows the C++ operand types: every float operation is one np.float32 operation, an int met by a float becomes a float,
float -> int truncates, `round` is C's (half away from zero), cvRound rounds half to even, `ceil` as written.

cv::FAST(img, keys, threshold, true) is OpenCV's FAST-9/16: a pixel at least 3 px inside `img` is a corner when nine contiguous pixels
of its 16-pixel ring are all brighter than v + threshold or all darker than v - threshold; its response is the largest threshold at
which it still is one, max(A, B) - 1 with A (B) the largest over the 16 arcs of the smallest amount by which the centre is above
(below) the arc; it is kept when its response is strictly greater than that of its eight neighbours, a neighbour that is no corner
-- or lies outside the evaluated pixels of `img` -- counting 0.  Keypoints come out in row-major order.  The reference calls it on the
cell's own sub-image (:1112), so the responses beyond a cell's evaluated pixels do not exist for that cell.

The one place where the reference is under-determined is the sort on pair<int, ExtractorNode*> (:927): nodes of equal count are
ordered by their heap addresses.  `tie` names the order used instead: "newest" (the project's normative choice: the node created
last is split first), "oldest", or a random.Random / seed for a random order.  The counter `cut_inside_tie_group` says when that
choice can matter for the selected SET: it is raised when the `break` of :983 fires at a node whose neighbour in the sorted vector,
on either side, has the same count.  Without it only the ORDER of the result depends on the rule.
"""
import math
import random
from collections import Counter

import numpy as np

F = np.float32

EDGE_THRESHOLD = 19          # ORBextractor.cc:76
PATCH_SIZE = 31              # :74
BORDER = EDGE_THRESHOLD - 3  # minBorderX / minBorderY (:1053-1054)

KEY_FIELDS = ("x", "y", "size", "response", "octave", "class_id")        # cv::KeyPoint without its angle

# every counter distribute_oct_tree names; tests/test_second_reading_extract_cpu.py wants each reached somewhere
COUNTERS = ("roots_erased", "roots_single", "key_outside_root_rect", "finished_in_full_pass", "finished_by_prev_size",
            "stop_in_first_pass_above_N", "final_phase", "final_walks", "second_walk", "break_fired", "break_mid_walk",
            "zero_gain_split", "response_tie_in_node", "cut_inside_tie_group", "split_w1", "split_w2", "split_w3", "split_h1", "split_h2", "split_h3")


def c_round(x):
    """C's round(): half away from zero."""
    x = float(x)
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def cv_round(x):
    """cvRound: to nearest, halves to even."""
    return int(np.rint(x))


# ---------------------------------------------------------------------------------------------------------------- constructor, pyramid
def scale_factors(scale_factor, nlevels):
    """mvScaleFactor / mvInvScaleFactor (:482-499)."""
    sf = [F(1.0)]
    for _ in range(1, nlevels):
        sf.append(F(sf[-1] * F(scale_factor)))                                   # :488
    return np.array(sf, F), np.array([F(F(1.0) / s) for s in sf], F)             # :498


def features_per_level(nfeatures, scale_factor, nlevels):
    """mnFeaturesPerLevel (:509-526)."""
    factor = F(F(1.0) / F(scale_factor))                                         # :509
    p = F(math.pow(float(factor), float(nlevels)))                               # (float)pow((double)factor, (double)nlevels)
    per_scale = F(F(F(nfeatures) * F(F(1) - factor)) / F(F(1) - p))              # :511
    out, total = [], 0
    for _ in range(nlevels - 1):                                                 # :516
        out.append(cv_round(per_scale)); total += out[-1]                        # :519-521
        per_scale = F(per_scale * factor)                                        # :523
    out.append(max(nfeatures - total, 0))                                        # :526
    return out


def level_sizes(w, h, scale_factor, nlevels):
    """Size of every pyramid level (:1668-1669): cvRound((float)cols * mvInvScaleFactor[level])."""
    isf = scale_factors(scale_factor, nlevels)[1]
    return [(cv_round(F(F(w) * s)), cv_round(F(F(h) * s))) for s in isf]


# ---------------------------------------------------------------------------------------------------------------- FAST, the cell loop
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3))                                                        # (dx, dy) once round the circle of radius 3


def fast_scores(img, threshold):
    """Response of every corner of img's pixels [3, h - 3) x [3, w - 3), 0 where there is none: an (h - 6, w - 6) array."""
    h, w = img.shape
    a = img.astype(np.int32)
    c = a[3:h - 3, 3:w - 3]
    d = np.stack([c - a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])
    d = np.concatenate([d, d[:8]])
    A = np.max(np.stack([d[s:s + 9].min(axis=0) for s in range(16)]), axis=0)
    B = np.max(np.stack([(-d[s:s + 9]).min(axis=0) for s in range(16)]), axis=0)
    m = np.maximum(A, B)
    return np.where(m > threshold, m - 1, 0)


def fast(img, threshold):
    """cv::FAST(img, keys, threshold, true): [(x, y, response)] in row-major order."""
    h, w = img.shape
    if h < 7 or w < 7:
        return []
    s = fast_scores(img, threshold)
    p = np.zeros((h - 4, w - 4), s.dtype)
    p[1:-1, 1:-1] = s                                                            # no response outside the evaluated pixels
    nb = [p[1 + dy:h - 5 + dy, 1 + dx:w - 5 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    keep = (s > 0) & (s > np.max(np.stack(nb), axis=0))
    ys, xs = np.nonzero(keep)                                                    # row-major
    return [(int(x) + 3, int(y) + 3, int(s[y, x])) for y, x in zip(ys, xs)]


def cell_grid(cols, rows):
    """The cells of a cols x rows level (:1055-1106): ([(iniX, iniY, maxX, maxY, i, j)], wCell, hCell) in the loop's order."""
    min_bx = min_by = BORDER
    max_bx = cols - EDGE_THRESHOLD + 3; max_by = rows - EDGE_THRESHOLD + 3      # :1055-1056
    width = F(max_bx - min_bx); height = F(max_by - min_by)                      # :1064-1065
    W = F(35)                                                                    # :1046
    n_cols = int(F(width / W)); n_rows = int(F(height / W))                      # :1068-1069
    assert n_cols > 0 and n_rows > 0, "a level narrower than one cell divides by zero at :1071"
    w_cell = int(math.ceil(F(width / F(n_cols)))); h_cell = int(math.ceil(F(height / F(n_rows))))     # :1071-1072
    cells = []
    for i in range(n_rows):                                                      # :1075
        ini_y = F(min_by + i * h_cell)                                           # :1078
        max_y = F(F(ini_y + F(h_cell)) + F(6))                                   # :1082
        if ini_y >= max_by - 3:                                                  # :1085
            continue
        if max_y > max_by:                                                       # :1089
            max_y = F(max_by)
        for j in range(n_cols):                                                  # :1093
            ini_x = F(min_bx + j * w_cell)                                       # :1096
            max_x = F(F(ini_x + F(w_cell)) + F(6))                               # :1098
            if ini_x >= max_bx - 6:                                              # :1102  (6, not 3)
                continue
            if max_x > max_bx:                                                   # :1105
                max_x = F(max_bx)
            cells.append((int(ini_x), int(ini_y), int(max_x), int(max_y), i, j))
    return cells, w_cell, h_cell


def cell_keys(level_image, ini_th, min_th, counters=None):
    """vToDistributeKeys of one level (:1059-1143) as an (n, 3) int array of (pt.x, pt.y, response): row of cells, column of cells,
    FAST's own order inside a cell; coordinates relative to (minBorderX, minBorderY)."""
    rows, cols = level_image.shape
    cells, w_cell, h_cell = cell_grid(cols, rows)
    t = counters if counters is not None else Counter()
    out = []
    for ini_x, ini_y, max_x, max_y, i, j in cells:
        sub = level_image[ini_y:max_y, ini_x:max_x]                              # rowRange(iniY, maxY).colRange(iniX, maxX)
        keys = fast(sub, ini_th)                                                 # :1112
        if not keys:                                                             # :1118
            keys = fast(sub, min_th)                                             # :1121
            t["cell_retry_min_th"] += 1
            t["cell_found_at_min_th"] += bool(keys)
        for x, y, r in keys:                                                     # :1131
            out.append((x + j * w_cell, y + i * h_cell, r))                      # :1136-1137
    return np.array(out, np.int64).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------- the quadtree
class _Node:
    __slots__ = ("ulx", "uly", "urx", "brx", "bry", "keys", "no_more", "seq", "rnd")

    def __init__(self):
        self.keys = []; self.no_more = False; self.seq = -1; self.rnd = 0.0


def divide_node(n, kx, ky, t=None):
    """ExtractorNode::DivideNode (:602-674): the four children n1..n4 (UL, UR, BL, BR quadrant) of node n."""
    if t is not None:                                                            # a rectangle of 1, 2 or 3 px is divided: ceil halves
        if n.urx - n.ulx <= 3:
            t["split_w%d" % (n.urx - n.ulx)] += 1
        if n.bry - n.uly <= 3:
            t["split_h%d" % (n.bry - n.uly)] += 1
    half_x = int(math.ceil(F(F(n.urx - n.ulx) / F(2))))                          # :608
    half_y = int(math.ceil(F(F(n.bry - n.uly) / F(2))))                          # :609
    mx, my = n.ulx + half_x, n.uly + half_y
    c = [_Node() for _ in range(4)]
    c[0].ulx, c[0].uly, c[0].urx, c[0].brx, c[0].bry = n.ulx, n.uly, mx, mx, my                     # :614-617
    c[1].ulx, c[1].uly, c[1].urx, c[1].brx, c[1].bry = mx, n.uly, n.urx, n.urx, my                  # :622-625
    c[2].ulx, c[2].uly, c[2].urx, c[2].brx, c[2].bry = n.ulx, my, mx, mx, n.bry                     # :629-632
    c[3].ulx, c[3].uly, c[3].urx, c[3].brx, c[3].bry = mx, my, n.urx, n.brx, n.bry                  # :636-639
    for k in n.keys:                                                             # :644
        if kx[k] < mx:                                                           # :651  strict, against n1.UR.x
            (c[0] if ky[k] < my else c[2]).keys.append(k)                        # :653
        elif ky[k] < my:                                                         # :658
            c[1].keys.append(k)
        else:
            c[3].keys.append(k)
    for ch in c:                                                                 # :666-673
        if len(ch.keys) == 1:
            ch.no_more = True
    return c


def distribute_oct_tree(keys, minX, maxX, minY, maxY, N, tie="newest"):
    """DistributeOctTree (:688-1034).  keys: (n, 3) of (pt.x, pt.y, response) relative to (minX, minY).
    Returns (indices into keys in the order of vResultKeys, Counter of the branches taken)."""
    keys = np.asarray(keys).reshape(-1, 3)
    kx = [float(F(v)) for v in keys[:, 0]]; ky = [float(F(v)) for v in keys[:, 1]]; kr = [float(F(v)) for v in keys[:, 2]]
    t = Counter()
    rng = tie if isinstance(tie, random.Random) else random.Random(tie) if isinstance(tie, int) else None
    assert rng is not None or tie in ("newest", "oldest")
    seq = [0]

    def born(n):                                                                 # a node enters lNodes
        n.seq = seq[0]; seq[0] += 1
        n.rnd = rng.random() if rng else 0.0
        return n

    def order(entry):                                                            # what stands in for the node's address at :927
        n = entry[1]
        return (entry[0], n.seq if tie == "newest" else -n.seq if tie == "oldest" else n.rnd)

    n_ini = c_round(F(F(maxX - minX) / F(maxY - minY)))                          # :695
    assert n_ini >= 1, "nIni == 0 divides by zero at :698"
    hX = F(F(maxX - minX) / F(n_ini))                                            # :698
    lnodes = []                                                                  # lNodes, front at index 0
    roots = []
    for i in range(n_ini):                                                       # :710
        n = _Node()
        n.ulx = int(F(hX * F(i))); n.urx = int(F(hX * F(i + 1)))                 # :717-718
        n.uly = 0; n.brx = n.urx; n.bry = maxY - minY                            # :719-720
        lnodes.append(born(n)); roots.append(n)                                  # :728-730
    for k in range(len(kx)):                                                     # :735
        r = int(F(F(kx[k]) / hX))                                                # :740
        assert 0 <= r < n_ini, "key outside every root: the reference indexes vpIniNodes out of range"
        roots[r].keys.append(k)
        if not (roots[r].ulx <= kx[k] < roots[r].urx):
            t["key_outside_root_rect"] += 1
    p = 0
    while p < len(lnodes):                                                       # :746
        if len(lnodes[p].keys) == 1:                                             # :749
            lnodes[p].no_more = True; t["roots_single"] += 1; p += 1
        elif not lnodes[p].keys:                                                 # :757
            del lnodes[p]; t["roots_erased"] += 1
        else:
            p += 1

    def push_children(children, vsp):                                            # :823-874 and :938-975
        gain = -1
        for ch in children:
            if ch.keys:
                lnodes.insert(0, born(ch)); gain += 1                            # push_front
                if len(ch.keys) > 1:
                    vsp.append((len(ch.keys), ch))
        return gain

    finish = False
    vsp = []                                                                     # vSizeAndPointerToNode
    first_pass = True
    while not finish:                                                            # :779
        prev_size = len(lnodes)                                                  # :785
        n_to_expand = 0                                                          # :791
        vsp = []                                                                 # :796
        p = 0
        while p < len(lnodes):                                                   # :800
            n = lnodes[p]
            if n.no_more:                                                        # :803
                p += 1
                continue
            before = len(vsp)
            children = divide_node(n, kx, ky, t)                                  # :818
            gain = push_children(children, vsp)
            n_to_expand += len(vsp) - before
            p += gain + 1                                                        # the iterator still points at the parent
            del lnodes[p]                                                        # :878; p is now the parent's successor
            t["zero_gain_split"] += gain == 0
        if len(lnodes) >= N or len(lnodes) == prev_size:                         # :889
            finish = True
            t["finished_in_full_pass" if len(lnodes) >= N else "finished_by_prev_size"] += 1
            t["stop_in_first_pass_above_N"] += first_pass and len(lnodes) > N
        elif len(lnodes) + n_to_expand * 3 > N:                                  # :909
            t["final_phase"] += 1
            walks = 0
            while not finish:                                                    # :914
                prev_size = len(lnodes)                                          # :917
                prev = sorted(vsp, key=order)                                    # :920-927
                vsp = []                                                         # :922
                walks += 1; t["final_walks"] += 1
                t["second_walk"] += walks == 2
                for j in range(len(prev) - 1, -1, -1):                           # :930  from the back
                    n = prev[j][1]
                    gain = push_children(divide_node(n, kx, ky, t), vsp)         # :934-975
                    lnodes.remove(n)                                             # :978  (list.remove compares identity: no __eq__)
                    t["zero_gain_split"] += gain == 0
                    if len(lnodes) >= N:                                         # :983
                        t["break_fired"] += 1
                        t["break_mid_walk"] += j > 0
                        same = (j > 0 and prev[j - 1][0] == prev[j][0]) or (j + 1 < len(prev) and prev[j + 1][0] == prev[j][0])
                        t["cut_inside_tie_group"] += bool(same)
                        break
                if len(lnodes) >= N or len(lnodes) == prev_size:                 # :990
                    finish = True
                    if len(lnodes) < N:
                        t["finished_by_prev_size"] += 1
        first_pass = False
    out = []
    for n in lnodes:                                                             # :1005
        best = n.keys[0]; max_response = kr[best]                                # :1011-1014
        for k in n.keys[1:]:                                                     # :1017
            if kr[k] > max_response:                                             # :1020  strict: the first of equals stays
                best = k; max_response = kr[k]
        t["response_tie_in_node"] += sum(1 for k in n.keys if kr[k] == max_response) > 1
        out.append(best)
    return out, +t


# ---------------------------------------------------------------------------------------------------------------- per level, epilogue
def level_keypoints(keys, selected, level, sf):
    """:1161-1176: the selected keys of one level as records of KEY_FIELDS."""
    size = int(F(F(PATCH_SIZE) * F(sf[level])))                                  # :1161
    out = []
    for k in selected:
        out.append((F(F(keys[k][0]) + F(BORDER)), F(F(keys[k][1]) + F(BORDER)), F(size), F(keys[k][2]), level, -1))   # :1170-1175
    return out


def assemble(levels, lapping, sf):
    """operator()'s epilogue (:1587-1658).  levels: per level the list level_keypoints returned.
    Returns (perm, fields, mono): output slot s holds keypoint perm[s] of the level-by-level concatenation; fields is a list of
    KEY_FIELDS tuples per slot; mono is the returned monoIndex."""
    n = sum(len(l) for l in levels)                                              # :1566-1567
    perm = [None] * n; fields = [None] * n
    mono, stereo = 0, n - 1                                                      # :1592
    g = 0
    for level, kps in enumerate(levels):                                         # :1593
        scale = F(sf[level])                                                     # :1633
        for x, y, size, resp, octave, cid in kps:                                # :1635
            if level != 0:                                                       # :1639
                x = F(F(x) * scale); y = F(F(y) * scale)                         # :1641
            if x >= F(lapping[0]) and x <= F(lapping[1]):                        # :1644
                perm[stereo] = g; fields[stereo] = (x, y, size, resp, octave, cid); stereo -= 1
            else:
                perm[mono] = g; fields[mono] = (x, y, size, resp, octave, cid); mono += 1
            g += 1
    return perm, fields, mono                                                    # :1658


def extract(level_images, nfeatures, scale_factor, ini_th, min_th, lapping, tie="newest"):
    """ComputeKeyPointsOctTree + the epilogue over given level images.  Returns a dict, per level: candidates ((n, 3) of pt.x, pt.y,
    response relative to the 16-px border), selected (indices into them in the quadtree's output order), level_keypoints ((n, 3) of
    the selected keys in level coordinates, border added); for the frame: perm, fields, mono, counters (summed), budget."""
    nlevels = len(level_images)
    sf = scale_factors(scale_factor, nlevels)[0]
    budget = features_per_level(nfeatures, scale_factor, nlevels)
    total = Counter()
    cands, sel, levels, lxy = [], [], [], []
    for l, img in enumerate(level_images):
        rows, cols = img.shape
        keys = cell_keys(img, ini_th, min_th, total)
        idx, t = distribute_oct_tree(keys, BORDER, cols - BORDER, BORDER, rows - BORDER, budget[l], tie)    # :1153-1158
        total.update(t)
        cands.append(keys); sel.append(idx)
        levels.append(level_keypoints(keys, idx, l, sf))
        lxy.append(np.array([(int(k[0]), int(k[1]), int(k[3])) for k in levels[-1]], np.int64).reshape(-1, 3))
    perm, fields, mono = assemble(levels, lapping, sf)
    return dict(candidates=cands, selected=sel, level_keypoints=lxy, perm=perm, fields=fields, mono=mono, counters=total, budget=budget)


def fields_array(fields):
    """The KEY_FIELDS tuples as a structured array (float32 x 4, int32 x 2) for bitwise comparison."""
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
    return np.array([tuple(f) for f in fields], dt) if fields else np.zeros(0, dt)
