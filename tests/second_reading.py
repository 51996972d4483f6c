"""A second, independent reading of the reference's matcher searches, in plain Python / numpy.

Written from the reference's ORBmatcher.cc, Frame.cc, KeyFrame.cc, Tracking.cc and CameraModels/Pinhole.cpp alone: it shares no
code with the CPU oracle, the host claim replays or the device kernels, and it imports none of them.  One reference function is
one function here and cites the lines it restates.  The functions work on the flattened arrays of the C ABI (keypoint records
with x / y / angle / octave fields, 32-byte descriptor rows, uright, the grid parameters and the per-query arrays after
projection), so a test can hand the same arrays to the oracle, to a device entry point and to this file.

Arithmetic follows the C++ operand types: every float operation is one np.float32 operation (no contraction), a float compared
with a double literal is promoted, float * int is a float product, round is C's (half away from zero), (int)floor / ceil as
written.  Every search also returns a collections.Counter of the branches it took, so that a test can prove that a constructed
scene reached the case it was built for.
"""
import math
from collections import Counter

import numpy as np

F = np.float32

TH_HIGH = 100        # ORBmatcher.cc:36
TH_LOW = 50          # ORBmatcher.cc:37
HISTO_LENGTH = 30    # ORBmatcher.cc:38
GRID_COLS = 64       # Frame.h:37
GRID_ROWS = 48       # Frame.h:38

NO_MATCH = -1        # slot never assigned
PRUNED = -2          # slot assigned and then set to NULL by the rotation cull (M4, M5: the row of an EXISTING mvpMapPoints)


def c_round(x):
    """C round(): to nearest, halves away from zero.  The argument is a float32 promoted to double, so x + 0.5 is exact."""
    x = float(x)
    return int(math.floor(x + 0.5)) if x >= 0.0 else -int(math.floor(-x + 0.5))


def is_half_way(x):
    x = float(x)
    return x - math.floor(x) == 0.5


# ---------------------------------------------------------------------------------------------------------------------------
# ORBmatcher::DescriptorDistance, ORBmatcher.cc:2911-2931
# ---------------------------------------------------------------------------------------------------------------------------
_C1, _C2, _C4, _C24 = np.uint32(1), np.uint32(2), np.uint32(4), np.uint32(24)
_M5, _M3, _MF, _M01 = np.uint32(0x55555555), np.uint32(0x33333333), np.uint32(0xF0F0F0F), np.uint32(0x1010101)


def descriptor_distances(a, rows):
    """Distance of one 32-byte row `a` to each row of `rows`: the 8-word SWAR loop of :2920-2928 on unsigned 32-bit words."""
    pa = np.ascontiguousarray(a, np.uint8).reshape(1, 32).view("<u4")
    pb = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32).view("<u4")
    v = pa ^ pb                                                    # :2922
    v = v - ((v >> _C1) & _M5)                                     # :2925
    v = (v & _M3) + ((v >> _C2) & _M3)                             # :2926
    v = (((v + (v >> _C4)) & _MF) * _M01) >> _C24                  # :2927, the product wraps at 32 bits
    return v.astype(np.int64).sum(axis=1)


def descriptor_distance(a, b):
    return int(descriptor_distances(a, b)[0])


# ---------------------------------------------------------------------------------------------------------------------------
# ORBmatcher::ComputeThreeMaxima, ORBmatcher.cc:2863-2905
# ---------------------------------------------------------------------------------------------------------------------------
def compute_three_maxima(sizes):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1                                        # the callers' initial values (:524-526 and siblings)
    for i in range(len(sizes)):
        s = int(sizes[i])
        if s > max1:                                               # :2872-2880
            max3 = max2; max2 = max1; max1 = s
            ind3 = ind2; ind2 = ind1; ind1 = i
        elif s > max2:                                             # :2881-2887
            max3 = max2; max2 = s
            ind3 = ind2; ind2 = i
        elif s > max3:                                             # :2888-2892
            max3 = s; ind3 = i
    if F(max2) < F(0.1) * F(max1):                                 # :2896, int against a float product
        ind2 = -1; ind3 = -1
    elif F(max3) < F(0.1) * F(max1):                               # :2901
        ind3 = -1
    return ind1, ind2, ind3


FACTOR_360 = F(HISTO_LENGTH) / F(360.0)    # the bin count over a full turn, int / float: ORBmatcher.cc:334, 978, 2480, 2736
FACTOR_INV = F(1.0) / F(HISTO_LENGTH)      # one over the bin count, float / int: ORBmatcher.cc:1441


def rotation_bin(angle_a, angle_b, factor, t):
    """The histogram bin of one match (ORBmatcher.cc:459-464 and its siblings): the angle difference as a float, a negative one (against
    the double zero) moved up by a full turn, scaled by `factor` in float, rounded half away from zero, and the last-plus-one bin
    folded onto bin 0."""
    rot = F(angle_a) - F(angle_b)
    if float(rot) < 0.0:
        rot = rot + F(360.0)
    p = rot * factor
    if is_half_way(p):
        t["half_way_bin"] += 1
    b = c_round(p)
    if b == HISTO_LENGTH:
        b = 0
        t["bin_30_wraps"] += 1
    assert 0 <= b < HISTO_LENGTH
    return b


def _culled_bins(rot_hist, t):
    """The bins whose entries are cleared (ORBmatcher.cc:529-543 and siblings)."""
    ind1, ind2, ind3 = compute_three_maxima([len(h) for h in rot_hist])
    t["bins_kept"] = sum(1 for x in (ind1, ind2, ind3) if x >= 0)
    return [i for i in range(HISTO_LENGTH) if i != ind1 and i != ind2 and i != ind3]


# ---------------------------------------------------------------------------------------------------------------------------
# Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:446-480, 883-899) and the two GetFeaturesInArea
# ---------------------------------------------------------------------------------------------------------------------------
class GridFrame:
    """The fields of a Frame / KeyFrame the searches read, with the grid built as the reference builds it."""

    def __init__(self, kps, desc, min_x, min_y, inv_w, inv_h, uright=None):
        self.n = len(kps)
        self.x = np.ascontiguousarray(kps["x"], np.float32)
        self.y = np.ascontiguousarray(kps["y"], np.float32)
        self.angle = np.ascontiguousarray(kps["angle"], np.float32)
        self.octave = np.ascontiguousarray(kps["octave"], np.int64)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.uright = None if uright is None else np.ascontiguousarray(uright, np.float32)
        self.min_x, self.min_y, self.inv_w, self.inv_h = F(min_x), F(min_y), F(inv_w), F(inv_h)
        self.trace = Counter()
        self.grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
        self.placed = 0
        for i in range(self.n):                                    # Frame.cc:464-479
            ok, px, py = self.pos_in_grid(self.x[i], self.y[i])
            if ok:
                self.grid[px][py].append(i)
                self.placed += 1
            else:
                self.trace["not_placed"] += 1

    def pos_in_grid(self, x, y):
        gx = (F(x) - self.min_x) * self.inv_w                      # Frame.cc:888
        gy = (F(y) - self.min_y) * self.inv_h                      # Frame.cc:889
        px, py = c_round(gx), c_round(gy)
        if is_half_way(gx) or is_half_way(gy):
            self.trace["half_way_cell"] += 1
        if px == GRID_COLS or py == GRID_ROWS:
            self.trace["rounded_onto_edge"] += 1
        if px < 0 or px >= GRID_COLS or py < 0 or py >= GRID_ROWS:  # Frame.cc:894
            return False, px, py
        return True, px, py

    def csr(self):
        """The grid as CSR with cell = ix * 48 + iy, entries in insertion order (the layout of the C ABI's frame view)."""
        start = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int32); idx = []
        for ix in range(GRID_COLS):
            for iy in range(GRID_ROWS):
                idx.extend(self.grid[ix][iy])
                start[ix * GRID_ROWS + iy + 1] = len(idx)
        return start, np.array(idx, np.int32)

    def _cells(self, x, y, r, t):
        x, y, r = F(x), F(y), F(r)
        lo_x = max(0, int(math.floor(float((x - self.min_x - r) * self.inv_w))))                 # Frame.cc:800
        if lo_x >= GRID_COLS:
            t["window_outside_grid"] += 1
            return None
        hi_x = min(GRID_COLS - 1, int(math.ceil(float((x - self.min_x + r) * self.inv_w))))       # Frame.cc:807
        if hi_x < 0:
            t["window_outside_grid"] += 1
            return None
        lo_y = max(0, int(math.floor(float((y - self.min_y - r) * self.inv_h))))                 # Frame.cc:814
        if lo_y >= GRID_ROWS:
            t["window_outside_grid"] += 1
            return None
        hi_y = min(GRID_ROWS - 1, int(math.ceil(float((y - self.min_y + r) * self.inv_h))))       # Frame.cc:820
        if hi_y < 0:
            t["window_outside_grid"] += 1
            return None
        if (float((x - self.min_x - r) * self.inv_w) < 0 or float((x - self.min_x + r) * self.inv_w) > GRID_COLS - 1
                or float((y - self.min_y - r) * self.inv_h) < 0 or float((y - self.min_y + r) * self.inv_h) > GRID_ROWS - 1):
            t["window_clipped"] += 1
        return lo_x, hi_x, lo_y, hi_y

    def _in_box(self, cand, x, y, r, t):
        if not cand:
            return []
        c = np.array(cand, np.int64)
        dx = np.abs(self.x[c] - F(x)); dy = np.abs(self.y[c] - F(y))                               # Frame.cc:860-861
        t["exactly_r_away"] += int(np.count_nonzero(((dx == F(r)) & (dy <= F(r))) | ((dy == F(r)) & (dx <= F(r)))))
        keep = (dx < F(r)) & (dy < F(r))                                                          # Frame.cc:864, strict
        return c[keep].tolist()

    def features_in_area(self, x, y, r, min_level=-1, max_level=-1, t=None):
        """Frame::GetFeaturesInArea, Frame.cc:784-871 (left camera)."""
        t = self.trace if t is None else t
        cells = self._cells(x, y, r, t)
        if cells is None:
            return []
        lo_x, hi_x, lo_y, hi_y = cells
        check_levels = (min_level > 0) or (max_level >= 0)                                        # Frame.cc:828
        if min_level == 0 and max_level < 0:
            t["levels_unchecked_min0"] += 1
        if min_level < 0 and max_level >= 0:
            t["levels_checked_min_negative"] += 1
        cand = []
        for ix in range(lo_x, hi_x + 1):                                                          # Frame.cc:831
            for iy in range(lo_y, hi_y + 1):                                                      # Frame.cc:833
                for j in self.grid[ix][iy]:
                    if check_levels:
                        if self.octave[j] < min_level:                                            # Frame.cc:852
                            continue
                        if max_level >= 0:
                            if self.octave[j] > max_level:                                        # Frame.cc:854-856
                                continue
                    cand.append(j)
        return self._in_box(cand, x, y, r, t)

    def kf_features_in_area(self, x, y, r, t=None):
        """KeyFrame::GetFeaturesInArea, KeyFrame.cc:916-962 (no level test)."""
        t = self.trace if t is None else t
        cells = self._cells(x, y, r, t)                                                           # KeyFrame.cc:924-939
        if cells is None:
            return []
        lo_x, hi_x, lo_y, hi_y = cells
        cand = []
        for ix in range(lo_x, hi_x + 1):
            for iy in range(lo_y, hi_y + 1):
                cand.extend(self.grid[ix][iy])
        return self._in_box(cand, x, y, r, t)                                                     # KeyFrame.cc:952-956


def _on_threshold(t, d, th, name):
    if d == th:
        t["dist_on_" + name] += 1
    if d == th + 1:
        t["dist_on_" + name + "_plus_1"] += 1


# ---------------------------------------------------------------------------------------------------------------------------
# M3  ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints), ORBmatcher.cc:45-166
# ---------------------------------------------------------------------------------------------------------------------------
def radius_by_viewing_cos(view_cos):
    """ORBmatcher.cc:242-249: the float is compared with the double 0.998."""
    return F(2.5) if float(F(view_cos)) > 0.998 else F(4.0)


def search_by_projection_points(fr, blocked, scale_factors, in_view, px, py, pxr, view_cos, level, qdesc, mp_obs, th, nnratio,
                                depth=None, th_far=None):
    """match[idx] = index of the MapPoint in F.mvpMapPoints[idx] at the end, or -1 for a slot the search did not write."""
    t = Counter()
    th, nnratio = F(th), F(nnratio)
    sf = np.asarray(scale_factors, np.float32)
    qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    match = np.full(fr.n, NO_MATCH, np.int32)
    has_obs = np.array(blocked, bool).copy()        # the slot holds a MapPoint that has observations (:102-104)
    nmatches = 0
    b_factor = float(th) != 1.0                                                                   # :50
    for i in range(len(in_view)):
        if not in_view[i]:                                                                        # :56
            continue
        if depth is not None and F(depth[i]) > F(th_far):                                         # :59
            t["far_point"] += 1
            continue
        lvl = int(level[i])                                                                       # :68
        r = radius_by_viewing_cos(view_cos[i])                                                    # :72
        if b_factor:
            r = r * th                                                                            # :75-76
        rs = r * sf[lvl]
        cand = fr.features_in_area(px[i], py[i], rs, lvl - 1, lvl, t)                             # :79-82
        if not cand:                                                                              # :85
            t["empty_window"] += 1
            continue
        dists = descriptor_distances(qdesc[i], fr.desc[cand])
        best, best_lvl, best2, best_lvl2, best_idx = 256, -1, 256, -1, -1                         # :89-93
        seen, tie_lower = 0, False
        for idx, dist in zip(cand, dists.tolist()):
            if has_obs[idx]:                                                                      # :102-104
                continue
            if fr.uright is not None and float(fr.uright[idx]) > 0:                               # :107
                t["stereo_gate_applied"] += 1
                er = abs(F(pxr[i]) - fr.uright[idx])                                              # :110
                if er > r * sf[lvl]:                                                              # :115
                    t["stereo_gate_rejected"] += 1
                    continue
            elif fr.uright is not None:
                t["stereo_gate_skipped"] += 1
            seen += 1
            tie_lower = (tie_lower and dist >= best) or (dist == best and idx < best_idx)
            if dist < best:                                                                       # :125-134
                best2 = best; best = dist
                best_lvl2 = best_lvl; best_lvl = int(fr.octave[idx])
                best_idx = idx
            elif dist < best2:                                                                    # :135-141
                best_lvl2 = int(fr.octave[idx]); best2 = dist
        if seen == 0:
            t["all_candidates_blocked"] += 1
        _on_threshold(t, best, TH_HIGH, "th_high")
        if best <= TH_HIGH:                                                                       # :147
            prod = nnratio * F(best2)                                                             # the ratio member times the int runner-up: a float product
            if F(best) == prod:
                t["ratio_exactly_equal"] += 1
            if best_lvl == best_lvl2 and F(best) > prod:                                          # :151-152
                t["ratio_rejected"] += 1
                continue
            if best_lvl != best_lvl2 or F(best) <= prod:                                          # :154
                if best_lvl != best_lvl2:
                    t["accepted_levels_differ"] += 1
                    if F(best) > prod:
                        t["ratio_bypassed_by_level"] += 1
                else:
                    t["accepted_same_level"] += 1
                if match[best_idx] >= 0:
                    t["overwrote_unobserved"] += 1
                t["tie_kept_first_not_lowest_index"] += int(tie_lower)
                match[best_idx] = i                                                               # :155
                has_obs[best_idx] = bool(mp_obs[i])
                nmatches += 1                                                                     # :163
    return nmatches, match, t


# ---------------------------------------------------------------------------------------------------------------------------
# M4  ORBmatcher::SearchByProjection(Frame& Cur, const Frame& Last, th, bMono), ORBmatcher.cc:2527-2612, 2686-2708 (Nleft == -1)
# ---------------------------------------------------------------------------------------------------------------------------
def search_by_projection_frame(fr, cur_blocked, scale_factors, valid, u, v, invzc, octave, angle, qdesc, mp_obs, th,
                               forward=False, backward=False, mbf=0.0, check_ori=True):
    """match[i2] = last-frame index in Cur.mvpMapPoints[i2], -1 untouched, -2 set to NULL by the rotation check."""
    t = Counter()
    th, mbf = F(th), F(mbf)
    sf = np.asarray(scale_factors, np.float32)
    qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    match = np.full(fr.n, NO_MATCH, np.int32)
    has_obs = np.array(cur_blocked, bool).copy() if cur_blocked is not None else np.zeros(fr.n, bool)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i in range(len(valid)):
        if not valid[i]:                                                                          # :2507-2528, the caller's gates
            continue
        o = int(octave[i])                                                                        # :2530
        radius = th * sf[o]                                                                       # :2535
        if forward:
            cand = fr.features_in_area(u[i], v[i], radius, o, -1, t)                              # :2545
            t["forward_band"] += 1
        elif backward:
            cand = fr.features_in_area(u[i], v[i], radius, 0, o, t)                               # :2547
            t["backward_band"] += 1
        else:
            cand = fr.features_in_area(u[i], v[i], radius, o - 1, o + 1, t)                       # :2549
        if not cand:                                                                              # :2551
            t["empty_window"] += 1
            continue
        dists = descriptor_distances(qdesc[i], fr.desc[cand])
        best, best_idx, seen, tie_lower = 256, -1, 0, False                                       # :2556-2557
        for i2, dist in zip(cand, dists.tolist()):
            if has_obs[i2]:                                                                       # :2565-2567
                continue
            if fr.uright is not None and float(fr.uright[i2]) > 0:                                # :2569
                t["stereo_gate_applied"] += 1
                ur = F(u[i]) - mbf * F(invzc[i])                                                  # :2572
                er = abs(ur - fr.uright[i2])                                                      # :2573
                if er > radius:                                                                   # :2574
                    t["stereo_gate_rejected"] += 1
                    continue
            elif fr.uright is not None:
                t["stereo_gate_skipped"] += 1
            seen += 1
            tie_lower = (tie_lower and dist >= best) or (dist == best and i2 < best_idx)
            if dist < best:                                                                       # :2582-2586
                best = dist; best_idx = i2
        if seen == 0:
            t["all_candidates_blocked"] += 1
        _on_threshold(t, best, TH_HIGH, "th_high")
        if best <= TH_HIGH:                                                                       # :2590
            if match[best_idx] >= 0:
                t["overwrote_unobserved"] += 1
            t["tie_kept_first_not_lowest_index"] += int(tie_lower)
            match[best_idx] = i                                                                   # :2592
            has_obs[best_idx] = bool(mp_obs[i])
            nmatches += 1
            if check_ori:                                                                         # :2596-2613
                rot_hist[rotation_bin(angle[i], fr.angle[best_idx], FACTOR_360, t)].append(best_idx)
    if check_ori:                                                                                 # :2688-2708
        occurrences = Counter(s for h in rot_hist for s in h)
        t["slots_in_histogram_twice"] = sum(1 for c in occurrences.values() if c > 1)
        culled = _culled_bins(rot_hist, t)
        seen_slots = set()
        for b in culled:
            for s in rot_hist[b]:
                if s in seen_slots:
                    t["slot_culled_twice"] += 1
                seen_slots.add(s)
                match[s] = PRUNED                                                                 # :2703
                nmatches -= 1                                                                     # :2704
                t["culled_entries"] += 1
        t["twice_in_histogram_and_culled"] = sum(1 for s in seen_slots if occurrences[s] > 1)
    return nmatches, match, t


def search_by_projection_frame_with_retry(fr, cur_blocked, scale_factors, valid, u, v, invzc, octave, angle, qdesc, mp_obs, th,
                                          forward=False, backward=False, mbf=0.0, check_ori=True, retry_below=20):
    """Tracking::TrackWithMotionModel's call and its wider second call from an emptied frame, Tracking.cc:3211-3221."""
    n, m, t = search_by_projection_frame(fr, cur_blocked, scale_factors, valid, u, v, invzc, octave, angle, qdesc, mp_obs, th,
                                         forward, backward, mbf, check_ori)
    retried = False
    if n < retry_below:                                                                           # Tracking.cc:3215
        n, m, t = search_by_projection_frame(fr, None, scale_factors, valid, u, v, invzc, octave, angle, qdesc, mp_obs,
                                             F(2) * F(th), forward, backward, mbf, check_ori)     # Tracking.cc:3218-3220
        retried = True
    return n, m, t, retried


# ---------------------------------------------------------------------------------------------------------------------------
# M5  ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist), ORBmatcher.cc:2723-2852
# ---------------------------------------------------------------------------------------------------------------------------
def search_by_projection_kf(fr, blocked, scale_factors, valid, u, v, level, angle, qdesc, th, orb_dist, check_ori=True):
    t = Counter()
    th = F(th); orb_dist = int(orb_dist)
    sf = np.asarray(scale_factors, np.float32)
    qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    match = np.full(fr.n, NO_MATCH, np.int32)
    held = np.array(blocked, bool).copy() if blocked is not None else np.zeros(fr.n, bool)   # the slot of the current frame holds a MapPoint (:2793)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i in range(len(valid)):
        if not valid[i]:                                                                          # :2745-2770, the caller's gates
            continue
        lvl = int(level[i])                                                                       # :2773
        radius = th * sf[lvl]                                                                     # :2777
        cand = fr.features_in_area(u[i], v[i], radius, lvl - 1, lvl + 1, t)                       # :2780
        if not cand:                                                                              # :2782
            t["empty_window"] += 1
            continue
        dists = descriptor_distances(qdesc[i], fr.desc[cand])
        best, best_idx, seen, tie_lower = 256, -1, 0, False
        for i2, dist in zip(cand, dists.tolist()):
            if held[i2]:                                                                          # :2793-2794
                continue
            seen += 1
            tie_lower = (tie_lower and dist >= best) or (dist == best and i2 < best_idx)
            if dist < best:                                                                       # :2800-2804
                best = dist; best_idx = i2
        if seen == 0:
            t["all_candidates_blocked"] += 1
        _on_threshold(t, best, orb_dist, "orb_dist")
        if best <= orb_dist:                                                                      # :2807
            t["tie_kept_first_not_lowest_index"] += int(tie_lower)
            match[best_idx] = i                                                                   # :2809
            held[best_idx] = True
            t["claims"] += 1
            nmatches += 1
            if check_ori:                                                                         # :2812-2822
                rot_hist[rotation_bin(angle[i], fr.angle[best_idx], FACTOR_360, t)].append(best_idx)
    if check_ori:                                                                                 # :2830-2849
        for b in _culled_bins(rot_hist, t):
            for s in rot_hist[b]:
                match[s] = PRUNED                                                                 # :2844
                nmatches -= 1
                t["culled_entries"] += 1
    return nmatches, match, t


# ---------------------------------------------------------------------------------------------------------------------------
# M6  ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th, ratioHamming), ORBmatcher.cc:549-679 after :632
# ---------------------------------------------------------------------------------------------------------------------------
def search_by_projection_sim3(kf, matched_in, scale_factors, valid, u, v, level, qdesc, th, ratio_hamming):
    """match[idx] = iMP for the slots this call wrote into vpMatched, else -1."""
    t = Counter()
    th = int(th); ratio = F(ratio_hamming)
    sf = np.asarray(scale_factors, np.float32)
    qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    match = np.full(kf.n, NO_MATCH, np.int32)
    held = np.array(matched_in, bool).copy() if matched_in is not None else np.zeros(kf.n, bool)   # the slot is already matched (:649)
    bound = F(TH_LOW) * ratio                                                                     # the int threshold times the float ratio: a float product (:670)
    nmatches = 0
    for i in range(len(valid)):
        if not valid[i]:                                                                          # :582-625, the caller's gates
            continue
        lvl = int(level[i])                                                                       # :628
        radius = F(th) * sf[lvl]                                                                  # :632, int * float
        cand = kf.kf_features_in_area(u[i], v[i], radius, t)                                      # :635
        if not cand:                                                                              # :637
            t["empty_window"] += 1
            continue
        dists = descriptor_distances(qdesc[i], kf.desc[cand])
        best, best_idx, seen, tie_lower = 256, -1, 0, False                                       # :643-644
        for idx, dist in zip(cand, dists.tolist()):
            if held[idx]:                                                                         # :649
                continue
            seen += 1
            kl = int(kf.octave[idx])
            if kl < lvl - 1 or kl > lvl:                                                          # :655
                t["level_rejected"] += 1
                continue
            tie_lower = (tie_lower and dist >= best) or (dist == best and idx < best_idx)
            if dist < best:                                                                       # :662-666
                best = dist; best_idx = idx
        if seen == 0:
            t["all_candidates_blocked"] += 1
        if F(best) == bound:
            t["dist_on_bound"] += 1
        if best == math.floor(float(bound)) + 1:
            t["dist_just_above_bound"] += 1
        if F(best) <= bound:                                                                      # :670
            t["tie_kept_first_not_lowest_index"] += int(tie_lower)
            match[best_idx] = i                                                                   # :672
            held[best_idx] = True
            t["claims"] += 1
            nmatches += 1
    return nmatches, match, t


# ---------------------------------------------------------------------------------------------------------------------------
# FeatureVector walk shared by the BoW searches (ORBmatcher.cc:343-347, 505-517; 987-990, 1070-1080; 1448-1450, 1584-1594)
# ---------------------------------------------------------------------------------------------------------------------------
def _common_buckets(fv1, fv2):
    """fv = (nodes ascending, start, idx): a std::map<NodeId, vector<unsigned>> as CSR.  Yields the index lists of equal nodes."""
    n1, s1, x1 = fv1; n2, s2, x2 = fv2
    i = j = 0
    while i < len(n1) and j < len(n2):
        if n1[i] == n2[j]:
            yield x1[s1[i]:s1[i + 1]], x2[s2[j]:s2[j + 1]]
            i += 1; j += 1
        elif n1[i] < n2[j]:
            i = int(np.searchsorted(n1, n2[j], "left"))                                           # lower_bound
        else:
            j = int(np.searchsorted(n2, n1[i], "left"))


# ---------------------------------------------------------------------------------------------------------------------------
# M7  ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches), ORBmatcher.cc:314-547 (F.Nleft == -1)
# ---------------------------------------------------------------------------------------------------------------------------
def search_by_bow(kps_kf, desc_kf, kf_good, fv_kf, kps_f, desc_f, fv_f, nnratio, check_ori=True):
    """f_match[iF] = KeyFrame feature whose MapPoint sits in vpMapPointMatches[iF], or -1 (NULL)."""
    t = Counter()
    nnratio = F(nnratio)
    desc_kf = np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32); desc_f = np.ascontiguousarray(desc_f, np.uint8).reshape(-1, 32)
    f_match = np.full(len(kps_f), NO_MATCH, np.int32)                                             # :320
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for ikf, iff in _common_buckets(fv_kf, fv_f):
        iff = np.asarray(iff, np.int64)
        for real_kf in ikf:                                                                       # :354
            real_kf = int(real_kf)
            if not kf_good[real_kf]:                                                              # :362-366
                continue
            dists = descriptor_distances(desc_kf[real_kf], desc_f[iff]).tolist() if len(iff) else []
            best1, best_idx, best2 = 256, -1, 256                                                 # :370-372
            for real_f, dist in zip(iff.tolist(), dists):                                         # :378
                if f_match[real_f] >= 0:                                                          # :385
                    continue
                if dist < best1:                                                                  # :394-399
                    best2 = best1; best1 = dist; best_idx = real_f
                elif dist < best2:                                                                # :401-404
                    if dist == best1:
                        t["runner_up_equals_best"] += 1
                    best2 = dist
            _on_threshold(t, best1, TH_LOW, "th_low")
            if best1 <= TH_LOW:                                                                   # :438
                if F(best1) < nnratio * F(best2):                                                 # :441
                    if best1 == TH_LOW:
                        t["accepted_on_th_low"] += 1
                    f_match[best_idx] = real_kf                                                   # :444
                    if check_ori:                                                                 # :452-467
                        rot_hist[rotation_bin(kps_kf["angle"][real_kf], kps_f["angle"][best_idx], FACTOR_360, t)].append(best_idx)
                    nmatches += 1
                else:
                    t["ratio_rejected"] += 1
    if check_ori:                                                                                 # :521-544
        for b in _culled_bins(rot_hist, t):
            for s in rot_hist[b]:
                f_match[s] = NO_MATCH                                                             # :540
                nmatches -= 1
                t["culled_entries"] += 1
    return nmatches, f_match, t


# ---------------------------------------------------------------------------------------------------------------------------
# M8  ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12), ORBmatcher.cc:955-1105 (NLeft == -1)
# ---------------------------------------------------------------------------------------------------------------------------
def search_by_bow_kf(kps1, desc1, good1, fv1, kps2, desc2, good2, fv2, nnratio, check_ori=True):
    """matches12[idx1] = idx2 or -1."""
    t = Counter()
    nnratio = F(nnratio)
    desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    m12 = np.full(len(kps1), NO_MATCH, np.int32)                                                  # :969
    matched2 = np.zeros(len(kps2), bool)                                                          # :970
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for b1, b2 in _common_buckets(fv1, fv2):
        b2 = np.asarray(b2, np.int64)
        for idx1 in b1:                                                                           # :993
            idx1 = int(idx1)
            if not good1[idx1]:                                                                   # :1000-1004
                continue
            dists = descriptor_distances(desc1[idx1], desc2[b2]).tolist() if len(b2) else []
            best1, best_idx2, best2 = 256, -1, 256                                                # :1008-1010
            for idx2, dist in zip(b2.tolist(), dists):                                            # :1013
                if matched2[idx2] or not good2[idx2]:                                             # :1024-1028
                    if matched2[idx2]:
                        t["skipped_claimed_side2"] += 1
                    continue
                if dist < best1:                                                                  # :1034-1039
                    best2 = best1; best1 = dist; best_idx2 = idx2
                elif dist < best2:                                                                # :1040-1043
                    if dist == best1:
                        t["runner_up_equals_best"] += 1
                    best2 = dist
            _on_threshold(t, best1, TH_LOW, "th_low")
            if best1 < TH_LOW:                                                                    # :1047, strict
                if F(best1) < nnratio * F(best2):                                                 # :1049
                    m12[idx1] = best_idx2                                                         # :1051
                    matched2[best_idx2] = True                                                    # :1052
                    if check_ori:                                                                 # :1054-1064
                        rot_hist[rotation_bin(kps1["angle"][idx1], kps2["angle"][best_idx2], FACTOR_360, t)].append(idx1)
                    nmatches += 1
                else:
                    t["ratio_rejected"] += 1
            elif best1 == TH_LOW:
                t["rejected_on_th_low"] += 1
    if check_ori:                                                                                 # :1084-1102
        for b in _culled_bins(rot_hist, t):
            for s in rot_hist[b]:
                m12[s] = NO_MATCH                                                                 # :1098
                nmatches -= 1
                t["culled_entries"] += 1
    return nmatches, m12, t


# ---------------------------------------------------------------------------------------------------------------------------
# M10 ORBmatcher::SearchForTriangulation_, ORBmatcher.cc:1388-1629, pinhole, no second camera
# ---------------------------------------------------------------------------------------------------------------------------
def epipolar_constrain(x1, y1, x2, y2, f12, unc, t):
    """Pinhole::epipolarConstrain_ after F12 is built, Pinhole.cpp:282-295.  f12: 3x3 row-major float32."""
    x1, y1, x2, y2 = F(x1), F(y1), F(x2), F(y2)
    a = x1 * f12[0, 0] + y1 * f12[1, 0] + f12[2, 0]                                               # :282
    b = x1 * f12[0, 1] + y1 * f12[1, 1] + f12[2, 1]                                               # :283
    c = x1 * f12[0, 2] + y1 * f12[1, 2] + f12[2, 2]                                               # :284
    num = a * x2 + b * y2 + c                                                                     # :286
    den = a * a + b * b                                                                           # :288
    if den == 0:                                                                                  # :290
        t["den_zero"] += 1
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        dsqr = num * num / den                                                                    # :293
    ok = float(dsqr) < 3.84 * float(F(unc))                                                       # :295, a double product
    if ok != bool(dsqr < F(3.84) * F(unc)):
        t["double_product_decides"] += 1
    t["epipolar_pass" if ok else "epipolar_fail"] += 1
    return ok


def search_for_triangulation(kps1, desc1, has_mp1, ur1, fv1, kps2, desc2, has_mp2, ur2, fv2, f12, ep, sf2, sigma2_2,
                             only_stereo=False, coarse=False, check_ori=False):
    """matches12[idx1] = idx2 or -1 (vMatches12 at :1621, before it is packed into pairs); returns nmatches (:1628)."""
    t = Counter()
    desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    f12 = np.ascontiguousarray(f12, np.float32).reshape(3, 3)
    epx, epy = F(ep[0]), F(ep[1])
    sf2 = np.asarray(sf2, np.float32); sigma2_2 = np.asarray(sigma2_2, np.float32)
    m12 = np.full(len(kps1), NO_MATCH, np.int32)                                                  # :1435
    claimed2 = Counter()
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for b1, b2 in _common_buckets(fv1, fv2):
        b2 = np.asarray(b2, np.int64)
        for idx1 in b1:                                                                           # :1452
            idx1 = int(idx1)
            if has_mp1[idx1]:                                                                     # :1456-1462
                continue
            stereo1 = ur1 is not None and float(F(ur1[idx1])) >= 0                                # :1464
            if only_stereo and not stereo1:                                                       # :1466-1468
                t["only_stereo_skipped"] += 1
                continue
            dists = descriptor_distances(desc1[idx1], desc2[b2]).tolist() if len(b2) else []
            best, best_idx2 = TH_LOW, -1                                                          # :1480-1481
            for idx2, dist in zip(b2.tolist(), dists):                                            # :1483
                if has_mp2[idx2]:                                                                 # :1487-1491; vbMatched2 is never set
                    continue
                stereo2 = ur2 is not None and float(F(ur2[idx2])) >= 0                            # :1493
                if only_stereo and not stereo2:                                                   # :1495-1497
                    t["only_stereo_skipped"] += 1
                    continue
                if dist > TH_LOW or dist > best:                                                  # :1503
                    continue
                if dist == TH_LOW:
                    t["dist_on_th_low"] += 1
                o2 = int(kps2["octave"][idx2])
                if not stereo1 and not stereo2:                                                   # :1512
                    t["epipole_gate_applied"] += 1
                    ex = epx - F(kps2["x"][idx2]); ey = epy - F(kps2["y"][idx2])                  # :1514-1515
                    if ex * ex + ey * ey < F(100) * sf2[o2]:                                      # :1516, int * float
                        t["epipole_gate_rejected"] += 1
                        continue
                else:
                    t["epipole_gate_skipped_stereo"] += 1
                ok = epipolar_constrain(kps1["x"][idx1], kps1["y"][idx1], kps2["x"][idx2], kps2["y"][idx2], f12, sigma2_2[o2], t)
                if ok or coarse:                                                                  # :1555
                    if not ok:
                        t["coarse_accepted"] += 1
                    if best_idx2 >= 0 and dist == best:
                        t["tie_goes_to_later"] += 1
                    best_idx2 = idx2; best = dist                                                 # :1557-1558
            if best_idx2 >= 0:                                                                    # :1562
                m12[idx1] = best_idx2                                                             # :1567
                claimed2[best_idx2] += 1
                nmatches += 1
                if check_ori:                                                                     # :1570-1580
                    rot_hist[rotation_bin(kps1["angle"][idx1], kps2["angle"][best_idx2], FACTOR_INV, t)].append(idx1)
    t["idx2_shared"] = sum(1 for c in claimed2.values() if c > 1)
    if check_ori:                                                                                 # :1597-1616
        for b in _culled_bins(rot_hist, t):
            for s in rot_hist[b]:
                m12[s] = NO_MATCH                                                                 # :1611
                nmatches -= 1
                t["culled_entries"] += 1
    return nmatches, m12, t


# ---------------------------------------------------------------------------------------------------------------------------
# M13 search core of ORBmatcher::Fuse: ORBmatcher.cc:1934-2010 (chi2 test) and :2131-2166 (Sim3 variant, none)
# ---------------------------------------------------------------------------------------------------------------------------
def fuse(kf, scale_factors, inv_sigma2, valid, u, v, ur, level, qdesc, th, chi2_gate=True):
    """best_idx[i] = KeyFrame feature MapPoint i fuses into, or -1; returns nFused."""
    t = Counter()
    th = F(th)
    sf = np.asarray(scale_factors, np.float32)
    isg = None if inv_sigma2 is None else np.asarray(inv_sigma2, np.float32)
    qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    best_out = np.full(len(valid), NO_MATCH, np.int32)
    nfused = 0
    for i in range(len(valid)):
        if not valid[i]:                                                                          # :1861-1928 / :2083-2124
            continue
        lvl = int(level[i])                                                                       # :1930 / :2127
        radius = th * sf[lvl]                                                                     # :1934 / :2131
        cand = kf.kf_features_in_area(u[i], v[i], radius, t)                                      # :1936 / :2134
        if not cand:                                                                              # :1938 / :2136
            t["empty_window"] += 1
            continue
        dists = descriptor_distances(qdesc[i], kf.desc[cand])
        best, best_idx, tie_lower = 256, -1, False                                                # :1948 (INT_MAX at :2143)
        for idx, dist in zip(cand, dists.tolist()):
            kl = int(kf.octave[idx])
            if kl < lvl - 1 or kl > lvl:                                                          # :1959 / :2150
                t["level_rejected"] += 1
                continue
            if chi2_gate:
                ex = F(u[i]) - kf.x[idx]; ey = F(v[i]) - kf.y[idx]                                # :1970-1971 / :1985-1986
                if kf.uright is not None and float(kf.uright[idx]) >= 0:                          # :1963
                    er = F(ur[i]) - kf.uright[idx]                                                # :1973
                    e2 = ex * ex + ey * ey + er * er                                              # :1974
                    t["chi2_stereo"] += 1
                    if float(e2 * isg[kl]) > 7.8:                                                 # :1977
                        t["chi2_rejected"] += 1
                        continue
                else:
                    e2 = ex * ex + ey * ey                                                        # :1987
                    t["chi2_mono"] += 1
                    if float(e2 * isg[kl]) > 5.99:                                                # :1990
                        t["chi2_rejected"] += 1
                        continue
            tie_lower = (tie_lower and dist >= best) or (dist == best and idx < best_idx)
            if dist < best:                                                                       # :2000-2004 / :2157-2161
                best = dist; best_idx = idx
            elif dist == best:
                t["tie_kept_first"] += 1
        _on_threshold(t, best, TH_LOW, "th_low")
        if best <= TH_LOW:                                                                        # :2010 / :2166
            t["tie_kept_first_not_lowest_index"] += int(tie_lower)
            best_out[i] = best_idx
            nfused += 1
    return nfused, best_out, t
