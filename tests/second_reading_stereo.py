"""A second, independent reading of Frame::ComputeStereoMatches, in plain Python / numpy.

Written from the reference's Frame.cc:1027-1276 and ORBmatcher::DescriptorDistance (ORBmatcher.cc:2911-2931, through
second_reading.descriptor_distances) alone: it imports no product code and no oracle.  The function is scalar on purpose -- one
keypoint, one line of the reference at a time -- and cites the lines it restates.  The un-blurred pyramid levels
(mvImagePyramid of the two extractors) and the scale tables are data and are handed in.

Arithmetic follows the C++ operand types: every float operation is one np.float32 operation (no contraction), a float compared with an
int is compared as float, float +/- int is a float sum, round is C's (half away from zero), (int)floor / ceil as written, the two
`0.01` lines (:1245-1246) are done in double and then narrowed, `1.5f*1.4f*median` (:1263) is a float product from left to right.

Where the reference is undefined, this reading does what include/orbm.h and the oracle state:
  * :1077 indexes vRowIndices with every row of a right keypoint's band, unchecked: rows outside [0, nRows) are dropped.
  * :1262 indexes an empty vDistIdx when no left keypoint got a match: the result is then kept = 0.
The slide itself (:1191-1207) takes columns scaleduR0 - 10 .. scaleduR0 + 10 of the right level, while :1187 only tests
scaleduR0 >= 0 on the left side: for scaleduR0 < 10 the reference's colRange leaves the Mat (cv::Mat asserts).  Such a shift has no
defined SAD; the reading sums the columns that exist (a lower bound), counts `slide_left_of_level`, and ASSERTS that the outcome
cannot depend on the missing pixels -- the winner is a complete shift whose SAD is below every lower bound, and the parabola reads
complete shifts only.

Preconditions (asserted, the device kernels do not range-check them): (int)vL of every left keypoint is a row of the image, and the
11 x 11 window of a left keypoint that reaches the SAD stage lies inside its pyramid level.
"""
import math
from collections import Counter

import numpy as np

from second_reading import F, c_round, descriptor_distances

TH_HIGH = 100        # ORBmatcher.cc:36
TH_LOW = 50          # ORBmatcher.cc:37

# every branch compute_stereo_matches names; tests/test_second_reading_stereo_cpu.py wants each reached, `deltaR_gate` never
BRANCHES = ("empty_row_list", "maxU_negative", "octave_band_reject", "u_range_reject", "distance_tie", "bestDist_ge_thOrbDist",
            "iniu_negative", "endu_ge_cols", "sad_tie_between_shifts", "bestincR_at_minus_L", "bestincR_at_plus_L", "deltaR_gate",
            "disparity_negative", "disparity_ge_maxD", "clamp", "cut", "kept")
# further counters mark an edge that was hit exactly: row_outside_image_dropped, empty_vDistIdx, iniu_zero, endu_cols_minus_1,
# deltaR_half, slide_left_of_level, uR_on_minU, uR_on_maxU, row_on_minr, row_on_maxr, bestDist_on_thOrbDist_minus_1, candidates_over_64


def compute_stereo_matches(kl, dl, kr, dr, levels_l, levels_r, sf, isf, mb, mbf):
    """Frame.cc:1027-1276.  kl / kr = mvKeys / mvKeysRight (records with x, y, octave), dl / dr = the descriptor rows, levels_* =
    mvImagePyramid of the left / right extractor (2-D uint8), sf / isf = mvScaleFactors / mvInvScaleFactors.
    Returns (kept, mvuRight, mvDepth, sad, branches)."""
    N, Nr = len(kl), len(kr)
    t = Counter()
    mb, mbf = F(mb), F(mbf)
    dl = np.ascontiguousarray(dl, np.uint8).reshape(-1, 32); dr = np.ascontiguousarray(dr, np.uint8).reshape(-1, 32)
    uright = np.full(N, -1, F)                                               # :1044
    depth = np.full(N, -1, F)                                                # :1045
    sad = np.full(N, -1, np.int64)
    th_orb_dist = (TH_HIGH + TH_LOW) // 2                                    # :1048
    n_rows = levels_l[0].shape[0]                                            # :1051
    row_indices = [[] for _ in range(n_rows)]                                # :1056
    band = []
    for iR in range(Nr):                                                     # :1064
        kp_y = F(kr[iR]["y"])                                                # :1068
        r = F(F(2.0) * F(sf[int(kr[iR]["octave"])]))                         # :1071
        maxr = int(math.ceil(F(kp_y + r)))                                   # :1072
        minr = int(math.floor(F(kp_y - r)))                                  # :1073
        band.append((minr, maxr))
        for yi in range(minr, maxr + 1):                                     # :1076
            if 0 <= yi < n_rows:
                row_indices[yi].append(iR)                                   # :1077
            else:
                t["row_outside_image_dropped"] += 1
    min_z = mb                                                               # :1086
    min_d = F(0)                                                             # :1087
    max_d = F(mbf / min_z)                                                   # :1088
    dist_idx = []                                                            # :1092
    with np.errstate(all="ignore"):
        for iL in range(N):                                                  # :1096
            level_l = int(kl[iL]["octave"])                                  # :1099
            v_l = F(kl[iL]["y"]); u_l = F(kl[iL]["x"])                       # :1100-1101
            assert 0 <= float(v_l) < n_rows, ("precondition: (int)vL is no row of the image", iL, float(v_l))
            row = int(v_l)                                                   # :1104, float -> size_t truncates
            candidates = row_indices[row]
            if not candidates:                                               # :1106
                t["empty_row_list"] += 1
                continue
            if len(candidates) > 64:
                t["candidates_over_64"] += 1
            min_u = F(u_l - max_d)                                           # :1109
            max_u = F(u_l - min_d)                                           # :1110
            if max_u < F(0):                                                 # :1113
                t["maxU_negative"] += 1
                continue
            best_dist = TH_HIGH                                              # :1116
            best_idx_r = 0                                                   # :1117
            for iR in candidates:                                            # :1122
                oct_r = int(kr[iR]["octave"])
                if oct_r < level_l - 1 or oct_r > level_l + 1:               # :1128
                    t["octave_band_reject"] += 1
                    continue
                u_r = F(kr[iR]["x"])                                         # :1132
                if u_r >= min_u and u_r <= max_u:                            # :1135
                    if u_r == min_u: t["uR_on_minU"] += 1
                    if u_r == max_u: t["uR_on_maxU"] += 1
                    if row == band[iR][0]: t["row_on_minr"] += 1
                    if row == band[iR][1]: t["row_on_maxr"] += 1
                    dist = int(descriptor_distances(dl[iL], dr[iR])[0])      # :1139
                    if dist < best_dist:                                     # :1142
                        best_dist = dist
                        best_idx_r = iR
                    elif dist == best_dist and best_dist < TH_HIGH:
                        t["distance_tie"] += 1                               # the earlier candidate stays
                else:
                    t["u_range_reject"] += 1
            if not best_dist < th_orb_dist:                                  # :1153
                t["bestDist_ge_thOrbDist"] += 1
                continue
            if best_dist == th_orb_dist - 1:
                t["bestDist_on_thOrbDist_minus_1"] += 1
            u_r0 = F(kr[best_idx_r]["x"])                                    # :1157
            scale_factor = F(isf[level_l])                                   # :1158
            scaled_ul = F(c_round(F(u_l * scale_factor)))                    # :1160
            scaled_vl = F(c_round(F(v_l * scale_factor)))                    # :1161
            scaled_ur0 = F(c_round(F(u_r0 * scale_factor)))                  # :1162
            w = 5                                                            # :1166
            img_l = levels_l[level_l]; img_r = levels_r[level_l]
            cy, cxl, cxr = int(scaled_vl), int(scaled_ul), int(scaled_ur0)
            assert cy - w >= 0 and cy + w + 1 <= img_l.shape[0] and cxl - w >= 0 and cxl + w + 1 <= img_l.shape[1], \
                ("precondition: the left window leaves its level", iL, cxl, cy, img_l.shape)
            patch_l = img_l[cy - w:cy + w + 1, cxl - w:cxl + w + 1].astype(np.int64)     # :1168
            best_sad = 2 ** 31 - 1                                           # :1171, INT_MAX
            best_inc_r = 0                                                   # :1173
            L = 5                                                            # :1175
            dists = [None] * (2 * L + 1)                                     # :1177-1178
            iniu = F(F(scaled_ur0 + F(L)) - F(w))                            # :1184
            endu = F(F(F(scaled_ur0 + F(L)) + F(w)) + F(1))                  # :1185
            cols = img_r.shape[1]
            if iniu < F(0):                                                  # :1187
                t["iniu_negative"] += 1
                continue
            if endu >= F(cols):
                t["endu_ge_cols"] += 1
                continue
            if iniu == F(0): t["iniu_zero"] += 1
            if endu == F(cols - 1): t["endu_cols_minus_1"] += 1
            assert cy + w + 1 <= img_r.shape[0]
            partial = [False] * (2 * L + 1)
            for inc_r in range(-L, L + 1):                                   # :1191
                c0 = cxr + inc_r - w; c1 = cxr + inc_r + w + 1               # :1194
                assert c1 <= cols                                            # guaranteed by :1187
                lo = max(c0, 0)
                if lo > c0:
                    partial[L + inc_r] = True
                    t["slide_left_of_level"] += 1
                patch_r = img_r[cy - w:cy + w + 1, lo:c1].astype(np.int64)
                dist = F(float(np.abs(patch_l[:, lo - c0:] - patch_r).sum()))           # :1197, double -> float
                if dist < F(best_sad):                                       # :1199, float against (float)int
                    best_sad = int(dist)                                     # :1201
                    best_inc_r = inc_r                                       # :1202
                elif dist == F(best_sad):
                    t["sad_tie_between_shifts"] += 1                         # the earlier shift stays
                dists[L + inc_r] = dist                                      # :1206
            if any(partial):
                # the shifts left of the level hold lower bounds: the outcome is defined only if a complete shift wins below all of them
                complete = [float(dists[k]) for k in range(2 * L + 1) if not partial[k]]
                assert complete and not partial[L + best_inc_r] and \
                    all(float(dists[k]) > min(complete) for k in range(2 * L + 1) if partial[k]), ("the outcome would depend on pixels outside the level", iL)
            if best_inc_r == -L or best_inc_r == L:                          # :1210
                t["bestincR_at_minus_L" if best_inc_r == -L else "bestincR_at_plus_L"] += 1
                continue
            assert not partial[L + best_inc_r - 1]
            dist1 = dists[L + best_inc_r - 1]                                # :1224
            dist2 = dists[L + best_inc_r]                                    # :1225
            dist3 = dists[L + best_inc_r + 1]                                # :1226
            delta_r = F(F(dist1 - dist3) / F(F(2.0) * F(F(dist1 + dist3) - F(F(2.0) * dist2))))    # :1228
            if delta_r < F(-1) or delta_r > F(1):                            # :1231
                t["deltaR_gate"] += 1
                continue
            if delta_r == F(0.5): t["deltaR_half"] += 1
            best_ur = F(F(sf[level_l]) * F(F(scaled_ur0 + F(best_inc_r)) + delta_r))     # :1235
            disparity = F(u_l - best_ur)                                     # :1237
            if disparity >= min_d and disparity < max_d:                     # :1239
                if disparity <= F(0):                                        # :1243
                    disparity = F(0.01)                                      # :1245, the double literal narrowed
                    best_ur = F(np.float64(u_l) - np.float64(0.01))          # :1246, a double difference narrowed
                    t["clamp"] += 1
                depth[iL] = F(mbf / disparity)                               # :1252
                uright[iL] = best_ur                                         # :1253
                dist_idx.append((best_sad, iL))                              # :1254
                sad[iL] = best_sad
            elif disparity < min_d:
                t["disparity_negative"] += 1
            else:
                assert disparity >= max_d
                t["disparity_ge_maxD"] += 1
        if not dist_idx:                                                     # :1262 would index an empty vector
            t["empty_vDistIdx"] += 1
            return 0, uright, depth, sad, t
        dist_idx.sort()                                                      # :1261, pairs: by SAD, then by iL
        median = F(dist_idx[len(dist_idx) // 2][0])                          # :1262
        th_dist = F(F(F(1.5) * F(1.4)) * median)                             # :1263
        kept = len(dist_idx)
        for i in range(len(dist_idx) - 1, -1, -1):                           # :1265
            if F(dist_idx[i][0]) < th_dist:                                  # :1267
                break
            uright[dist_idx[i][1]] = F(-1)                                   # :1272
            depth[dist_idx[i][1]] = F(-1)                                    # :1273
            kept -= 1
            t["cut"] += 1
    t["kept"] += kept
    return kept, uright, depth, sad, t
