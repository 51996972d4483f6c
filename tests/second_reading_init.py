"""A second, independent reading of ORBmatcher::SearchForInitialization (M9), in plain Python / numpy.

Written from the reference's ORBmatcher.cc:799-943 and Frame.cc's GetFeaturesInArea alone, in the manner of tests/second_reading.py
(whose helpers it uses): it shares no code with the CPU oracle, the host claim replay or the device kernels, and it imports none of
them.  Every float operation is one np.float32 operation, and the search returns a collections.Counter of the branches it took, so
that a test can prove that a constructed scene reached the case it was built for.
"""
from collections import Counter

import numpy as np

from second_reading import F, HISTO_LENGTH, TH_LOW, FACTOR_360, GridFrame, compute_three_maxima, descriptor_distances, rotation_bin

INT_MAX = 2147483647


def _best_two(ind2, dists):
    """:856-865 over the whole list, without the test of :853."""
    best, best2, best_idx = INT_MAX, INT_MAX, -1
    for i2, d in zip(ind2, dists):
        if d < best:
            best2 = best; best = d; best_idx = i2
        elif d < best2:
            best2 = d
    return best, best2, best_idx


def _outcome(best, best2, best_idx, nn):
    return best_idx if best <= TH_LOW and F(best) < F(best2) * nn else -1


def search_for_initialization(f1, f2, prev_matched, window_size, nnratio, check_ori=True, use_skip=True):
    """ORBmatcher::SearchForInitialization, ORBmatcher.cc:799-943.  f1, f2: GridFrame; prev_matched [n1][2] (vbPrevMatched).
    Returns (nmatches, vnMatches12, vbPrevMatched after the call, trace).  use_skip = False disables the vMatchedDistance test of :853
    (NOT the reference: the what-if a test compares against to show that the skip decided something)."""
    t = Counter()
    nmatches = 0                                                       # :801
    n1, n2 = f1.n, f2.n
    matches12 = np.full(n1, -1, np.int64)                              # :803
    prev = np.array(prev_matched, np.float32).reshape(n1, 2).copy()
    rot_hist = [[] for _ in range(HISTO_LENGTH)]                       # :806
    factor = FACTOR_360                                                # :812  HISTO_LENGTH / 360.0f
    matched_distance = [INT_MAX] * n2                                  # :815
    matches21 = [-1] * n2                                              # :817
    nn = F(nnratio)
    for i1 in range(n1):                                               # :820
        level1 = int(f1.octave[i1])                                    # :823
        if level1 > 0:                                                 # :825
            t["level_skip"] += 1
            continue
        ind2 = f2.features_in_area(prev[i1, 0], prev[i1, 1], F(window_size), level1, level1, t)   # :831
        if not ind2:                                                   # :834
            t["empty_window"] += 1
            continue
        t["candidates"] += len(ind2)
        dists = descriptor_distances(f1.desc[i1], f2.desc[np.array(ind2, np.int64)])   # :851
        best, best2, best_idx = INT_MAX, INT_MAX, -1                   # :840-842
        for i2, d in zip(ind2, dists.tolist()):                        # :845
            if use_skip and matched_distance[i2] <= d:                 # :853
                t["skipped_by_matched_distance"] += 1
                continue
            if d < best:                                               # :856
                best2 = best; best = d; best_idx = i2
            elif d < best2:                                            # :862
                best2 = d
        if use_skip and _outcome(best, best2, best_idx, nn) != _outcome(*_best_two(ind2, dists.tolist()), nn):
            t["query_outcome_changed_by_skip"] += 1                    # accepted slot, or acceptance, differs from the same query without :853
        if best <= TH_LOW:                                             # :870
            if best == TH_LOW:
                t["dist_on_th_low"] += 1
            if F(best) < F(best2) * nn:                                # :873  int against a float32 product
                t["ratio_pass"] += 1
                if matches21[best_idx] >= 0:                           # :876
                    t["steal"] += 1
                    matches12[matches21[best_idx]] = -1                # :878
                    nmatches -= 1                                      # :879
                matches12[i1] = best_idx                               # :883
                matches21[best_idx] = i1                               # :884
                matched_distance[best_idx] = best                      # :885
                nmatches += 1                                          # :886
                if check_ori:                                          # :889
                    b = rotation_bin(f1.angle[i1], f2.angle[best_idx], factor, t)   # :892-900
                    rot_hist[b].append(i1)                             # :902, never undone
            else:
                t["ratio_fail"] += 1
        else:
            if best == TH_LOW + 1:
                t["dist_on_th_low_plus_1"] += 1
            if best != INT_MAX:
                t["over_th_low"] += 1
            else:
                t["all_candidates_skipped"] += 1
    t["matches_before_cull"] = nmatches
    t["row_before_cull"] = tuple(int(v) for v in matches12)
    if check_ori:                                                      # :910
        sizes = [len(h) for h in rot_hist]
        ind = compute_three_maxima(sizes)                              # :916
        t["bins_kept"] = sum(1 for x in ind if x >= 0)
        for i in range(HISTO_LENGTH):                                  # :918
            if i in ind:                                               # :920
                continue
            for idx1 in rot_hist[i]:                                   # :923
                if matches12[idx1] >= 0:                               # :926
                    matches12[idx1] = -1
                    nmatches -= 1
                    t["cull_live"] += 1
                else:
                    t["cull_robbed"] += 1
        t["hist_sizes"] = tuple(sizes)
    for i1 in range(n1):                                               # :938
        if matches12[i1] >= 0:
            prev[i1, 0] = f2.x[matches12[i1]]                          # :940
            prev[i1, 1] = f2.y[matches12[i1]]
    return nmatches, matches12.astype(np.int32), prev, t


def cull_from_finished_row(f1, f2, matches12):
    """What a cull computed from the FINISHED vnMatches12 row would keep (NOT the reference: robbed queries are missing from the bin sizes).
    A test asserts that the reference's result differs from this where robbed entries decide the three maxima."""
    t = Counter()
    m = np.array(matches12, np.int64).copy()
    bins = {}
    sizes = [0] * HISTO_LENGTH
    for i1 in np.nonzero(m >= 0)[0]:
        bins[int(i1)] = rotation_bin(f1.angle[i1], f2.angle[m[i1]], FACTOR_360, t)
        sizes[bins[int(i1)]] += 1
    ind = compute_three_maxima(sizes)
    for i1, b in bins.items():
        if b not in ind:
            m[i1] = -1
    return int((m >= 0).sum()), m.astype(np.int32)
