"""A second, independent reading of M3 with F.Nleft != -1: ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th,
bFarPoints, thFarPoints) on a fisheye stereo rig -- Tracking::SearchLocalPoints --, ORBmatcher.cc:45-249, in plain Python / numpy.

Written from those reference lines and Frame::GetFeaturesInArea (Frame.cc:784-871, with bRight) alone.  It imports GridFrame and
descriptor_distances from second_reading.py (the frame with its grid, and DescriptorDistance) and nothing of the oracle, the host
claim replay, the device kernels or any other reading's search.  The arrays are those of the C ABI: the ten mbTrackInView... fields
are the caller's, mp_obs is Observations() > 0 of the query, blocked_* says that a slot of F.mvpMapPoints holds a MapPoint with
observations when the search starts.  mvpMapPoints is ONE array here as it is in the reference: slots [0, Nleft) belong to mvKeys,
slots [Nleft, Nleft + Nright) to mvKeysRight.

Besides both rows and the count the search returns a Counter of the rules it met, so that a test can prove that a constructed case
reached the rule it was built for.
"""
from collections import Counter

import numpy as np

from second_reading import GridFrame, descriptor_distances  # noqa: F401  (GridFrame: the callers' frames)

F = np.float32
TH_HIGH = 100        # ORBmatcher.cc:36
NO_MATCH = -1        # slot never assigned


def _radius_by_viewing_cos(view_cos):
    """:242-249: the float argument against the double literal 0.998."""
    if float(F(view_cos)) > 0.998:                                                                # :245
        return F(2.5)
    return F(4.0)


def _best_two(cand, dists, octave, has_obs, offset):
    """The candidate loops of :97-142 and :190-216 (F.Nleft != -1, so the mvuRight test of :107 never applies).  Returns bestDist,
    bestLevel, bestDist2, bestLevel2, bestIdx and how many candidates were passed over as observed."""
    best, best_lvl, best2, best_lvl2, best_idx = 256, -1, 256, -1, -1                             # :89-93, :183-187
    passed = 0
    for idx, dist in zip(cand, dists):
        if has_obs[idx + offset]:                                                                 # :102-104, :194-196
            passed += 1
            continue
        if dist < best:                                                                           # :125-134, :203-210
            best2 = best; best = dist
            best_lvl2 = best_lvl; best_lvl = int(octave[idx])
            best_idx = idx
        elif dist < best2:                                                                        # :135-141, :211-215
            best_lvl2 = int(octave[idx]); best2 = dist
    return best, best_lvl, best2, best_lvl2, best_idx, passed


def search_by_projection_points_fisheye(fl, fr, blocked_l, blocked_r, l2r, r2l, scale_factors, in_view, px, py, view_cos, level,
                                        in_view_r, pxr, pyr, view_cos_r, level_r, qdesc, mp_obs, th, nnratio, depth=None, th_far=None,
                                        th_on_right=False, free_on_cross=False):
    """fl, fr: GridFrame of the left / right camera.  Returns (nmatches, match_l, match_r, trace): match_x[k] = index of the query
    whose MapPoint sits in that slot of F.mvpMapPoints at the end, -1 for a slot the search did not write.  th_on_right is NOT the
    reference: it applies th to the right radius as well, for the test that shows that :173-176 do not.
    The blocked set: a claim goes only to a slot that is not blocked, so `the slot's MapPoint has observations` can change from true to
    false in one way alone -- a cross write (:158, :225) of a query WITHOUT observations over a slot whose MapPoint had them.  The entry
    points (oracle, host form, batched call) keep such a slot blocked: their blocked set only grows.  That is the default here, and
    every such write is counted as unobserved_cross_write_over_observed; free_on_cross reads :102-104 / :194-196 to the letter and
    frees the slot."""
    t = Counter()
    th, nnratio = F(th), F(nnratio)
    sf = np.asarray(scale_factors, np.float32)
    qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    nleft, nright = fl.n, fr.n
    slots = np.full(nleft + nright, NO_MATCH, np.int64)                                           # F.mvpMapPoints
    has_obs = np.zeros(nleft + nright, bool)                                                      # ...[k] && ...[k]->Observations() > 0
    if blocked_l is not None:
        has_obs[:nleft] = np.asarray(blocked_l[:nleft]) != 0
    if blocked_r is not None:
        has_obs[nleft:] = np.asarray(blocked_r[:nright]) != 0
    l2r = np.full(nleft, -1, np.int64) if l2r is None else np.asarray(l2r[:nleft], np.int64)      # F.mvLeftToRightMatch
    r2l = np.full(nright, -1, np.int64) if r2l is None else np.asarray(r2l[:nright], np.int64)    # F.mvRightToLeftMatch
    if nleft == 0:
        t["left_row_empty"] += 1
    if nright == 0:
        t["right_row_empty"] += 1
    if len(in_view) == 0:
        t["no_queries"] += 1
    nmatches = 0                                                                                  # :47
    b_factor = float(th) != 1.0                                                                   # :50

    crossed = {}                                                                                  # slot -> the query whose cross write blocked it

    def put(g, i, cross):
        """F.mvpMapPoints[g] = pMP"""
        if cross and mp_obs[i]:
            crossed[g] = i
        elif g in crossed:
            del crossed[g]
        if slots[g] >= 0:
            t["overwrote"] += 1
            if cross and has_obs[g]:
                t["cross_overwrote_observed"] += 1
        slots[g] = i
        if has_obs[g] and not mp_obs[i]:                                                          # only a cross write gets here
            t["unobserved_cross_write_over_observed"] += 1
            if not free_on_cross:
                return
        has_obs[g] = bool(mp_obs[i])

    for i in range(len(in_view)):                                                                 # :53
        if not in_view[i] and not in_view_r[i]:                                                   # :56-57
            t["neither_in_view"] += 1
            continue
        if depth is not None and F(depth[i]) > F(th_far):                                         # :59-60
            t["far_point"] += 1
            continue
        if in_view[i] and not in_view_r[i]:
            t["left_only"] += 1
        if in_view_r[i] and not in_view[i]:
            t["right_only"] += 1
        counted = 0
        left_claim = -1
        cross_blocked = -1                                                                        # right slot this query's left block blocked
        cross_slot = -1                                                                           # right slot this query's left block wrote
        left_state = None
        if in_view[i]:                                                                            # :65
            lvl = int(level[i])                                                                   # :68
            r = _radius_by_viewing_cos(view_cos[i])                                               # :72
            if b_factor:                                                                          # :75-76
                r = r * th
            cand = fl.features_in_area(px[i], py[i], r * sf[lvl], lvl - 1, lvl, t)                # :79-82
            if not cand:                                                                          # :85
                left_state = "left_empty"
            else:
                dists = descriptor_distances(qdesc[i], fl.desc[cand]).tolist()                    # :86, :119-122
                t["later_query_sees_cross_block"] += sum(1 for c in cand if has_obs[c] and crossed.get(c, i) != i)
                best, best_lvl, best2, best_lvl2, best_idx, passed = _best_two(cand, dists, fl.octave, has_obs, 0)
                if passed == len(cand):
                    left_state = "left_all_blocked"
                elif best > TH_HIGH:
                    left_state = "left_above_th_high"
                if best <= TH_HIGH:                                                               # :147
                    prod = nnratio * F(best2)                                                     # float member times int: a float product
                    if best_lvl == best_lvl2 and F(best) > prod:                                  # :151-152: the next MapPoint
                        t["left_ratio_rejected"] += 1
                        if in_view_r[i] and int(level_r[i]) != -1:
                            t["left_ratio_rejected_right_in_view"] += 1
                        continue
                    if best_lvl != best_lvl2 or F(best) <= prod:                                  # :154
                        put(best_idx, i, False)                                                   # :155
                        left_claim = best_idx
                        t["left_claims"] += 1
                        if l2r[best_idx] != -1:                                                   # :157
                            g = int(l2r[best_idx]) + nleft
                            put(g, i, True)                                                       # :158
                            nmatches += 1; counted += 1                                           # :159
                            t["l2r_cross_writes"] += 1
                            cross_slot = int(l2r[best_idx])
                            if mp_obs[i]:
                                t["l2r_cross_blocks"] += 1
                                cross_blocked = int(l2r[best_idx])
                            else:
                                t["l2r_cross_open"] += 1
                        nmatches += 1; counted += 1                                               # :163
        if in_view_r[i]:                                                                          # :170 (F.Nleft != -1)
            lvl = int(level_r[i])                                                                 # :171
            if lvl == -1:                                                                         # :172
                t["level_r_minus_1"] += 1
            else:
                r = _radius_by_viewing_cos(view_cos_r[i])                                         # :173, and no `r *= th` follows
                if th_on_right and b_factor:
                    r = r * th
                cand = fr.features_in_area(pxr[i], pyr[i], r * sf[lvl], lvl - 1, lvl, t)          # :175-176
                if left_state is not None:
                    t[left_state + "_right_searched"] += 1
                if b_factor and not th_on_right:
                    wide = fr.features_in_area(pxr[i], pyr[i], (r * th) * sf[lvl], lvl - 1, lvl, Counter())
                    t["right_between_r_and_th_r"] += len(wide) - len(cand)
                if not cand:                                                                      # :178-179
                    t["right_window_empty"] += 1
                    continue
                dists = descriptor_distances(qdesc[i], fr.desc[cand]).tolist()                    # :181, :199-201
                if cross_blocked in cand:
                    t["right_block_sees_own_cross_block"] += 1
                t["later_query_sees_cross_block"] += sum(1 for c in cand if has_obs[c + nleft] and crossed.get(c + nleft, i) != i)
                best, best_lvl, best2, best_lvl2, best_idx, passed = _best_two(cand, dists, fr.octave, has_obs, nleft)
                if best <= TH_HIGH:                                                               # :219
                    if best_lvl == best_lvl2 and F(best) > nnratio * F(best2):                    # :221-222
                        t["right_ratio_rejected"] += 1
                        continue
                    if r2l[best_idx] != -1:                                                       # :224
                        g = int(r2l[best_idx])
                        if g == left_claim:
                            t["r2l_onto_own_left_claim"] += 1
                        put(g, i, True)                                                           # :225
                        nmatches += 1; counted += 1                                               # :226
                        t["r2l_cross_writes"] += 1
                    if best_idx == cross_slot:
                        t["right_claims_own_cross_slot"] += 1
                    put(best_idx + nleft, i, False)                                               # :231
                    nmatches += 1; counted += 1                                                   # :232
                    t["right_claims"] += 1
        if counted >= 3:
            t["query_counted_3"] += 1
    return nmatches, slots[:nleft].astype(np.int32), slots[nleft:].astype(np.int32), t            # :238
