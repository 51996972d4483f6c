"""A second, independent reading of M4 with CurrentFrame.Nleft != -1: ORBmatcher::SearchByProjection(Frame& Cur, const Frame& Last, th,
bMono) on a fisheye stereo rig, ORBmatcher.cc:2469-2711, in plain Python / numpy.

Written from those reference lines (and Frame::GetFeaturesInArea with bRight, Frame.cc:784-871; Tracking.cc:3211-3221 for the retry)
alone.  It imports GridFrame, rotation_bin, compute_three_maxima and descriptor_distances from second_reading.py and nothing of the
oracle, the host claim replay or the device kernels.  The arrays are those of the C ABI: the projections are the caller's, `valid`
folds the tests of :2505-2528 (made on the LEFT projection only), (ur, vr) is the projection of Trl * x3Dc into the right camera
(:2616-2618).  mvpMapPoints is ONE array here as it is in the reference: slots [0, Nleft) belong to mvKeys, slots [Nleft, Nleft +
Nright) to mvKeysRight, and the rotation histogram holds those global indices (:2612, :2677).
"""
from collections import Counter

import numpy as np

from second_reading import GridFrame, compute_three_maxima, descriptor_distances, rotation_bin  # noqa: F401  (GridFrame: the callers' frames)

F = np.float32
TH_HIGH = 100        # ORBmatcher.cc:36
HISTO_LENGTH = 30    # ORBmatcher.cc:38
NO_MATCH = -1        # slot never assigned
PRUNED = -2          # slot assigned and then set to NULL by the rotation check (:2703)


def _window(frame, x, y, radius, o, forward, backward, t):
    """The three GetFeaturesInArea calls of :2544-2549 (left, bRight = false) and :2628-2633 (right, bRight = true): the frame
    handed in IS that camera's keys and grid, so bRight only picks which one the caller passes."""
    if forward:
        return frame.features_in_area(x, y, radius, o, -1, t)
    if backward:
        return frame.features_in_area(x, y, radius, 0, o, t)
    return frame.features_in_area(x, y, radius, o - 1, o + 1, t)


def _best(cand, dists, has_obs, offset):
    """The candidate loops of :2560-2587 and :2640-2656: a slot whose MapPoint has observations is passed over, `dist < bestDist`
    keeps the first candidate of least distance."""
    best, best_idx = 256, -1                                                                      # :2556-2557, :2637-2638
    for i2, dist in zip(cand, dists):
        if has_obs[i2 + offset]:                                                                  # :2565-2567, :2643-2645
            continue
        if dist < best:                                                                           # :2582, :2651
            best, best_idx = dist, i2
    return best, best_idx


def search_by_projection_frame_fisheye(fl, fr, blocked_l, blocked_r, scale_factors, valid, u, v, ur, vr, octave, angle, qdesc, mp_obs, th,
                                       forward=False, backward=False, check_ori=True):
    """fl, fr: GridFrame of the left / right camera.  Returns (nmatches, match_l, match_r, trace): match_x[i2] = last-frame index now
    in that slot of Cur.mvpMapPoints, -1 untouched, -2 set to NULL by the rotation check."""
    t = Counter()
    th = F(th)
    sf = np.asarray(scale_factors, np.float32)
    qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    nleft, nright = fl.n, fr.n
    slots = np.full(nleft + nright, NO_MATCH, np.int64)                                           # Cur.mvpMapPoints
    has_obs = np.zeros(nleft + nright, bool)                                                      # ...[k] && ...[k]->Observations() > 0
    if blocked_l is not None:
        has_obs[:nleft] = np.asarray(blocked_l[:nleft]) != 0
    if blocked_r is not None:
        has_obs[nleft:] = np.asarray(blocked_r[:nright]) != 0
    cur_angle = np.concatenate([fl.angle, fr.angle])                                              # :2602-2604, :2668
    factor = F(HISTO_LENGTH) / F(360.0)                                                           # :2480
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i in range(len(valid)):                                                                   # :2503
        if not valid[i]:                                                                          # :2505-2528
            continue
        o = int(octave[i])                                                                        # :2530
        radius = th * sf[o]                                                                       # :2535
        cand = _window(fl, u[i], v[i], radius, o, forward, backward, t)                           # :2544-2549
        if not cand:                                                                              # :2551: leaves the loop body, :2615 is not reached
            t["left_window_empty"] += 1
            continue
        best, best_idx = _best(cand, descriptor_distances(qdesc[i], fl.desc[cand]).tolist(), has_obs, 0)
        if best_idx < 0:
            t["left_all_blocked"] += 1
        if best <= TH_HIGH:                                                                       # :2590
            if slots[best_idx] >= 0:
                t["overwrote"] += 1
            slots[best_idx] = i                                                                   # :2592
            has_obs[best_idx] = bool(mp_obs[i])
            nmatches += 1                                                                         # :2593
            t["left_claims"] += 1
            if check_ori:                                                                         # :2596-2613
                rot_hist[rotation_bin(angle[i], cur_angle[best_idx], factor, t)].append(best_idx)
        # :2615 CurrentFrame.Nleft != -1
        radius_r = th * sf[o]                                                                     # :2620-2624
        cand_r = _window(fr, ur[i], vr[i], radius_r, o, forward, backward, t)                     # :2628-2633
        if not cand_r:
            t["right_window_empty"] += 1
        dists_r = descriptor_distances(qdesc[i], fr.desc[cand_r]).tolist() if cand_r else []
        best, best_idx = _best(cand_r, dists_r, has_obs, nleft)                                   # :2637-2656
        if cand_r and best_idx < 0:
            t["right_all_blocked"] += 1
        if best <= TH_HIGH:                                                                       # :2658
            g = best_idx + nleft
            if slots[g] >= 0:
                t["overwrote"] += 1
            slots[g] = i                                                                          # :2660
            has_obs[g] = bool(mp_obs[i])
            nmatches += 1                                                                         # :2661
            t["right_claims"] += 1
            if check_ori:                                                                         # :2662-2678
                rot_hist[rotation_bin(angle[i], cur_angle[g], factor, t)].append(g)
    if check_ori:                                                                                 # :2688-2708
        ind1, ind2, ind3 = compute_three_maxima([len(h) for h in rot_hist])                       # :2690-2694
        for b in range(HISTO_LENGTH):
            if b != ind1 and b != ind2 and b != ind3:                                             # :2699
                for g in rot_hist[b]:
                    slots[g] = PRUNED                                                             # :2703
                    nmatches -= 1                                                                 # :2704
                    t["culled_left" if g < nleft else "culled_right"] += 1
    return nmatches, slots[:nleft].astype(np.int32), slots[nleft:].astype(np.int32), t


def search_by_projection_frame_fisheye_with_retry(fl, fr, blocked_l, blocked_r, scale_factors, valid, u, v, ur, vr, octave, angle, qdesc,
                                                  mp_obs, th, forward=False, backward=False, check_ori=True, retry_below=20):
    """Tracking::TrackWithMotionModel, Tracking.cc:3211-3221: the call, and below `retry_below` matches the frame's mvpMapPoints are
    all reset to NULL and the search runs again at 2 * th.  Returns (nmatches, match_l, match_r, trace, retried)."""
    n, ml, mr, t = search_by_projection_frame_fisheye(fl, fr, blocked_l, blocked_r, scale_factors, valid, u, v, ur, vr, octave, angle, qdesc,
                                                      mp_obs, th, forward, backward, check_ori)
    if n < retry_below:                                                                           # Tracking.cc:3215
        n, ml, mr, t = search_by_projection_frame_fisheye(fl, fr, None, None, scale_factors, valid, u, v, ur, vr, octave, angle, qdesc,
                                                          mp_obs, F(2) * F(th), forward, backward, check_ori)   # Tracking.cc:3217-3220
        return n, ml, mr, t, True
    return n, ml, mr, t, False
