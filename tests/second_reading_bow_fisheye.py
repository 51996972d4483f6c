"""A second, independent reading of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) for a two-camera Frame
(M7 with F.Nleft != -1), in plain Python / numpy.

Written from the reference's ORBmatcher.cc:314-547 alone, in the manner of tests/second_reading.py (whose helpers it uses): it shares
no code with the CPU oracle, the host claim replay or the device kernels, and it imports none of them.  Every float operation is one
np.float32 operation, and the search returns a collections.Counter of the branches it took, so that a test can prove that a
constructed case reached the rule it was built for.

The Frame is given as the reference holds it: kps_f and desc_f are the left rows followed by the right rows (mvKeys then mvKeysRight,
mDescriptors stacked), nleft = F.Nleft, and fv_f is the FeatureVector over those combined indices.  The KeyFrame likewise is one stacked
row, and kps_kf carries the angle of mvKeys / mvKeysRight for each of its features (:447-450).
"""
from collections import Counter

import numpy as np

from second_reading import F, HISTO_LENGTH, TH_LOW, FACTOR_360, NO_MATCH, _common_buckets, _culled_bins, descriptor_distances, rotation_bin


def search_by_bow_fisheye(kps_kf, desc_kf, kf_good, fv_kf, kps_f, desc_f, nleft, fv_f, nnratio, check_ori=True):
    """Returns (nmatches, f_match, trace): f_match[realIdxF] = KeyFrame feature whose MapPoint sits in vpMapPointMatches[realIdxF], or
    -1 (NULL), over the combined indices (left row = f_match[:nleft], right row = f_match[nleft:])."""
    t = Counter()
    nnratio = F(nnratio)
    nleft = int(nleft)
    desc_kf = np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32); desc_f = np.ascontiguousarray(desc_f, np.uint8).reshape(-1, 32)
    f_match = np.full(len(kps_f), NO_MATCH, np.int32)                                             # :320
    rot_hist = [[] for _ in range(HISTO_LENGTH)]                                                  # :328
    nmatches = 0                                                                                  # :325
    for ikf, iff in _common_buckets(fv_kf, fv_f):                                                 # :343-347, :505-517
        iff = np.asarray(iff, np.int64)
        for real_kf in ikf:                                                                       # :354
            real_kf = int(real_kf)
            if not kf_good[real_kf]:                                                              # :362-366
                continue
            dists = descriptor_distances(desc_kf[real_kf], desc_f[iff]).tolist() if len(iff) else []
            best1, best_idx, best2 = 256, -1, 256                                                 # :370-372
            best1r, best_idx_r, best2r = 256, -1, 256                                             # :374-376
            for real_f, dist in zip(iff.tolist(), dists):                                         # :378, the else branch :406-433
                if f_match[real_f] >= 0:                                                          # :409
                    t["skipped_claimed_right" if real_f >= nleft else "skipped_claimed_left"] += 1
                    continue
                if real_f < nleft and dist < best1:                                               # :416
                    best2 = best1; best1 = dist; best_idx = real_f
                elif real_f < nleft and dist < best2:                                             # :421
                    best2 = dist
                if real_f >= nleft and dist < best1r:                                             # :425
                    best2r = best1r; best1r = dist; best_idx_r = real_f
                elif real_f >= nleft and dist < best2r:                                           # :430
                    best2r = dist
            if best1 <= TH_LOW:                                                                   # :438
                left_ok = bool(F(best1) < nnratio * F(best2))                                     # :441
                if left_ok:
                    f_match[best_idx] = real_kf                                                   # :444
                    if check_ori:                                                                 # :452-466
                        rot_hist[rotation_bin(kps_kf["angle"][real_kf], kps_f["angle"][best_idx], FACTOR_360, t)].append(best_idx)
                    nmatches += 1                                                                 # :468
                    t["left_claimed"] += 1
                else:
                    t["left_ratio_failed"] += 1
                if best1r <= TH_LOW:                                                              # :471
                    # :473  `static_cast<float>(bestDist1R) < mfNNratio * static_cast<float>(bestDist2R) || true`
                    if not left_ok:
                        t["right_claimed_left_ratio_failed"] += 1
                    if best1r == best2r:
                        t["right_claimed_best_equals_runner_up"] += 1
                    if not bool(F(best1r) < nnratio * F(best2r)):
                        t["right_claimed_own_ratio_failed"] += 1
                    if left_ok:
                        t["both_cameras_claimed"] += 1
                    f_match[best_idx_r] = real_kf                                                 # :475
                    if check_ori:                                                                 # :482-497
                        rot_hist[rotation_bin(kps_kf["angle"][real_kf], kps_f["angle"][best_idx_r], FACTOR_360, t)].append(best_idx_r)
                    nmatches += 1                                                                 # :498
                    t["right_claimed"] += 1
            elif best1r <= TH_LOW:                                                                # the right block sits INSIDE :438
                if best1 == 256 and best_idx == -1:
                    t["right_refused_no_left_candidate"] += 1
                else:
                    t["right_refused_left_over_th_low"] += 1
    if check_ori:                                                                                 # :521-544
        for b in _culled_bins(rot_hist, t):
            for s in rot_hist[b]:
                f_match[s] = NO_MATCH                                                             # :540
                nmatches -= 1                                                                     # :541
                t["culled_right" if s >= nleft else "culled_left"] += 1
    return nmatches, f_match, t
