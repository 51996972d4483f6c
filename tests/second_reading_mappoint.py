"""A second, independent reading of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:450-538) and
MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:578-652), in numpy, written from the reference's lines and from the numeric rules that
facade/cvcompat.h states in its header comment (norm = square root of a double sum; Mat / s multiplies by (float)(1.0 / s)).  It shares
no code with the product.  One MapPoint at a time, the way the reference works; the batch helpers at the bottom only walk the CSR that
include/orbm.h describes and apply its skip rules.

Observation entries are (row, slot, flags): flags bit 0 = the entry is a right-camera observation, bit 1 = the KeyFrame isBad()."""
import numpy as np

F = np.float32
RIGHT, BAD_KF = 1, 2


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance: the number of differing bits of two 32-byte descriptors."""
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def compute_distinctive(descs):
    """:490-537 on the list vDescriptors -> (BestIdx, BestMedian), or (-1, -1) for an empty list (:490-491 returns)."""
    n = len(descs)
    if n == 0:
        return -1, -1
    dist = np.zeros((n, n), np.int64)                                       # float Distances[N][N] holds small integers exactly
    for i in range(n):
        for j in range(i + 1, n):
            dist[i, j] = dist[j, i] = descriptor_distance(descs[i], descs[j])
    best_median, best_idx = np.iinfo(np.int32).max, 0
    for i in range(n):
        v = sorted(int(x) for x in dist[i])                                 # :518-519
        median = v[int(0.5 * (n - 1))]                                      # :521
        if median < best_median:                                            # :524, strict
            best_median, best_idx = median, i
    return best_idx, best_median


def _norm(d):
    """cv::norm of a 3-vector of floats: the square root of a double sum of squares."""
    s = 0.0
    for c in d:
        s += float(c) * float(c)
    return np.sqrt(np.float64(s))


def update_normal_and_depth(pos, centres, ref_centre, level, scale_factors):
    """:601-649.  centres: the camera centre (3 floats) of every n++ of the loop, in loop order; ref_centre: pRefKF->GetCameraCenter();
    level: the octave of the reference keypoint -> (normal [3], min_dist, max_dist), or None when there is nothing to average."""
    pos = np.asarray(pos, F)
    normal = np.zeros(3, F)
    n = 0
    with np.errstate(all="ignore"):
        for ow in centres:
            normali = (pos - np.asarray(ow, F)).astype(F)                   # :612 / :618
            s = F(1.0 / _norm(normali))                                     # Mat / s: (float)(1.0 / s)
            normal = (normal + (normali * s).astype(F)).astype(F)           # :613: a float product, then a float sum
            n += 1
        if n == 0:
            return None
        pc = (pos - np.asarray(ref_centre, F)).astype(F)                    # :624
        dist = F(_norm(pc))                                                 # :625
        sf = np.asarray(scale_factors, F)
        max_d = F(dist * sf[level])                                         # :647
        min_d = F(max_d / sf[len(sf) - 1])                                  # :648
        normal = (normal * F(1.0 / n)).astype(F)                            # :649: normal / n
    return normal, min_d, max_d


# ---- the batch contract of include/orbm.h around the two functions -----------------------------------------------------------

def _entries(mp, obs_off, nobs, valid):
    if valid is not None and not valid[mp]:
        return range(0)
    a, b = int(obs_off[mp]), int(obs_off[mp + 1])
    if a < 0 or b > nobs or b <= a or b - a > 65535:
        return range(0)
    return range(a, b)


def _in_pool(row, slot, counts, cap):
    return 0 <= row < len(counts) and 0 <= slot < min(int(counts[row]), cap)


def distinctive_batch(desc_kf, counts_kf, obs_off, obs_row, obs_slot, obs_flags, valid, mp_desc_in):
    """-> (mp_desc, best_obs, best_median): best_obs counts skipped entries; rows without a winner keep mp_desc_in."""
    nmp, cap = len(obs_off) - 1, desc_kf.shape[1]
    out = np.array(mp_desc_in, np.uint8).reshape(nmp, 32).copy()
    best_obs = np.full(nmp, -1, np.int32); best_median = np.full(nmp, -1, np.int32)
    for mp in range(nmp):
        pos, descs = [], []
        ent = _entries(mp, obs_off, len(obs_row), valid)
        for e in ent:
            if obs_flags[e] & BAD_KF or not _in_pool(int(obs_row[e]), int(obs_slot[e]), counts_kf, cap):
                continue
            pos.append(e - ent[0]); descs.append(desc_kf[obs_row[e], obs_slot[e]])
        i, med = compute_distinctive(descs)
        if i >= 0:
            out[mp] = descs[i]; best_obs[mp] = pos[i]; best_median[mp] = med
    return out, best_obs, best_median


def normal_depth_batch(kps_kf, counts_kf, ow_l, ow_r, obs_off, obs_row, obs_slot, obs_flags, valid, pw, ref_row, ref_slot, scale_factors,
                       normal_in, min_in, max_in):
    """-> (normal, min_dist, max_dist, updated); rows that are not updated keep the *_in values."""
    nmp, cap = len(obs_off) - 1, kps_kf.shape[1]
    normal = np.array(normal_in, F).reshape(nmp, 3).copy(); mn = np.array(min_in, F).copy(); mx = np.array(max_in, F).copy()
    updated = np.zeros(nmp, np.uint8)
    for mp in range(nmp):
        centres = []
        for e in _entries(mp, obs_off, len(obs_row), valid):
            r, s = int(obs_row[e]), int(obs_slot[e])
            if not _in_pool(r, s, counts_kf, cap):
                continue
            if obs_flags[e] & RIGHT:
                if ow_r is None:
                    continue
                centres.append(ow_r[r])
            else:
                centres.append(ow_l[r])
        rr, rs = int(ref_row[mp]), int(ref_slot[mp])
        if not centres or not _in_pool(rr, rs, counts_kf, cap):
            continue
        level = int(kps_kf[rr, rs]["octave"])
        if not 0 <= level < len(scale_factors):
            continue
        normal[mp], mn[mp], mx[mp] = update_normal_and_depth(pw[mp], centres, ow_l[rr], level, scale_factors)
        updated[mp] = 1
    return normal, mn, mx, updated
