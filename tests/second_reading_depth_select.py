"""A second, independent reading of the reference's depth point selection, in plain Python / numpy.

Written from the reference's Tracking.cc alone -- UpdateLastFrame's walk (:3094-3163), CreateNewKeyFrame's walk (:3694-3783) and
NeedNewKeyFrame's close counts (:3524-3546): it imports no product code and no oracle.  One reference loop is one function here and
cites the lines it restates; the loops are scalar on purpose, one slot and one line of the reference at a time.

std::sort over vector<pair<float,int>> is `sorted` over (float, int) tuples: pair's operator< compares the depth first and the slot
second, as tuple comparison does; no NaN enters the list (z > 0 is false for a NaN), so the order is total.  A float compared with a
float stays a float: np.float32 comparisons.
"""
import numpy as np

F = np.float32


def depth_index(mv_depth):
    """Tracking.cc:3096-3106 and :3701-3712: the (z, i) pairs of the slots with z > 0, in slot order."""
    v = []
    for i in range(len(mv_depth)):                                       # :3098 / :3704
        z = F(mv_depth[i])                                               # :3100 / :3706
        if z > 0:                                                        # :3101 / :3707 -- false for NaN, 0 and negatives; true for +inf
            v.append((z, i))                                             # :3104 / :3710
    return v


def _walk(mv_depth, keeps_mp, th_depth, max_points):
    """The loop both functions share, :3118-3163 and :3721-3783.  Returns (order, create_new): the visited slots in visiting order
    and, per slot, whether the walk created a new MapPoint there."""
    n = len(mv_depth)
    th = F(th_depth)
    create_new = np.zeros(n, np.uint8)
    order = []
    v = depth_index(mv_depth)
    if not v:                                                            # :3109-3110 / :3714
        return order, create_new
    v = sorted(v)                                                        # :3113 / :3717
    n_points = 0                                                         # :3118 / :3721
    for j in range(len(v)):                                              # :3119 / :3722
        i = v[j][1]                                                      # :3121 / :3724
        order.append(i)
        b_create_new = False                                             # :3123 / :3726
        p_mp = keeps_mp is not None and bool(keeps_mp[i])                # pMP && pMP->Observations() >= 1
        if not p_mp:                                                     # :3127-3133 / :3730-3736: !pMP, or Observations() < 1
            b_create_new = True
        if b_create_new:                                                 # :3135 / :3739
            create_new[i] = 1                                            # :3139-3146 / :3741-3767
            n_points += 1                                                # :3147 / :3768
        else:
            n_points += 1                                                # :3152 / :3773
        if v[j][0] > th and n_points > max_points:                       # :3159 / :3779 -- false for a NaN threshold
            break                                                        # :3161 / :3781
    return order, create_new


def update_last_frame(mv_depth, keeps_mp, th_depth):
    """Tracking::UpdateLastFrame, Tracking.cc:3094-3163: the literal 100 of :3159."""
    return _walk(mv_depth, keeps_mp, th_depth, 100)


def create_new_keyframe(mv_depth, keeps_mp, th_depth, max_point=100):
    """Tracking::CreateNewKeyFrame, Tracking.cc:3694-3783: maxPoint = 100 (:3697-3699), N = the frame's slots (Nleft == -1)."""
    return _walk(mv_depth, keeps_mp, th_depth, max_point)


def select(mv_depth, keeps_mp, th_depth, max_points):
    """The walk with max_points left open -> (nvisit, order, create_new, ncreate)."""
    order, create_new = _walk(mv_depth, keeps_mp, th_depth, max_points)
    return len(order), np.array(order, np.int32), create_new, int(create_new.sum())


def close_counts(mv_depth, tracked, th_depth):
    """Tracking::NeedNewKeyFrame, Tracking.cc:3524-3546 -> (nTrackedClose, nNonTrackedClose).  tracked[i] = mvpMapPoints[i] &&
    !mvbOutlier[i] (:3535)."""
    th = F(th_depth)
    n_non_tracked_close = 0                                              # :3524
    n_tracked_close = 0                                                  # :3525
    for i in range(len(mv_depth)):                                       # :3530
        z = F(mv_depth[i])
        if z > 0 and z < th:                                             # :3533
            if tracked is not None and tracked[i]:                       # :3535
                n_tracked_close += 1                                     # :3536
            else:
                n_non_tracked_close += 1                                 # :3538
    return n_tracked_close, n_non_tracked_close
