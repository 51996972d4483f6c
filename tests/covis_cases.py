"""Constructed maps for the covisibility votes and the local map points (tests/second_reading_covis.py): every case is small enough to
be worked by hand, and the seeded random maps mix all of their ingredients.  KeyFrame k has addr = mnId = k unless a case says so."""
import numpy as np

import second_reading_covis as sr


def world(n, N=8, stereo=(), other_map=(), bad=()):
    """n KeyFrames of N slots in one map; `stereo` rows are two-camera rows of N / 2 left and N / 2 right slots; `other_map` rows lie in a
    second map; `bad` rows are isBad()."""
    m, m2 = sr.Map(), sr.Map()
    kfs = []
    for k in range(n):
        kf = sr.KeyFrame(k, k, [0] * N, m2 if k in other_map else m, NLeft=N // 2 if k in stereo else -1, camera2=k in stereo)
        kf.mbBad = k in bad
        kfs.append(kf)
    return m, kfs


def point(addr, obs):
    """A MapPoint observed at (KeyFrame, slot) pairs."""
    mp = sr.MapPoint(addr)
    for kf, idx in obs:
        sr.link(kf, idx, mp)
    return mp


# ---- votes: name -> (kfs, query KeyFrame index or a Frame, expected {KeyFrame index: votes}) -----------------------------------
def own_row():
    _, k = world(2)
    for i in range(3):
        point(i, [(k[0], i), (k[1], i)])
    return k, 0, {1: 3}


def bad_keyframe():
    """KeyFrame 2 is bad and sees two of the three MapPoints: UpdateConnections drops it, UpdateLocalKeyFrames counts it."""
    _, k = world(3, bad=(2,))
    for i in range(3):
        point(i, [(k[0], i), (k[1], i)] + ([(k[2], i)] if i < 2 else []))
    return k, 0, {1: 3}


def bad_keyframe_frame():
    k, _, _ = bad_keyframe()
    return k, sr.Frame(100, k[0].GetMapPointMatches()), {0: 3, 1: 3, 2: 2}


def other_map():
    _, k = world(3, other_map=(2,))
    for i in range(4):
        point(i, [(k[0], i), (k[1], i), (k[2], i)])
    return k, 0, {1: 4}


def other_map_frame():
    k, _, _ = other_map()
    return k, sr.Frame(100, k[0].GetMapPointMatches()), {0: 4, 1: 4, 2: 4}


def left_right_pair():
    """KeyFrame 1 is a two-camera row and sees the MapPoint in slot 1 (left) and slot 5 (right): one vote."""
    _, k = world(2, stereo=(1,))
    point(0, [(k[0], 0), (k[1], 1), (k[1], 5)])
    point(1, [(k[0], 1), (k[1], 2)])
    return k, 0, {1: 2}


def lone_right():
    _, k = world(2, stereo=(1,))
    point(0, [(k[0], 0), (k[1], 6)])
    return k, 0, {1: 1}


def two_slots():
    """The same MapPoint in slots 0 and 1 of the query votes twice."""
    _, k = world(3)
    mp = point(0, [(k[0], 0), (k[1], 3), (k[2], 4)])
    k[0].mvpMapPoints[1] = mp
    return k, 0, {1: 2, 2: 2}


def bad_or_null_point():
    _, k = world(2)
    point(0, [(k[0], 0), (k[1], 0)])
    dead = point(1, [(k[0], 2), (k[1], 1)])
    dead.mbBad = True
    return k, 0, {1: 1}


def bad_point_frame():
    """UpdateLocalKeyFrames sets the slot of a bad MapPoint to NULL (:3986)."""
    k, _, _ = bad_or_null_point()
    return k, sr.Frame(100, k[0].GetMapPointMatches()), {0: 1, 1: 1}


def fourteen_fifteen():
    """KeyFrame 1 shares 14 MapPoints, KeyFrame 2 shares 15: one row at or above th = 15."""
    _, k = world(3, N=16)
    for i in range(15):
        point(i, [(k[0], i), (k[2], i)] + ([(k[1], i)] if i < 14 else []))
    return k, 0, {1: 14, 2: 15}


def empty_vote():
    _, k = world(2)
    return k, 0, {}


def tie_in_pointer_order():
    """Two KeyFrames with the same count: pKFmax is the one with the lower address, whatever its mnId is."""
    _, k = world(3)
    k[1].addr, k[2].addr = 9, 5
    for i in range(2):
        point(i, [(k[0], i), (k[1], i), (k[2], i)])
    return k, 0, {1: 2, 2: 2}


VOTE_CASES = {f.__name__: f for f in (own_row, bad_keyframe, bad_keyframe_frame, other_map, other_map_frame, left_right_pair, lone_right, two_slots,
                                       bad_or_null_point, bad_point_frame, fourteen_fifteen, empty_vote, tie_in_pointer_order)}


# ---- local points: name -> (mvpLocalKeyFrames, expected MapPoint addrs in order) -----------------------------------------------
def dedupe():
    """Walked in reverse: KeyFrame 1 first (points 2, 1), then KeyFrame 0 (point 0; 1 is there already)."""
    _, k = world(2)
    point(0, [(k[0], 0)]); point(1, [(k[0], 1), (k[1], 3)]); point(2, [(k[1], 0)])
    return [k[0], k[1]], [2, 1, 0]


def listed_twice():
    _, k = world(2)
    point(0, [(k[0], 0)]); point(1, [(k[1], 1)])
    return [k[0], k[1], k[0]], [0, 1]


def reverse_order():
    """The same map as dedupe with the list the other way round: another order of the same three points."""
    kfs, _ = dedupe()
    return kfs[::-1], [0, 1, 2]


def bad_points():
    _, k = world(2)
    point(0, [(k[0], 5)]); dead = point(1, [(k[0], 0), (k[1], 0)]); point(2, [(k[1], 7)])
    dead.mbBad = True
    return [k[1], k[0]], [0, 2]


def no_keyframes():
    return [], []


LOCAL_CASES = {f.__name__: f for f in (dedupe, listed_twice, reverse_order, bad_points, no_keyframes)}


# ---- seeded random maps ---------------------------------------------------------------------------------------------------------
def random_map(seed):
    """-> (KeyFrames, a Frame, mvpLocalKeyFrames): 6 to 14 KeyFrames of 6 to 24 slots, some two-camera, some bad, some in another map,
    MapPoints with 1 to 8 observers (left / right pairs, lone right entries), bad MapPoints, MapPoints in two slots."""
    rng = np.random.RandomState(1000 + seed)
    n = int(rng.randint(6, 15))
    m, m2 = sr.Map(), sr.Map()
    addrs = rng.permutation(100)[:n]
    kfs = []
    for k in range(n):
        N = int(rng.randint(3, 13)) * 2
        st = rng.rand() < 0.3
        kf = sr.KeyFrame(int(addrs[k]), k, [0] * N, m2 if rng.rand() < 0.15 else m, NLeft=N // 2 if st else -1, camera2=st,
                         uRight=None if st else list(rng.choice([-1.0, 3.0], N)))
        kfs.append(kf)
    mps = []
    for a in range(int(rng.randint(10, 60))):
        mp = sr.MapPoint(a)
        for k in rng.permutation(n)[:int(rng.randint(1, 9))]:
            kf = kfs[k]
            free = [i for i in range(kf.N) if kf.mvpMapPoints[i] is None]
            if not free:
                continue
            if kf.NLeft != -1:
                left = [i for i in free if i < kf.NLeft]; right = [i for i in free if i >= kf.NLeft]
                u = rng.rand()
                if u < 0.4 and left and right:
                    sr.link(kf, left[0], mp); sr.link(kf, right[0], mp)
                elif u < 0.7 and right:
                    sr.link(kf, right[-1], mp)
                elif left:
                    sr.link(kf, left[-1], mp)
            else:
                sr.link(kf, int(rng.choice(free)), mp)
        mps.append(mp)
    for mp in mps:
        if rng.rand() < 0.1:
            mp.mbBad = True
    for kf in kfs:
        if rng.rand() < 0.15:
            kf.mbBad = True
        if rng.rand() < 0.3 and mps:                                        # a MapPoint in a second slot, with no observation entry of its own
            free = [i for i in range(kf.N) if kf.mvpMapPoints[i] is None]
            if free:
                kf.mvpMapPoints[free[0]] = mps[int(rng.randint(len(mps)))]
    slots = [None if rng.rand() < 0.3 else mps[int(rng.randint(len(mps)))] for _ in range(int(rng.randint(0, 40)))]
    local = [kfs[int(k)] for k in rng.randint(0, n, int(rng.randint(0, 8)))]
    return kfs, sr.Frame(500 + seed, slots), local
