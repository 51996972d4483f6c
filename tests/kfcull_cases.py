"""Constructed maps for KeyFrameCulling: every rule of the contract in include/orbm.h gets a named case, built on the plain objects of
tests/second_reading_kfcull.py.  A case carries the covisible list, the sensor flag, the threshold, an optional `tweak` of the flattened
arrays (rules that only exist at the array level: out-of-range indices, short counts, skipped entries) and the hand-worked answers:
  seq  one (n_mps, n_redundant, cull, erased afterwards) per KeyFrame the sequential reading counts
  con  one (n_mps, n_redundant, cull) per candidate of ONE contract call without erased flags on the tweaked arrays; None = the same as
       seq up to and including the first cull
random_map(seed) lays the seeded maps of tests/test_kfcull_rule_cpu.py and tests/test_gpu_kfcull.py."""
import numpy as np

import second_reading_kfcull as sr

NAN = float("nan")


class Builder:
    def __init__(self, init_id=0):
        self.map = sr.Map(init_id)
        self.kfs, self.mps = [], []

    def kf(self, octaves, mnId=None, **kw):
        k = sr.KeyFrame(len(self.kfs), len(self.kfs) + 1 if mnId is None else mnId, octaves, self.map, **kw)
        self.kfs.append(k)
        return k

    def mp(self, *seen):
        """A MapPoint observed at the (KeyFrame, slot) pairs given."""
        m = sr.MapPoint(len(self.mps))
        self.mps.append(m)
        for kf, idx in seen:
            sr.link(kf, idx, m)
        return m

    def observers(self, n, slots, octave=2, **kw):
        return [self.kf([octave] * slots, **kw) for _ in range(n)]

    def pad_redundant(self, cand, first, n, obs, obs_first):
        """n MapPoints in slots first.. of cand, each also seen by the four KeyFrames obs at slots obs_first..: redundant while those live."""
        for t in range(n):
            self.mp((cand, first + t), *[(o, obs_first + t) for o in obs])


class Case:
    def __init__(self, name, covisible, seq, monocular=True, th=0.9, con=None, tweak=None, abort=False, builder=None):
        self.name, self.covisible, self.seq, self.monocular, self.th, self.con, self.tweak, self.abort = name, covisible, seq, monocular, th, con, tweak, abort
        self.builder = builder


def _gate_obs_3_and_4():
    """Observations() 3 and 4 against th_obs 3.  Two MapPoints, each seen by the candidate and four passing KeyFrames: both redundant in
    the map (Observations 5).  With mp_nobs rewritten to 3 and 4 the first stays at `counted`, the second is redundant: 1 > 0.9f * 2 is
    false."""
    b = Builder()
    c = b.kf([2, 2]); obs = b.observers(4, 2)
    b.pad_redundant(c, 0, 2, obs, 0)

    def tweak(F):
        F["mp_nobs"][0] = 3; F["mp_nobs"][1] = 4
    return Case("gate_obs_3_and_4", [c], [(2, 2, 1, True)], con=[(2, 1, 0)], tweak=tweak, builder=b)


def _level_l1_and_l2():
    """The candidate's keypoint is at level 2.  MapPoint a: four observers at level 3 = L + 1, all pass.  MapPoint b: three at level 3 and
    one at level 4 = L + 2: the count is 3, not above 3."""
    b = Builder()
    c = b.kf([2, 2]); obs = [b.kf([3, 3]), b.kf([3, 3]), b.kf([3, 3]), b.kf([3, 4])]
    b.pad_redundant(c, 0, 2, obs, 0)
    return Case("level_L1_and_L2", [c], [(2, 1, 0, False)], builder=b)


def _own_entry():
    """Seen by the candidate and three passing KeyFrames: Observations() is 4 > 3, the candidate's own entry does not count, 3 is not > 3."""
    b = Builder()
    c = b.kf([2]); obs = b.observers(3, 1)
    b.mp((c, 0), *[(o, 0) for o in obs])
    return Case("own_entry", [c], [(1, 0, 0, False)], builder=b)


def _pair():
    """A two-camera KeyFrame P (two left, two right slots).  MapPoint a: P's left keypoint at level 7 fails, its right one at level 1
    passes, plus three passing KeyFrames: 4 > 3, redundant.  MapPoint b: both of P's keypoints pass, plus two others: P counts once, 3 is
    not > 3 (per entry it would be 4)."""
    b = Builder()
    c = b.kf([2, 2]); p = b.kf([7, 1, 1, 1], NLeft=2, camera2=True); obs = b.observers(3, 2)
    b.mp((c, 0), (p, 0), (p, 2), *[(o, 0) for o in obs])
    b.mp((c, 1), (p, 1), (p, 3), (obs[0], 1), (obs[1], 1))
    return Case("pair_only_right_passes", [c], [(2, 1, 0, False)], builder=b)


def _right_without_left():
    """P sees the MapPoint with its right camera only; with three others that is 4 > 3.  1 > 0.9f * 1: voted out and erased."""
    b = Builder()
    c = b.kf([2]); p = b.kf([7, 7, 1, 1], NLeft=2, camera2=True); obs = b.observers(3, 1)
    b.mp((c, 0), (p, 3), *[(o, 0) for o in obs])
    return Case("right_without_left", [c], [(1, 1, 1, True)], builder=b)


def _depth():
    """A stereo candidate, mThDepth 35: depths 35 (== th), -1, -0.0, NaN, 36 and 5.  Counted: == th, -0.0, NaN and 5."""
    b = Builder()
    c = b.kf([2] * 6, uRight=[10.0] * 6, depth=[35.0, -1.0, -0.0, NAN, 36.0, 5.0], thDepth=35.0)
    for i in range(6):
        b.mp((c, i))
    return Case("depth_gate", [c], [(4, 0, 0, False)], monocular=False, builder=b)


def _null_bad_oor():
    """Slot 0 NULL, slot 1 a bad MapPoint, slots 2 and 3 live ones; the arrays then get an out-of-range kf_mp in slot 3."""
    b = Builder()
    c = b.kf([2] * 4)
    bad = b.mp((c, 1)); bad.mbBad = True
    b.mp((c, 2)); b.mp((c, 3))

    def tweak(F):
        F["kf_mp"][0, 3] = len(F["mp_nobs"]) + 5
    return Case("null_bad_out_of_range_kf_mp", [c], [(2, 0, 0, False)], con=[(1, 0, 0)], tweak=tweak, builder=b)


def _beyond_counts():
    """Three redundant slots; with counts_kf of the candidate's row cut to 1 only slot 0 is walked: 1 of 1."""
    b = Builder()
    c = b.kf([2] * 3); obs = b.observers(4, 3)
    b.pad_redundant(c, 0, 3, obs, 0)

    def tweak(F):
        F["counts_kf"][F["cand_row"][0]] = 1
    return Case("slots_beyond_counts_kf", [c], [(3, 3, 1, True)], con=[(1, 1, 1)], tweak=tweak, builder=b)


def _skipped_entry():
    """Redundant through four observers; with one observer entry's slot sent out of range it is skipped and 3 is not > 3."""
    b = Builder()
    c = b.kf([2]); obs = b.observers(4, 1)
    b.pad_redundant(c, 0, 1, obs, 0)

    def tweak(F):
        F["obs_slot"][2] = 10000
    return Case("skipped_csr_entry", [c], [(1, 1, 1, True)], con=[(1, 0, 0)], tweak=tweak, builder=b)


def _erasure(stereo_first):
    """c1 holds 30 redundant MapPoints and three shared ones, of which a is redundant for c1 too (c2 and three others): 31 > 0.9f * 33 =
    29.7, voted out and erased.  c2 then meets
      a   seen by c1, c2 and three others: 5 before; afterwards 4 > 3 but only three observers are left: counted, not redundant
      a2  seen by c1, c2 and two others: the erasure lowers Observations() to 3, not > 3: counted
      b   seen by c1, c2 and one other: lowered to 2: bad, gone from c2
    With a stereo c1 (weight 2) a2 falls from 5 to 3 and b from 4 to 2: the same answers through weight-2 entries."""
    b = Builder()
    kw = dict(uRight=[5.0] * 33, depth=[1.0] * 33) if stereo_first else {}
    c1 = b.kf([2] * 33, **kw); c2 = b.kf([2] * 3); pad = b.observers(4, 30); o = b.observers(3, 3)
    b.pad_redundant(c1, 0, 30, pad, 0)
    b.mp((c1, 30), (c2, 0), (o[0], 0), (o[1], 0), (o[2], 0))
    b.mp((c1, 31), (c2, 1), (o[0], 1), (o[1], 1))
    b.mp((c1, 32), (c2, 2), (o[0], 2))
    # one call without flags sees the map before the erasure: a is redundant for c2 (c1 and three others), 1 > 0.9f * 3 is false
    return Case("erasure_weight2" if stereo_first else "erasure_to_3_and_to_2", [c1, c2], [(33, 31, 1, True), (2, 0, 0, False)],
                con=[(33, 31, 1), (3, 1, 0)], builder=b)


def _ratio(n_red, n, cull):
    b = Builder()
    c = b.kf([2] * n); obs = b.observers(4, n)
    b.pad_redundant(c, 0, n_red, obs, 0)
    for i in range(n_red, n):
        b.mp((c, i))
    return Case("ratio_%d_of_%d" % (n_red, n), [c], [(n, n_red, cull, bool(cull))], builder=b)


def _no_mps():
    """No MapPoint at all: 0 > 0.9f * 0 is false."""
    b = Builder()
    return Case("n_mps_zero", [b.kf([2] * 5)], [(0, 0, 0, False)], builder=b)


def _not_erasable_twice():
    """Two KeyFrames in a row that loop closing holds (mbNotErase): both are voted out, both stay, nothing changes in between."""
    b = Builder()
    c1 = b.kf([2] * 2, notErase=True); c2 = b.kf([2] * 2, notErase=True); obs = b.observers(4, 4)
    b.pad_redundant(c1, 0, 2, obs, 0); b.pad_redundant(c2, 0, 2, obs, 2)
    return Case("not_erasable_twice", [c1, c2], [(2, 2, 1, False), (2, 2, 1, False)], con=[(2, 2, 1), (2, 2, 1)], builder=b)


def _skips():
    """The initial KeyFrame and a bad one are passed over (:1272); the third is counted."""
    b = Builder(init_id=1)
    first = b.kf([2]); gone = b.kf([2]); gone.mbBad = True; c = b.kf([2])
    b.mp((first, 0)); b.mp((c, 0))
    return Case("skip_initial_and_bad", [first, gone, c], [(1, 0, 0, False)], builder=b)


def _count_rule(abort):
    """104 empty KeyFrames, the second one bad: count advances on it too, the loop leaves after the KeyFrame with count 101 (21 with
    mbAbortBA): 100 / 20 records."""
    b = Builder()
    kfs = [b.kf([2]) for _ in range(104)]
    kfs[1].mbBad = True
    n = 20 if abort else 100
    return Case("count_rule_abort" if abort else "count_rule", kfs, [(0, 0, 0, False)] * n, abort=abort, builder=b)


def all_cases():
    return [_gate_obs_3_and_4(), _level_l1_and_l2(), _own_entry(), _pair(), _right_without_left(), _depth(), _null_bad_oor(), _beyond_counts(),
            _skipped_entry(), _erasure(False), _erasure(True), _ratio(9, 10, 0), _ratio(10, 11, 1), _no_mps(), _not_erasable_twice(), _skips(),
            _count_rule(False), _count_rule(True)]


CASE_NAMES = [c.name for c in all_cases()]


def case(name):
    return [c for c in all_cases() if c.name == name][0]


def random_map(seed):
    """A seeded map: 6..12 KeyFrames of 8..40 slots, mono or stereo (weight-2 entries), some two-camera KeyFrames among those of a mono
    map, some KeyFrames not erasable; MapPoints seen by 3..9 KeyFrames with levels 1..5, so that several KeyFrames are voted out one
    after the other and MapPoints fall to two observations on the way.  -> (Builder, covisible, monocular, th)"""
    rng = np.random.RandomState(seed)
    b = Builder()
    stereo = bool(rng.randint(2))
    nkf = int(rng.randint(6, 13))
    for k in range(nkf):
        n = int(rng.randint(8, 41))
        octs = [int(v) for v in rng.choice([1, 2, 2, 2, 2, 3, 3, 5], n)]
        not_erase = bool(rng.rand() < 0.15)
        if stereo:
            ur = np.where(rng.rand(n) < 0.7, 10.0, -1.0)
            dp = np.where(ur >= 0, rng.choice([1.0, 5.0, 35.0, 40.0], n), -1.0)
            b.kf(octs, uRight=[float(v) for v in ur], depth=[float(v) for v in dp], thDepth=35.0, notErase=not_erase)
        elif rng.rand() < 0.2:
            b.kf(octs, NLeft=n // 2, camera2=True, notErase=not_erase)
        else:
            b.kf(octs, notErase=not_erase)
    free = [list(rng.permutation(k.N)) for k in b.kfs]
    for _ in range(int(rng.randint(20, 70))):
        want = int(rng.choice([3, 3, 5, 6, 6, 7, 8, 9]))
        who = [int(k) for k in rng.permutation(nkf)[:want] if free[k]]
        if len(who) < 2:
            continue
        b.mp(*[(b.kfs[k], int(free[k].pop())) for k in who])
    cov = [b.kfs[i] for i in rng.permutation(nkf)]
    return b, cov, not stereo, 0.9 if rng.rand() < 0.7 else 0.5
