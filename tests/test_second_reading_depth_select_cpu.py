"""Hand-worked known answers for tests/second_reading_depth_select.py, the yardstick of the depth point selection
(tests/test_gpu_depth_select.py lays the same cases into device rows).  Every expected value is worked out in the comment beside it from
the reference's lines (Tracking.cc:3094-3163, :3694-3783, :3524-3546), not taken from any code.  No GPU."""
import numpy as np
import pytest

import second_reading_depth_select as R

F = np.float32
NAN, INF = float("nan"), float("inf")


def _case(name, depth, th, max_points, nvisit, order, create, close, keeps=None, tracked=None):
    depth = np.asarray(depth, F)
    return dict(name=name, depth=depth, keeps=None if keeps is None else np.asarray(keeps, np.uint8),
                tracked=None if tracked is None else np.asarray(tracked, np.uint8), th=th, max_points=max_points, nvisit=nvisit,
                order=np.asarray(order, np.int32), create=np.asarray(create, np.uint8), close=close)


def _ones(n, upto):
    a = np.zeros(n, np.uint8); a[:upto] = 1
    return a


def _close_far(c, nfar=50):
    """c close points at 1 + i / 128 (exact floats, ascending) in slots 0..c-1, then nfar far points at 100 + i."""
    return np.concatenate([1 + np.arange(c) / 128.0, 100.0 + np.arange(nfar)]).astype(F)


CASES = [
    # 150 far points (50 .. 199 > 40), no close one: position j = 100 is the first with nPoints = 101 > 100, and it is visited before the
    # break: 101 slots, not 100.  Slots are in ascending depth, so they are visited 0 .. 100.  Nothing is < 40: no close point.
    _case("101_points", 50.0 + np.arange(150), 40.0, 100, 101, np.arange(101), _ones(150, 101), (0, 0)),
    # c = 99 close points: positions 0..98 never stop (depth <= th).  Position 99 is far but nPoints = 100 is not > 100; position 100 is
    # far with nPoints = 101: stop after it.  99 close + 2 far = 101 = max(99, 100) + 1.
    _case("c_99", _close_far(99), 40.0, 100, 101, np.arange(101), _ones(149, 101), (0, 99)),
    # c = 100: position 100 is the first far one, nPoints = 101 > 100: stop after it.  100 close + 1 far = 101.
    _case("c_100", _close_far(100), 40.0, 100, 101, np.arange(101), _ones(150, 101), (0, 100)),
    # c = 101: positions 0..100 are close; position 101 is far with nPoints = 102: stop after it.  102 = max(101, 100) + 1.
    _case("c_101", _close_far(101), 40.0, 100, 102, np.arange(102), _ones(151, 102), (0, 101)),
    # |D| = 0: vDepthIdx is empty, the function returns (:3109).
    _case("D_0", [-1.0, 0.0, -1.0], 40.0, 100, 0, [], [0, 0, 0], (0, 0)),
    # |D| = 1, far: visited (nPoints = 1 is not > 100), then the list ends.
    _case("D_1", [-1.0, 77.0], 40.0, 100, 1, [1], [0, 1], (0, 0)),
    # |D| = 100, all far: nPoints reaches 100, never > 100: all 100 visited.
    _case("D_100", 50.0 + np.arange(100), 40.0, 100, 100, np.arange(100), _ones(100, 100), (0, 0)),
    # |D| = 101, all far: the break fires at the last position, after visiting it: 101.
    _case("D_101", 50.0 + np.arange(101), 40.0, 100, 101, np.arange(101), _ones(101, 101), (0, 0)),
    # equal depths: pair<float,int> orders (1, 1) < (1, 3) < (2, 0) < (2, 2) < (2, 4): by slot within a depth.  All are < 40.
    _case("ties", [2.0, 1.0, 2.0, 1.0, 2.0], 40.0, 100, 5, [1, 3, 0, 2, 4], [1, 1, 1, 1, 1], (0, 5)),
    # max_points = 0 and depths 4, 5, 5, 6, 7 against th = 5: 5 > 5 is false, so positions 0..2 do not stop; position 3 (depth 6) is far
    # with nPoints = 4 > 0: stop after it.  4 visited, slot 4 (depth 7) is not.  Close (< 5, strict): only the 4.
    _case("equal_to_threshold", [5.0, 7.0, 4.0, 6.0, 5.0], 5.0, 0, 4, [2, 0, 4, 3], [1, 0, 1, 1, 1], (0, 1)),
    # +inf is a depth point (inf > 0) and sorts last; against th = +inf nothing is far (inf > inf is false): all visited, slot 1 first, the
    # two infinities by slot.  Close: depth < inf holds for the finite one alone.
    _case("inf_depth_inf_th", [INF, 1.0, INF], INF, 0, 3, [1, 0, 2], [1, 1, 1], (0, 1)),
    # the same depths against th = 10, max_points = 0: position 0 (depth 1) is close; position 1 (inf > 10, nPoints = 2 > 0) stops the walk
    # after slot 0 is visited; slot 2 is not.
    _case("inf_depth", [INF, 1.0, INF], 10.0, 0, 2, [1, 0], [1, 1, 0], (0, 1)),
    # NaN threshold: depth > NaN is false at every position, the walk never stops: all 150.  depth < NaN is false: no close point.
    _case("nan_threshold", 50.0 + np.arange(150), NAN, 100, 150, np.arange(150), _ones(150, 150), (0, 0)),
    # NaN, 0, -1, -0.0 and -inf are no depth points (z > 0 is false): D = {slot 4 (3.0), slot 6 (2.0)}, visited 6 then 4.
    _case("no_depth_values", [NAN, 0.0, -1.0, -0.0, 3.0, -INF, 2.0], 40.0, 100, 2, [6, 4], [0, 0, 0, 0, 1, 0, 1], (1, 1), tracked=[1, 1, 1, 1, 1, 1, 0]),
    # keeps_mp: slots 0 and 2 hold a MapPoint with observations: they are visited (order 1, 2, 0) but create nothing; slot 3 has keeps_mp
    # set and no depth: never visited.  tracked splits the close ones: slots 0 and 1 tracked, slot 2 not.
    _case("keeps_mp", [3.0, 1.0, 2.0, -1.0], 40.0, 100, 3, [1, 2, 0], [0, 1, 0, 0], (2, 1), keeps=[1, 0, 1, 1], tracked=[1, 1, 0, 1]),
    # max_points = 0, th = 2.5: 1 and 2 are close, 3 is far with nPoints = 3 > 0: stop after it; 4 is not visited.
    _case("max_points_0", [1.0, 2.0, 3.0, 4.0], 2.5, 0, 3, [0, 1, 2], [1, 1, 1, 0], (0, 2)),
    # max_points = 0 and nothing close: the first point is far with nPoints = 1 > 0: one visited.
    _case("max_points_0_all_far", [4.0, 2.0, 3.0], 0.5, 0, 1, [1], [0, 1, 0], (0, 0)),
    # a negative threshold: every depth point is far and none is close; max_points = 2 gives 3 visited.
    _case("negative_threshold", [4.0, 2.0, 3.0, 1.0], -1.0, 2, 3, [3, 1, 2], [0, 1, 1, 1], (0, 0)),
]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_known_answers(case):
    nv, order, create, ncreate = R.select(case["depth"], case["keeps"], case["th"], case["max_points"])
    assert nv == case["nvisit"] and np.array_equal(order, case["order"])
    assert np.array_equal(create, case["create"]) and ncreate == int(case["create"].sum())
    assert R.close_counts(case["depth"], case["tracked"], case["th"]) == case["close"]


def test_the_two_functions_use_100():
    """UpdateLastFrame's literal 100 (:3159) and CreateNewKeyFrame's maxPoint = 100 (:3697): the 101-point answer from both."""
    d = (50.0 + np.arange(150)).astype(F)
    for fn in (R.update_last_frame, R.create_new_keyframe):
        order, create = fn(d, None, 40.0)
        assert order == list(range(101)) and int(create.sum()) == 101


def test_closed_form_agrees_with_the_walk():
    """nvisit = min(|D|, max(c, max_points) + 1) with c = #{ d in D : !(d > th) }, on random rows with thresholds including NaN and inf."""
    rng = np.random.default_rng(11)
    for _ in range(300):
        n = int(rng.integers(0, 260))
        d = rng.choice(np.array([0.5, 1.0, 2.0, 3.0, 40.0, 41.0, 90.0, -1.0, 0.0, NAN, INF], F), n)
        th = float(rng.choice(np.array([0.0, 1.0, 2.5, 40.0, 90.0, NAN, INF, -3.0])))
        mp = int(rng.choice([0, 1, 5, 100, 300]))
        nv, order, create, _ = R.select(d, None, th, mp)
        D = d[d > 0]
        c = int(np.sum(~(D > F(th))))
        assert nv == min(len(D), max(c, mp) + 1)
        assert np.array_equal(order, np.array(sorted((float(z), i) for i, z in enumerate(d) if z > 0), np.float64).reshape(-1, 2)[:nv, 1].astype(np.int32))
