"""Hand-worked known answers for tests/second_reading_mappoint.py (no GPU): the yardstick of tests/test_gpu_mappoint.py."""
import numpy as np

import second_reading_mappoint as R

F = np.float32


def _flip(base, bits):
    d = np.array(base, np.uint8).copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


A = np.arange(32, dtype=np.uint8) * 7 + 3


def test_descriptor_distance():
    assert R.descriptor_distance(A, A) == 0 and R.descriptor_distance(A, ~A) == 256
    assert R.descriptor_distance(A, _flip(A, [0, 9, 255])) == 3


def test_n1_and_n2_choose_entry_0():
    """The median index is (int)(0.5 * (N - 1)) = 0 for N = 1 and N = 2: the self distance 0 in every row, so row 0 wins."""
    assert R.compute_distinctive([A]) == (0, 0)
    assert R.compute_distinctive([A, _flip(A, range(40))]) == (0, 0)
    assert R.compute_distinctive([]) == (-1, -1)


def test_n3_and_n4_lower_median():
    # N = 3, index 1: rows (0, 10, 30) (0, 10, 20) (0, 20, 30) -> medians 10, 10, 20 -> the first 10
    d0, d1, d2 = A, _flip(A, range(10)), _flip(A, range(10, 40))
    assert R.descriptor_distance(d1, d2) == 40
    # rows: d0: 0 10 30 -> 10; d1: 0 10 40 -> 10; d2: 0 30 40 -> 30
    assert R.compute_distinctive([d0, d1, d2]) == (0, 10)
    assert R.compute_distinctive([d2, d1, d0]) == (1, 10)
    # N = 4, index (int)1.5 = 1, the LOWER median: x = A, y = 4 bits, z = 4 + 6 bits, w = 100 other bits
    x, y, z, w = A, _flip(A, range(4)), _flip(A, range(10)), _flip(A, range(100, 200))
    # rows sorted: x: 0 4 10 100 -> 4; y: 0 4 6 104 -> 4; z: 0 6 10 110 -> 6; w: 0 100 104 110 -> 100 (the upper median would give 10, 6, 10, 104)
    assert R.compute_distinctive([x, y, z, w]) == (0, 4)
    assert R.compute_distinctive([z, w, y, x]) == (2, 4)


def test_three_equal_is_a_tie_for_entry_0():
    assert R.compute_distinctive([A, A.copy(), A.copy()]) == (0, 0)


def test_complement_distance_256_survives():
    """A, ~A, ~A: rows (0, 256, 256) (0, 0, 256) (0, 0, 256) -> medians 256, 0, 0 -> entry 1.  Distances wrapped to 8 bits would read
    (0, 0, 0) in row 0 and answer entry 0."""
    assert R.compute_distinctive([A, ~A, ~A]) == (1, 0)


def test_two_clusters_tie_the_earlier_wins():
    """Clusters {p, p+2 bits, p+4 bits} and {q, q+2 bits, q+4 bits}, far apart, interleaved: N = 6, median index 2.  The rows of p+2 and
    q+2 hold (0, 2, 2, far...) -> median 2; p, p+4, q, q+4 hold (0, 2, 4, far...) -> median 4.  The first row of median 2 wins."""
    p = A; q = _flip(A, range(100, 220))
    p2, p4, q2, q4 = _flip(p, [0, 1]), _flip(p, [0, 1, 2, 3]), _flip(q, [8, 9]), _flip(q, [8, 9, 10, 11])
    assert R.compute_distinctive([q, p, q2, p2, q4, p4]) == (2, 2)
    assert R.compute_distinctive([q, p, p2, q2, q4, p4]) == (2, 2)
    assert R.compute_distinctive([p4, q4, p, q, p2, q2]) == (4, 2)


def _pool():
    kps = np.zeros((3, 4), [("x", F), ("y", F), ("size", F), ("angle", F), ("response", F), ("octave", np.int32), ("class_id", np.int32)])
    kps["octave"] = [[0, 1, 2, 3], [1, 1, 1, 1], [2, 0, 7, 9]]
    desc = np.zeros((3, 4, 32), np.uint8)
    desc[0, 0] = A; desc[1, 1] = ~A; desc[2, 2] = ~A; desc[2, 0] = _flip(A, [5])
    counts = np.array([4, 2, 3], np.int32)
    ow_l = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], F); ow_r = ow_l + F(0.5)
    return kps, desc, counts, ow_l, ow_r


def test_bad_keyframe_entry_is_skipped_by_the_descriptor_but_counted_by_the_normal():
    kps, desc, counts, ow_l, ow_r = _pool()
    off = np.array([0, 3], np.int32); row = np.array([0, 1, 2], np.int32); slot = np.array([0, 1, 2], np.int32)
    sf = np.array([1.0, 1.2, 1.44], F)
    pw = np.array([[0.5, 0.25, 4.0]], F)
    keep = np.full((1, 32), 0xAB, np.uint8)
    for flags, want_obs in (([0, 0, 0], 1), ([0, R.BAD_KF, 0], 0), ([R.BAD_KF, 0, 0], 1)):
        fl = np.array(flags, np.uint8)
        d, bo, bm = R.distinctive_batch(desc, counts, off, row, slot, fl, None, keep)
        assert bo[0] == want_obs and bm[0] == 0 and np.array_equal(d[0], desc[row[want_obs], slot[want_obs]])
        n, mn, mx, up = R.normal_depth_batch(kps, counts, ow_l, ow_r, off, row, slot, fl, None, pw, [0], [1], sf, np.zeros((1, 3)), [0], [0])
        assert up[0] == 1
        e = R.update_normal_and_depth(pw[0], [ow_l[0], ow_l[1], ow_l[2]], ow_l[0], 1, sf)       # all three, whatever the flags say
        assert np.array_equal(n[0].view(np.uint32), e[0].view(np.uint32)) and mn[0] == e[1] and mx[0] == e[2]
    # every entry bad: no descriptor, the caller's bytes stay; an entry outside the row's count is skipped by both
    d, bo, bm = R.distinctive_batch(desc, counts, off, row, slot, np.full(3, R.BAD_KF, np.uint8), None, keep)
    assert bo[0] == -1 and bm[0] == -1 and np.all(d == 0xAB)
    slot2 = np.array([0, 2, 2], np.int32)                                   # row 1 holds 2 slots
    d, bo, bm = R.distinctive_batch(desc, counts, off, row, slot2, np.zeros(3, np.uint8), None, keep)
    assert bo[0] == 0 and bm[0] == 0                                        # N = 2: A and ~A, entry 0
    n, mn, mx, up = R.normal_depth_batch(kps, counts, ow_l, ow_r, off, row, slot2, np.zeros(3, np.uint8), None, pw, [0], [1], sf, np.zeros((1, 3)), [0], [0])
    e = R.update_normal_and_depth(pw[0], [ow_l[0], ow_l[2]], ow_l[0], 1, sf)
    assert np.array_equal(n[0].view(np.uint32), e[0].view(np.uint32))


def test_right_camera_entry_uses_ow_r_and_known_values():
    """pw = (3, 0, 4) seen from the origin: d = (3, 0, 4), norm 5, s = 0.2f; one observation: normal = d * s / 1."""
    sf = np.array([1.0, 1.2, 1.44], F)
    n, mn, mx = R.update_normal_and_depth([3, 0, 4], [[0, 0, 0]], [0, 0, 0], 1, sf)
    assert np.array_equal(n, np.array([3, 0, 4], F) * F(0.2)) and mx == F(5) * F(1.2) and mn == F(F(5) * F(1.2)) / F(1.44)
    kps, desc, counts, ow_l, ow_r = _pool()
    off = np.array([0, 1], np.int32); row = np.array([1], np.int32); slot = np.array([0], np.int32)
    pw = np.array([[3.5, 0.5, 4.5]], F)                                     # ow_r[1] = (1.5, 0.5, 0.5): d = (2, 0, 4)
    args = (pw, [1], [0], sf, np.zeros((1, 3)), [0], [0])
    nr = R.normal_depth_batch(kps, counts, ow_l, ow_r, off, row, slot, np.array([R.RIGHT], np.uint8), None, *args)
    nl = R.normal_depth_batch(kps, counts, ow_l, ow_r, off, row, slot, np.array([0], np.uint8), None, *args)
    s = F(1.0 / np.sqrt(20.0))
    assert np.array_equal(nr[0][0], np.array([2, 0, 4], F) * s) and not np.array_equal(nr[0][0], nl[0][0])
    assert nr[2][0] == nl[2][0]                                             # dist is always taken to the LEFT centre of the reference KeyFrame (:624)
    assert nr[2][0] == F(F(np.sqrt(2.5 * 2.5 + 0.5 * 0.5 + 4.5 * 4.5)) * sf[1])
    none = R.normal_depth_batch(kps, counts, ow_l, None, off, row, slot, np.array([R.RIGHT], np.uint8), None, *args)
    assert none[3][0] == 0                                                  # no right centres: the entry is skipped, n = 0


def test_gates_leave_rows_untouched():
    kps, desc, counts, ow_l, ow_r = _pool()
    off = np.array([0, 1], np.int32); row = np.array([0], np.int32); slot = np.array([0], np.int32); fl = np.zeros(1, np.uint8)
    sf = np.array([1.0, 1.2, 1.44], F); pw = np.array([[1, 2, 3]], F)
    keep = (np.full((1, 3), 7, F), np.array([8], F), np.array([9], F))
    for valid, rr, rs in (([0], 0, 0), (None, 3, 0), (None, -1, 0), (None, 1, 2), (None, 0, -1), (None, 0, 3), (None, 2, 2)):   # [0][3] and [2][2]: octaves 3 and 7
        n, mn, mx, up = R.normal_depth_batch(kps, counts, ow_l, ow_r, off, row, slot, fl, valid, pw, [rr], [rs], sf, *keep)
        assert up[0] == 0 and np.all(n == 7) and mn[0] == 8 and mx[0] == 9, (valid, rr, rs)
    n, mn, mx, up = R.normal_depth_batch(kps, counts, ow_l, ow_r, off, row, slot, fl, None, pw, [0], [2], sf, *keep)
    assert up[0] == 1 and mx[0] == F(F(np.sqrt(14.0)) * sf[2])
    for bad_off in ([1, 1], [1, 0], [0, 2], [-1, 1]):                       # empty, decreasing, past nobs, negative
        n, mn, mx, up = R.normal_depth_batch(kps, counts, ow_l, ow_r, np.array(bad_off, np.int32), row, slot, fl, None, pw, [0], [2], sf, *keep)
        assert up[0] == 0
        d, bo, bm = R.distinctive_batch(desc, counts, np.array(bad_off, np.int32), row, slot, fl, None, np.zeros((1, 32), np.uint8))
        assert bo[0] == -1


def test_normal_depends_on_entry_order():
    """Float addition is not associative: the same three centres in two orders give different bits."""
    pw = np.array([0.3, -0.2, 5.1], F)
    rng = np.random.default_rng(4)
    sf = np.array([1.0, 1.2], F)
    seen = 0
    for _ in range(200):
        c = rng.uniform(-2, 2, (3, 3)).astype(F)
        a = R.update_normal_and_depth(pw, [c[0], c[1], c[2]], c[0], 0, sf)[0]
        b = R.update_normal_and_depth(pw, [c[2], c[1], c[0]], c[0], 0, sf)[0]
        assert np.allclose(a, b, atol=1e-6)
        seen += not np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert seen > 0
