"""Hand-computed known answers for tests/second_reading_rgbd.py, the yardstick of the RGB-D entry points (tests/test_gpu_rgbd.py).
Every expected value below is worked out in the comment beside it from the reference's lines, not taken from any code.  No GPU."""
import numpy as np

import second_reading_rgbd as R

F = np.float32
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def _kps(xy):
    k = np.zeros(len(xy), KP)
    k["x"] = [p[0] for p in xy]; k["y"] = [p[1] for p in xy]
    return k


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def test_u16_5000_at_tum_factor_is_one_metre():
    """TUM: DepthMapFactor 5000 -> mDepthMapFactor = 1.0f / 5000.  5000 * (1.0f / 5000) rounds to exactly 1 in float32 (the product
    5000 * fl(1/5000) is within half an ulp of 1), so d = 1 and uright = x - mbf / 1 = x - mbf."""
    img = np.zeros((8, 8), np.uint16); img[3, 2] = 5000
    k = _kps([(2.0, 3.0)])
    factor = F(1.0) / F(5000.0)
    ur, dp, n = R.compute_stereo_from_rgbd(k, k, img, factor, 40.0)
    assert n == 1 and dp[0] == F(1.0) and ur[0] == F(2.0 - 40.0)


def test_truncation_reads_row_20_column_10():
    """(10.9, 20.9): (int)20.9 = 20, (int)10.9 = 10 -- not the rounded pixel (21, 11)."""
    img = np.zeros((32, 32), np.float32); img[20, 10] = 2.0; img[21, 11] = 7.0
    k = _kps([(10.9, 20.9)])
    ur, dp, n = R.compute_stereo_from_rgbd(k, k, img, 1.0, 8.0)
    assert n == 1 and dp[0] == F(2.0) and ur[0] == F(F(10.9) - F(4.0))
    # truncation is towards zero: (-0.5, -0.5) reads pixel (0, 0); -1.0 is outside
    img[0, 0] = 4.0
    ur, dp, n = R.compute_stereo_from_rgbd(_kps([(-0.5, -0.5), (-1.0, 3.0), (3.0, 32.0)]), _kps([(5.0, 5.0)] * 3), img, 1.0, 8.0)
    assert n == 1 and dp.tolist() == [4.0, -1.0, -1.0] and ur.tolist() == [3.0, -1.0, -1.0]


def test_undistorted_x_enters_uright_raw_xy_pick_the_pixel():
    img = np.zeros((8, 8), np.float32); img[1, 6] = 2.0; img[5, 5] = 4.0
    raw = _kps([(6.0, 1.0)]); un = _kps([(5.0, 5.0)])
    ur, dp, _ = R.compute_stereo_from_rgbd(raw, un, img, 1.0, 1.0)
    assert dp[0] == F(2.0) and ur[0] == F(5.0 - 0.5)


def test_zero_negative_nan_and_inf_depths():
    """d > 0 fails for 0, a negative and NaN: -1 / -1.  +inf passes: mbf / inf = 0, uright = x."""
    img = np.array([[0.0, -2.5, np.nan, np.inf, 1.0]], np.float32)
    k = _kps([(c, 0.0) for c in range(5)])
    ur, dp, n = R.compute_stereo_from_rgbd(k, k, img, 1.0, 3.0)
    assert n == 2
    assert np.array_equal(_bits(dp), _bits([-1, -1, -1, np.inf, 1]))
    assert np.array_equal(_bits(ur), _bits([-1, -1, -1, 3.0, 4.0 - 3.0]))
    # a NaN coordinate reads nothing
    k2 = _kps([(np.nan, 0.0), (4.0, np.nan)])
    ur, dp, n = R.compute_stereo_from_rgbd(k2, k2, img, 1.0, 3.0)
    assert n == 0 and np.all(ur == -1) and np.all(dp == -1)


def test_f32_factor_within_1e5_of_one_is_passed_through():
    """fl32(1 + 5e-6) = 1 + 42 * 2^-23 = 1.0000050068: |f - 1| = 5.0068e-6 is not > 1e-5, so an F32 image is NOT converted and the
    pixel 3.0 stays 3.0.  fl32(1 + 2e-5) = 1 + 168 * 2^-23: |f - 1| = 2.0027e-5 > 1e-5, so 3.0 becomes 3 * (1 + 168 * 2^-23) =
    3 + 504 * 2^-23 = 3 + 252 * 2^-22, representable (ulp of 3 is 2^-22): exactly 3.00006008148193359375."""
    img = np.full((2, 2), 3.0, np.float32)
    k = _kps([(0.0, 0.0)])
    f1 = F(1.0 + 5e-6); f2 = F(1.0 + 2e-5)
    assert float(f1) == 1.0 + 42 * 2.0 ** -23 and float(f2) == 1.0 + 168 * 2.0 ** -23
    assert not R.needs_conversion(True, f1) and R.needs_conversion(True, f2) and R.needs_conversion(False, f1)
    assert R.compute_stereo_from_rgbd(k, k, img, f1, 1.0)[1][0] == F(3.0)
    assert float(R.compute_stereo_from_rgbd(k, k, img, f2, 1.0)[1][0]) == 3.0 + 252 * 2.0 ** -22


def test_u16_always_goes_through_the_multiply():
    """type != CV_32F converts whatever the factor: factor 1 gives (float)raw; the near-one factor that F32 passes through scales a U16
    pixel: 3 * (1 + 42 * 2^-23) = 3 + 126 * 2^-23 = 3 + 63 * 2^-22, representable."""
    img = np.array([[3, 65535]], np.uint16)
    k = _kps([(0.0, 0.0), (1.0, 0.0)])
    assert R.compute_stereo_from_rgbd(k, k, img, 1.0, 1.0)[1].tolist() == [3.0, 65535.0]
    assert float(R.compute_stereo_from_rgbd(k, k, img, F(1.0 + 5e-6), 1.0)[1][0]) == 3.0 + 63 * 2.0 ** -22
    # 65535 * 0.5 = 32767.5 exactly; uright = 1 - 10 / 32767.5
    ur, dp, _ = R.compute_stereo_from_rgbd(k, k, img, 0.5, 10.0)
    assert dp[1] == F(32767.5) and ur[1] == F(F(1.0) - F(F(10.0) / F(32767.5)))


def test_unproject_identity_pose():
    """fx = fy = 2 (invfx = 0.5 exactly), cx = 10, cy = 20, keypoint (14, 26), z = 3: x = (14 - 10) * 3 * 0.5 = 6, y = (26 - 20) * 3 *
    0.5 = 9; Rwc = I, Ow = (1, 2, 3) -> (7, 11, 6).  Slots with depth -1, 0 and NaN have no point."""
    un = _kps([(14.0, 26.0)] * 4)
    T = np.array([1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3], F)
    x, has = R.unproject_stereo(un, np.array([3.0, -1.0, 0.0, np.nan], F), T, (2.0, 2.0, 10.0, 20.0))
    assert has.tolist() == [1, 0, 0, 0]
    assert x[0].tolist() == [7.0, 11.0, 6.0] and not x[1:].any()


def test_unproject_rotated_90_degrees_about_z():
    """Rwc = Rz(90 deg) = [[0, -1, 0], [1, 0, 0], [0, 0, 1]], Ow = 0: the camera point (6, 9, 3) of the previous case becomes (-9, 6, 3)."""
    un = _kps([(14.0, 26.0)])
    T = np.array([0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0], F)
    x, has = R.unproject_stereo(un, np.array([3.0], F), T, (2.0, 2.0, 10.0, 20.0))
    assert has[0] == 1 and x[0].tolist() == [-9.0, 6.0, 3.0]


def test_mat_product_rounds_once():
    """The cv::Mat rule: 1e8 + 1 - 1e8 summed in double is 1; a float accumulator (the Matx rule) would lose the 1."""
    assert R.mat_product_row(np.array([1, 1, 1], F), np.array([1e8, 1.0, -1e8], F)) == F(1.0)
