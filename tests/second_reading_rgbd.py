"""A second, independent reading of the reference's RGB-D frame steps, in plain Python / numpy.

Written from the reference's Frame.cc (ComputeStereoFromRGBD :1279-1309, UnprojectStereo :1312-1326), Tracking.cc (GrabImageRGBD's
depth conversion :1353-1354) and the cv::Mat product rule of facade/cvcompat.h alone: it imports no product code and no oracle.  One
reference function is one function here and cites the lines it restates.  The loops are scalar on purpose -- one keypoint, one line of
the reference at a time; the test shapes are small.

Arithmetic follows the C++ operand types: every float operation is one np.float32 operation (no contraction), a float compared with a
double literal is promoted, (int)float truncates towards zero.
"""
import math

import numpy as np

F = np.float32
F64 = np.float64

DEPTH_U16, DEPTH_F32 = 0, 1


def needs_conversion(depth_is_f32, depth_factor):
    """Tracking.cc:1353: `(fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F` -- a float difference, its absolute value
    promoted to double against the double literal."""
    diff = F(depth_factor) - F(1.0)
    return bool(float(abs(diff)) > 1e-5) or not depth_is_f32


def convert_pixel(raw, depth_is_f32, depth_factor):
    """Tracking.cc:1354 for one pixel: imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) = saturate_cast<float>(raw * alpha + 0) with
    alpha applied in float: one float32 multiply ((float)raw is exact for 16-bit values; a multiply-add with a zero addend rounds as the
    multiply alone).  Without the conversion the float pixel is used as it is."""
    with np.errstate(all="ignore"):
        if needs_conversion(depth_is_f32, depth_factor):
            return F(F(raw) * F(depth_factor))
        return F(raw)


def pixel_index(c, limit):
    """(int)c of Mat::at<float>(float, float)'s arguments (Frame.cc:1300), or None where the reference would read outside the image
    (index outside [0, limit), or a NaN, whose conversion is undefined)."""
    c = float(c)
    if math.isnan(c) or math.isinf(c):
        return None
    i = int(c)                                                           # truncation towards zero, as the C++ conversion
    return i if 0 <= i < limit else None


def compute_stereo_from_rgbd(kps, kps_un, img, depth_factor, mbf):
    """Frame.cc:1279-1309.  kps = mvKeys, kps_un = mvKeysUn (records with x, y), img = the UNCONVERTED 2-D depth image (uint16 or
    float32).  Returns (mvuRight, mvDepth, number of keypoints with depth)."""
    n = len(kps)
    h, w = img.shape
    is_f32 = img.dtype == np.float32
    assert is_f32 or img.dtype == np.uint16
    mbf = F(mbf)
    uright = np.full(n, -1, F)                                           # :1284
    depth = np.full(n, -1, F)                                            # :1285
    cnt = 0
    with np.errstate(all="ignore"):
        for i in range(n):                                               # :1288
            v = kps[i]["y"]; u = kps[i]["x"]                             # :1296-1297, the RAW keypoint
            row = pixel_index(v, h); col = pixel_index(u, w)
            if row is None or col is None:
                continue                                                 # out of the image: the contract's -1 / -1
            d = convert_pixel(img[row, col], is_f32, depth_factor)       # :1300 on the converted image
            if d > 0:                                                    # :1303
                depth[i] = d                                             # :1305
                uright[i] = F(F(kps_un[i]["x"]) - F(mbf / d))            # :1306
                cnt += 1
    return uright, depth, cnt


def mat_product_row(r, x):
    """One element of a cv::Mat product under facade/cvcompat.h: a double sum from 0, in k order, of exact double products, rounded
    once to float."""
    s = F64(0)
    for k in range(len(r)):
        s = s + F64(r[k]) * F64(x[k])
    return F(s)


def unproject_stereo(kps_un, depth, twc, k):
    """Frame.cc:1312-1326 for every keypoint.  twc = row-major 3x4 [mRwc | mOw], k = (fx, fy, cx, cy).  Returns (x3Dw [n][3],
    has_depth [n]): where the reference returns an empty Mat the row is (0, 0, 0) and has_depth 0."""
    T = np.asarray(twc, F).reshape(3, 4)
    fx, fy, cx, cy = (F(a) for a in k)
    invfx = F(F(1.0) / fx); invfy = F(F(1.0) / fy)                       # Frame.cc:301-302
    n = len(kps_un)
    x3dw = np.zeros((n, 3), F); has = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for i in range(n):
            z = F(depth[i])                                              # :1314
            if z > 0:                                                    # :1315
                u = F(kps_un[i]["x"]); v = F(kps_un[i]["y"])             # :1317-1318
                x = F(F(F(u - cx) * z) * invfx)                          # :1319
                y = F(F(F(v - cy) * z) * invfy)                          # :1320
                c = (x, y, z)                                            # :1321
                for r in range(3):                                       # :1322, mRwc * x3Dc + mOw
                    x3dw[i, r] = F(mat_product_row(T[r, :3], c) + T[r, 3])
                has[i] = 1
    return x3dw, has
