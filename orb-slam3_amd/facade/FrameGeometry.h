// FrameGeometry.h -- the Frame-level steps around the ORB hot path as drop-in helpers over the C ABI:
//   Frame::UndistortKeyPoints   (src/Frame.cc:924-970)   -> UndistortKeyPoints()
//   Frame::ComputeImageBounds   (src/Frame.cc:977-1021)  -> ComputeImageBounds()
//   Frame::isInFrustum for all local map points (src/Frame.cc:603-671, src/Tracking.cc:3808-3862) -> IsInFrustumBatch()
//   the pose rows of the batched device form orbm_is_in_frustum_batch_async (mRcwx, mtcwx, mOwx) -> FrustumPoseRow()
//   cvtColor(..., COLOR_*2GRAY) (src/Tracking.cc:1264-1290) -> see orbx_gray_from_color in include/orbx.h
//   Frame::ComputeStereoFromRGBD (src/Frame.cc:1279-1309) + the depth conversion of GrabImageRGBD (src/Tracking.cc:1353-1354) -> ComputeStereoFromRGBD()
//   Frame::UnprojectStereo for every keypoint (src/Frame.cc:1312-1326) -> UnprojectStereoAll()
//   the sorted walk over the depth points in Tracking::UpdateLastFrame / CreateNewKeyFrame (src/Tracking.cc:3094-3163, :3694-3783) -> SelectDepthPoints()
// The bodies only flatten the reference's containers into plain arrays; all arithmetic runs in liborbslam3_amd.so.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#ifdef ORBX_WITH_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvcompat.h"
#endif
#include "../../include/orbm.h"

namespace ORB_SLAM3 {

// mvKeysUn = undistort(mvKeys).  K = (fx, fy, cx, cy) of toK(); dist = mDistCoef (4 or 5 floats); newK = mK.
inline void UndistortKeyPoints(orbm_t* m, const std::vector<cv::KeyPoint>& keys, const float K[4], const std::vector<float>& dist,
                               const float newK[4], std::vector<cv::KeyPoint>& keysUn) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbm_kp_t), "cv::KeyPoint layout");
    keysUn.resize(keys.size());
    if (keys.empty()) return;
    const int rc = orbm_undistort_keypoints(m, ORBM_HOST, (const orbm_kp_t*)keys.data(), (int)keys.size(), K, dist.data(), (int)dist.size(), newK,
                                            (orbm_kp_t*)keysUn.data());
    if (rc < 0) throw std::runtime_error(std::string("orbm_undistort_keypoints: ") + orbm_last_error());
}

// mnMinX, mnMaxX, mnMinY, mnMaxY
inline void ComputeImageBounds(orbm_t* m, int cols, int rows, const float K[4], const std::vector<float>& dist, const float newK[4],
                               float& minX, float& maxX, float& minY, float& maxY) {
    float b[4];
    if (orbm_image_bounds(m, cols, rows, K, dist.data(), (int)dist.size(), newK, b) != ORBM_OK)
        throw std::runtime_error(std::string("orbm_image_bounds: ") + orbm_last_error());
    minX = b[0]; maxX = b[1]; minY = b[2]; maxY = b[3];
}

// One call for the loop `for (pMP : mvpLocalMapPoints) if (mCurrentFrame.isInFrustum(pMP, 0.5)) ...` (Tracking.cc:3838-3856).
// MapPointT supplies GetWorldPos2()/GetNormal2() as 3-float arrays and mfMinDistance/mfMaxDistance through the accessors
// passed in; the results are written back to the mTrack* members by the caller-supplied sink.
struct FrustumOut { std::vector<uint8_t> inView; std::vector<float> projX, projY, projXR, depth, viewCos; std::vector<int32_t> level; };
inline int IsInFrustumBatch(orbm_t* m, const std::vector<float>& Pw3, const std::vector<float>& normal3, const std::vector<float>& minDist,
                            const std::vector<float>& maxDist, const float Rcw[9], const float tcw[3], const float Ow[3], const float K[4],
                            const float bounds[4], float bf, float viewingCosLimit, float logScaleFactor, int nScaleLevels, FrustumOut& out) {
    const int n = (int)minDist.size();
    out.inView.assign(n, 0); out.projX.assign(n, -1.f); out.projY.assign(n, -1.f); out.projXR.assign(n, 0.f); out.depth.assign(n, 0.f);
    out.viewCos.assign(n, 0.f); out.level.assign(n, -1);
    if (n == 0) return 0;
    const int rc = orbm_is_in_frustum(m, ORBM_HOST, n, Pw3.data(), normal3.data(), minDist.data(), maxDist.data(), Rcw, tcw, Ow, K, bounds, bf,
                                      viewingCosLimit, logScaleFactor, nScaleLevels, out.inView.data(), out.projX.data(), out.projY.data(),
                                      out.projXR.data(), out.depth.data(), out.level.data(), out.viewCos.data());
    if (rc < 0) throw std::runtime_error(std::string("orbm_is_in_frustum: ") + orbm_last_error());
    return rc;
}

// One frame's row of the pose arrays orbm_is_in_frustum_batch_async reads, from the members Frame::isInFrustum uses (Frame.cc:621, :651):
// tcwRow[12] = the row-major 3x4 [mRcwx | mtcwx], owRow[3] = mOwx -- the very floats IsInFrustumBatch hands over as Rcw, tcw and Ow.
// Upload row f to tcw + 12 * f and ow + 3 * f; a captured step then follows the frame's pose.  Pinhole frames (Nleft == -1) only: the
// fisheye isInFrustum (KannalaBrandt8::project) stays with the caller.
inline void FrustumPoseRow(const cv::Matx33f& Rcw, const cv::Matx31f& tcw, const cv::Matx31f& Ow, float tcwRow[12], float owRow[3]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) tcwRow[4 * r + c] = Rcw(r, c);
        tcwRow[4 * r + 3] = tcw(r);
        owRow[r] = Ow(r);
    }
}
template <class FrameT> inline void FrustumPoseRow(const FrameT& F, float tcwRow[12], float owRow[3]) {
    FrustumPoseRow(F.mRcwx, F.mtcwx, F.mOwx, tcwRow, owRow);
}

// mvuRight, mvDepth of an RGB-D frame from the UNCONVERTED depth image and mDepthMapFactor: the caller drops its own
// imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (Tracking.cc:1353-1354; the conversion is applied to the sampled pixels), or
// passes the converted CV_32F image with factor 1.  depthType = ORBM_DEPTH_U16 | ORBM_DEPTH_F32, stepBytes = imDepth.step.
// Returns the number of keypoints with depth.
inline int ComputeStereoFromRGBD(orbm_t* m, const std::vector<cv::KeyPoint>& keys, const std::vector<cv::KeyPoint>& keysUn,
                                 const void* depth, int depthType, int cols, int rows, size_t stepBytes, float depthMapFactor, float bf,
                                 std::vector<float>& uRight, std::vector<float>& vDepth) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbm_kp_t), "cv::KeyPoint layout");
    if (keysUn.size() != keys.size()) throw std::runtime_error("ComputeStereoFromRGBD: mvKeys and mvKeysUn differ in size");
    uRight.assign(keys.size(), -1.f); vDepth.assign(keys.size(), -1.f);               // Frame.cc:1284-1285
    if (keys.empty()) return 0;
    const int rc = orbm_stereo_from_rgbd(m, (int)keys.size(), (const orbm_kp_t*)keys.data(), (const orbm_kp_t*)keysUn.data(), depth, depthType, cols, rows,
                                         (int)stepBytes, depthMapFactor, bf, uRight.data(), vDepth.data());
    if (rc < 0) throw std::runtime_error(std::string("orbm_stereo_from_rgbd: ") + orbm_last_error());
    return rc;
}
#ifdef ORBX_WITH_OPENCV
inline int ComputeStereoFromRGBD(orbm_t* m, const std::vector<cv::KeyPoint>& keys, const std::vector<cv::KeyPoint>& keysUn, const cv::Mat& imDepth,
                                 float depthMapFactor, float bf, std::vector<float>& uRight, std::vector<float>& vDepth) {
    if (imDepth.type() != CV_16UC1 && imDepth.type() != CV_32FC1) throw std::runtime_error("ComputeStereoFromRGBD: the depth image must be CV_16UC1 or CV_32FC1");
    return ComputeStereoFromRGBD(m, keys, keysUn, imDepth.data, imDepth.type() == CV_32FC1 ? ORBM_DEPTH_F32 : ORBM_DEPTH_U16, imDepth.cols, imDepth.rows,
                                 imDepth.step, depthMapFactor, bf, uRight, vDepth);
}
#endif

// One call for `for (i < N) x3D = UnprojectStereo(i)` (Tracking.cc: StereoInitialization, UpdateLastFrame, CreateNewKeyFrame).
// Rwc / Ow = mRwc (row-major) / mOw, K = (fx, fy, cx, cy).  x3Dw holds 3 floats per keypoint; hasDepth[i] = 0 (and a zero point) where the
// reference returns an empty Mat.  Returns the number of points.
inline int UnprojectStereoAll(orbm_t* m, const std::vector<cv::KeyPoint>& keysUn, const std::vector<float>& vDepth, const float Rwc[9], const float Ow[3],
                              const float K[4], std::vector<float>& x3Dw, std::vector<uint8_t>& hasDepth) {
    if (vDepth.size() != keysUn.size()) throw std::runtime_error("UnprojectStereoAll: mvKeysUn and mvDepth differ in size");
    x3Dw.assign(3 * keysUn.size(), 0.f); hasDepth.assign(keysUn.size(), 0);
    if (keysUn.empty()) return 0;
    const float twc[12] = {Rwc[0], Rwc[1], Rwc[2], Ow[0], Rwc[3], Rwc[4], Rwc[5], Ow[1], Rwc[6], Rwc[7], Rwc[8], Ow[2]};
    const int rc = orbm_unproject_stereo(m, (int)keysUn.size(), (const orbm_kp_t*)keysUn.data(), vDepth.data(), twc, K, x3Dw.data(), hasDepth.data());
    if (rc < 0) throw std::runtime_error(std::string("orbm_unproject_stereo: ") + orbm_last_error());
    return rc;
}

// The walk `sort(vDepthIdx); for (j ...) { ...; if (vDepthIdx[j].first > mThDepth && nPoints > 100) break; }` of Tracking::UpdateLastFrame
// (Tracking.cc:3094-3163) and Tracking::CreateNewKeyFrame (:3694-3783) in one call.  keepsMp[i] = `pMP && pMP->Observations() >= 1` for
// mvpMapPoints[i] (empty = no slot holds one); maxPoints = the reference's 100.  order = the visited slots, closest first, equal depths by
// slot; createNew[i] = 1 where the walk creates a MapPoint.  Returns the number of visited slots (order.size()).
// Recipe, both functions:
//     UnprojectStereoAll(m, mvKeysUn, mvDepth, Rwc, Ow, K, x3Dw, hasDepth);
//     SelectDepthPoints(m, mvDepth, keepsMp, mThDepth, 100, order, createNew);
//     for (int i : order) if (createNew[i]) { x3D = x3Dw[3 * i .. 3 * i + 2]; ... }
//   UpdateLastFrame:   pNewMP = new MapPoint(x3D, pMap, &mLastFrame, i); mLastFrame.mvpMapPoints[i] = pNewMP; mlpTemporalPoints.push_back(pNewMP);
//   CreateNewKeyFrame: pNewMP = new MapPoint(x3D, pKF, pMap) and the map surgery of :3750-3767 (AddObservation, AddMapPoint,
//                      ComputeDistinctiveDescriptors, UpdateNormalAndDepth, the Atlas); a slot whose MapPoint has no observation is cleared
//                      first (:3735).  With Nleft != -1 the UnprojectStereoFishEye point and the mvLeftToRightMatch partner stay with the caller.
// Creating in `order` keeps the MapPoint ids in the reference's sequence.
inline int SelectDepthPoints(orbm_t* m, const std::vector<float>& vDepth, const std::vector<uint8_t>& keepsMp, float thDepth, int maxPoints,
                             std::vector<int>& order, std::vector<uint8_t>& createNew) {
    if (!keepsMp.empty() && keepsMp.size() != vDepth.size()) throw std::runtime_error("SelectDepthPoints: mvDepth and keepsMp differ in size");
    order.assign(vDepth.size(), -1); createNew.assign(vDepth.size(), 0);
    if (vDepth.empty()) return 0;
    static_assert(sizeof(int) == sizeof(int32_t), "int is 32 bits");
    const int rc = orbm_select_depth_points(m, (int)vDepth.size(), vDepth.data(), keepsMp.empty() ? nullptr : keepsMp.data(), nullptr, thDepth, maxPoints,
                                            (int32_t*)order.data(), createNew.data(), nullptr, nullptr, nullptr);
    if (rc < 0) throw std::runtime_error(std::string("orbm_select_depth_points: ") + orbm_last_error());
    order.resize(rc);
    return rc;
}

}  // namespace ORB_SLAM3
