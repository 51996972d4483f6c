// PoseOptimization.h -- Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:943-1286) as a drop-in template over the host form
// orbm_pose_optimization of include/orbm.h:
//   int nGood = PoseOptimization(matcher, &mCurrentFrame);       // Tracking.cc:3027, :3237, :3339, :4292, :4320, :4345
// flattens the frame -- mvpMapPoints[i]->GetWorldPos(), mvKeysUn, mvuRight, mvInvLevelSigma2, mTcw, fx .. cy, mbf -- runs the four rounds of
// Levenberg-Marquardt in ONE kernel launch, writes mvbOutlier for the slots that hold a MapPoint, calls SetPose with the optimised pose and
// returns nInitialCorrespondences - nBad.  With fewer than 3 correspondences it returns 0, clears those flags and leaves the pose alone, as
// the reference does.  The result is the library's own arithmetic (csrc/orbm_poseopt.h): within the tolerance DESIGN section 8 states of
// g2o's, not bit-identical to it.
//
// Scope: !pFrame->mpCamera2 -- pinhole, Nleft == -1, mono and stereo edges.  A frame with a second camera (the fisheye rig,
// EdgeSE3ProjectXYZOnlyPoseToBody, Optimizer.cc:1085-1152) is REFUSED with std::runtime_error: the facade does not guess.  The discard
// loops that follow each call in Tracking.cc stay in the reference's text here (they walk host vectors); a caller whose frames live on
// the device uses orbm_pose_optimization_batch_async and orbm_discard_outliers_batch_async directly.
//
// FrameT: N, mvpMapPoints, mvKeysUn, mvuRight, mvInvLevelSigma2, mTcw (4x4 CV_32F), fx, fy, cx, cy, mbf, mpCamera2, mvbOutlier,
// SetPose(cv::Mat).  MapPointT: GetWorldPos() -> 3x1 CV_32F.  matcher: anything with handle() -> orbm_t* (facade/ORBmatcher.h), or the
// orbm_t* itself.
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
namespace poseopt {

// The arrays of one call: one frame, cap = max(N, 1) slots.
struct Flat {
    int n = 0, cap = 1, nmp = 1, nlevels = 0;
    std::vector<orbm_kp_t> kps;
    std::vector<float> uright, pw, ils2;
    std::vector<int32_t> qMp;
    float tcw[12], k[4], bf = 0.f;
    bool haveUright = false;

    template <class FrameT> void build(const FrameT& F) {
        if (F.mpCamera2) throw std::runtime_error("PoseOptimization: a frame with a second camera (mpCamera2, fisheye rig) is outside this call: "
                                                  "Optimizer.cc:1085-1152 stays with the caller");
        n = F.N; cap = n > 0 ? n : 1;
        static_assert(sizeof(cv::KeyPoint) == sizeof(orbm_kp_t), "cv::KeyPoint layout");
        kps.assign(cap, orbm_kp_t());
        for (int i = 0; i < n; ++i) kps[i] = *(const orbm_kp_t*)&F.mvKeysUn[i];
        haveUright = (int)F.mvuRight.size() >= n && n > 0;
        uright.assign(cap, -1.f);
        for (int i = 0; i < n && haveUright; ++i) uright[i] = F.mvuRight[i];
        qMp.assign(cap, -1); pw.clear();
        for (int i = 0; i < n; ++i) {
            if (!F.mvpMapPoints[i]) continue;
            const cv::Mat Xw = F.mvpMapPoints[i]->GetWorldPos();            // the position as this slot's edge reads it: one pool row per slot
            qMp[i] = (int32_t)(pw.size() / 3);
            pw.push_back(Xw.template at<float>(0)); pw.push_back(Xw.template at<float>(1)); pw.push_back(Xw.template at<float>(2));
        }
        nmp = (int)(pw.size() / 3);
        if (nmp == 0) { pw.assign(3, 0.f); nmp = 1; }
        ils2.assign(F.mvInvLevelSigma2.begin(), F.mvInvLevelSigma2.end());
        nlevels = (int)ils2.size();
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) tcw[4 * r + c] = F.mTcw.template at<float>(r, c);
        k[0] = F.fx; k[1] = F.fy; k[2] = F.cx; k[3] = F.cy; bf = F.mbf;
    }
};

}  // namespace poseopt

template <class FrameT> int PoseOptimization(orbm_t* m, FrameT* pFrame) {
    poseopt::Flat A;
    A.build(*pFrame);
    if (A.nlevels < 1) throw std::runtime_error("PoseOptimization: mvInvLevelSigma2 is empty");
    std::vector<uint8_t> outlier(A.cap, 2);                                  // 2 = not written: the slot holds no MapPoint
    float tcwOut[12];
    int32_t nCorr = 0, nGood = 0, count = A.n;
    if (orbm_pose_optimization(m, 1, 0, A.cap, A.kps.data(), &count, A.haveUright ? A.uright.data() : nullptr, A.qMp.data(), A.nmp, A.pw.data(),
                               A.tcw, A.k, A.bf, A.ils2.data(), A.nlevels, tcwOut, outlier.data(), &nCorr, &nGood) != ORBM_OK)
        throw std::runtime_error(std::string("orbm_pose_optimization: ") + orbm_last_error());
    for (int i = 0; i < A.n; ++i)
        if (outlier[i] != 2) pFrame->mvbOutlier[i] = outlier[i] != 0;
    if (nCorr < 3) return 0;                                                 // Optimizer.cc:1158: flags cleared, pose untouched
    cv::Mat pose(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) pose.at<float>(r, c) = tcwOut[4 * r + c];
    pose.at<float>(3, 0) = 0.f; pose.at<float>(3, 1) = 0.f; pose.at<float>(3, 2) = 0.f; pose.at<float>(3, 3) = 1.f;
    pFrame->SetPose(pose);
    return nGood;
}

template <class MatcherT, class FrameT> int PoseOptimization(MatcherT& matcher, FrameT* pFrame) { return PoseOptimization(matcher.handle(), pFrame); }

}  // namespace ORB_SLAM3
