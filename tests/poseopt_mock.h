// Mock Frame / MapPoint types with the members facade/PoseOptimization.h reads and writes, filled from a case of tests/poseopt_case_io.h.
#pragma once
#include <vector>
#include "../orb-slam3_amd/facade/cvcompat.h"
#include "poseopt_case_io.h"

struct MapPoint {
    cv::Mat mWorldPos;
    MapPoint() : mWorldPos(3, 1, CV_32F) {}
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
};

struct Frame {
    int N = 0;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<bool> mvbOutlier;
    cv::Mat mTcw;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    const void* mpCamera2 = nullptr;
    int nSetPose = 0;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); ++nSetPose; }
};

// mvbOutlier starts all true so that a flag the call clears can be told from one it never wrote
static void frame_from_case(const Case& c, Frame& F, std::vector<MapPoint>& pool) {
    F.N = c.n;
    pool.clear(); pool.resize(c.n);
    for (MapPoint& mp : pool) mp.mWorldPos = cv::Mat(3, 1, CV_32F);        // a copied cv::Mat shares its data: one matrix per point
    F.mvpMapPoints.assign(c.n, nullptr); F.mvKeysUn.assign(c.n, cv::KeyPoint()); F.mvbOutlier.assign(c.n, true);
    F.mvuRight.clear();
    for (int i = 0; i < c.n; ++i) {
        F.mvKeysUn[i].pt.x = c.x[i]; F.mvKeysUn[i].pt.y = c.y[i]; F.mvKeysUn[i].octave = c.octave[i];
        F.mvKeysUn[i].size = 31.f; F.mvKeysUn[i].angle = (float)i;
        if (c.haveUright) F.mvuRight.push_back(c.ur[i]);
        if (c.has[i]) {
            for (int k = 0; k < 3; ++k) pool[i].mWorldPos.at<float>(k) = c.pw[3 * (size_t)i + k];
            F.mvpMapPoints[i] = &pool[i];
        }
    }
    F.mvInvLevelSigma2 = c.ils2;
    F.mTcw = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 4; ++k) F.mTcw.at<float>(r, k) = c.tcw[4 * r + k];
    F.fx = c.k[0]; F.fy = c.k[1]; F.cx = c.k[2]; F.cy = c.k[3]; F.mbf = c.bf;
}
