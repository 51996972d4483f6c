// CreateNewMapPoints.h -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:487-930) as a template over the host form
// orbm_triangulate_new_points of include/orbm.h:
//   int nNew = CreateNewMapPoints(matcher, mpCurrentKeyFrame, vpNeighKFs, mbMonocular, bCoarse, mbFarPoints, mThFarPoints,
//                                 [&](const cv::Matx31f& x3D, KeyFrame* pKF2, int idx1, int idx2) {
//                                     MapPoint* pMP = new MapPoint(cv::Mat(x3D), mpCurrentKeyFrame, mpAtlas->GetCurrentMap());   // :897-916
//                                     pMP->AddObservation(mpCurrentKeyFrame, idx1); pMP->AddObservation(pKF2, idx2); ... });
// It runs the baseline / median-depth tests (:552-578), computes F12 (ComputeF12_, :1102-1119) for every neighbour that passes, searches
// each of them with matcher.SearchForTriangulation_ -- all from the MapPoint state at the start, which is what
// orbm_search_for_triangulation_batch_async computes in one launch for a caller whose KeyFrames live on the device -- then makes ONE
// orbm_triangulate_new_points call for all neighbours (parallax, triangulation, reprojection and scale gates, the cross-pair rule) and
// walks `order`: onNewPoint is called in the order the reference creates its MapPoints, pair by pair and ascending idx1 inside a pair.
// new MapPoint / AddObservation / AddMapPoint stay in the reference's text inside the callback; because every search ran before the
// first callback, a later neighbour's match for a feature that already got its point has been dropped by the call (INTEGRATION.md,
// the cross-pair rule), as the reference's own search would have skipped it.  The CheckNewKeyFrames() early return (:545) stays with the
// caller: pass the neighbours to be processed.
// x3D is the library's own arithmetic (csrc/orbm_triangulate.h): within the tolerance DESIGN section 8 states of cv::SVD's, not
// bit-identical to it.
//
// Scope: pinhole KeyFrames with NLeft == -1 and no second camera.  Anything else is REFUSED with std::runtime_error: the facade does not
// guess.  The neighbours share one camera and one pyramid (fx .. invfy, mb, mvScaleFactors, mvLevelSigma2), as the KeyFrames of one
// map do; a neighbour that differs is refused too.
//
// KeyFrameT: N, NLeft, mvKeysUn, mvKeys, mvuRight, mvDepth, fx, fy, cx, cy, invfx, invfy, mb, mbf, mfScaleFactor, mvScaleFactors,
// mvLevelSigma2, mpCamera (GetType(), CAM_PINHOLE, project), mpCamera2, GetRotation_(), GetTranslation_(), GetCameraCenter_(),
// ComputeSceneMedianDepth(int) and what SearchForTriangulation_ reads.  matcher: handle() -> orbm_t* and SearchForTriangulation_
// (facade/ORBmatcher.h).
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#ifdef ORBX_WITH_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvcompat.h"
#endif
#include "../../include/orbm.h"

namespace ORB_SLAM3 {
namespace newpoints {

// cv::Matx33f::inv() of an upper-triangular K (toK_()): the closed form of the 3x3 fast path, cofactors over the determinant in float
inline cv::Matx33f inv33(const cv::Matx33f& a) {
    const float d0 = a(0, 0) * (a(1, 1) * a(2, 2) - a(2, 1) * a(1, 2)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(2, 0) * a(1, 2)) +
                     a(0, 2) * (a(1, 0) * a(2, 1) - a(2, 0) * a(1, 1));
    cv::Matx33f b;
    if (d0 == 0) return b;
    const float d = 1 / d0;
    b(0, 0) = (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) * d; b(0, 1) = (a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2)) * d; b(0, 2) = (a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)) * d;
    b(1, 0) = (a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2)) * d; b(1, 1) = (a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0)) * d; b(1, 2) = (a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)) * d;
    b(2, 0) = (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)) * d; b(2, 1) = (a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1)) * d; b(2, 2) = (a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)) * d;
    return b;
}
template <class KeyFrameT> cv::Matx33f toK(const KeyFrameT& K) {
    cv::Matx33f k;
    k(0, 0) = K.fx; k(0, 2) = K.cx; k(1, 1) = K.fy; k(1, 2) = K.cy; k(2, 2) = 1.f;
    return k;
}
// LocalMapping::ComputeF12_ (:1102-1119)
template <class KeyFrameT> cv::Matx33f ComputeF12(KeyFrameT* pKF1, KeyFrameT* pKF2) {
    auto R1w = pKF1->GetRotation_(); auto t1w = pKF1->GetTranslation_();
    auto R2w = pKF2->GetRotation_(); auto t2w = pKF2->GetTranslation_();
    auto R12 = R1w * R2w.t();
    auto t12 = -R1w * R2w.t() * t2w + t1w;
    cv::Matx33f t12x;                                                        // SkewSymmetricMatrix_
    t12x(0, 1) = -t12(2, 0); t12x(0, 2) = t12(1, 0); t12x(1, 0) = t12(2, 0); t12x(1, 2) = -t12(0, 0); t12x(2, 0) = -t12(1, 0); t12x(2, 1) = t12(0, 0);
    return inv33(toK(*pKF1).t()) * t12x * R12 * inv33(toK(*pKF2));
}
inline float norm31(const cv::Matx31f& v) {                                  // cv::norm: the square root of a double sum
    double s = 0;
    for (int i = 0; i < 3; ++i) s += (double)v(i, 0) * (double)v(i, 0);
    return (float)std::sqrt(s);
}

// The arrays of one call: pool 1 = the current KeyFrame (one row of cap1 slots), pool 2 = the neighbours that pass the baseline test
// (one row of cap2 slots each), one group.
struct Flat {
    int cap1 = 1, cap2 = 1, npairs = 0, nlevels = 0;
    std::vector<orbm_kp_t> kpsUn1, kps1, kpsUn2, kps2;
    std::vector<float> uright1, depth1, uright2, depth2, tcw1, ow1, tcw2, ow2, sf, ls;
    std::vector<int32_t> counts1, counts2, row1, row2, matches12;
    std::vector<int> neigh;                                                  // pair p is vpNeighKFs[neigh[p]]
    std::vector<cv::Matx33f> F12;
    float k[6], mb = 0, mbf = 0, ratioFactor = 0;

    template <class KeyFrameT> static void check(const KeyFrameT& K) {
        if (K.mpCamera2 || K.NLeft != -1) throw std::runtime_error("CreateNewMapPoints: a KeyFrame with a second camera (mpCamera2 / NLeft != -1) is outside this call: "
                                                                   "LocalMapping.cc:644-709 stays with the caller");
        if (K.mpCamera->GetType() != K.mpCamera->CAM_PINHOLE) throw std::runtime_error("CreateNewMapPoints: only the Pinhole camera model is restated");
    }
    template <class KeyFrameT> static void row(const KeyFrameT& K, int cap, orbm_kp_t* un, orbm_kp_t* raw, float* ur, float* dp, float* tcw, float* ow) {
        static_assert(sizeof(cv::KeyPoint) == sizeof(orbm_kp_t), "cv::KeyPoint layout");
        for (int i = 0; i < cap; ++i) { ur[i] = -1.f; dp[i] = -1.f; un[i] = orbm_kp_t(); raw[i] = orbm_kp_t(); }
        for (int i = 0; i < K.N; ++i) {
            un[i] = *(const orbm_kp_t*)&K.mvKeysUn[i]; raw[i] = *(const orbm_kp_t*)&K.mvKeys[i];
            if ((int)K.mvuRight.size() > i) ur[i] = K.mvuRight[i];
            if ((int)K.mvDepth.size() > i) dp[i] = K.mvDepth[i];
        }
        auto R = const_cast<KeyFrameT&>(K).GetRotation_(); auto t = const_cast<KeyFrameT&>(K).GetTranslation_(); auto O = const_cast<KeyFrameT&>(K).GetCameraCenter_();
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) tcw[4 * r + c] = R(r, c); tcw[4 * r + 3] = t(r, 0); ow[r] = O(r, 0); }
    }
    // everything but the matches: which neighbours pass (:552-578), their rows and F12
    template <class KeyFrameT> void build(KeyFrameT* cur, const std::vector<KeyFrameT*>& vpNeighKFs, bool bMonocular) {
        check(*cur);
        cap1 = cur->N > 0 ? cur->N : 1;
        kpsUn1.resize(cap1); kps1.resize(cap1); uright1.resize(cap1); depth1.resize(cap1); tcw1.resize(12); ow1.resize(3);
        row(*cur, cap1, kpsUn1.data(), kps1.data(), uright1.data(), depth1.data(), tcw1.data(), ow1.data());
        counts1.assign(1, cur->N);
        k[0] = cur->fx; k[1] = cur->fy; k[2] = cur->cx; k[3] = cur->cy; k[4] = cur->invfx; k[5] = cur->invfy;
        mb = cur->mb; mbf = cur->mbf; ratioFactor = 1.5f * cur->mfScaleFactor;
        sf.assign(cur->mvScaleFactors.begin(), cur->mvScaleFactors.end()); ls.assign(cur->mvLevelSigma2.begin(), cur->mvLevelSigma2.end());
        nlevels = (int)sf.size();
        if (nlevels < 1 || ls.size() != sf.size()) throw std::runtime_error("CreateNewMapPoints: mvScaleFactors / mvLevelSigma2 are empty or differ in length");
        auto Ow1 = cur->GetCameraCenter_();
        neigh.clear(); F12.clear(); cap2 = 1;
        for (size_t i = 0; i < vpNeighKFs.size(); ++i) {
            KeyFrameT* pKF2 = vpNeighKFs[i];
            check(*pKF2);
            if (pKF2->fx != cur->fx || pKF2->fy != cur->fy || pKF2->cx != cur->cx || pKF2->cy != cur->cy || pKF2->invfx != cur->invfx || pKF2->invfy != cur->invfy ||
                pKF2->mb != cur->mb || pKF2->mvScaleFactors != cur->mvScaleFactors || pKF2->mvLevelSigma2 != cur->mvLevelSigma2)
                throw std::runtime_error("CreateNewMapPoints: a neighbour with another camera or pyramid than the current KeyFrame");
            auto Ow2 = pKF2->GetCameraCenter_();
            cv::Matx31f vBaseline;
            for (int r = 0; r < 3; ++r) vBaseline(r, 0) = Ow2(r, 0) - Ow1(r, 0);
            const float baseline = norm31(vBaseline);
            if (!bMonocular) { if (baseline < pKF2->mb) continue; }
            else {
                const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
                const float ratioBaselineDepth = baseline / medianDepthKF2;
                if (ratioBaselineDepth < 0.01) continue;
            }
            neigh.push_back((int)i); F12.push_back(ComputeF12(cur, pKF2));
            if (pKF2->N > cap2) cap2 = pKF2->N;
        }
        npairs = (int)neigh.size();
        const size_t s2 = (size_t)(npairs > 0 ? npairs : 1) * cap2;
        kpsUn2.resize(s2); kps2.resize(s2); uright2.resize(s2); depth2.resize(s2); tcw2.resize(12 * (size_t)(npairs > 0 ? npairs : 1)); ow2.resize(3 * (size_t)(npairs > 0 ? npairs : 1));
        counts2.assign(npairs > 0 ? npairs : 1, 0); row1.assign(npairs, 0); row2.resize(npairs);
        for (int p = 0; p < npairs; ++p) {
            const KeyFrameT& K2 = *vpNeighKFs[neigh[p]];
            row(K2, cap2, &kpsUn2[(size_t)p * cap2], &kps2[(size_t)p * cap2], &uright2[(size_t)p * cap2], &depth2[(size_t)p * cap2], &tcw2[12 * (size_t)p], &ow2[3 * (size_t)p]);
            counts2[p] = K2.N; row2[p] = p;
        }
        matches12.assign((size_t)npairs * cap1, -1);
    }
    void set_matches(int p, const std::vector<std::pair<size_t, size_t>>& pairs) {
        for (const auto& m : pairs) matches12[(size_t)p * cap1 + m.first] = (int32_t)m.second;
    }
};

// the triangulation call and the walk over `order`; returns the number of points created
template <class KeyFrameT, class OnNewPoint>
int triangulate(orbm_t* h, const Flat& A, const std::vector<KeyFrameT*>& vpNeighKFs, bool bFarPoints, float thFarPoints, OnNewPoint& onNewPoint) {
    if (A.npairs < 1) return 0;
    if (A.npairs > ORBM_TRI_MAX_GROUP_PAIRS) throw std::runtime_error("CreateNewMapPoints: more than 64 neighbours in one call");
    const int32_t gs[2] = {0, A.npairs};
    std::vector<int32_t> wonPair(A.cap1), wonIdx2(A.cap1), order(A.cap1), ncreated(A.npairs);
    std::vector<float> x3d(3 * (size_t)A.cap1);
    int32_t ntotal = 0;
    if (orbm_triangulate_new_points(h, ORBM_HOST, 1, gs, A.npairs, 1, A.cap1, A.kpsUn1.data(), A.kps1.data(), A.counts1.data(), A.uright1.data(), A.depth1.data(),
                                    A.tcw1.data(), A.ow1.data(), A.npairs, A.cap2, A.kpsUn2.data(), A.kps2.data(), A.counts2.data(), A.uright2.data(),
                                    A.depth2.data(), A.tcw2.data(), A.ow2.data(), A.row1.data(), A.row2.data(), A.matches12.data(), A.k, A.k, A.mb, A.mbf, A.mb,
                                    A.sf.data(), A.ls.data(), A.sf.data(), A.ls.data(), A.nlevels, A.ratioFactor, bFarPoints ? thFarPoints : 0.f,
                                    wonPair.data(), wonIdx2.data(), x3d.data(), nullptr, ncreated.data(), order.data(), &ntotal) != ORBM_OK)
        throw std::runtime_error(std::string("orbm_triangulate_new_points: ") + orbm_last_error());
    for (int i = 0; i < ntotal; ++i) {
        const int idx1 = order[i];
        cv::Matx31f x3D;
        for (int r = 0; r < 3; ++r) x3D(r, 0) = x3d[3 * (size_t)idx1 + r];
        onNewPoint(x3D, vpNeighKFs[A.neigh[wonPair[idx1]]], idx1, (int)wonIdx2[idx1]);
    }
    return ntotal;
}

}  // namespace newpoints

template <class MatcherT, class KeyFrameT, class OnNewPoint>
int CreateNewMapPoints(MatcherT& matcher, KeyFrameT* pCurrentKF, const std::vector<KeyFrameT*>& vpNeighKFs, bool bMonocular, bool bCoarse, bool bFarPoints,
                       float thFarPoints, OnNewPoint onNewPoint) {
    newpoints::Flat A;
    A.build(pCurrentKF, vpNeighKFs, bMonocular);
    for (int p = 0; p < A.npairs; ++p) {
        std::vector<std::pair<size_t, size_t>> vMatchedIndices;
        matcher.SearchForTriangulation_(pCurrentKF, vpNeighKFs[A.neigh[p]], A.F12[p], vMatchedIndices, false, bCoarse);     // :592
        A.set_matches(p, vMatchedIndices);
    }
    return newpoints::triangulate(matcher.handle(), A, vpNeighKFs, bFarPoints, thFarPoints, onNewPoint);
}

}  // namespace ORB_SLAM3
