// MapPointRefresh.h -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:450-538) and MapPoint::UpdateNormalAndDepth
// (src/MapPoint.cc:578-652) as drop-in templates over the host forms of include/orbm.h:
//   ComputeDistinctiveDescriptors(m, pMP), UpdateNormalAndDepth(m, pMP)   one MapPoint, one library call
//   RefreshMapPoints(m, vpMPs)                                            a batch: ONE call of each function for all of them
// The bodies only flatten the reference's containers: the mObservations walk in map order (left entry before the right entry of a
// KeyFrame, :481-486 / :610-621), the ref_slot rule of :627-638 and the write-back under the reference's own conditions.  The N x N
// Hamming tables, the medians and the float sums run in liborbslam3_amd.so.
//
// MapPointT: isBad(), GetObservations() -> std::map<KeyFrameT*, std::tuple<int, int>>, GetReferenceKeyFrame(), GetWorldPos() (3x1
// CV_32F) and the members mDescriptor, mNormalVector, mfMinDistance, mfMaxDistance (protected in the reference: declare these templates
// friends, or call them from member functions).  KeyFrameT: isBad(), mDescriptors (rows of 32 bytes; a two-camera KeyFrame holds the
// left rows, then the right rows), NLeft, mvKeysUn, mvKeys, mvKeysRight, GetCameraCenter(), GetRightCameraCenter(), mvScaleFactors,
// mnScaleLevels.  The scale table is read from the first KeyFrame met: every KeyFrame of a map shares the extractor's settings.
//
// Numerics of the normal: NormalAndDepthOnMat below states them on cv::Mat, the way the reference writes them; compiled against
// cvcompat.h (norm = square root of a double sum, Mat / s = multiply by (float)(1.0 / s)) it gives, bit for bit, what the library
// computes (tests/mappoint_normal.cpp, tests/test_gpu_mappoint.py).  The library call is the product path; the cv::Mat statement is
// the contract, not a fallback.  It stays in this header, and not in the test, because it is what a maintainer who builds with
// ORBX_WITH_OPENCV compares against real cv::Mat: the same function then states the rule on OpenCV's own operators.
//
// Cost of the single-MapPoint forms: every call gathers and uploads the whole descriptor rows of every KeyFrame that observes the
// MapPoint (rows x 32 bytes each, several hundred KB for a well-observed point).  They are there for the isolated call sites
// (MapPoint::Replace, :389); wherever the reference loops over MapPoints, call RefreshMapPoints once for all of them.
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>
#ifdef ORBX_WITH_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "cvcompat.h"
#endif
#include "../../include/orbm.h"

namespace ORB_SLAM3 {

// The arithmetic of UpdateNormalAndDepth for one MapPoint on cv::Mat: centres holds the camera centre of every n++ of the loop, in loop
// order; refCentre = pRefKF->GetCameraCenter(); level = the reference keypoint's octave.  centres must not be empty.
inline void NormalAndDepthOnMat(const cv::Mat& Pos, const std::vector<cv::Mat>& centres, const cv::Mat& refCentre, int level,
                                const std::vector<float>& scaleFactors, cv::Mat& normalOut, float& minDistance, float& maxDistance) {
    cv::Mat normal = cv::Mat::zeros(3, 1, CV_32F);
    int n = 0;
    for (const cv::Mat& Owi : centres) {
        cv::Mat normali = Pos - Owi;
        normal = normal + normali / cv::norm(normali);
        n++;
    }
    cv::Mat PC = Pos - refCentre;
    const float dist = cv::norm(PC);
    maxDistance = dist * scaleFactors[level];
    minDistance = maxDistance / scaleFactors[scaleFactors.size() - 1];
    normalOut = normal / n;
}

namespace mprefresh {

// the arrays of one call: a pool of the KeyFrames the MapPoints observe (one row each) and the CSR of their observations
template <class KeyFrameT> struct Flat {
    std::map<KeyFrameT*, int> rowOf;
    std::vector<KeyFrameT*> rows;
    std::vector<int32_t> off, row, slot, refRow, refSlot, counts;
    std::vector<uint8_t> flags, valid, desc;
    std::vector<float> pw, owl, owr, scale;
    std::vector<orbm_kp_t> kps;
    int cap = 1;
    bool anyRight = false;

    int rowFor(KeyFrameT* pKF) {
        auto it = rowOf.find(pKF);
        if (it != rowOf.end()) return it->second;
        const int r = (int)rows.size();
        rowOf[pKF] = r; rows.push_back(pKF);
        if (pKF->mDescriptors.rows > cap) cap = pKF->mDescriptors.rows;
        return r;
    }

    template <class MapPointT> void add(MapPointT* pMP) {
        const bool bad = pMP->isBad();
        valid.push_back(bad ? 0 : 1);
        int rr = -1, rs = -1;
        float p[3] = {0.f, 0.f, 0.f};
        if (!bad) {
            auto observations = pMP->GetObservations();
            KeyFrameT* pRefKF = pMP->GetReferenceKeyFrame();
            const cv::Mat Pos = pMP->GetWorldPos();
            for (int i = 0; i < 3; ++i) p[i] = Pos.template at<float>(i);
            for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
                KeyFrameT* pKF = mit->first;
                const int r = rowFor(pKF);
                const uint8_t badKF = pKF->isBad() ? 2 : 0;
                const int leftIndex = std::get<0>(mit->second), rightIndex = std::get<1>(mit->second);
                if (leftIndex != -1) { row.push_back(r); slot.push_back(leftIndex); flags.push_back(badKF); }
                if (rightIndex != -1) { row.push_back(r); slot.push_back(rightIndex); flags.push_back(badKF | 1); anyRight = true; }
            }
            if (pRefKF && !observations.empty()) {                          // :627-638
                rr = rowFor(pRefKF);
                int leftIndex = 0, rightIndex = 0;                          // observations[pRefKF] of a KeyFrame that is not in the map: a zeroed tuple
                auto it = observations.find(pRefKF);
                if (it != observations.end()) { leftIndex = std::get<0>(it->second); rightIndex = std::get<1>(it->second); }
                rs = (pRefKF->NLeft == -1 || leftIndex != -1) ? leftIndex : rightIndex;   // rightIndex already counts from the stacked row's start
            }
        }
        off.push_back((int32_t)row.size());
        refRow.push_back(rr); refSlot.push_back(rs);
        pw.insert(pw.end(), p, p + 3);
    }

    // the pool rows: descriptors for ComputeDistinctiveDescriptors, octaves and centres for UpdateNormalAndDepth
    void fillPool(bool withDesc, bool withGeometry) {
        const size_t nr = rows.size();
        counts.assign(nr, 0);
        if (withDesc) desc.assign(nr * cap * 32, 0);
        if (withGeometry) { kps.assign(nr * cap, orbm_kp_t()); owl.assign(nr * 3, 0.f); owr.assign(nr * 3, 0.f); }
        for (size_t r = 0; r < nr; ++r) {
            KeyFrameT* pKF = rows[r];
            const int n = pKF->mDescriptors.rows;
            counts[r] = n;
            if (withDesc) for (int i = 0; i < n; ++i) std::memcpy(&desc[(r * cap + i) * 32], pKF->mDescriptors.ptr(i), 32);
            if (!withGeometry) continue;
            if (scale.empty()) scale.assign(pKF->mvScaleFactors.begin(), pKF->mvScaleFactors.begin() + pKF->mnScaleLevels);
            for (int i = 0; i < n; ++i) {                                   // the octave each branch of :630-638 reads
                int octave = -1;
                if (pKF->NLeft == -1) { if (i < (int)pKF->mvKeysUn.size()) octave = pKF->mvKeysUn[i].octave; }
                else if (i < pKF->NLeft) { if (i < (int)pKF->mvKeys.size()) octave = pKF->mvKeys[i].octave; }
                else if (i - pKF->NLeft < (int)pKF->mvKeysRight.size()) octave = pKF->mvKeysRight[i - pKF->NLeft].octave;
                kps[r * cap + i].octave = octave;
            }
            const cv::Mat Ow = pKF->GetCameraCenter();
            for (int i = 0; i < 3; ++i) owl[r * 3 + i] = Ow.template at<float>(i);
            if (anyRight && pKF->NLeft != -1) {
                const cv::Mat Owr = pKF->GetRightCameraCenter();
                for (int i = 0; i < 3; ++i) owr[r * 3 + i] = Owr.template at<float>(i);
            }
        }
    }
};

template <class MapPointT> struct KeyFrameOf {
    typedef decltype(std::declval<MapPointT>().GetObservations()) Map;
    typedef typename std::remove_pointer<typename Map::key_type>::type type;
};

template <class MapPointT> void run(orbm_t* m, const std::vector<MapPointT*>& vpMPs, bool descriptors, bool normals) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbm_kp_t), "cv::KeyPoint layout");
    const int nmp = (int)vpMPs.size();
    if (nmp == 0) return;
    Flat<typename KeyFrameOf<MapPointT>::type> F;
    F.off.push_back(0);
    for (MapPointT* pMP : vpMPs) F.add(pMP);
    if (F.rows.empty()) return;                                             // no observation anywhere: both functions return early for every MapPoint
    F.fillPool(descriptors, normals);
    const int nobs = (int)F.row.size(), nrows = (int)F.rows.size();
    static const int32_t zero = 0; static const uint8_t zero8 = 0;
    const int32_t* prow = nobs ? F.row.data() : &zero; const int32_t* pslot = nobs ? F.slot.data() : &zero; const uint8_t* pfl = nobs ? F.flags.data() : &zero8;
    if (descriptors) {
        std::vector<uint8_t> out((size_t)nmp * 32, 0);
        std::vector<int32_t> best(nmp, -1);
        const int rc = orbm_distinctive_descriptors(m, nmp, nrows, F.cap, F.desc.data(), F.counts.data(), nobs, F.off.data(), prow, pslot, pfl, F.valid.data(),
                                                    out.data(), best.data(), nullptr);
        if (rc < 0) throw std::runtime_error(std::string("orbm_distinctive_descriptors: ") + orbm_last_error());
        for (int i = 0; i < nmp; ++i) {
            if (best[i] < 0) continue;                                      // :460, :465, :490: the reference returns without touching mDescriptor
            cv::Mat d(1, 32, CV_8U);
            std::memcpy(d.ptr(0), &out[(size_t)i * 32], 32);
            vpMPs[i]->mDescriptor = d;                                      // :536
        }
    }
    if (normals) {
        std::vector<float> normal((size_t)nmp * 3, 0.f), mn(nmp, 0.f), mx(nmp, 0.f);
        std::vector<uint8_t> updated(nmp, 0);
        const int rc = orbm_update_normal_and_depth(m, nmp, nrows, F.cap, F.kps.data(), F.counts.data(), F.owl.data(), F.anyRight ? F.owr.data() : nullptr,
                                                    nobs, F.off.data(), prow, pslot, pfl, F.valid.data(), F.pw.data(), F.refRow.data(), F.refSlot.data(),
                                                    F.scale.data(), (int)F.scale.size(), normal.data(), mn.data(), mx.data(), updated.data());
        if (rc < 0) throw std::runtime_error(std::string("orbm_update_normal_and_depth: ") + orbm_last_error());
        for (int i = 0; i < nmp; ++i) {
            if (!updated[i]) continue;                                      // :587, :595: nothing is written
            cv::Mat nv(3, 1, CV_32F);
            for (int r = 0; r < 3; ++r) nv.template at<float>(r) = normal[(size_t)i * 3 + r];
            vpMPs[i]->mfMaxDistance = mx[i];                                // :647-649
            vpMPs[i]->mfMinDistance = mn[i];
            vpMPs[i]->mNormalVector = nv;
        }
    }
}

}  // namespace mprefresh

template <class MapPointT> void ComputeDistinctiveDescriptors(orbm_t* m, MapPointT* pMP) {
    mprefresh::run(m, std::vector<MapPointT*>(1, pMP), true, false);
}
template <class MapPointT> void UpdateNormalAndDepth(orbm_t* m, MapPointT* pMP) {
    mprefresh::run(m, std::vector<MapPointT*>(1, pMP), false, true);
}
// `for (pMP : vpMPs) { pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth(); }` (LocalMapping.cc:1061-1064,
// LoopClosing.cc:1449 and the other sites) with one library call per function.
template <class MapPointT> void RefreshMapPoints(orbm_t* m, const std::vector<MapPointT*>& vpMPs) {
    mprefresh::run(m, vpMPs, true, true);
}

}  // namespace ORB_SLAM3
