// KeyFrameCulling.h -- LocalMapping::KeyFrameCulling (src/LocalMapping.cc:1218-1400) as a drop-in template over the host form
// orbm_keyframe_culling of include/orbm.h:
//   KeyFrameCulling(m, pCurrentKF, bMonocular, redundant_th, pbAbortBA, onRedundant)   the loop; onRedundant(pKF) is the caller's :1350-1392
//   KeyFrameCulling(m, pCurrentKF, bMonocular, redundant_th, pbAbortBA)                the non-inertial branch: pKF->SetBadFlag() (:1391)
// The body runs UpdateBestCovisibles() and GetVectorCovisibleKeyFrames() (:1234-1236), applies the skips of :1272 and the count rule of
// :1395 (count also advances on skipped KeyFrames, and a `continue` passes the test by), flattens the candidates ONCE (kfcull::Flat) and
// makes one library call for all of them.  The (candidates x slots x observations) level compares run in liborbslam3_amd.so.
//
// The sequential rule.  The reference erases a KeyFrame the moment it is voted out, so every later candidate is counted on a changed
// map.  The library's answers are exact for candidates 0 .. first_cull; the loop hands candidate first_cull to onRedundant, and if the
// KeyFrame is really gone afterwards (pKF->isBad(); mbNotErase leaves it alive) it sets erased[row] and calls again for the candidates
// behind it, on the same arrays: no CSR, pool or kf_mp row is rebuilt.  A map in which nothing is voted out costs one call.
// The erased rule assumes the map invariant the reference keeps: an observation entry of KeyFrame X exists exactly where X's mvpMapPoints
// holds that MapPoint (KeyFrame::AddMapPoint with MapPoint::AddObservation, EraseMapPointMatch with EraseObservation).  KeyFrame::SetBadFlag
// walks mvpMapPoints (KeyFrame.cc:773-780), the library walks the entries; where the two disagree, so do the answers.
//
// onRedundant(pKF) returns false where the reference `continue`s (:1356, :1359: the count test of :1395 is then passed by) and true
// otherwise.  The inertial side conditions (mPrevKF / mNextKF / time, the preintegration merge) live in it, with the caller.
//
// Deviation from the reference.  For a two-camera candidate the reference reads mvKeysRight[i].octave with the stacked index i
// (:1303-1305): past the end of the vector, or the wrong feature.  The library reads slot i of the stacked row, that is
// mvKeysRight[i - NLeft].  The observers' levels (:1316-1328) are the reference's.
//
// KeyFrameT: mnId, N, NLeft, mvKeysUn, mvKeys, mvKeysRight, mvuRight, mvDepth, mThDepth, mpCamera2, GetMap()->GetInitKFid(), isBad(),
// GetMapPointMatches(), UpdateBestCovisibles(), GetVectorCovisibleKeyFrames(), SetBadFlag().  MapPointT (taken from
// GetMapPointMatches()): isBad(), Observations(), GetObservations() -> std::map<KeyFrameT*, std::tuple<int, int>>.
#pragma once
#include <cstdint>
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
namespace kfcull {

template <class KeyFrameT> struct MapPointOf {
    typedef decltype(std::declval<KeyFrameT>().GetMapPointMatches()) Vec;
    typedef typename std::remove_pointer<typename Vec::value_type>::type type;
};

// The arrays of one call.  Pool rows: the candidates in order, then every other observing KeyFrame in the order it is met (the row
// assignment of mprefresh::Flat); the MapPoint list: the order in which the candidates' slots meet them.  Entries per MapPoint in map
// order, the left entry before the right one; flags bit 0 = right camera, bit 1 = the KeyFrame isBad(), bit 2 = the entry weighs 2 in nObs
// (MapPoint.cc:212).  A bad MapPoint gets an empty list.
template <class KeyFrameT, class MapPointT = typename MapPointOf<KeyFrameT>::type> struct Flat {
    std::map<KeyFrameT*, int> rowOf;
    std::map<MapPointT*, int> mpOf;
    std::vector<KeyFrameT*> rows;
    std::vector<int32_t> candRow, off, row, slot, counts, kfMp, mpNobs;
    std::vector<uint8_t> flags, valid;
    std::vector<float> depth;
    std::vector<orbm_kp_t> kps;
    int cap = 1;
    float thDepth = 0.f;

    int rowFor(KeyFrameT* pKF) {
        auto it = rowOf.find(pKF);
        if (it != rowOf.end()) return it->second;
        const int r = (int)rows.size();
        rowOf[pKF] = r; rows.push_back(pKF);
        if (pKF->N > cap) cap = pKF->N;
        return r;
    }

    void build(const std::vector<KeyFrameT*>& cands, bool bMonocular) {
        static_assert(sizeof(cv::KeyPoint) == sizeof(orbm_kp_t), "cv::KeyPoint layout");
        for (KeyFrameT* pKF : cands) candRow.push_back(rowFor(pKF));
        off.assign(1, 0);
        std::vector<std::vector<int32_t>> perCand;
        for (KeyFrameT* pKF : cands) {
            const auto vpMapPoints = pKF->GetMapPointMatches();
            std::vector<int32_t> idx(vpMapPoints.size(), -1);
            for (size_t i = 0; i < vpMapPoints.size(); ++i) {
                MapPointT* pMP = vpMapPoints[i];
                if (!pMP) continue;
                auto it = mpOf.find(pMP);
                if (it == mpOf.end()) {
                    it = mpOf.insert(std::make_pair(pMP, (int)mpNobs.size())).first;
                    const bool bad = pMP->isBad();
                    valid.push_back(bad ? 0 : 1);
                    mpNobs.push_back(pMP->Observations());
                    if (!bad) {
                        const auto observations = pMP->GetObservations();
                        for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
                            KeyFrameT* pKFi = mit->first;
                            const int r = rowFor(pKFi);
                            const uint8_t badKF = pKFi->isBad() ? 2 : 0;
                            const int leftIndex = std::get<0>(mit->second), rightIndex = std::get<1>(mit->second);
                            if (leftIndex != -1) {
                                const uint8_t two = (!pKFi->mpCamera2 && pKFi->mvuRight[leftIndex] >= 0) ? 4 : 0;   // MapPoint.cc:212, :232
                                row.push_back(r); slot.push_back(leftIndex); flags.push_back(badKF | two);
                            }
                            if (rightIndex != -1) { row.push_back(r); slot.push_back(rightIndex); flags.push_back(badKF | 1); }
                        }
                    }
                    off.push_back((int32_t)row.size());
                }
                idx[i] = it->second;
            }
            perCand.push_back(idx);
        }
        const size_t nr = rows.size(), nc = cands.size();
        counts.assign(nr, 0);
        orbm_kp_t none = orbm_kp_t();
        none.octave = -1;
        kps.assign(nr * cap, none);
        for (size_t r = 0; r < nr; ++r) {
            KeyFrameT* pKF = rows[r];
            counts[r] = pKF->N;
            for (int i = 0; i < pKF->N; ++i) {                              // the octave each branch of :1303-1305 / :1316-1328 reads
                int octave = -1;
                if (pKF->NLeft == -1) { if (i < (int)pKF->mvKeysUn.size()) octave = pKF->mvKeysUn[i].octave; }
                else if (i < pKF->NLeft) { if (i < (int)pKF->mvKeys.size()) octave = pKF->mvKeys[i].octave; }
                else if (i - pKF->NLeft < (int)pKF->mvKeysRight.size()) octave = pKF->mvKeysRight[i - pKF->NLeft].octave;
                kps[r * cap + i].octave = octave;
            }
        }
        kfMp.assign(nc * cap, -1);
        if (!bMonocular) depth.assign(nc * cap, -1.f);
        for (size_t k = 0; k < nc; ++k) {
            for (size_t i = 0; i < perCand[k].size() && i < (size_t)cap; ++i) kfMp[k * cap + i] = perCand[k][i];
            if (!bMonocular)
                for (size_t i = 0; i < cands[k]->mvDepth.size() && i < (size_t)cap; ++i) depth[k * cap + i] = cands[k]->mvDepth[i];
        }
        if (nc) thDepth = cands[0]->mThDepth;
    }
};

}  // namespace kfcull

template <class KeyFrameT, class OnRedundant>
void KeyFrameCulling(orbm_t* m, KeyFrameT* pCurrentKF, bool bMonocular, float redundant_th, const bool* pbAbortBA, OnRedundant onRedundant) {
    pCurrentKF->UpdateBestCovisibles();
    const std::vector<KeyFrameT*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
    const int thObs = 3;
    size_t pos = 0;
    int count = 0;
    while (pos < vpLocalKeyFrames.size()) {
        // the candidates up to and including the first whose count is above 100: the loop goes on behind it only through a `continue`
        std::vector<KeyFrameT*> cands;
        std::vector<int> countAt;
        while (pos < vpLocalKeyFrames.size()) {
            KeyFrameT* pKF = vpLocalKeyFrames[pos++];
            count++;
            if ((pKF->mnId == pKF->GetMap()->GetInitKFid()) || pKF->isBad()) continue;   // :1272
            cands.push_back(pKF); countAt.push_back(count);
            if (count > 100) break;
        }
        if (cands.empty()) return;
        kfcull::Flat<KeyFrameT> F;
        F.build(cands, bMonocular);
        const int nc = (int)cands.size(), nmp = (int)F.mpNobs.size(), nobs = (int)F.row.size(), nrows = (int)F.rows.size();
        static const int32_t zero = 0; static const uint8_t zero8 = 0;
        const int32_t* prow = nobs ? F.row.data() : &zero; const int32_t* pslot = nobs ? F.slot.data() : &zero; const uint8_t* pfl = nobs ? F.flags.data() : &zero8;
        std::vector<uint8_t> erased(nrows, 0), cull(nc, 0);
        std::vector<int32_t> nMPs(nc, 0), nRedundant(nc, 0);
        bool anyErased = false;
        int start = 0;
        while (start < nc) {
            const int n = nc - start;
            int32_t first = -1;
            if (nmp > 0) {                                                  // no MapPoint anywhere: every count is 0 and 0 > th * 0 is false
                const int rc = orbm_keyframe_culling(m, n, F.candRow.data() + start, nrows, F.cap, F.kps.data(), F.counts.data(),
                                                     F.kfMp.data() + (size_t)start * F.cap, bMonocular ? nullptr : F.depth.data() + (size_t)start * F.cap,
                                                     F.thDepth, nmp, nobs, F.off.data(), prow, pslot, pfl, F.valid.data(), F.mpNobs.data(),
                                                     anyErased ? erased.data() : nullptr, thObs, redundant_th, nMPs.data(), nRedundant.data(),
                                                     cull.data(), nullptr, &first);
                if (rc < 0) throw std::runtime_error(std::string("orbm_keyframe_culling: ") + orbm_last_error());
            }
            const int last = first < 0 ? n - 1 : first;                    // exact up to and including the first KeyFrame voted out
            for (int k = 0; k <= last; ++k) {
                KeyFrameT* pKF = cands[start + k];
                bool through = true;
                if (k == first) {                                           // :1349
                    through = onRedundant(pKF);
                    if (pKF->isBad()) { erased[F.candRow[start + k]] = 1; anyErased = true; }
                }
                if (!through) continue;
                const int c = countAt[start + k];
                if ((c > 20 && pbAbortBA && *pbAbortBA) || c > 100) return;   // :1395
            }
            start += last + 1;
        }
    }
}

template <class KeyFrameT>
void KeyFrameCulling(orbm_t* m, KeyFrameT* pCurrentKF, bool bMonocular, float redundant_th, const bool* pbAbortBA) {
    KeyFrameCulling(m, pCurrentKF, bMonocular, redundant_th, pbAbortBA, [](KeyFrameT* pKF) { pKF->SetBadFlag(); return true; });
}

}  // namespace ORB_SLAM3
