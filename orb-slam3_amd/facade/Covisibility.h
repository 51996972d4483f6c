// Covisibility.h -- the covisibility votes and the local map points as drop-in templates over the host forms orbm_covisibility_votes and
// orbm_local_points of include/orbm.h:
//   covis::ConnectionCounts(m, pKF)              the KFcounter of KeyFrame::UpdateConnections step 1 (src/KeyFrame.cc:474-512)
//   covis::ConnectionCountsBatch(m, vpKFs)       the same for a whole LoopClosing loop in ONE library call (nothing changes an observation
//                                                between the iterations of those loops: LoopClosing.cc:1421, :1480, :2001, :2009, :2415, :2423)
//   covis::LocalKeyFrameVotes(m, frame)          the keyframeCounter of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:3964-4013); sets
//                                                frame.mvpMapPoints[i] = NULL for bad MapPoints as :3986 does
//   covis::LocalMapPoints(m, vpLocalKeyFrames)   mvpLocalMapPoints of Tracking::UpdateLocalPoints (:3917-3948) in the reference's order
// The vote itself (slots x observations) and the deduplicating walk run in liborbslam3_amd.so; the flatten follows kfcull::Flat and
// mprefresh::Flat: the same row assignment (the query KeyFrames in order, then every other observing KeyFrame in the order it is met) and
// the same entry order (per MapPoint in map order, the left entry before the right one; flags bit 0 = right camera, bit 1 = the KeyFrame
// isBad(), bit 2 = the entry weighs 2 in nObs).  A bad MapPoint gets an empty list.
//
// What stays with the caller.  The library reports only counts.  The reference's tie rules -- pKFmax is the first maximum in pointer
// order with strict > (:536, Tracking.cc:4037), sort(vPairs) on (weight, pointer) pairs -- work on the std::map these functions return,
// which holds the KeyFrames in pointer order as the reference's does, so the rest of UpdateConnections and UpdateLocalKeyFrames stays in
// the reference's text.  LocalMapPoints does not write MapPoint::mnTrackReferenceForFrame, which the reference uses only for the test
// the library replaces; a caller that reads it elsewhere sets it from the returned vector.
//
// KeyFrameT: mnId, N, mvuRight, mpCamera2, isBad(), GetMap(), GetMapPointMatches().  FrameT: N, mvpMapPoints.  MapPointT: isBad(),
// GetObservations() -> std::map<KeyFrameT*, std::tuple<int, int>>.
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
namespace covis {

template <class KeyFrameT> struct MapPointOf {
    typedef decltype(std::declval<KeyFrameT>().GetMapPointMatches()) Vec;
    typedef typename std::remove_pointer<typename Vec::value_type>::type type;
};

// the KeyFrame type a Frame's MapPoints are observed by: the key of MapPoint::GetObservations()
template <class FrameT> struct TypesOfFrame {
    typedef typename std::remove_pointer<typename std::decay<decltype(std::declval<FrameT>().mvpMapPoints[0])>::type>::type MapPointT;
    typedef typename std::remove_pointer<typename decltype(std::declval<MapPointT>().GetObservations())::key_type>::type KeyFrameT;
};

// The arrays of one vote call: queries are slot lists of MapPoint pointers.
template <class KeyFrameT, class MapPointT = typename MapPointOf<KeyFrameT>::type> struct Flat {
    std::map<KeyFrameT*, int> rowOf;
    std::map<MapPointT*, int> mpOf;
    std::vector<KeyFrameT*> rows;
    std::vector<int32_t> qMp, qN, selfRow, off, row, slot, counts;
    std::vector<uint8_t> flags, valid, kfSkip;
    int cap = 1, qStride = 1;

    int rowFor(KeyFrameT* pKF) {
        auto it = rowOf.find(pKF);
        if (it != rowOf.end()) return it->second;
        const int r = (int)rows.size();
        rowOf[pKF] = r; rows.push_back(pKF);
        if (pKF->N > cap) cap = pKF->N;
        return r;
    }

    // selfKFs: per query the query KeyFrame, or empty for Frames
    void build(const std::vector<std::vector<MapPointT*>>& queries, const std::vector<KeyFrameT*>& selfKFs) {
        for (KeyFrameT* pKF : selfKFs) rowFor(pKF);
        off.assign(1, 0);
        std::vector<std::vector<int32_t>> perQuery;
        for (const std::vector<MapPointT*>& vpMP : queries) {
            std::vector<int32_t> idx(vpMP.size(), -1);
            for (size_t i = 0; i < vpMP.size(); ++i) {
                MapPointT* pMP = vpMP[i];
                if (!pMP) continue;
                auto it = mpOf.find(pMP);
                if (it == mpOf.end()) {
                    it = mpOf.insert(std::make_pair(pMP, (int)valid.size())).first;
                    const bool bad = pMP->isBad();
                    valid.push_back(bad ? 0 : 1);
                    if (!bad) {
                        const auto observations = pMP->GetObservations();
                        for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
                            KeyFrameT* pKFi = mit->first;
                            const int r = rowFor(pKFi);
                            const uint8_t badKF = pKFi->isBad() ? 2 : 0;
                            const int leftIndex = std::get<0>(mit->second), rightIndex = std::get<1>(mit->second);
                            if (leftIndex != -1) {
                                const uint8_t two = (!pKFi->mpCamera2 && pKFi->mvuRight[leftIndex] >= 0) ? 4 : 0;
                                row.push_back(r); slot.push_back(leftIndex); flags.push_back(badKF | two);
                            }
                            if (rightIndex != -1) { row.push_back(r); slot.push_back(rightIndex); flags.push_back(badKF | 1); }
                        }
                    }
                    off.push_back((int32_t)row.size());
                }
                idx[i] = it->second;
            }
            if ((int)idx.size() > qStride) qStride = (int)idx.size();
            perQuery.push_back(idx);
        }
        const size_t nq = queries.size();
        qMp.assign(nq * qStride, -1); qN.assign(nq, 0);
        for (size_t q = 0; q < nq; ++q) {
            qN[q] = (int32_t)perQuery[q].size();
            for (size_t i = 0; i < perQuery[q].size(); ++i) qMp[q * qStride + i] = perQuery[q][i];
        }
        for (KeyFrameT* pKF : selfKFs) selfRow.push_back(rowOf[pKF]);
        counts.clear();
        for (KeyFrameT* pKF : rows) counts.push_back(pKF->N);
    }

    // kf_skip of UpdateConnections: GetMap() != mpMap (KeyFrame.cc:503)
    template <class MapT> void skipOtherMaps(MapT* pMap) {
        kfSkip.assign(rows.size(), 0);
        for (size_t r = 0; r < rows.size(); ++r) kfSkip[r] = rows[r]->GetMap() != pMap ? 1 : 0;
    }

    // one library call; votes [nq][rows]
    std::vector<int32_t> call(orbm_t* m, int skipBad, int th) {
        const int nq = (int)qN.size(), nmp = (int)valid.size(), nobs = (int)row.size(), nrows = (int)rows.size();
        std::vector<int32_t> votes((size_t)nq * (nrows > 0 ? nrows : 1), 0);
        if (nq < 1 || nmp < 1 || nrows < 1) return votes;                   // no MapPoint anywhere: nobody votes
        static const int32_t zero = 0; static const uint8_t zero8 = 0;
        std::vector<int32_t> nVoted(nq), maxVotes(nq), nOver(nq);
        const int rc = orbm_covisibility_votes(m, nq, qStride, qMp.data(), qN.data(), selfRow.empty() ? nullptr : selfRow.data(), nrows, cap, counts.data(),
                                               kfSkip.empty() ? nullptr : kfSkip.data(), skipBad, nmp, nobs, off.data(), nobs ? row.data() : &zero,
                                               nobs ? slot.data() : &zero, nobs ? flags.data() : &zero8, valid.data(), th, 0, votes.data(), nVoted.data(),
                                               maxVotes.data(), nOver.data(), nullptr, nullptr);
        if (rc < 0) throw std::runtime_error(std::string("orbm_covisibility_votes: ") + orbm_last_error());
        return votes;
    }

    std::map<KeyFrameT*, int> counter(const std::vector<int32_t>& votes, size_t q) const {
        std::map<KeyFrameT*, int> out;
        for (size_t r = 0; r < rows.size(); ++r)
            if (votes[q * rows.size() + r] > 0) out[rows[r]] = votes[q * rows.size() + r];
        return out;
    }
};

// KeyFrame.cc:474-512 for every KeyFrame of vpKFs, which lie in one map, in one library call
template <class KeyFrameT>
std::vector<std::map<KeyFrameT*, int>> ConnectionCountsBatch(orbm_t* m, const std::vector<KeyFrameT*>& vpKFs) {
    typedef typename MapPointOf<KeyFrameT>::type MapPointT;
    std::vector<std::map<KeyFrameT*, int>> out(vpKFs.size());
    if (vpKFs.empty()) return out;
    std::vector<std::vector<MapPointT*>> queries;
    for (KeyFrameT* pKF : vpKFs) queries.push_back(pKF->GetMapPointMatches());
    Flat<KeyFrameT> F;
    F.build(queries, vpKFs);
    F.skipOtherMaps(vpKFs[0]->GetMap());
    for (KeyFrameT* pKF : vpKFs)
        if (pKF->GetMap() != vpKFs[0]->GetMap()) throw std::invalid_argument("ConnectionCountsBatch: the KeyFrames of one call lie in one map");
    const std::vector<int32_t> votes = F.call(m, 1, 15);
    for (size_t q = 0; q < vpKFs.size(); ++q) out[q] = F.counter(votes, q);
    return out;
}

// KFcounter of KeyFrame::UpdateConnections.  In the reference's text:
//     map<KeyFrame*,int> KFcounter = covis::ConnectionCounts(m, this);      // replaces :474-512
template <class KeyFrameT>
std::map<KeyFrameT*, int> ConnectionCounts(orbm_t* m, KeyFrameT* pKF) {
    return ConnectionCountsBatch(m, std::vector<KeyFrameT*>(1, pKF))[0];
}

// keyframeCounter of Tracking::UpdateLocalKeyFrames for mCurrentFrame (or mLastFrame, :3993): bad KeyFrames are counted (the reference
// drops them at :4033), no map test, no own row
template <class FrameT>
std::map<typename TypesOfFrame<FrameT>::KeyFrameT*, int> LocalKeyFrameVotes(orbm_t* m, FrameT& frame) {
    typedef typename TypesOfFrame<FrameT>::KeyFrameT KeyFrameT;
    typedef typename TypesOfFrame<FrameT>::MapPointT MapPointT;
    std::vector<MapPointT*> slots(frame.mvpMapPoints.begin(), frame.mvpMapPoints.begin() + frame.N);
    for (int i = 0; i < frame.N; ++i)
        if (frame.mvpMapPoints[i] && frame.mvpMapPoints[i]->isBad()) frame.mvpMapPoints[i] = NULL;   // :3986
    Flat<KeyFrameT> F;
    F.build(std::vector<std::vector<MapPointT*>>(1, slots), std::vector<KeyFrameT*>());
    return F.counter(F.call(m, 0, 15), 0);
}

// The arrays of one orbm_local_points call for one frame: pool rows = the KeyFrames in the order the reverse walk meets them
template <class KeyFrameT, class MapPointT = typename MapPointOf<KeyFrameT>::type> struct LocalFlat {
    std::map<KeyFrameT*, int> rowOf;
    std::map<MapPointT*, int> mpOf;
    std::vector<MapPointT*> mps;
    std::vector<int32_t> lkfRow, counts, kfMp;
    std::vector<uint8_t> valid;
    int cap = 1;

    void build(const std::vector<KeyFrameT*>& vpLocalKeyFrames) {
        std::vector<KeyFrameT*> rows;
        for (auto it = vpLocalKeyFrames.rbegin(); it != vpLocalKeyFrames.rend(); ++it) {   // the reverse iterator of :3924
            auto f = rowOf.find(*it);
            if (f == rowOf.end()) {
                f = rowOf.insert(std::make_pair(*it, (int)rows.size())).first;
                rows.push_back(*it);
                if ((*it)->N > cap) cap = (*it)->N;
            }
            lkfRow.push_back(f->second);
        }
        kfMp.assign(rows.size() * cap, -1);
        for (size_t r = 0; r < rows.size(); ++r) {
            const auto vpMPs = rows[r]->GetMapPointMatches();
            counts.push_back(rows[r]->N);
            for (size_t i = 0; i < vpMPs.size() && i < (size_t)cap; ++i) {
                MapPointT* pMP = vpMPs[i];
                if (!pMP) continue;
                auto it = mpOf.find(pMP);
                if (it == mpOf.end()) {
                    it = mpOf.insert(std::make_pair(pMP, (int)mps.size())).first;
                    mps.push_back(pMP); valid.push_back(pMP->isBad() ? 0 : 1);
                }
                kfMp[r * cap + i] = it->second;
            }
        }
    }
};

template <class KeyFrameT>
std::vector<typename MapPointOf<KeyFrameT>::type*> LocalMapPoints(orbm_t* m, const std::vector<KeyFrameT*>& vpLocalKeyFrames) {
    typedef typename MapPointOf<KeyFrameT>::type MapPointT;
    std::vector<MapPointT*> out;
    LocalFlat<KeyFrameT> F;
    F.build(vpLocalKeyFrames);
    const int nmp = (int)F.mps.size(), nl = (int)F.lkfRow.size();
    if (nmp < 1 || nl < 1) return out;
    std::vector<int32_t> localMp(nmp, -1);
    int32_t nTotal = 0, nq = 0;
    const int rc = orbm_local_points(m, 1, nl, F.lkfRow.data(), &nl, (int)F.counts.size(), F.cap, F.counts.data(), F.kfMp.data(), nmp, F.valid.data(), nmp,
                                     localMp.data(), &nTotal, &nq);
    if (rc < 0) throw std::runtime_error(std::string("orbm_local_points: ") + orbm_last_error());
    for (int i = 0; i < nq; ++i) out.push_back(F.mps[localMp[i]]);
    return out;
}

}  // namespace covis
}  // namespace ORB_SLAM3
