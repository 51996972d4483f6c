// KeyFrameDatabase.h -- KeyFrameDatabase::add / erase / clearMap (src/KeyFrameDatabase.cc:40-103), DetectRelocalizationCandidates
// (:869-981) and DetectNBestCandidates (:660-866) as drop-in templates over orbm_kfdb_query_batch_async of include/orbm.h.
//   KeyFrameDatabaseRows<KeyFrameT>   owns the device pool of BowVector rows: add appends a row, erase clears its db_active flag, and it
//                                     maps row <-> KeyFrame*.  The row index is the order of the add calls, which is the order of every
//                                     inverted-file list of the reference.
//   KeyFrameDatabase<KeyFrameT>       add, erase, clearMap, DetectRelocalizationCandidates(F, pMap),
//                                     DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates) with the reference's signatures
//   SelectRelocalizationCandidates / SelectNBestCandidates   everything behind the query, on three plain arrays per query (common,
//                                     first_word, score): they need no device and no library (tests/kfdb_facade.cpp)
// The inverted-file walk, the shared-word counts and the L1 scores run in liborbslam3_amd.so.  What stays here is the reference's own
// text: the maximum, `int minCommonWords = maxCommonWords*0.8f`, the covisibility accumulation, compFirst, `0.75f*bestAccScore`, the map
// tests and the duplicate set.
//
// List order.  lKFsSharingWords is rebuilt as the rows with common > 0 in (first_word, row) order: the reference visits the query's words
// in ascending order and each word's list in add order, and pushes a KeyFrame at the first word it shares (:877-891, :675-709).
//
// Members.  mnRelocQuery / mnRelocWords (mnPlaceRecognitionQuery / mnPlaceRecognitionWords) are written for every KeyFrame of the list,
// mRelocScore (mPlaceRecognitionScore) only where the reference writes it: for the KeyFrames above minCommonWords.  A neighbour that
// shares words but was not scored therefore contributes its OLD score to accScore, as at :943-946 / :777-780.  Two differences, both on
// values nobody reads: a KeyFrame that DetectNBestCandidates excludes as connected keeps its mnPlaceRecognitionWords (the reference
// leaves 1 there, :690-701, and never reads it, because its mnPlaceRecognitionQuery is not the query's), and the reference's test
// `mnRelocQuery != F->mnId` is taken as true for every KeyFrame: a query id is used for one query.
//
// The reference's DetectNBestCandidates never advances past a bad KeyFrame (:815-816: `continue` above `i++; it++`), so it spins forever
// once one heads the list.  SelectNBestCandidates advances past it.
//
// FrameT: mnId, mBowVec (iterates (word, value) in ascending word order: DBoW2::BowVector).  KeyFrameT: mnId, mBowVec, the six members
// above, GetBestCovisibilityKeyFrames(int), GetConnectedKeyFrames() -> std::set<KeyFrameT*>, GetMap(), isBad(); its map type: IsBad().
// DetectLoopCandidates, DetectCandidates and DetectBestCandidates have no caller in the reference and are not provided.
#pragma once
#include <algorithm>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../include/orbm.h"
#include "../../include/orbx.h"

namespace ORB_SLAM3 {

namespace kfdb {

// bool KeyFrameDatabase::compFirst(a, b) (include/KeyFrameDatabase.h): descending by score
template <class KeyFrameT> inline bool compFirst(const std::pair<float, KeyFrameT*>& a, const std::pair<float, KeyFrameT*>& b) { return a.first > b.first; }

// the rows with common > 0 in (first_word, row) order: lKFsSharingWords as row indices
inline std::vector<int> SharingOrder(int nrows, const int32_t* common, const int32_t* first_word) {
    std::vector<int> order;
    for (int r = 0; r < nrows; ++r) if (common[r] > 0) order.push_back(r);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first_word[a] < first_word[b]; });
    return order;
}

}  // namespace kfdb

// DetectRelocalizationCandidates from :894 on.  rows[r] is the KeyFrame of database row r; common / first_word / score are row q of the
// query's outputs; queryId = F->mnId.
template <class KeyFrameT, class MapT>
std::vector<KeyFrameT*> SelectRelocalizationCandidates(const std::vector<KeyFrameT*>& rows, long unsigned int queryId, MapT* pMap,
                                                       const int32_t* common, const int32_t* first_word, const float* score) {
    using namespace std;
    const vector<int> order = kfdb::SharingOrder((int)rows.size(), common, first_word);
    list<KeyFrameT*> lKFsSharingWords;
    map<KeyFrameT*, int> rowOf;
    for (int r : order) {                                                   // :884-890
        KeyFrameT* pKFi = rows[r];
        pKFi->mnRelocWords = common[r];
        pKFi->mnRelocQuery = queryId;
        lKFsSharingWords.push_back(pKFi);
        rowOf[pKFi] = r;
    }
    if (lKFsSharingWords.empty())
        return vector<KeyFrameT*>();

    // Only compare against those keyframes that share enough words
    int maxCommonWords = 0;
    for (typename list<KeyFrameT*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
        if ((*lit)->mnRelocWords > maxCommonWords)
            maxCommonWords = (*lit)->mnRelocWords;
    }

    int minCommonWords = maxCommonWords * 0.8f;

    list<pair<float, KeyFrameT*> > lScoreAndMatch;

    // Compute similarity score.
    for (typename list<KeyFrameT*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
        KeyFrameT* pKFi = *lit;

        if (pKFi->mnRelocWords > minCommonWords) {
            float si = score[rowOf[pKFi]];                                  // mpVoc->score(F->mBowVec, pKFi->mBowVec), :919
            pKFi->mRelocScore = si;
            lScoreAndMatch.push_back(make_pair(si, pKFi));
        }
    }

    if (lScoreAndMatch.empty())
        return vector<KeyFrameT*>();

    list<pair<float, KeyFrameT*> > lAccScoreAndMatch;
    float bestAccScore = 0;

    // Lets now accumulate score by covisibility
    for (typename list<pair<float, KeyFrameT*> >::iterator it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
        KeyFrameT* pKFi = it->second;
        vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);

        float bestScore = it->first;
        float accScore = bestScore;
        KeyFrameT* pBestKF = pKFi;
        for (typename vector<KeyFrameT*>::iterator vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
            KeyFrameT* pKF2 = *vit;
            if (pKF2->mnRelocQuery != queryId)
                continue;

            accScore += pKF2->mRelocScore;
            if (pKF2->mRelocScore > bestScore) {
                pBestKF = pKF2;
                bestScore = pKF2->mRelocScore;
            }
        }
        lAccScoreAndMatch.push_back(make_pair(accScore, pBestKF));
        if (accScore > bestAccScore)
            bestAccScore = accScore;
    }

    // Return all those keyframes with a score higher than 0.75*bestScore
    float minScoreToRetain = 0.75f * bestAccScore;
    set<KeyFrameT*> spAlreadyAddedKF;
    vector<KeyFrameT*> vpRelocCandidates;
    vpRelocCandidates.reserve(lAccScoreAndMatch.size());
    for (typename list<pair<float, KeyFrameT*> >::iterator it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
        const float& si = it->first;
        if (si > minScoreToRetain) {
            KeyFrameT* pKFi = it->second;
            if (pKFi->GetMap() != pMap)
                continue;
            if (!spAlreadyAddedKF.count(pKFi)) {
                vpRelocCandidates.push_back(pKFi);
                spAlreadyAddedKF.insert(pKFi);
            }
        }
    }

    return vpRelocCandidates;
}

// DetectNBestCandidates from :712 on.  The query ran with exclude = spConnectedKF.count(rows[r]) (:692), so a connected KeyFrame has
// common 0 and is not in the list.
template <class KeyFrameT>
void SelectNBestCandidates(const std::vector<KeyFrameT*>& rows, KeyFrameT* pKF, const int32_t* common, const int32_t* first_word, const float* score,
                           std::vector<KeyFrameT*>& vpLoopCand, std::vector<KeyFrameT*>& vpMergeCand, int nNumCandidates) {
    using namespace std;
    const vector<int> order = kfdb::SharingOrder((int)rows.size(), common, first_word);
    list<KeyFrameT*> lKFsSharingWords;
    map<KeyFrameT*, int> rowOf;
    for (int r : order) {                                                   // :687-701
        KeyFrameT* pKFi = rows[r];
        pKFi->mnPlaceRecognitionWords = common[r];
        pKFi->mnPlaceRecognitionQuery = pKF->mnId;
        lKFsSharingWords.push_back(pKFi);
        rowOf[pKFi] = r;
    }
    if (lKFsSharingWords.empty())
        return;

    // Only compare against those keyframes that share enough words
    int maxCommonWords = 0;
    for (typename list<KeyFrameT*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
        if ((*lit)->mnPlaceRecognitionWords > maxCommonWords)
            maxCommonWords = (*lit)->mnPlaceRecognitionWords;
    }

    int minCommonWords = maxCommonWords * 0.8f;

    list<pair<float, KeyFrameT*> > lScoreAndMatch;

    // Compute similarity score.
    for (typename list<KeyFrameT*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
        KeyFrameT* pKFi = *lit;

        if (pKFi->mnPlaceRecognitionWords > minCommonWords) {
            float si = score[rowOf[pKFi]];                                  // mpVoc->score(pKF->mBowVec, pKFi->mBowVec), :743
            pKFi->mPlaceRecognitionScore = si;
            lScoreAndMatch.push_back(make_pair(si, pKFi));
        }
    }

    if (lScoreAndMatch.empty())
        return;

    list<pair<float, KeyFrameT*> > lAccScoreAndMatch;
    float bestAccScore = 0;

    // Lets now accumulate score by covisibility
    for (typename list<pair<float, KeyFrameT*> >::iterator it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
        KeyFrameT* pKFi = it->second;
        vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);

        float bestScore = it->first;
        float accScore = bestScore;
        KeyFrameT* pBestKF = pKFi;
        for (typename vector<KeyFrameT*>::iterator vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
            KeyFrameT* pKF2 = *vit;
            if (pKF2->mnPlaceRecognitionQuery != pKF->mnId)
                continue;

            accScore += pKF2->mPlaceRecognitionScore;
            if (pKF2->mPlaceRecognitionScore > bestScore) {
                pBestKF = pKF2;
                bestScore = pKF2->mPlaceRecognitionScore;
            }
        }
        lAccScoreAndMatch.push_back(make_pair(accScore, pBestKF));
        if (accScore > bestAccScore)
            bestAccScore = accScore;
    }

    lAccScoreAndMatch.sort(kfdb::compFirst<KeyFrameT>);

    vpLoopCand.reserve(nNumCandidates);
    vpMergeCand.reserve(nNumCandidates);
    set<KeyFrameT*> spAlreadyAddedKF;
    size_t i = 0;
    typename list<pair<float, KeyFrameT*> >::iterator it = lAccScoreAndMatch.begin();
    while (i < lAccScoreAndMatch.size() && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates)) {
        KeyFrameT* pKFi = it->second;
        if (pKFi->isBad()) {                                                // the reference `continue`s here without advancing (:815-816) and never returns
            i++;
            it++;
            continue;
        }

        if (!spAlreadyAddedKF.count(pKFi)) {
            if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() < nNumCandidates) {
                vpLoopCand.push_back(pKFi);
            } else if (pKF->GetMap() != pKFi->GetMap() && (int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad()) {
                vpMergeCand.push_back(pKFi);
            }
            spAlreadyAddedKF.insert(pKFi);
        }
        i++;
        it++;
    }
}

// The device pool.  db_cap is fixed when the pool is made (the most words a BowVector can hold: the extractor's nFeatures); the number of
// rows grows by doubling, the host mirror re-uploaded into the new block.  A row is never reused: erase only clears its flag, so that the
// rows that remain keep the order of their add calls.
template <class KeyFrameT> class KeyFrameDatabaseRows {
public:
    KeyFrameDatabaseRows(orbm_t* m, int db_cap) : m_(m), cap_(db_cap) {
        if (!m || db_cap < 1 || db_cap > 65535) throw std::invalid_argument("KeyFrameDatabaseRows: a matcher handle and 1 <= db_cap <= 65535");
    }
    ~KeyFrameDatabaseRows() { release(); }
    KeyFrameDatabaseRows(const KeyFrameDatabaseRows&) = delete;
    KeyFrameDatabaseRows& operator=(const KeyFrameDatabaseRows&) = delete;

    int size() const { return (int)rows_.size(); }
    int cap() const { return cap_; }
    orbm_t* matcher() const { return m_; }
    const std::vector<KeyFrameT*>& rows() const { return rows_; }
    int rowOf(KeyFrameT* pKF) const { auto it = rowOf_.find(pKF); return it == rowOf_.end() ? -1 : it->second; }
    const int32_t* dWord() const { return dWord_; }
    const double* dVal() const { return dVal_; }
    const int32_t* dN() const { return dN_; }
    const uint8_t* dActive() const { return dActive_; }
    int rowsAllocated() const { return alloc_; }

    // KeyFrameDatabase::add (:40-47)
    void add(KeyFrameT* pKF) {
        if (rowOf_.count(pKF)) throw std::invalid_argument("KeyFrameDatabaseRows::add: the KeyFrame has a row already");
        const int r = (int)rows_.size();
        if (r >= ORBM_KFDB_MAX_ROWS) throw std::length_error("KeyFrameDatabaseRows::add: ORBM_KFDB_MAX_ROWS rows");
        std::vector<int32_t> w; std::vector<double> v;
        flatten(pKF->mBowVec, cap_, w, v);
        hWord_.insert(hWord_.end(), w.begin(), w.end()); hWord_.resize((size_t)(r + 1) * cap_, 0);
        hVal_.insert(hVal_.end(), v.begin(), v.end()); hVal_.resize((size_t)(r + 1) * cap_, 0.0);
        hN_.push_back((int32_t)w.size()); hActive_.push_back(1);
        rows_.push_back(pKF); rowOf_[pKF] = r;
        if (r >= alloc_) grow();
        else {
            up(dWord_ + (size_t)r * cap_, &hWord_[(size_t)r * cap_], sizeof(int32_t) * cap_);
            up(dVal_ + (size_t)r * cap_, &hVal_[(size_t)r * cap_], sizeof(double) * cap_);
            up(dN_ + r, &hN_[r], sizeof(int32_t)); up(dActive_ + r, &hActive_[r], 1);
        }
    }
    // KeyFrameDatabase::erase (:50-70): the KeyFrame leaves every list
    void erase(KeyFrameT* pKF) {
        const int r = rowOf(pKF);
        if (r < 0 || !hActive_[r]) return;
        hActive_[r] = 0;
        up(dActive_ + r, &hActive_[r], 1);
    }
    // KeyFrameDatabase::clearMap (:79-103)
    template <class MapT> void clearMap(MapT* pMap) {
        for (size_t r = 0; r < rows_.size(); ++r) if (hActive_[r] && rows_[r]->GetMap() == pMap) erase(rows_[r]);
    }

    // (word, value) pairs of a BowVector as two arrays; more than cap words do not fit a row
    template <class BowT> static void flatten(const BowT& bow, int cap, std::vector<int32_t>& w, std::vector<double>& v) {
        for (auto it = bow.begin(); it != bow.end(); ++it) { w.push_back((int32_t)it->first); v.push_back((double)it->second); }
        if ((int)w.size() > cap) throw std::length_error("KeyFrameDatabaseRows: a BowVector of " + std::to_string(w.size()) + " words, db_cap " + std::to_string(cap));
    }
    static void up(const void* dst, const void* src, size_t bytes) {
        if (orbx_memcpy_h2d(const_cast<void*>(dst), src, bytes) != 0) throw std::runtime_error("KeyFrameDatabaseRows: upload failed");
    }

private:
    void release() {
        orbx_dev_free(dWord_); orbx_dev_free(dVal_); orbx_dev_free(dN_); orbx_dev_free(dActive_);
        dWord_ = nullptr; dVal_ = nullptr; dN_ = nullptr; dActive_ = nullptr;
    }
    void grow() {
        orbm_sync(m_);                                                      // a query still running reads the old block
        const int n = std::max(64, alloc_ * 2);
        release();
        dWord_ = (int32_t*)orbx_dev_alloc(sizeof(int32_t) * (size_t)n * cap_); dVal_ = (double*)orbx_dev_alloc(sizeof(double) * (size_t)n * cap_);
        dN_ = (int32_t*)orbx_dev_alloc(sizeof(int32_t) * n); dActive_ = (uint8_t*)orbx_dev_alloc(n);
        if (!dWord_ || !dVal_ || !dN_ || !dActive_) throw std::runtime_error("KeyFrameDatabaseRows: device allocation failed");
        alloc_ = n;
        up(dWord_, hWord_.data(), sizeof(int32_t) * hWord_.size()); up(dVal_, hVal_.data(), sizeof(double) * hVal_.size());
        up(dN_, hN_.data(), sizeof(int32_t) * hN_.size()); up(dActive_, hActive_.data(), hActive_.size());
    }

    orbm_t* m_;
    int cap_, alloc_ = 0;
    std::vector<KeyFrameT*> rows_;
    std::map<KeyFrameT*, int> rowOf_;
    std::vector<int32_t> hWord_, hN_;
    std::vector<double> hVal_;
    std::vector<uint8_t> hActive_;
    int32_t *dWord_ = nullptr, *dN_ = nullptr;
    double* dVal_ = nullptr;
    uint8_t* dActive_ = nullptr;
};

template <class KeyFrameT> class KeyFrameDatabase {
public:
    KeyFrameDatabase(orbm_t* m, int db_cap) : pool_(m, db_cap) {}
    ~KeyFrameDatabase() { orbx_dev_free(dQ_); orbx_dev_free(dOut_); }

    void add(KeyFrameT* pKF) { pool_.add(pKF); }
    void erase(KeyFrameT* pKF) { pool_.erase(pKF); }
    template <class MapT> void clearMap(MapT* pMap) { pool_.clearMap(pMap); }
    KeyFrameDatabaseRows<KeyFrameT>& Rows() { return pool_; }

    // Relocalization (:869-981)
    template <class FrameT, class MapT> std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F, MapT* pMap) {
        if (pool_.size() == 0) return std::vector<KeyFrameT*>();
        query(F->mBowVec, nullptr);
        return SelectRelocalizationCandidates(pool_.rows(), F->mnId, pMap, common_.data(), first_.data(), score_.data());
    }

    // Loop and merge candidates (:660-866)
    void DetectNBestCandidates(KeyFrameT* pKF, std::vector<KeyFrameT*>& vpLoopCand, std::vector<KeyFrameT*>& vpMergeCand, int nNumCandidates) {
        if (pool_.size() == 0) return;
        const std::set<KeyFrameT*> spConnectedKF = pKF->GetConnectedKeyFrames();      // :672
        std::vector<uint8_t> exclude(pool_.size(), 0);
        for (KeyFrameT* c : spConnectedKF) { const int r = pool_.rowOf(c); if (r >= 0) exclude[r] = 1; }
        query(pKF->mBowVec, exclude.data());
        SelectNBestCandidates(pool_.rows(), pKF, common_.data(), first_.data(), score_.data(), vpLoopCand, vpMergeCand, nNumCandidates);
    }

private:
    // one query against the pool: the BowVector goes up as a one-row pool, three rows come back
    template <class BowT> void query(const BowT& bow, const uint8_t* exclude) {
        const int n = pool_.size(), cap = pool_.cap();
        std::vector<int32_t> w; std::vector<double> v;
        KeyFrameDatabaseRows<KeyFrameT>::flatten(bow, cap, w, v);
        const int32_t head[2] = {0, (int32_t)w.size()};                     // q_row[0], q_n[0]
        w.resize(cap, 0); v.resize(cap, 0.0);
        // the query block: val [cap] | word [cap] | q_row, q_n | exclude [rows]; the result block: common, first_word, score, four counts, scored
        const size_t oWord = sizeof(double) * cap, oHead = oWord + sizeof(int32_t) * cap, oExc = oHead + 8;
        if (pool_.rowsAllocated() > outRows_) {
            orbm_sync(pool_.matcher());
            orbx_dev_free(dQ_); orbx_dev_free(dOut_);
            outRows_ = pool_.rowsAllocated();
            dQ_ = (uint8_t*)orbx_dev_alloc(oExc + outRows_);
            dOut_ = (uint8_t*)orbx_dev_alloc((size_t)outRows_ * 13 + 16);
            if (!dQ_ || !dOut_) throw std::runtime_error("KeyFrameDatabase: device allocation failed");
        }
        typedef KeyFrameDatabaseRows<KeyFrameT> R;
        R::up(dQ_, v.data(), sizeof(double) * cap); R::up(dQ_ + oWord, w.data(), sizeof(int32_t) * cap); R::up(dQ_ + oHead, head, 8);
        if (exclude) R::up(dQ_ + oExc, exclude, n);
        int32_t* dCommon = (int32_t*)dOut_; int32_t* dFirst = dCommon + outRows_; float* dScore = (float*)(dFirst + outRows_);
        int32_t* dCnt = (int32_t*)(dScore + outRows_); uint8_t* dScored = (uint8_t*)(dCnt + 4);
        const int rc = orbm_kfdb_query_batch_async(pool_.matcher(), 1, (const int32_t*)(dQ_ + oHead), 1, cap, (const int32_t*)(dQ_ + oWord), (const double*)dQ_,
                                                   (const int32_t*)(dQ_ + oHead + 4), n, cap, pool_.dWord(), pool_.dVal(), pool_.dN(), pool_.dActive(),
                                                   exclude ? dQ_ + oExc : nullptr, dCommon, dFirst, dScore, dScored, dCnt, dCnt + 1, dCnt + 2, dCnt + 3);
        if (rc < 0) throw std::runtime_error(std::string("orbm_kfdb_query_batch_async: ") + orbm_last_error());
        if (orbm_sync(pool_.matcher()) < 0) throw std::runtime_error(std::string("orbm_sync: ") + orbm_last_error());
        common_.resize(n); first_.resize(n); score_.resize(n);
        if (orbx_memcpy_d2h(common_.data(), dCommon, sizeof(int32_t) * n) != 0 || orbx_memcpy_d2h(first_.data(), dFirst, sizeof(int32_t) * n) != 0 ||
            orbx_memcpy_d2h(score_.data(), dScore, sizeof(float) * n) != 0)
            throw std::runtime_error("KeyFrameDatabase: download failed");
    }

    KeyFrameDatabaseRows<KeyFrameT> pool_;
    uint8_t *dQ_ = nullptr, *dOut_ = nullptr;
    int outRows_ = 0;
    std::vector<int32_t> common_, first_;
    std::vector<float> score_;
};

}  // namespace ORB_SLAM3
