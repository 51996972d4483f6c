// KeyFrameDatabase::DetectRelocalizationCandidates up to lScoreAndMatch (KeyFrameDatabase.cc:869-923) as the reference runs it: one
// thread, std::vector<std::list<KeyFrame*>> for the inverted file, std::map<unsigned, double> for a BowVector, L1Scoring::score with its
// lower_bound walk (ScoringObject.cpp:23-68) restated in plain C++.  The baseline of tools/kfdb_query.py.  Not part of the product.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <utility>
#include <vector>

typedef std::map<unsigned, double> BowVector;
struct KeyFrame { BowVector mBowVec; long mnRelocQuery = -1; int mnRelocWords = 0; float mRelocScore = 0.f; };

static double l1(const BowVector& v1, const BowVector& v2) {
    BowVector::const_iterator a = v1.begin(), b = v2.begin();
    double score = 0;
    while (a != v1.end() && b != v2.end()) {
        const double vi = a->second, wi = b->second;
        if (a->first == b->first) { score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi); ++a; ++b; }
        else if (a->first < b->first) a = v1.lower_bound(b->first);
        else b = v2.lower_bound(a->first);
    }
    return -score / 2.0;
}

// db rows [nrows][cap] (word ascending, val, n); the query likewise.  Returns the median milliseconds of reps queries; the three counts
// let the caller compare with the device.
extern "C" double kfdb_query_host(int nwords, int nrows, int cap, const int32_t* word, const double* val, const int32_t* n, int qn, const int32_t* qword,
                                  const double* qval, int reps, int* nsharing_out, int* nscored_out, int* max_common_out) {
    std::vector<KeyFrame> kfs(nrows);
    std::vector<std::list<KeyFrame*> > inverted(nwords);
    for (int r = 0; r < nrows; ++r) {
        for (int i = 0; i < n[r]; ++i) kfs[r].mBowVec[(unsigned)word[(size_t)r * cap + i]] = val[(size_t)r * cap + i];
        for (BowVector::const_iterator it = kfs[r].mBowVec.begin(); it != kfs[r].mBowVec.end(); ++it) inverted[it->first].push_back(&kfs[r]);   // add, :40-47
    }
    BowVector q;
    for (int i = 0; i < qn; ++i) q[(unsigned)qword[i]] = qval[i];
    std::vector<double> ms;
    for (int rep = 0; rep < reps; ++rep) {
        const long id = 1000 + rep;
        const auto t0 = std::chrono::steady_clock::now();
        std::list<KeyFrame*> sharing;
        for (BowVector::const_iterator vit = q.begin(); vit != q.end(); ++vit) {
            std::list<KeyFrame*>& l = inverted[vit->first];
            for (std::list<KeyFrame*>::iterator lit = l.begin(); lit != l.end(); ++lit) {
                KeyFrame* k = *lit;
                if (k->mnRelocQuery != id) { k->mnRelocWords = 0; k->mnRelocQuery = id; sharing.push_back(k); }
                k->mnRelocWords++;
            }
        }
        int maxCommon = 0;
        for (KeyFrame* k : sharing) if (k->mnRelocWords > maxCommon) maxCommon = k->mnRelocWords;
        const int minCommon = maxCommon * 0.8f;
        std::list<std::pair<float, KeyFrame*> > scores;
        for (KeyFrame* k : sharing)
            if (k->mnRelocWords > minCommon) { const float si = (float)l1(q, k->mBowVec); k->mRelocScore = si; scores.push_back(std::make_pair(si, k)); }
        const auto t1 = std::chrono::steady_clock::now();
        ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        *nsharing_out = (int)sharing.size(); *nscored_out = (int)scores.size(); *max_common_out = maxCommon;
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}
