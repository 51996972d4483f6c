// Drives facade/KeyFrameDatabase.h on mock KeyFrame / Frame / Map types from a text file of cases (tests/kfdb_cases.py: facade_text) and
// prints, per case, the candidate lists as row indices and the members of every row afterwards.
//   kfdb_facade select FILE   SelectRelocalizationCandidates / SelectNBestCandidates on the three result rows the file carries: no
//                             device, no library (build with g++ -ffp-contract=off)
//   kfdb_facade device FILE   KeyFrameDatabase<KeyFrame>: add, erase, the query on the device, the same selection (build with
//                             -DKFDB_WITH_LIBRARY and link liborbslam3_amd.so)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "../orb-slam3_amd/facade/KeyFrameDatabase.h"

struct Map {
    bool bad = false;
    bool IsBad() const { return bad; }
};

struct KeyFrame {
    long unsigned int mnId = 0;
    std::map<unsigned, double> mBowVec;
    long unsigned int mnRelocQuery = (long unsigned int)-1, mnPlaceRecognitionQuery = (long unsigned int)-1;
    int mnRelocWords = 0, mnPlaceRecognitionWords = 0;
    float mRelocScore = 0.f, mPlaceRecognitionScore = 0.f;
    Map* map = nullptr;
    bool bad = false;
    std::vector<KeyFrame*> covisible;
    std::set<KeyFrame*> connected;
    Map* GetMap() const { return map; }
    bool isBad() const { return bad; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(int n) const {
        return (int)covisible.size() < n ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + n);
    }
    std::set<KeyFrame*> GetConnectedKeyFrames() const { return connected; }
};

struct Frame {
    long unsigned int mnId = 0;
    std::map<unsigned, double> mBowVec;
};

static double from_bits64(unsigned long long b) { double d; std::memcpy(&d, &b, 8); return d; }
static float from_bits32(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
static unsigned bits32(float f) { unsigned b; std::memcpy(&b, &f, 4); return b; }

static void read_bow(std::istream& in, std::map<unsigned, double>& bow) {
    int n; in >> n;
    std::vector<unsigned> ids(n);
    for (int i = 0; i < n; ++i) in >> ids[i];
    for (int i = 0; i < n; ++i) { unsigned long long b; in >> b; bow[ids[i]] = from_bits64(b); }
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: kfdb_facade select|device FILE\n"); return 2; }
    const bool device = std::strcmp(argv[1], "device") == 0;
    std::ifstream in(argv[2]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
#ifdef KFDB_WITH_LIBRARY
    orbm_t* m = nullptr;
    if (device && orbm_create(&m, 0) != ORBM_OK) { std::fprintf(stderr, "orbm_create: %s\n", orbm_last_error()); return 3; }
#else
    if (device) { std::fprintf(stderr, "built without the library\n"); return 2; }
#endif
    int ncases; in >> ncases;
    for (int c = 0; c < ncases; ++c) {
        int place, nrows, queryMap, nNum, nmaps, dbCap; long unsigned int queryId;
        in >> place >> nrows >> queryId >> queryMap >> nNum >> nmaps >> dbCap;
        std::vector<Map> maps(nmaps);
        for (int i = 0; i < nmaps; ++i) { int b; in >> b; maps[i].bad = b != 0; }
        std::map<unsigned, double> qbow;
        read_bow(in, qbow);
        std::vector<KeyFrame> kfs(nrows);
        std::vector<int> active(nrows), exclude(nrows);
        std::vector<std::vector<int>> cov(nrows);
        for (int r = 0; r < nrows; ++r) {
            KeyFrame& kf = kfs[r];
            int mp, bad, words, ncov; unsigned sb;
            in >> mp >> bad >> active[r] >> exclude[r] >> words >> sb >> ncov;
            kf.mnId = 100 + r; kf.map = &maps[mp]; kf.bad = bad != 0;
            kf.mnRelocWords = kf.mnPlaceRecognitionWords = words;
            kf.mRelocScore = kf.mPlaceRecognitionScore = from_bits32(sb);
            cov[r].resize(ncov);
            for (int i = 0; i < ncov; ++i) in >> cov[r][i];
            read_bow(in, kf.mBowVec);
        }
        for (int r = 0; r < nrows; ++r) for (int i : cov[r]) kfs[r].covisible.push_back(&kfs[i]);
        std::vector<int32_t> common(nrows), first(nrows);
        std::vector<float> score(nrows);
        for (int r = 0; r < nrows; ++r) in >> common[r];
        for (int r = 0; r < nrows; ++r) in >> first[r];
        for (int r = 0; r < nrows; ++r) { unsigned b; in >> b; score[r] = from_bits32(b); }
        if (!in) { std::fprintf(stderr, "case %d: the file ends early\n", c); return 2; }

        std::vector<KeyFrame*> rows;
        for (auto& kf : kfs) rows.push_back(&kf);
        std::map<KeyFrame*, int> rowOf;
        for (int r = 0; r < nrows; ++r) rowOf[rows[r]] = r;
        KeyFrame query; query.mnId = queryId; query.map = &maps[queryMap]; query.mBowVec = qbow;
        for (int r = 0; r < nrows; ++r) if (exclude[r]) query.connected.insert(rows[r]);
        Frame frame; frame.mnId = queryId; frame.mBowVec = qbow;
        std::vector<KeyFrame*> reloc, loop, merge;
        if (!device) {
            if (place) ORB_SLAM3::SelectNBestCandidates(rows, &query, common.data(), first.data(), score.data(), loop, merge, nNum);
            else reloc = ORB_SLAM3::SelectRelocalizationCandidates(rows, frame.mnId, &maps[queryMap], common.data(), first.data(), score.data());
        }
#ifdef KFDB_WITH_LIBRARY
        else {
            ORB_SLAM3::KeyFrameDatabase<KeyFrame> db(m, dbCap);
            for (KeyFrame* kf : rows) db.add(kf);
            for (int r = 0; r < nrows; ++r) if (!active[r]) db.erase(rows[r]);
            if (place) db.DetectNBestCandidates(&query, loop, merge, nNum);
            else reloc = db.DetectRelocalizationCandidates(&frame, &maps[queryMap]);
        }
#endif
        std::printf("case %d", c);
        auto list = [&](const char* tag, const std::vector<KeyFrame*>& v) {
            std::printf(" %s %zu", tag, v.size());
            for (KeyFrame* kf : v) std::printf(" %d", rowOf[kf]);
        };
        if (place) { list("L", loop); list("M", merge); } else list("R", reloc);
        std::printf("\n");
        for (int r = 0; r < nrows; ++r) {
            const KeyFrame& kf = kfs[r];
            if (place) std::printf("%lld %d %u\n", (long long)kf.mnPlaceRecognitionQuery, kf.mnPlaceRecognitionWords, bits32(kf.mPlaceRecognitionScore));
            else std::printf("%lld %d %u\n", (long long)kf.mnRelocQuery, kf.mnRelocWords, bits32(kf.mRelocScore));
        }
    }
#ifdef KFDB_WITH_LIBRARY
    if (m) orbm_destroy(m);
#endif
    return 0;
}
