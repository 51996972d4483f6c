// Drives facade/Covisibility.h (ConnectionCounts, ConnectionCountsBatch, LocalKeyFrameVotes, LocalMapPoints) through the library on the
// mock types of tests/kfcull_mock.h / tests/covis_mock.h and compares every result with the reference's loops restated in plain C++
// (tests/covis_mock.h) on the same seeded maps: two-camera KeyFrames with left / right pairs and lone right entries, bad KeyFrames,
// KeyFrames of a second map, bad MapPoints, a MapPoint in two slots.
// Without a GPU it only proves that the templates compile and link (exit 0; exit 1 with an argument).
#include <cstdio>
#include <vector>
#include "covis_mock.h"
#include "../include/orbx.h"

#define CHECK(cond, code) do { if (!(cond)) { std::printf("facade_covis_smoke: check failed at line %d (map %d): %s\n", __LINE__, seed, #cond); return code; } } while (0)

static void build(MockMap& M, Map& other, Frame& frame, std::vector<KeyFrame*>& local, unsigned seed) {
    unsigned s = seed * 2654435761u + 777u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    static const int camera2Tag = 0;
    const int nkf = 6 + (int)(rnd() % 9);
    M.map.initId = 1000000;
    M.kfs.resize(nkf); M.mps.resize(30 + rnd() % 60);
    for (int k = 0; k < nkf; ++k) {
        KeyFrame& kf = M.kfs[k];
        kf.mnId = k; kf.mpMap = rnd() % 7 == 0 ? &other : &M.map;
        const int n = 2 * (6 + (int)(rnd() % 20));
        if (rnd() % 3 == 0) { kf.NLeft = n / 2; kf.mpCamera2 = &camera2Tag; }
        kf.setOctaves(std::vector<int>(n, 0));
        kf.mvuRight.assign(n, -1.f); kf.mvDepth.assign(n, -1.f);
    }
    for (MapPoint& mp : M.mps) {
        const int want = 1 + (int)(rnd() % 8);
        for (int t = 0; t < want; ++t) {
            KeyFrame& kf = M.kfs[rnd() % nkf];
            if (mp.mObservations.count(&kf)) continue;
            std::vector<int> freeL, freeR;
            for (int i = 0; i < kf.N; ++i) if (!kf.mvpMapPoints[i]) (kf.NLeft != -1 && i >= kf.NLeft ? freeR : freeL).push_back(i);
            const unsigned u = rnd() % 10;
            if (kf.NLeft != -1 && u < 4 && !freeL.empty() && !freeR.empty()) {
                kf.mvpMapPoints[freeL[0]] = &mp; mp.AddObservation(&kf, freeL[0]);
                kf.mvpMapPoints[freeR[0]] = &mp; mp.AddObservation(&kf, freeR[0]);
            } else if (kf.NLeft != -1 && u < 7 && !freeR.empty()) {
                kf.mvpMapPoints[freeR.back()] = &mp; mp.AddObservation(&kf, freeR.back());
            } else if (!freeL.empty()) {
                kf.mvpMapPoints[freeL.back()] = &mp; mp.AddObservation(&kf, freeL.back());
            }
        }
        if (rnd() % 10 == 0) mp.mbBad = true;
    }
    for (KeyFrame& kf : M.kfs) {
        if (rnd() % 6 == 0) kf.mbBad = true;
        if (rnd() % 3 == 0)                                                 // a MapPoint in a second slot
            for (int i = 0; i < kf.N; ++i) if (!kf.mvpMapPoints[i]) { kf.mvpMapPoints[i] = &M.mps[rnd() % M.mps.size()]; break; }
    }
    frame.N = (int)(rnd() % 50);
    for (int i = 0; i < frame.N; ++i) frame.mvpMapPoints.push_back(rnd() % 4 == 0 ? nullptr : &M.mps[rnd() % M.mps.size()]);
    const int nl = (int)(rnd() % 8);
    for (int i = 0; i < nl; ++i) local.push_back(&M.kfs[rnd() % nkf]);
}

int main(int argc, char** argv) {
    using namespace ORB_SLAM3;
    int seed = 0;
    const bool haveGpu = orbx_device_count() >= 1;
    orbm_t* m = nullptr;
    if (haveGpu) CHECK(orbm_create(&m, 0) == ORBM_OK, 2);
    int nVotes = 0, nBatch = 0, nLocal = 0, nCleared = 0;
    for (seed = 0; seed < 40; ++seed) {
        MockMap M; Map other; Frame frame; std::vector<KeyFrame*> local;
        build(M, other, frame, local, (unsigned)seed);
        if (!haveGpu) {                                                     // the instantiations are what this build proves
            if (seed == 0 && argc > 99) { covis::ConnectionCounts(m, &M.kfs[0]); covis::LocalKeyFrameVotes(m, frame); covis::LocalMapPoints(m, local); }
            continue;
        }
        std::vector<KeyFrame*> queries;
        for (KeyFrame& kf : M.kfs) if (!kf.isBad() && kf.GetMap() == &M.map) queries.push_back(&kf);
        const auto batch = covis::ConnectionCountsBatch(m, queries);
        CHECK(batch.size() == queries.size(), 3);
        for (size_t q = 0; q < queries.size(); ++q) {
            const std::map<KeyFrame*, int> want = ReferenceConnectionCounts(queries[q]);
            CHECK(batch[q] == want, 4);
            if (q < 2) CHECK(covis::ConnectionCounts(m, queries[q]) == want, 5);
            for (auto& kv : want) nVotes += kv.second;
        }
        nBatch += (int)queries.size();
        Frame twin = frame;
        const std::map<KeyFrame*, int> fv = covis::LocalKeyFrameVotes(m, frame);
        CHECK(fv == ReferenceLocalKeyFrameVotes(twin) && frame.mvpMapPoints == twin.mvpMapPoints, 6);
        for (int i = 0; i < frame.N; ++i) nCleared += !frame.mvpMapPoints[i];
        TrackTable track(M.mps);
        const std::vector<MapPoint*> lp = covis::LocalMapPoints(m, local);
        CHECK(lp == ReferenceLocalMapPoints(local, 1, track), 7);
        nLocal += (int)lp.size();
    }
    if (!haveGpu) { std::printf("facade Covisibility compiled; no GPU here\n"); return argc > 1 ? 1 : 0; }
    seed = -1;
    CHECK(nVotes > 2000 && nBatch > 150 && nLocal > 500 && nCleared > 100, 8);
    orbm_destroy(m);
    std::printf("facade_covis_smoke ok: %d votes over %d KeyFrame queries, %d local MapPoints, %d frame slots NULL\n", nVotes, nBatch, nLocal, nCleared);
    return 0;
}
