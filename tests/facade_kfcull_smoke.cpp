// Drives facade/KeyFrameCulling.h (KeyFrameCulling with and without the callback) on the mock types of tests/kfcull_mock.h and compares
// what it does to the map -- which KeyFrames are voted out, in which order, which are erased, which MapPoints go bad, every nObs --
// with LocalMapping.cc:1266-1399 restated in plain C++ (ReferenceKeyFrameCulling) on a twin of the same map.
// Build with -ffp-contract=off.  Without a GPU it only proves that the templates compile and link (exit 0; exit 1 with an argument).
#include <cstdio>
#include <vector>
#include "kfcull_mock.h"
#include "../include/orbx.h"

#define CHECK(cond, code) do { if (!(cond)) { std::printf("facade_kfcull_smoke: check failed at line %d (map %d): %s\n", __LINE__, seed, #cond); return code; } } while (0)

// a seeded map: mono or stereo (weight-2 entries), some two-camera and some not-erasable KeyFrames, MapPoints seen by 3 .. 9 KeyFrames
static void build(MockMap& M, unsigned seed, bool& bMonocular) {
    unsigned s = seed * 2654435761u + 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    static const int camera2Tag = 0;
    const bool stereo = rnd() % 2 == 0;
    bMonocular = !stereo;
    const int nkf = 6 + (int)(rnd() % 7);
    M.map.initId = 1;                                                       // the first KeyFrame is the map's initial one
    M.kfs.resize(nkf); M.mps.resize(20 + rnd() % 50);
    std::vector<std::vector<int>> freeSlots(nkf);
    static const int levels[8] = {1, 2, 2, 2, 2, 3, 3, 5};
    for (int k = 0; k < nkf; ++k) {
        KeyFrame& kf = M.kfs[k];
        kf.mnId = k + 1; kf.mpMap = &M.map;
        const int n = 8 + (int)(rnd() % 33);
        if (!stereo && rnd() % 5 == 0) { kf.NLeft = n / 2; kf.mpCamera2 = &camera2Tag; }
        std::vector<int> o(n);
        for (int& v : o) v = levels[rnd() % 8];
        kf.setOctaves(o);
        kf.mvuRight.assign(n, -1.f); kf.mvDepth.assign(n, -1.f);
        if (stereo) {
            static const float depths[4] = {1.f, 5.f, 35.f, 40.f};
            for (int i = 0; i < n; ++i) if (rnd() % 10 < 7) { kf.mvuRight[i] = 10.f; kf.mvDepth[i] = depths[rnd() % 4]; }
        }
        kf.mbNotErase = rnd() % 7 == 0;
        for (int i = 0; i < n; ++i) freeSlots[k].push_back(i);
    }
    for (MapPoint& mp : M.mps) {
        static const int wants[8] = {3, 3, 5, 6, 6, 7, 8, 9};
        const int want = wants[rnd() % 8];
        for (int t = 0; t < 40 && (int)mp.mObservations.size() < want; ++t) {
            const int k = (int)(rnd() % nkf);
            if (freeSlots[k].empty() || mp.mObservations.count(&M.kfs[k])) continue;
            const int at = (int)(rnd() % freeSlots[k].size());
            const int idx = freeSlots[k][at];
            freeSlots[k].erase(freeSlots[k].begin() + at);
            M.kfs[k].mvpMapPoints[idx] = &mp;
            mp.AddObservation(&M.kfs[k], idx);
        }
    }
    for (int k = nkf - 1; k >= 0; --k) M.covisible.push_back(&M.kfs[(k * 5 + 2) % nkf]);
    M.kfs[0].covisible = M.covisible;                                       // kfs[0] plays mpCurrentKeyFrame
}

int main(int argc, char** argv) {
    int seed = 0;
    const bool haveGpu = orbx_device_count() >= 1;
    orbm_t* m = nullptr;
    if (haveGpu) CHECK(orbm_create(&m, 0) == ORBM_OK, 2);
    int nVoted = 0, nErased = 0, nHeld = 0, nBadPoints = 0, nMulti = 0;
    const bool abortBA = false;
    for (seed = 0; seed < 40; ++seed) {
        MockMap A, B;
        bool bMonocular = true;
        build(A, (unsigned)seed, bMonocular); build(B, (unsigned)seed, bMonocular);
        const float th = seed % 3 == 2 ? 0.5f : 0.9f;
        if (!haveGpu) {                                                     // the instantiations are what this build proves
            if (seed == 0 && argc > 99) { ORB_SLAM3::KeyFrameCulling(m, &B.kfs[0], bMonocular, th, &abortBA); }
            continue;
        }
        const std::vector<KeyFrame*> want = ReferenceKeyFrameCulling(&A.kfs[0], bMonocular, th, &abortBA);
        std::vector<KeyFrame*> got;
        if (seed % 2) {
            ORB_SLAM3::KeyFrameCulling(m, &B.kfs[0], bMonocular, th, &abortBA, [&](KeyFrame* pKF) { got.push_back(pKF); pKF->SetBadFlag(); return true; });
            CHECK(got.size() == want.size(), 3);
            for (size_t i = 0; i < got.size(); ++i) CHECK(got[i] - &B.kfs[0] == want[i] - &A.kfs[0], 4);
        } else {
            ORB_SLAM3::KeyFrameCulling(m, &B.kfs[0], bMonocular, th, &abortBA);
        }
        CHECK(B.kfs[0].nUpdateBest == 1, 5);
        int erased = 0;
        for (size_t k = 0; k < A.kfs.size(); ++k) {
            CHECK(A.kfs[k].mbBad == B.kfs[k].mbBad && A.kfs[k].mbToBeErased == B.kfs[k].mbToBeErased, 6);
            for (int i = 0; i < A.kfs[k].N; ++i) CHECK((A.kfs[k].mvpMapPoints[i] == nullptr) == (B.kfs[k].mvpMapPoints[i] == nullptr), 7);
            erased += A.kfs[k].mbBad; nHeld += A.kfs[k].mbToBeErased;
        }
        for (size_t j = 0; j < A.mps.size(); ++j) {
            CHECK(A.mps[j].mbBad == B.mps[j].mbBad && A.mps[j].nObs == B.mps[j].nObs && A.mps[j].mObservations.size() == B.mps[j].mObservations.size(), 8);
            nBadPoints += A.mps[j].mbBad;
        }
        nVoted += (int)want.size(); nErased += erased; nMulti += erased > 1;
    }
    if (!haveGpu) { std::printf("facade KeyFrameCulling compiled; no GPU here\n"); return argc > 1 ? 1 : 0; }
    seed = -1;
    CHECK(nErased >= 20 && nMulti >= 5 && nHeld >= 3 && nBadPoints >= 20 && nVoted >= nErased, 9);   // the maps do exercise the sequential rule
    // the count rule: 104 empty KeyFrames and mbAbortBA set: the loop leaves after the KeyFrame with count 21
    {
        MockMap C;
        C.map.initId = 1000; C.kfs.resize(104);
        int visited = 0;
        for (int k = 0; k < 104; ++k) { C.kfs[k].mnId = k + 1; C.kfs[k].mpMap = &C.map; C.kfs[k].setOctaves(std::vector<int>(1, 2)); C.covisible.push_back(&C.kfs[k]); }
        C.kfs[0].covisible = C.covisible;
        const bool yes = true;
        ORB_SLAM3::KeyFrameCulling(m, &C.kfs[0], true, 0.9f, &yes, [&](KeyFrame*) { ++visited; return true; });
        CHECK(visited == 0, 10);
    }
    orbm_destroy(m);
    std::printf("facade_kfcull_smoke ok: %d votes, %d KeyFrames erased (%d maps with more than one), %d held, %d MapPoints gone bad\n", nVoted, nErased, nMulti,
                nHeld, nBadPoints);
    return 0;
}
