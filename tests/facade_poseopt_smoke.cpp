// Drives facade/PoseOptimization.h through the library on the mock types of tests/poseopt_mock.h: seeded scenes built in this file are
// optimised through the facade on the GPU and through the host run of csrc/orbm_poseopt.h (tests/poseopt_case_io.h); return value,
// mvbOutlier and the pose SetPose received must agree bit for bit; a frame with a second camera must be refused.
// Without a GPU it only proves that the templates compile and link (exit 0; exit 1 with an argument).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include "poseopt_mock.h"
#include "../orb-slam3_amd/facade/PoseOptimization.h"
#include "../include/orbx.h"

#define CHECK(cond, code) do { if (!(cond)) { std::printf("facade_poseopt_smoke: check failed at line %d (scene %d): %s\n", __LINE__, seed, #cond); return code; } } while (0)

struct Handle { orbm_t* h; orbm_t* handle() { return h; } };                 // stands in for facade/ORBmatcher.h's handle()

static void build(Case& c, unsigned seed) {
    unsigned s = seed * 2654435761u + 99u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f; };
    c.name = "scene"; c.nlevels = 8; c.haveUright = seed % 3 != 0;
    c.k[0] = 458.654f; c.k[1] = 457.296f; c.k[2] = 367.215f; c.k[3] = 248.375f; c.bf = 47.906f;
    c.ils2.resize(8);
    for (int l = 0; l < 8; ++l) c.ils2[l] = 1.f / std::pow(1.2f, 2.f * l);
    const int counts[] = {0, 2, 5, 40, 257, 700};
    c.n = counts[seed % 6] + (int)(rnd() * 30);
    const float yaw = 0.2f * rnd(), tx = rnd() - 0.5f, ty = rnd() - 0.5f, tz = rnd() - 0.5f;
    const float R[9] = {std::cos(yaw), 0.f, std::sin(yaw), 0.f, 1.f, 0.f, -std::sin(yaw), 0.f, std::cos(yaw)}, t[3] = {tx, ty, tz};
    c.x.resize(c.n); c.y.resize(c.n); c.ur.assign(c.n, -1.f); c.pw.assign(3 * (size_t)c.n, 0.f); c.octave.resize(c.n); c.has.assign(c.n, 0);
    for (int i = 0; i < c.n; ++i) {
        const float u = 30.f + 690.f * rnd(), v = 30.f + 420.f * rnd(), z = 2.f + 9.f * rnd();
        c.octave[i] = (int)(rnd() * 8) % 8;
        c.has[i] = rnd() < 0.7f || i < counts[seed % 6];
        const float Xc[3] = {(u - c.k[2]) * z / c.k[0], (v - c.k[3]) * z / c.k[1], z};
        for (int r = 0; r < 3; ++r) c.pw[3 * i + r] = R[r] * (Xc[0] - t[0]) + R[3 + r] * (Xc[1] - t[1]) + R[6 + r] * (Xc[2] - t[2]);   // R^T (Xc - t)
        const float sig = 0.6f * std::pow(1.2f, (float)c.octave[i]), off = rnd() < 0.15f ? 40.f : 0.f;
        c.x[i] = u + sig * (rnd() - 0.5f) + off; c.y[i] = v + sig * (rnd() - 0.5f);
        if (c.haveUright && rnd() < 0.5f) c.ur[i] = u - c.bf / z + sig * (rnd() - 0.5f);
    }
    const float e = 0.01f;                                                   // the start: off by a small rotation about z and a shift
    const float Rz[9] = {std::cos(e), -std::sin(e), 0.f, std::sin(e), std::cos(e), 0.f, 0.f, 0.f, 1.f};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) c.tcw[4 * r + k] = Rz[3 * r] * R[k] + Rz[3 * r + 1] * R[3 + k] + Rz[3 * r + 2] * R[6 + k];
        c.tcw[4 * r + 3] = Rz[3 * r] * t[0] + Rz[3 * r + 1] * t[1] + Rz[3 * r + 2] * t[2] + 0.02f * (float)(r + 1);
    }
}

int main(int argc, char** argv) {
    int seed = 0;
    const bool haveGpu = orbx_device_count() >= 1;
    orbm_t* m = nullptr;
    if (haveGpu) CHECK(orbm_create(&m, 0) == ORBM_OK, 2);
    Handle matcher{m};
    int nFrames = 0, nOptimised = 0, nFlagged = 0, nGoodAll = 0;
    for (seed = 0; seed < 18; ++seed) {
        Case c;
        build(c, (unsigned)seed);
        Frame F; std::vector<MapPoint> pool;
        frame_from_case(c, F, pool);
        if (!haveGpu) {                                                     // the instantiations are what this build proves
            if (seed == 0 && argc > 99) { ORB_SLAM3::PoseOptimization(matcher, &F); ORB_SLAM3::PoseOptimization(m, &F); }
            continue;
        }
        Result want;
        run(c, want);
        const int got = seed % 2 ? ORB_SLAM3::PoseOptimization(matcher, &F) : ORB_SLAM3::PoseOptimization(m, &F);
        CHECK(got == want.nGood, 3);
        for (int i = 0; i < c.n; ++i) CHECK(F.mvbOutlier[i] == (want.state[i] == PO_NONE ? true : want.state[i] == PO_OUTLIER), 4);
        CHECK(F.nSetPose == (want.nCorr >= 3 ? 1 : 0), 5);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 4; ++k) {
                const float a = F.mTcw.at<float>(r, k), b = want.nCorr >= 3 ? want.tcw[4 * r + k] : c.tcw[4 * r + k];
                CHECK(std::memcmp(&a, &b, 4) == 0, 6);
            }
        ++nFrames; nOptimised += want.nCorr >= 3; nGoodAll += got;
        for (int i = 0; i < c.n; ++i) nFlagged += want.state[i] == PO_OUTLIER;
        static const int camera2 = 0;
        F.mpCamera2 = &camera2;
        bool refused = false;
        try { ORB_SLAM3::PoseOptimization(m, &F); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused, 7);
    }
    if (!haveGpu) { std::printf("facade PoseOptimization compiled; no GPU here\n"); return argc > 1 ? 1 : 0; }
    seed = -1;
    CHECK(nFrames == 18 && nOptimised >= 12 && nFlagged > 100 && nGoodAll > 1000, 8);
    orbm_destroy(m);
    std::printf("facade_poseopt_smoke ok: %d frames, %d optimised, %d inliers, %d outliers flagged\n", nFrames, nOptimised, nGoodAll, nFlagged);
    return 0;
}
