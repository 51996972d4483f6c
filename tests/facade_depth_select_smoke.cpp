// Drives facade/FrameGeometry.h's SelectDepthPoints on mock vectors and compares it, entry for entry, with the walk of
// Tracking::UpdateLastFrame (Tracking.cc:3094-3163) written out in plain C++ in this file (std::sort over pair<float,int>).
// Without a GPU it only proves that the helper compiles and links (exit 0; exit 1 with an argument).
#include <algorithm>
#include <cstdio>
#include <limits>
#include <utility>
#include <vector>
#include "../orb-slam3_amd/facade/FrameGeometry.h"
#include "../include/orbx.h"

#define CHECK(cond, code) do { if (!(cond)) { std::printf("facade_depth_select_smoke: check failed at line %d: %s\n", __LINE__, #cond); return code; } } while (0)

static void expect_walk(const std::vector<float>& mvDepth, const std::vector<uint8_t>& keeps, float mThDepth, int maxPoint, std::vector<int>& order,
                        std::vector<uint8_t>& createNew) {
    order.clear(); createNew.assign(mvDepth.size(), 0);
    std::vector<std::pair<float, int> > vDepthIdx;
    for (int i = 0; i < (int)mvDepth.size(); i++) {
        float z = mvDepth[i];
        if (z > 0) vDepthIdx.push_back(std::make_pair(z, i));
    }
    if (vDepthIdx.empty()) return;
    std::sort(vDepthIdx.begin(), vDepthIdx.end());
    int nPoints = 0;
    for (size_t j = 0; j < vDepthIdx.size(); j++) {
        int i = vDepthIdx[j].second;
        order.push_back(i);
        bool bCreateNew = keeps.empty() || !keeps[i];
        if (bCreateNew) { createNew[i] = 1; nPoints++; } else { nPoints++; }
        if (vDepthIdx[j].first > mThDepth && nPoints > maxPoint) break;
    }
}

int main(int argc, char** argv) {
    const int n = 700;
    unsigned s = 77;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    std::vector<float> depth(n);
    std::vector<uint8_t> keeps(n);
    for (int i = 0; i < n; ++i) {
        const unsigned r = rnd();
        depth[i] = (r % 6 == 0) ? -1.f : (r % 5 == 0) ? 2.5f : 0.3f + (float)(r & 0xFFF) / 512.f;   // holes, ties at 2.5, 0.3 .. 8.3 m
        keeps[i] = rnd() % 3 == 0;
    }
    depth[3] = std::numeric_limits<float>::infinity(); depth[4] = std::numeric_limits<float>::quiet_NaN(); depth[5] = 0.f; depth[6] = 1e-40f;
    if (orbx_device_count() < 1) { std::printf("facade SelectDepthPoints compiled; no GPU here\n"); return argc > 1 ? 1 : 0; }
    orbm_t* m = nullptr;
    CHECK(orbm_create(&m, 0) == ORBM_OK, 2);
    std::vector<int> order, eorder; std::vector<uint8_t> cn, ecn;
    int total = 0;
    const float ths[] = {2.5f, 0.1f, 100.f, std::numeric_limits<float>::quiet_NaN()};
    for (float th : ths)
        for (int maxPoints : {100, 0, 650}) {
            const int nv = ORB_SLAM3::SelectDepthPoints(m, depth, keeps, th, maxPoints, order, cn);
            expect_walk(depth, keeps, th, maxPoints, eorder, ecn);
            CHECK(nv == (int)eorder.size() && order == eorder && cn == ecn, 3);
            total += nv;
        }
    // 150 far points: 101 visited, not 100; no keepsMp: every visited slot creates
    std::vector<float> far(150);
    for (int i = 0; i < 150; ++i) far[i] = 50.f + (float)(149 - i);
    const std::vector<uint8_t> nokeeps;
    CHECK(ORB_SLAM3::SelectDepthPoints(m, far, nokeeps, 40.f, 100, order, cn) == 101 && order.size() == 101 && order[0] == 149 && order[100] == 49, 4);
    CHECK(std::count(cn.begin(), cn.end(), 1) == 101 && cn[48] == 0 && cn[49] == 1, 5);
    // the denormal is the closest point of the first vector
    CHECK(ORB_SLAM3::SelectDepthPoints(m, depth, keeps, 2.5f, 100, order, cn) > 100 && order[0] == 6, 6);
    // an empty frame comes back empty without a call; a size mismatch and a refused argument throw
    const std::vector<float> none;
    CHECK(ORB_SLAM3::SelectDepthPoints(m, none, nokeeps, 40.f, 100, order, cn) == 0 && order.empty() && cn.empty(), 7);
    bool threw = false;
    try { ORB_SLAM3::SelectDepthPoints(m, far, keeps, 40.f, 100, order, cn); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw, 8);
    threw = false;
    try { ORB_SLAM3::SelectDepthPoints(m, far, nokeeps, 40.f, -1, order, cn); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw, 9);
    orbm_destroy(m);
    std::printf("facade_depth_select_smoke ok: %d slots visited over 12 walks\n", total);
    return 0;
}
