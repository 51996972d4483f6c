// facade_triangulate_smoke.cpp -- facade/CreateNewMapPoints.h end to end on the GPU with mock KeyFrames: a synthetic current KeyFrame and
// three neighbours (one closer than the stereo baseline, so it must not be passed), matches handed out by a mock matcher, ONE
// orbm_triangulate_new_points call behind the template.  The callback must see the reference's creation order and points that
// reproject onto both keypoints.  `facade_triangulate_smoke need-gpu` fails without a device; without the argument it skips.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "../orb-slam3_amd/facade/CreateNewMapPoints.h"
#include "triangulate_mock.h"

using namespace ORB_SLAM3;

int main(int argc, char** argv) {
    orbm_t* h = nullptr;
    if (orbm_create(&h, 0) != ORBM_OK) {
        if (argc > 1 && !strcmp(argv[1], "need-gpu")) { fprintf(stderr, "no device: %s\n", orbm_last_error()); return 1; }
        printf("facade_triangulate_smoke skipped (no device)\n"); return 0;
    }
    const int n = 200, P = 3;
    TriCase c;
    c.ng = 1; c.npairs = P; c.nl = 8;
    c.fl = {420.f, 420.f, 376.f, 240.f, 1.f / 420.f, 1.f / 420.f, 420.f, 420.f, 376.f, 240.f, 1.f / 420.f, 1.f / 420.f, 0.11f, 46.2f, 0.11f, 1.8f, 0.f};
    float s = 1.f;
    for (int l = 0; l < 8; ++l) { c.sf1.push_back(s); c.ls1.push_back(s * s); s *= 1.2f; }
    c.sf2 = c.sf1; c.ls2 = c.ls1;
    auto pool = [&](Pool& p, int rows) {
        p.rows = rows; p.cap = n; const size_t t = (size_t)rows * n;
        p.ux.assign(t, 0); p.uy.assign(t, 0); p.kx.assign(t, 0); p.ky.assign(t, 0); p.uright.assign(t, -1.f); p.depth.assign(t, -1.f); p.octave.assign(t, 0);
        p.counts.assign(rows, n); p.tcw.assign(12 * (size_t)rows, 0); p.ow.assign(3 * (size_t)rows, 0);
        for (int r = 0; r < rows; ++r) { p.tcw[12 * r] = 1; p.tcw[12 * r + 5] = 1; p.tcw[12 * r + 10] = 1; }
    };
    pool(c.a, 1); pool(c.b, P);
    const float bx[P] = {0.05f, 0.4f, -0.6f};                               // neighbour 0 is closer than mb = 0.11: skipped by the baseline test
    for (int p = 0; p < P; ++p) { c.b.tcw[12 * p + 3] = -bx[p]; c.b.ow[3 * p] = bx[p]; }
    c.gs = {0, P}; c.row1.assign(P, 0); c.row2 = {0, 1, 2}; c.m12.assign((size_t)P * n, -1);
    std::vector<float> X(3 * n);
    unsigned rs = 12345u;
    auto rnd = [&]() { rs = rs * 1664525u + 1013904223u; return (float)(rs >> 8) / 16777216.f; };
    for (int i = 0; i < n; ++i) {
        const float z = 2.f + 8.f * rnd(), x = (rnd() - 0.5f) * z, y = (rnd() - 0.5f) * 0.6f * z;
        X[3 * i] = x; X[3 * i + 1] = y; X[3 * i + 2] = z;
        const int oct = z < 3.f ? 2 : z < 5.f ? 4 : 6;
        c.a.ux[i] = c.a.kx[i] = 420.f * x / z + 376.f; c.a.uy[i] = c.a.ky[i] = 420.f * y / z + 240.f; c.a.octave[i] = oct;
        for (int p = 0; p < P; ++p) {
            const size_t o = (size_t)p * n + (n - 1 - i);                     // the neighbours hold the points in reverse order
            c.b.ux[o] = c.b.kx[o] = 420.f * (x - bx[p]) / z + 376.f; c.b.uy[o] = c.b.ky[o] = 420.f * y / z + 240.f; c.b.octave[o] = oct;
            if (i % (p + 2) == 0) c.m12[(size_t)p * n + i] = n - 1 - i;      // pair 1: every third point, pair 2: every fourth (twelfths in both)
        }
    }
    MockScene sc(c);
    MockMatcher mm(c, sc, h);
    struct Got { int idx1, idx2, kf; float x[3]; };
    std::vector<Got> got;
    const int nNew = CreateNewMapPoints(mm, &sc.cur, sc.neigh, false, true, false, 0.f, [&](const cv::Matx31f& x3D, MockKeyFrame* k2, int i1, int i2) {
        got.push_back(Got{i1, i2, (int)(k2 - &sc.store[0]), {x3D(0, 0), x3D(1, 0), x3D(2, 0)}});
    });
    int bad = 0, want = 0;
    for (int i = 0; i < n; ++i) want += (i % 3 == 0) || (i % 4 == 0);
    if (nNew != (int)got.size() || nNew != want) { printf("created %d, callback %zu, want %d\n", nNew, got.size(), want); ++bad; }
    if (mm.searches != 2 || mm.lastCoarse != 1) { printf("searches %d coarse %d\n", mm.searches, mm.lastCoarse); ++bad; }
    for (size_t j = 0; j < got.size(); ++j) {
        const Got& g = got[j];
        const int wantKf = g.idx1 % 3 == 0 ? 1 : 2;                          // pair 1 (neighbour 1) comes first and keeps the twelfths
        if (g.kf != wantKf || g.idx2 != n - 1 - g.idx1) { ++bad; continue; }
        if (j > 0 && (got[j - 1].kf > g.kf || (got[j - 1].kf == g.kf && got[j - 1].idx1 >= g.idx1))) ++bad;      // pair by pair, ascending idx1
        for (int k = 0; k < 3; ++k) if (std::fabs(g.x[k] - X[3 * g.idx1 + k]) > 2e-3f * X[3 * g.idx1 + 2]) ++bad;
    }
    orbm_destroy(h);
    if (bad) { printf("facade_triangulate_smoke FAILED (%d)\n", bad); return 1; }
    printf("facade_triangulate_smoke ok: %d new points from 2 of 3 neighbours\n", nNew);
    return 0;
}
