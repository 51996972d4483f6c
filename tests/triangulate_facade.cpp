// triangulate_facade.cpp -- facade/CreateNewMapPoints.h on mock KeyFrames (tests/triangulate_mock.h), g++ on cvcompat.h, no GPU:
// `triangulate_facade <case> <out>` builds the KeyFrames of a one-group case, runs newpoints::Flat::build and the match collection and
// writes the flattened arrays in the case's own binary form, so that the test can compare them byte for byte with the case it wrote.
// It also prints the baseline / median-depth decisions, F12 of every passing pair and the refusals.
#include <cstdio>
#include <stdexcept>
#include "../orb-slam3_amd/facade/CreateNewMapPoints.h"
#include "triangulate_mock.h"

using namespace ORB_SLAM3;

static void split(const std::vector<orbm_kp_t>& k, std::vector<float>& x, std::vector<float>& y, std::vector<int32_t>* oct) {
    x.clear(); y.clear(); if (oct) oct->clear();
    for (const auto& p : k) { x.push_back(p.x); y.push_back(p.y); if (oct) oct->push_back(p.octave); }
}
static void write_pool(FILE* f, const std::vector<orbm_kp_t>& un, const std::vector<orbm_kp_t>& raw, const std::vector<int32_t>& counts, const std::vector<float>& ur,
                       const std::vector<float>& dp, const std::vector<float>& tcw, const std::vector<float>& ow) {
    std::vector<float> x, y; std::vector<int32_t> oct;
    split(un, x, y, &oct); wr(f, x); wr(f, y); wr(f, oct);
    split(raw, x, y, nullptr); wr(f, x); wr(f, y);
    wr(f, counts); wr(f, ur); wr(f, dp); wr(f, tcw); wr(f, ow);
}
template <class Fn> static bool refused(Fn fn) { try { fn(); } catch (const std::runtime_error&) { return true; } return false; }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: triangulate_facade <case> <out>\n"); return 2; }
    TriCase c;
    if (!read_case(argv[1], c) || c.ng != 1 || c.npairs < 1) { fprintf(stderr, "need a one-group case\n"); return 2; }
    MockScene s(c);
    MockMatcher mm(c, s, nullptr);
    newpoints::Flat A;
    A.build(&s.cur, s.neigh, false);
    for (int p = 0; p < A.npairs; ++p) {
        std::vector<std::pair<size_t, size_t>> pairs;
        mm.SearchForTriangulation_(&s.cur, s.neigh[A.neigh[p]], A.F12[p], pairs, false, true);
        A.set_matches(p, pairs);
    }
    printf("pairs %d of %d cap1 %d cap2 %d searches %d\n", A.npairs, c.npairs, A.cap1, A.cap2, mm.searches);
    for (int p = 0; p < A.npairs; ++p) {
        printf("F12 %d", A.neigh[p]);
        for (int i = 0; i < 9; ++i) printf(" %a", (double)A.F12[p].val[i]);
        printf("\n");
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 2;
    const int32_t h[8] = {1, A.npairs, 1, A.cap1, A.npairs, A.cap2, A.nlevels, 0};
    fwrite(h, sizeof(int32_t), 8, f);
    const std::vector<int32_t> gs = {0, A.npairs};
    wr(f, gs); wr(f, A.row1); wr(f, A.row2); wr(f, A.matches12);
    write_pool(f, A.kpsUn1, A.kps1, A.counts1, A.uright1, A.depth1, A.tcw1, A.ow1);
    write_pool(f, A.kpsUn2, A.kps2, A.counts2, A.uright2, A.depth2, A.tcw2, A.ow2);
    std::vector<float> fl(A.k, A.k + 6); fl.insert(fl.end(), A.k, A.k + 6);
    fl.push_back(A.mb); fl.push_back(A.mbf); fl.push_back(A.mb); fl.push_back(A.ratioFactor); fl.push_back(c.fl[16]);
    wr(f, fl); wr(f, A.sf); wr(f, A.ls); wr(f, A.sf); wr(f, A.ls);
    fclose(f);
    // the baseline tests: a neighbour closer than mb (stereo) or with baseline / median depth < 0.01 (monocular) is not passed
    {
        MockScene t(c);
        for (int i = 0; i < 3; ++i) t.store[0].O[i] = t.cur.O[i];
        t.store[0].O[0] += 0.5f * t.cur.mb;
        newpoints::Flat B; B.build(&t.cur, t.neigh, false);
        printf("check short_baseline_is_skipped %d\n", B.npairs == c.npairs - 1 && (B.npairs == 0 || B.neigh[0] == 1));
        newpoints::Flat M; M.build(&t.cur, t.neigh, true);
        printf("check monocular_uses_the_median_depth %d\n", M.npairs == c.npairs);           // 0.5 mb / 5 m = 0.011 >= 0.01
        t.store[0].medianDepth = 50.f;
        newpoints::Flat M2; M2.build(&t.cur, t.neigh, true);
        printf("check monocular_ratio_below_0.01_is_skipped %d\n", M2.npairs == c.npairs - 1);
    }
    {
        MockScene t(c); int dummy = 0;
        t.store[c.npairs - 1].mpCamera2 = &dummy;
        printf("check second_camera_of_a_neighbour_is_refused %d\n", refused([&] { newpoints::Flat B; B.build(&t.cur, t.neigh, false); }));
        MockScene u(c); u.cur.mpCamera2 = &dummy;
        printf("check second_camera_is_refused %d\n", refused([&] { newpoints::Flat B; B.build(&u.cur, u.neigh, false); }));
        MockScene v(c); v.cur.NLeft = 10;
        printf("check nleft_is_refused %d\n", refused([&] { newpoints::Flat B; B.build(&v.cur, v.neigh, false); }));
        MockScene w(c); w.store[0].cam.mnType = 1;
        printf("check fisheye_is_refused %d\n", refused([&] { newpoints::Flat B; B.build(&w.cur, w.neigh, false); }));
        MockScene x(c); x.store[0].fx += 1.f;
        printf("check another_camera_is_refused %d\n", refused([&] { newpoints::Flat B; B.build(&x.cur, x.neigh, false); }));
    }
    return 0;
}
