// triangulate_header.cpp -- orb-slam3_amd/csrc/orbm_triangulate.h built with g++ (-ffp-contract=off) as a stand-alone program: reads a case
// in the binary form tests/triangulate_io.py writes, walks every group the way k_triangulate_new / k_triangulate_order do (per idx1 the
// pairs in order, the first success wins; then pair by pair, ascending idx1) and writes every output plus the unit x3D_h of each
// triangulated match.  `triangulate_header <case> <out> [reps]`: with reps the walk is repeated and its time printed (the host leg of
// tools/triangulate_new_points_batch.py).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../orb-slam3_amd/csrc/orbm_triangulate.h"
#include "triangulate_case_io.h"

static TriPose pose_of(const Pool& p, int row) {
    TriPose P;
    memcpy(P.T, &p.tcw[12 * (size_t)row], sizeof P.T); memcpy(P.ow, &p.ow[3 * (size_t)row], sizeof P.ow);
    return P;
}
static TriObs obs_of(const Pool& p, int row, int i) {
    const size_t s = (size_t)row * p.cap + i;
    return TriObs{p.ux[s], p.uy[s], p.kx[s], p.ky[s], p.octave[s], p.uright[s], p.depth[s]};
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: triangulate_header <case> <out> [reps]\n"); return 2; }
    TriCase c;
    if (!read_case(argv[1], c)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int ng = c.ng, npairs = c.npairs, nl = c.nl, cap1 = c.a.cap;
    const Pool &a = c.a, &b = c.b;
    const std::vector<int32_t>&gs = c.gs, &row1 = c.row1, &row2 = c.row2, &m12 = c.m12;
    const std::vector<float>&fl = c.fl, &sf1 = c.sf1, &ls1 = c.ls1, &sf2 = c.sf2, &ls2 = c.ls2;
    const TriCam K1{fl[0], fl[1], fl[2], fl[3], fl[4], fl[5]}, K2{fl[6], fl[7], fl[8], fl[9], fl[10], fl[11]};
    const float mb1 = fl[12], mbf1 = fl[13], mb2 = fl[14], rf = fl[15], thFar = fl[16];
    const int reps = argc > 3 ? atoi(argv[3]) : 1;
    const size_t so = (size_t)ng * cap1, sp = (size_t)npairs * cap1;
    std::vector<int32_t> wonPair, wonIdx2, ncreated, order, ntotal, reason;
    std::vector<float> x3d, xh;
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < (reps > 0 ? reps : 1); ++rep) {
        wonPair.assign(so, -1); wonIdx2.assign(so, -1); x3d.assign(3 * so, 0.f); reason.assign(sp, TRI_NO_MATCH); ncreated.assign(npairs, 0);
        order.assign(so, -1); ntotal.assign(ng, 0); xh.assign(4 * sp, 0.f);
        for (int g = 0; g < ng; ++g) {
            const int p0 = gs[g], p1 = gs[g + 1];
            if (p0 < 0 || p1 > npairs || p1 <= p0) continue;
            const int r1 = row1[p0];
            bool mixed = false;
            for (int p = p0 + 1; p < p1; ++p) mixed = mixed || row1[p] != r1;
            if (mixed) { for (size_t i = (size_t)p0 * cap1; i < (size_t)p1 * cap1; ++i) reason[i] = TRI_MIXED_ROW1; continue; }
            if (r1 < 0 || r1 >= a.rows) continue;
            int n1 = a.counts[r1]; n1 = n1 < 0 ? 0 : n1 > cap1 ? cap1 : n1;
            const TriPose P1 = pose_of(a, r1);
            for (int i1 = 0; i1 < n1; ++i1) {                                  // the lane's walk over the pairs
                const TriObs o1 = obs_of(a, r1, i1);
                int won = -1;
                for (int p = p0; p < p1; ++p) {
                    const int r2 = row2[p];
                    if (r2 < 0 || r2 >= b.rows) continue;
                    int n2 = b.counts[r2]; n2 = n2 < 0 ? 0 : n2 > b.cap ? b.cap : n2;
                    const int i2 = m12[(size_t)p * cap1 + i1];
                    if (i2 < 0 || i2 >= n2) continue;
                    if (won >= 0) { reason[(size_t)p * cap1 + i1] = TRI_TAKEN; continue; }
                    float x[3];
                    const int r = tri_one_match(K1, K2, mb1, mbf1, mb2, P1, pose_of(b, r2), o1, obs_of(b, r2, i2), sf1.data(), ls1.data(), sf2.data(),
                                                ls2.data(), nl, rf, thFar, x, &xh[4 * ((size_t)p * cap1 + i1)]);
                    reason[(size_t)p * cap1 + i1] = r;
                    if (tri_ok(r)) {
                        won = p;
                        const size_t o = (size_t)g * cap1 + i1;
                        wonPair[o] = p; wonIdx2[o] = i2; x3d[3 * o] = x[0]; x3d[3 * o + 1] = x[1]; x3d[3 * o + 2] = x[2];
                    }
                }
            }
            for (int p = p0; p < p1; ++p)                                      // the creation order: pair by pair, ascending idx1
                for (int i1 = 0; i1 < cap1; ++i1)
                    if (wonPair[(size_t)g * cap1 + i1] == p) { order[(size_t)g * cap1 + ntotal[g]++] = i1; ++ncreated[p]; }
        }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (reps > 1) printf("time_ms %.6f\n", ms / reps);
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    wr(o, wonPair); wr(o, wonIdx2); wr(o, x3d); wr(o, reason); wr(o, ncreated); wr(o, order); wr(o, ntotal); wr(o, xh);
    fclose(o);
    return 0;
}
