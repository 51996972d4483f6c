// The text form of a pose-optimisation case (tests/poseopt_io.py: write_cases) and the host run of csrc/orbm_poseopt.h on it, shared by
// tests/poseopt_header.cpp, tests/poseopt_facade.cpp and tests/facade_poseopt_smoke.cpp.
#pragma once
#include <cstdio>
#include <string>
#include <vector>
#include "../orb-slam3_amd/csrc/orbm_poseopt.h"

struct Case {
    std::string name;
    int n = 0, nlevels = 0, haveUright = 0;
    float k[4], bf, tcw[12];
    std::vector<float> ils2, x, y, ur, pw;
    std::vector<int> octave, has;
};

static bool read_case(FILE* f, Case& c) {
    char name[128];
    if (fscanf(f, "%127s %d %d %d", name, &c.n, &c.nlevels, &c.haveUright) != 4) return false;
    c.name = name;
    if (c.n < 0 || c.nlevels < 0 || c.n > (1 << 24) || c.nlevels > (1 << 16)) return false;
    for (int i = 0; i < 4; ++i) if (fscanf(f, "%f", &c.k[i]) != 1) return false;
    if (fscanf(f, "%f", &c.bf) != 1) return false;
    c.ils2.resize(c.nlevels);
    for (int i = 0; i < c.nlevels; ++i) if (fscanf(f, "%f", &c.ils2[i]) != 1) return false;
    for (int i = 0; i < 12; ++i) if (fscanf(f, "%f", &c.tcw[i]) != 1) return false;
    c.x.resize(c.n); c.y.resize(c.n); c.ur.resize(c.n); c.pw.resize(3 * (size_t)c.n); c.octave.resize(c.n); c.has.resize(c.n);
    for (int i = 0; i < c.n; ++i)
        if (fscanf(f, "%f %f %d %f %d %f %f %f", &c.x[i], &c.y[i], &c.octave[i], &c.ur[i], &c.has[i], &c.pw[3 * i], &c.pw[3 * i + 1], &c.pw[3 * i + 2]) != 8)
            return false;
    return true;
}

struct Result { int nCorr, nGood; double T[12]; float tcw[12]; std::vector<unsigned char> state; };

static void run(const Case& c, Result& r) {
    std::vector<PoEdge> edges(c.n);
    r.state.assign(c.n, PO_NONE);
    r.nCorr = 0;
    for (int i = 0; i < c.n; ++i)
        if (c.has[i] && po_make_edge(c.x[i], c.y[i], c.octave[i], c.haveUright ? &c.ur[i] : nullptr, &c.pw[3 * (size_t)i], c.ils2.data(), c.nlevels, edges[i])) {
            r.state[i] = PO_INLIER;
            ++r.nCorr;
        }
    for (int i = 0; i < 12; ++i) { r.T[i] = (double)c.tcw[i]; r.tcw[i] = c.tcw[i]; }
    r.nGood = 0;
    if (r.nCorr < 3) return;
    PoCpuReduce ctx{PoCam{(double)c.k[0], (double)c.k[1], (double)c.k[2], (double)c.k[3], (double)c.bf}, c.n, edges.data(), r.state.data()};
    double T0[12];
    po_pose_from_float(c.tcw, T0);
    r.nGood = po_four_rounds(ctx, r.nCorr, T0, r.T);
    for (int i = 0; i < 12; ++i) r.tcw[i] = (float)r.T[i];
}

