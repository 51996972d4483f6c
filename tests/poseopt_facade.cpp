// facade/PoseOptimization.h compiled with plain g++ against cvcompat.h on the mock types of tests/poseopt_mock.h, with no library: this
// file supplies orbm_pose_optimization as the host run of csrc/orbm_poseopt.h and records the arrays the facade hands over.  For every
// case of the input file it prints the flattened arrays (floats as bit patterns) and what the facade left in the frame; with a second
// argument it gives the first case's frame a second camera and prints whether the facade refused it.
#include <cstdint>
#include <cstring>
#include "poseopt_mock.h"
#include "../orb-slam3_amd/facade/PoseOptimization.h"

struct Seen {
    int calls = 0, nframes, first, cap, nmp, nlevels, count;
    bool haveUright;
    std::vector<orbm_kp_t> kps;
    std::vector<float> uright, pw, ils2, tcw, k;
    std::vector<int32_t> qMp;
    float bf;
};
static Seen g;

extern "C" const char* orbm_last_error(void) { return "stub"; }
extern "C" int orbm_pose_optimization(orbm_t*, int nframes, int first, int cap, const orbm_kp_t* kps_un, const int32_t* counts, const float* uright,
                                      const int32_t* q_mp, int nmp, const float* mp_pw, const float* tcw_in, const float* k_host, float bf,
                                      const float* ils2, int nlevels, float* tcw_out, uint8_t* outlier, int32_t* n_corr, int32_t* n_good) {
    ++g.calls;
    g.nframes = nframes; g.first = first; g.cap = cap; g.nmp = nmp; g.nlevels = nlevels; g.count = counts[0]; g.haveUright = uright != nullptr; g.bf = bf;
    g.kps.assign(kps_un, kps_un + cap); g.qMp.assign(q_mp, q_mp + cap); g.pw.assign(mp_pw, mp_pw + 3 * (size_t)nmp);
    g.uright.assign(cap, -1.f);
    if (uright) g.uright.assign(uright, uright + cap);
    g.ils2.assign(ils2, ils2 + nlevels); g.tcw.assign(tcw_in, tcw_in + 12); g.k.assign(k_host, k_host + 4);
    Case c;                                                                  // the contract, through the same host run as tests/poseopt_header.cpp
    c.n = counts[0]; c.nlevels = nlevels; c.haveUright = uright != nullptr; c.bf = bf;
    for (int i = 0; i < 4; ++i) c.k[i] = k_host[i];
    for (int i = 0; i < 12; ++i) c.tcw[i] = tcw_in[i];
    c.ils2 = g.ils2;
    c.x.resize(c.n); c.y.resize(c.n); c.ur.resize(c.n); c.pw.assign(3 * (size_t)c.n, 0.f); c.octave.resize(c.n); c.has.resize(c.n);
    for (int i = 0; i < c.n; ++i) {
        const orbm_kp_t& kp = kps_un[i];
        c.x[i] = kp.x; c.y[i] = kp.y; c.octave[i] = kp.octave; c.ur[i] = uright ? uright[i] : -1.f;
        c.has[i] = q_mp[i] >= 0 && q_mp[i] < nmp;
        if (c.has[i]) for (int t = 0; t < 3; ++t) c.pw[3 * (size_t)i + t] = mp_pw[3 * (size_t)q_mp[i] + t];
    }
    Result r;
    run(c, r);
    for (int i = 0; i < c.n; ++i) if (r.state[i] != PO_NONE) outlier[i] = r.state[i] == PO_OUTLIER;
    for (int i = 0; i < 12; ++i) tcw_out[i] = r.tcw[i];
    *n_corr = r.nCorr; *n_good = r.nGood;
    return ORBM_OK;
}

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
template <class V, class F> static void line(const char* name, const V& v, F f) {
    std::printf("%s %zu", name, v.size());
    for (const auto& x : v) std::printf(" %lld", (long long)f(x));
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    Case c;
    int ncases = 0;
    while (read_case(f, c)) {
        Frame F; std::vector<MapPoint> pool;
        frame_from_case(c, F, pool);
        if (argc > 2) {
            static const int camera2 = 0;
            F.mpCamera2 = &camera2;
            bool refused = false;
            try { ORB_SLAM3::PoseOptimization((orbm_t*)nullptr, &F); } catch (const std::runtime_error&) { refused = true; }
            std::printf("refused 1 %d\ncalls 1 %d\n", refused ? 1 : 0, g.calls);
            return 0;
        }
        g = Seen();
        const int ret = ORB_SLAM3::PoseOptimization((orbm_t*)nullptr, &F);
        auto id = [](long long v) { return v; };
        std::printf("case %s\n", c.name.c_str());
        line("shape", std::vector<int>{g.calls, g.nframes, g.first, g.cap, g.nmp, g.nlevels, g.count, g.haveUright ? 1 : 0, ret, F.nSetPose}, id);
        line("x", g.kps, [](const orbm_kp_t& k) { return bits(k.x); });
        line("y", g.kps, [](const orbm_kp_t& k) { return bits(k.y); });
        line("octave", g.kps, [](const orbm_kp_t& k) { return k.octave; });
        line("uright", g.uright, bits); line("q_mp", g.qMp, id); line("pw", g.pw, bits); line("ils2", g.ils2, bits); line("tcw", g.tcw, bits);
        line("k", g.k, bits); line("bf", std::vector<float>{g.bf}, bits);
        std::vector<int> out(F.mvbOutlier.begin(), F.mvbOutlier.end());
        line("outlier", out, id);
        std::vector<float> pose;
        for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) pose.push_back(F.mTcw.at<float>(r, k));
        line("pose", pose, bits);
        ++ncases;
    }
    return ncases ? 0 : 1;
}
