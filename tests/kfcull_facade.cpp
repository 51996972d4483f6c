// facade/KeyFrameCulling.h's flatten (kfcull::Flat) on the mock types of tests/kfcull_mock.h: reads a map in text form, applies the
// skips of :1272 and the chunk rule of the facade's loop, and prints every array of the library call, floats as their 32 bits.
// tests/test_kfcull_facade_cpu.py compares them with the flatten of tests/second_reading_kfcull.py.  No GPU, no library.
//   kfcull_facade MAPFILE monocular(0|1)
#include <cstdio>
#include <cstdlib>
#include "kfcull_mock.h"

template <class T> static void put(const char* name, const std::vector<T>& v) {
    std::printf("%s %zu", name, v.size());
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "r");
    MockMap M;
    if (!f || !LoadMockMap(f, M)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
    const bool bMonocular = std::atoi(argv[2]) != 0;
    std::vector<KeyFrame*> cands;
    int count = 0;
    for (KeyFrame* pKF : M.covisible) {
        count++;
        if ((pKF->mnId == pKF->GetMap()->GetInitKFid()) || pKF->isBad()) continue;
        cands.push_back(pKF);
        if (count > 100) break;
    }
    ORB_SLAM3::kfcull::Flat<KeyFrame> F;
    F.build(cands, bMonocular);
    std::printf("cap 1 %d\nth_depth 1 %u\n", F.cap, float_bits(F.thDepth));
    put("cand_row", F.candRow); put("counts_kf", F.counts); put("kf_mp", F.kfMp);
    std::vector<int> oct; for (const orbm_kp_t& k : F.kps) oct.push_back(k.octave);
    put("octave", oct);
    std::vector<uint32_t> d; for (float v : F.depth) d.push_back(float_bits(v));
    put("depth", d);
    put("obs_off", F.off); put("obs_row", F.row); put("obs_slot", F.slot); put("obs_flags", F.flags); put("mp_valid", F.valid); put("mp_nobs", F.mpNobs);
    std::vector<long long> rows; for (KeyFrame* p : F.rows) rows.push_back(p - &M.kfs[0]);
    put("rows", rows);
    return 0;
}
