// Evaluates facade/MapPointRefresh.h's statement of UpdateNormalAndDepth (NormalAndDepthOnMat: MapPoint.cc:601-649 on cv::Mat)
// against facade/cvcompat.h, for the cases in argv[1]; writes per case (normal[3], min_dist, max_dist) as five float32 to argv[2].
// tests/test_mappoint_normal_cpu.py compares them bit for bit with tests/second_reading_mappoint.py, which tests/test_gpu_mappoint.py
// uses as the reference of orbm_update_normal_and_depth(_batch_async).  Build with -ffp-contract=off.
// Input (float32): nlevels n, scale[nlevels], then per case pos[3] ref_centre[3] level ncentres centres[MAXC][3].
#include <cstdio>
#include <vector>
#include "../orb-slam3_amd/facade/MapPointRefresh.h"

enum { MAXC = 8 };

static cv::Mat vec3(const float* p) {
    cv::Mat m(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) m.at<float>(r) = p[r];
    return m;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    float hdr[2];
    if (std::fread(hdr, sizeof(float), 2, fi) != 2) return 2;
    const int nLevels = (int)hdr[0], n = (int)hdr[1];
    std::vector<float> mvScaleFactors(nLevels);
    if (std::fread(mvScaleFactors.data(), sizeof(float), nLevels, fi) != (size_t)nLevels) return 2;
    const int stride = 8 + 3 * MAXC;
    std::vector<float> in((size_t)n * stride), out((size_t)n * 5, 0.f);
    if (std::fread(in.data(), sizeof(float), in.size(), fi) != in.size()) return 2;
    std::fclose(fi);
    for (int i = 0; i < n; ++i) {
        const float* c = &in[(size_t)i * stride];
        const cv::Mat mWorldPos = vec3(c), refCentre = vec3(c + 3);
        const int level = (int)c[6], ncent = (int)c[7];
        std::vector<cv::Mat> centres;                                       // one per n++ of the loop, in loop order
        for (int k = 0; k < ncent; ++k) centres.push_back(vec3(c + 8 + 3 * k));
        cv::Mat mNormalVector;
        float mfMinDistance = 0.f, mfMaxDistance = 0.f;
        ORB_SLAM3::NormalAndDepthOnMat(mWorldPos, centres, refCentre, level, mvScaleFactors, mNormalVector, mfMinDistance, mfMaxDistance);
        float* o = &out[(size_t)i * 5];
        for (int r = 0; r < 3; ++r) o[r] = mNormalVector.at<float>(r);
        o[3] = mfMinDistance; o[4] = mfMaxDistance;
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(float), out.size(), fo) != out.size()) return 2;
    std::fclose(fo);
    std::printf("mappoint_normal ok: %d cases\n", n);
    return 0;
}
