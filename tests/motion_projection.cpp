// Evaluates the pose and projection expressions of the facade's M4 (orb-slam3_amd/facade/ORBmatcher.h, SearchByProjection(CurrentFrame,
// LastFrame, th, bMono): ORBmatcher.cc:2481-2527) on cv::Mat from facade/cvcompat.h, for the cases in argv[1]; writes per case
// (valid, u, v, invzc, dir) as five float32 to argv[2].  tests/test_motion_projection_cpu.py compares them with its numpy restatement,
// which tests/test_gpu_motion_model_batch.py uses as the reference of orbm_project_last_frame_batch_async.
// Input (float32): fx fy cx cy  minX maxX minY maxY  mb mono  n, then per case Tcw_cur[12] Tcw_last[12] (row-major 3x4) x3Dw[3].
#include <cstdio>
#include <vector>
#include "../orb-slam3_amd/facade/cvcompat.h"

struct Pinhole {                                                // CameraModels/Pinhole.cpp:33-37
    float fx, fy, cx, cy;
    cv::Point2f project(const cv::Point3f& p) const { return cv::Point2f(fx * p.x / p.z + cx, fy * p.y / p.z + cy); }
    cv::Point2f project(const cv::Mat& m) const { return project(cv::Point3f(m.at<float>(0), m.at<float>(1), m.at<float>(2))); }
};

static cv::Mat tcw44(const float* t) {
    cv::Mat m = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m.at<float>(r, c) = t[r * 4 + c];
    return m;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    float hdr[11];
    if (std::fread(hdr, sizeof(float), 11, fi) != 11) return 2;
    const Pinhole cam{hdr[0], hdr[1], hdr[2], hdr[3]};
    const float mnMinX = hdr[4], mnMaxX = hdr[5], mnMinY = hdr[6], mnMaxY = hdr[7], mb = hdr[8];
    const bool bMono = hdr[9] != 0;
    const int n = (int)hdr[10];
    std::vector<float> in((size_t)n * 27), out((size_t)n * 5, 0.f);
    if (std::fread(in.data(), sizeof(float), in.size(), fi) != in.size()) return 2;
    std::fclose(fi);
    for (int i = 0; i < n; ++i) {
        const float* c = &in[(size_t)i * 27];
        const cv::Mat CurTcw = tcw44(c), LastTcw = tcw44(c + 12);
        cv::Mat x3Dw(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) x3Dw.at<float>(r) = c[24 + r];
        // the facade's lines, verbatim but for the frame members
        const cv::Mat Rcw = CurTcw.rowRange(0, 3).colRange(0, 3), tcw = CurTcw.rowRange(0, 3).col(3);
        const cv::Mat twc = -Rcw.t() * tcw;
        const cv::Mat Rlw = LastTcw.rowRange(0, 3).colRange(0, 3), tlw = LastTcw.rowRange(0, 3).col(3);
        const cv::Mat tlc = Rlw * twc + tlw;
        const bool bForward = tlc.at<float>(2) > mb && !bMono;
        const bool bBackward = -tlc.at<float>(2) > mb && !bMono;
        float* o = &out[(size_t)i * 5];
        o[4] = bForward ? 1.f : bBackward ? 2.f : 0.f;
        cv::Mat x3Dc = Rcw * x3Dw + tcw;
        const float invzc = 1.0 / x3Dc.at<float>(2);
        if (invzc < 0) continue;
        cv::Point2f uv = cam.project(x3Dc);
        if (uv.x < mnMinX || uv.x > mnMaxX) continue;
        if (uv.y < mnMinY || uv.y > mnMaxY) continue;
        o[0] = 1.f; o[1] = uv.x; o[2] = uv.y; o[3] = invzc;
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(float), out.size(), fo) != out.size()) return 2;
    std::fclose(fo);
    std::printf("motion_projection ok: %d cases\n", n);
    return 0;
}
