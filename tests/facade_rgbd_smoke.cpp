// Drives the two RGB-D helpers of facade/FrameGeometry.h (ComputeStereoFromRGBD, UnprojectStereoAll) on mock vectors and compares
// them, bit for bit, with the reference's lines (Frame.cc:1279-1326, Tracking.cc:1353-1354) evaluated in plain C++ in this file.
// Build with -ffp-contract=off.  Without a GPU it only proves that the helpers compile and link (exit 0; exit 1 with an argument).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../orb-slam3_amd/facade/FrameGeometry.h"
#include "../include/orbx.h"

#define CHECK(cond, code) do { if (!(cond)) { std::printf("facade_rgbd_smoke: check failed at line %d: %s\n", __LINE__, #cond); return code; } } while (0)

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

template <class T>
static void expect_rgbd(const std::vector<cv::KeyPoint>& keys, const std::vector<cv::KeyPoint>& un, const T* img, int w, int h, int strideElems,
                        bool isF32, float factor, float bf, std::vector<float>& ur, std::vector<float>& dp, int& cnt) {
    const bool convert = (std::fabs(factor - 1.0f) > 1e-5) || !isF32;                  // Tracking.cc:1353
    ur.assign(keys.size(), -1.f); dp.assign(keys.size(), -1.f); cnt = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        const float v = keys[i].pt.y, u = keys[i].pt.x;
        if (!(u > -1.f && u < (float)w && v > -1.f && v < (float)h)) continue;         // outside the image: the contract's -1 / -1
        const T raw = img[(size_t)(int)v * strideElems + (int)u];
        const float d = convert ? (float)raw * factor : (float)raw;
        if (d > 0) { dp[i] = d; ur[i] = un[i].pt.x - bf / d; ++cnt; }                  // Frame.cc:1303-1307
    }
}

int main(int argc, char** argv) {
    const int w = 97, h = 61, pad = 5, n = 300;
    unsigned s = 2024;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    std::vector<uint16_t> img16((size_t)h * (w + pad));
    std::vector<float> img32((size_t)h * (w + pad));
    for (size_t i = 0; i < img16.size(); ++i) {
        const unsigned r = rnd();
        img16[i] = (r % 5 == 0) ? 0 : (uint16_t)(r & 0xFFFF);
        img32[i] = (r % 5 == 0) ? 0.f : (r % 7 == 0) ? -1.5f : 0.25f + (float)(r & 0xFFF) / 512.f;
    }
    img16[0] = 65535; img32[1] = std::numeric_limits<float>::infinity(); img32[2] = std::numeric_limits<float>::quiet_NaN();
    std::vector<cv::KeyPoint> keys(n), un(n);
    for (int i = 0; i < n; ++i) {
        keys[i].pt.x = (float)(rnd() % (unsigned)(w * 100)) / 100.f; keys[i].pt.y = (float)(rnd() % (unsigned)(h * 100)) / 100.f;
        un[i] = keys[i]; un[i].pt.x += 0.375f; un[i].pt.y -= 0.125f;
    }
    keys[0].pt = cv::Point2f(0.f, 0.f); keys[1].pt = cv::Point2f(1.f, 0.f); keys[2].pt = cv::Point2f(2.f, 0.f);
    keys[3].pt = cv::Point2f((float)w - 0.01f, (float)h - 0.01f); keys[4].pt = cv::Point2f((float)w, 3.f); keys[5].pt = cv::Point2f(3.f, -1.f);
    if (orbx_device_count() < 1) { std::printf("facade RGB-D helpers compiled; no GPU here\n"); return argc > 1 ? 1 : 0; }
    orbm_t* m = nullptr;
    CHECK(orbm_create(&m, 0) == ORBM_OK, 2);
    const float bf = 40.f;
    std::vector<float> ur, dp, eur, edp; int ecnt = 0;
    // U16 at the TUM factor, padded rows
    const float tum = 1.0f / 5000.f;
    int got = ORB_SLAM3::ComputeStereoFromRGBD(m, keys, un, img16.data(), ORBM_DEPTH_U16, w, h, (size_t)(w + pad) * 2, tum, bf, ur, dp);
    expect_rgbd(keys, un, img16.data(), w, h, w + pad, false, tum, bf, eur, edp, ecnt);
    CHECK(got == ecnt && ecnt > n / 2 && ecnt < n, 3);
    for (int i = 0; i < n; ++i) CHECK(same(ur[i], eur[i]) && same(dp[i], edp[i]), 4);
    CHECK(dp[0] == 65535.f * tum && dp[4] == -1.f && dp[5] == -1.f && ur[4] == -1.f, 5);
    // F32 passed through (factor 1) and scaled (factor 0.5)
    for (float factor : {1.0f, 0.5f}) {
        got = ORB_SLAM3::ComputeStereoFromRGBD(m, keys, un, img32.data(), ORBM_DEPTH_F32, w, h, (size_t)(w + pad) * 4, factor, bf, ur, dp);
        expect_rgbd(keys, un, img32.data(), w, h, w + pad, true, factor, bf, eur, edp, ecnt);
        CHECK(got == ecnt && ecnt > n / 3, 6);
        for (int i = 0; i < n; ++i) CHECK(same(ur[i], eur[i]) && same(dp[i], edp[i]), 7);
        CHECK(std::isinf(dp[1]) && same(ur[1], un[1].pt.x) && dp[2] == -1.f, 8);
    }
    // an unknown depth type is refused by the library and surfaces as an exception
    bool threw = false;
    std::vector<float> ur2, dp2;
    try { ORB_SLAM3::ComputeStereoFromRGBD(m, keys, un, img32.data(), 7, w, h, (size_t)(w + pad) * 4, 1.f, bf, ur2, dp2); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw, 9);
    // UnprojectStereoAll against Frame.cc:1314-1322 under the cv::Mat product rule of cvcompat.h
    const float K[4] = {517.3f, 516.5f, 318.6f, 255.3f};
    const float c = std::cos(0.3f), sn = std::sin(0.3f);
    const float Rwc[9] = {c, 0.f, sn, 0.f, 1.f, 0.f, -sn, 0.f, c}, Ow[3] = {0.5f, -0.25f, 2.f};
    std::vector<float> x3; std::vector<uint8_t> has;
    dp[1] = -1.f;                                                                      // an infinite depth unprojects to NaNs, whose bits are not pinned
    const int np = ORB_SLAM3::UnprojectStereoAll(m, un, dp, Rwc, Ow, K, x3, has);
    const float invfx = 1.0f / K[0], invfy = 1.0f / K[1];
    cv::Mat R(3, 3, CV_32F), O(3, 1, CV_32F);
    for (int i = 0; i < 9; ++i) R.at<float>(i / 3, i % 3) = Rwc[i];
    for (int i = 0; i < 3; ++i) O.at<float>(i) = Ow[i];
    int want = 0;
    for (int i = 0; i < n; ++i) {
        const float z = dp[i];
        if (z > 0) {
            cv::Mat x3Dc(3, 1, CV_32F);
            x3Dc.at<float>(0) = (un[i].pt.x - K[2]) * z * invfx; x3Dc.at<float>(1) = (un[i].pt.y - K[3]) * z * invfy; x3Dc.at<float>(2) = z;
            const cv::Mat x3Dw = R * x3Dc + O;
            ++want;
            CHECK(has[i] == 1, 10);
            for (int r = 0; r < 3; ++r) CHECK(same(x3[3 * i + r], x3Dw.at<float>(r)), 11);
        } else {
            CHECK(has[i] == 0 && x3[3 * i] == 0.f && x3[3 * i + 1] == 0.f && x3[3 * i + 2] == 0.f, 12);
        }
    }
    CHECK(np == want && want > n / 3, 13);
    // empty frames come back empty without a call
    std::vector<cv::KeyPoint> none;
    CHECK(ORB_SLAM3::ComputeStereoFromRGBD(m, none, none, img16.data(), ORBM_DEPTH_U16, w, h, (size_t)(w + pad) * 2, tum, bf, ur, dp) == 0 && ur.empty(), 14);
    CHECK(ORB_SLAM3::UnprojectStereoAll(m, none, dp, Rwc, Ow, K, x3, has) == 0 && x3.empty() && has.empty(), 15);
    orbm_destroy(m);
    std::printf("facade_rgbd_smoke ok: %d depth points of %d keypoints unprojected\n", want, n);
    return 0;
}
