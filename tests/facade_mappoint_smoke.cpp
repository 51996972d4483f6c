// Drives facade/MapPointRefresh.h (ComputeDistinctiveDescriptors, UpdateNormalAndDepth, RefreshMapPoints) on mock MapPoint / KeyFrame
// types and compares the members it writes, bit for bit, with MapPoint.cc:450-538 and :578-652 restated in plain C++ in this file.
// Build with -ffp-contract=off.  Without a GPU it only proves that the templates compile and link (exit 0; exit 1 with an argument).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>
#include "../orb-slam3_amd/facade/MapPointRefresh.h"
#include "../include/orbx.h"

#define CHECK(cond, code) do { if (!(cond)) { std::printf("facade_mappoint_smoke: check failed at line %d: %s\n", __LINE__, #cond); return code; } } while (0)

struct KeyFrame {
    cv::Mat mDescriptors;
    int NLeft = -1;
    std::vector<cv::KeyPoint> mvKeysUn, mvKeys, mvKeysRight;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 8;
    float ow[3] = {0, 0, 0}, owr[3] = {0, 0, 0};
    bool bad = false;
    bool isBad() const { return bad; }
    cv::Mat centre(const float* p) const { cv::Mat m(3, 1, CV_32F); for (int i = 0; i < 3; ++i) m.at<float>(i) = p[i]; return m; }
    cv::Mat GetCameraCenter() const { return centre(ow); }
    cv::Mat GetRightCameraCenter() const { return centre(owr); }
};

struct MapPoint {
    std::map<KeyFrame*, std::tuple<int, int>> mObservations;
    KeyFrame* mpRefKF = nullptr;
    cv::Mat mWorldPos, mDescriptor, mNormalVector;
    float mfMinDistance = -1.f, mfMaxDistance = -1.f;
    bool mbBad = false;
    bool isBad() const { return mbBad; }
    std::map<KeyFrame*, std::tuple<int, int>> GetObservations() const { return mObservations; }
    KeyFrame* GetReferenceKeyFrame() const { return mpRefKF; }
    cv::Mat GetWorldPos() const { return mWorldPos.clone(); }
};

static int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// :450-538 -> the winning descriptor, or empty
static std::vector<uint8_t> expect_descriptor(const MapPoint& mp) {
    std::vector<const uint8_t*> v;
    if (mp.mbBad) return {};
    for (auto& o : mp.mObservations) {
        if (o.first->isBad()) continue;
        if (std::get<0>(o.second) != -1) v.push_back(o.first->mDescriptors.ptr(std::get<0>(o.second)));
        if (std::get<1>(o.second) != -1) v.push_back(o.first->mDescriptors.ptr(std::get<1>(o.second)));
    }
    if (v.empty()) return {};
    const size_t N = v.size();
    int bestMedian = 1 << 30; size_t bestIdx = 0;
    for (size_t i = 0; i < N; ++i) {
        std::vector<int> d(N);
        for (size_t j = 0; j < N; ++j) d[j] = i == j ? 0 : hamming(v[i], v[j]);
        std::sort(d.begin(), d.end());
        const int median = d[(size_t)(0.5 * (N - 1))];
        if (median < bestMedian) { bestMedian = median; bestIdx = i; }
    }
    return std::vector<uint8_t>(v[bestIdx], v[bestIdx] + 32);
}

static double norm3(const float d[3]) { return std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]); }

// :578-652 -> false when the reference returns early
static bool expect_normal(const MapPoint& mp, float normal[3], float& mn, float& mx) {
    if (mp.mbBad || mp.mObservations.empty()) return false;
    float p[3], acc[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < 3; ++i) p[i] = mp.mWorldPos.at<float>(i);
    int n = 0;
    auto add = [&](const float* ow) {
        float d[3] = {p[0] - ow[0], p[1] - ow[1], p[2] - ow[2]};
        const float s = (float)(1.0 / norm3(d));
        for (int i = 0; i < 3; ++i) { const float t = d[i] * s; acc[i] = acc[i] + t; }
        ++n;
    };
    for (auto& o : mp.mObservations) {
        if (std::get<0>(o.second) != -1) add(o.first->ow);
        if (std::get<1>(o.second) != -1) add(o.first->owr);
    }
    const KeyFrame* ref = mp.mpRefKF;
    float pc[3] = {p[0] - ref->ow[0], p[1] - ref->ow[1], p[2] - ref->ow[2]};
    const float dist = (float)norm3(pc);
    auto it = mp.mObservations.find(mp.mpRefKF);
    const int left = std::get<0>(it->second), right = std::get<1>(it->second);
    int level;
    if (ref->NLeft == -1) level = ref->mvKeysUn[left].octave;
    else if (left != -1) level = ref->mvKeys[left].octave;
    else level = ref->mvKeysRight[right - ref->NLeft].octave;
    mx = dist * ref->mvScaleFactors[level];
    mn = mx / ref->mvScaleFactors[ref->mnScaleLevels - 1];
    const float inv = (float)(1.0 / n);
    for (int i = 0; i < 3; ++i) normal[i] = acc[i] * inv;
    return true;
}

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main(int argc, char** argv) {
    unsigned s = 77;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    auto frnd = [&](float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xFFFF) / 65535.f; };
    const int nkf = 9, nmp = 120;
    std::vector<KeyFrame> kfs(nkf);
    for (int k = 0; k < nkf; ++k) {
        KeyFrame& kf = kfs[k];
        const bool two = k % 3 == 2;                                        // every third KeyFrame has two cameras: 40 left + 30 right rows
        const int nl = two ? 40 : 50 + 5 * k, nr = two ? 30 : 0;
        kf.NLeft = two ? nl : -1;
        kf.mDescriptors = cv::Mat(nl + nr, 32, CV_8U);
        for (int i = 0; i < nl + nr; ++i) for (int b = 0; b < 32; ++b) kf.mDescriptors.ptr(i)[b] = (uint8_t)rnd();
        std::vector<cv::KeyPoint>& left = two ? kf.mvKeys : kf.mvKeysUn;
        left.resize(nl); kf.mvKeysRight.resize(nr);
        for (auto& kp : left) kp.octave = (int)(rnd() % 8);
        for (auto& kp : kf.mvKeysRight) kp.octave = (int)(rnd() % 8);
        float f = 1.f;
        for (int l = 0; l < 8; ++l) { kf.mvScaleFactors.push_back(f); f *= 1.2f; }
        for (int i = 0; i < 3; ++i) { kf.ow[i] = frnd(-2.f, 2.f); kf.owr[i] = kf.ow[i] + frnd(-0.2f, 0.2f); }
        kf.bad = k == 4;
    }
    std::vector<MapPoint> mps(nmp);
    std::vector<uint8_t> keepDesc(32, 0xAB);
    for (int i = 0; i < nmp; ++i) {
        MapPoint& mp = mps[i];
        mp.mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) mp.mWorldPos.at<float>(r) = frnd(-6.f, 6.f);
        const int nobs = i % 10 == 0 ? 0 : 1 + (int)(rnd() % nkf);          // every tenth MapPoint has no observation at all
        for (int o = 0; o < nobs; ++o) {
            KeyFrame* kf = &kfs[rnd() % nkf];
            int left = (int)(rnd() % (unsigned)(kf->NLeft == -1 ? kf->mDescriptors.rows : kf->NLeft)), right = -1;
            if (kf->NLeft != -1) {
                right = kf->NLeft + (int)(rnd() % (unsigned)kf->mvKeysRight.size());
                if (rnd() % 3 == 0) left = -1;                              // seen by the right camera only
                else if (rnd() % 2 == 0) right = -1;
            }
            mp.mObservations[kf] = std::make_tuple(left, right);
            if (!mp.mpRefKF || rnd() % 4 == 0) mp.mpRefKF = kf;
        }
        if (i % 10 == 5) {                                                   // only the bad KeyFrame observes it: no descriptor, but a normal
            mp.mObservations.clear();
            mp.mObservations[&kfs[4]] = std::make_tuple(3, -1);
            mp.mpRefKF = &kfs[4];
        }
        mp.mbBad = i % 17 == 3;
        mp.mDescriptor = cv::Mat(1, 32, CV_8U); std::memcpy(mp.mDescriptor.ptr(0), keepDesc.data(), 32);
        mp.mNormalVector = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) mp.mNormalVector.at<float>(r) = -9.f;
    }
    // the duplicate / complement case: A, ~A, ~A over three KeyFrames in pointer order picks the first ~A
    {
        MapPoint& mp = mps[1];
        mp.mObservations.clear();
        for (int k = 0; k < 3; ++k) mp.mObservations[&kfs[k]] = std::make_tuple(k == 2 ? -1 : 7, k == 2 ? kfs[2].NLeft + 2 : -1);
        for (int b = 0; b < 32; ++b) {
            const uint8_t a = kfs[0].mDescriptors.ptr(7)[b];
            kfs[1].mDescriptors.ptr(7)[b] = (uint8_t)~a; kfs[2].mDescriptors.ptr(kfs[2].NLeft + 2)[b] = (uint8_t)~a;
        }
        mp.mpRefKF = &kfs[2]; mp.mbBad = false;
    }
    if (orbx_device_count() < 1) { std::printf("facade MapPoint refresh compiled; no GPU here\n"); return argc > 1 ? 1 : 0; }
    orbm_t* m = nullptr;
    CHECK(orbm_create(&m, 0) == ORBM_OK, 2);
    std::vector<MapPoint*> vp;
    for (auto& mp : mps) vp.push_back(&mp);
    ORB_SLAM3::RefreshMapPoints(m, vp);
    int ndesc = 0, nnormal = 0, nkept = 0;
    for (int i = 0; i < nmp; ++i) {
        const MapPoint& mp = mps[i];
        const std::vector<uint8_t> want = expect_descriptor(mp);
        if (want.empty()) { CHECK(std::memcmp(mp.mDescriptor.ptr(0), keepDesc.data(), 32) == 0, 3); ++nkept; }
        else { CHECK(std::memcmp(mp.mDescriptor.ptr(0), want.data(), 32) == 0, 4); ++ndesc; }
        float nv[3], mn, mx;
        if (expect_normal(mp, nv, mn, mx)) {
            for (int r = 0; r < 3; ++r) CHECK(same(mp.mNormalVector.at<float>(r), nv[r]), 5);
            CHECK(same(mp.mfMinDistance, mn) && same(mp.mfMaxDistance, mx), 6);
            ++nnormal;
        } else {
            CHECK(mp.mNormalVector.at<float>(0) == -9.f && mp.mfMinDistance == -1.f && mp.mfMaxDistance == -1.f, 7);
        }
    }
    CHECK(ndesc > nmp / 2 && nkept >= nmp / 10 && nnormal > ndesc, 8);      // the bad-KeyFrame-only MapPoints get a normal and no descriptor
    CHECK(std::memcmp(mps[1].mDescriptor.ptr(0), kfs[1].mDescriptors.ptr(7), 32) == 0, 9);
    // the single-MapPoint forms write the same members
    MapPoint one = mps[2];
    one.mDescriptor = mps[2].mDescriptor.clone(); std::memcpy(one.mDescriptor.ptr(0), keepDesc.data(), 32);   // a copy: cv::Mat shares its bytes
    one.mfMinDistance = one.mfMaxDistance = -1.f;
    ORB_SLAM3::ComputeDistinctiveDescriptors(m, &one);
    CHECK(one.mfMaxDistance == -1.f && std::memcmp(one.mDescriptor.ptr(0), mps[2].mDescriptor.ptr(0), 32) == 0, 10);
    ORB_SLAM3::UpdateNormalAndDepth(m, &one);
    CHECK(same(one.mfMaxDistance, mps[2].mfMaxDistance) && same(one.mNormalVector.at<float>(2), mps[2].mNormalVector.at<float>(2)), 11);
    std::vector<MapPoint*> none;
    ORB_SLAM3::RefreshMapPoints(m, none);
    orbm_destroy(m);
    std::printf("facade_mappoint_smoke ok: %d descriptors, %d normals, %d MapPoints left untouched\n", ndesc, nnormal, nkept);
    return 0;
}
