// Mock KeyFrame / camera / matcher types with the members facade/CreateNewMapPoints.h reads, filled from a case of
// tests/triangulate_case_io.h: the current KeyFrame is row row1[0] of pool 1, the neighbours are the rows row2[p] of pool 2.
#pragma once
#include <utility>
#include <vector>
#include "../orb-slam3_amd/facade/cvcompat.h"
#include "../include/orbm.h"
#include "triangulate_case_io.h"

struct MockCamera {
    unsigned int mnType = 0;
    unsigned int GetType() { return mnType; }
    const unsigned int CAM_PINHOLE = 0;
    const unsigned int CAM_FISHEYE = 1;
};

struct MockKeyFrame {
    int N = 0, NLeft = -1;
    std::vector<cv::KeyPoint> mvKeysUn, mvKeys;
    std::vector<float> mvuRight, mvDepth, mvScaleFactors, mvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mb = 0, mbf = 0, mfScaleFactor = 1.2f, medianDepth = 5.f;
    MockCamera cam;
    MockCamera* mpCamera = &cam;
    const void* mpCamera2 = nullptr;
    float T[12] = {0}, O[3] = {0};
    cv::Matx33f GetRotation_() { cv::Matx33f R; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R(i, j) = T[4 * i + j]; return R; }
    cv::Matx31f GetTranslation_() { cv::Matx31f t; for (int i = 0; i < 3; ++i) t(i, 0) = T[4 * i + 3]; return t; }
    cv::Matx31f GetCameraCenter_() { cv::Matx31f o; for (int i = 0; i < 3; ++i) o(i, 0) = O[i]; return o; }
    float ComputeSceneMedianDepth(int) { return medianDepth; }
};

static void keyframe_from_pool(const Pool& p, int row, const float* k, float mb, float mbf, const std::vector<float>& sf, const std::vector<float>& ls,
                               MockKeyFrame& K) {
    int n = p.counts[row]; n = n < 0 ? 0 : n > p.cap ? p.cap : n;
    K.N = n;
    K.mvKeysUn.assign(n, cv::KeyPoint()); K.mvKeys.assign(n, cv::KeyPoint()); K.mvuRight.resize(n); K.mvDepth.resize(n);
    for (int i = 0; i < n; ++i) {
        const size_t s = (size_t)row * p.cap + i;
        K.mvKeysUn[i].pt.x = p.ux[s]; K.mvKeysUn[i].pt.y = p.uy[s]; K.mvKeysUn[i].octave = p.octave[s];
        K.mvKeys[i].pt.x = p.kx[s]; K.mvKeys[i].pt.y = p.ky[s]; K.mvKeys[i].octave = p.octave[s];
        K.mvuRight[i] = p.uright[s]; K.mvDepth[i] = p.depth[s];
    }
    K.fx = k[0]; K.fy = k[1]; K.cx = k[2]; K.cy = k[3]; K.invfx = k[4]; K.invfy = k[5]; K.mb = mb; K.mbf = mbf;
    K.mvScaleFactors = sf; K.mvLevelSigma2 = ls; K.mfScaleFactor = sf.size() > 1 ? sf[1] : 1.2f;
    for (int i = 0; i < 12; ++i) K.T[i] = p.tcw[12 * (size_t)row + i];
    for (int i = 0; i < 3; ++i) K.O[i] = p.ow[3 * (size_t)row + i];
}

// the KeyFrames of a one-group case: cur and one neighbour per pair
struct MockScene {
    MockKeyFrame cur;
    std::vector<MockKeyFrame> store;
    std::vector<MockKeyFrame*> neigh;
    explicit MockScene(const TriCase& c) : store(c.npairs) {
        keyframe_from_pool(c.a, c.row1[0], &c.fl[0], c.fl[12], c.fl[13], c.sf1, c.ls1, cur);
        for (int p = 0; p < c.npairs; ++p) {
            keyframe_from_pool(c.b, c.row2[p], &c.fl[6], c.fl[14], c.fl[14] * c.fl[6], c.sf2, c.ls2, store[p]);
            neigh.push_back(&store[p]);
        }
    }
};

// A matcher that answers SearchForTriangulation_ with the case's matches12 row of the neighbour asked about (the M10 facade itself is
// exercised by tests/facade_smoke.cpp); handle() is the real handle, or NULL in the CPU program, which never calls the library.
struct MockMatcher {
    const TriCase& c; const MockScene& s; orbm_t* h;
    int searches = 0, lastCoarse = -1;
    MockMatcher(const TriCase& c_, const MockScene& s_, orbm_t* h_) : c(c_), s(s_), h(h_) {}
    orbm_t* handle() { return h; }
    int SearchForTriangulation_(MockKeyFrame* k1, MockKeyFrame* k2, cv::Matx33f, std::vector<std::pair<size_t, size_t>>& out, bool, bool bCoarse) {
        ++searches; lastCoarse = bCoarse;
        out.clear();
        const int p = (int)(k2 - &s.store[0]);
        for (int i = 0; i < k1->N; ++i) {
            const int m = c.m12[(size_t)p * c.a.cap + i];
            if (m >= 0 && m < k2->N) out.push_back(std::make_pair((size_t)i, (size_t)m));
        }
        return (int)out.size();
    }
};
