// The two MapPoint refresh loops as a caller runs them today, single-threaded on the host over the same arrays as the library calls
// (MapPoint.cc:450-538 and :578-652 restated in plain C++): the baseline of tools/mappoint_refresh_batch.py.  Not part of the product.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

static inline int ham(const uint8_t* a, const uint8_t* b) {
    uint64_t x[4], y[4];
    std::memcpy(x, a, 32); std::memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

extern "C" int mp_refresh_host(int nmp, int nkf_rows, int cap, const uint8_t* desc_kf, const int32_t* kp_octave, const int32_t* counts_kf, const float* ow_l,
                               const float* ow_r, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot, const uint8_t* obs_flags,
                               const float* pw, const int32_t* ref_row, const int32_t* ref_slot, const float* scale, int nlevels,
                               uint8_t* mp_desc, float* normal, float* min_dist, float* max_dist) {
    std::vector<const uint8_t*> v;
    std::vector<float> dist;
    std::vector<int> rowd;
    int done = 0;
    for (int mp = 0; mp < nmp; ++mp) {
        v.clear();
        float acc[3] = {0.f, 0.f, 0.f};
        int n = 0;
        const float* p = pw + 3 * mp;
        for (int e = obs_off[mp]; e < obs_off[mp + 1]; ++e) {
            const int r = obs_row[e], s = obs_slot[e];
            if (r < 0 || r >= nkf_rows || s < 0 || s >= counts_kf[r]) continue;
            if (!(obs_flags[e] & 2)) v.push_back(desc_kf + ((size_t)r * cap + s) * 32);
            const float* ow = ((obs_flags[e] & 1) ? ow_r : ow_l) + 3 * r;
            const float d[3] = {p[0] - ow[0], p[1] - ow[1], p[2] - ow[2]};
            const float sc = (float)(1.0 / std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]));
            for (int i = 0; i < 3; ++i) { const float t = d[i] * sc; acc[i] = acc[i] + t; }
            ++n;
        }
        const size_t N = v.size();
        if (N) {
            dist.assign(N * N, 0.f);
            for (size_t i = 0; i < N; ++i)
                for (size_t j = i + 1; j < N; ++j) dist[i * N + j] = dist[j * N + i] = (float)ham(v[i], v[j]);
            int best = 1 << 30; size_t bi = 0;
            for (size_t i = 0; i < N; ++i) {
                rowd.assign(dist.begin() + i * N, dist.begin() + (i + 1) * N);
                std::sort(rowd.begin(), rowd.end());
                const int med = rowd[(size_t)(0.5 * (N - 1))];
                if (med < best) { best = med; bi = i; }
            }
            std::memcpy(mp_desc + (size_t)mp * 32, v[bi], 32);
            ++done;
        }
        const int rr = ref_row[mp], rs = ref_slot[mp];
        if (n && rr >= 0 && rr < nkf_rows && rs >= 0 && rs < counts_kf[rr]) {
            const int level = kp_octave[(size_t)rr * cap + rs];
            if (level < 0 || level >= nlevels) continue;
            const float* ow = ow_l + 3 * rr;
            const float d[3] = {p[0] - ow[0], p[1] - ow[1], p[2] - ow[2]};
            const float dd = (float)std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
            max_dist[mp] = dd * scale[level];
            min_dist[mp] = max_dist[mp] / scale[nlevels - 1];
            const float inv = (float)(1.0 / n);
            for (int i = 0; i < 3; ++i) normal[3 * mp + i] = acc[i] * inv;
        }
    }
    return done;
}
