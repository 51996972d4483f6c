// A single-thread C++ loop over the flattened arrays of orbm_keyframe_culling (include/orbm.h), for tools/keyframe_culling.py: the same
// contract -- skip rules, erased rows, weights, pairs, the float compare -- with the reference's early break where no row is erased.
// It is NOT the reference: LocalMapping::KeyFrameCulling walks std::map nodes and KeyFrame objects behind pointers and takes a mutex per
// MapPoint; this loop reads the contiguous arrays a device-resident caller would have to download or rebuild first.  Compiled with
// g++ -O2 when the tool starts.  Returns the median time of `reps` runs in ms.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <vector>

struct Kp { float x, y, size, angle, response; int32_t octave, class_id; };

static void run(int ncand, const int32_t* cand_row, int nkf_rows, int cap, const Kp* kps, const int32_t* counts, const int32_t* kf_mp, const float* depth,
                float th_depth, int nmp, int nobs, const int32_t* off, const int32_t* row, const int32_t* slot, const uint8_t* flags, const uint8_t* valid,
                const int32_t* mp_nobs, const uint8_t* erased, int th_obs, float th, int32_t* n_mps, int32_t* n_red, uint8_t* cull) {
    auto live = [&](int e) { const int r = row[e], s = slot[e]; return r >= 0 && r < nkf_rows && s >= 0 && s < std::min(counts[r], cap); };
    for (int k = 0; k < ncand; ++k) {
        n_mps[k] = n_red[k] = 0; cull[k] = 0;
        const int r = cand_row[k];
        if (r < 0 || r >= nkf_rows || (erased && erased[r])) continue;
        const int n = std::min(counts[r], cap);
        for (int i = 0; i < n; ++i) {
            const size_t at = (size_t)k * cap + i;
            const int j = kf_mp[at];
            if (j < 0 || j >= nmp || (valid && !valid[j])) continue;
            if (depth && (depth[at] > th_depth || depth[at] < 0)) continue;
            int a = off[j], b = off[j + 1];
            if (a < 0 || b > nobs || b <= a || b - a > 65535) a = b = 0;
            long long eff = mp_nobs[j];
            bool any = false;
            if (erased)
                for (int e = a; e < b; ++e)
                    if (live(e) && erased[row[e]]) { eff -= (flags[e] & 4) ? 2 : 1; any = true; }
            if (any && eff <= 2) continue;
            n_mps[k]++;
            if (eff <= th_obs) continue;
            const long long top = (long long)kps[(size_t)r * cap + i].octave + 1;
            int cnt = 0;
            bool prevPass = false; int prevRow = -1; bool prevLeft = false;
            for (int e = a; e < b; ++e) {
                bool pass = false, lv = live(e);
                const int re = lv ? row[e] : -1;
                if (lv && !(erased && erased[re]) && re != r) pass = kps[(size_t)re * cap + slot[e]].octave <= top;
                const bool paired = lv && (flags[e] & 1) && prevRow == re && prevLeft && prevPass;
                if (pass && !paired) { if (++cnt > th_obs) break; }
                prevPass = pass; prevRow = re; prevLeft = lv && !(flags[e] & 1);
            }
            if (cnt > th_obs) n_red[k]++;
        }
        cull[k] = (float)n_red[k] > th * (float)n_mps[k];
    }
}

extern "C" double kfcull_host(int ncand, const int32_t* cand_row, int nkf_rows, int cap, const Kp* kps, const int32_t* counts, const int32_t* kf_mp,
                              const float* depth, float th_depth, int nmp, int nobs, const int32_t* off, const int32_t* row, const int32_t* slot,
                              const uint8_t* flags, const uint8_t* valid, const int32_t* mp_nobs, const uint8_t* erased, int th_obs, float th,
                              int32_t* n_mps, int32_t* n_red, uint8_t* cull, int reps) {
    std::vector<double> ms;
    for (int t = 0; t < reps; ++t) {
        const auto t0 = std::chrono::steady_clock::now();
        run(ncand, cand_row, nkf_rows, cap, kps, counts, kf_mp, depth, th_depth, nmp, nobs, off, row, slot, flags, valid, mp_nobs, erased, th_obs, th, n_mps, n_red, cull);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}
