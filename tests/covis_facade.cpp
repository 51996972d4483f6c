// facade/Covisibility.h on the mock types of tests/kfcull_mock.h, without a GPU and without the library: this file defines
// orbm_covisibility_votes and orbm_local_points itself, as plain loops over the contract of include/orbm.h, so the facade's flatten and its
// results can be compared with tests/second_reading_covis.py on the CPU (tests/test_covis_facade_cpu.py).  It also restates the
// reference's own loops (tests/covis_mock.h) on the mock objects: the single-thread baseline of tools/covisibility_batch.py.
//   covis_facade MAPFILE          prints the flatten and the three results
//   covis_facade bench nq nslots nkf mean_obs hot T nlkf lslots reps   times the reference loops on a synthetic map, microseconds per call
// MAPFILE: the text form of tests/kfcull_mock.h, then
//   nother | KeyFrame indices that lie in a second map
//   nslots | the Frame's MapPoint indices (-1 = NULL)
//   nlocal | KeyFrame indices of mvpLocalKeyFrames
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include "covis_mock.h"

// ---- the two host entry points as loops over the contract ------------------------------------------------------------------
static bool live(int e, int nkf_rows, int cap, const int32_t* counts_kf, const int32_t* obs_row, const int32_t* obs_slot) {
    const int r = obs_row[e], s = obs_slot[e];
    return r >= 0 && r < nkf_rows && s >= 0 && s < (counts_kf[r] < cap ? counts_kf[r] : cap);
}
extern "C" const char* orbm_last_error(void) { return "stand-in"; }
extern "C" int orbm_covisibility_votes(orbm_t*, int nq, int q_stride, const int32_t* q_mp, const int32_t* q_n, const int32_t* self_row, int nkf_rows, int cap,
                                       const int32_t* counts_kf, const uint8_t* kf_skip, int skip_bad, int nmp, int nobs, const int32_t* obs_off,
                                       const int32_t* obs_row, const int32_t* obs_slot, const uint8_t* obs_flags, const uint8_t* mp_valid, int th, int list_cap,
                                       int32_t* votes, int32_t* n_voted, int32_t* max_votes, int32_t* n_over, int32_t* list_row, int32_t* list_votes) {
    auto voter = [&](int e, int self) {
        if (!live(e, nkf_rows, cap, counts_kf, obs_row, obs_slot)) return -1;
        const int r = obs_row[e];
        if (r == self || (kf_skip && kf_skip[r]) || (skip_bad && (obs_flags[e] & 2))) return -1;
        return r;
    };
    for (int q = 0; q < nq; ++q) {
        int32_t* v = votes + (size_t)q * nkf_rows;
        for (int r = 0; r < nkf_rows; ++r) v[r] = 0;
        const int self = self_row ? self_row[q] : -1;
        const int n = q_n[q] < 0 ? 0 : (q_n[q] < q_stride ? q_n[q] : q_stride);
        for (int i = 0; i < n; ++i) {
            const int j = q_mp[(size_t)q * q_stride + i];
            if (j < 0 || j >= nmp || (mp_valid && !mp_valid[j])) continue;
            const int a = obs_off[j], b = obs_off[j + 1];
            if (a < 0 || b > nobs || b <= a || b - a > ORBM_MP_MAX_OBS) continue;
            for (int e = a; e < b; ++e) {
                const int r = voter(e, self);
                if (r < 0) continue;
                if ((obs_flags[e] & 1) && e > a && obs_row[e - 1] == r && !(obs_flags[e - 1] & 1) && voter(e - 1, self) == r) continue;
                v[r]++;
            }
        }
        int nv = 0, mx = 0, no = 0;
        for (int r = 0; r < nkf_rows; ++r)
            if (v[r] > 0) {
                if (nv < list_cap) { list_row[(size_t)q * list_cap + nv] = r; list_votes[(size_t)q * list_cap + nv] = v[r]; }
                nv++; if (v[r] > mx) mx = v[r]; if (v[r] >= th) no++;
            }
        n_voted[q] = nv; max_votes[q] = mx; n_over[q] = no;
    }
    return 0;
}
extern "C" int orbm_local_points(orbm_t*, int T, int lkf_stride, const int32_t* lkf_row, const int32_t* n_lkf, int nkf_rows, int cap, const int32_t* counts_kf,
                                 const int32_t* kf_mp, int nmp, const uint8_t* mp_valid, int q_stride, int32_t* local_mp, int32_t* n_total, int32_t* nq) {
    for (int f = 0; f < T; ++f) {
        std::vector<char> seen(nmp, 0);
        int n = 0;
        const int nl = n_lkf[f] < 0 ? 0 : (n_lkf[f] < lkf_stride ? n_lkf[f] : lkf_stride);
        for (int k = 0; k < nl; ++k) {
            const int r = lkf_row[(size_t)f * lkf_stride + k];
            if (r < 0 || r >= nkf_rows) continue;
            for (int i = 0; i < (counts_kf[r] < cap ? counts_kf[r] : cap); ++i) {
                const int j = kf_mp[(size_t)r * cap + i];
                if (j < 0 || j >= nmp || (mp_valid && !mp_valid[j]) || seen[j]) continue;
                seen[j] = 1;
                if (n < q_stride) local_mp[(size_t)f * q_stride + n] = j;
                n++;
            }
        }
        n_total[f] = n; nq[f] = n < q_stride ? n : q_stride;
    }
    return 0;
}

template <class T> static void put(const char* name, const std::vector<T>& v) {
    std::printf("%s %zu", name, v.size());
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}
static void putCounter(const char* name, int q, const MockMap& M, const std::map<KeyFrame*, int>& c) {
    std::printf("%s%d %zu", name, q, 2 * c.size());
    for (auto& kv : c) std::printf(" %lld %d", (long long)(kv.first - &M.kfs[0]), kv.second);
    std::printf("\n");
}

static int bench(int argc, char** argv) {
    if (argc < 11) return 2;
    const int nq = atoi(argv[2]), nslots = atoi(argv[3]), nkf = atoi(argv[4]), meanObs = atoi(argv[5]), hot = atoi(argv[6]), T = atoi(argv[7]), nlkf = atoi(argv[8]),
              lslots = atoi(argv[9]), reps = atoi(argv[10]);
    std::mt19937 rng(7);
    MockMap M;
    M.kfs.resize(nkf); M.mps.resize((size_t)nq * nslots);
    for (int k = 0; k < nkf; ++k) { M.kfs[k].mnId = k; M.kfs[k].mpMap = &M.map; }
    // every MapPoint is seen by about meanObs KeyFrames, nine in ten of them among the first `hot` rows; a KeyFrame grows a slot per observation
    for (MapPoint& mp : M.mps) {
        const int n = 1 + (int)(rng() % (2 * meanObs - 1));
        for (int e = 0; e < n; ++e) {
            KeyFrame& kf = M.kfs[(rng() % 10) ? rng() % hot : rng() % nkf];
            if (mp.mObservations.count(&kf)) continue;
            kf.mvpMapPoints.push_back(&mp); kf.mvuRight.push_back(-1.f);
            mp.AddObservation(&kf, kf.N++);
        }
    }
    std::vector<Frame> frames(nq);
    for (int q = 0; q < nq; ++q) { frames[q].N = nslots; for (int i = 0; i < nslots; ++i) frames[q].mvpMapPoints.push_back(&M.mps[(size_t)q * nslots + i]); }
    // the local map: nlkf KeyFrames of lslots slots over a pool in which a MapPoint sits in about four of them
    std::vector<KeyFrame> lkfs(nlkf);
    std::vector<MapPoint> lmps((size_t)nlkf * lslots / 4 + 1);
    std::vector<KeyFrame*> local;
    for (KeyFrame& kf : lkfs) {
        kf.N = lslots; kf.mpMap = &M.map;
        for (int i = 0; i < lslots; ++i) kf.mvpMapPoints.push_back(&lmps[rng() % lmps.size()]);
        local.push_back(&kf);
    }
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    size_t sink = 0;
    double t0 = now();
    for (int r = 0; r < reps; ++r) for (int q = 0; q < nq; ++q) sink += ReferenceLocalKeyFrameVotes(frames[q]).size();
    const double votes_us = (now() - t0) / reps;
    t0 = now();
    for (int r = 0; r < reps; ++r) for (int q = 0; q < nq && q < hot; ++q) sink += ReferenceConnectionCounts(&M.kfs[q]).size();
    const double conn_us = (now() - t0) / reps;
    TrackTable track(lmps);
    t0 = now();
    for (int r = 0; r < reps; ++r) for (int f = 0; f < T; ++f) sink += ReferenceLocalMapPoints(local, (unsigned long)(r * T + f), track).size();
    const double local_us = (now() - t0) / reps;
    std::printf("{\"votes_frame_us\": %.1f, \"votes_keyframe_us\": %.1f, \"local_points_us\": %.1f, \"sink\": %zu}\n", votes_us, conn_us, local_us, sink);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "bench") return bench(argc, argv);
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    MockMap M;
    if (!f || !LoadMockMap(f, M)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    Map other;
    Frame frame;
    std::vector<KeyFrame*> local;
    int n, k;
    if (std::fscanf(f, "%d", &n) != 1) return 2;
    for (int i = 0; i < n; ++i) { if (std::fscanf(f, "%d", &k) != 1) return 2; M.kfs[k].mpMap = &other; }
    if (std::fscanf(f, "%d", &n) != 1) return 2;
    for (int i = 0; i < n; ++i) { if (std::fscanf(f, "%d", &k) != 1) return 2; frame.mvpMapPoints.push_back(k < 0 ? nullptr : &M.mps[k]); }
    frame.N = n;
    if (std::fscanf(f, "%d", &n) != 1) return 2;
    for (int i = 0; i < n; ++i) { if (std::fscanf(f, "%d", &k) != 1) return 2; local.push_back(&M.kfs[k]); }
    std::fclose(f);
    using namespace ORB_SLAM3;
    // the batch of every KeyFrame of the first map that is not bad: flatten, then the facade's results beside the reference's loops
    std::vector<KeyFrame*> queries;
    for (KeyFrame& kf : M.kfs) if (!kf.isBad() && kf.GetMap() == &M.map) queries.push_back(&kf);
    bool ok = true;
    if (!queries.empty()) {
        std::vector<std::vector<MapPoint*>> slots;
        for (KeyFrame* p : queries) slots.push_back(p->GetMapPointMatches());
        covis::Flat<KeyFrame> F;
        F.build(slots, queries);
        F.skipOtherMaps(&M.map);
        std::printf("cap 1 %d\nq_stride 1 %d\n", F.cap, F.qStride);
        put("q_mp", F.qMp); put("q_n", F.qN); put("self_row", F.selfRow); put("counts_kf", F.counts); put("kf_skip", F.kfSkip);
        put("obs_off", F.off); put("obs_row", F.row); put("obs_slot", F.slot); put("obs_flags", F.flags); put("mp_valid", F.valid);
        std::vector<long long> rows; for (KeyFrame* p : F.rows) rows.push_back(p - &M.kfs[0]);
        put("rows", rows);
        const auto batch = covis::ConnectionCountsBatch(nullptr, queries);
        for (size_t q = 0; q < queries.size(); ++q) {
            putCounter("conn", (int)q, M, batch[q]);
            ok = ok && batch[q] == ReferenceConnectionCounts(queries[q]) && batch[q] == covis::ConnectionCounts((orbm_t*)nullptr, queries[q]);
        }
    }
    Frame twin = frame;
    const auto fv = covis::LocalKeyFrameVotes((orbm_t*)nullptr, frame);
    putCounter("frame", 0, M, fv);
    ok = ok && fv == ReferenceLocalKeyFrameVotes(twin) && twin.mvpMapPoints == frame.mvpMapPoints;
    std::vector<long long> cleared; for (MapPoint* p : frame.mvpMapPoints) cleared.push_back(p ? p - &M.mps[0] : -1);
    put("frame_slots", cleared);
    const auto lp = covis::LocalMapPoints((orbm_t*)nullptr, local);
    TrackTable track(M.mps);
    ok = ok && lp == ReferenceLocalMapPoints(local, 1, track);
    std::vector<long long> lpi; for (MapPoint* p : lp) lpi.push_back(p - &M.mps[0]);
    put("local", lpi);
    std::printf("same_as_reference_loops 1 %d\n", ok ? 1 : 0);
    return 0;
}
