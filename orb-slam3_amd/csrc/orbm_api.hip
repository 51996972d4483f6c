// orbm_api.hip -- C ABI (include/orbm.h) over the gfx950 matcher kernels.  No CPU fallback for the
// device entry points; orbm_hamming / orbm_three_maxima are the reference's scalar helpers and stay scalar.
#include "../../include/orbm.h"
#include "orbm_kernels.hip.h"

#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace orbmk;

// A/B switches and test knobs exist only in the -DORBX_AB build (see orbx_api.hip)
#ifdef ORBX_AB
static inline const char* ab_env(const char* name) { return getenv(name); }
#else
static inline const char* ab_env(const char*) { return nullptr; }
#endif

static thread_local std::string g_merr;
static void set_merr(const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_merr = buf;
}
#define MHIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_merr("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); return ORBM_E_HIP; } } while (0)

struct orbm {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t ownStream = nullptr;                           // the stream created with the handle (orbm_set_stream may point `stream` elsewhere)
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    bool timed = false, gridFirst = false;
    bool dselLds = false;                                      // k_depth_select's dynamic LDS limit has been raised (orbm_select_depth_points*)
    bool bowvLds = false;                                      // k_bow_vector's dynamic LDS limit has been raised (orbm_bow_vector_batch_async)
    bool initLds = false;                                      // k_init_search's dynamic LDS limit has been raised (orbm_search_for_initialization_batch_async)
    // Scratch arena of the single-frame entry points: ONE device block and a pinned host mirror of the same size.  Uploads are
    // staged in the mirror and sent with one asynchronous copy before the kernel, results come back with one copy after it
    // (a dozen hipMalloc / small pageable copies per call cost over a millisecond).
    uint8_t* arDev = nullptr; uint8_t* arPin = nullptr;
    size_t arCap = 0, arOff = 0, arUp = 0, arOutLo = (size_t)-1, arOutHi = 0;   // bump offset; [0, arUp) staged uploads; small outputs in [arOutLo, arOutHi)
    uint8_t* scr = nullptr; size_t scrCap = 0;                 // grow-only device scratch of the batched (enqueue-only) entry points
    std::vector<uint8_t*> scrOld;                              // superseded scratch blocks: graphs captured earlier still hold their addresses, so they live as long as the handle
    int* hStatus = nullptr;                                    // pinned, device-visible status word of the enqueue-only entry points (capacity overflows); read by orbm_sync
};

// scratch of the enqueue-only entry points: grows outside a capture only (an allocation cannot be recorded into a graph)
static uint8_t* batch_scratch(orbm* m, size_t bytes) {
    if (bytes <= m->scrCap && m->scr) return m->scr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(m->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) return nullptr;
    // grow by ADDING: a step graph captured through orbx_capture_begin keeps the old block's address in its kernel nodes, and
    // a later eager call with more pairs must not turn that graph's next replay into a use-after-free
    uint8_t* nb = nullptr;
    if (hipMalloc((void**)&nb, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (m->scr) m->scrOld.push_back(m->scr);
    m->scr = nb; m->scrCap = bytes;
    return m->scr;
}

// time stamps: under stream capture (the caller replays this enqueue sequence as a HIP graph, orbx_capture_begin) an event
// record stamps nothing on replay, so it is skipped there: orbm_last_timing keeps reporting the last eagerly enqueued call
static hipError_t rec_time(orbm* m, hipEvent_t ev) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(m->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) return hipSuccess;
    return hipEventRecord(ev, m->stream);
}

// A frame kept in HBM across searches (orbm_frame_create): keypoints, descriptors, mvuRight and the 64 x 48 grid as CSR.
struct orbm_dframe {
    int device = 0, n = 0;
    uint8_t* block = nullptr;                                  // owned allocation: [kps | desc | uright] (host-created frames) + [grid_start | grid_idx]
    const KpIn* dKps = nullptr; const uint8_t* dDesc = nullptr; const float* dUr = nullptr;
    int *dGs = nullptr, *dGi = nullptr;
    std::vector<orbm_kp_t> hkps;                               // host copy: the replay reads angle / octave of the matched keypoint
    float min_x = 0, min_y = 0, inv_w = 0, inv_h = 0;
};

static inline size_t grid_cs_lds(int n) { return (size_t)(2 * GRID_CELLS + 1) * sizeof(int) + (size_t)std::max(n, 1) * sizeof(unsigned short) + 16; }
// Above GRID_WIDE_MIN keypoints the grid builders run the WIDE counting form, whose dynamic LDS (155 666 B at 65535, with 2 068 B static
// beside it: 160 KB hold both) is above 48 KB: the attribute always at the largest legal size, so that a graph captured earlier with
// bigger rows still launches after a call with smaller ones.
static inline hipError_t grid_wide_attr(const void* kernel) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)grid_cs_lds(65535));
}

namespace { int knn2_host(orbm* m, const uint8_t* q, int q_stride, const int32_t* nq, const uint8_t* t, int t_stride, const int32_t* nt,
                          int npairs, int32_t* idx2, int32_t* dist2); }

extern "C" {

const char* orbm_last_error(void) { return g_merr.c_str(); }

int orbm_create(orbm_t** out, int device_id) {
    if (!out) return ORBM_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_merr("no HIP device: the MI355X matcher has no CPU fallback"); return ORBM_E_HIP; }
    if (device_id < 0 || device_id >= ndev) { set_merr("device %d out of range", device_id); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(device_id));
    orbm* m = new orbm;
    m->device = device_id;
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&m->e0) != hipSuccess ||
        hipEventCreate(&m->e1) != hipSuccess || hipEventCreate(&m->e2) != hipSuccess ||
        hipHostMalloc((void**)&m->hStatus, 64, hipHostMallocDefault) != hipSuccess) { set_merr("stream/event creation failed"); orbm_destroy(m); return ORBM_E_HIP; }
    *m->hStatus = 0;
    m->ownStream = m->stream;
    *out = m;
    return ORBM_OK;
}

void orbm_destroy(orbm_t* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->ownStream) { (void)hipStreamSynchronize(m->ownStream); (void)hipStreamDestroy(m->ownStream); }
    if (m->arDev) (void)hipFree(m->arDev);
    if (m->scr) (void)hipFree(m->scr);
    for (uint8_t* p : m->scrOld) (void)hipFree(p);
    if (m->hStatus) (void)hipHostFree(m->hStatus);
    if (m->arPin) (void)hipHostFree(m->arPin);
    if (m->e0) (void)hipEventDestroy(m->e0);
    if (m->e1) (void)hipEventDestroy(m->e1);
    if (m->e2) (void)hipEventDestroy(m->e2);
    delete m;
}

int orbm_sync(orbm_t* m) {
    if (!m) return ORBM_E_INVALID;
    MHIPCHK(hipSetDevice(m->device));
    MHIPCHK(hipStreamSynchronize(m->stream));
    if (m->hStatus && *(volatile int*)m->hStatus) {             // set by a kernel of an enqueue-only call since the last sync
        const int st = *(volatile int*)m->hStatus;
        *(volatile int*)m->hStatus = 0;
        set_merr("a batched call overflowed a device-side list (status 0x%x: 1 = stereo row lists): results of that call are incomplete", st);
        return ORBM_E_CAPACITY;
    }
    return ORBM_OK;
}

void* orbm_stream(const orbm_t* m) { return m ? (void*)m->stream : nullptr; }

int orbm_set_stream(orbm_t* m, void* stream) {
    if (!m) return ORBM_E_INVALID;
    hipStream_t ns = stream ? (hipStream_t)stream : m->ownStream;
    if (ns == m->stream) return ORBM_OK;                        // nothing to drain (and safe while that stream is being captured)
    MHIPCHK(hipSetDevice(m->device));
    MHIPCHK(hipStreamSynchronize(m->stream));
    m->stream = ns;
    return ORBM_OK;
}

int orbm_hamming(const uint8_t* a, const uint8_t* b) {
    uint64_t x[4], y[4];
    memcpy(x, a, 32); memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) +
           __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

void orbm_three_maxima(const int* sz, int L, int* ind3) {
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < L; ++i) {
        const int s = sz[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if (max3 < 0.1f * (float)max1) i3 = -1;
    ind3[0] = i1; ind3[1] = i2; ind3[2] = i3;
}

static int knn2_launch(orbm_t* m, const uint8_t* q, int q_stride, const int32_t* nq, const uint8_t* t, int t_stride,
                       const int32_t* nt, int npairs, int32_t* idx2, int32_t* dist2, double ratio, uint8_t* good);

int orbm_knn2_batch_async(orbm_t* m, const uint8_t* q, int q_stride, const int32_t* nq, const uint8_t* t, int t_stride,
                          const int32_t* nt, int npairs, int max_nt, int32_t* idx2, int32_t* dist2) {
    (void)max_nt;
    return knn2_launch(m, q, q_stride, nq, t, t_stride, nt, npairs, idx2, dist2, 0.0, nullptr);
}

int orbm_knn2_ratio_batch_async(orbm_t* m, const uint8_t* q, int q_stride, const int32_t* nq, const uint8_t* t, int t_stride,
                                const int32_t* nt, int npairs, double ratio, int32_t* idx2, int32_t* dist2, uint8_t* good) {
    if (!good) return ORBM_E_INVALID;
    return knn2_launch(m, q, q_stride, nq, t, t_stride, nt, npairs, idx2, dist2, ratio, good);
}

static int knn2_launch(orbm_t* m, const uint8_t* q, int q_stride, const int32_t* nq, const uint8_t* t, int t_stride,
                       const int32_t* nt, int npairs, int32_t* idx2, int32_t* dist2, double ratio, uint8_t* good) {
    if (!m || !q || !t || !nq || !nt || !idx2 || !dist2 || npairs < 1 || q_stride < 1 || t_stride < 1) return ORBM_E_INVALID;
    if (t_stride >= (1 << 22)) { set_merr("knn2: more than 2^22 train descriptors per pair"); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(m->device));
    m->gridFirst = false;
    MHIPCHK(rec_time(m, m->e0));
    // matrix-core kernel unless the train set is beyond its 19-bit row field (or ORBM_KNN2_VALU asks for the popcount kernel: A/B)
    const bool forceValu = ab_env("ORBM_KNN2_VALU") != nullptr;   // read per call: tests flip it
    if (t_stride <= KM_MAX_NT && !forceValu)
        hipLaunchKernelGGL(k_knn2_mfma, dim3((q_stride + 255) / 256, npairs), dim3(256), 0, m->stream, q, q_stride, nq, t, t_stride, nt, idx2, dist2, ratio, good);
    else
        hipLaunchKernelGGL(k_knn2, dim3((q_stride + 63) / 64, npairs), dim3(256), 0, m->stream, q, q_stride, nq, t, t_stride, nt, idx2, dist2, ratio, good);
    MHIPCHK(rec_time(m, m->e1));
    MHIPCHK(hipGetLastError());
    m->timed = true;
    return ORBM_OK;
}

int orbm_knn2_batch(orbm_t* m, int space, const uint8_t* q, int q_stride, const int32_t* nq, const uint8_t* t, int t_stride,
                    const int32_t* nt, int npairs, int32_t* idx2, int32_t* dist2) {
    if (!m) return ORBM_E_INVALID;
    if (space == ORBM_DEVICE) {
        int rc = orbm_knn2_batch_async(m, q, q_stride, nq, t, t_stride, nt, npairs, t_stride, idx2, dist2);
        if (rc) return rc;
        return orbm_sync(m);
    }
    if (!q || !t || !nq || !nt || !idx2 || !dist2 || npairs < 1 || q_stride < 1 || t_stride < 1) return ORBM_E_INVALID;
    return knn2_host(m, q, q_stride, nq, t, t_stride, nt, npairs, idx2, dist2);
}

int orbm_last_timing(orbm_t* m, float* ms) {
    if (!m || !m->timed) return ORBM_E_INVALID;
    MHIPCHK(hipSetDevice(m->device));
    MHIPCHK(hipStreamSynchronize(m->stream));
    MHIPCHK(hipEventElapsedTime(ms, m->gridFirst ? m->e2 : m->e0, m->e1));
    return ORBM_OK;
}

}  // extern "C"

// =================================================================================================
// Flattened searches: GPU distance phase + host replay of the reference's sequential bookkeeping
// =================================================================================================
extern "C" int orbx_internal_levels(void* o, int frame, int* nlevels, const uint8_t** ptr, int* pitch, int* w, int* h,
                                    float* sf, float* isf, int* device);

namespace {

// Arena sub-allocations.  A DevBuf is an (offset, size) view, resolved against the arena's current blocks when used, so the
// arena may grow (reallocate) while a function is still collecting its buffers.  Protocol inside one entry point:
//   arena_reset(m); UP(...) / AL(...) for every buffer (uploads first); ARENA_FLUSH(m); launch; sync; ARENA_FETCH(m); read .host()
struct DevBuf {
    orbm* m = nullptr; size_t off = 0, bytes = 0; bool ok = false;
    template <class T> T* as() { return ok ? (T*)(m->arDev + off) : nullptr; }
    void* ptr() { return as<void>(); }
    const void* host() const { return m->arPin + off; }
    bool alloc(orbm* mm, size_t n) {
        m = mm; bytes = n;
        const size_t start = (m->arOff + 255) & ~(size_t)255, end = start + std::max<size_t>(n, 4);
        if (end > m->arCap) {                               // grow: new blocks, staged bytes move over, old blocks go
            const size_t ncap = std::max(end * 2, (size_t)1 << 20);
            uint8_t *nd = nullptr, *np = nullptr;
            if (hipMalloc((void**)&nd, ncap) != hipSuccess || hipHostMalloc((void**)&np, ncap, hipHostMallocDefault) != hipSuccess) {
                if (nd) (void)hipFree(nd);
                return false;
            }
            if (m->arPin && m->arOff) memcpy(np, m->arPin, m->arOff);
            (void)hipStreamSynchronize(m->stream);
            if (m->arDev) (void)hipFree(m->arDev);
            if (m->arPin) (void)hipHostFree(m->arPin);
            m->arDev = nd; m->arPin = np; m->arCap = ncap;
        }
        off = start; m->arOff = end; ok = true;
        return true;
    }
    bool upload(orbm* mm, const void* src, size_t n) {
        if (!alloc(mm, n)) return false;
        if (n) memcpy(m->arPin + off, src, n);
        m->arUp = m->arOff;
        return true;
    }
};
static inline void arena_reset(orbm* m) { m->arOff = 0; m->arUp = 0; m->arOutLo = (size_t)-1; m->arOutHi = 0; }
#define UP(buf, src, bytes) do { if (!(buf).upload(m, (src), (bytes))) { set_merr("device upload failed (%zu B)", (size_t)(bytes)); return ORBM_E_HIP; } } while (0)
#define AL(buf, bytes) do { if (!(buf).alloc(m, (bytes))) { set_merr("device allocation failed (%zu B)", (size_t)(bytes)); return ORBM_E_HIP; } \
                            m->arOutLo = std::min(m->arOutLo, (buf).off); m->arOutHi = std::max(m->arOutHi, m->arOff); } while (0)
// large output read back selectively by the caller (not part of the ARENA_FETCH range): allocate these LAST
#define AL_BIG(buf, bytes) do { if (!(buf).alloc(m, (bytes))) { set_merr("device allocation failed (%zu B)", (size_t)(bytes)); return ORBM_E_HIP; } } while (0)
#define UPIO(buf, src, bytes) do { UP(buf, src, bytes); m->arOutLo = std::min(m->arOutLo, (buf).off); m->arOutHi = std::max(m->arOutHi, m->arOff); } while (0)   /* in/out buffer */
// one host-to-device copy for everything staged so far / one device-to-host copy of everything behind the uploads
#define ARENA_FLUSH(m) do { if ((m)->arUp) MHIPCHK(hipMemcpyAsync((m)->arDev, (m)->arPin, (m)->arUp, hipMemcpyHostToDevice, (m)->stream)); } while (0)
#define ARENA_FETCH(m) do { if ((m)->arOutHi > (m)->arOutLo) MHIPCHK(hipMemcpy((m)->arPin + (m)->arOutLo, (m)->arDev + (m)->arOutLo, (m)->arOutHi - (m)->arOutLo, hipMemcpyDeviceToHost)); } while (0)

// host-array form of orbm_knn2_batch (Frame::ComputeStereoFishEyeMatches hands over host descriptors): through the arena
int knn2_host(orbm* m, const uint8_t* q, int q_stride, const int32_t* nq, const uint8_t* t, int t_stride, const int32_t* nt,
              int npairs, int32_t* idx2, int32_t* dist2) {
    MHIPCHK(hipSetDevice(m->device));
    const size_t qb = (size_t)npairs * q_stride * 32, tb = (size_t)npairs * t_stride * 32, ob = (size_t)npairs * q_stride * 2 * sizeof(int);
    DevBuf dq, dt, dnq, dnt, di, dd;
    arena_reset(m);
    UP(dq, q, qb); UP(dt, t, tb); UP(dnq, nq, sizeof(int) * npairs); UP(dnt, nt, sizeof(int) * npairs);
    AL(di, ob); AL(dd, ob);
    ARENA_FLUSH(m);
    int rc = orbm_knn2_batch_async(m, dq.as<uint8_t>(), q_stride, dnq.as<int32_t>(), dt.as<uint8_t>(), t_stride, dnt.as<int32_t>(), npairs, t_stride,
                                   di.as<int32_t>(), dd.as<int32_t>());
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(idx2, di.host(), ob); memcpy(dist2, dd.host(), ob);
    return ORBM_OK;
}

struct RotHist {                                             // rotation-consistency histogram (e.g. ORBmatcher.cc:459-466)
    std::vector<int> bins[ORBM_HISTO_LENGTH];
    void add(float a1, float a2, float factor, int idx) {
        float rot = a1 - a2;
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == ORBM_HISTO_LENGTH) bin = 0;
        if (bin >= 0 && bin < ORBM_HISTO_LENGTH) bins[bin].push_back(idx);
    }
    void maxima(int* ind) const {
        int sz[ORBM_HISTO_LENGTH];
        for (int i = 0; i < ORBM_HISTO_LENGTH; ++i) sz[i] = (int)bins[i].size();
        orbm_three_maxima(sz, ORBM_HISTO_LENGTH, ind);
    }
    // fn(entry) for every entry of every bin outside the three maxima, in bin order then insertion order (e.g. :2694-2707); an
    // entry that sits in the histogram twice is handed over twice
    template <class Fn> void cull(Fn fn) const {
        int ind[3];
        maxima(ind);
        for (int b = 0; b < ORBM_HISTO_LENGTH; ++b)
            if (b != ind[0] && b != ind[1] && b != ind[2])
                for (int e : bins[b]) fn(e);
    }
};

// The queries of one window pass: centre, radius (r < 0: no window), level band [lo, hi] (hi < 0: no upper bound), the stereo gate's
// expected uright and tolerance (both may be NULL; er < 0: no gate) and the descriptors.
struct WindowQuery { int nq; const float *x, *y, *r; const int32_t *lo, *hi; const float *ur, *er; const uint8_t* desc; };

// the three tables a search computes per query
struct WindowTables {
    std::vector<float> r; std::vector<int32_t> lo, hi;
    explicit WindowTables(int nq) : r(nq), lo(nq), hi(nq) {}
    void skip(int i) { r[i] = -1.f; lo[i] = 0; hi[i] = -1; }                // a query that is not searched: an empty window
    void set(int i, float radius, int l, int h) { r[i] = radius; lo[i] = l; hi[i] = h; }
    WindowQuery query(const float* x, const float* y, const float* ur, const float* er, const uint8_t* desc) const {
        return WindowQuery{(int)r.size(), x, y, r.data(), lo.data(), hi.data(), ur, er, desc};
    }
};

// runs k_window for q.nq windows against frame f; candidate lists come back in host vectors
int window_pass(orbm* m, const orbm_frame_t* f, const WindowQuery& q, int& cap, std::vector<int>& cnt, std::vector<int>& idx, std::vector<int>& dist,
                bool retry = false, const orbm_dframe* df = nullptr) {
    // `cap` in: capacity of a window on the device; out: row stride of idx / dist (= the longest candidate list, >= 1)
    const int nq = q.nq;
    cnt.assign(nq, 0);
    if (nq == 0 || f->n == 0) return ORBM_OK;
    if (const char* e = retry ? nullptr : ab_env("ORBM_WINDOW_CAP")) cap = std::max(1, std::min(cap, atoi(e)));   // test knob: a small first capacity forces the retry below
    MHIPCHK(hipSetDevice(m->device));
    DevBuf dk, dd, du, dgs, dgi, dqx, dqy, dqr, dmin, dmax, dqu, dqe, dqd, dcnt, didx, ddist, dovf, dpack;
    arena_reset(m);
    if (!df) {                                                  // host frame: it travels with every call (a resident frame does not)
        UP(dk, f->kps, sizeof(KpIn) * f->n); UP(dd, f->desc, (size_t)32 * f->n);
        if (f->uright) UP(du, f->uright, sizeof(float) * f->n);
        UP(dgs, f->grid_start, sizeof(int) * (ORBM_GRID_COLS * ORBM_GRID_ROWS + 1));
        UP(dgi, f->grid_idx, sizeof(int) * f->n);
    }
    UP(dqx, q.x, sizeof(float) * nq); UP(dqy, q.y, sizeof(float) * nq); UP(dqr, q.r, sizeof(float) * nq);
    UP(dmin, q.lo, sizeof(int) * nq); UP(dmax, q.hi, sizeof(int) * nq);
    if (q.ur) UP(dqu, q.ur, sizeof(float) * nq);
    if (q.er) UP(dqe, q.er, sizeof(float) * nq);
    UP(dqd, q.desc, (size_t)32 * nq);
    AL(dcnt, sizeof(int) * nq); AL(dovf, sizeof(int));
    AL_BIG(didx, sizeof(int) * (size_t)nq * cap); AL_BIG(ddist, sizeof(int) * (size_t)nq * cap);   // [nq][cap]: only the used columns come back
    AL_BIG(dpack, 2 * sizeof(int) * (size_t)nq * cap);       // packed copy of the used columns (reserved now: the arena must not grow after the launch)
    MHIPCHK(hipMemsetAsync(dovf.ptr(), 0, sizeof(int), m->stream));
    MHIPCHK(rec_time(m, m->e0));
    ARENA_FLUSH(m);
    hipLaunchKernelGGL(k_window, dim3((nq + 3) / 4), dim3(256), 0, m->stream, df ? df->dKps : dk.as<KpIn>(), df ? df->dDesc : dd.as<uint8_t>(),
                       df ? (f->uright ? df->dUr : nullptr) : (f->uright ? du.as<float>() : nullptr), df ? df->dGs : dgs.as<int>(), df ? df->dGi : dgi.as<int>(),
                       f->min_x, f->min_y, f->inv_w, f->inv_h,
                       nq, dqx.as<float>(), dqy.as<float>(), dqr.as<float>(), dmin.as<int>(), dmax.as<int>(),
                       q.ur ? dqu.as<float>() : nullptr, q.er ? dqe.as<float>() : nullptr, dqd.as<uint8_t>(), cap,
                       dcnt.as<int>(), didx.as<int>(), ddist.as<int>(), dovf.as<int>());
    MHIPCHK(rec_time(m, m->e1));
    m->timed = true;
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    int ovf = 0;
    memcpy(&ovf, dovf.host(), sizeof(int));
    memcpy(cnt.data(), dcnt.host(), sizeof(int) * nq);
    const int devCap = cap;
    int maxc = 0;
    for (int i = 0; i < nq; ++i) maxc = std::max(maxc, std::min(cnt[i], devCap));
    const size_t pn = (size_t)nq * std::max(maxc, 1);
    idx.resize(pn); dist.resize(pn);
    if (maxc > 0) {                                         // pack the used columns on the device: one contiguous copy, stride maxc
        hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((pn + 255) / 256)), dim3(256), 0, m->stream, didx.as<int>(), ddist.as<int>(), nq, devCap, maxc,
                           dpack.as<int>(), dpack.as<int>() + pn);
        MHIPCHK(hipGetLastError());
        MHIPCHK(hipMemcpyAsync(m->arPin + dpack.off, m->arDev + dpack.off, 2 * sizeof(int) * pn, hipMemcpyDeviceToHost, m->stream));
        MHIPCHK(hipStreamSynchronize(m->stream));
        memcpy(idx.data(), dpack.host(), sizeof(int) * pn);
        memcpy(dist.data(), (const int*)dpack.host() + pn, sizeof(int) * pn);
    }
    if (ovf) {
        // Frame::GetFeaturesInArea is unbounded (Frame.cc:784-871): a window that holds more than the default capacity (dense
        // frames, the 100-px initialisation window) is simply run again with room for every keypoint of the frame
        if (devCap < f->n) {
            cap = f->n;
            return window_pass(m, f, q, cap, cnt, idx, dist, true, df);
        }
        set_merr("a search window returned more than %d candidates", devCap);
        return ORBM_E_CAPACITY;
    }
    // Everything below indexes host arrays with what the device reported: counts beyond the row stride or keypoint indices
    // beyond the frame must stop here, not in a caller's replay loop (round 2's ORBM_WINDOW_CAP=4 run died in such a loop,
    // profiles/NOTES.md "18:59 segfault").
    for (int i = 0; i < nq; ++i)
        if (cnt[i] < 0 || cnt[i] > devCap) { set_merr("window %d reports %d candidates for a capacity of %d without the overflow flag", i, cnt[i], devCap); return ORBM_E_HIP; }
    for (int i = 0; i < nq; ++i)
        for (int c = 0; c < cnt[i]; ++c)
            if ((unsigned)idx[(size_t)i * maxc + c] >= (unsigned)f->n) { set_merr("window %d candidate %d: keypoint index %d outside the frame (%d keypoints)", i, c, idx[(size_t)i * maxc + c], f->n); return ORBM_E_HIP; }
    cap = std::max(maxc, 1);
    return ORBM_OK;
}

// k_window_topk against a resident frame: per window the candidate count and the WT_K smallest (distance, position) keys.
// One upload of the queries, one kernel, one download.
int window_topk_pass(orbm* m, const orbm_dframe* df, bool stereo_gate, const WindowQuery& q, const int** cnt, const unsigned int** keys) {
    // results stay in the arena's pinned mirror (valid until the handle's next call): *cnt [nq], *keys [nq][WT_K]
    *cnt = nullptr; *keys = nullptr;
    const int nq = q.nq;
    if (nq == 0 || df->n == 0) return ORBM_OK;
    MHIPCHK(hipSetDevice(m->device));
    DevBuf dqx, dqy, dqr, dmin, dmax, dqu, dqe, dqd, dcnt, dkeys;
    arena_reset(m);
    UP(dqx, q.x, sizeof(float) * nq); UP(dqy, q.y, sizeof(float) * nq); UP(dqr, q.r, sizeof(float) * nq);
    UP(dmin, q.lo, sizeof(int) * nq); UP(dmax, q.hi, sizeof(int) * nq);
    if (q.ur) UP(dqu, q.ur, sizeof(float) * nq);
    if (q.er) UP(dqe, q.er, sizeof(float) * nq);
    UP(dqd, q.desc, (size_t)32 * nq);
    AL(dcnt, sizeof(int) * nq); AL(dkeys, sizeof(unsigned int) * (size_t)nq * WT_K);
    static const bool prof = getenv("ORBM_PROFILE") != nullptr;
    static const bool copies = ab_env("ORBM_TOPK_COPIES") != nullptr;     // A/B: staged copies instead of zero-copy
    auto T = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = prof ? T() : 0;
    if (prof) MHIPCHK(rec_time(m, m->e0));                       // a latency path: no event records unless someone is looking
    // Zero-copy: the queries sit in the arena's pinned host mirror, which the GPU can address; the kernel reads them over PCIe
    // and writes counts and keys straight back into it.  ~110 KB in all: two copy commands would cost more in latency (~10 us
    // each) than the link takes to move the bytes, and this is a latency path (Tracking waits for the result).
    auto hp = [&](DevBuf& b) { return (void*)(m->arPin + b.off); };
    if (copies) ARENA_FLUSH(m);
#define QP(buf, T_) (copies ? (buf).as<T_>() : (T_*)hp(buf))
    hipLaunchKernelGGL(k_window_topk, dim3((nq + 3) / 4), dim3(256), 0, m->stream, df->dKps, df->dDesc, stereo_gate ? df->dUr : nullptr, df->dGs, df->dGi,
                       df->min_x, df->min_y, df->inv_w, df->inv_h, nq, QP(dqx, float), QP(dqy, float), QP(dqr, float), QP(dmin, int), QP(dmax, int),
                       q.ur ? QP(dqu, float) : nullptr, q.er ? QP(dqe, float) : nullptr, QP(dqd, uint8_t), QP(dcnt, int), QP(dkeys, unsigned int));
#undef QP
    if (prof) { MHIPCHK(rec_time(m, m->e1)); m->timed = true; }
    MHIPCHK(hipGetLastError());
    if (copies) MHIPCHK(hipMemcpyAsync(m->arPin + m->arOutLo, m->arDev + m->arOutLo, m->arOutHi - m->arOutLo, hipMemcpyDeviceToHost, m->stream));
    const double t1 = prof ? T() : 0;
    MHIPCHK(hipStreamSynchronize(m->stream));
    if (prof) fprintf(stderr, "orbm profile:   enqueue %.1f us, wait %.1f us (%s)\n", t1 - t0, T() - t1, copies ? "staged copies" : "zero-copy");
    *cnt = (const int*)dcnt.host(); *keys = (const unsigned int*)dkeys.host();
    {   // the replays index the frame's arrays with the low 20 bits of every returned key: check them once, branch-free
        const int* c_ = *cnt; const unsigned int* k_ = *keys;
        unsigned bad = 0;
        for (int i = 0; i < nq; ++i) {
            const int nc = std::min(std::max(c_[i], 0), (int)WT_K);
            bad |= (unsigned)(c_[i] < 0);
            for (int c = 0; c < nc; ++c) bad |= (unsigned)((k_[(size_t)i * WT_K + c] & 0xFFFFFu) >= (unsigned)df->n);
        }
        if (bad) { set_merr("top-K window pass returned a keypoint index outside the resident frame (%d keypoints)", df->n); *cnt = nullptr; *keys = nullptr; return ORBM_E_HIP; }
    }
    return ORBM_OK;
}

// merge-join of two FeatureVector CSRs (ORBmatcher.cc:343-518 / 1448-1595) -> jobs + GPU distances
struct JoinJobs { std::vector<int> q, l2, len, off, node_b; int total = 0; };

int bucket_pass(orbm* m, const uint8_t* d1, int n1, const uint8_t* d2, int n2, const int32_t* idx2, int nidx2,
                const JoinJobs& J, std::vector<int>& dist) {
    dist.assign(J.total, 0);
    if (J.total == 0) return ORBM_OK;
    MHIPCHK(hipSetDevice(m->device));
    DevBuf b1, b2, bi, bq, bl, bo, bout;
    arena_reset(m);
    UP(b1, d1, (size_t)32 * n1); UP(b2, d2, (size_t)32 * n2); UP(bi, idx2, sizeof(int) * nidx2);
    const int nj = (int)J.q.size();
    UP(bq, J.q.data(), sizeof(int) * nj); UP(bl, J.l2.data(), sizeof(int) * nj); UP(bo, J.off.data(), sizeof(int) * nj);
    AL(bout, sizeof(int) * (size_t)J.total);
    MHIPCHK(rec_time(m, m->e0));
    ARENA_FLUSH(m);
    hipLaunchKernelGGL(k_pairdist, dim3((J.total + 255) / 256), dim3(256), 0, m->stream, b1.as<uint8_t>(), b2.as<uint8_t>(),
                       bi.as<int>(), nj, bq.as<int>(), bl.as<int>(), bo.as<int>(), J.total, bout.as<int>());
    MHIPCHK(rec_time(m, m->e1));
    m->timed = true;
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(dist.data(), bout.host(), sizeof(int) * (size_t)J.total);
    return ORBM_OK;
}

void join_nodes(int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1, int nn2, const int32_t* nodes2,
                const int32_t* start2, JoinJobs& J) {
    int a = 0, b = 0;                                                       // lower_bound jumps == this linear merge on sorted keys
    while (a < nn1 && b < nn2) {
        if (nodes1[a] == nodes2[b]) {
            const int len = start2[b + 1] - start2[b];
            for (int i = start1[a]; i < start1[a + 1]; ++i) {
                J.q.push_back(idx1[i]); J.l2.push_back(start2[b]); J.len.push_back(len); J.off.push_back(J.total); J.node_b.push_back(b);
                J.total += len;
            }
            ++a; ++b;
        } else if (nodes1[a] < nodes2[b]) ++a; else ++b;
    }
}

// The jobs of a BoW search as its replay walks them, in the reference's (node, side-1 feature) order: job j is side-1 feature
// query(j) against the count(j) side-2 features of the common node, index(j, c) at distance(j, c).
struct BucketJobs {
    JoinJobs J; std::vector<int> dist; const int32_t* idx2 = nullptr;
    size_t size() const { return J.q.size(); }
    int query(size_t j) const { return J.q[j]; }
    int count(size_t j) const { return J.len[j]; }
    int index(size_t j, int c) const { return idx2[J.l2[j] + c]; }
    int distance(size_t j, int c) const { return dist[J.off[j] + c]; }
};

// prologue of M7 / M7-fisheye / M8 / M10: join the two FeatureVectors, one distance pass over every job, `out` reset to -1
int bucket_jobs(orbm* m, const uint8_t* desc1, int n1, int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                const uint8_t* desc2, int n2, int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                int32_t* out, int nout, BucketJobs& B) {
    join_nodes(nn1, nodes1, start1, idx1, nn2, nodes2, start2, B.J);
    B.idx2 = idx2;
    const int rc = bucket_pass(m, desc1, n1, desc2, n2, idx2, start2[nn2], B.J, B.dist);
    if (rc) return rc;
    for (int i = 0; i < nout; ++i) out[i] = -1;
    return ORBM_OK;
}

// Candidate lists as the claim replays see them: either the full [queries][stride] lists of window_pass (window_lists, which
// owns them), or the K best (distance, position) keys of window_topk_pass, which are a prefix of the list in exactly the order
// that matters to a `dist < bestDist` scan (see k_window_topk).  trunc(i): the list of query i was cut.
struct CandLists {
    std::vector<int> ownCnt, ownIdx, ownDist;                           // storage of the full lists
    const int* cnt = nullptr; const int* idx = nullptr; const int* dist = nullptr; int stride = 0;
    const unsigned int* keys = nullptr;                                 // dist << 20 | keypoint index, in (distance, visiting order) rank
    CandLists() = default;
    CandLists(const CandLists&) = delete;                               // cnt / idx / dist point into the own vectors
    int count(int i) const { return keys ? std::min(cnt[i], (int)WT_K) : std::min(cnt[i], stride); }   // (never beyond a row: window_pass has checked)
    bool trunc(int i) const { return keys && cnt[i] > WT_K; }
    int index(int i, int c) const { return keys ? (int)(keys[(size_t)i * WT_K + c] & 0xFFFFFu) : idx[(size_t)i * stride + c]; }
    int distance(int i, int c) const { return keys ? (int)(keys[(size_t)i * WT_K + c] >> 20) : dist[(size_t)i * stride + c]; }
};

// Full candidate lists of q's windows in `frame` (df: its resident twin, or NULL).  A search without a stereo gate sweeps a copy
// of the frame without uright.  first_cap: the window capacity of the first attempt (window_pass runs again with room for the
// whole frame when one overflows); the row stride of the lists is whatever the pass packed them to.
int window_lists(orbm* m, const orbm_frame_t* frame, bool stereo_gate, const WindowQuery& q, int first_cap, CandLists& out, const orbm_dframe* df = nullptr) {
    orbm_frame_t f = *frame;
    if (!stereo_gate) f.uright = nullptr;
    int cap = std::max(1, std::min(f.n, first_cap));
    const int rc = window_pass(m, &f, q, cap, out.ownCnt, out.ownIdx, out.ownDist, false, df);
    if (rc) return rc;
    out.cnt = out.ownCnt.data(); out.idx = out.ownIdx.data(); out.dist = out.ownDist.data(); out.stride = cap; out.keys = nullptr;
    return ORBM_OK;
}

// first minimum over the candidates of query i that `blocked` does not exclude: (bestDist, bestIdx), (256, -1) without one
std::pair<int, int> best_unblocked(const CandLists& L, int i, const uint8_t* blocked) {
    int bestDist = 256, bestIdx = -1;
    for (int c = 0, nc = L.count(i); c < nc; ++c) {
        const int k = L.index(i, c);
        if (blocked[k]) continue;
        const int d = L.distance(i, c);
        if (d < bestDist) { bestDist = d; bestIdx = k; }
    }
    return {bestDist, bestIdx};
}

// best and second-best distance over the unblocked candidates of query i, with their pyramid levels (ORBmatcher.cc:119-141);
// seen: how many candidates were unblocked
struct BestTwo { int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1, seen = 0; };
BestTwo best_two_levels(const CandLists& L, int i, const uint8_t* blocked, const orbm_kp_t* kps) {
    BestTwo b;
    for (int c = 0, nc = L.count(i); c < nc; ++c) {
        const int k = L.index(i, c);
        if (blocked[k]) continue;
        ++b.seen;
        const int d = L.distance(i, c);
        if (d < b.bestDist) { b.bestDist2 = b.bestDist; b.bestDist = d; b.bestLevel2 = b.bestLevel; b.bestLevel = kps[k].octave; b.bestIdx = k; }
        else if (d < b.bestDist2) { b.bestLevel2 = kps[k].octave; b.bestDist2 = d; }
    }
    return b;
}

// Driver of the resident M3 / M4: replay the WT_K best keys of every window; where a cut list ran out of candidates the replay
// returns false and runs again over the full lists.  Without a resident frame the full lists at once.  replay(lists) fills
// match and nmatches; an empty pass (no query, no keypoint) leaves match at -1 and returns 0.
template <class Replay>
int search_lists(orbm* m, const orbm_frame_t* f, const orbm_dframe* df, const WindowQuery& q, bool profile, int32_t* match, const int& nmatches, Replay replay) {
    if (df) {
        static const bool env = getenv("ORBM_PROFILE") != nullptr;
        const bool prof = env && profile;
        auto T = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t0 = prof ? T() : 0;
        CandLists Lk;
        const int rc = window_topk_pass(m, df, f->uright != nullptr, q, &Lk.cnt, &Lk.keys);
        if (rc) return rc;
        const double t1 = prof ? T() : 0;
        if (!Lk.cnt) for (int i = 0; i < f->n; ++i) match[i] = -1;
        const bool done = !Lk.cnt || replay(Lk);
        if (prof) fprintf(stderr, "orbm profile: top-K pass %.1f us, replay %.1f us%s\n", t1 - t0, T() - t1, done ? "" : " (fallback)");
        if (done) return Lk.cnt ? nmatches : 0;
    }
    CandLists Lf;
    const int rc = window_lists(m, f, true, q, 2048, Lf, df);
    if (rc) return rc;
    replay(Lf);
    return nmatches;
}

}  // namespace

extern "C" {

int orbm_grid_build(orbm_t* m, const orbm_kp_t* kps, int n, float min_x, float min_y, float inv_w, float inv_h,
                    int32_t* grid_start, int32_t* grid_idx) {
    if (!m || !grid_start || !grid_idx || n < 0 || (n > 0 && !kps)) return ORBM_E_INVALID;
    if (n > 65535) { set_merr("grid build supports at most 65535 keypoints"); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    int n2 = 64; while (n2 < n) n2 <<= 1;
    DevBuf dk, dgs, dgi, dpl;
    arena_reset(m);
    UP(dk, kps, sizeof(KpIn) * n);
    AL(dgs, sizeof(int) * (ORBM_GRID_COLS * ORBM_GRID_ROWS + 1)); AL(dgi, sizeof(int) * (n + 1)); AL(dpl, sizeof(int));
    ARENA_FLUSH(m);
    if (n <= GRID_CS_MAX)
        hipLaunchKernelGGL(k_grid_build_cs, dim3(1), dim3(256), grid_cs_lds(n), m->stream, dk.as<KpIn>(), n, min_x, min_y, inv_w, inv_h,
                           dgs.as<int>(), dgi.as<int>(), dpl.as<int>());
    else if (n > GRID_WIDE_MIN) {
        MHIPCHK(grid_wide_attr((const void*)k_grid_build_wide));
        hipLaunchKernelGGL(k_grid_build_wide, dim3(1), dim3(256), grid_cs_lds(n), m->stream, dk.as<KpIn>(), n, min_x, min_y, inv_w, inv_h,
                           dgs.as<int>(), dgi.as<int>(), dpl.as<int>());
    } else {
        MHIPCHK(hipFuncSetAttribute((const void*)k_grid_build, hipFuncAttributeMaxDynamicSharedMemorySize, n2 * 4));
        hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(256), (size_t)n2 * 4, m->stream, dk.as<KpIn>(), n, n2, min_x, min_y, inv_w, inv_h,
                           dgs.as<int>(), dgi.as<int>(), dpl.as<int>());
    }
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    int placed = 0;
    memcpy(&placed, dpl.host(), sizeof(int));
    memcpy(grid_start, dgs.host(), sizeof(int) * (ORBM_GRID_COLS * ORBM_GRID_ROWS + 1));
    if (placed) memcpy(grid_idx, dgi.host(), sizeof(int) * placed);
    return placed;
}

int orbm_window_candidates(orbm_t* m, const orbm_frame_t* f, int nq, const float* qx, const float* qy, const float* qr,
                           const int32_t* min_level, const int32_t* max_level, const float* q_ur, const float* q_er_max,
                           const uint8_t* qdesc, int cap, int32_t* out_cnt, int32_t* out_idx, int32_t* out_dist) {
    if (!m || !f || nq < 0 || cap < 1) return ORBM_E_INVALID;
    std::vector<int> cnt, idx, dist;
    int stride = cap;                                        // in: window capacity; out: row stride of the packed lists
    int rc = window_pass(m, f, WindowQuery{nq, qx, qy, qr, min_level, max_level, q_ur, q_er_max, qdesc}, stride, cnt, idx, dist);
    if (rc && rc != ORBM_E_CAPACITY) return rc;
    for (int i = 0; i < nq; ++i) {
        out_cnt[i] = cnt[i];
        const int c = std::min(cnt[i], cap);
        if (c > 0 && !idx.empty()) {
            memcpy(out_idx + (size_t)i * cap, &idx[(size_t)i * stride], sizeof(int) * c);
            memcpy(out_dist + (size_t)i * cap, &dist[(size_t)i * stride], sizeof(int) * c);
        }
    }
    return rc;
}

// M4 body.  cur: the frame's view (host arrays, or the resident frame's host-side copy of what the replay reads); df: resident frame or NULL
static int search_by_projection_frame_impl(orbm_t* m, const orbm_frame_t* cur, const orbm_dframe* df, const uint8_t* cur_blocked, const float* sf,
                                           int nq, const uint8_t* valid, const float* u, const float* v, const float* invzc,
                                           const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                           float th, int bForward, int bBackward, float mbf, int check_ori, int32_t* match) {
    // windows exactly as ORBmatcher.cc:2543-2549; invalid queries get an empty window (r < 0)
    WindowTables W(nq);
    std::vector<float> qur(nq), qer(nq);
    for (int i = 0; i < nq; ++i) {
        if (!valid[i]) { W.skip(i); qur[i] = 0; qer[i] = -1.f; continue; }
        const int o = octave[i];
        const float radius = th * sf[o];
        if (bForward) W.set(i, radius, o, -1);
        else if (bBackward) W.set(i, radius, 0, o);
        else W.set(i, radius, o - 1, o + 1);
        qur[i] = u[i] - mbf * invzc[i];                                    // :2571
        qer[i] = cur->uright ? radius : -1.f;
    }
    // sequential replay of the claims (ORBmatcher.cc:2553-2612); false = a cut list ran out of unblocked candidates
    int nmatches = 0;
    auto replay = [&](const CandLists& Lc) -> bool {
        nmatches = 0;
        RotHist rh;
        const float factor = ORBM_HISTO_LENGTH / 360.0f;
        std::vector<uint8_t> blocked(cur_blocked, cur_blocked + cur->n);
        for (int i = 0; i < cur->n; ++i) match[i] = -1;
        for (int i = 0; i < nq; ++i) {
            const int nc = valid[i] ? Lc.count(i) : 0;
            if (nc == 0) continue;
            const auto [bestDist, bestIdx2] = best_unblocked(Lc, i, blocked.data());
            if (bestIdx2 < 0 && Lc.trunc(i)) return false;
            if (bestDist <= ORBM_TH_HIGH) {
                match[bestIdx2] = i;
                if (mp_obs[i]) blocked[bestIdx2] = 1;
                nmatches++;
                if (check_ori) rh.add(angle[i], cur->kps[bestIdx2].angle, factor, bestIdx2);
            }
        }
        if (check_ori) rh.cull([&](int k) { match[k] = ORBM_MATCH_PRUNED; nmatches--; });
        return true;
    };
    return search_lists(m, cur, df, W.query(u, v, qur.data(), qer.data(), qdesc), true, match, nmatches, replay);
}

int orbm_search_by_projection_frame(orbm_t* m, const orbm_frame_t* cur, const uint8_t* cur_blocked, const float* sf,
                                    int nq, const uint8_t* valid, const float* u, const float* v, const float* invzc,
                                    const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                    float th, int bForward, int bBackward, float mbf, int check_ori, int32_t* match) {
    if (!m || !cur || nq < 0) return ORBM_E_INVALID;
    return search_by_projection_frame_impl(m, cur, nullptr, cur_blocked, sf, nq, valid, u, v, invzc, octave, angle, qdesc, mp_obs, th, bForward, bBackward, mbf,
                                           check_ori, match);
}

static int search_by_projection_points_impl(orbm_t* m, const orbm_frame_t* f, const orbm_dframe* df, const uint8_t* blocked_in, const float* sf,
                                            int nq, const uint8_t* in_view, const float* px, const float* py, const float* pxr,
                                            const float* view_cos, const int32_t* level, const uint8_t* qdesc, const uint8_t* mp_obs,
                                            float th, float nnratio, int32_t* match) {
    const bool bFactor = th != 1.0;
    WindowTables W(nq);
    std::vector<float> qer(nq);
    for (int i = 0; i < nq; ++i) {
        if (!in_view[i]) { W.skip(i); qer[i] = -1.f; continue; }
        float r = view_cos[i] > 0.998 ? 2.5f : 4.0f;                       // RadiusByViewingCos (:242-249)
        if (bFactor) r *= th;
        W.set(i, r * sf[level[i]], level[i] - 1, level[i]);
        qer[i] = f->uright ? r * sf[level[i]] : -1.f;                      // :107-117
    }
    // replay of ORBmatcher.cc:119-166; false = a cut list held fewer than two unblocked candidates
    int nmatches = 0;
    auto replay = [&](const CandLists& Lc) -> bool {
        nmatches = 0;
        std::vector<uint8_t> blocked(blocked_in, blocked_in + f->n);
        for (int i = 0; i < f->n; ++i) match[i] = -1;
        for (int iMP = 0; iMP < nq; ++iMP) {
            const int nc = in_view[iMP] ? Lc.count(iMP) : 0;
            if (nc == 0) continue;
            const BestTwo b = best_two_levels(Lc, iMP, blocked.data(), f->kps);
            if (b.seen < 2 && Lc.trunc(iMP)) return false;                  // best AND second must come from the unblocked candidates
            if (b.bestDist <= ORBM_TH_HIGH) {
                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;
                if (b.bestLevel != b.bestLevel2 || b.bestDist <= nnratio * b.bestDist2) {
                    match[b.bestIdx] = iMP;
                    if (mp_obs[iMP]) blocked[b.bestIdx] = 1;
                    nmatches++;
                }
            }
        }
        return true;
    };
    return search_lists(m, f, df, W.query(px, py, pxr, qer.data(), qdesc), false, match, nmatches, replay);
}

int orbm_search_by_projection_points(orbm_t* m, const orbm_frame_t* f, const uint8_t* blocked_in, const float* sf,
                                     int nq, const uint8_t* in_view, const float* px, const float* py, const float* pxr,
                                     const float* view_cos, const int32_t* level, const uint8_t* qdesc, const uint8_t* mp_obs,
                                     float th, float nnratio, int32_t* match) {
    if (!m || !f || nq < 0) return ORBM_E_INVALID;
    return search_by_projection_points_impl(m, f, nullptr, blocked_in, sf, nq, in_view, px, py, pxr, view_cos, level, qdesc, mp_obs, th, nnratio, match);
}

// ---- frames resident in HBM: what Tracking's 2-4 searches per frame work on (Tracking.cc:3002-3211, 3867-3891) ----
void orbm_frame_destroy(orbm_dframe_t* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->block) (void)hipFree(f->block);
    delete f;
}

int orbm_frame_create(orbm_t* m, int space, int n, const orbm_kp_t* kps, const uint8_t* desc, const float* uright,
                      float min_x, float min_y, float inv_w, float inv_h, orbm_dframe_t** out) {
    if (!m || !out || n < 0 || (n > 0 && (!kps || !desc))) return ORBM_E_INVALID;
    *out = nullptr;
    if (n > 65535) { set_merr("a resident frame holds at most 65535 keypoints"); return ORBM_E_CAPACITY; }
    int n2 = 64; while (n2 < n) n2 <<= 1;
    MHIPCHK(hipSetDevice(m->device));
    orbm_dframe* f = new orbm_dframe;
    f->device = m->device; f->n = n; f->min_x = min_x; f->min_y = min_y; f->inv_w = inv_w; f->inv_h = inv_h;
    const size_t ncells = ORBM_GRID_COLS * ORBM_GRID_ROWS + 1;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t bKps = space == ORBM_HOST ? al(sizeof(KpIn) * (size_t)std::max(n, 1)) : 0, bDesc = space == ORBM_HOST ? al((size_t)32 * std::max(n, 1)) : 0,
                 bUr = space == ORBM_HOST && uright ? al(sizeof(float) * (size_t)std::max(n, 1)) : 0, bGs = al(sizeof(int) * ncells), bGi = al(sizeof(int) * (size_t)(n + 1)) + 256;
    if (hipMalloc((void**)&f->block, bKps + bDesc + bUr + bGs + bGi) != hipSuccess) { set_merr("hipMalloc failed"); delete f; return ORBM_E_HIP; }
    uint8_t* p = f->block;
    f->hkps.resize(std::max(n, 1));
    hipError_t e = hipSuccess;
    if (space == ORBM_HOST) {
        f->dKps = (const KpIn*)p; p += bKps; f->dDesc = p; p += bDesc;
        if (uright) { f->dUr = (const float*)p; p += bUr; }
        if (n > 0) {
            memcpy(f->hkps.data(), kps, sizeof(orbm_kp_t) * n);
            e = hipMemcpyAsync((void*)f->dKps, kps, sizeof(KpIn) * n, hipMemcpyHostToDevice, m->stream);
            if (e == hipSuccess) e = hipMemcpyAsync((void*)f->dDesc, desc, (size_t)32 * n, hipMemcpyHostToDevice, m->stream);
            if (e == hipSuccess && uright) e = hipMemcpyAsync((void*)f->dUr, uright, sizeof(float) * n, hipMemcpyHostToDevice, m->stream);
        }
    } else {                                                     // adopt the caller's device arrays (an extractor's result block): no copy of them
        f->dKps = (const KpIn*)kps; f->dDesc = desc; f->dUr = uright;
        if (n > 0) e = hipMemcpyAsync(f->hkps.data(), kps, sizeof(orbm_kp_t) * n, hipMemcpyDeviceToHost, m->stream);
    }
    f->dGs = (int*)p; p += bGs; f->dGi = (int*)p;
    int* dPlaced = f->dGi + (n + 1);
    if (e == hipSuccess && n > 0) {
        if (n <= GRID_CS_MAX)
            hipLaunchKernelGGL(k_grid_build_cs, dim3(1), dim3(256), grid_cs_lds(n), m->stream, f->dKps, n, min_x, min_y, inv_w, inv_h, f->dGs, f->dGi, dPlaced);
        else if (n > GRID_WIDE_MIN) {
            e = grid_wide_attr((const void*)k_grid_build_wide);
            if (e == hipSuccess) hipLaunchKernelGGL(k_grid_build_wide, dim3(1), dim3(256), grid_cs_lds(n), m->stream, f->dKps, n, min_x, min_y, inv_w, inv_h, f->dGs, f->dGi, dPlaced);
        } else {
            if (n2 * 4 > 48 * 1024) e = hipFuncSetAttribute((const void*)k_grid_build, hipFuncAttributeMaxDynamicSharedMemorySize, n2 * 4);
            if (e == hipSuccess) hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(256), (size_t)n2 * 4, m->stream, f->dKps, n, n2, min_x, min_y, inv_w, inv_h, f->dGs, f->dGi, dPlaced);
        }
        if (e == hipSuccess) e = hipGetLastError();
    } else if (e == hipSuccess) e = hipMemsetAsync(f->dGs, 0, sizeof(int) * ncells, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) { set_merr("resident frame setup failed: %s", hipGetErrorString(e)); orbm_frame_destroy(f); return ORBM_E_HIP; }
    *out = f;
    return ORBM_OK;
}

int orbm_frame_size(const orbm_dframe_t* f) { return f ? f->n : ORBM_E_INVALID; }

static orbm_frame_t resident_view(const orbm_dframe* f, bool stereo_gate) {
    orbm_frame_t v;
    v.n = f->n; v.kps = f->hkps.data(); v.desc = nullptr; v.uright = stereo_gate && f->dUr ? (const float*)f->hkps.data() /* non-NULL marker: only tested, never read */ : nullptr;
    v.min_x = f->min_x; v.min_y = f->min_y; v.inv_w = f->inv_w; v.inv_h = f->inv_h; v.grid_start = nullptr; v.grid_idx = nullptr;
    return v;
}

int orbm_search_by_projection_frame_resident(orbm_t* m, const orbm_dframe_t* cur, const uint8_t* cur_blocked, const float* sf,
                                             int nq, const uint8_t* valid, const float* u, const float* v, const float* invzc,
                                             const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                             float th, int bForward, int bBackward, float mbf, int check_ori, int32_t* match) {
    if (!m || !cur || nq < 0 || cur->device != m->device) return ORBM_E_INVALID;
    const orbm_frame_t view = resident_view(cur, true);
    return search_by_projection_frame_impl(m, &view, cur, cur_blocked, sf, nq, valid, u, v, invzc, octave, angle, qdesc, mp_obs, th, bForward, bBackward, mbf,
                                           check_ori, match);
}

int orbm_search_by_projection_points_resident(orbm_t* m, const orbm_dframe_t* f, const uint8_t* blocked_in, const float* sf,
                                              int nq, const uint8_t* in_view, const float* px, const float* py, const float* pxr,
                                              const float* view_cos, const int32_t* level, const uint8_t* qdesc, const uint8_t* mp_obs,
                                              float th, float nnratio, int32_t* match) {
    if (!m || !f || nq < 0 || f->device != m->device) return ORBM_E_INVALID;
    const orbm_frame_t view = resident_view(f, true);
    return search_by_projection_points_impl(m, &view, f, blocked_in, sf, nq, in_view, px, py, pxr, view_cos, level, qdesc, mp_obs, th, nnratio, match);
}

int orbm_search_for_initialization(orbm_t* m, const orbm_frame_t* F1, const orbm_frame_t* F2, float* prev, int windowSize,
                                   float nnratio, int check_ori, int32_t* vnMatches12) {
    if (!m || !F1 || !F2) return ORBM_E_INVALID;
    const int n1 = F1->n;
    std::vector<float> qx(n1), qy(n1);
    WindowTables W(n1);
    for (int i = 0; i < n1; ++i) {
        const int l1 = F1->kps[i].octave;
        qx[i] = prev[2 * i]; qy[i] = prev[2 * i + 1];
        if (l1 > 0) W.skip(i);                                             // :825
        else W.set(i, (float)windowSize, l1, l1);
    }
    CandLists L;
    int rc = window_lists(m, F2, false, W.query(qx.data(), qy.data(), nullptr, nullptr, F1->desc), 4096, L);   // (the 100-px window is dense)
    if (rc) return rc;
    int nmatches = 0;
    for (int i = 0; i < n1; ++i) vnMatches12[i] = -1;
    RotHist rh;
    const float factor = ORBM_HISTO_LENGTH / 360.0f;
    std::vector<int> vMatchedDistance(F2->n, INT_MAX), vnMatches21(F2->n, -1);
    for (int i1 = 0; i1 < n1; ++i1) {
        if (F1->kps[i1].octave > 0 || L.count(i1) == 0) continue;
        int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
        for (int c = 0, nc = L.count(i1); c < nc; ++c) {
            const int i2 = L.index(i1, c), d = L.distance(i1, c);
            if (vMatchedDistance[i2] <= d) continue;
            if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestIdx2 = i2; }
            else if (d < bestDist2) bestDist2 = d;
        }
        if (bestDist <= ORBM_TH_LOW && bestDist < (float)bestDist2 * nnratio) {
            if (vnMatches21[bestIdx2] >= 0) { vnMatches12[vnMatches21[bestIdx2]] = -1; nmatches--; }
            vnMatches12[i1] = bestIdx2; vnMatches21[bestIdx2] = i1; vMatchedDistance[bestIdx2] = bestDist;
            nmatches++;
            if (check_ori) rh.add(F1->kps[i1].angle, F2->kps[bestIdx2].angle, factor, i1);
        }
    }
    if (check_ori) rh.cull([&](int i1) { if (vnMatches12[i1] >= 0) { vnMatches12[i1] = -1; nmatches--; } });   // only entries still matched (:926)
    for (int i1 = 0; i1 < n1; ++i1)
        if (vnMatches12[i1] >= 0) { prev[2 * i1] = F2->kps[vnMatches12[i1]].x; prev[2 * i1 + 1] = F2->kps[vnMatches12[i1]].y; }
    return nmatches;
}

static int triangulation_impl(orbm_t* m, bool legacy, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* has_mp1, const float* uright1,
                                  int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                                  int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* has_mp2, const float* uright2,
                                  int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                                  const float* F12, float epx, float epy, const float* sf2, const float* sigma2_2,
                                  int bOnlyStereo, int bCoarse, int check_ori, int32_t* vMatches12,
                                  orbm_pair_gate_fn gate = nullptr, void* gate_user = nullptr) {
    if (!m || n1 < 0 || n2 < 0) return ORBM_E_INVALID;
    std::vector<uint8_t> vbMatched2(n2, 0);                                 // only maintained by the legacy overload (:1319)
    BucketJobs B;
    int rc = bucket_jobs(m, desc1, n1, nn1, nodes1, start1, idx1, desc2, n2, nn2, nodes2, start2, idx2, vMatches12, n1, B);
    if (rc) return rc;
    int nmatches = 0;
    RotHist rh;
    const float factor = legacy ? ORBM_HISTO_LENGTH / 360.0f : 1.0f / ORBM_HISTO_LENGTH;   // :1166 vs :1441 (sic)
    for (size_t j = 0; j < B.size(); ++j) {
        const int i1 = B.query(j);
        if (has_mp1[i1]) continue;
        const bool bStereo1 = uright1 && uright1[i1] >= 0;
        if (bOnlyStereo && !bStereo1) continue;
        const orbm_kp_t& kp1 = kps1[i1];
        int bestDist = ORBM_TH_LOW, bestIdx2 = -1;
        for (int c = 0; c < B.count(j); ++c) {
            const int i2 = B.index(j, c);
            if (vbMatched2[i2] || has_mp2[i2]) continue;
            const bool bStereo2 = uright2 && uright2[i2] >= 0;
            if (bOnlyStereo && !bStereo2) continue;
            const int d = B.distance(j, c);
            if (d > ORBM_TH_LOW || d > bestDist) continue;
            const orbm_kp_t& kp2 = kps2[i2];
            if (!bStereo1 && !bStereo2 && sf2) {                            // sf2 == NULL: pKF1->mpCamera2 set (:1517) / M12, which has no such gate
                const float distex = epx - kp2.x, distey = epy - kp2.y;
                if (distex * distex + distey * distey < 100 * sf2[kp2.octave]) continue;
            }
            bool epi = false;
            if (gate) epi = gate(gate_user, i1, i2) != 0;                   // the caller's camera model, called where the reference calls it (:1552 / :1729)
            else {   // Pinhole::epipolarConstrain_ (Pinhole.cpp:281-295)
                const float a = kp1.x * F12[0] + kp1.y * F12[3] + F12[6];
                const float b = kp1.x * F12[1] + kp1.y * F12[4] + F12[7];
                const float c2 = kp1.x * F12[2] + kp1.y * F12[5] + F12[8];
                const float num = a * kp2.x + b * kp2.y + c2;
                const float den = a * a + b * b;
                if (den != 0) { const float dsqr = num * num / den; epi = dsqr < 3.84 * sigma2_2[kp2.octave]; }
            }
            if (epi || bCoarse) { bestIdx2 = i2; bestDist = d; }
        }
        if (bestIdx2 >= 0) {
            vMatches12[i1] = bestIdx2;
            if (legacy) vbMatched2[bestIdx2] = 1;
            nmatches++;
            if (check_ori) rh.add(kp1.angle, kps2[bestIdx2].angle, factor, i1);
        }
    }
    if (check_ori) rh.cull([&](int i) { if (legacy) vbMatched2[vMatches12[i]] = 0; vMatches12[i] = -1; nmatches--; });
    return nmatches;
}

int orbm_search_for_triangulation(orbm_t* m, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* has_mp1, const float* uright1,
                                  int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                                  int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* has_mp2, const float* uright2,
                                  int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                                  const float* F12, float epx, float epy, const float* sf2, const float* sigma2_2,
                                  int bOnlyStereo, int bCoarse, int check_ori, int32_t* vMatches12) {
    return triangulation_impl(m, false, n1, kps1, desc1, has_mp1, uright1, nn1, nodes1, start1, idx1, n2, kps2, desc2, has_mp2, uright2,
                              nn2, nodes2, start2, idx2, F12, epx, epy, sf2, sigma2_2, bOnlyStereo, bCoarse, check_ori, vMatches12);
}

int orbm_search_for_triangulation_legacy(orbm_t* m, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* has_mp1, const float* uright1,
                                  int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                                  int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* has_mp2, const float* uright2,
                                  int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                                  const float* F12, float epx, float epy, const float* sf2, const float* sigma2_2,
                                  int bOnlyStereo, int bCoarse, int check_ori, int32_t* vMatches12) {
    return triangulation_impl(m, true, n1, kps1, desc1, has_mp1, uright1, nn1, nodes1, start1, idx1, n2, kps2, desc2, has_mp2, uright2,
                              nn2, nodes2, start2, idx2, F12, epx, epy, sf2, sigma2_2, bOnlyStereo, bCoarse, check_ori, vMatches12);
}

int orbm_search_for_triangulation_gated(orbm_t* m, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* has_mp1,
                                        int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                                        int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* has_mp2,
                                        int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                                        orbm_pair_gate_fn gate, void* user, int check_ori, int32_t* vMatches12) {
    if (!gate) { set_merr("orbm_search_for_triangulation_gated needs a gate callback"); return ORBM_E_INVALID; }
    return triangulation_impl(m, false, n1, kps1, desc1, has_mp1, nullptr, nn1, nodes1, start1, idx1, n2, kps2, desc2, has_mp2, nullptr,
                              nn2, nodes2, start2, idx2, nullptr, 0.f, 0.f, nullptr, nullptr, 0, 0, check_ori, vMatches12, gate, user);
}

int orbm_search_by_projection_kf(orbm_t* m, const orbm_frame_t* cur, const uint8_t* blocked_in, const float* sf,
                                 int nq, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                                 const float* angle, const uint8_t* qdesc, float th, int ORBdist, int check_ori, int32_t* match) {
    if (!m || !cur || nq < 0) return ORBM_E_INVALID;
    WindowTables W(nq);
    for (int i = 0; i < nq; ++i) {
        if (!valid[i]) { W.skip(i); continue; }
        W.set(i, th * sf[level[i]], level[i] - 1, level[i] + 1);            // :2775-2778
    }
    CandLists L;
    int rc = window_lists(m, cur, false, W.query(u, v, nullptr, nullptr, qdesc), 2048, L);   // this overload has no stereo gate
    if (rc) return rc;
    int nmatches = 0;
    RotHist rh;
    const float factor = ORBM_HISTO_LENGTH / 360.0f;                        // :2736
    std::vector<uint8_t> taken(blocked_in, blocked_in + cur->n);
    for (int i = 0; i < cur->n; ++i) match[i] = -1;
    for (int i = 0; i < nq; ++i) {
        if (!valid[i] || L.count(i) == 0) continue;
        const auto [bestDist, bestIdx2] = best_unblocked(L, i, taken.data());   // :2793
        if (bestDist <= ORBdist) {
            match[bestIdx2] = i; taken[bestIdx2] = 1;
            nmatches++;
            if (check_ori) rh.add(angle[i], cur->kps[bestIdx2].angle, factor, bestIdx2);
        }
    }
    if (check_ori) rh.cull([&](int k) { match[k] = ORBM_MATCH_PRUNED; nmatches--; });
    return nmatches;
}

int orbm_search_by_projection_sim3(orbm_t* m, const orbm_frame_t* kf, const uint8_t* matched_in, const float* sf,
                                   int nq, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                                   const uint8_t* qdesc, int th, float ratioHamming, int32_t* match) {
    if (!m || !kf || nq < 0) return ORBM_E_INVALID;
    WindowTables W(nq);
    for (int i = 0; i < nq; ++i) {
        if (!valid[i]) { W.skip(i); continue; }
        W.set(i, th * sf[level[i]], level[i] - 1, level[i]);                // :600-601, :625-627
    }
    CandLists L;
    int rc = window_lists(m, kf, false, W.query(u, v, nullptr, nullptr, qdesc), 2048, L);
    if (rc) return rc;
    int nmatches = 0;
    std::vector<uint8_t> matched(matched_in, matched_in + kf->n);
    for (int i = 0; i < kf->n; ++i) match[i] = -1;
    for (int i = 0; i < nq; ++i) {
        if (!valid[i] || L.count(i) == 0) continue;
        const auto [bestDist, bestIdx] = best_unblocked(L, i, matched.data());   // :621-622
        if (bestDist <= ORBM_TH_LOW * ratioHamming) { match[bestIdx] = i; matched[bestIdx] = 1; nmatches++; }
    }
    return nmatches;
}

int orbm_fuse(orbm_t* m, const orbm_frame_t* kf, const float* sf, const float* inv_sigma2,
              int nq, const uint8_t* valid, const float* u, const float* v, const float* ur, const int32_t* level,
              const uint8_t* qdesc, float th, int chi2_gate, int32_t* best_idx) {
    if (!m || !kf || nq < 0) return ORBM_E_INVALID;
    WindowTables W(nq);
    for (int i = 0; i < nq; ++i) {
        if (!valid[i]) { W.skip(i); continue; }
        W.set(i, th * sf[level[i]], level[i] - 1, level[i]);
    }
    CandLists L;
    int rc = window_lists(m, kf, false, W.query(u, v, nullptr, nullptr, qdesc), 2048, L);   // the chi2 gate below is not a window gate
    if (rc) return rc;
    int nFused = 0;
    for (int i = 0; i < nq; ++i) {
        best_idx[i] = -1;
        if (!valid[i] || L.count(i) == 0) continue;
        int bestDist = chi2_gate ? 256 : INT_MAX, bestIdx = -1;
        for (int c = 0, nc = L.count(i); c < nc; ++c) {
            const int k = L.index(i, c);
            if (chi2_gate) {                                                 // :1925-1949
                const orbm_kp_t& kp = kf->kps[k];
                if (kf->uright && kf->uright[k] >= 0) {
                    const float ex = u[i] - kp.x, ey = v[i] - kp.y, er = ur[i] - kf->uright[k];
                    const float e2 = ex * ex + ey * ey + er * er;
                    if (e2 * inv_sigma2[kp.octave] > 7.8) continue;
                } else {
                    const float ex = u[i] - kp.x, ey = v[i] - kp.y;
                    const float e2 = ex * ex + ey * ey;
                    if (e2 * inv_sigma2[kp.octave] > 5.99) continue;
                }
            }
            const int d = L.distance(i, c);
            if (d < bestDist) { bestDist = d; bestIdx = k; }
        }
        if (bestDist <= ORBM_TH_LOW) { best_idx[i] = bestIdx; nFused++; }
    }
    return nFused;
}

static int sim3_one_way(orbm* m, const orbm_frame_t* src, const orbm_frame_t* dst, const float* sf_dst, const uint8_t* valid,
                        const float* u, const float* v, const int32_t* level, const uint8_t* qdesc, float th, std::vector<int>& vnMatch) {
    const int nq = src->n;
    vnMatch.assign(nq, -1);
    WindowTables W(nq);
    for (int i = 0; i < nq; ++i) {
        if (!valid[i]) { W.skip(i); continue; }
        W.set(i, th * sf_dst[level[i]], level[i] - 1, level[i]);
    }
    CandLists L;
    int rc = window_lists(m, dst, false, W.query(u, v, nullptr, nullptr, qdesc), 2048, L);
    if (rc) return rc;
    for (int i = 0; i < nq; ++i) {
        if (!valid[i]) continue;
        int bestDist = INT_MAX, bestIdx = -1;
        for (int c = 0, nc = L.count(i); c < nc; ++c) {
            const int d = L.distance(i, c);
            if (d < bestDist) { bestDist = d; bestIdx = L.index(i, c); }
        }
        if (bestDist <= ORBM_TH_HIGH) vnMatch[i] = bestIdx;
    }
    return ORBM_OK;
}

int orbm_search_by_sim3(orbm_t* m, const orbm_frame_t* kf1, const orbm_frame_t* kf2, const float* sf1, const float* sf2,
                        const uint8_t* valid1, const float* u1, const float* v1, const int32_t* level1, const uint8_t* qdesc1,
                        const uint8_t* valid2, const float* u2, const float* v2, const int32_t* level2, const uint8_t* qdesc2,
                        float th, int32_t* matches12) {
    if (!m || !kf1 || !kf2) return ORBM_E_INVALID;
    std::vector<int> vnMatch1, vnMatch2;
    int rc = sim3_one_way(m, kf1, kf2, sf2, valid1, u1, v1, level1, qdesc1, th, vnMatch1);
    if (rc) return rc;
    rc = sim3_one_way(m, kf2, kf1, sf1, valid2, u2, v2, level2, qdesc2, th, vnMatch2);
    if (rc) return rc;
    int nFound = 0;
    for (int i1 = 0; i1 < kf1->n; ++i1) {
        matches12[i1] = -1;
        const int idx2 = vnMatch1[i1];
        if (idx2 >= 0 && vnMatch2[idx2] == i1) { matches12[i1] = idx2; nFound++; }
    }
    return nFound;
}

int orbm_grid_build_batch_async(orbm_t* m, const orbm_kp_t* kps, const int32_t* counts, int nframes, int cap,
                                float min_x, float min_y, float inv_w, float inv_h, int32_t* grid_start, int32_t* grid_idx) {
    if (!m || !kps || !counts || !grid_start || !grid_idx || nframes < 1 || cap < 1 || cap > 65535) return ORBM_E_INVALID;
    MHIPCHK(hipSetDevice(m->device));
    int n2 = 64; while (n2 < cap) n2 <<= 1;
    if (cap > GRID_WIDE_MIN) MHIPCHK(grid_wide_attr((const void*)k_grid_build_batch_wide));
    else if (cap > GRID_CS_MAX && n2 * 4 > 48 * 1024) MHIPCHK(hipFuncSetAttribute((const void*)k_grid_build_batch, hipFuncAttributeMaxDynamicSharedMemorySize, n2 * 4));
    MHIPCHK(rec_time(m, m->e2));
    m->gridFirst = true;                                                    // orbm_last_timing then spans grid build + the next kernel
    if (cap <= GRID_CS_MAX)
        hipLaunchKernelGGL(k_grid_build_batch_cs, dim3(nframes), dim3(256), grid_cs_lds(cap), m->stream, (const KpIn*)kps, counts, cap,
                           min_x, min_y, inv_w, inv_h, grid_start, grid_idx);
    else if (cap > GRID_WIDE_MIN)
        hipLaunchKernelGGL(k_grid_build_batch_wide, dim3(nframes), dim3(256), grid_cs_lds(cap), m->stream, (const KpIn*)kps, counts, cap,
                           min_x, min_y, inv_w, inv_h, grid_start, grid_idx);
    else
        hipLaunchKernelGGL(k_grid_build_batch, dim3(nframes), dim3(256), (size_t)n2 * 4, m->stream, (const KpIn*)kps, counts, cap, n2,
                           min_x, min_y, inv_w, inv_h, grid_start, grid_idx);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

// the first nlevels scale factors, the last one repeated to the table's 12 entries
static ScaleTab scale_tab(const float* sf, int nlevels) {
    ScaleTab st;
    for (int i = 0; i < 12; ++i) st.sf[i] = i < nlevels ? sf[i] : sf[nlevels - 1];
    return st;
}

// the capacity refusals of the points (M3) and frame (M4) batch calls: the candidate words hold a keypoint index and its grid
// position in 16 bits each; the per-query arrays are indexed batch * q_stride + q
static int lp_capacity(const char* call, int cap, int q_stride, int nlevels, int nbatch, const char* batch_name) {
    if (cap > 65535) { set_merr("%s: %d keypoint slots per frame (the candidate words hold 65535)", call, cap); return ORBM_E_CAPACITY; }
    if (q_stride > ORBM_LP_MAX_QUERIES) { set_merr("%s: q_stride %d above %d", call, q_stride, (int)ORBM_LP_MAX_QUERIES); return ORBM_E_CAPACITY; }
    if (nlevels > 12) { set_merr("%s: %d scale levels (the scale table holds 12)", call, nlevels); return ORBM_E_CAPACITY; }
    if (nbatch > 65535) { set_merr("%s: %d %s in one call (at most 65535)", call, nbatch, batch_name); return ORBM_E_CAPACITY; }
    return ORBM_OK;
}

// the searched pool of a batched search as its entry point names it (counts NULL where the search reads none)
static Pool pool_view(const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap, const int32_t* grid_start, const int32_t* grid_idx,
                      float min_x, float min_y, float inv_w, float inv_h) {
    return Pool{(const KpIn*)kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h};
}

// The handle's scratch carved for a batched search over `rows` query rows:
//   [win: a float4 per row] | ncam x [cnt | keys | r] | [acc: nacc words] | [tail bytes]
// win and r only with SC_WIN / SC_R (M4 and M5 used to keep acc in front of r; nothing depends on the order).  cnt is padded to 256 bytes, keys / r / acc with their SC_PAD_ flag: the byte counts the entry points
// have always asked for (a captured graph relies on an earlier eager call having grown the block to its size).
enum { SC_WIN = 1, SC_R = 2, SC_PAD_KEYS = 4, SC_PAD_R = 8, SC_PAD_ACC = 16 };
struct SearchScratch { float4* win; TopList cam[2]; unsigned* acc; uint8_t* tail; };
static int search_scratch(orbm* m, const char* call, size_t rows, int ncam, unsigned flags, size_t nacc, size_t tail, SearchScratch& S) {
    const auto sized = [&](size_t b, unsigned pad) { return flags & pad ? (b + 255) & ~(size_t)255 : b; };
    const size_t bWin = flags & SC_WIN ? rows * sizeof(float4) : 0, bCnt = (rows * sizeof(int) + 255) & ~(size_t)255,
                 bKeys = sized(rows * TK_K * sizeof(unsigned), SC_PAD_KEYS), bR = flags & SC_R ? sized(rows * sizeof(float), SC_PAD_R) : 0,
                 bCam = bCnt + bKeys + bR, bAcc = sized(nacc * sizeof(unsigned), SC_PAD_ACC), bytes = bWin + ncam * bCam + bAcc + tail;
    uint8_t* scr = batch_scratch(m, bytes);
    if (!scr) { set_merr("%s scratch of %zu B unavailable (inside a capture, run the call once eagerly first)", call, bytes); return ORBM_E_HIP; }
    S.win = (float4*)scr;
    for (int c = 0; c < ncam; ++c) {
        uint8_t* b = scr + bWin + c * bCam;
        S.cam[c] = TopList{(int*)b, (unsigned*)(b + bCnt), flags & SC_R ? (float*)(b + bCnt + bKeys) : nullptr};
    }
    S.acc = (unsigned*)(scr + bWin + ncam * bCam);
    S.tail = scr + bWin + ncam * bCam + bAcc;
    return ORBM_OK;
}

// the common ending of a batched search: the closing time stamp of orbm_last_timing (the opening one is rec_time(m, m->e0) before the launches)
static int timed_end(orbm* m) {
    MHIPCHK(rec_time(m, m->e1));
    MHIPCHK(hipGetLastError());
    m->timed = true;
    return ORBM_OK;
}

int orbm_track_window_batch_async(orbm_t* m, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                  const int32_t* grid_start, const int32_t* grid_idx,
                                  float min_x, float min_y, float inv_w, float inv_h,
                                  int q_first, int t_first, int npairs, float th, const float* sf, int nlevels,
                                  float dx, float dy, int32_t* best_idx, int32_t* best_dist, int32_t* second_dist) {
    if (!m || !kps || !desc || !counts || !grid_start || !grid_idx || !best_idx || !best_dist || !second_dist || npairs < 1 ||
        nlevels < 1 || nlevels > 12 || !sf) return ORBM_E_INVALID;
    MHIPCHK(hipSetDevice(m->device));
    const Pool pool = pool_view(kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    const TrackArgs A{q_first, t_first, th, dx, dy, 0.f};
    const ScaleTab st = scale_tab(sf, nlevels);
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_track_window, dim3((cap + 3) / 4, npairs), dim3(256), 0, m->stream, pool, A, st, best_idx, best_dist, second_dist);
    return timed_end(m);
}

int orbm_search_by_projection_batch_async(orbm_t* m, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                          const int32_t* grid_start, const int32_t* grid_idx,
                                          float min_x, float min_y, float inv_w, float inv_h,
                                          int q_first, int t_first, int npairs, float th, const float* sf, int nlevels,
                                          float dx, float dy, const uint8_t* t_blocked, const uint8_t* q_obs, int check_orientation,
                                          int32_t* match, int32_t* nmatches) {
    if (!m || !kps || !desc || !counts || !grid_start || !grid_idx || !match || !nmatches || npairs < 1 || cap < 1 || cap > 65535 ||
        nlevels < 1 || nlevels > 12 || !sf || q_first < 0 || t_first < 0) return ORBM_E_INVALID;
    MHIPCHK(hipSetDevice(m->device));
    const size_t lds = (size_t)(2 * ((cap + 31) >> 5) + 32 + cap) * sizeof(unsigned);   // blocked bits, rotation histogram, observed bits, proposal tags
    if (lds > 64 * 1024) { set_merr("SearchByProjection batch: %d keypoint slots per frame need %zu B of LDS (limit 64 KB, ~16 000 slots)", cap, lds); return ORBM_E_INVALID; }
    // scratch of the handle: per query the window population and its TK_K best candidates, per pair the (slot, bin) list of the assignments,
    // and the searched frames' grid entries, packed (k_track_pack)
    const size_t rows = (size_t)npairs * cap;
    SearchScratch S;
    if (const int rc = search_scratch(m, "SearchByProjection batch", rows, 1, SC_PAD_KEYS | SC_PAD_ACC, rows, rows * sizeof(uint4), S)) return rc;
    const TopList L = S.cam[0];
    uint4* ent = (uint4*)S.tail;
    const Pool pool = pool_view(kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    const TrackArgs A{q_first, t_first, th, dx, dy, ORBM_HISTO_LENGTH / 360.0f};   // factor: ORBmatcher.cc:2478
    const ScaleTab st = scale_tab(sf, nlevels);
    MHIPCHK(rec_time(m, m->e0));
#ifdef ORBX_AB
    if (ab_env("ORBM_TOPK_WAVE"))                                           // A/B: a wave per query
        hipLaunchKernelGGL(k_track_topk, dim3((cap + 3) / 4, npairs), dim3(256), 0, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h,
                           q_first, t_first, th, st, dx, dy, A.factor, L.cnt, L.keys);
    else
#endif
    {
        hipLaunchKernelGGL(k_track_pack, dim3((cap + 255) / 256, npairs), dim3(256), 0, m->stream, pool, t_first, ent);
#ifdef ORBX_AB
        if (ab_env("ORBM_TOPK16_V1"))                                       // A/B: descriptors and distances for every grid entry
            hipLaunchKernelGGL(k_track_topk16_v1, dim3((cap + 15) / 16, npairs), dim3(256), 0, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, ent, min_x, min_y, inv_w, inv_h,
                               q_first, t_first, th, st, dx, dy, A.factor, L.cnt, L.keys);
        else
#endif
        hipLaunchKernelGGL(k_track_topk16, dim3((cap + 15) / 16, npairs), dim3(256), 0, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, ent, min_x, min_y, inv_w, inv_h,
                           q_first, t_first, th, st, dx, dy, A.factor, L.cnt, L.keys);
    }
#ifdef ORBX_AB
    if (ab_env("ORBM_CLAIM_V1"))                                            // A/B: eight queries per step
        hipLaunchKernelGGL(k_track_claim, dim3(npairs), dim3(64), lds, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h, q_first, t_first, th, st, dx, dy, A.factor, L.cnt, L.keys, t_blocked, q_obs, check_orientation, S.acc, match, nmatches);
    else
#endif
    hipLaunchKernelGGL(k_track_claim64, dim3(npairs), dim3(64), lds, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h, q_first, t_first, th, st, dx, dy, A.factor, L.cnt, L.keys, t_blocked, q_obs, check_orientation, S.acc, match, nmatches);
    return timed_end(m);
}

int orbm_search_by_projection_points_batch_async(orbm_t* m, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                                 const int32_t* grid_start, const int32_t* grid_idx,
                                                 float min_x, float min_y, float inv_w, float inv_h, int t_first, int nframes,
                                                 const float* uright, const uint8_t* t_blocked, const int32_t* nq, int q_stride,
                                                 const uint8_t* in_view, const float* proj_x, const float* proj_y, const float* proj_xr,
                                                 const float* view_cos, const int32_t* level, const float* depth, float th_far,
                                                 const uint8_t* qdesc, const uint8_t* mp_obs, int q_shared,
                                                 float th, float nnratio, const float* scale_factors_host, int nlevels,
                                                 int32_t* match, int32_t* nmatches) {
    if (!m || !kps || !desc || !counts || !grid_start || !grid_idx || !nq || !in_view || !proj_x || !proj_y || !view_cos || !level ||
        !qdesc || !mp_obs || !match || !nmatches || !scale_factors_host || (uright && !proj_xr)) {
        set_merr("SearchByProjection points batch: a required array is NULL (proj_xr is required with uright)");
        return ORBM_E_INVALID;
    }
    if (nframes < 1 || cap < 1 || q_stride < 1 || t_first < 0 || nlevels < 1) {
        set_merr("SearchByProjection points batch: nframes, cap, q_stride and nlevels must be >= 1, t_first >= 0");
        return ORBM_E_INVALID;
    }
    if (const int rc = lp_capacity("SearchByProjection points batch", cap, q_stride, nlevels, nframes, "frames")) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const ScaleTab st = scale_tab(scale_factors_host, nlevels);
    const size_t lds = (size_t)(((cap + 31) >> 5) + 32 + 64 * TK_K) * sizeof(unsigned);   // k_claim's layout: blocked bits, histogram (unused here), the current 64 queries' lists
    // scratch of the handle: per query the window population, its TK_K best candidates and its radius
    SearchScratch S;
    if (const int rc = search_scratch(m, "SearchByProjection points batch", (size_t)nframes * q_stride, 1, SC_R, 0, 0, S)) return rc;
    const Pool pool = pool_view(kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    LpRows R;
    R.nq = nq; R.q_stride = q_stride;
    R.in_view = in_view; R.px = proj_x; R.py = proj_y; R.pxr = proj_xr; R.view_cos = view_cos; R.level = level;
    R.depth = depth; R.th_far = th_far;
    R.qdesc = qdesc; R.mp_obs = mp_obs; R.q_shared = q_shared != 0;
    R.th = th; R.nlevels = nlevels;
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_lp_topk, dim3((q_stride + 3) / 4, nframes), dim3(256), 0, m->stream, pool, t_first, uright, R, st, S.cam[0]);
    hipLaunchKernelGGL(k_lp_claim, dim3(nframes), dim3(64), lds, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h, t_first, uright, t_blocked, R, nnratio, S.cam[0], match, nmatches);
    return timed_end(m);
}

int orbm_search_by_projection_frame_batch_async(orbm_t* m, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                                const int32_t* grid_start, const int32_t* grid_idx,
                                                float min_x, float min_y, float inv_w, float inv_h, int t_first, int npairs,
                                                const float* uright, float mbf, const uint8_t* t_blocked, const uint8_t* dir,
                                                const int32_t* nq, int q_stride, const uint8_t* valid, const float* u, const float* v,
                                                const float* invzc, const int32_t* octave, const float* angle, const uint8_t* qdesc,
                                                const uint8_t* mp_obs, float th, int retry_below, const float* scale_factors_host, int nlevels,
                                                int check_orientation, int32_t* match, int32_t* nmatches, uint8_t* retried) {
    if (!m || !kps || !desc || !counts || !grid_start || !grid_idx || !nq || !valid || !u || !v || !octave || !angle || !qdesc || !mp_obs ||
        !match || !nmatches || !scale_factors_host || (uright && !invzc)) {
        set_merr("SearchByProjection frame batch: a required array is NULL (invzc is required with uright)");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || cap < 1 || q_stride < 1 || t_first < 0 || nlevels < 1 || retry_below < 0) {
        set_merr("SearchByProjection frame batch: npairs, cap, q_stride and nlevels must be >= 1, t_first and retry_below >= 0");
        return ORBM_E_INVALID;
    }
    if (const int rc = lp_capacity("SearchByProjection frame batch", cap, q_stride, nlevels, npairs, "pairs")) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const ScaleTab st = scale_tab(scale_factors_host, nlevels);
    const size_t lds = (size_t)(((cap + 31) >> 5) + 32 + 64 * TK_K) * sizeof(unsigned);   // blocked bits, histogram, the current 64 queries' lists
    // scratch of the handle: per query the window population, its TK_K best candidates and a slot of the accepted-assignment list
    const size_t rows = (size_t)npairs * q_stride;
    SearchScratch S;
    if (const int rc = search_scratch(m, "SearchByProjection frame batch", rows, 1, SC_R, rows, 0, S)) return rc;
    const Pool pool = pool_view(kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    MmRows R;
    R.nq = nq; R.q_stride = q_stride;
    R.valid = valid; R.u = u; R.v = v; R.invzc = invzc; R.octave = octave; R.angle = angle;
    R.qdesc = qdesc; R.mp_obs = mp_obs; R.dir = dir;
    R.mbf = mbf; R.factor = ORBM_HISTO_LENGTH / 360.0f;                     // ORBmatcher.cc:2478
    R.nlevels = nlevels; R.retry_below = retry_below; R.check_ori = check_orientation != 0;
    const dim3 gTop((q_stride + 3) / 4, npairs);
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_mm_topk<false>, gTop, dim3(256), 0, m->stream, pool, t_first, uright, R, st, th, nmatches, S.cam[0]);
    hipLaunchKernelGGL(k_mm_claim<false>, dim3(npairs), dim3(64), lds, m->stream, pool, t_first, uright, t_blocked, R, S.cam[0], S.acc, match, nmatches, retried);
    if (retry_below > 0) {                                                  // Tracking.cc:3213-3221, decided per pair on the device
        const float th2 = 2 * th;
        hipLaunchKernelGGL(k_mm_topk<true>, gTop, dim3(256), 0, m->stream, pool, t_first, uright, R, st, th2, nmatches, S.cam[0]);
        hipLaunchKernelGGL(k_mm_claim<true>, dim3(npairs), dim3(64), lds, m->stream, pool, t_first, uright, nullptr, R, S.cam[0], S.acc, match, nmatches, retried);
    }
    return timed_end(m);
}

int orbm_search_by_projection_frame_fisheye_batch_async(orbm_t* m, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                                        const int32_t* grid_start, const int32_t* grid_idx,
                                                        float min_x, float min_y, float inv_w, float inv_h, int first_l, int first_r, int npairs,
                                                        const uint8_t* blocked_l, const uint8_t* blocked_r, const uint8_t* dir,
                                                        const int32_t* nq, int q_stride, const uint8_t* valid,
                                                        const float* u, const float* v, const float* ur, const float* vr,
                                                        const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                                        float th, int retry_below, const float* scale_factors_host, int nlevels, int check_orientation,
                                                        int32_t* match_l, int32_t* match_r, int32_t* nmatches, uint8_t* retried) {
    if (!m || !kps || !desc || !counts || !grid_start || !grid_idx || !nq || !valid || !u || !v || !ur || !vr || !octave || !angle || !qdesc ||
        !mp_obs || !match_l || !match_r || !nmatches || !scale_factors_host) {
        set_merr("SearchByProjection frame fisheye batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || cap < 1 || q_stride < 1 || first_l < 0 || first_r < 0 || nlevels < 1 || retry_below < 0) {
        set_merr("SearchByProjection frame fisheye batch: npairs, cap, q_stride and nlevels must be >= 1, first_l, first_r and retry_below >= 0");
        return ORBM_E_INVALID;
    }
    if (const int rc = lp_capacity("SearchByProjection frame fisheye batch", cap, q_stride, nlevels, npairs, "pairs")) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const ScaleTab st = scale_tab(scale_factors_host, nlevels);
    const size_t lds = (size_t)(2 * ((cap + 31) >> 5) + 32 + 2 * 64 * TK_K) * sizeof(unsigned);   // two blocked bit arrays, histogram, both cameras' lists of the current 64 queries
    // scratch of the handle: per query and camera the window population, its TK_K best candidates and its radius; per query two slots of
    // the accepted-assignment list
    const size_t rows = (size_t)npairs * q_stride;
    SearchScratch S;
    if (const int rc = search_scratch(m, "SearchByProjection frame fisheye batch", rows, 2, SC_R | SC_PAD_R, 2 * rows, 0, S)) return rc;
    const Pool pool = pool_view(kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    MmRows R;
    R.nq = nq; R.q_stride = q_stride;
    R.valid = valid; R.u = u; R.v = v; R.invzc = nullptr; R.octave = octave; R.angle = angle;   // no stereo gate when Nleft != -1 (ORBmatcher.cc:2569)
    R.qdesc = qdesc; R.mp_obs = mp_obs; R.dir = dir;
    R.mbf = 0.f; R.factor = ORBM_HISTO_LENGTH / 360.0f;                     // ORBmatcher.cc:2480
    R.nlevels = nlevels; R.retry_below = retry_below; R.check_ori = check_orientation != 0;
    MmRows Rr = R;                                                          // the right camera's candidate pass: the same rows at (ur, vr), :2616-2633
    Rr.u = ur; Rr.v = vr;
    const dim3 gTop((q_stride + 3) / 4, npairs);
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_mm_topk<false>, gTop, dim3(256), 0, m->stream, pool, first_l, nullptr, R, st, th, nmatches, S.cam[0]);
    hipLaunchKernelGGL(k_mm_topk<false>, gTop, dim3(256), 0, m->stream, pool, first_r, nullptr, Rr, st, th, nmatches, S.cam[1]);
    hipLaunchKernelGGL(k_mmf_claim<false>, dim3(npairs), dim3(64), lds, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h, first_l, first_r, blocked_l, blocked_r, R, ur, vr,
                       S.cam[0], S.cam[1], S.acc, match_l, match_r, nmatches, retried);
    if (retry_below > 0) {                                                  // Tracking.cc:3213-3221, decided per pair on the device
        const float th2 = 2 * th;
        hipLaunchKernelGGL(k_mm_topk<true>, gTop, dim3(256), 0, m->stream, pool, first_l, nullptr, R, st, th2, nmatches, S.cam[0]);
        hipLaunchKernelGGL(k_mm_topk<true>, gTop, dim3(256), 0, m->stream, pool, first_r, nullptr, Rr, st, th2, nmatches, S.cam[1]);
        hipLaunchKernelGGL(k_mmf_claim<true>, dim3(npairs), dim3(64), lds, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h, first_l, first_r, nullptr, nullptr, R, ur, vr,
                           S.cam[0], S.cam[1], S.acc, match_l, match_r, nmatches, retried);
    }
    return timed_end(m);
}

int orbm_search_by_projection_points_fisheye_batch_async(orbm_t* m, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                                         const int32_t* grid_start, const int32_t* grid_idx,
                                                         float min_x, float min_y, float inv_w, float inv_h, int first_l, int first_r, int npairs,
                                                         const uint8_t* blocked_l, const uint8_t* blocked_r, const int32_t* l2r, const int32_t* r2l,
                                                         const int32_t* nq, int q_stride,
                                                         const uint8_t* in_view, const float* proj_x, const float* proj_y, const float* view_cos, const int32_t* level,
                                                         const uint8_t* in_view_r, const float* proj_xr, const float* proj_yr, const float* view_cos_r, const int32_t* level_r,
                                                         const float* depth, float th_far, const uint8_t* qdesc, const uint8_t* mp_obs, int q_shared,
                                                         float th, float nnratio, const float* scale_factors_host, int nlevels,
                                                         int32_t* match_l, int32_t* match_r, int32_t* nmatches) {
    if (!m) return ORBM_E_INVALID;
    if (!kps || !desc || !counts || !grid_start || !grid_idx || !nq || !in_view || !proj_x || !proj_y || !view_cos || !level ||
        !in_view_r || !proj_xr || !proj_yr || !view_cos_r || !level_r || !qdesc || !mp_obs || !match_l || !match_r || !nmatches ||
        !scale_factors_host) {
        set_merr("SearchByProjection points fisheye batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || cap < 1 || q_stride < 1 || first_l < 0 || first_r < 0 || nlevels < 1) {
        set_merr("SearchByProjection points fisheye batch: npairs, cap, q_stride and nlevels must be >= 1, first_l and first_r >= 0");
        return ORBM_E_INVALID;
    }
    if (const int rc = lp_capacity("SearchByProjection points fisheye batch", cap, q_stride, nlevels, npairs, "pairs")) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const ScaleTab st = scale_tab(scale_factors_host, nlevels);
    const size_t lds = (size_t)(2 * ((cap + 31) >> 5) + 2 * 64 * TK_K) * sizeof(unsigned);   // two blocked bit arrays, both cameras' lists of the current 64 queries
    // scratch of the handle: per query and camera the window population, its TK_K best candidates and its radius
    SearchScratch S;
    if (const int rc = search_scratch(m, "SearchByProjection points fisheye batch", (size_t)npairs * q_stride, 2, SC_R | SC_PAD_R, 0, 0, S)) return rc;
    const Pool pool = pool_view(kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    LpRows R;
    R.nq = nq; R.q_stride = q_stride;
    R.in_view = in_view; R.px = proj_x; R.py = proj_y; R.pxr = nullptr; R.view_cos = view_cos; R.level = level;   // no stereo gate when Nleft != -1 (ORBmatcher.cc:107)
    R.depth = depth; R.th_far = th_far;
    R.qdesc = qdesc; R.mp_obs = mp_obs; R.q_shared = q_shared != 0;
    R.th = th; R.nlevels = nlevels;
    LpRows Rr = R;                                                          // the right camera's candidate pass: the mbTrackInViewR fields, no th factor (:173-176)
    Rr.in_view = in_view_r; Rr.px = proj_xr; Rr.py = proj_yr; Rr.view_cos = view_cos_r; Rr.level = level_r;
    Rr.th = 1.0f;
    const dim3 gTop((q_stride + 3) / 4, npairs);
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_lp_topk, gTop, dim3(256), 0, m->stream, pool, first_l, nullptr, R, st, S.cam[0]);
    hipLaunchKernelGGL(k_lp_topk, gTop, dim3(256), 0, m->stream, pool, first_r, nullptr, Rr, st, S.cam[1]);
    hipLaunchKernelGGL(k_lpf_claim, dim3(npairs), dim3(64), lds, m->stream, (const KpIn*)kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h, first_l, first_r, blocked_l, blocked_r, l2r, r2l, R, Rr, nnratio,
                       S.cam[0], S.cam[1], match_l, match_r, nmatches);
    return timed_end(m);
}

int orbm_project_last_frame_batch_async(orbm_t* m, int npairs, const float* tcw_cur, const float* tcw_last, const int32_t* nq, int q_stride,
                                        const float* x3dw, const uint8_t* has_mp, const float* k_host, const float* bounds_host, float mb, int mono,
                                        uint8_t* valid, float* u, float* v, float* invzc, uint8_t* dir) {
    if (!m || !tcw_cur || !tcw_last || !nq || !x3dw || !has_mp || !k_host || !bounds_host || !valid || !u || !v || !invzc || !dir) {
        set_merr("project last frame batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || q_stride < 1) { set_merr("project last frame batch: npairs and q_stride must be >= 1"); return ORBM_E_INVALID; }
    if (q_stride > ORBM_LP_MAX_QUERIES) { set_merr("project last frame batch: q_stride %d above %d", q_stride, (int)ORBM_LP_MAX_QUERIES); return ORBM_E_CAPACITY; }
    if (npairs > 65535) { set_merr("project last frame batch: %d pairs in one call (at most 65535)", npairs); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    MmProj P;
    for (int i = 0; i < 4; ++i) { P.k[i] = k_host[i]; P.bounds[i] = bounds_host[i]; }
    P.mb = mb; P.mono = mono != 0; P.q_stride = q_stride;
    hipLaunchKernelGGL(k_mm_project, dim3((q_stride + 255) / 256, npairs), dim3(256), 0, m->stream, tcw_cur, tcw_last, nq, x3dw, has_mp, P,
                       valid, u, v, invzc, dir);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_fuse_batch_async(orbm_t* m, int npairs,
                          int nkf_rows, int cap, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const float* uright_kf,
                          const int32_t* grid_start, const int32_t* grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                          const int32_t* kf_row, const float* tcw, const float* ow,
                          const int32_t* nq, int q_stride, const uint8_t* valid,
                          const float* pw, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* qdesc, int q_shared,
                          const float* k_host, const float* bounds_host, float bf,
                          float th, int chi2_gate, const float* scale_factors_host, const float* inv_sigma2_host,
                          float log_scale_factor, int nlevels,
                          int32_t* best_idx, int32_t* nfused, int32_t* level_out) {
    if (!m || !kps_kf || !desc_kf || !grid_start || !grid_idx || !tcw || !ow || !nq || !valid || !pw || !normal || !min_dist || !max_dist ||
        !qdesc || !k_host || !bounds_host || !scale_factors_host || (chi2_gate && !inv_sigma2_host) || !best_idx || !nfused) {
        set_merr("Fuse batch: a required array is NULL (inv_sigma2 is required with chi2_gate)");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || nkf_rows < 1 || cap < 1 || q_stride < 1 || nlevels < 1 || !std::isfinite(th)) {
        set_merr("Fuse batch: npairs, nkf_rows, cap, q_stride and nlevels must be >= 1, th finite");
        return ORBM_E_INVALID;
    }
    if (const int rc = lp_capacity("Fuse batch", cap, q_stride, nlevels, npairs, "pairs")) return rc;
    MHIPCHK(hipSetDevice(m->device));
    FuseRows R;
    R.nq = nq; R.valid = valid; R.pw = pw; R.normal = normal; R.min_dist = min_dist; R.max_dist = max_dist; R.qdesc = qdesc;
    FuseParams P;
    for (int i = 0; i < 4; ++i) { P.k[i] = k_host[i]; P.bounds[i] = bounds_host[i]; }
    P.bf = bf; P.th = th; P.logSF = log_scale_factor;
    P.nlevels = nlevels; P.q_stride = q_stride; P.q_shared = q_shared != 0; P.chi2 = chi2_gate != 0; P.nkf_rows = nkf_rows;
    const ScaleTab st = scale_tab(scale_factors_host, nlevels);
    for (int i = 0; i < 12; ++i) {
        P.sf[i] = st.sf[i];
        P.isg[i] = chi2_gate ? inv_sigma2_host[std::min(i, nlevels - 1)] : 0.f;
    }
    const Pool pool = pool_view(kps_kf, desc_kf, nullptr, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_fuse_topk, dim3((q_stride + 3) / 4, npairs), dim3(256), 0, m->stream, pool, uright_kf, kf_row, tcw, ow, R, P, best_idx, level_out);
    hipLaunchKernelGGL(k_fuse_count, dim3(npairs), dim3(256), 0, m->stream, best_idx, q_stride, nfused);
    return timed_end(m);
}

int orbm_search_by_projection_kf_batch_async(orbm_t* m, int npairs,
                                             int nf_rows, int cap, const orbm_kp_t* kps_f, const uint8_t* desc_f, const int32_t* counts_f,
                                             const int32_t* grid_start, const int32_t* grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                                             const int32_t* f_row, const uint8_t* f_blocked, const float* tcw, const float* ow,
                                             const int32_t* nq, int q_stride, const uint8_t* valid, const float* pw,
                                             const float* min_dist, const float* max_dist, const float* angle, const uint8_t* qdesc,
                                             const float* k_host, const float* bounds_host, float th, int orb_dist,
                                             const float* scale_factors_host, float log_scale_factor, int nlevels, int check_orientation,
                                             int32_t* match, int32_t* nmatches) {
    if (!m || !kps_f || !desc_f || !counts_f || !grid_start || !grid_idx || !tcw || !ow || !nq || !valid || !pw || !min_dist || !max_dist ||
        !angle || !qdesc || !k_host || !bounds_host || !scale_factors_host || !match || !nmatches) {
        set_merr("SearchByProjection KF batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || nf_rows < 1 || cap < 1 || q_stride < 1 || nlevels < 1 || !std::isfinite(th) || orb_dist > 255) {
        set_merr("SearchByProjection KF batch: npairs, nf_rows, cap, q_stride and nlevels must be >= 1, th finite, orb_dist <= 255");
        return ORBM_E_INVALID;
    }
    if (const int rc = lp_capacity("SearchByProjection KF batch", cap, q_stride, nlevels, npairs, "pairs")) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const size_t lds = (size_t)(((cap + 31) >> 5) + 32 + 64 * TK_K) * sizeof(unsigned);   // blocked bits, histogram, the current 64 queries' lists
    // scratch of the handle: per query the window population, its TK_K best candidates, a slot of the accepted-assignment list, the
    // radius and the window centre / level (the last two read back only by a rescan)
    const size_t rows = (size_t)npairs * q_stride;
    SearchScratch S;
    if (const int rc = search_scratch(m, "SearchByProjection KF batch", rows, 1, SC_WIN | SC_R, rows, 0, S)) return rc;
    const Pool pool = pool_view(kps_f, desc_f, counts_f, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    RlRows R;
    R.nq = nq; R.valid = valid; R.pw = pw; R.min_dist = min_dist; R.max_dist = max_dist; R.angle = angle; R.qdesc = qdesc;
    RlParams P;
    for (int i = 0; i < 4; ++i) { P.k[i] = k_host[i]; P.bounds[i] = bounds_host[i]; }
    P.th = th; P.logSF = log_scale_factor; P.factor = ORBM_HISTO_LENGTH / 360.0f;   // ORBmatcher.cc:2736
    P.nlevels = nlevels; P.q_stride = q_stride; P.nf_rows = nf_rows; P.orb_dist = orb_dist; P.check_ori = check_orientation != 0;
    const ScaleTab st = scale_tab(scale_factors_host, nlevels);
    for (int i = 0; i < 12; ++i) P.sf[i] = st.sf[i];
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_rl_topk, dim3((q_stride + 3) / 4, npairs), dim3(256), 0, m->stream, pool, f_row, tcw, ow, R, P, S.cam[0], S.win);
    hipLaunchKernelGGL(k_claim<RlPol>, dim3(npairs), dim3(64), lds, m->stream, (const KpIn*)kps_f, desc_f, counts_f, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h, f_row, f_blocked, R, P, S.cam[0].cnt, S.cam[0].keys, S.cam[0].r, S.win, S.acc, match, nmatches);
    return timed_end(m);
}

int orbm_search_by_projection_sim3_batch_async(orbm_t* m, int npairs,
                                               int nkf_rows, int cap, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const int32_t* counts_kf,
                                               const int32_t* grid_start, const int32_t* grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                                               const int32_t* kf_row, const uint8_t* matched_in, const float* tcw, const float* ow,
                                               const int32_t* nq, int q_stride, const uint8_t* valid, const float* pw, const float* normal,
                                               const float* min_dist, const float* max_dist, const uint8_t* qdesc,
                                               const float* k_host, const float* bounds_host, int th, float ratio_hamming, int proj_form,
                                               const float* scale_factors_host, float log_scale_factor, int nlevels,
                                               int32_t* match, int32_t* nmatches) {
    if (!m || !kps_kf || !desc_kf || !counts_kf || !grid_start || !grid_idx || !tcw || !ow || !nq || !valid || !pw || !normal || !min_dist ||
        !max_dist || !qdesc || !k_host || !bounds_host || !scale_factors_host || !match || !nmatches) {
        set_merr("SearchByProjection Sim3 batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    const float maxDist = ORBM_TH_LOW * ratio_hamming;                       // the reference's float product (:651, :773)
    if (npairs < 1 || nkf_rows < 1 || cap < 1 || q_stride < 1 || nlevels < 1 || !std::isfinite(ratio_hamming) || !(maxDist < 256.f) ||
        (proj_form != 0 && proj_form != 1)) {
        set_merr("SearchByProjection Sim3 batch: npairs, nkf_rows, cap, q_stride and nlevels must be >= 1, ratio_hamming finite with "
                 "50 * ratio_hamming < 256, proj_form 0 or 1");
        return ORBM_E_INVALID;
    }
    if (const int rc = lp_capacity("SearchByProjection Sim3 batch", cap, q_stride, nlevels, npairs, "pairs")) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const size_t lds = (size_t)(((cap + 31) >> 5) + 32 + 64 * TK_K) * sizeof(unsigned);   // k_claim's layout: blocked bits, histogram (unused here), the current 64 queries' lists
    // scratch of the handle, as M5's: per query the window population, its TK_K best candidates, the radius and the window centre / level
    SearchScratch S;
    if (const int rc = search_scratch(m, "SearchByProjection Sim3 batch", (size_t)npairs * q_stride, 1, SC_WIN | SC_R, 0, 0, S)) return rc;
    const Pool pool = pool_view(kps_kf, desc_kf, counts_kf, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h);
    FuseRows R;
    R.nq = nq; R.valid = valid; R.pw = pw; R.normal = normal; R.min_dist = min_dist; R.max_dist = max_dist; R.qdesc = qdesc;
    FuseParams P;
    for (int i = 0; i < 4; ++i) { P.k[i] = k_host[i]; P.bounds[i] = bounds_host[i]; }
    P.bf = 0.f; P.th = (float)th; P.logSF = log_scale_factor;
    P.nlevels = nlevels; P.q_stride = q_stride; P.q_shared = 0; P.chi2 = 0; P.nkf_rows = nkf_rows;
    const ScaleTab st = scale_tab(scale_factors_host, nlevels);
    for (int i = 0; i < 12; ++i) { P.sf[i] = st.sf[i]; P.isg[i] = 0.f; }
    const S3Claim Cp{q_stride, nkf_rows, maxDist};
    MHIPCHK(rec_time(m, m->e0));
    const dim3 tg((q_stride + 3) / 4, npairs);
    if (proj_form) hipLaunchKernelGGL(k_s3_topk<1>, tg, dim3(256), 0, m->stream, pool, kf_row, tcw, ow, R, P, S.cam[0], S.win);
    else hipLaunchKernelGGL(k_s3_topk<0>, tg, dim3(256), 0, m->stream, pool, kf_row, tcw, ow, R, P, S.cam[0], S.win);
    hipLaunchKernelGGL(k_claim<S3Pol>, dim3(npairs), dim3(64), lds, m->stream, (const KpIn*)kps_kf, desc_kf, counts_kf, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h, kf_row, matched_in, S3Rows{nq, qdesc}, Cp, S.cam[0].cnt, S.cam[0].keys, S.cam[0].r, S.win,
                       (unsigned*)nullptr, match, nmatches);
    return timed_end(m);
}

// ---- DBoW2 vocabulary ----
struct orbm_vocab {
    int k = 0, L = 0, nnodes = 0, nwords = 0, device = 0;
    // level-major layout (k_bow_transform2): node rows renumbered breadth-first, the children of a node contiguous in child order
    unsigned* dInfo = nullptr;                                 // [nnodes] first child << 5 | child count
    int *dOrig = nullptr, *dWord = nullptr;                    // [nnodes] the vocabulary's own node id; word id (leaves)
    uint8_t* dDesc = nullptr;
    double* dWeight = nullptr;
};

void orbm_vocab_destroy(orbm_vocab_t* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    void* ptrs[] = {v->dInfo, v->dOrig, v->dWord, v->dDesc, v->dWeight};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete v;
}

int orbm_vocab_create(orbm_t* m, orbm_vocab_t** out, int k, int L, int nnodes, const int32_t* parent, const uint8_t* is_leaf,
                      const uint8_t* desc, const double* weight) {
    if (!m || !out || nnodes < 2 || !parent || !is_leaf || !desc || !weight) return ORBM_E_INVALID;
    *out = nullptr;
    // children lists in node-id order, word ids in leaf order: what loadFromTextFile builds (:1385-1420)
    std::vector<int> cstart(nnodes + 1, 0), cidx(nnodes - 1), word(nnodes, 0);
    for (int i = 1; i < nnodes; ++i) {
        if (parent[i] < 0 || parent[i] >= i) { set_merr("vocabulary node %d has parent %d (must precede it)", i, parent[i]); return ORBM_E_INVALID; }
        cstart[parent[i] + 1]++;
    }
    for (int i = 0; i < nnodes; ++i) cstart[i + 1] += cstart[i];
    std::vector<int> fill(cstart.begin(), cstart.end() - 1);
    int nwords = 0;
    for (int i = 1; i < nnodes; ++i) { cidx[fill[parent[i]]++] = i; if (is_leaf[i]) word[i] = nwords++; }
    for (int i = 1; i < nnodes; ++i) {
        if ((cstart[i + 1] == cstart[i]) != (is_leaf[i] != 0)) { set_merr("vocabulary node %d: leaf flag disagrees with its children", i); return ORBM_E_INVALID; }
        if (cstart[i + 1] - cstart[i] > 31) { set_merr("vocabulary node %d has %d children (at most 31 supported; DBoW2 allows k <= 20)", i, cstart[i + 1] - cstart[i]); return ORBM_E_INVALID; }
    }
    if (cstart[1] - cstart[0] > 31) { set_merr("vocabulary root has more than 31 children"); return ORBM_E_INVALID; }
    // level-major renumbering: breadth-first from the root, children of a node consecutive in their child-list order
    std::vector<int> order; order.reserve(nnodes);             // new row -> vocabulary node id
    std::vector<int> newOf(nnodes, -1);
    order.push_back(0); newOf[0] = 0;
    for (size_t h = 0; h < order.size(); ++h) {
        const int id = order[h];
        for (int c = cstart[id]; c < cstart[id + 1]; ++c) { newOf[cidx[c]] = (int)order.size(); order.push_back(cidx[c]); }
    }
    if ((int)order.size() != nnodes) { set_merr("vocabulary is not one tree (%zu of %d nodes reachable from the root)", order.size(), nnodes); return ORBM_E_INVALID; }
    std::vector<unsigned> info(nnodes);
    std::vector<int> wordN(nnodes);
    std::vector<double> weightN(nnodes);
    std::vector<uint8_t> descN((size_t)32 * nnodes);
    for (int r = 0; r < nnodes; ++r) {
        const int id = order[r];
        const int cnt = cstart[id + 1] - cstart[id];
        info[r] = cnt ? ((unsigned)newOf[cidx[cstart[id]]] << 5) | (unsigned)cnt : 0u;
        wordN[r] = word[id]; weightN[r] = weight[id];
        memcpy(&descN[(size_t)32 * r], desc + (size_t)32 * id, 32);
    }
    MHIPCHK(hipSetDevice(m->device));
    orbm_vocab* v = new orbm_vocab;
    v->k = k; v->L = L; v->nnodes = nnodes; v->nwords = nwords; v->device = m->device;
    bool ok = hipMalloc((void**)&v->dInfo, sizeof(unsigned) * nnodes) == hipSuccess && hipMalloc((void**)&v->dOrig, sizeof(int) * nnodes) == hipSuccess &&
              hipMalloc((void**)&v->dWord, sizeof(int) * nnodes) == hipSuccess && hipMalloc((void**)&v->dDesc, (size_t)32 * nnodes) == hipSuccess &&
              hipMalloc((void**)&v->dWeight, sizeof(double) * nnodes) == hipSuccess;
    ok = ok && hipMemcpy(v->dInfo, info.data(), sizeof(unsigned) * nnodes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(v->dOrig, order.data(), sizeof(int) * nnodes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(v->dWord, wordN.data(), sizeof(int) * nnodes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(v->dDesc, descN.data(), (size_t)32 * nnodes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(v->dWeight, weightN.data(), sizeof(double) * nnodes, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { set_merr("vocabulary upload failed"); orbm_vocab_destroy(v); return ORBM_E_HIP; }
    *out = v;
    return ORBM_OK;
}

int orbm_vocab_load_text(orbm_t* m, orbm_vocab_t** out, const char* path) {
    if (!m || !out || !path) return ORBM_E_INVALID;
    FILE* f = fopen(path, "r");
    if (!f) { set_merr("cannot open vocabulary %s", path); return ORBM_E_INVALID; }
    int k = 0, L = 0, n1 = 0, n2 = 0;
    if (fscanf(f, "%d %d %d %d", &k, &L, &n1, &n2) != 4 || k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) {
        fclose(f); set_merr("vocabulary %s: not a correct text file", path); return ORBM_E_INVALID;       // :1359-1363
    }
    // the reference switches transform on the two fields (:1145-1193: addWeight or addIfNotExist, L1 / L2 / division by v.size());
    // orbm_bow_vectors implements TF_IDF (0) + L1_NORM (0), ORBvoc's header, and nothing else
    if (n1 != 0 || n2 != 0) {
        fclose(f);
        set_merr("vocabulary %s: scoring %d / weighting %d in the header; only scoring 0 (L1_NORM) with weighting 0 (TF_IDF) is implemented", path, n1, n2);
        return ORBM_E_INVALID;
    }
    std::vector<int> parent(1, 0);
    std::vector<uint8_t> leaf(1, 0), desc(32, 0);
    std::vector<double> weight(1, 0.0);
    for (;;) {
        int pid, isleaf;
        if (fscanf(f, "%d %d", &pid, &isleaf) != 2) break;
        uint8_t d[32];
        bool good = true;
        for (int i = 0; i < 32; ++i) { int b; if (fscanf(f, "%d", &b) != 1) { good = false; break; } d[i] = (uint8_t)b; }
        double w;
        if (!good || fscanf(f, "%lf", &w) != 1) break;
        parent.push_back(pid); leaf.push_back(isleaf > 0); weight.push_back(w);
        desc.insert(desc.end(), d, d + 32);
    }
    fclose(f);
    return orbm_vocab_create(m, out, k, L, (int)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data());
}

int orbm_vocab_info(const orbm_vocab_t* v, int* k, int* L, int* nnodes, int* nwords) {
    if (!v) return ORBM_E_INVALID;
    *k = v->k; *L = v->L; *nnodes = v->nnodes; *nwords = v->nwords;
    return ORBM_OK;
}

int orbm_bow_transform(orbm_t* m, const orbm_vocab_t* v, const uint8_t* desc, int n, int levelsup,
                       int32_t* word_id, int32_t* node_id, double* weight) {
    if (!m || !v || n < 0 || (n > 0 && (!desc || !word_id || !node_id || !weight))) return ORBM_E_INVALID;
    if (n == 0) return ORBM_OK;
    if (v->device != m->device) { set_merr("vocabulary lives on another device"); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(m->device));
    DevBuf dd, dw, dn, dwt;
    arena_reset(m);
    UP(dd, desc, (size_t)32 * n); AL(dw, sizeof(int) * n); AL(dn, sizeof(int) * n); AL(dwt, sizeof(double) * n);
    m->gridFirst = false;
    MHIPCHK(rec_time(m, m->e0));
    ARENA_FLUSH(m);
    hipLaunchKernelGGL(k_bow_transform2, dim3((unsigned)(((size_t)n * 16 + 255) / 256)), dim3(256), 0, m->stream, dd.as<uint8_t>(), n, v->dInfo,
                       v->dDesc, v->dOrig, v->dWord, v->dWeight, v->L, levelsup, dw.as<int>(), dn.as<int>(), dwt.as<double>());
    MHIPCHK(rec_time(m, m->e1));
    m->timed = true;
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(word_id, dw.host(), sizeof(int) * n);
    memcpy(node_id, dn.host(), sizeof(int) * n);
    memcpy(weight, dwt.host(), sizeof(double) * n);
    return ORBM_OK;
}

int orbm_bow_vectors(int n, const int32_t* word_id, const int32_t* node_id, const double* weight,
                     int32_t* bow_ids, double* bow_vals, int* nbow,
                     int32_t* fv_nodes, int32_t* fv_start, int32_t* fv_idx, int* nfv) {
    // BowVector::addWeight in feature order (BowVector.cpp:34-46), then L1 normalisation in word order (:62-84);
    // FeatureVector::addFeature (FeatureVector.cpp:34-46).  Sorted vectors instead of std::map, same summation order.
    std::vector<std::pair<int, int>> byWord, byNode;             // (key, feature)
    for (int i = 0; i < n; ++i) if (weight[i] > 0) { byWord.push_back(std::make_pair(word_id[i], i)); byNode.push_back(std::make_pair(node_id[i], i)); }
    std::stable_sort(byWord.begin(), byWord.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
    std::stable_sort(byNode.begin(), byNode.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
    int b = 0;
    for (size_t i = 0; i < byWord.size();) {
        size_t j = i;
        double acc = weight[byWord[i].second];
        for (j = i + 1; j < byWord.size() && byWord[j].first == byWord[i].first; ++j) acc += weight[byWord[j].second];
        bow_ids[b] = byWord[i].first; bow_vals[b] = acc; ++b;
        i = j;
    }
    double norm = 0.0;
    for (int i = 0; i < b; ++i) norm += fabs(bow_vals[i]);
    if (norm > 0.0) for (int i = 0; i < b; ++i) bow_vals[i] /= norm;
    *nbow = b;
    int c = 0, o = 0;
    for (size_t i = 0; i < byNode.size();) {
        size_t j = i;
        fv_nodes[c] = byNode[i].first; fv_start[c] = o;
        for (j = i; j < byNode.size() && byNode[j].first == byNode[i].first; ++j) fv_idx[o++] = byNode[j].second;
        ++c;
        i = j;
    }
    fv_start[c] = o;
    *nfv = c;
    return ORBM_OK;
}

int orbm_search_by_projection_frame_fisheye(orbm_t* m, const orbm_frame_t* cur_l, const orbm_frame_t* cur_r,
                                            const uint8_t* blocked_l_in, const uint8_t* blocked_r_in, const float* sf,
                                            int nq, const uint8_t* valid, const float* u, const float* v, const float* ur, const float* vr,
                                            const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                            float th, int bForward, int bBackward, int check_ori, int32_t* match_l, int32_t* match_r) {
    if (!m || !cur_l || !cur_r || nq < 0) return ORBM_E_INVALID;
    WindowTables W(nq);
    for (int i = 0; i < nq; ++i) {
        if (!valid[i]) { W.skip(i); continue; }
        const int o = octave[i];
        if (bForward) W.set(i, th * sf[o], o, -1); else if (bBackward) W.set(i, th * sf[o], 0, o); else W.set(i, th * sf[o], o - 1, o + 1);
    }
    CandLists Ll, Lr;                                                       // no stereo gate when Nleft != -1 (:2569)
    int rc = window_lists(m, cur_l, false, W.query(u, v, nullptr, nullptr, qdesc), 2048, Ll);
    if (rc) return rc;
    rc = window_lists(m, cur_r, false, W.query(ur, vr, nullptr, nullptr, qdesc), 2048, Lr);
    if (rc) return rc;
    int nmatches = 0;
    const int Nleft = cur_l->n;
    RotHist rh;
    const float factor = ORBM_HISTO_LENGTH / 360.0f;
    std::vector<uint8_t> bl(blocked_l_in, blocked_l_in + cur_l->n), br(blocked_r_in, blocked_r_in + cur_r->n);
    for (int i = 0; i < cur_l->n; ++i) match_l[i] = -1;
    for (int i = 0; i < cur_r->n; ++i) match_r[i] = -1;
    // one camera's claim of query i (:2556-2613 left, :2637-2678 right); `first`: the camera's offset in the histogram's entries
    auto claim = [&](const CandLists& L, const orbm_frame_t* f, std::vector<uint8_t>& blocked, int32_t* match, int first, int i) {
        const auto [bestDist, bestIdx2] = best_unblocked(L, i, blocked.data());
        if (bestDist <= ORBM_TH_HIGH) {
            match[bestIdx2] = i;
            if (mp_obs[i]) blocked[bestIdx2] = 1;
            nmatches++;
            if (check_ori) rh.add(angle[i], f->kps[bestIdx2].angle, factor, bestIdx2 + first);
        }
    };
    for (int i = 0; i < nq; ++i) {
        if (!valid[i] || Ll.count(i) == 0) continue;                        // an empty left window skips the right block too (:2551)
        claim(Ll, cur_l, bl, match_l, 0, i);
        claim(Lr, cur_r, br, match_r, Nleft, i);
    }
    if (check_ori) rh.cull([&](int k) { if (k < Nleft) match_l[k] = ORBM_MATCH_PRUNED; else match_r[k - Nleft] = ORBM_MATCH_PRUNED; nmatches--; });
    return nmatches;
}

int orbm_search_by_projection_points_fisheye(orbm_t* m, const orbm_frame_t* f_l, const orbm_frame_t* f_r,
                                             const uint8_t* blocked_l_in, const uint8_t* blocked_r_in,
                                             const int32_t* l2r, const int32_t* r2l, const float* sf,
                                             int nq, const uint8_t* in_view, const float* px, const float* py, const float* view_cos, const int32_t* level,
                                             const uint8_t* in_view_r, const float* pxr, const float* pyr, const float* view_cos_r, const int32_t* level_r,
                                             const uint8_t* qdesc, const uint8_t* mp_obs, float th, float nnratio, int32_t* match_l, int32_t* match_r) {
    if (!m || !f_l || !f_r || nq < 0) return ORBM_E_INVALID;
    const bool bFactor = th != 1.0;
    WindowTables Wl(nq), Wr(nq);
    for (int i = 0; i < nq; ++i) {
        if (!in_view[i]) Wl.skip(i);
        else {
            float r = view_cos[i] > 0.998 ? 2.5f : 4.0f;
            if (bFactor) r *= th;
            Wl.set(i, r * sf[level[i]], level[i] - 1, level[i]);
        }
        if (!in_view_r[i] || level_r[i] == -1) Wr.skip(i);
        else {
            const float r = view_cos_r[i] > 0.998 ? 2.5f : 4.0f;             // the right block applies no th factor (:174)
            Wr.set(i, r * sf[level_r[i]], level_r[i] - 1, level_r[i]);
        }
    }
    CandLists Ll, Lr;
    int rc = window_lists(m, f_l, false, Wl.query(px, py, nullptr, nullptr, qdesc), 2048, Ll);
    if (rc) return rc;
    rc = window_lists(m, f_r, false, Wr.query(pxr, pyr, nullptr, nullptr, qdesc), 2048, Lr);
    if (rc) return rc;
    int nmatches = 0;
    std::vector<uint8_t> bl(blocked_l_in, blocked_l_in + f_l->n), br(blocked_r_in, blocked_r_in + f_r->n);
    for (int i = 0; i < f_l->n; ++i) match_l[i] = -1;
    for (int i = 0; i < f_r->n; ++i) match_r[i] = -1;
    for (int iMP = 0; iMP < nq; ++iMP) {
        if (!in_view[iMP] && !in_view_r[iMP]) continue;
        if (in_view[iMP] && Ll.count(iMP) > 0) {
            const BestTwo b = best_two_levels(Ll, iMP, bl.data(), f_l->kps);
            if (b.bestDist <= ORBM_TH_HIGH) {
                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;          // :151-152 (skips the right block)
                if (b.bestLevel != b.bestLevel2 || b.bestDist <= nnratio * b.bestDist2) {
                    match_l[b.bestIdx] = iMP;
                    if (mp_obs[iMP]) bl[b.bestIdx] = 1;
                    if (l2r[b.bestIdx] != -1) { match_r[l2r[b.bestIdx]] = iMP; if (mp_obs[iMP]) br[l2r[b.bestIdx]] = 1; nmatches++; }
                    nmatches++;
                }
            }
        }
        if (in_view_r[iMP] && level_r[iMP] != -1) {
            if (Lr.count(iMP) == 0) continue;
            const BestTwo b = best_two_levels(Lr, iMP, br.data(), f_r->kps);
            if (b.bestDist <= ORBM_TH_HIGH) {
                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;
                if (r2l[b.bestIdx] != -1) { match_l[r2l[b.bestIdx]] = iMP; if (mp_obs[iMP]) bl[r2l[b.bestIdx]] = 1; nmatches++; }
                match_r[b.bestIdx] = iMP;
                if (mp_obs[iMP]) br[b.bestIdx] = 1;
                nmatches++;
            }
        }
    }
    return nmatches;
}

int orbm_search_by_bow_fisheye(orbm_t* m, int nkf, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const uint8_t* kf_good,
                               int nnk, const int32_t* nodes_k, const int32_t* start_k, const int32_t* idx_k,
                               int nf, int nleft, const orbm_kp_t* kps_f, const uint8_t* desc_f,
                               int nnf, const int32_t* nodes_f, const int32_t* start_f, const int32_t* idx_f,
                               float nnratio, int check_ori, int32_t* f_match) {
    if (!m || nkf < 0 || nf < 0) return ORBM_E_INVALID;
    BucketJobs B;
    int rc = bucket_jobs(m, desc_kf, nkf, nnk, nodes_k, start_k, idx_k, desc_f, nf, nnf, nodes_f, start_f, idx_f, f_match, nf, B);
    if (rc) return rc;
    int nmatches = 0;
    RotHist rh;
    const float factor = ORBM_HISTO_LENGTH / 360.0f;
    for (size_t j = 0; j < B.size(); ++j) {
        const int iKF = B.query(j);
        if (!kf_good[iKF]) continue;
        int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256, bestDist1R = 256, bestIdxFR = -1, bestDist2R = 256;
        for (int c = 0; c < B.count(j); ++c) {
            const int iF = B.index(j, c);
            if (f_match[iF] >= 0) continue;
            const int d = B.distance(j, c);
            if (iF < nleft && d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdxF = iF; }
            else if (iF < nleft && d < bestDist2) bestDist2 = d;
            if (iF >= nleft && d < bestDist1R) { bestDist2R = bestDist1R; bestDist1R = d; bestIdxFR = iF; }
            else if (iF >= nleft && d < bestDist2R) bestDist2R = d;
        }
        if (bestDist1 <= ORBM_TH_LOW) {
            if (static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {
                f_match[bestIdxF] = iKF;
                if (check_ori) rh.add(kps_kf[iKF].angle, kps_f[bestIdxF].angle, factor, bestIdxF);
                nmatches++;
            }
            if (bestDist1R <= ORBM_TH_LOW) {                                 // nested; ratio test disabled by `|| true` (:471-473)
                f_match[bestIdxFR] = iKF;
                if (check_ori) rh.add(kps_kf[iKF].angle, kps_f[bestIdxFR].angle, factor, bestIdxFR);
                nmatches++;
            }
        }
    }
    if (check_ori) rh.cull([&](int i) { f_match[i] = -1; nmatches--; });
    return nmatches;
}

int orbm_search_by_bow_kf(orbm_t* m, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* good1,
                          int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                          int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* good2,
                          int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                          float nnratio, int check_ori, int32_t* vpMatches12) {
    if (!m || n1 < 0 || n2 < 0) return ORBM_E_INVALID;
    BucketJobs B;
    int rc = bucket_jobs(m, desc1, n1, nn1, nodes1, start1, idx1, desc2, n2, nn2, nodes2, start2, idx2, vpMatches12, n1, B);
    if (rc) return rc;
    std::vector<uint8_t> vbMatched2(n2, 0);
    int nmatches = 0;
    RotHist rh;
    const float factor = ORBM_HISTO_LENGTH / 360.0f;                        // :978
    for (size_t j = 0; j < B.size(); ++j) {
        const int i1 = B.query(j);
        if (!good1[i1]) continue;
        int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
        for (int c = 0; c < B.count(j); ++c) {
            const int i2 = B.index(j, c);
            if (vbMatched2[i2] || !good2[i2]) continue;
            const int d = B.distance(j, c);
            if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdx2 = i2; }
            else if (d < bestDist2) bestDist2 = d;
        }
        if (bestDist1 < ORBM_TH_LOW && static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {
            vpMatches12[i1] = bestIdx2;
            vbMatched2[bestIdx2] = 1;
            if (check_ori) rh.add(kps1[i1].angle, kps2[bestIdx2].angle, factor, i1);
            nmatches++;
        }
    }
    if (check_ori) rh.cull([&](int i) { vpMatches12[i] = -1; nmatches--; });
    return nmatches;
}

int orbm_search_by_bow(orbm_t* m, int nkf, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const uint8_t* kf_good,
                       int nnk, const int32_t* nodes_k, const int32_t* start_k, const int32_t* idx_k,
                       int nf, const orbm_kp_t* kps_f, const uint8_t* desc_f,
                       int nnf, const int32_t* nodes_f, const int32_t* start_f, const int32_t* idx_f,
                       float nnratio, int check_ori, int32_t* f_match) {
    if (!m || nkf < 0 || nf < 0) return ORBM_E_INVALID;
    BucketJobs B;
    int rc = bucket_jobs(m, desc_kf, nkf, nnk, nodes_k, start_k, idx_k, desc_f, nf, nnf, nodes_f, start_f, idx_f, f_match, nf, B);
    if (rc) return rc;
    int nmatches = 0;
    RotHist rh;
    const float factor = ORBM_HISTO_LENGTH / 360.0f;                        // :334
    for (size_t j = 0; j < B.size(); ++j) {                                // jobs are in the reference's (node, iKF) order
        const int iKF = B.query(j);
        if (!kf_good[iKF]) continue;
        int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
        for (int c = 0; c < B.count(j); ++c) {
            const int iF = B.index(j, c);
            if (f_match[iF] >= 0) continue;                                 // :385 -- order-dependent gate
            const int d = B.distance(j, c);
            if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdxF = iF; }
            else if (d < bestDist2) bestDist2 = d;
        }
        if (bestDist1 <= ORBM_TH_LOW && static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {
            f_match[bestIdxF] = iKF;
            if (check_ori) rh.add(kps_kf[iKF].angle, kps_f[bestIdxF].angle, factor, bestIdxF);
            nmatches++;
        }
    }
    if (check_ori) rh.cull([&](int i) { f_match[i] = -1; nmatches--; });
    return nmatches;
}

int orbm_stereo_matches(orbm_t* m, void* left, int frame_l, void* right, int frame_r,
                        int nl, const orbm_kp_t* kl, const uint8_t* dl, int nr, const orbm_kp_t* kr, const uint8_t* dr,
                        float mb, float mbf, float* uright, float* depth) {
    if (!m || !left || !right || nl < 0 || nr < 0 || nr > 65535) return ORBM_E_INVALID;
    for (int i = 0; i < nl; ++i) { uright[i] = -1.0f; depth[i] = -1.0f; }
    if (nl == 0 || nr == 0) return 0;
    StereoLevels lv;
    memset(&lv, 0, sizeof lv);
    int nlev = 0, nlevR = 0, devL = 0, devR = 0, wl[12], hl[12], hr[12];
    float sfR[12], isfR[12];
    if (orbx_internal_levels(left, frame_l, &nlev, lv.L, lv.pitchL, wl, hl, lv.sf, lv.isf, &devL) ||
        orbx_internal_levels(right, frame_r, &nlevR, lv.R, lv.pitchR, lv.wR, hr, sfR, isfR, &devR)) {
        set_merr("extractor handles hold no pyramid for the requested batch slot"); return ORBM_E_INVALID;
    }
    if (nlev != nlevR || devL != m->device || devR != m->device) { set_merr("extractors and matcher must share one device and level count"); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(m->device));
    DevBuf bkl, bdl, bkr, bdr, bur, bde, bsad;
    arena_reset(m);
    UP(bkl, kl, sizeof(KpIn) * nl); UP(bdl, dl, (size_t)32 * nl); UP(bkr, kr, sizeof(KpIn) * nr); UP(bdr, dr, (size_t)32 * nr);
    AL(bur, sizeof(float) * nl); AL(bde, sizeof(float) * nl); AL(bsad, sizeof(int) * nl);
    MHIPCHK(rec_time(m, m->e0));
    ARENA_FLUSH(m);
    hipLaunchKernelGGL(k_stereo, dim3((nl + 3) / 4), dim3(256), 0, m->stream, bkl.as<KpIn>(), bdl.as<uint8_t>(), nl, bkr.as<KpIn>(),
                       bdr.as<uint8_t>(), nr, lv, mb, mbf, bur.as<float>(), bde.as<float>(), bsad.as<int>());
    MHIPCHK(rec_time(m, m->e1));
    m->timed = true;
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    std::vector<int> sad(nl);
    memcpy(uright, bur.host(), sizeof(float) * nl);
    memcpy(depth, bde.host(), sizeof(float) * nl);
    memcpy(sad.data(), bsad.host(), sizeof(int) * nl);
    // median cut (Frame.cc:1261-1275)
    std::vector<std::pair<int, int>> vDistIdx;
    for (int i = 0; i < nl; ++i) if (sad[i] >= 0) vDistIdx.push_back(std::make_pair(sad[i], i));
    if (vDistIdx.empty()) return 0;
    std::sort(vDistIdx.begin(), vDistIdx.end());
    const float median = vDistIdx[vDistIdx.size() / 2].first;
    const float thDist = 1.5f * 1.4f * median;
    int kept = (int)vDistIdx.size();
    for (int i = (int)vDistIdx.size() - 1; i >= 0; --i) {
        if (vDistIdx[i].first < thDist) break;
        uright[vDistIdx[i].second] = -1; depth[vDistIdx[i].second] = -1; --kept;
    }
    return kept;
}

// ---- batched, device-resident forms of M15 / 8(f).1 / M10 (config C3 of bench.py: nothing leaves HBM between the extraction and
// the match lists) ------------------------------------------------------------------------------------------
extern "C" int orbx_internal_batch_layout(void* o, const uint8_t* const** l0tab, int* l0pitch, const uint8_t** pyr, size_t* frameBytes,
                                          int* nlevels, int* off, int* pitch, int* w, int* h, float* sf, float* isf, int* device, int* maxBatch, int* kpCap);

int orbm_stereo_batch_async(orbm_t* m, void* extractor, int first_l, int first_r, int npairs, const orbm_kp_t* kps, const uint8_t* desc,
                            const int32_t* counts, int cap, float mb, float mbf, float* uright, float* depth, int32_t* sad, int32_t* kept) {
    if (!m || !extractor || !kps || !desc || !counts || !uright || !depth || !sad || !kept || npairs < 1 || first_l < 0 || first_r < 0 || cap < 1 || cap > 65535) return ORBM_E_INVALID;
    StereoBatchLayout B;
    memset(&B, 0, sizeof B);
    int nlev = 0, dev = 0, maxBatch = 0, kpCap = 0, hl[12] = {};
    if (orbx_internal_batch_layout(extractor, &B.l0, &B.l0pitch, &B.pyr, &B.frameBytes, &nlev, B.off, B.pitch, B.w, hl, B.sf, B.isf, &dev, &maxBatch, &kpCap)) {
        set_merr("the extractor handle holds no geometry"); return ORBM_E_INVALID;
    }
    if (dev != m->device || cap != kpCap || first_l + npairs > maxBatch || first_r + npairs > maxBatch) { set_merr("extractor / matcher mismatch (device, capacity or batch range)"); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(m->device));
    int n2 = 64; while (n2 < cap) n2 <<= 1;
    if (n2 * 4 > 48 * 1024) MHIPCHK(hipFuncSetAttribute((const void*)k_stereo_cut, hipFuncAttributeMaxDynamicSharedMemorySize, n2 * 4));
    // vRowIndices (Frame.cc:1064-1083) of every right image as CSR in the handle's scratch: [npairs][nrows + 1] starts + [npairs][rowCap] indices
    // A keypoint enters rows floor(y - r) .. ceil(y + r), r = 2 * sf[octave] (Frame.cc:1071-1077): at most floor(2 r) + 3 rows (and never
    // more than the image has), so [cap] keypoints of the coarsest level bound every right image's list.
    float sfMax = 1.f;
    for (int l = 0; l < nlev; ++l) sfMax = std::max(sfMax, B.sf[l]);
    const int nrows = hl[0];
    const long long perKp = std::min<long long>((long long)floorf(4.f * sfMax) + 3, nrows);
    if (perKp * cap > 0x7fffffffLL) { set_merr("stereo row lists too large"); return ORBM_E_INVALID; }
    const int rowCap = (int)(perKp * cap);
    const size_t bStart = ((size_t)npairs * (nrows + 1) * sizeof(int) + 255) & ~(size_t)255, bIdx = ((size_t)npairs * rowCap * sizeof(unsigned short) + 255) & ~(size_t)255;
    uint8_t* scr = batch_scratch(m, bStart + bIdx + 256);
    if (!scr) { set_merr("stereo scratch of %zu B unavailable (inside a capture, run the call once eagerly first)", bStart + bIdx + 256); return ORBM_E_HIP; }
    int* rowStart = (int*)scr; unsigned short* rowIdx = (unsigned short*)(scr + bStart);
    int* rowErr = m->hStatus;                                    // cannot happen with the bound above; if it ever does, orbm_sync reports ORBM_E_CAPACITY
    const size_t ldsRows = (size_t)(2 * nrows + 2) * sizeof(int);
    if (ldsRows > 48 * 1024) MHIPCHK(hipFuncSetAttribute((const void*)k_stereo_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsRows));
    m->gridFirst = false;
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_stereo_rows, dim3(npairs), dim3(256), ldsRows, m->stream, (const KpIn*)kps, counts, cap, first_r, B, nrows, rowCap, rowStart, rowIdx, rowErr);
    hipLaunchKernelGGL(k_stereo_batch, dim3((cap + 256 / ST_GS - 1) / (256 / ST_GS), npairs), dim3(256), 0, m->stream, (const KpIn*)kps, desc, counts, cap, first_l, first_r, B, mb, mbf,
                       uright, depth, sad, rowStart, rowIdx, nrows, rowCap);
    hipLaunchKernelGGL(k_stereo_cut, dim3(npairs), dim3(256), 0, m->stream, counts, cap, first_l, n2, sad, uright, depth, kept);
    MHIPCHK(rec_time(m, m->e1));
    m->timed = true;
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_bow_nodes_batch_async(orbm_t* m, const orbm_vocab_t* v, const uint8_t* desc, int nrows, int levelsup, int32_t* node_id) {
    if (!m || !v || !desc || !node_id || nrows < 1) return ORBM_E_INVALID;
    if (v->device != m->device) { set_merr("vocabulary lives on another device"); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(m->device));
    hipLaunchKernelGGL(k_bow_transform2, dim3((unsigned)(((size_t)nrows * 16 + 255) / 256)), dim3(256), 0, m->stream, desc, nrows, v->dInfo, v->dDesc, v->dOrig,
                       v->dWord, v->dWeight, v->L, levelsup, (int*)nullptr, node_id, (double*)nullptr);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_bow_transform_batch_async(orbm_t* m, const orbm_vocab_t* v, const uint8_t* desc, int nrows, int levelsup,
                                   int32_t* word_id, int32_t* node_id, double* weight) {
    if (!m || !v || !desc || !node_id || nrows < 1) { set_merr("bow transform batch: a required array is NULL or nrows < 1"); return ORBM_E_INVALID; }
    if (v->device != m->device) { set_merr("vocabulary lives on another device"); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(m->device));
    hipLaunchKernelGGL(k_bow_transform2, dim3((unsigned)(((size_t)nrows * 16 + 255) / 256)), dim3(256), 0, m->stream, desc, nrows, v->dInfo, v->dDesc, v->dOrig,
                       v->dWord, v->dWeight, v->L, levelsup, word_id, node_id, weight);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_search_by_bow_batch_async(orbm_t* m, int npairs,
                                   int nkf_rows, int cap_kf, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const int32_t* counts_kf,
                                   const int32_t* node_kf, const double* weight_kf, const uint8_t* good_kf,
                                   int nf_rows, int cap_f, const orbm_kp_t* kps_f, const uint8_t* desc_f, const int32_t* counts_f,
                                   const int32_t* node_f, const double* weight_f,
                                   const int32_t* kf_row, const int32_t* f_row, float nnratio, int check_orientation,
                                   int32_t* f_match, int32_t* nmatches) {
    if (!m || !kps_kf || !desc_kf || !counts_kf || !node_kf || !good_kf || !kps_f || !desc_f || !counts_f || !node_f || !f_match || !nmatches) {
        set_merr("SearchByBoW batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || nkf_rows < 1 || nf_rows < 1 || cap_kf < 1 || cap_f < 1 || !std::isfinite(nnratio)) {
        set_merr("SearchByBoW batch: npairs, nkf_rows, nf_rows, cap_kf and cap_f must be >= 1 and nnratio finite");
        return ORBM_E_INVALID;
    }
    if (cap_kf > ORBM_BOW_MAX_CAP || cap_f > ORBM_BOW_MAX_CAP) {
        set_merr("SearchByBoW batch: cap_kf %d / cap_f %d above %d (the bucket lists and the row live in LDS)", cap_kf, cap_f, (int)ORBM_BOW_MAX_CAP);
        return ORBM_E_CAPACITY;
    }
    if (npairs > 65535) { set_merr("SearchByBoW batch: %d pairs in one call (at most 65535)", npairs); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    const size_t lds = bow_search_lds(cap_kf, cap_f);
    // above 48 KB the launch needs the attribute on the current device; always the largest legal size, so that a graph captured
    // earlier with bigger rows still launches after a call with smaller ones
    if (lds > 48 * 1024)
        MHIPCHK(hipFuncSetAttribute((const void*)k_bow_search<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bow_search_lds(ORBM_BOW_MAX_CAP, ORBM_BOW_MAX_CAP)));
    BowSide K{(const KpIn*)kps_kf, desc_kf, counts_kf, node_kf, weight_kf, good_kf, nkf_rows, cap_kf};
    BowSide F{(const KpIn*)kps_f, desc_f, counts_f, node_f, weight_f, nullptr, nf_rows, cap_f};
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_bow_search<false>, dim3(npairs), dim3(BOW_WAVES * 64), lds, m->stream, npairs, K, F, kf_row, f_row, nnratio,
                       check_orientation, f_match, nmatches);
    MHIPCHK(rec_time(m, m->e1));
    MHIPCHK(hipGetLastError());
    m->timed = true;
    return ORBM_OK;
}

int orbm_search_by_bow_fisheye_batch_async(orbm_t* m, int npairs,
                                           int nkf_rows, int cap_kf, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const int32_t* counts_kf,
                                           const int32_t* node_kf, const double* weight_kf, const uint8_t* good_kf,
                                           int nf_rows, int cap_f, const orbm_kp_t* kps_f, const uint8_t* desc_f, const int32_t* counts_f,
                                           const int32_t* node_f, const double* weight_f,
                                           const int32_t* kf_row, const int32_t* fl_row, const int32_t* fr_row, float nnratio, int check_orientation,
                                           int32_t* f_match_l, int32_t* f_match_r, int32_t* nmatches) {
    if (!m || !kps_kf || !desc_kf || !counts_kf || !node_kf || !good_kf || !kps_f || !desc_f || !counts_f || !node_f || !fl_row || !fr_row ||
        !f_match_l || !f_match_r || !nmatches) {
        set_merr("SearchByBoW fisheye batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || nkf_rows < 1 || nf_rows < 1 || cap_kf < 1 || cap_f < 1 || !std::isfinite(nnratio)) {
        set_merr("SearchByBoW fisheye batch: npairs, nkf_rows, nf_rows, cap_kf and cap_f must be >= 1 and nnratio finite");
        return ORBM_E_INVALID;
    }
    if (cap_kf > ORBM_BOW_MAX_CAP || cap_f > ORBM_BOW_FISHEYE_MAX_CAP_F) {
        set_merr("SearchByBoW fisheye batch: cap_kf %d above %d or cap_f %d above %d per camera (the bucket lists and the row over both cameras live in LDS)",
                 cap_kf, (int)ORBM_BOW_MAX_CAP, cap_f, (int)ORBM_BOW_FISHEYE_MAX_CAP_F);
        return ORBM_E_CAPACITY;
    }
    if (npairs > 65535) { set_merr("SearchByBoW fisheye batch: %d pairs in one call (at most 65535)", npairs); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    const size_t lds = bow_search_lds(cap_kf, 2 * cap_f);                   // the frame list and the claimed row run over both cameras
    if (lds > 48 * 1024)                                                     // as orbm_search_by_bow_batch_async: always the largest legal size
        MHIPCHK(hipFuncSetAttribute((const void*)k_bow_search_fisheye, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)bow_search_lds(ORBM_BOW_MAX_CAP, 2 * ORBM_BOW_FISHEYE_MAX_CAP_F)));
    BowSide K{(const KpIn*)kps_kf, desc_kf, counts_kf, node_kf, weight_kf, good_kf, nkf_rows, cap_kf};
    BowSide F{(const KpIn*)kps_f, desc_f, counts_f, node_f, weight_f, nullptr, nf_rows, cap_f};
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_bow_search_fisheye, dim3(npairs), dim3(BOW_WAVES * 64), lds, m->stream, npairs, K, F, kf_row, fl_row, fr_row, nnratio,
                       check_orientation, f_match_l, f_match_r, nmatches);
    MHIPCHK(rec_time(m, m->e1));
    MHIPCHK(hipGetLastError());
    m->timed = true;
    return ORBM_OK;
}

int orbm_search_by_bow_kf_batch_async(orbm_t* m, int npairs,
                                      int nrows1, int cap1, const orbm_kp_t* kps1, const uint8_t* desc1, const int32_t* counts1,
                                      const int32_t* node1, const double* weight1, const uint8_t* good1,
                                      int nrows2, int cap2, const orbm_kp_t* kps2, const uint8_t* desc2, const int32_t* counts2,
                                      const int32_t* node2, const double* weight2, const uint8_t* good2,
                                      const int32_t* row1, const int32_t* row2, float nnratio, int check_orientation,
                                      int32_t* matches12, int32_t* nmatches) {
    if (!m || !kps1 || !desc1 || !counts1 || !node1 || !good1 || !kps2 || !desc2 || !counts2 || !node2 || !good2 || !matches12 || !nmatches) {
        set_merr("SearchByBoW KF batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || nrows1 < 1 || nrows2 < 1 || cap1 < 1 || cap2 < 1 || !std::isfinite(nnratio)) {
        set_merr("SearchByBoW KF batch: npairs, nrows1, nrows2, cap1 and cap2 must be >= 1 and nnratio finite");
        return ORBM_E_INVALID;
    }
    if (cap1 > ORBM_BOW_MAX_CAP || cap2 > ORBM_BOW_MAX_CAP) {
        set_merr("SearchByBoW KF batch: cap1 %d / cap2 %d above %d (the bucket lists and the claimed row live in LDS)", cap1, cap2, (int)ORBM_BOW_MAX_CAP);
        return ORBM_E_CAPACITY;
    }
    if (npairs > 65535) { set_merr("SearchByBoW KF batch: %d pairs in one call (at most 65535)", npairs); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    const size_t lds = bow_search_lds(cap1, cap2);
    if (lds > 48 * 1024)                                                     // as orbm_search_by_bow_batch_async: always the largest legal size
        MHIPCHK(hipFuncSetAttribute((const void*)k_bow_search<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bow_search_lds(ORBM_BOW_MAX_CAP, ORBM_BOW_MAX_CAP)));
    BowSide K{(const KpIn*)kps1, desc1, counts1, node1, weight1, good1, nrows1, cap1};
    BowSide F{(const KpIn*)kps2, desc2, counts2, node2, weight2, good2, nrows2, cap2};
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_bow_search<true>, dim3(npairs), dim3(BOW_WAVES * 64), lds, m->stream, npairs, K, F, row1, row2, nnratio,
                       check_orientation, matches12, nmatches);
    MHIPCHK(rec_time(m, m->e1));
    MHIPCHK(hipGetLastError());
    m->timed = true;
    return ORBM_OK;
}

int orbm_triangulation_batch_async(orbm_t* m, int npairs, int cap,
                                   const orbm_kp_t* kps1, const uint8_t* desc1, const int32_t* counts1, const int32_t* node1, const float* uright1,
                                   const orbm_kp_t* kps2, const uint8_t* desc2, const int32_t* counts2, const int32_t* node2, const float* uright2,
                                   const float* F12, float epx, float epy, const float* scale_factors2, const float* level_sigma2_2, int nlevels,
                                   int only_stereo, int coarse, int32_t* matches12, int32_t* nmatches) {
    if (!m || npairs < 1 || cap < 1 || cap > 65535 || !kps1 || !desc1 || !counts1 || !node1 || !kps2 || !desc2 || !counts2 || !node2 || !F12 || !scale_factors2 ||
        !level_sigma2_2 || nlevels < 1 || nlevels > 12 || !matches12 || !nmatches) return ORBM_E_INVALID;
    MHIPCHK(hipSetDevice(m->device));
    TriParams P;
    for (int i = 0; i < 9; ++i) P.F12[i] = F12[i];
    P.epx = epx; P.epy = epy; P.onlyStereo = only_stereo; P.coarse = coarse;
    for (int i = 0; i < 12; ++i) { P.sf2[i] = scale_factors2[std::min(i, nlevels - 1)]; P.sigma2[i] = level_sigma2_2[std::min(i, nlevels - 1)]; }
    const size_t bS = ((size_t)npairs * 257 * sizeof(int) + 255) & ~(size_t)255, bI = ((size_t)npairs * cap * sizeof(unsigned short) + 255) & ~(size_t)255;
    uint8_t* scr = batch_scratch(m, bS + bI);
    if (!scr) { set_merr("triangulation scratch of %zu B unavailable (inside a capture, run the call once eagerly first)", bS + bI); return ORBM_E_HIP; }
    int* bStart = (int*)scr; unsigned short* bIdx = (unsigned short*)(scr + bS);
    MHIPCHK(hipMemsetAsync(nmatches, 0, sizeof(int) * npairs, m->stream));
    hipLaunchKernelGGL(k_tri_buckets, dim3(npairs), dim3(256), 0, m->stream, counts2, node2, cap, bStart, bIdx);
    hipLaunchKernelGGL(k_triangulate_batch, dim3((cap + 255) / 256, npairs), dim3(256), 0, m->stream, (const KpIn*)kps1, desc1, counts1, node1, uright1,
                       (const KpIn*)kps2, desc2, counts2, node2, uright2, cap, P, matches12, nmatches, bStart, bIdx);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_search_for_triangulation_batch_async(orbm_t* m, int npairs,
                                              int nrows1, int cap1, const orbm_kp_t* kps1, const uint8_t* desc1, const int32_t* counts1,
                                              const int32_t* node1, const double* weight1, const uint8_t* has_mp1, const float* uright1,
                                              int nrows2, int cap2, const orbm_kp_t* kps2, const uint8_t* desc2, const int32_t* counts2,
                                              const int32_t* node2, const double* weight2, const uint8_t* has_mp2, const float* uright2,
                                              const int32_t* row1, const int32_t* row2, const float* F12, const float* ep,
                                              const float* scale_factors2_host, const float* level_sigma2_2_host, int nlevels,
                                              int only_stereo, int coarse, int check_orientation,
                                              int32_t* matches12, int32_t* nmatches) {
    if (!m || !kps1 || !desc1 || !counts1 || !node1 || !has_mp1 || !kps2 || !desc2 || !counts2 || !node2 || !has_mp2 || !F12 || !ep ||
        !scale_factors2_host || !level_sigma2_2_host || !matches12 || !nmatches) {
        set_merr("SearchForTriangulation batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || nrows1 < 1 || nrows2 < 1 || cap1 < 1 || cap2 < 1 || nlevels < 1) {
        set_merr("SearchForTriangulation batch: npairs, nrows1, nrows2, cap1, cap2 and nlevels must be >= 1");
        return ORBM_E_INVALID;
    }
    if (cap1 > 65535 || cap2 > 65535) { set_merr("SearchForTriangulation batch: cap1 %d / cap2 %d above 65535 (16-bit bucket lists)", cap1, cap2); return ORBM_E_CAPACITY; }
    if (nlevels > 12) { set_merr("SearchForTriangulation batch: %d pyramid levels (at most 12)", nlevels); return ORBM_E_CAPACITY; }
    if (npairs > 65535) { set_merr("SearchForTriangulation batch: %d pairs in one call (at most 65535)", npairs); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    TriBatchParams P;
    for (int i = 0; i < 12; ++i) { P.sf2[i] = scale_factors2_host[std::min(i, nlevels - 1)]; P.sigma2[i] = level_sigma2_2_host[std::min(i, nlevels - 1)]; }
    P.nlevels = nlevels; P.onlyStereo = only_stereo != 0; P.coarse = coarse != 0; P.npairs = npairs;
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t bS = pad((size_t)nrows2 * 257 * sizeof(int)), bE = pad((size_t)nrows2 * cap2 * sizeof(uint2));
    uint8_t* scr = batch_scratch(m, bS + bE);
    if (!scr) { set_merr("SearchForTriangulation batch: scratch of %zu B unavailable (inside a capture, run the call once eagerly first)", bS + bE); return ORBM_E_HIP; }
    int* bStart = (int*)scr; uint2* bEnt = (uint2*)(scr + bS);
    const TriSide A{(const KpIn*)kps1, desc1, counts1, node1, weight1, has_mp1, uright1, nrows1, cap1};
    const TriSide B{(const KpIn*)kps2, desc2, counts2, node2, weight2, has_mp2, uright2, nrows2, cap2};
    int lpf = 16;                                                            // lanes per pKF1 feature: the measured choice (profiles/NOTES.md); 1 and 4 for A/B runs
    if (const char* e = ab_env("ORBM_TRI_LPF")) { const int v = atoi(e); if (v == 1 || v == 4) lpf = v; }   // anything else keeps 16: the grid below is sized by lpf
    MHIPCHK(rec_time(m, m->e0));
    MHIPCHK(hipMemsetAsync(matches12, 0xFF, sizeof(int32_t) * (size_t)npairs * cap1, m->stream));   // every entry -1
    hipLaunchKernelGGL(k_trib_buckets, dim3(nrows2), dim3(256), 0, m->stream, B, row2, P, bStart, bEnt);
    const dim3 grid(((size_t)cap1 * lpf + 255) / 256, npairs);
#define TRIB_SEARCH(L) hipLaunchKernelGGL(k_trib_search<L>, grid, dim3(256), 0, m->stream, A, B, row1, row2, F12, ep, P, bStart, bEnt, matches12)
    if (lpf == 1) TRIB_SEARCH(1); else if (lpf == 4) TRIB_SEARCH(4); else TRIB_SEARCH(16);
#undef TRIB_SEARCH
    hipLaunchKernelGGL(k_trib_tail, dim3(npairs), dim3(256), 0, m->stream, A, B, row1, row2, check_orientation, matches12, nmatches);
    MHIPCHK(rec_time(m, m->e1));
    MHIPCHK(hipGetLastError());
    m->timed = true;
    return ORBM_OK;
}

int orbm_search_for_initialization_batch_async(orbm_t* m, int npairs,
                                               int nrows1, int cap1, const orbm_kp_t* kps1, const uint8_t* desc1, const int32_t* counts1,
                                               int nrows2, int cap2, const orbm_kp_t* kps2, const uint8_t* desc2, const int32_t* counts2,
                                               const int32_t* grid_start, const int32_t* grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                                               const int32_t* row1, const int32_t* row2, const float* prev_in,
                                               int window_size, float nnratio, int check_orientation,
                                               int32_t* matches12, int32_t* nmatches, float* prev_out) {
    if (!m || !kps1 || !desc1 || !counts1 || !kps2 || !desc2 || !counts2 || !grid_start || !grid_idx || !prev_in || !matches12 || !nmatches || !prev_out) {
        set_merr("SearchForInitialization batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (npairs < 1 || nrows1 < 1 || nrows2 < 1 || cap1 < 1 || cap2 < 1 || window_size < 0) {
        set_merr("SearchForInitialization batch: npairs, nrows1, nrows2, cap1 and cap2 must be >= 1, window_size >= 0");
        return ORBM_E_INVALID;
    }
    if (cap1 > ORBM_INIT_MAX_CAP || cap2 > ORBM_INIT_MAX_CAP) {
        set_merr("SearchForInitialization batch: cap1 %d / cap2 %d above %d (16-bit owners; the claimed row over cap2 lives in LDS)", cap1, cap2, (int)ORBM_INIT_MAX_CAP);
        return ORBM_E_CAPACITY;
    }
    if (npairs > 65535) { set_merr("SearchForInitialization batch: %d pairs in one call (at most 65535)", npairs); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    // candidate lists: per workgroup the first query's region (cap2) + room for the rest of a chunk; no list is capped, a full scratch ends a chunk
    const int nwg = std::min(npairs, 128);
    InitParams P{min_x, min_y, inv_w, inv_h, (float)window_size, nnratio, ORBM_HISTO_LENGTH / 360.0f, check_orientation != 0, npairs,
                 (unsigned)cap2 + (256u << 10)};
    if (const char* e = ab_env("ORBM_INIT_ROOM")) P.budget = (unsigned)cap2 + (unsigned)std::max(0, atoi(e));   // test knob: a chunk per query at 0
    const size_t bytes = (size_t)nwg * P.budget * sizeof(unsigned int);
    uint8_t* scr = batch_scratch(m, bytes);
    if (!scr) { set_merr("SearchForInitialization batch: scratch of %zu B unavailable (inside a capture, run the call once eagerly first)", bytes); return ORBM_E_HIP; }
    const size_t lds = (size_t)cap2 * sizeof(unsigned int);
    if (!m->initLds) {                                                       // once per handle, on its first (eager) call: the largest legal size
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(m->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) {
            set_merr("SearchForInitialization batch: inside a capture, run the call once eagerly first");
            return ORBM_E_HIP;
        }
        MHIPCHK(hipFuncSetAttribute((const void*)k_init_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(ORBM_INIT_MAX_CAP * sizeof(unsigned int))));
        m->initLds = true;
    }
    const InitSide A{(const KpIn*)kps1, desc1, counts1, nrows1, cap1};
    const InitSide B{(const KpIn*)kps2, desc2, counts2, nrows2, cap2};
    MHIPCHK(rec_time(m, m->e0));
    hipLaunchKernelGGL(k_init_search, dim3(nwg), dim3(INIT_WAVES * 64), lds, m->stream, A, B, grid_start, grid_idx, row1, row2, prev_in, prev_out, P,
                       (unsigned int*)scr, matches12, nmatches);
    MHIPCHK(rec_time(m, m->e1));
    MHIPCHK(hipGetLastError());
    m->timed = true;
    return ORBM_OK;
}

// ---- SURVEY 8(f).2 / 8(f).3 ------------------------------------------------------------------------------
static bool fill_undist(UndistParams& P, const float* k, const float* dist, int ndist, const float* newk) {
    for (double& d : P.k) d = 0.0;
    for (int i = 0; i < ndist && i < 14; ++i) P.k[i] = (double)dist[i];
    P.fx = k[0]; P.fy = k[1]; P.cx = k[2]; P.cy = k[3];
    P.nfx = newk[0]; P.nfy = newk[1]; P.ncx = newk[2]; P.ncy = newk[3];
    return ndist < 1 || dist[0] == 0.0f;                         // Frame.cc:928: first coefficient zero -> no undistortion
}

// tauX / tauY (dist[12], dist[13]): undistort_point has no inverse tilt, so a call that sets either is refused instead of
// quietly getting the 12-term answer
static bool has_tilt(const float* dist, int ndist) {
    for (int i = 12; i < ndist && i < 14; ++i)
        if (!(dist[i] == 0.0f)) { set_merr("undistortion: the tilted sensor model (dist[12], dist[13] nonzero) is not implemented"); return true; }
    return false;
}

int orbm_undistort_keypoints(orbm_t* m, int space, const orbm_kp_t* kps, int n, const float* k, const float* dist, int ndist,
                             const float* newk, orbm_kp_t* out) {
    if (!m || n < 0 || !k || !newk || ndist < 0 || ndist > 14 || (ndist > 0 && !dist) || (n > 0 && (!kps || !out))) return ORBM_E_INVALID;
    if (has_tilt(dist, ndist)) return ORBM_E_INVALID;
    if (n == 0) return 0;
    MHIPCHK(hipSetDevice(m->device));
    UndistParams P;
    const int pass = fill_undist(P, k, dist, ndist, newk) ? 1 : 0;
    if (space == ORBM_DEVICE) {
        hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, m->stream, (const KpIn*)kps, n, P, pass, (KpIn*)out);
        MHIPCHK(hipGetLastError());
        return n;
    }
    DevBuf di, dout;
    arena_reset(m);
    UP(di, kps, sizeof(KpIn) * n); AL(dout, sizeof(KpIn) * n);
    ARENA_FLUSH(m);
    hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, m->stream, di.as<KpIn>(), n, P, pass, dout.as<KpIn>());
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(out, dout.host(), sizeof(KpIn) * n);
    return n;
}

int orbm_image_bounds(orbm_t* m, int cols, int rows, const float* k, const float* dist, int ndist, const float* newk, float* bounds) {
    if (!m || !k || !newk || !bounds || ndist < 0 || ndist > 14 || (ndist > 0 && !dist)) return ORBM_E_INVALID;
    if (has_tilt(dist, ndist)) return ORBM_E_INVALID;
    if (ndist < 1 || dist[0] == 0.0f) { bounds[0] = 0.f; bounds[1] = (float)cols; bounds[2] = 0.f; bounds[3] = (float)rows; return ORBM_OK; }
    orbm_kp_t c[4], u[4];
    memset(c, 0, sizeof(c));
    c[1].x = (float)cols; c[2].y = (float)rows; c[3].x = (float)cols; c[3].y = (float)rows;
    int rc = orbm_undistort_keypoints(m, ORBM_HOST, c, 4, k, dist, ndist, newk, u);
    if (rc < 0) return rc;
    bounds[0] = std::min(u[0].x, u[2].x); bounds[1] = std::max(u[1].x, u[3].x);      // Frame.cc:1005-1008
    bounds[2] = std::min(u[0].y, u[1].y); bounds[3] = std::max(u[2].y, u[3].y);
    return ORBM_OK;
}

int orbm_is_in_frustum(orbm_t* m, int space, int n, const float* pw, const float* normal, const float* min_dist, const float* max_dist,
                       const float* rcw, const float* tcw, const float* ow, const float* k, const float* bounds,
                       float bf, float viewing_cos_limit, float log_scale_factor, int n_scale_levels,
                       uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr, float* depth, int32_t* level, float* view_cos) {
    if (!m || n < 0 || !rcw || !tcw || !ow || !k || !bounds || n_scale_levels < 1) return ORBM_E_INVALID;
    if (n == 0) return 0;
    if (!pw || !normal || !min_dist || !max_dist || !in_view || !proj_x || !proj_y || !proj_xr || !depth || !level || !view_cos) return ORBM_E_INVALID;
    MHIPCHK(hipSetDevice(m->device));
    FrustumParams F;
    memcpy(F.rcw, rcw, sizeof(F.rcw)); memcpy(F.tcw, tcw, sizeof(F.tcw)); memcpy(F.ow, ow, sizeof(F.ow));
    memcpy(F.k, k, sizeof(F.k)); memcpy(F.bounds, bounds, sizeof(F.bounds));
    F.bf = bf; F.cosLimit = viewing_cos_limit; F.logSF = log_scale_factor; F.nLevels = n_scale_levels;
    const dim3 grid((n + 255) / 256), block(256);
    if (space == ORBM_DEVICE) {
        hipLaunchKernelGGL(k_frustum, grid, block, 0, m->stream, n, pw, normal, min_dist, max_dist, F, in_view, proj_x, proj_y, proj_xr,
                           depth, level, view_cos);
        MHIPCHK(hipGetLastError());
        return 0;
    }
    DevBuf dp, dn, dmin, dmax, div, dx, dy, dxr, dd, dl, dvc;
    arena_reset(m);
    UP(dp, pw, sizeof(float) * 3 * n); UP(dn, normal, sizeof(float) * 3 * n); UP(dmin, min_dist, sizeof(float) * n); UP(dmax, max_dist, sizeof(float) * n);
    AL(div, n); AL(dx, sizeof(float) * n); AL(dy, sizeof(float) * n);
    // the reference leaves mTrackProjXR / mTrackDepth / mnTrackScaleLevel / mTrackViewCos untouched for rejected points:
    // in/out buffers that start from the caller's values
    UPIO(dxr, proj_xr, sizeof(float) * n); UPIO(dd, depth, sizeof(float) * n); UPIO(dl, level, sizeof(int) * n); UPIO(dvc, view_cos, sizeof(float) * n);
    ARENA_FLUSH(m);
    hipLaunchKernelGGL(k_frustum, grid, block, 0, m->stream, n, dp.as<float>(), dn.as<float>(), dmin.as<float>(), dmax.as<float>(), F,
                       div.as<uint8_t>(), dx.as<float>(), dy.as<float>(), dxr.as<float>(), dd.as<float>(), dl.as<int>(), dvc.as<float>());
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(in_view, div.host(), n); memcpy(proj_x, dx.host(), sizeof(float) * n);
    memcpy(proj_y, dy.host(), sizeof(float) * n); memcpy(proj_xr, dxr.host(), sizeof(float) * n);
    memcpy(depth, dd.host(), sizeof(float) * n); memcpy(level, dl.host(), sizeof(int) * n);
    memcpy(view_cos, dvc.host(), sizeof(float) * n);
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += in_view[i] ? 1 : 0;
    return cnt;
}

// Frame::isInFrustum for every frame of a batch in one launch: poses, counts and skip flags from device rows, the rows M3 reads written in place
int orbm_is_in_frustum_batch_async(orbm_t* m, int nframes, const float* tcw, const float* ow, const int32_t* nq, int q_stride, const uint8_t* skip,
                                   const float* pw, const float* normal, const float* min_dist, const float* max_dist, int q_shared,
                                   const float* k_host, const float* bounds_host, float bf, float viewing_cos_limit, float log_scale_factor,
                                   int n_scale_levels, uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr, float* depth, int32_t* level,
                                   float* view_cos, int32_t* n_in_view) {
    const char* who = "isInFrustum batch";
    if (!m) {                                                                // no handle: orbm_create has refused, for want of a device or of a call
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_merr("%s: no HIP device: the MI355X matcher has no CPU fallback", who); return ORBM_E_HIP; }
        set_merr("%s: the handle is NULL", who);
        return ORBM_E_INVALID;
    }
    const struct { const void* p; const char* name; } req[] = {
        {tcw, "tcw"}, {ow, "ow"}, {nq, "nq"}, {pw, "pw"}, {normal, "normal"}, {min_dist, "min_dist"}, {max_dist, "max_dist"}, {k_host, "k_host"},
        {bounds_host, "bounds_host"}, {in_view, "in_view"}, {proj_x, "proj_x"}, {proj_y, "proj_y"}, {proj_xr, "proj_xr"}, {depth, "depth"},
        {level, "level"}, {view_cos, "view_cos"}};
    for (const auto& r : req)
        if (!r.p) { set_merr("%s: %s is NULL", who, r.name); return ORBM_E_INVALID; }
    if (nframes < 1) { set_merr("%s: nframes %d must be >= 1", who, nframes); return ORBM_E_INVALID; }
    if (q_stride < 1) { set_merr("%s: q_stride %d must be >= 1", who, q_stride); return ORBM_E_INVALID; }
    if (n_scale_levels < 1) { set_merr("%s: n_scale_levels %d must be >= 1", who, n_scale_levels); return ORBM_E_INVALID; }
    if (!std::isfinite(viewing_cos_limit)) { set_merr("%s: viewing_cos_limit is not finite", who); return ORBM_E_INVALID; }
    if (!std::isfinite(log_scale_factor)) { set_merr("%s: log_scale_factor is not finite", who); return ORBM_E_INVALID; }
    if (nframes > 65535) { set_merr("%s: nframes %d above 65535", who, nframes); return ORBM_E_CAPACITY; }
    if (q_stride > ORBM_LP_MAX_QUERIES) { set_merr("%s: q_stride %d above %d", who, q_stride, (int)ORBM_LP_MAX_QUERIES); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    FrustumParams C;
    memset(&C, 0, sizeof(C));                                                // the pose fields come from the device rows
    memcpy(C.k, k_host, sizeof(C.k)); memcpy(C.bounds, bounds_host, sizeof(C.bounds));
    C.bf = bf; C.cosLimit = viewing_cos_limit; C.logSF = log_scale_factor; C.nLevels = n_scale_levels;
    // the counts start from zero inside the enqueued work: a replayed graph replays the memset
    if (n_in_view) MHIPCHK(hipMemsetAsync(n_in_view, 0, sizeof(int32_t) * nframes, m->stream));
    hipLaunchKernelGGL(k_frustum_batch, dim3((q_stride + 255) / 256, nframes), dim3(256), 0, m->stream, tcw, ow, nq, q_stride, skip, pw, normal,
                       min_dist, max_dist, q_shared ? 1 : 0, C, in_view, proj_x, proj_y, proj_xr, depth, level, view_cos, n_in_view);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

// ---- RGB-D frames: Frame::ComputeStereoFromRGBD and Frame::UnprojectStereo ----------------------------------
// the argument tests the host and the device form share; fills the kernel's parameter block
static int rgbd_params(const char* who, int first, int cap, int depth_type, int w, int h, int stride_bytes, float depth_factor, float mbf, RgbdParams& P) {
    if (depth_type != ORBM_DEPTH_U16 && depth_type != ORBM_DEPTH_F32) { set_merr("%s: unknown depth_type %d", who, depth_type); return ORBM_E_INVALID; }
    const int es = depth_type == ORBM_DEPTH_F32 ? 4 : 2;
    if (cap < 1 || w < 1 || h < 1 || first < 0) { set_merr("%s: cap, w and h must be >= 1 and first >= 0", who); return ORBM_E_INVALID; }
    if ((long long)stride_bytes < (long long)w * es || stride_bytes % es) {
        set_merr("%s: stride_bytes %d is below w * %d or not a multiple of the %d-byte element", who, stride_bytes, es, es);
        return ORBM_E_INVALID;
    }
    if (!std::isfinite(depth_factor)) { set_merr("%s: depth_factor is not finite", who); return ORBM_E_INVALID; }
    P.first = first; P.cap = cap; P.w = w; P.h = h; P.stride_bytes = stride_bytes;
    P.f32 = depth_type == ORBM_DEPTH_F32;
    P.scale = !P.f32 || std::fabs(depth_factor - 1.0f) > 1e-5;             // Tracking.cc:1353, the condition as written
    P.factor = depth_factor; P.mbf = mbf;
    return ORBM_OK;
}

int orbm_stereo_from_rgbd_batch_async(orbm_t* m, int nframes, int first, int cap,
                                      const orbm_kp_t* kps, const orbm_kp_t* kps_un, const int32_t* counts,
                                      const void* const* depth_imgs, int depth_type, int w, int h, int stride_bytes,
                                      float depth_factor, float mbf, float* uright, float* depth, int32_t* nvalid) {
    if (!m || !kps || !kps_un || !counts || !depth_imgs || !uright || !depth || !nvalid) {
        set_merr("ComputeStereoFromRGBD batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (nframes < 1) { set_merr("ComputeStereoFromRGBD batch: nframes must be >= 1"); return ORBM_E_INVALID; }
    RgbdParams P;
    const int rc = rgbd_params("ComputeStereoFromRGBD batch", first, cap, depth_type, w, h, stride_bytes, depth_factor, mbf, P);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    hipLaunchKernelGGL(k_rgbd_stereo, dim3(nframes), dim3(256), 0, m->stream, (const KpIn*)kps, (const KpIn*)kps_un, counts, depth_imgs, P,
                       uright, depth, nvalid);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_stereo_from_rgbd(orbm_t* m, int n, const orbm_kp_t* kps, const orbm_kp_t* kps_un,
                          const void* depth_img, int depth_type, int w, int h, int stride_bytes,
                          float depth_factor, float mbf, float* uright, float* depth) {
    if (!m || n < 0 || !depth_img || (n > 0 && (!kps || !kps_un || !uright || !depth))) {
        set_merr("ComputeStereoFromRGBD: a required array is NULL or n < 0");
        return ORBM_E_INVALID;
    }
    RgbdParams P;
    const int rc = rgbd_params("ComputeStereoFromRGBD", 0, std::max(n, 1), depth_type, w, h, stride_bytes, depth_factor, mbf, P);
    if (rc) return rc;
    if (n == 0) return 0;
    MHIPCHK(hipSetDevice(m->device));
    const size_t img_bytes = (size_t)(h - 1) * stride_bytes + (size_t)w * (P.f32 ? 4 : 2);   // the last row's padding is not the caller's to give
    const void* tab0 = nullptr;
    DevBuf dk, du, dc, dimg, dtab, dur, ddp, dnv;
    arena_reset(m);
    UP(dk, kps, sizeof(KpIn) * n);
    if (kps_un != kps) UP(du, kps_un, sizeof(KpIn) * n);
    UP(dc, &n, sizeof(int)); UP(dimg, depth_img, img_bytes); UP(dtab, &tab0, sizeof(void*));
    AL(dur, sizeof(float) * n); AL(ddp, sizeof(float) * n); AL(dnv, sizeof(int));
    const void* dev_img = dimg.ptr();                                       // the arena no longer moves: the table can name the image
    memcpy(m->arPin + dtab.off, &dev_img, sizeof(void*));
    ARENA_FLUSH(m);
    hipLaunchKernelGGL(k_rgbd_stereo, dim3(1), dim3(256), 0, m->stream, dk.as<KpIn>(), kps_un != kps ? du.as<KpIn>() : dk.as<KpIn>(), dc.as<int>(),
                       dtab.as<const void*>(), P, dur.as<float>(), ddp.as<float>(), dnv.as<int>());
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(uright, dur.host(), sizeof(float) * n); memcpy(depth, ddp.host(), sizeof(float) * n);
    return *(const int*)dnv.host();
}

int orbm_unproject_stereo_batch_async(orbm_t* m, int nrows, int first, int cap, const orbm_kp_t* kps_un, const int32_t* counts,
                                      const float* depth, const float* twc, const float* k_host, float* x3dw, uint8_t* has_depth) {
    if (!m || !kps_un || !counts || !depth || !twc || !k_host || !x3dw || !has_depth) {
        set_merr("UnprojectStereo batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (nrows < 1 || cap < 1 || first < 0) { set_merr("UnprojectStereo batch: nrows and cap must be >= 1 and first >= 0"); return ORBM_E_INVALID; }
    if (nrows > 65535) { set_merr("UnprojectStereo batch: %d rows in one call (at most 65535)", nrows); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    const UnprojParams P{first, cap, k_host[2], k_host[3], 1.0f / k_host[0], 1.0f / k_host[1]};   // invfx = 1.0f / fx (Frame.cc:301-302)
    hipLaunchKernelGGL(k_unproject_stereo, dim3((cap + 255) / 256, nrows), dim3(256), 0, m->stream, (const KpIn*)kps_un, counts, depth, twc, P,
                       x3dw, has_depth);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_unproject_stereo(orbm_t* m, int n, const orbm_kp_t* kps_un, const float* depth, const float* twc12, const float* k,
                          float* x3dw, uint8_t* has_depth) {
    if (!m || n < 0 || !twc12 || !k || (n > 0 && (!kps_un || !depth || !x3dw || !has_depth))) {
        set_merr("UnprojectStereo: a required array is NULL or n < 0");
        return ORBM_E_INVALID;
    }
    if (n == 0) return 0;
    MHIPCHK(hipSetDevice(m->device));
    DevBuf dk, dc, dd, dt, dx, dh;
    arena_reset(m);
    UP(dk, kps_un, sizeof(KpIn) * n); UP(dc, &n, sizeof(int)); UP(dd, depth, sizeof(float) * n); UP(dt, twc12, sizeof(float) * 12);
    AL(dx, sizeof(float) * 3 * n); AL(dh, n);
    ARENA_FLUSH(m);
    const UnprojParams P{0, n, k[2], k[3], 1.0f / k[0], 1.0f / k[1]};
    hipLaunchKernelGGL(k_unproject_stereo, dim3((n + 255) / 256, 1), dim3(256), 0, m->stream, dk.as<KpIn>(), dc.as<int>(), dd.as<float>(), dt.as<float>(), P,
                       dx.as<float>(), dh.as<uint8_t>());
    MHIPCHK(hipGetLastError());
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(x3dw, dx.host(), sizeof(float) * 3 * n); memcpy(has_depth, dh.host(), n);
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += has_depth[i] ? 1 : 0;
    return cnt;
}

// ---- Depth point selection: the sorted walk of Tracking::UpdateLastFrame / CreateNewKeyFrame and NeedNewKeyFrame's close counts ----
// the tests the host and the device form share; fills the kernel's parameter block (the thresholds as bit patterns: DepthSelParams)
static int depth_select_params(const char* who, int first, int cap, float th_depth, int max_points, DepthSelParams& P) {
    if (cap < 1 || first < 0 || max_points < 0) { set_merr("%s: cap must be >= 1, first and max_points >= 0", who); return ORBM_E_INVALID; }
    if (cap > ORBM_DEPTH_SELECT_MAX_CAP) {
        set_merr("%s: cap %d above %d (the row's 64-bit keys are sorted in LDS)", who, cap, (int)ORBM_DEPTH_SELECT_MAX_CAP);
        return ORBM_E_CAPACITY;
    }
    int n2 = 1;
    while (n2 < cap) n2 <<= 1;
    unsigned int tb;
    memcpy(&tb, &th_depth, sizeof(tb));
    const bool nan = std::isnan(th_depth), neg = (tb >> 31) != 0;           // -0.0f counts as negative: every positive depth is > it and none is < it
    P.first = first; P.cap = cap; P.n2 = n2; P.max_points = max_points;
    P.far_above = nan ? 0xFFFFFFFFu : neg ? 0u : tb;                         // depth > th on the bits of a positive depth; never with a NaN th
    P.close_below = (nan || neg) ? 0u : tb;                                  // depth < th likewise
    return ORBM_OK;
}

static int depth_select_launch(orbm_t* m, const char* who, int nrows, const int32_t* counts, const float* depth, const uint8_t* keeps_mp,
                               const uint8_t* tracked, const DepthSelParams& P, int32_t* order, uint8_t* create_new, int32_t* nvisit,
                               int32_t* ncreate, int32_t* nclose_tracked, int32_t* nclose_untracked) {
    if (!m->dselLds) {                                                       // once per handle, on its first (eager) call: the largest legal size
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(m->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) {
            set_merr("%s: inside a capture, run the call once eagerly first", who);
            return ORBM_E_HIP;
        }
        MHIPCHK(hipFuncSetAttribute((const void*)k_depth_select, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(ORBM_DEPTH_SELECT_MAX_CAP * sizeof(unsigned long long))));
        m->dselLds = true;
    }
    const int threads = std::min(1024, std::max(64, P.n2 / 2));              // one thread per pair of the bitonic network, whole waves
    hipLaunchKernelGGL(k_depth_select, dim3(nrows), dim3(threads), (size_t)P.n2 * sizeof(unsigned long long), m->stream, counts, depth, keeps_mp, tracked,
                       P, order, create_new, nvisit, ncreate, nclose_tracked, nclose_untracked);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_select_depth_points_batch_async(orbm_t* m, int nrows, int first, int cap, const int32_t* counts, const float* depth,
                                         const uint8_t* keeps_mp, const uint8_t* tracked, float th_depth, int max_points,
                                         int32_t* order, uint8_t* create_new, int32_t* nvisit, int32_t* ncreate,
                                         int32_t* nclose_tracked, int32_t* nclose_untracked) {
    if (!m || !counts || !depth || !order || !create_new || !nvisit || !ncreate) {
        set_merr("SelectDepthPoints batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (nrows < 1) { set_merr("SelectDepthPoints batch: nrows must be >= 1"); return ORBM_E_INVALID; }
    DepthSelParams P;
    const int rc = depth_select_params("SelectDepthPoints batch", first, cap, th_depth, max_points, P);
    if (rc) return rc;
    if (nrows > 65535) { set_merr("SelectDepthPoints batch: %d rows in one call (at most 65535)", nrows); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    return depth_select_launch(m, "SelectDepthPoints batch", nrows, counts, depth, keeps_mp, tracked, P, order, create_new, nvisit, ncreate,
                               nclose_tracked, nclose_untracked);
}

int orbm_select_depth_points(orbm_t* m, int n, const float* depth, const uint8_t* keeps_mp, const uint8_t* tracked, float th_depth, int max_points,
                             int32_t* order, uint8_t* create_new, int32_t* ncreate, int32_t* nclose_tracked, int32_t* nclose_untracked) {
    if (!m || n < 0 || (n > 0 && (!depth || !order || !create_new))) {
        set_merr("SelectDepthPoints: a required array is NULL or n < 0");
        return ORBM_E_INVALID;
    }
    DepthSelParams P;
    const int rc = depth_select_params("SelectDepthPoints", 0, std::max(n, 1), th_depth, max_points, P);
    if (rc) return rc;
    if (ncreate) *ncreate = 0;
    if (nclose_tracked) *nclose_tracked = 0;
    if (nclose_untracked) *nclose_untracked = 0;
    if (n == 0) return 0;
    MHIPCHK(hipSetDevice(m->device));
    DevBuf dc, dd, dk, dt, dord, dcn, dcnt;
    arena_reset(m);
    UP(dc, &n, sizeof(int)); UP(dd, depth, sizeof(float) * n);
    if (keeps_mp) UP(dk, keeps_mp, n);
    if (tracked) UP(dt, tracked, n);
    AL(dord, sizeof(int) * n); AL(dcn, n); AL(dcnt, sizeof(int) * 4);
    ARENA_FLUSH(m);
    int* cnt = dcnt.as<int>();
    const int rl = depth_select_launch(m, "SelectDepthPoints", 1, dc.as<int>(), dd.as<float>(), keeps_mp ? dk.as<uint8_t>() : nullptr,
                                       tracked ? dt.as<uint8_t>() : nullptr, P, dord.as<int>(), dcn.as<uint8_t>(), cnt, cnt + 1, cnt + 2, cnt + 3);
    if (rl) return rl;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(order, dord.host(), sizeof(int) * n); memcpy(create_new, dcn.host(), n);
    const int* hc = (const int*)dcnt.host();
    if (ncreate) *ncreate = hc[1];
    if (nclose_tracked) *nclose_tracked = hc[2];
    if (nclose_untracked) *nclose_untracked = hc[3];
    return hc[0];
}

int orbm_adopt_new_points_batch_async(orbm_t* m, int nrows, int first, int cap, const int32_t* counts, const uint8_t* create_new,
                                      const float* x3d_new, const uint8_t* desc, const uint8_t* outlier,
                                      float* x3dw, uint8_t* has_mp, uint8_t* mp_obs, uint8_t* qdesc) {
    if (!m || !counts || !create_new || !x3d_new || !desc || !x3dw || !has_mp || !mp_obs || !qdesc) {
        set_merr("AdoptNewPoints batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (nrows < 1 || cap < 1 || first < 0) { set_merr("AdoptNewPoints batch: nrows and cap must be >= 1 and first >= 0"); return ORBM_E_INVALID; }
    if (nrows > 65535) { set_merr("AdoptNewPoints batch: %d rows in one call (at most 65535)", nrows); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    hipLaunchKernelGGL(k_adopt_new_points, dim3((cap + 255) / 256, nrows), dim3(256), 0, m->stream, counts, first, cap, create_new, x3d_new, desc, outlier,
                       x3dw, has_mp, mp_obs, qdesc);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

// ---- MapPoint refresh: MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth -------------------------
// the argument tests the four entry points share; fills the observation block of the kernels
static int mp_obs_args(const char* who, int nmp, int nkf_rows, int cap, int nobs, const int32_t* obs_off, const int32_t* obs_row,
                       const int32_t* obs_slot, const uint8_t* obs_flags, const uint8_t* valid, MpObs& O) {
    if (!obs_off || !obs_row || !obs_slot || !obs_flags) { set_merr("%s: an observation array is NULL", who); return ORBM_E_INVALID; }
    if (nmp < 1 || nkf_rows < 1 || cap < 1 || nobs < 0) { set_merr("%s: nmp, nkf_rows and cap must be >= 1 and nobs >= 0", who); return ORBM_E_INVALID; }
    if (nmp > ORBM_MP_MAX_BATCH) { set_merr("%s: %d MapPoints in one call (at most %d)", who, nmp, (int)ORBM_MP_MAX_BATCH); return ORBM_E_CAPACITY; }
    if ((long long)nkf_rows * cap > INT_MAX) { set_merr("%s: %d rows of %d slots (the pool holds at most 2^31 - 1 slots)", who, nkf_rows, cap); return ORBM_E_CAPACITY; }
    O = MpObs{obs_off, obs_row, obs_slot, obs_flags, valid, nobs, nmp, nkf_rows, cap};
    return ORBM_OK;
}

int orbm_distinctive_descriptors_batch_async(orbm_t* m, int nmp, int nkf_rows, int cap, const uint8_t* desc_kf, const int32_t* counts_kf,
                                             int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                             const uint8_t* obs_flags, const uint8_t* valid,
                                             uint8_t* mp_desc, int32_t* best_obs, int32_t* best_median) {
    if (!m || !desc_kf || !counts_kf || !mp_desc || !best_obs) { set_merr("ComputeDistinctiveDescriptors batch: a required array is NULL"); return ORBM_E_INVALID; }
    MpObs O;
    const int rc = mp_obs_args("ComputeDistinctiveDescriptors batch", nmp, nkf_rows, cap, nobs, obs_off, obs_row, obs_slot, obs_flags, valid, O);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
#ifdef ORBX_AB
#define MP_PACKED(G) do { hipLaunchKernelGGL(k_mp_distinctive_packed<G>, dim3((unsigned)(((long long)nmp * G + 255) / 256)), dim3(256), 0, m->stream, desc_kf, counts_kf, O, mp_desc, best_obs, best_median); \
                          hipLaunchKernelGGL(k_mp_distinctive_long<G>, dim3((nmp + 3) / 4), dim3(256), 0, m->stream, desc_kf, counts_kf, O, mp_desc, best_obs, best_median); } while (0)
    const char* packed = ab_env("ORBM_MP_PACKED");                          // A/B: several MapPoints per wave in groups of 8, 16 or 32 lanes
    const int g = packed ? atoi(packed) : 0;
    if (g == 8) MP_PACKED(8);
    else if (g == 16) MP_PACKED(16);
    else if (g == 32) MP_PACKED(32);
    else
#endif
    hipLaunchKernelGGL(k_mp_distinctive, dim3((nmp + 3) / 4), dim3(256), 0, m->stream, desc_kf, counts_kf, O, mp_desc, best_obs, best_median);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_distinctive_descriptors(orbm_t* m, int nmp, int nkf_rows, int cap, const uint8_t* desc_kf, const int32_t* counts_kf,
                                 int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                 const uint8_t* obs_flags, const uint8_t* valid,
                                 uint8_t* mp_desc, int32_t* best_obs, int32_t* best_median) {
    if (!m || !desc_kf || !counts_kf || !mp_desc || !best_obs) { set_merr("ComputeDistinctiveDescriptors: a required array is NULL"); return ORBM_E_INVALID; }
    MpObs O;
    int rc = mp_obs_args("ComputeDistinctiveDescriptors", nmp, nkf_rows, cap, nobs, obs_off, obs_row, obs_slot, obs_flags, valid, O);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const size_t ne = (size_t)std::max(nobs, 1);
    DevBuf dd, dc, doff, drow, dslot, dfl, dv, dmp, dbo, dbm;
    arena_reset(m);
    UP(dd, desc_kf, (size_t)nkf_rows * cap * 32); UP(dc, counts_kf, sizeof(int) * nkf_rows); UP(doff, obs_off, sizeof(int) * ((size_t)nmp + 1));
    UP(drow, obs_row, sizeof(int) * ne * (nobs > 0)); UP(dslot, obs_slot, sizeof(int) * ne * (nobs > 0)); UP(dfl, obs_flags, ne * (nobs > 0));
    if (valid) UP(dv, valid, nmp);
    UPIO(dmp, mp_desc, (size_t)nmp * 32);                                    // in/out: a MapPoint without a winner keeps the caller's bytes
    AL(dbo, sizeof(int) * nmp); AL(dbm, sizeof(int) * nmp);
    ARENA_FLUSH(m);
    rc = orbm_distinctive_descriptors_batch_async(m, nmp, nkf_rows, cap, dd.as<uint8_t>(), dc.as<int32_t>(), nobs, doff.as<int32_t>(), drow.as<int32_t>(),
                                                  dslot.as<int32_t>(), dfl.as<uint8_t>(), valid ? dv.as<uint8_t>() : nullptr,
                                                  dmp.as<uint8_t>(), dbo.as<int32_t>(), dbm.as<int32_t>());
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(mp_desc, dmp.host(), (size_t)nmp * 32); memcpy(best_obs, dbo.host(), sizeof(int) * nmp);
    if (best_median) memcpy(best_median, dbm.host(), sizeof(int) * nmp);
    int cnt = 0;
    for (int i = 0; i < nmp; ++i) cnt += best_obs[i] >= 0 ? 1 : 0;
    return cnt;
}

int orbm_update_normal_and_depth_batch_async(orbm_t* m, int nmp, int nkf_rows, int cap, const orbm_kp_t* kps_kf, const int32_t* counts_kf,
                                             const float* ow_l, const float* ow_r,
                                             int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                             const uint8_t* obs_flags, const uint8_t* valid,
                                             const float* pw, const int32_t* ref_row, const int32_t* ref_slot, const float* scale_factors_host, int nlevels,
                                             float* normal, float* min_dist, float* max_dist, uint8_t* updated) {
    if (!m || !kps_kf || !counts_kf || !ow_l || !pw || !ref_row || !ref_slot || !scale_factors_host || !normal || !min_dist || !max_dist || !updated) {
        set_merr("UpdateNormalAndDepth batch: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (nlevels < 1) { set_merr("UpdateNormalAndDepth batch: nlevels must be >= 1"); return ORBM_E_INVALID; }
    if (nlevels > 12) { set_merr("UpdateNormalAndDepth batch: %d scale levels (the scale table holds 12)", nlevels); return ORBM_E_CAPACITY; }
    MpObs O;
    const int rc = mp_obs_args("UpdateNormalAndDepth batch", nmp, nkf_rows, cap, nobs, obs_off, obs_row, obs_slot, obs_flags, valid, O);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const MpNdParams P{nlevels, scale_tab(scale_factors_host, nlevels)};
    hipLaunchKernelGGL(k_mp_normal_depth, dim3((nmp + 255) / 256), dim3(256), 0, m->stream, (const KpIn*)kps_kf, counts_kf, ow_l, ow_r, O, pw, ref_row, ref_slot, P,
                       normal, min_dist, max_dist, updated);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_update_normal_and_depth(orbm_t* m, int nmp, int nkf_rows, int cap, const orbm_kp_t* kps_kf, const int32_t* counts_kf,
                                 const float* ow_l, const float* ow_r,
                                 int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                 const uint8_t* obs_flags, const uint8_t* valid,
                                 const float* pw, const int32_t* ref_row, const int32_t* ref_slot, const float* scale_factors, int nlevels,
                                 float* normal, float* min_dist, float* max_dist, uint8_t* updated) {
    if (!m || !kps_kf || !counts_kf || !ow_l || !pw || !ref_row || !ref_slot || !scale_factors || !normal || !min_dist || !max_dist || !updated) {
        set_merr("UpdateNormalAndDepth: a required array is NULL");
        return ORBM_E_INVALID;
    }
    if (nlevels < 1) { set_merr("UpdateNormalAndDepth: nlevels must be >= 1"); return ORBM_E_INVALID; }
    if (nlevels > 12) { set_merr("UpdateNormalAndDepth: %d scale levels (the scale table holds 12)", nlevels); return ORBM_E_CAPACITY; }
    MpObs O;
    int rc = mp_obs_args("UpdateNormalAndDepth", nmp, nkf_rows, cap, nobs, obs_off, obs_row, obs_slot, obs_flags, valid, O);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const size_t ne = (size_t)std::max(nobs, 1), nslots = (size_t)nkf_rows * cap;
    DevBuf dk, dc, dol, dor, doff, drow, dslot, dfl, dv, dpw, drr, drs, dn, dmin, dmax, dup;
    arena_reset(m);
    UP(dk, kps_kf, sizeof(KpIn) * nslots); UP(dc, counts_kf, sizeof(int) * nkf_rows); UP(dol, ow_l, sizeof(float) * 3 * nkf_rows);
    if (ow_r) UP(dor, ow_r, sizeof(float) * 3 * nkf_rows);
    UP(doff, obs_off, sizeof(int) * ((size_t)nmp + 1));
    UP(drow, obs_row, sizeof(int) * ne * (nobs > 0)); UP(dslot, obs_slot, sizeof(int) * ne * (nobs > 0)); UP(dfl, obs_flags, ne * (nobs > 0));
    if (valid) UP(dv, valid, nmp);
    UP(dpw, pw, sizeof(float) * 3 * nmp); UP(drr, ref_row, sizeof(int) * nmp); UP(drs, ref_slot, sizeof(int) * nmp);
    UPIO(dn, normal, sizeof(float) * 3 * nmp); UPIO(dmin, min_dist, sizeof(float) * nmp); UPIO(dmax, max_dist, sizeof(float) * nmp);   // rows not updated keep the caller's values
    AL(dup, nmp);
    ARENA_FLUSH(m);
    rc = orbm_update_normal_and_depth_batch_async(m, nmp, nkf_rows, cap, (const orbm_kp_t*)dk.as<KpIn>(), dc.as<int32_t>(), dol.as<float>(),
                                                  ow_r ? dor.as<float>() : nullptr, nobs, doff.as<int32_t>(), drow.as<int32_t>(), dslot.as<int32_t>(),
                                                  dfl.as<uint8_t>(), valid ? dv.as<uint8_t>() : nullptr, dpw.as<float>(), drr.as<int32_t>(), drs.as<int32_t>(),
                                                  scale_factors, nlevels, dn.as<float>(), dmin.as<float>(), dmax.as<float>(), dup.as<uint8_t>());
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(normal, dn.host(), sizeof(float) * 3 * nmp); memcpy(min_dist, dmin.host(), sizeof(float) * nmp); memcpy(max_dist, dmax.host(), sizeof(float) * nmp);
    memcpy(updated, dup.host(), nmp);
    int cnt = 0;
    for (int i = 0; i < nmp; ++i) cnt += updated[i] ? 1 : 0;
    return cnt;
}

// ---- KeyFrameDatabase queries: BowVector rows on the device, then DetectRelocalizationCandidates / DetectNBestCandidates up to the scores ----
int orbm_bow_vector_batch_async(orbm_t* m, const int32_t* word_id, const double* weight, const int32_t* counts, int nrows, int cap,
                                int32_t* bow_word, double* bow_val, int32_t* nbow) {
    if (!m || !word_id || !weight || !counts || !bow_word || !bow_val || !nbow) { set_merr("BowVector batch: a required array is NULL"); return ORBM_E_INVALID; }
    if (nrows < 1 || cap < 1) { set_merr("BowVector batch: nrows and cap must be >= 1"); return ORBM_E_INVALID; }
    if (cap > ORBM_BOWVEC_MAX_CAP) {
        set_merr("BowVector batch: cap %d above %d (the row's 64-bit keys are sorted in LDS)", cap, (int)ORBM_BOWVEC_MAX_CAP);
        return ORBM_E_CAPACITY;
    }
    if (nrows > 65535) { set_merr("BowVector batch: %d rows in one call (at most 65535)", nrows); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    if (!m->bowvLds) {                                                       // once per handle, on its first (eager) call: the largest legal size
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(m->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) {
            set_merr("BowVector batch: inside a capture, run the call once eagerly first");
            return ORBM_E_HIP;
        }
        MHIPCHK(hipFuncSetAttribute((const void*)k_bow_vector, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(ORBM_BOWVEC_MAX_CAP * sizeof(unsigned long long))));
        m->bowvLds = true;
    }
    int n2 = 1;
    while (n2 < cap) n2 <<= 1;
    const int threads = std::min(1024, std::max(64, n2 / 2));                // one thread per pair of the bitonic network, whole waves
    hipLaunchKernelGGL(k_bow_vector, dim3(nrows), dim3(threads), (size_t)n2 * sizeof(unsigned long long), m->stream, word_id, weight, counts, cap, n2,
                       bow_word, bow_val, nbow);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

// the argument tests the host and the device form share
static int kfdb_args(const char* who, orbm_t* m, int nq, const int32_t* q_row, int nq_rows, int q_cap, const int32_t* q_word, const double* q_val,
                     const int32_t* q_n, int ndb_rows, int db_cap, const int32_t* db_word, const double* db_val, const int32_t* db_n,
                     int32_t* common, int32_t* first_word, float* score, uint8_t* scored, int32_t* max_common, int32_t* min_common,
                     int32_t* nsharing, int32_t* nscored) {
    if (!m || !q_row || !q_word || !q_val || !q_n || !db_word || !db_val || !db_n || !common || !first_word || !score || !scored || !max_common ||
        !min_common || !nsharing || !nscored) {
        set_merr("%s: a required array is NULL", who);
        return ORBM_E_INVALID;
    }
    if (nq < 1 || nq_rows < 1 || q_cap < 1 || ndb_rows < 1 || db_cap < 1) {
        set_merr("%s: nq, nq_rows, q_cap, ndb_rows and db_cap must be >= 1", who);
        return ORBM_E_INVALID;
    }
    if (q_cap > 65535 || db_cap > 65535) { set_merr("%s: q_cap %d / db_cap %d above 65535", who, q_cap, db_cap); return ORBM_E_CAPACITY; }
    if (ndb_rows > ORBM_KFDB_MAX_ROWS) { set_merr("%s: %d database rows (at most %d)", who, ndb_rows, (int)ORBM_KFDB_MAX_ROWS); return ORBM_E_CAPACITY; }
    if (nq > ORBM_KFDB_MAX_QUERIES) { set_merr("%s: %d queries in one call (at most %d)", who, nq, (int)ORBM_KFDB_MAX_QUERIES); return ORBM_E_CAPACITY; }
    return ORBM_OK;
}

int orbm_kfdb_query_batch_async(orbm_t* m, int nq, const int32_t* q_row, int nq_rows, int q_cap, const int32_t* q_word, const double* q_val,
                                const int32_t* q_n, int ndb_rows, int db_cap, const int32_t* db_word, const double* db_val, const int32_t* db_n,
                                const uint8_t* db_active, const uint8_t* exclude, int32_t* common, int32_t* first_word, float* score,
                                uint8_t* scored, int32_t* max_common, int32_t* min_common, int32_t* nsharing, int32_t* nscored) {
    const int rc = kfdb_args("KeyFrameDatabase query batch", m, nq, q_row, nq_rows, q_cap, q_word, q_val, q_n, ndb_rows, db_cap, db_word, db_val, db_n,
                             common, first_word, score, scored, max_common, min_common, nsharing, nscored);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const KfdbParams P{nq, nq_rows, q_cap, ndb_rows, db_cap, q_row, q_word, q_val, q_n, db_word, db_val, db_n, db_active, exclude};
    // the three reduced rows start from zero inside the enqueued work: a replayed graph replays the memsets
    MHIPCHK(hipMemsetAsync(max_common, 0, sizeof(int32_t) * nq, m->stream));
    MHIPCHK(hipMemsetAsync(nsharing, 0, sizeof(int32_t) * nq, m->stream));
    MHIPCHK(hipMemsetAsync(nscored, 0, sizeof(int32_t) * nq, m->stream));
    const dim3 grid((ndb_rows + 3) / 4, nq);
    hipLaunchKernelGGL(k_kfdb_common, grid, dim3(256), 0, m->stream, P, common, first_word, max_common, nsharing);
    MHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_kfdb_score, grid, dim3(256), 0, m->stream, P, common, max_common, score, scored, min_common, nscored);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_kfdb_query(orbm_t* m, int nq, const int32_t* q_row, int nq_rows, int q_cap, const int32_t* q_word, const double* q_val,
                    const int32_t* q_n, int ndb_rows, int db_cap, const int32_t* db_word, const double* db_val, const int32_t* db_n,
                    const uint8_t* db_active, const uint8_t* exclude, int32_t* common, int32_t* first_word, float* score,
                    uint8_t* scored, int32_t* max_common, int32_t* min_common, int32_t* nsharing, int32_t* nscored) {
    int rc = kfdb_args("KeyFrameDatabase query", m, nq, q_row, nq_rows, q_cap, q_word, q_val, q_n, ndb_rows, db_cap, db_word, db_val, db_n,
                       common, first_word, score, scored, max_common, min_common, nsharing, nscored);
    if (rc) return rc;
    for (int q = 0; q < nq; ++q)
        if (q_row[q] < 0 || q_row[q] >= nq_rows) { set_merr("KeyFrameDatabase query: q_row[%d] = %d outside [0, %d)", q, q_row[q], nq_rows); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(m->device));
    const size_t nqs = (size_t)nq_rows * q_cap, nds = (size_t)ndb_rows * db_cap, nout = (size_t)nq * ndb_rows;
    const bool same = q_word == db_word && q_val == db_val && q_n == db_n && nq_rows == ndb_rows && q_cap == db_cap;   // one pool: one upload
    DevBuf dqr, dqw, dqv, dqn, dw, dv, dn, da, dx, dcnt, dcom, dfw, dsc, dsd;
    arena_reset(m);
    UP(dqr, q_row, sizeof(int32_t) * nq);
    UP(dw, db_word, sizeof(int32_t) * nds); UP(dv, db_val, sizeof(double) * nds); UP(dn, db_n, sizeof(int32_t) * ndb_rows);
    if (!same) { UP(dqw, q_word, sizeof(int32_t) * nqs); UP(dqv, q_val, sizeof(double) * nqs); UP(dqn, q_n, sizeof(int32_t) * nq_rows); }
    if (db_active) UP(da, db_active, ndb_rows);
    if (exclude) UP(dx, exclude, nout);
    AL(dcnt, sizeof(int32_t) * 4 * nq); AL(dcom, sizeof(int32_t) * nout); AL(dfw, sizeof(int32_t) * nout); AL(dsc, sizeof(float) * nout); AL(dsd, nout);
    ARENA_FLUSH(m);
    int32_t* cnt = dcnt.as<int32_t>();
    rc = orbm_kfdb_query_batch_async(m, nq, dqr.as<int32_t>(), nq_rows, q_cap, same ? dw.as<int32_t>() : dqw.as<int32_t>(),
                                     same ? dv.as<double>() : dqv.as<double>(), same ? dn.as<int32_t>() : dqn.as<int32_t>(), ndb_rows, db_cap,
                                     dw.as<int32_t>(), dv.as<double>(), dn.as<int32_t>(), db_active ? da.as<uint8_t>() : nullptr,
                                     exclude ? dx.as<uint8_t>() : nullptr, dcom.as<int32_t>(), dfw.as<int32_t>(), dsc.as<float>(), dsd.as<uint8_t>(),
                                     cnt, cnt + nq, cnt + 2 * (size_t)nq, cnt + 3 * (size_t)nq);
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(common, dcom.host(), sizeof(int32_t) * nout); memcpy(first_word, dfw.host(), sizeof(int32_t) * nout);
    memcpy(score, dsc.host(), sizeof(float) * nout); memcpy(scored, dsd.host(), nout);
    const int32_t* hc = (const int32_t*)dcnt.host();
    memcpy(max_common, hc, sizeof(int32_t) * nq); memcpy(min_common, hc + nq, sizeof(int32_t) * nq);
    memcpy(nsharing, hc + 2 * (size_t)nq, sizeof(int32_t) * nq); memcpy(nscored, hc + 3 * (size_t)nq, sizeof(int32_t) * nq);
    return ORBM_OK;
}

// ---- KeyFrameCulling: LocalMapping::KeyFrameCulling's redundancy counts over the pool and the CSR of the MapPoint refresh ----
// the argument tests the host and the device form share; fills the observation block of the kernel
static int kfcull_args(const char* who, orbm_t* m, int ncand, const int32_t* cand_row, int nkf_rows, int cap, const orbm_kp_t* kps_kf,
                       const int32_t* counts_kf, const int32_t* kf_mp, int nmp, int nobs, const int32_t* obs_off, const int32_t* obs_row,
                       const int32_t* obs_slot, const uint8_t* obs_flags, const uint8_t* mp_valid, const int32_t* mp_nobs, int th_obs,
                       int32_t* n_mps, int32_t* n_redundant, uint8_t* cull, MpObs& O) {
    if (!m) {                                                                // no handle: orbm_create has refused, for want of a device or of a call
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_merr("%s: no HIP device: the MI355X matcher has no CPU fallback", who); return ORBM_E_HIP; }
        set_merr("%s: the handle is NULL", who);
        return ORBM_E_INVALID;
    }
    const struct { const void* p; const char* name; } req[] = {
        {cand_row, "cand_row"}, {kps_kf, "kps_kf"}, {counts_kf, "counts_kf"}, {kf_mp, "kf_mp"}, {obs_off, "obs_off"}, {obs_row, "obs_row"},
        {obs_slot, "obs_slot"}, {obs_flags, "obs_flags"}, {mp_nobs, "mp_nobs"}, {n_mps, "n_mps"}, {n_redundant, "n_redundant"}, {cull, "cull"}};
    for (const auto& r : req)
        if (!r.p) { set_merr("%s: %s is NULL", who, r.name); return ORBM_E_INVALID; }
    if (ncand < 1) { set_merr("%s: ncand %d must be >= 1", who, ncand); return ORBM_E_INVALID; }
    if (th_obs < 0) { set_merr("%s: th_obs %d must be >= 0", who, th_obs); return ORBM_E_INVALID; }
    if (nmp < 1 || nkf_rows < 1 || cap < 1 || nobs < 0) { set_merr("%s: nmp, nkf_rows and cap must be >= 1 and nobs >= 0", who); return ORBM_E_INVALID; }
    if (ncand > ORBM_KFCULL_MAX_CAND) { set_merr("%s: %d candidates in one call (at most %d)", who, ncand, (int)ORBM_KFCULL_MAX_CAND); return ORBM_E_CAPACITY; }
    if (cap > ORBM_KFCULL_MAX_CAP) { set_merr("%s: cap %d above %d", who, cap, (int)ORBM_KFCULL_MAX_CAP); return ORBM_E_CAPACITY; }
    return mp_obs_args(who, nmp, nkf_rows, cap, nobs, obs_off, obs_row, obs_slot, obs_flags, mp_valid, O);
}

int orbm_keyframe_culling_batch_async(orbm_t* m, int ncand, const int32_t* cand_row, int nkf_rows, int cap, const orbm_kp_t* kps_kf,
                                      const int32_t* counts_kf, const int32_t* kf_mp, const float* depth, float th_depth, int nmp, int nobs,
                                      const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot, const uint8_t* obs_flags,
                                      const uint8_t* mp_valid, const int32_t* mp_nobs, const uint8_t* erased, int th_obs, float redundant_th,
                                      int32_t* n_mps, int32_t* n_redundant, uint8_t* cull, uint8_t* slot_state, int32_t* first_cull) {
    MpObs O;
    const int rc = kfcull_args("KeyFrameCulling batch", m, ncand, cand_row, nkf_rows, cap, kps_kf, counts_kf, kf_mp, nmp, nobs, obs_off, obs_row,
                               obs_slot, obs_flags, mp_valid, mp_nobs, th_obs, n_mps, n_redundant, cull, O);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const KfcullParams P{ncand, th_obs, th_depth, cand_row, (const KpIn*)kps_kf, counts_kf, kf_mp, depth, mp_nobs, erased};
    // the two count rows start from zero inside the enqueued work: a replayed graph replays the memsets
    MHIPCHK(hipMemsetAsync(n_mps, 0, sizeof(int32_t) * ncand, m->stream));
    MHIPCHK(hipMemsetAsync(n_redundant, 0, sizeof(int32_t) * ncand, m->stream));
    hipLaunchKernelGGL(k_kfcull, dim3((cap + 15) / 16, ncand), dim3(256), 0, m->stream, P, O, n_mps, n_redundant, slot_state);
    MHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_kfcull_finish, dim3(1), dim3(1024), 0, m->stream, ncand, n_mps, n_redundant, redundant_th, cull, first_cull);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_keyframe_culling(orbm_t* m, int ncand, const int32_t* cand_row, int nkf_rows, int cap, const orbm_kp_t* kps_kf,
                          const int32_t* counts_kf, const int32_t* kf_mp, const float* depth, float th_depth, int nmp, int nobs,
                          const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot, const uint8_t* obs_flags,
                          const uint8_t* mp_valid, const int32_t* mp_nobs, const uint8_t* erased, int th_obs, float redundant_th,
                          int32_t* n_mps, int32_t* n_redundant, uint8_t* cull, uint8_t* slot_state, int32_t* first_cull) {
    MpObs O;
    int rc = kfcull_args("KeyFrameCulling", m, ncand, cand_row, nkf_rows, cap, kps_kf, counts_kf, kf_mp, nmp, nobs, obs_off, obs_row, obs_slot,
                         obs_flags, mp_valid, mp_nobs, th_obs, n_mps, n_redundant, cull, O);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const size_t ne = (size_t)std::max(nobs, 1), nslots = (size_t)nkf_rows * cap, ncs = (size_t)ncand * cap;
    DevBuf dcr, dk, dc, dkm, dd, doff, drow, dslot, dfl, dv, dno, de, dcnt, dcu, dss;
    arena_reset(m);
    UP(dcr, cand_row, sizeof(int32_t) * ncand); UP(dk, kps_kf, sizeof(KpIn) * nslots); UP(dc, counts_kf, sizeof(int32_t) * nkf_rows);
    UP(dkm, kf_mp, sizeof(int32_t) * ncs);
    if (depth) UP(dd, depth, sizeof(float) * ncs);
    UP(doff, obs_off, sizeof(int32_t) * ((size_t)nmp + 1));
    UP(drow, obs_row, sizeof(int32_t) * ne * (nobs > 0)); UP(dslot, obs_slot, sizeof(int32_t) * ne * (nobs > 0)); UP(dfl, obs_flags, ne * (nobs > 0));
    if (mp_valid) UP(dv, mp_valid, nmp);
    UP(dno, mp_nobs, sizeof(int32_t) * nmp);
    if (erased) UP(de, erased, nkf_rows);
    AL(dcnt, sizeof(int32_t) * (2 * (size_t)ncand + 1)); AL(dcu, ncand);
    if (slot_state) AL(dss, ncs);
    ARENA_FLUSH(m);
    int32_t* cnt = dcnt.as<int32_t>();
    rc = orbm_keyframe_culling_batch_async(m, ncand, dcr.as<int32_t>(), nkf_rows, cap, (const orbm_kp_t*)dk.as<KpIn>(), dc.as<int32_t>(), dkm.as<int32_t>(),
                                           depth ? dd.as<float>() : nullptr, th_depth, nmp, nobs, doff.as<int32_t>(), drow.as<int32_t>(),
                                           dslot.as<int32_t>(), dfl.as<uint8_t>(), mp_valid ? dv.as<uint8_t>() : nullptr, dno.as<int32_t>(),
                                           erased ? de.as<uint8_t>() : nullptr, th_obs, redundant_th, cnt, cnt + ncand, dcu.as<uint8_t>(),
                                           slot_state ? dss.as<uint8_t>() : nullptr, cnt + 2 * (size_t)ncand);
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    const int32_t* hc = (const int32_t*)dcnt.host();
    memcpy(n_mps, hc, sizeof(int32_t) * ncand); memcpy(n_redundant, hc + ncand, sizeof(int32_t) * ncand);
    memcpy(cull, dcu.host(), ncand);
    if (slot_state) memcpy(slot_state, dss.host(), ncs);
    if (first_cull) *first_cull = hc[2 * (size_t)ncand];
    int n = 0;
    for (int k = 0; k < ncand; ++k) n += cull[k] ? 1 : 0;
    return n;
}


// ---- Covisibility votes, local map points and their gather: KeyFrame::UpdateConnections step 1, Tracking::UpdateLocalKeyFrames' vote,
// Tracking::UpdateLocalPoints and the query rows of SearchLocalPoints, over the pool and the CSR of the MapPoint refresh ----
static int covis_handle(const char* who, orbm_t* m) {
    if (m) return ORBM_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_merr("%s: no HIP device: the MI355X matcher has no CPU fallback", who); return ORBM_E_HIP; }
    set_merr("%s: the handle is NULL", who);
    return ORBM_E_INVALID;
}

// the argument tests the host and the device form share; fills the observation block of the kernel
static int covis_args(const char* who, orbm_t* m, int nq, int q_stride, const int32_t* q_mp, const int32_t* q_n, int nkf_rows, int cap,
                      const int32_t* counts_kf, int nmp, int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                      const uint8_t* obs_flags, const uint8_t* mp_valid, int list_cap, int32_t* votes, int32_t* n_voted, int32_t* max_votes,
                      int32_t* n_over, int32_t* list_row, int32_t* list_votes, MpObs& O) {
    if (const int rc = covis_handle(who, m)) return rc;
    const struct { const void* p; const char* name; } req[] = {
        {q_mp, "q_mp"}, {q_n, "q_n"}, {counts_kf, "counts_kf"}, {obs_off, "obs_off"}, {obs_row, "obs_row"}, {obs_slot, "obs_slot"},
        {obs_flags, "obs_flags"}, {votes, "votes"}, {n_voted, "n_voted"}, {max_votes, "max_votes"}, {n_over, "n_over"}};
    for (const auto& r : req)
        if (!r.p) { set_merr("%s: %s is NULL", who, r.name); return ORBM_E_INVALID; }
    if (nq < 1 || q_stride < 1) { set_merr("%s: nq %d and q_stride %d must be >= 1", who, nq, q_stride); return ORBM_E_INVALID; }
    if (list_cap < 0 || (list_cap > 0 && (!list_row || !list_votes))) { set_merr("%s: list_cap %d needs list_row and list_votes", who, list_cap); return ORBM_E_INVALID; }
    if (nmp < 1 || nkf_rows < 1 || cap < 1 || nobs < 0) { set_merr("%s: nmp, nkf_rows and cap must be >= 1 and nobs >= 0", who); return ORBM_E_INVALID; }
    if (nq > ORBM_COVIS_MAX_QUERIES || q_stride > ORBM_COVIS_MAX_SLOTS) {
        set_merr("%s: %d queries of %d slots (at most %d of %d)", who, nq, q_stride, (int)ORBM_COVIS_MAX_QUERIES, (int)ORBM_COVIS_MAX_SLOTS);
        return ORBM_E_CAPACITY;
    }
    if (nkf_rows > ORBM_COVIS_MAX_ROWS) { set_merr("%s: %d pool rows (at most %d)", who, nkf_rows, (int)ORBM_COVIS_MAX_ROWS); return ORBM_E_CAPACITY; }
    if ((long long)nq * nkf_rows > ORBM_COVIS_MAX_VOTES) { set_merr("%s: %d queries x %d rows of votes (at most 2^28)", who, nq, nkf_rows); return ORBM_E_CAPACITY; }
    return mp_obs_args(who, nmp, nkf_rows, cap, nobs, obs_off, obs_row, obs_slot, obs_flags, mp_valid, O);
}

int orbm_covisibility_votes_batch_async(orbm_t* m, int nq, int q_stride, const int32_t* q_mp, const int32_t* q_n, const int32_t* self_row,
                                        int nkf_rows, int cap, const int32_t* counts_kf, const uint8_t* kf_skip, int skip_bad,
                                        int nmp, int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                        const uint8_t* obs_flags, const uint8_t* mp_valid, int th, int list_cap,
                                        int32_t* votes, int32_t* n_voted, int32_t* max_votes, int32_t* n_over, int32_t* list_row, int32_t* list_votes) {
    MpObs O;
    const int rc = covis_args("CovisibilityVotes batch", m, nq, q_stride, q_mp, q_n, nkf_rows, cap, counts_kf, nmp, nobs, obs_off, obs_row, obs_slot,
                              obs_flags, mp_valid, list_cap, votes, n_voted, max_votes, n_over, list_row, list_votes, O);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const CovisParams P{q_stride, skip_bad ? 1 : 0, q_mp, q_n, self_row, counts_kf, kf_skip};
    // the vote rows start from zero inside the enqueued work: a replayed graph replays the memsets
    MHIPCHK(hipMemsetAsync(votes, 0, sizeof(int32_t) * (size_t)nq * nkf_rows, m->stream));
    MHIPCHK(hipMemsetAsync(n_voted, 0, sizeof(int32_t) * nq, m->stream));
    MHIPCHK(hipMemsetAsync(max_votes, 0, sizeof(int32_t) * nq, m->stream));
    MHIPCHK(hipMemsetAsync(n_over, 0, sizeof(int32_t) * nq, m->stream));
    const dim3 grid((q_stride + COVIS_WG_SLOTS - 1) / COVIS_WG_SLOTS, nq);
#ifdef ORBX_AB
    if (ab_env("ORBM_COVIS_PLAIN"))                                         // A/B: one global atomicAdd per vote
        hipLaunchKernelGGL(k_covis_votes<false>, grid, dim3(256), 0, m->stream, P, O, votes);
    else
#endif
    hipLaunchKernelGGL(k_covis_votes<true>, grid, dim3(256), 0, m->stream, P, O, votes);
    MHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_covis_finish, dim3(nq), dim3(1024), 0, m->stream, nkf_rows, th, list_cap, votes, n_voted, max_votes, n_over, list_row, list_votes);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_covisibility_votes(orbm_t* m, int nq, int q_stride, const int32_t* q_mp, const int32_t* q_n, const int32_t* self_row,
                            int nkf_rows, int cap, const int32_t* counts_kf, const uint8_t* kf_skip, int skip_bad,
                            int nmp, int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                            const uint8_t* obs_flags, const uint8_t* mp_valid, int th, int list_cap,
                            int32_t* votes, int32_t* n_voted, int32_t* max_votes, int32_t* n_over, int32_t* list_row, int32_t* list_votes) {
    MpObs O;
    int rc = covis_args("CovisibilityVotes", m, nq, q_stride, q_mp, q_n, nkf_rows, cap, counts_kf, nmp, nobs, obs_off, obs_row, obs_slot, obs_flags,
                        mp_valid, list_cap, votes, n_voted, max_votes, n_over, list_row, list_votes, O);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const size_t ne = (size_t)std::max(nobs, 1), nv = (size_t)nq * nkf_rows, nl = (size_t)nq * list_cap;
    DevBuf dqm, dqn, dself, dc, dks, doff, drow, dslot, dfl, dv, dcnt, dvotes, dlr, dlv;
    arena_reset(m);
    UP(dqm, q_mp, sizeof(int32_t) * (size_t)nq * q_stride); UP(dqn, q_n, sizeof(int32_t) * nq);
    if (self_row) UP(dself, self_row, sizeof(int32_t) * nq);
    UP(dc, counts_kf, sizeof(int32_t) * nkf_rows);
    if (kf_skip) UP(dks, kf_skip, nkf_rows);
    UP(doff, obs_off, sizeof(int32_t) * ((size_t)nmp + 1));
    UP(drow, obs_row, sizeof(int32_t) * ne * (nobs > 0)); UP(dslot, obs_slot, sizeof(int32_t) * ne * (nobs > 0)); UP(dfl, obs_flags, ne * (nobs > 0));
    if (mp_valid) UP(dv, mp_valid, nmp);
    AL(dcnt, sizeof(int32_t) * 3 * (size_t)nq); AL(dvotes, sizeof(int32_t) * nv);
    if (list_cap > 0) { AL(dlr, sizeof(int32_t) * nl); AL(dlv, sizeof(int32_t) * nl); }
    ARENA_FLUSH(m);
    int32_t* cnt = dcnt.as<int32_t>();
    rc = orbm_covisibility_votes_batch_async(m, nq, q_stride, dqm.as<int32_t>(), dqn.as<int32_t>(), self_row ? dself.as<int32_t>() : nullptr, nkf_rows, cap,
                                             dc.as<int32_t>(), kf_skip ? dks.as<uint8_t>() : nullptr, skip_bad, nmp, nobs, doff.as<int32_t>(),
                                             drow.as<int32_t>(), dslot.as<int32_t>(), dfl.as<uint8_t>(), mp_valid ? dv.as<uint8_t>() : nullptr, th, list_cap,
                                             dvotes.as<int32_t>(), cnt, cnt + nq, cnt + 2 * (size_t)nq, list_cap > 0 ? dlr.as<int32_t>() : nullptr,
                                             list_cap > 0 ? dlv.as<int32_t>() : nullptr);
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    const int32_t* hc = (const int32_t*)dcnt.host();
    memcpy(n_voted, hc, sizeof(int32_t) * nq); memcpy(max_votes, hc + nq, sizeof(int32_t) * nq); memcpy(n_over, hc + 2 * (size_t)nq, sizeof(int32_t) * nq);
    memcpy(votes, dvotes.host(), sizeof(int32_t) * nv);
    for (int q = 0; q < nq && list_cap > 0; ++q) {                           // the rest of a list row keeps the caller's bytes
        const size_t n = (size_t)std::min(n_voted[q], list_cap), o = (size_t)q * list_cap;
        memcpy(list_row + o, (const int32_t*)dlr.host() + o, sizeof(int32_t) * n); memcpy(list_votes + o, (const int32_t*)dlv.host() + o, sizeof(int32_t) * n);
    }
    return ORBM_OK;
}

static int lp_args(const char* who, orbm_t* m, int T, int lkf_stride, const int32_t* lkf_row, const int32_t* n_lkf, int nkf_rows, int cap,
                   const int32_t* counts_kf, const int32_t* kf_mp, int nmp, int q_stride, int32_t* local_mp, int32_t* n_total, int32_t* nq) {
    if (const int rc = covis_handle(who, m)) return rc;
    const struct { const void* p; const char* name; } req[] = {
        {lkf_row, "lkf_row"}, {n_lkf, "n_lkf"}, {counts_kf, "counts_kf"}, {kf_mp, "kf_mp"}, {local_mp, "local_mp"}, {n_total, "n_total"}, {nq, "nq"}};
    for (const auto& r : req)
        if (!r.p) { set_merr("%s: %s is NULL", who, r.name); return ORBM_E_INVALID; }
    if (T < 1 || lkf_stride < 1 || nkf_rows < 1 || cap < 1 || nmp < 1 || q_stride < 1) {
        set_merr("%s: T, lkf_stride, nkf_rows, cap, nmp and q_stride must be >= 1", who);
        return ORBM_E_INVALID;
    }
    if (T > ORBM_LOCALPTS_MAX_FRAMES || lkf_stride > ORBM_LOCALPTS_MAX_KFS || cap > ORBM_LOCALPTS_MAX_CAP) {
        set_merr("%s: %d frames of %d KeyFrames of %d slots (at most %d, %d, %d)", who, T, lkf_stride, cap, (int)ORBM_LOCALPTS_MAX_FRAMES,
                 (int)ORBM_LOCALPTS_MAX_KFS, (int)ORBM_LOCALPTS_MAX_CAP);
        return ORBM_E_CAPACITY;
    }
    if ((long long)lkf_stride * cap > INT_MAX) { set_merr("%s: %d x %d positions (the key holds 2^31 - 1)", who, lkf_stride, cap); return ORBM_E_CAPACITY; }
    if (nmp > ORBM_MP_MAX_BATCH) { set_merr("%s: %d MapPoints in one call (at most %d)", who, nmp, (int)ORBM_MP_MAX_BATCH); return ORBM_E_CAPACITY; }
    if ((long long)T * nmp > ORBM_COVIS_MAX_VOTES) { set_merr("%s: %d frames x %d MapPoints of first positions (at most 2^28)", who, T, nmp); return ORBM_E_CAPACITY; }
    return ORBM_OK;
}

int orbm_local_points_batch_async(orbm_t* m, int T, int lkf_stride, const int32_t* lkf_row, const int32_t* n_lkf, int nkf_rows, int cap,
                                  const int32_t* counts_kf, const int32_t* kf_mp, int nmp, const uint8_t* mp_valid, int q_stride,
                                  int32_t* local_mp, int32_t* n_total, int32_t* nq) {
    const int rc = lp_args("LocalPoints batch", m, T, lkf_stride, lkf_row, n_lkf, nkf_rows, cap, counts_kf, kf_mp, nmp, q_stride, local_mp, n_total, nq);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const unsigned npos = (unsigned)lkf_stride * (unsigned)cap;
    const int nchunks = (int)((npos + LP_CHUNK - 1) / LP_CHUNK);
    const size_t bFirst = (sizeof(unsigned) * (size_t)T * nmp + 255) & ~(size_t)255, bCnt = sizeof(int) * (size_t)T * nchunks;
    uint8_t* scr = batch_scratch(m, bFirst + bCnt);
    if (!scr) { set_merr("LocalPoints scratch of %zu B unavailable (inside a capture, run the call once eagerly first)", bFirst + bCnt); return ORBM_E_HIP; }
    unsigned* first_pos = (unsigned*)scr;
    int* chunk = (int*)(scr + bFirst);
    const LpParams P{lkf_stride, nkf_rows, cap, nmp, nchunks, lkf_row, n_lkf, counts_kf, kf_mp, mp_valid};
    MHIPCHK(hipMemsetAsync(first_pos, 0xFF, sizeof(unsigned) * (size_t)T * nmp, m->stream));
    hipLaunchKernelGGL(k_lp_mark, dim3((npos + 255) / 256, T), dim3(256), 0, m->stream, P, npos, first_pos);
    MHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_lp_count, dim3(nchunks, T), dim3(256), 0, m->stream, P, npos, first_pos, chunk);
    MHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_lp_scan, dim3(T), dim3(1024), 0, m->stream, nchunks, q_stride, chunk, n_total, nq);
    MHIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_lp_write, dim3(nchunks, T), dim3(256), 0, m->stream, P, npos, first_pos, chunk, q_stride, local_mp);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_local_points(orbm_t* m, int T, int lkf_stride, const int32_t* lkf_row, const int32_t* n_lkf, int nkf_rows, int cap,
                      const int32_t* counts_kf, const int32_t* kf_mp, int nmp, const uint8_t* mp_valid, int q_stride,
                      int32_t* local_mp, int32_t* n_total, int32_t* nq) {
    int rc = lp_args("LocalPoints", m, T, lkf_stride, lkf_row, n_lkf, nkf_rows, cap, counts_kf, kf_mp, nmp, q_stride, local_mp, n_total, nq);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    DevBuf dl, dn, dc, dkm, dv, dcnt, dout;
    arena_reset(m);
    UP(dl, lkf_row, sizeof(int32_t) * (size_t)T * lkf_stride); UP(dn, n_lkf, sizeof(int32_t) * T); UP(dc, counts_kf, sizeof(int32_t) * nkf_rows);
    UP(dkm, kf_mp, sizeof(int32_t) * (size_t)nkf_rows * cap);
    if (mp_valid) UP(dv, mp_valid, nmp);
    AL(dcnt, sizeof(int32_t) * 2 * (size_t)T); AL(dout, sizeof(int32_t) * (size_t)T * q_stride);
    ARENA_FLUSH(m);
    int32_t* cnt = dcnt.as<int32_t>();
    rc = orbm_local_points_batch_async(m, T, lkf_stride, dl.as<int32_t>(), dn.as<int32_t>(), nkf_rows, cap, dc.as<int32_t>(), dkm.as<int32_t>(), nmp,
                                       mp_valid ? dv.as<uint8_t>() : nullptr, q_stride, dout.as<int32_t>(), cnt, cnt + T);
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    const int32_t* hc = (const int32_t*)dcnt.host();
    memcpy(n_total, hc, sizeof(int32_t) * T); memcpy(nq, hc + T, sizeof(int32_t) * T);
    for (int f = 0; f < T; ++f)                                              // slots at and beyond nq keep the caller's bytes
        memcpy(local_mp + (size_t)f * q_stride, (const int32_t*)dout.host() + (size_t)f * q_stride, sizeof(int32_t) * (size_t)std::max(nq[f], 0));
    return ORBM_OK;
}

int orbm_gather_map_points_batch_async(orbm_t* m, int T, int q_stride, const int32_t* local_mp, const int32_t* nq, int nmp,
                                       const float* mp_pw, const float* mp_normal, const float* mp_min_dist, const float* mp_max_dist,
                                       const uint8_t* mp_desc, const int32_t* mp_nobs, const uint8_t* mp_skip,
                                       float* pw, float* normal, float* min_dist, float* max_dist, uint8_t* qdesc, uint8_t* mp_obs, uint8_t* skip) {
    const char* who = "GatherMapPoints batch";
    if (const int rc = covis_handle(who, m)) return rc;
    if (!local_mp || !nq) { set_merr("%s: local_mp or nq is NULL", who); return ORBM_E_INVALID; }
    if (T < 1 || q_stride < 1 || nmp < 1) { set_merr("%s: T, q_stride and nmp must be >= 1", who); return ORBM_E_INVALID; }
    if (T > ORBM_LOCALPTS_MAX_FRAMES) { set_merr("%s: %d frames in one call (at most %d)", who, T, (int)ORBM_LOCALPTS_MAX_FRAMES); return ORBM_E_CAPACITY; }
    if (nmp > ORBM_MP_MAX_BATCH) { set_merr("%s: %d MapPoints (at most %d)", who, nmp, (int)ORBM_MP_MAX_BATCH); return ORBM_E_CAPACITY; }
    if ((((uintptr_t)mp_desc) | ((uintptr_t)qdesc)) & 15) { set_merr("%s: mp_desc and qdesc must be 16-byte aligned", who); return ORBM_E_INVALID; }
    MHIPCHK(hipSetDevice(m->device));
    const GatherMpParams P{q_stride, nmp, local_mp, nq, mp_pw, mp_normal, mp_min_dist, mp_max_dist, mp_desc, mp_nobs, mp_skip,
                           pw, normal, min_dist, max_dist, qdesc, mp_obs, skip};
    hipLaunchKernelGGL(k_gather_map_points, dim3((q_stride + 255) / 256, T), dim3(256), 0, m->stream, P);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

// ---- Pose optimisation and the bookkeeping around it: Optimizer::PoseOptimization(Frame*) and the discard loops of Tracking ----
// the argument tests the host and the device form share; fills the kernel's parameter block (rows still unset)
static int poseopt_args(const char* who, orbm_t* m, int nframes, int first, int cap, const orbm_kp_t* kps_un, const int32_t* counts,
                        const int32_t* q_mp, int nmp, const float* mp_pw, const float* tcw_in, const float* k_host, float bf,
                        const float* ils2_host, int nlevels, float* tcw_out, uint8_t* outlier, int32_t* n_corr, int32_t* n_good, PoseOptParams& P) {
    if (const int rc = covis_handle(who, m)) return rc;
    const struct { const void* p; const char* name; } req[] = {
        {kps_un, "kps_un"}, {counts, "counts"}, {q_mp, "q_mp"}, {mp_pw, "mp_pw"}, {tcw_in, "tcw_in"}, {k_host, "k_host"},
        {ils2_host, "inv_level_sigma2_host"}, {tcw_out, "tcw_out"}, {outlier, "outlier"}, {n_corr, "n_corr"}, {n_good, "n_good"}};
    for (const auto& r : req)
        if (!r.p) { set_merr("%s: %s is NULL", who, r.name); return ORBM_E_INVALID; }
    if (nframes < 1 || cap < 1 || nmp < 1 || nlevels < 1 || first < 0) {
        set_merr("%s: nframes, cap, nmp and nlevels must be >= 1 and first >= 0", who);
        return ORBM_E_INVALID;
    }
    if (!std::isfinite(bf) || !std::isfinite(k_host[0]) || !std::isfinite(k_host[1]) || !std::isfinite(k_host[2]) || !std::isfinite(k_host[3])) {
        set_merr("%s: k_host or bf is not finite", who);
        return ORBM_E_INVALID;
    }
    if (nframes > ORBM_POSEOPT_MAX_FRAMES || cap > ORBM_POSEOPT_MAX_CAP) {
        set_merr("%s: %d frames of %d slots (at most %d of %d)", who, nframes, cap, (int)ORBM_POSEOPT_MAX_FRAMES, (int)ORBM_POSEOPT_MAX_CAP);
        return ORBM_E_CAPACITY;
    }
    if (nlevels > ORBM_POSEOPT_MAX_LEVELS) { set_merr("%s: %d pyramid levels (at most %d)", who, nlevels, (int)ORBM_POSEOPT_MAX_LEVELS); return ORBM_E_CAPACITY; }
    if (nmp > ORBM_MP_MAX_BATCH) { set_merr("%s: %d MapPoints (at most %d)", who, nmp, (int)ORBM_MP_MAX_BATCH); return ORBM_E_CAPACITY; }
    if ((long long)(first + (long long)nframes) * cap > INT_MAX) { set_merr("%s: (first + nframes) * cap exceeds 2^31 - 1", who); return ORBM_E_CAPACITY; }
    static_assert(ORBM_POSEOPT_MAX_LEVELS == PO_MAX_LEVELS, "the kernel's level table");
    P = PoseOptParams{};
    P.first = first; P.cap = cap; P.nmp = nmp; P.nlevels = nlevels; P.bf = bf;
    for (int i = 0; i < 4; ++i) P.k[i] = k_host[i];
    for (int i = 0; i < PO_MAX_LEVELS; ++i) P.ils2[i] = i < nlevels ? ils2_host[i] : 0.0f;
    return ORBM_OK;
}

static int poseopt_launch(orbm_t* m, int nframes, PoseOptParams& P, const orbm_kp_t* kps_un, const int32_t* counts, const float* uright,
                          const int32_t* q_mp, const float* mp_pw, const float* tcw_in, float* tcw_out, uint8_t* outlier, int32_t* n_corr,
                          int32_t* n_good) {
    P.kps_un = (const KpIn*)kps_un; P.counts = counts; P.uright = uright; P.q_mp = q_mp; P.mp_pw = mp_pw; P.tcw_in = tcw_in;
    P.tcw_out = tcw_out; P.outlier = outlier; P.n_corr = n_corr; P.n_good = n_good;
    if (P.cap <= PO_LDS_CAP) hipLaunchKernelGGL(k_pose_opt<true>, dim3(nframes), dim3(PO_THREADS), 0, m->stream, P);
    else hipLaunchKernelGGL(k_pose_opt<false>, dim3(nframes), dim3(PO_THREADS), 0, m->stream, P);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_pose_optimization_batch_async(orbm_t* m, int nframes, int first, int cap, const orbm_kp_t* kps_un, const int32_t* counts,
                                       const float* uright, const int32_t* q_mp, int nmp, const float* mp_pw, const float* tcw_in,
                                       const float* k_host, float bf, const float* inv_level_sigma2_host, int nlevels,
                                       float* tcw_out, uint8_t* outlier, int32_t* n_corr, int32_t* n_good) {
    PoseOptParams P;
    const int rc = poseopt_args("PoseOptimization batch", m, nframes, first, cap, kps_un, counts, q_mp, nmp, mp_pw, tcw_in, k_host, bf,
                                inv_level_sigma2_host, nlevels, tcw_out, outlier, n_corr, n_good, P);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    return poseopt_launch(m, nframes, P, kps_un, counts, uright, q_mp, mp_pw, tcw_in, tcw_out, outlier, n_corr, n_good);
}

int orbm_pose_optimization(orbm_t* m, int nframes, int first, int cap, const orbm_kp_t* kps_un, const int32_t* counts,
                           const float* uright, const int32_t* q_mp, int nmp, const float* mp_pw, const float* tcw_in,
                           const float* k_host, float bf, const float* inv_level_sigma2_host, int nlevels,
                           float* tcw_out, uint8_t* outlier, int32_t* n_corr, int32_t* n_good) {
    PoseOptParams P;
    int rc = poseopt_args("PoseOptimization", m, nframes, first, cap, kps_un, counts, q_mp, nmp, mp_pw, tcw_in, k_host, bf, inv_level_sigma2_host,
                          nlevels, tcw_out, outlier, n_corr, n_good, P);
    if (rc) return rc;
    MHIPCHK(hipSetDevice(m->device));
    const size_t rows = (size_t)nframes * cap;
    DevBuf dk, dc, du, dq, dp, dt, dout, dcnt, dto;
    arena_reset(m);
    UP(dk, kps_un + (size_t)first * cap, sizeof(KpIn) * rows); UP(dc, counts + first, sizeof(int32_t) * nframes);   // the block's rows first .. first + nframes - 1
    if (uright) UP(du, uright, sizeof(float) * rows);
    UP(dq, q_mp, sizeof(int32_t) * rows); UP(dp, mp_pw, sizeof(float) * 3 * (size_t)nmp); UP(dt, tcw_in, sizeof(float) * 12 * nframes);
    UPIO(dout, outlier, rows);                                              // slots without a MapPoint keep the caller's bytes
    AL(dcnt, sizeof(int32_t) * 2 * (size_t)nframes); AL(dto, sizeof(float) * 12 * nframes);
    ARENA_FLUSH(m);
    P.first = 0;
    int32_t* cnt = dcnt.as<int32_t>();
    rc = poseopt_launch(m, nframes, P, (const orbm_kp_t*)dk.ptr(), dc.as<int32_t>(), uright ? du.as<float>() : nullptr, dq.as<int32_t>(), dp.as<float>(),
                        dt.as<float>(), dto.as<float>(), dout.as<uint8_t>(), cnt, cnt + nframes);
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    const int32_t* hc = (const int32_t*)dcnt.host();
    memcpy(n_corr, hc, sizeof(int32_t) * nframes); memcpy(n_good, hc + nframes, sizeof(int32_t) * nframes);
    memcpy(tcw_out, dto.host(), sizeof(float) * 12 * nframes); memcpy(outlier, dout.host(), rows);
    return ORBM_OK;
}

int orbm_discard_outliers_batch_async(orbm_t* m, int nframes, int cap, const int32_t* counts, int32_t* q_mp, uint8_t* outlier,
                                      int nmp, const int32_t* mp_nobs, const uint8_t* mp_valid, int discard, int clear_bad,
                                      uint8_t* mp_seen, int32_t* n_matches_map, int32_t* n_discarded) {
    const char* who = "DiscardOutliers batch";
    if (const int rc = covis_handle(who, m)) return rc;
    if (!counts || !q_mp || !outlier || !mp_nobs) { set_merr("%s: counts, q_mp, outlier or mp_nobs is NULL", who); return ORBM_E_INVALID; }
    if (nframes < 1 || cap < 1 || nmp < 1) { set_merr("%s: nframes, cap and nmp must be >= 1", who); return ORBM_E_INVALID; }
    if (nframes > ORBM_POSEOPT_MAX_FRAMES || cap > ORBM_POSEOPT_MAX_CAP) {
        set_merr("%s: %d frames of %d slots (at most %d of %d)", who, nframes, cap, (int)ORBM_POSEOPT_MAX_FRAMES, (int)ORBM_POSEOPT_MAX_CAP);
        return ORBM_E_CAPACITY;
    }
    if (nmp > ORBM_MP_MAX_BATCH) { set_merr("%s: %d MapPoints (at most %d)", who, nmp, (int)ORBM_MP_MAX_BATCH); return ORBM_E_CAPACITY; }
    if ((long long)nframes * nmp > ORBM_COVIS_MAX_VOTES) { set_merr("%s: %d frames x %d MapPoints of seen flags (at most 2^28)", who, nframes, nmp); return ORBM_E_CAPACITY; }
    MHIPCHK(hipSetDevice(m->device));
    // the rows start from zero inside the enqueued work: a replayed graph replays the memsets
    if (mp_seen) MHIPCHK(hipMemsetAsync(mp_seen, 0, (size_t)nframes * nmp, m->stream));
    if (n_matches_map) MHIPCHK(hipMemsetAsync(n_matches_map, 0, sizeof(int32_t) * nframes, m->stream));
    if (n_discarded) MHIPCHK(hipMemsetAsync(n_discarded, 0, sizeof(int32_t) * nframes, m->stream));
    const DiscardParams P{cap, nmp, discard ? 1 : 0, clear_bad ? 1 : 0, counts, q_mp, outlier, mp_nobs, mp_valid, mp_seen, n_matches_map, n_discarded};
    hipLaunchKernelGGL(k_discard_outliers, dim3((cap + 255) / 256, nframes), dim3(256), 0, m->stream, P);
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

// ---- CreateNewMapPoints behind M10: the parallax tests, the triangulation, the gates and the creation order (LocalMapping.cc:609-892) ----
struct TriPoolArgs {
    int nrows, cap; const orbm_kp_t* kps_un; const orbm_kp_t* kps; const int32_t* counts; const float* uright; const float* depth;
    const float* tcw; const float* ow;
};
struct TriOutArgs { int32_t* won_pair; int32_t* won_idx2; float* x3d; uint8_t* reason; int32_t* ncreated; int32_t* order; int32_t* ntotal; };

// the argument tests both forms share; fills the kernels' parameter block (pointers and group_start still unset)
static int tri_args(const char* who, orbm_t* m, int ngroups, const int32_t* group_start, int npairs, const TriPoolArgs& a, const TriPoolArgs& b,
                    const int32_t* row1, const int32_t* row2, const int32_t* matches12, const float* k1, const float* k2,
                    const float* sf1, const float* ls1, const float* sf2, const float* ls2, int nlevels, float ratio_factor, const TriOutArgs& o,
                    TriNewParams& P) {
    if (const int rc = covis_handle(who, m)) return rc;
    const struct { const void* p; const char* name; } req[] = {
        {group_start, "group_start"}, {a.kps_un, "kps_un1"}, {a.counts, "counts1"}, {a.tcw, "tcw1"}, {a.ow, "ow1"},
        {b.kps_un, "kps_un2"}, {b.counts, "counts2"}, {b.tcw, "tcw2"}, {b.ow, "ow2"}, {row1, "row1"}, {row2, "row2"}, {matches12, "matches12"},
        {k1, "k1_host"}, {k2, "k2_host"}, {sf1, "scale_factors1_host"}, {ls1, "level_sigma2_1_host"}, {sf2, "scale_factors2_host"},
        {ls2, "level_sigma2_2_host"}, {o.won_pair, "won_pair"}, {o.won_idx2, "won_idx2"}, {o.x3d, "x3d"}, {o.ncreated, "ncreated"},
        {o.order, "order"}, {o.ntotal, "ntotal"}};
    for (const auto& r : req)
        if (!r.p) { set_merr("%s: %s is NULL", who, r.name); return ORBM_E_INVALID; }
    if (ngroups < 1 || npairs < 1 || a.nrows < 1 || a.cap < 1 || b.nrows < 1 || b.cap < 1 || nlevels < 1) {
        set_merr("%s: ngroups, npairs, nrows1, cap1, nrows2, cap2 and nlevels must be >= 1", who);
        return ORBM_E_INVALID;
    }
    if (!std::isfinite(ratio_factor)) { set_merr("%s: ratio_factor is not finite", who); return ORBM_E_INVALID; }
    if (a.cap > ORBM_TRI_MAX_CAP || b.cap > ORBM_TRI_MAX_CAP || npairs > ORBM_TRI_MAX_PAIRS) {
        set_merr("%s: cap1 %d, cap2 %d, npairs %d (at most %d, %d, %d)", who, a.cap, b.cap, npairs, (int)ORBM_TRI_MAX_CAP, (int)ORBM_TRI_MAX_CAP,
                 (int)ORBM_TRI_MAX_PAIRS);
        return ORBM_E_CAPACITY;
    }
    if (nlevels > ORBM_TRI_MAX_LEVELS) { set_merr("%s: %d pyramid levels (at most %d)", who, nlevels, (int)ORBM_TRI_MAX_LEVELS); return ORBM_E_CAPACITY; }
    if (ngroups > npairs || group_start[0] != 0 || group_start[ngroups] != npairs) {
        set_merr("%s: group_start must run from 0 to npairs over at most npairs groups", who);
        return ORBM_E_INVALID;
    }
    for (int g = 0; g < ngroups; ++g) {
        const long long n = (long long)group_start[g + 1] - group_start[g];
        if (n < 0 || group_start[g + 1] > npairs) { set_merr("%s: group_start is not monotone at group %d", who, g); return ORBM_E_INVALID; }
        if (n > ORBM_TRI_MAX_GROUP_PAIRS) { set_merr("%s: group %d holds %lld pairs (at most %d)", who, g, n, (int)ORBM_TRI_MAX_GROUP_PAIRS); return ORBM_E_CAPACITY; }
    }
    static_assert(ORBM_TRI_MAX_LEVELS == TRI_MAX_LEVELS && ORBM_TRI_MAX_GROUP_PAIRS == TRI_MAX_GROUP_PAIRS, "the kernels' tables");
    P = TriNewParams{};
    P.npairs = npairs; P.nlevels = nlevels; P.ratio_factor = ratio_factor;
    P.k1 = TriCam{k1[0], k1[1], k1[2], k1[3], k1[4], k1[5]}; P.k2 = TriCam{k2[0], k2[1], k2[2], k2[3], k2[4], k2[5]};
    for (int i = 0; i < TRI_MAX_LEVELS; ++i) {
        P.sf1[i] = i < nlevels ? sf1[i] : 1.0f; P.ls1[i] = i < nlevels ? ls1[i] : 1.0f;
        P.sf2[i] = i < nlevels ? sf2[i] : 1.0f; P.ls2[i] = i < nlevels ? ls2[i] : 1.0f;
    }
    return ORBM_OK;
}

static TriPool tri_pool(const TriPoolArgs& a) {
    const KpIn* un = (const KpIn*)a.kps_un;
    return TriPool{a.nrows, a.cap, un, a.kps ? (const KpIn*)a.kps : un, a.counts, a.uright, a.depth, a.tcw, a.ow};
}

// TRI_GROUPS_PER_LAUNCH groups per launch pair: group_start rides in the kernel arguments, so nothing is staged or allocated
static int tri_launch(orbm_t* m, int ngroups, const int32_t* group_start, TriNewParams& P, const TriPoolArgs& a, const TriPoolArgs& b,
                      const int32_t* row1, const int32_t* row2, const int32_t* matches12, const TriOutArgs& o) {
    P.p1 = tri_pool(a); P.p2 = tri_pool(b); P.row1 = row1; P.row2 = row2; P.matches12 = matches12;
    P.won_pair = o.won_pair; P.won_idx2 = o.won_idx2; P.x3d = o.x3d; P.reason = o.reason; P.ncreated = o.ncreated; P.order = o.order; P.ntotal = o.ntotal;
    for (int g0 = 0; g0 < ngroups; g0 += TRI_GROUPS_PER_LAUNCH) {
        const int ng = std::min(ngroups - g0, (int)TRI_GROUPS_PER_LAUNCH);
        P.g0 = g0;
        for (int i = 0; i <= TRI_GROUPS_PER_LAUNCH; ++i) P.gstart[i] = group_start[g0 + std::min(i, ng)];
        hipLaunchKernelGGL(k_triangulate_new, dim3((a.cap + 255) / 256, ng), dim3(256), 0, m->stream, P);
        hipLaunchKernelGGL(k_triangulate_order, dim3(ng), dim3(64), 0, m->stream, P);
    }
    MHIPCHK(hipGetLastError());
    return ORBM_OK;
}

int orbm_triangulate_new_points_batch_async(orbm_t* m, int ngroups, const int32_t* group_start_host, int npairs,
                                            int nrows1, int cap1, const orbm_kp_t* kps_un1, const orbm_kp_t* kps1, const int32_t* counts1,
                                            const float* uright1, const float* depth1, const float* tcw1, const float* ow1,
                                            int nrows2, int cap2, const orbm_kp_t* kps_un2, const orbm_kp_t* kps2, const int32_t* counts2,
                                            const float* uright2, const float* depth2, const float* tcw2, const float* ow2,
                                            const int32_t* row1, const int32_t* row2, const int32_t* matches12,
                                            const float* k1_host, const float* k2_host, float mb1, float mbf1, float mb2,
                                            const float* scale_factors1_host, const float* level_sigma2_1_host,
                                            const float* scale_factors2_host, const float* level_sigma2_2_host,
                                            int nlevels, float ratio_factor, float th_far,
                                            int32_t* won_pair, int32_t* won_idx2, float* x3d, uint8_t* reason, int32_t* ncreated,
                                            int32_t* order, int32_t* ntotal) {
    const TriPoolArgs a{nrows1, cap1, kps_un1, kps1, counts1, uright1, depth1, tcw1, ow1}, b{nrows2, cap2, kps_un2, kps2, counts2, uright2, depth2, tcw2, ow2};
    const TriOutArgs o{won_pair, won_idx2, x3d, reason, ncreated, order, ntotal};
    TriNewParams P;
    const int rc = tri_args("TriangulateNewPoints batch", m, ngroups, group_start_host, npairs, a, b, row1, row2, matches12, k1_host, k2_host,
                            scale_factors1_host, level_sigma2_1_host, scale_factors2_host, level_sigma2_2_host, nlevels, ratio_factor, o, P);
    if (rc) return rc;
    P.mb1 = mb1; P.mbf1 = mbf1; P.mb2 = mb2; P.th_far = th_far;
    MHIPCHK(hipSetDevice(m->device));
    return tri_launch(m, ngroups, group_start_host, P, a, b, row1, row2, matches12, o);
}

int orbm_triangulate_new_points(orbm_t* m, int space, int ngroups, const int32_t* group_start_host, int npairs,
                                int nrows1, int cap1, const orbm_kp_t* kps_un1, const orbm_kp_t* kps1, const int32_t* counts1,
                                const float* uright1, const float* depth1, const float* tcw1, const float* ow1,
                                int nrows2, int cap2, const orbm_kp_t* kps_un2, const orbm_kp_t* kps2, const int32_t* counts2,
                                const float* uright2, const float* depth2, const float* tcw2, const float* ow2,
                                const int32_t* row1, const int32_t* row2, const int32_t* matches12,
                                const float* k1_host, const float* k2_host, float mb1, float mbf1, float mb2,
                                const float* scale_factors1_host, const float* level_sigma2_1_host,
                                const float* scale_factors2_host, const float* level_sigma2_2_host,
                                int nlevels, float ratio_factor, float th_far,
                                int32_t* won_pair, int32_t* won_idx2, float* x3d, uint8_t* reason, int32_t* ncreated,
                                int32_t* order, int32_t* ntotal) {
    const char* who = "TriangulateNewPoints";
    if (space != ORBM_HOST && space != ORBM_DEVICE) {
        if (const int rc = covis_handle(who, m)) return rc;
        set_merr("%s: space must be ORBM_HOST or ORBM_DEVICE", who);
        return ORBM_E_INVALID;
    }
    TriPoolArgs a{nrows1, cap1, kps_un1, kps1, counts1, uright1, depth1, tcw1, ow1}, b{nrows2, cap2, kps_un2, kps2, counts2, uright2, depth2, tcw2, ow2};
    TriOutArgs o{won_pair, won_idx2, x3d, reason, ncreated, order, ntotal};
    TriNewParams P;
    int rc = tri_args(who, m, ngroups, group_start_host, npairs, a, b, row1, row2, matches12, k1_host, k2_host, scale_factors1_host,
                      level_sigma2_1_host, scale_factors2_host, level_sigma2_2_host, nlevels, ratio_factor, o, P);
    if (rc) return rc;
    P.mb1 = mb1; P.mbf1 = mbf1; P.mb2 = mb2; P.th_far = th_far;
    MHIPCHK(hipSetDevice(m->device));
    if (space == ORBM_DEVICE) {
        rc = tri_launch(m, ngroups, group_start_host, P, a, b, row1, row2, matches12, o);
        if (rc) return rc;
        MHIPCHK(hipStreamSynchronize(m->stream));
        return ORBM_OK;
    }
    for (int g = 0; g < ngroups; ++g)                          // readable here: a group is the pairs of ONE current KeyFrame
        for (int p = group_start_host[g] + 1; p < group_start_host[g + 1]; ++p)
            if (row1[p] != row1[group_start_host[g]]) { set_merr("%s: the pairs of group %d do not share one row1", who, g); return ORBM_E_INVALID; }
    const size_t s1 = (size_t)nrows1 * cap1, s2 = (size_t)nrows2 * cap2, so = (size_t)ngroups * cap1, sp = (size_t)npairs * cap1;
    // pool 2 may be pool 1 (one pool passed twice): each distinct host array goes up once
    const bool samePool = nrows1 == nrows2 && cap1 == cap2 && kps_un1 == kps_un2 && kps1 == kps2 && counts1 == counts2 && uright1 == uright2 &&
                          depth1 == depth2 && tcw1 == tcw2 && ow1 == ow2;
    DevBuf du1, dk1, dc1, dr1, dd1, dt1, do1, du2, dk2, dc2, dr2, dd2, dt2, do2, drow1, drow2, dm, dwp, dwi, dx, dre, dnc, dord, dnt;
    arena_reset(m);
    UP(du1, kps_un1, sizeof(KpIn) * s1); UP(dc1, counts1, sizeof(int32_t) * nrows1); UP(dt1, tcw1, sizeof(float) * 12 * nrows1); UP(do1, ow1, sizeof(float) * 3 * nrows1);
    if (kps1 && kps1 != kps_un1) UP(dk1, kps1, sizeof(KpIn) * s1);
    if (uright1) UP(dr1, uright1, sizeof(float) * s1);
    if (depth1) UP(dd1, depth1, sizeof(float) * s1);
    if (!samePool) {
        UP(du2, kps_un2, sizeof(KpIn) * s2); UP(dc2, counts2, sizeof(int32_t) * nrows2); UP(dt2, tcw2, sizeof(float) * 12 * nrows2); UP(do2, ow2, sizeof(float) * 3 * nrows2);
        if (kps2 && kps2 != kps_un2) UP(dk2, kps2, sizeof(KpIn) * s2);
        if (uright2) UP(dr2, uright2, sizeof(float) * s2);
        if (depth2) UP(dd2, depth2, sizeof(float) * s2);
    }
    UP(drow1, row1, sizeof(int32_t) * npairs); UP(drow2, row2, sizeof(int32_t) * npairs); UP(dm, matches12, sizeof(int32_t) * sp);
    AL(dwp, sizeof(int32_t) * so); AL(dwi, sizeof(int32_t) * so); AL(dx, sizeof(float) * 3 * so); AL(dnc, sizeof(int32_t) * npairs);
    AL(dord, sizeof(int32_t) * so); AL(dnt, sizeof(int32_t) * ngroups);
    if (reason) AL(dre, sp);
    ARENA_FLUSH(m);
    a = TriPoolArgs{nrows1, cap1, (const orbm_kp_t*)du1.ptr(), kps1 && kps1 != kps_un1 ? (const orbm_kp_t*)dk1.ptr() : nullptr, dc1.as<int32_t>(),
                    uright1 ? dr1.as<float>() : nullptr, depth1 ? dd1.as<float>() : nullptr, dt1.as<float>(), do1.as<float>()};
    if (samePool) b = a;
    else b = TriPoolArgs{nrows2, cap2, (const orbm_kp_t*)du2.ptr(), kps2 && kps2 != kps_un2 ? (const orbm_kp_t*)dk2.ptr() : nullptr, dc2.as<int32_t>(),
                         uright2 ? dr2.as<float>() : nullptr, depth2 ? dd2.as<float>() : nullptr, dt2.as<float>(), do2.as<float>()};
    o = TriOutArgs{dwp.as<int32_t>(), dwi.as<int32_t>(), dx.as<float>(), reason ? dre.as<uint8_t>() : nullptr, dnc.as<int32_t>(), dord.as<int32_t>(),
                   dnt.as<int32_t>()};
    rc = tri_launch(m, ngroups, group_start_host, P, a, b, drow1.as<int32_t>(), drow2.as<int32_t>(), dm.as<int32_t>(), o);
    if (rc) return rc;
    MHIPCHK(hipStreamSynchronize(m->stream));
    ARENA_FETCH(m);
    memcpy(won_pair, dwp.host(), sizeof(int32_t) * so); memcpy(won_idx2, dwi.host(), sizeof(int32_t) * so); memcpy(x3d, dx.host(), sizeof(float) * 3 * so);
    memcpy(ncreated, dnc.host(), sizeof(int32_t) * npairs); memcpy(order, dord.host(), sizeof(int32_t) * so); memcpy(ntotal, dnt.host(), sizeof(int32_t) * ngroups);
    if (reason) memcpy(reason, dre.host(), sp);
    return ORBM_OK;
}

}  // extern "C"
