// orbm_kernels.hip.h -- hand-written gfx950 kernels of the ORB matcher primitives.
// Integer/bitwise bound: 256-bit XOR + popcount (v_bcnt) per pair, operands broadcast from LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#define PO_FN __host__ __device__ static inline
#include "orbm_poseopt.h"          // the arithmetic of k_pose_opt, shared with the host tests
#define TRI_FN __host__ __device__ static inline
#include "orbm_triangulate.h"      // the arithmetic of k_triangulate_new, shared with the host tests

namespace orbmk {

typedef unsigned long long u64;

__device__ __forceinline__ int ham256(const u64 a[4], u64 b0, u64 b1, u64 b2, u64 b3) {
    return __popcll(a[0] ^ b0) + __popcll(a[1] ^ b1) + __popcll(a[2] ^ b2) + __popcll(a[3] ^ b3);
}

__device__ __forceinline__ unsigned bcnt_acc(unsigned x, unsigned acc) {   // popcount(x) + acc in one instruction
#if __HIP_DEVICE_COMPILE__
    unsigned r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
#else
    return (unsigned)__builtin_popcount(x) + acc;
#endif
}

__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
#if __HIP_DEVICE_COMPILE__
    unsigned r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return max(min(a, b), min(max(a, b), c));
#endif
}

// (dist, idx) lexicographic insert into a sorted top-2
__device__ __forceinline__ void top2_insert(int d, int j, int& d0, int& j0, int& d1, int& j1) {
    if (d < d0 || (d == d0 && j < j0)) { d1 = d0; j1 = j0; d0 = d; j0 = j; }
    else if (d < d1 || (d == d1 && j < j1)) { d1 = d; j1 = j; }
}

// ------------------------------------------------------------------------------------------------
// k_knn2: dense brute-force 2-NN in Hamming space (Frame.cc:1440-1480, cv::BFMatcher knnMatch k=2).
// grid (ceil(q_stride/64), npairs), 256 threads.  The block stages the pair's train descriptors in LDS
// in chunks; lane = query, the 4 waves scan interleaved quarters of each chunk (all lanes of a wave read
// the same LDS address -> broadcast, conflict free); per-wave top-2 are merged through LDS at the end.
// ------------------------------------------------------------------------------------------------
#define KNN_CHUNK 1024
__global__ __launch_bounds__(256) void k_knn2(const uint8_t* __restrict__ q, int q_stride, const int* __restrict__ nq,
                                              const uint8_t* __restrict__ t, int t_stride, const int* __restrict__ nt,
                                              int* __restrict__ idx2, int* __restrict__ dist2, double ratio, uint8_t* __restrict__ good) {
    __shared__ __attribute__((aligned(16))) u64 tr[KNN_CHUNK * 4];
    __shared__ int mrg[4][64][4];
    const int pair = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nQ = nq[pair], nT = nt[pair];
    const int qi = blockIdx.x * 64 + lane;
    if (blockIdx.x * 64 >= nQ) return;                      // whole block idle (uniform)
    u64 a[4] = {0, 0, 0, 0};
    if (qi < nQ) {
        const uint4* qp = (const uint4*)(q + ((size_t)pair * q_stride + qi) * 32);
        const uint4 lo = qp[0], hi = qp[1];
        a[0] = (u64)lo.x | ((u64)lo.y << 32); a[1] = (u64)lo.z | ((u64)lo.w << 32);
        a[2] = (u64)hi.x | ((u64)hi.y << 32); a[3] = (u64)hi.z | ((u64)hi.w << 32);
    }
    // top-2 as packed keys (distance << 22 | train index): unsigned order == (distance, index) lexicographic, which is the
    // tie rule (lower train index first); one v_min + one v_med3 per candidate.  t_stride < 2^22 is checked by the host.
    unsigned k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu;
    const unsigned* a32 = (const unsigned*)a;
    const uint8_t* tb = t + (size_t)pair * t_stride * 32;
    for (int c0 = 0; c0 < nT; c0 += KNN_CHUNK) {
        const int cn = min(KNN_CHUNK, nT - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < cn * 2; i += 256)       // 16 B per thread per step, coalesced
            ((uint4*)tr)[i] = ((const uint4*)(tb + (size_t)c0 * 32))[i];
        __syncthreads();
        const uint4* tv = (const uint4*)tr;
        auto one = [&](int j) {
            const uint4 lo = tv[2 * j], hi = tv[2 * j + 1];     // same address in every lane: LDS broadcast
            unsigned d = bcnt_acc(a32[0] ^ lo.x, 0u);
            d = bcnt_acc(a32[1] ^ lo.y, d); d = bcnt_acc(a32[2] ^ lo.z, d); d = bcnt_acc(a32[3] ^ lo.w, d);
            d = bcnt_acc(a32[4] ^ hi.x, d); d = bcnt_acc(a32[5] ^ hi.y, d); d = bcnt_acc(a32[6] ^ hi.z, d);
            d = bcnt_acc(a32[7] ^ hi.w, d);                                           // 8 xor + 8 accumulating v_bcnt
            const unsigned key = (d << 22) | (unsigned)(c0 + j);
            k1 = umed3(k0, k1, key);           // second smallest of {k0 <= k1, key}
            k0 = min(k0, key);
        };
        int j = wv;
        for (; j + 12 < cn; j += 16) { one(j); one(j + 4); one(j + 8); one(j + 12); }
        for (; j < cn; j += 4) one(j);
    }
    __syncthreads();
    unsigned* mk = (unsigned*)mrg;                            // [4][64][2] keys
    mk[(wv * 64 + lane) * 2] = k0; mk[(wv * 64 + lane) * 2 + 1] = k1;
    __syncthreads();
    if (wv == 0 && qi < nQ) {
        for (int w = 1; w < 4; ++w)
            for (int e = 0; e < 2; ++e) {
                const unsigned key = mk[(w * 64 + lane) * 2 + e];
                k1 = umed3(k0, k1, key);
                k0 = min(k0, key);
            }
        const size_t o = ((size_t)pair * q_stride + qi) * 2;
        const bool h0 = k0 != 0xFFFFFFFFu, h1 = k1 != 0xFFFFFFFFu;
        idx2[o] = h0 ? (int)(k0 & 0x3FFFFFu) : -1; idx2[o + 1] = h1 ? (int)(k1 & 0x3FFFFFu) : -1;
        dist2[o] = h0 ? (int)(k0 >> 22) : -1; dist2[o + 1] = h1 ? (int)(k1 >> 22) : -1;
        if (good) good[o >> 1] = (h0 && h1 && (double)(float)(int)(k0 >> 22) < (double)(float)(int)(k1 >> 22) * ratio) ? 1 : 0;   // Frame.cc:1465
    }
}


// ------------------------------------------------------------------------------------------------
// k_knn2_mfma: the same dense 2-NN on the matrix cores.  A 1000 x 1000 x 256-bit Hamming table is O(n^2) integer work
// on 64 KB of operands -- compute bound, the one GEMM-shaped piece of the path -- and it is exact in int8:
//   ham(q, t) = popc(q) + sum_k t_k * (1 - 2 q_k)            (t_k, q_k the descriptor bits)
// so with train bits as 0/1 bytes in the A operand and query bits as +-1 bytes in the B operand, v_mfma_i32_32x32x32_i8
// accumulates ham - popc(q) for 32 train rows x 32 query columns; popc(q) is constant per column and is added at the end.
// Bit -> byte expansion is one v_and per operand dword: a word is rotated once so that bits 4h + e + 8i sit at 3 + e + 8i, and
// dword e of the fragment = rotated & (0x08080808 << e), i.e. bytes worth 0 or 2^(3+e); the query side carries the matching
// +-2^(6-e), so every product is +-512 and the accumulator is 512 * (ham - popc(q)).  Which k each (lane half h, byte) lands on
// does not matter: A and B use the same map.
// Selection without leaving the accumulator layout (column = lane & 31 = query, 16 train rows per lane): the accumulator
// starts at C = 2^17 + row, so the result IS a packed key (ham' + 256) << 9 | row whose unsigned order is (distance, train
// index) -- the reference's tie rule -- and one v_min + one v_med3 per distance keep the two smallest: no per-distance op
// besides those two.  Rows are tile-relative: tiles are walked from the last to the first and the kept keys move up by 32 per
// tile; the 9-bit row field holds 16 tiles, after which the two keys are widened to (distance + 256) << 19 | absolute index.
// A wave owns 64 queries (two B fragments sets) and streams the pair's train descriptors from L2; no LDS, no barrier.
// Limits (host-checked): t_stride <= KM_MAX_NT.
// ------------------------------------------------------------------------------------------------
#define KM_MAX_NT ((1 << 19) - 64)
typedef int km_i32x4 __attribute__((ext_vector_type(4)));
typedef int km_i32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void k_knn2_mfma(const uint8_t* __restrict__ q, int q_stride, const int* __restrict__ nq,
                                                   const uint8_t* __restrict__ t, int t_stride, const int* __restrict__ nt,
                                                   int* __restrict__ idx2, int* __restrict__ dist2, double ratio, uint8_t* __restrict__ good) {
#if __HIP_DEVICE_COMPILE__
    const int pair = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nQ = nq[pair], nT = nt[pair];
    const int q0 = blockIdx.x * 256 + wv * 64;
    if (q0 >= nQ) return;                                     // wave-uniform; the kernel has no barrier
    const int r = lane & 31, h = lane >> 5;
    // ---- query side: +-2^(6-e) bytes, built once
    km_i32x4 bf[2][8];
    int pq[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int qi = q0 + n * 32 + r;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
        if (qi < nQ) {
            const uint4* qp = (const uint4*)(q + ((size_t)pair * q_stride + qi) * 32);
            lo = qp[0]; hi = qp[1];
        }
        const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        int pc = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            pc += __popc(w[s]);
            const unsigned wp = w[s] >> (4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned y = (wp >> e) & 0x01010101u;              // the bit, per byte
                const unsigned mag = 64u >> e;
                bf[n][s][e] = (int)(mag * 0x01010101u + y * (256u - 2u * mag));   // bit ? -mag : +mag as int8 (no carries: <= 255 per byte)
            }
        }
        pq[n] = pc;
    }
    km_i32x16 cin;
#pragma unroll
    for (int i = 0; i < 16; ++i) cin[i] = (1 << 17) + (i & 3) + 8 * (i >> 2) + 4 * h;
    const unsigned SENT = 0x7FFFFE00u;                        // window key "no neighbour" (survives 16 x += 32)
    unsigned k0[2] = {SENT, SENT}, k1[2] = {SENT, SENT};      // two smallest window keys per query set
    unsigned G0[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, G1[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};   // two smallest (distance+256) << 19 | train index
    const int rot = h ? 1 : 29;                               // rotate right: bits 4h + e + 8i of a word -> positions 3 + e + 8i
    const uint8_t* tb = t + (size_t)pair * t_stride * 32;
    const int ntile = (nT + 31) >> 5;
    uint4 nlo = make_uint4(0, 0, 0, 0), nhi = nlo;
    if (ntile > 0 && (ntile - 1) * 32 + r < nT) {
        const uint4* tp = (const uint4*)(tb + (size_t)((ntile - 1) * 32 + r) * 32);
        nlo = tp[0]; nhi = tp[1];
    }
    for (int tile = ntile - 1; tile >= 0; --tile) {
        const uint4 lo = nlo, hi = nhi;
        if (tile > 0) {                                       // the next tile is always a full one
            const uint4* tp = (const uint4*)(tb + (size_t)((tile - 1) * 32 + r) * 32);
            nlo = tp[0]; nhi = tp[1];
        }
        const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        km_i32x16 acc0 = cin, acc1 = cin;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const unsigned wp = __builtin_amdgcn_alignbit(w[s], w[s], rot);
            km_i32x4 a;
            a[0] = (int)(wp & 0x08080808u); a[1] = (int)(wp & 0x10101010u); a[2] = (int)(wp & 0x20202020u); a[3] = (int)(wp & 0x40404040u);
            acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bf[0][s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bf[1][s], acc1, 0, 0, 0);
        }
        k0[0] += 32u; k1[0] += 32u; k0[1] += 32u; k1[1] += 32u;          // kept keys become relative to this tile's first row
        if (tile * 32 + 32 <= nT) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                k1[0] = umed3(k0[0], k1[0], (unsigned)acc0[i]); k0[0] = min(k0[0], (unsigned)acc0[i]);
                k1[1] = umed3(k0[1], k1[1], (unsigned)acc1[i]); k0[1] = min(k0[1], (unsigned)acc1[i]);
            }
        } else {                                              // the ragged last tile: rows past nT are not candidates
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool ok = tile * 32 + (i & 3) + 8 * (i >> 2) + 4 * h < nT;
                const unsigned ka = ok ? (unsigned)acc0[i] : SENT, kb = ok ? (unsigned)acc1[i] : SENT;
                k1[0] = umed3(k0[0], k1[0], ka); k0[0] = min(k0[0], ka);
                k1[1] = umed3(k0[1], k1[1], kb); k0[1] = min(k0[1], kb);
            }
        }
        if ((tile & 15) == 0) {                               // window done: widen its two keys to absolute train indices
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const unsigned base = (unsigned)tile * 32u;
                const unsigned g0 = k0[n] < 0x40000000u ? ((k0[n] >> 9) << 19) | (base + (k0[n] & 511u)) : 0xFFFFFFFFu;
                const unsigned g1 = k1[n] < 0x40000000u ? ((k1[n] >> 9) << 19) | (base + (k1[n] & 511u)) : 0xFFFFFFFFu;
                G1[n] = umed3(G0[n], G1[n], g0); G0[n] = min(G0[n], g0);
                G1[n] = umed3(G0[n], G1[n], g1); G0[n] = min(G0[n], g1);
                k0[n] = SENT; k1[n] = SENT;
            }
        }
    }
    // ---- the two lane halves saw disjoint train rows of the same query: merge, then half h stores query set h
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const unsigned o0 = (unsigned)__shfl_xor((int)G0[n], 32), o1 = (unsigned)__shfl_xor((int)G1[n], 32);
        G1[n] = umed3(G0[n], G1[n], o0); G0[n] = min(G0[n], o0);
        G1[n] = umed3(G0[n], G1[n], o1); G0[n] = min(G0[n], o1);
    }
    const unsigned f0 = h ? G0[1] : G0[0], f1 = h ? G1[1] : G1[0];
    const int pqs = h ? pq[1] : pq[0];
    const int qi = q0 + h * 32 + r;
    if (qi < nQ) {
        const size_t o = ((size_t)pair * q_stride + qi) * 2;
        const bool h0 = f0 != 0xFFFFFFFFu, h1 = f1 != 0xFFFFFFFFu;
        idx2[o] = h0 ? (int)(f0 & 0x7FFFFu) : -1; idx2[o + 1] = h1 ? (int)(f1 & 0x7FFFFu) : -1;
        const int d0 = h0 ? (int)(f0 >> 19) - 256 + pqs : -1, d1 = h1 ? (int)(f1 >> 19) - 256 + pqs : -1;
        dist2[o] = d0;
        dist2[o + 1] = d1;
        // Lowe's ratio as Frame.cc:1465 writes it: two neighbours and (float)d0 < (float)d1 * 0.7 evaluated in double
        if (good) good[(size_t)pair * q_stride + qi] = (h0 && h1 && (double)(float)d0 < (double)(float)d1 * ratio) ? 1 : 0;
    }
#endif
}


// ------------------------------------------------------------------------------------------------
// k_grid_build: Frame::AssignFeaturesToGrid (Frame.cc:446-480).  One workgroup per frame.
// Stable order inside a cell = ascending keypoint index: sort keys (cell<<16 | index) with a bitonic
// sort in LDS, then every cell finds its start with a binary search.
// ------------------------------------------------------------------------------------------------
struct KpIn { float x, y, size, angle, response; int octave, class_id; };

// Counting sort form of the grid build (n <= GRID_CS_MAX): cell histogram in LDS -> exclusive scan over the 3072 cells ->
// scatter into a per-cell cursor -> each cell's short list sorted by keypoint index (insertion order of the reference,
// Frame.cc:446-480: i ascending) -> written out.  One pass over the keypoints instead of a 66-stage bitonic sort of n keys.
// Above GRID_WIDE_MIN keypoints (where the bitonic form's n2 = 65536 keys no longer fit the LDS) the counting form runs again as
// WIDE: the same histogram, scan and scatter, but a cell list longer than GRID_WIDE_SHORT is put in order by the whole workgroup
// (grid_sort_list) instead of by one lane, so that the time is bounded whatever the keypoints' spread.
#define GRID_CS_MAX 8192
#define GRID_CELLS (64 * 48)
#define GRID_WIDE_MIN 32768
#define GRID_WIDE_SHORT 64
#define GRID_WIDE_LONG_CELLS 1024                              // cells of more than 64 entries among at most 65535 keypoints: <= 1008

// Ascending in-place sort of p[0, len) (distinct keys) by the 256 threads of the workgroup; every thread calls it with the same
// arguments.  The bitonic network in its one-direction form (first step of a merge pairs i with i ^ (k - 1), the others i with i ^ j,
// the smaller key always to the lower index), so that positions at and past len stand for +inf keys that no exchange ever moves and
// are never touched.  sum over k = 2 .. len2 of log2 k steps (136 at len = 65535), each ceil(len / 256) iterations per thread.
__device__ __forceinline__ void grid_sort_list(unsigned short* p, int len) {
    const int tid = threadIdx.x;
    for (int k = 2; (k >> 1) < len; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int mask = j == (k >> 1) ? k - 1 : j;
            for (int i = tid; i < len; i += 256) {
                const int o = i ^ mask;
                if (o > i && o < len) {
                    const unsigned short a = p[i], b = p[o];
                    if (a > b) { p[i] = b; p[o] = a; }
                }
            }
            __syncthreads();
        }
    }
}

template <bool WIDE>
__device__ __forceinline__ int grid_build_counting(const KpIn* __restrict__ kp, int n, float min_x, float min_y, float inv_w, float inv_h,
                                                   int* __restrict__ gs, int* __restrict__ gi, unsigned char* smem,
                                                   int* s_nlong = nullptr, unsigned short* s_long = nullptr) {   // WIDE: the long cells, [1] and [GRID_WIDE_LONG_CELLS] in LDS
    int* hist = (int*)smem;                                    // [GRID_CELLS + 1] counts -> starts
    int* cur = hist + GRID_CELLS + 1;                          // [GRID_CELLS] fill cursors
    unsigned short* lgi = (unsigned short*)(cur + GRID_CELLS); // [n] indices, cell by cell
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int c = tid; c <= GRID_CELLS; c += 256) hist[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int px = (int)roundf((kp[i].x - min_x) * inv_w);              // PosInGrid: round, not floor (Frame.cc:888-889)
        const int py = (int)roundf((kp[i].y - min_y) * inv_h);
        if (px >= 0 && px < 64 && py >= 0 && py < 48) atomicAdd(&hist[px * 48 + py], 1);
    }
    __syncthreads();
    // exclusive scan: thread t owns cells [12 t, 12 t + 12) (3072 = 256 * 12)
    int loc[12], sum = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) { loc[k] = hist[12 * tid + k]; sum += loc[k]; }
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    int base = inc - sum;
    for (int w = 0; w < wv; ++w) base += s_wave[w];
    const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; ++k) { hist[12 * tid + k] = base; cur[12 * tid + k] = base; base += loc[k]; }
    if (tid == 0) hist[GRID_CELLS] = total;
    __syncthreads();
    for (int c = tid; c <= GRID_CELLS; c += 256) gs[c] = hist[c];
    for (int i = tid; i < n; i += 256) {
        const int px = (int)roundf((kp[i].x - min_x) * inv_w);
        const int py = (int)roundf((kp[i].y - min_y) * inv_h);
        if (px >= 0 && px < 64 && py >= 0 && py < 48) lgi[atomicAdd(&cur[px * 48 + py], 1)] = (unsigned short)i;
    }
    __syncthreads();
    if (WIDE) {
        if (tid == 0) *s_nlong = 0;
        __syncthreads();
    }
    for (int c = tid; c < GRID_CELLS; c += 256) {                            // restore insertion order inside every cell (lists are short)
        const int a = hist[c], b = hist[c + 1];
        if (WIDE && b - a > GRID_WIDE_SHORT) {                               // ... and where one is not, it is left to the whole workgroup
            const int k = atomicAdd(s_nlong, 1);
            if (k < GRID_WIDE_LONG_CELLS) s_long[k] = (unsigned short)c;
            continue;
        }
        for (int i = a + 1; i < b; ++i) {
            const unsigned short v = lgi[i];
            int j = i - 1;
            while (j >= a && lgi[j] > v) { lgi[j + 1] = lgi[j]; --j; }
            lgi[j + 1] = v;
        }
    }
    __syncthreads();
    if (WIDE) {
        const int nlong = min(*s_nlong, GRID_WIDE_LONG_CELLS);                // the same for every thread: the barriers inside are uniform
        for (int k = 0; k < nlong; ++k) {
            const int c = s_long[k];
            grid_sort_list(lgi + hist[c], hist[c + 1] - hist[c]);
        }
    }
    for (int i = tid; i < total; i += 256) gi[i] = (int)lgi[i];
    return total;
}
__global__ __launch_bounds__(256) void k_grid_build_cs(const KpIn* __restrict__ kps, int n, float min_x, float min_y, float inv_w, float inv_h,
                                                       int* __restrict__ grid_start, int* __restrict__ grid_idx, int* __restrict__ placed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
    const int total = grid_build_counting<false>(kps, n, min_x, min_y, inv_w, inv_h, grid_start, grid_idx, gsm);
    if (threadIdx.x == 0) *placed = total;
}
__global__ __launch_bounds__(256) void k_grid_build_batch_cs(const KpIn* __restrict__ kps, const int* __restrict__ counts, int cap,
                                                             float min_x, float min_y, float inv_w, float inv_h,
                                                             int* __restrict__ grid_start, int* __restrict__ grid_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
    const int frame = blockIdx.x;
    (void)grid_build_counting<false>(kps + (size_t)frame * cap, min(counts[frame], cap), min_x, min_y, inv_w, inv_h,
                                     grid_start + (size_t)frame * (GRID_CELLS + 1), grid_idx + (size_t)frame * cap, gsm);
}
// the WIDE forms, for n / cap above GRID_WIDE_MIN
__global__ __launch_bounds__(256) void k_grid_build_wide(const KpIn* __restrict__ kps, int n, float min_x, float min_y, float inv_w, float inv_h,
                                                         int* __restrict__ grid_start, int* __restrict__ grid_idx, int* __restrict__ placed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
    __shared__ int s_nlong;
    __shared__ unsigned short s_long[GRID_WIDE_LONG_CELLS];
    const int total = grid_build_counting<true>(kps, n, min_x, min_y, inv_w, inv_h, grid_start, grid_idx, gsm, &s_nlong, s_long);
    if (threadIdx.x == 0) *placed = total;
}
__global__ __launch_bounds__(256) void k_grid_build_batch_wide(const KpIn* __restrict__ kps, const int* __restrict__ counts, int cap,
                                                               float min_x, float min_y, float inv_w, float inv_h,
                                                               int* __restrict__ grid_start, int* __restrict__ grid_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
    __shared__ int s_nlong;
    __shared__ unsigned short s_long[GRID_WIDE_LONG_CELLS];
    const int frame = blockIdx.x;
    (void)grid_build_counting<true>(kps + (size_t)frame * cap, max(min(counts[frame], cap), 0), min_x, min_y, inv_w, inv_h,
                                    grid_start + (size_t)frame * (GRID_CELLS + 1), grid_idx + (size_t)frame * cap, gsm, &s_nlong, s_long);
}

__global__ __launch_bounds__(256) void k_grid_build(const KpIn* __restrict__ kps, int n, int n2, float min_x, float min_y,
                                                    float inv_w, float inv_h, int* __restrict__ grid_start,
                                                    int* __restrict__ grid_idx, int* __restrict__ placed) {
    extern __shared__ unsigned int keys[];
    const int tid = threadIdx.x;
    __shared__ int s_placed;
    if (tid == 0) s_placed = 0;
    __syncthreads();
    for (int i = tid; i < n2; i += 256) {
        unsigned int key = 0xFFFFFFFFu;
        if (i < n) {
            const int px = (int)roundf((kps[i].x - min_x) * inv_w);          // PosInGrid: round, not floor (Frame.cc:888-889)
            const int py = (int)roundf((kps[i].y - min_y) * inv_h);
            if (px >= 0 && px < 64 && py >= 0 && py < 48) { key = ((unsigned)(px * 48 + py) << 16) | (unsigned)i; atomicAdd(&s_placed, 1); }
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned int a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    const int np = s_placed;
    for (int i = tid; i < np; i += 256) grid_idx[i] = (int)(keys[i] & 0xFFFFu);
    for (int c = tid; c <= 64 * 48; c += 256) {
        const unsigned int target = (unsigned)c << 16;
        int lo = 0, hi = np;                                                  // first key >= target
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < target) lo = mid + 1; else hi = mid; }
        grid_start[c] = lo;
    }
    if (tid == 0) *placed = np;
}

// ------------------------------------------------------------------------------------------------
// k_window: Frame::GetFeaturesInArea (Frame.cc:784-871) + DescriptorDistance for a batch of windows.
// One wavefront per window.  Cells of one grid column are contiguous in the CSR (cell = ix*48+iy), so for every
// ix the lanes sweep ONE index range in the reference's visiting order; survivors are compacted with a ballot
// (order preserved) and their 256-bit Hamming distance to the window's descriptor is taken on the spot.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                const float* __restrict__ uright, const int* __restrict__ gs,
                                                const int* __restrict__ gi, float min_x, float min_y, float inv_w, float inv_h,
                                                int nq, const float* __restrict__ qx, const float* __restrict__ qy,
                                                const float* __restrict__ qr, const int* __restrict__ qminl,
                                                const int* __restrict__ qmaxl, const float* __restrict__ qur,
                                                const float* __restrict__ qer, const uint8_t* __restrict__ qdesc, int cap,
                                                int* __restrict__ out_cnt, int* __restrict__ out_idx, int* __restrict__ out_dist,
                                                int* __restrict__ overflow) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const float x = qx[q], y = qy[q], r = qr[q];
    const int minLevel = qminl[q], maxLevel = qmaxl[q];
    int cnt = 0;
    const int nMinCellX = max(0, (int)floorf((x - min_x - r) * inv_w));
    const int nMaxCellX = min(63, (int)ceilf((x - min_x + r) * inv_w));
    const int nMinCellY = max(0, (int)floorf((y - min_y - r) * inv_h));
    const int nMaxCellY = min(47, (int)ceilf((y - min_y + r) * inv_h));
    if (r >= 0 && nMinCellX < 64 && nMaxCellX >= 0 && nMinCellY < 48 && nMaxCellY >= 0) {
        const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
        const uint4* qp = (const uint4*)(qdesc + (size_t)q * 32);
        const uint4 qlo = qp[0], qhi = qp[1];
        const u64 a[4] = {(u64)qlo.x | ((u64)qlo.y << 32), (u64)qlo.z | ((u64)qlo.w << 32),
                          (u64)qhi.x | ((u64)qhi.y << 32), (u64)qhi.z | ((u64)qhi.w << 32)};
        const float er = qer ? qer[q] : -1.f, ur = qur ? qur[q] : 0.f;
        const unsigned long long lt = (1ull << lane) - 1ull;
        for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
            const int j0 = gs[ix * 48 + nMinCellY], j1 = gs[ix * 48 + nMaxCellY + 1];
            for (int jb = j0; jb < j1; jb += 64) {
                const int j = jb + lane;
                bool ok = false;
                int k = 0;
                if (j < j1) {
                    k = gi[j];
                    const KpIn kp = kps[k];
                    ok = true;
                    if (bCheckLevels) {
                        if (kp.octave < minLevel) ok = false;
                        if (maxLevel >= 0 && kp.octave > maxLevel) ok = false;
                    }
                    const float distx = kp.x - x, disty = kp.y - y;
                    if (!(fabsf(distx) < r && fabsf(disty) < r)) ok = false;
                    if (ok && er >= 0.f && uright) {
                        const float urk = uright[k];
                        if (urk > 0 && fabsf(ur - urk) > er) ok = false;
                    }
                }
                const unsigned long long bal = __ballot(ok);
                if (ok) {
                    const int pos = cnt + __popcll(bal & lt);
                    if (pos < cap) {
                        const uint4* tp = (const uint4*)(desc + (size_t)k * 32);
                        const uint4 lo = tp[0], hi = tp[1];
                        const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                                             (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
                        out_idx[(size_t)q * cap + pos] = k;
                        out_dist[(size_t)q * cap + pos] = d;
                    } else *overflow = 1;
                }
                cnt += __popcll(bal);
            }
        }
    }
    if (lane == 0) out_cnt[q] = min(cnt, cap);
}

// ------------------------------------------------------------------------------------------------
// k_window_topk: the same windows, but only what the sequential claim replay of the projection searches can ever look at
// comes back: per window the WT_K candidates with the smallest (distance, position in the reference's visiting order) and
// the candidate count.  The replay takes the first (M4, M5) or the first two (M3: best and second) candidates that are not
// blocked in that order -- exactly the order in which `dist < bestDist` / `else if dist < bestDist2` would have met them --
// so unless every returned candidate of a longer list is blocked, the full [windows][capacity] lists never leave the GPU.
// key = dist << 40 | position << 20 | keypoint index; the running top-K lives in wave-uniform registers.
// ------------------------------------------------------------------------------------------------
#define WT_K 8
__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        const u64 w = (u64)lo | ((u64)hi << 32);
        v = w < v ? w : v;
    }
    return v;
}
__global__ __launch_bounds__(256) void k_window_topk(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                     const float* __restrict__ uright, const int* __restrict__ gs,
                                                     const int* __restrict__ gi, float min_x, float min_y, float inv_w, float inv_h,
                                                     int nq, const float* __restrict__ qx, const float* __restrict__ qy,
                                                     const float* __restrict__ qr, const int* __restrict__ qminl,
                                                     const int* __restrict__ qmaxl, const float* __restrict__ qur,
                                                     const float* __restrict__ qer, const uint8_t* __restrict__ qdesc,
                                                     int* __restrict__ out_cnt, unsigned int* __restrict__ out_keys) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const float x = qx[q], y = qy[q], r = qr[q];
    const int minLevel = qminl[q], maxLevel = qmaxl[q];
    const u64 INV = ~0ull;
    u64 top[WT_K];
#pragma unroll
    for (int i = 0; i < WT_K; ++i) top[i] = INV;
    int cnt = 0;
    const int nMinCellX = max(0, (int)floorf((x - min_x - r) * inv_w));
    const int nMaxCellX = min(63, (int)ceilf((x - min_x + r) * inv_w));
    const int nMinCellY = max(0, (int)floorf((y - min_y - r) * inv_h));
    const int nMaxCellY = min(47, (int)ceilf((y - min_y + r) * inv_h));
    if (r >= 0 && nMinCellX < 64 && nMaxCellX >= 0 && nMinCellY < 48 && nMaxCellY >= 0) {
        const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
        const uint4* qp = (const uint4*)(qdesc + (size_t)q * 32);
        const uint4 qlo = qp[0], qhi = qp[1];
        const u64 a[4] = {(u64)qlo.x | ((u64)qlo.y << 32), (u64)qlo.z | ((u64)qlo.w << 32),
                          (u64)qhi.x | ((u64)qhi.y << 32), (u64)qhi.z | ((u64)qhi.w << 32)};
        const float er = qer ? qer[q] : -1.f, ur = qur ? qur[q] : 0.f;
        const unsigned long long lt = (1ull << lane) - 1ull;
        for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
            const int j0 = gs[ix * 48 + nMinCellY], j1 = gs[ix * 48 + nMaxCellY + 1];
            for (int jb = j0; jb < j1; jb += 64) {
                const int j = jb + lane;
                bool ok = false;
                int k = 0;
                if (j < j1) {
                    k = gi[j];
                    const KpIn kp = kps[k];
                    ok = true;
                    if (bCheckLevels) {
                        if (kp.octave < minLevel) ok = false;
                        if (maxLevel >= 0 && kp.octave > maxLevel) ok = false;
                    }
                    const float distx = kp.x - x, disty = kp.y - y;
                    if (!(fabsf(distx) < r && fabsf(disty) < r)) ok = false;
                    if (ok && er >= 0.f && uright) {
                        const float urk = uright[k];
                        if (urk > 0 && fabsf(ur - urk) > er) ok = false;
                    }
                }
                const unsigned long long bal = __ballot(ok);
                u64 key = INV;
                if (ok) {
                    const int pos = cnt + __popcll(bal & lt);
                    const uint4* tp = (const uint4*)(desc + (size_t)k * 32);
                    const uint4 lo = tp[0], hi = tp[1];
                    const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                                         (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
                    key = ((u64)d << 40) | ((u64)pos << 20) | (u64)k;
                }
                cnt += __popcll(bal);
                if (bal == 0) continue;
                // merge this chunk into the running top-K: pull its minima one by one until one no longer beats the K-th
                for (int rnd = 0; rnd < WT_K; ++rnd) {
                    const u64 m = wave_min_u64(key);
                    if (m >= top[WT_K - 1]) break;               // INV included
                    if (key == m) key = INV;                     // keys are unique (position)
                    u64 c = m;
#pragma unroll
                    for (int i = 0; i < WT_K; ++i) { const u64 t = top[i]; const bool sw = c < t; top[i] = sw ? c : t; c = sw ? t : c; }
                }
            }
        }
    }
    if (lane == 0) {
        out_cnt[q] = cnt;
#pragma unroll
        for (int i = 0; i < WT_K; ++i)                            // the array position carries the (distance, visiting order) rank: 32 bits suffice
            out_keys[(size_t)q * WT_K + i] = top[i] == INV ? 0xFFFFFFFFu : (unsigned)((top[i] >> 40) << 20) | (unsigned)(top[i] & 0xFFFFFu);
    }
}

// ------------------------------------------------------------------------------------------------
// k_pairdist: Hamming distances for a job list (bucket joins of SearchByBoW / SearchForTriangulation_).
// job j: query row q1[j] of set 1 against rows idx2[l2[j] .. l2[j]+len[j]) of set 2, outputs at off[j]...
// One thread per output element (the job is found by binary search in the output offsets).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pairdist(const uint8_t* __restrict__ d1, const uint8_t* __restrict__ d2,
                                                  const int* __restrict__ idx2, int njobs, const int* __restrict__ jq,
                                                  const int* __restrict__ jl2, const int* __restrict__ joff, int total,
                                                  int* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int lo = 0, hi = njobs;                                                   // last job with joff <= e
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (joff[mid] <= e) lo = mid; else hi = mid; }
    const int k2 = idx2[jl2[lo] + (e - joff[lo])];
    const uint4* p1 = (const uint4*)(d1 + (size_t)jq[lo] * 32);
    const uint4* p2 = (const uint4*)(d2 + (size_t)k2 * 32);
    const uint4 a0 = p1[0], a1 = p1[1], b0 = p2[0], b1 = p2[1];
    out[e] = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
             __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// ------------------------------------------------------------------------------------------------
// k_stereo: Frame::ComputeStereoMatches (Frame.cc:1027-1256) up to (not including) the median cut.
// One wavefront per left keypoint.  Candidates = right keypoints whose row band [floor(y-r), ceil(y+r)],
// r = 2*scale[octave], contains (int)vL (the reference's vRowIndices table, visited in iR order), octave within
// +-1 and u in [uL-maxD, uL]; best = min (distance, iR).  Then the 11x11 SAD slide over +-5 px on the two
// un-blurred pyramids, parabola refinement and the disparity gates, all in the reference's float arithmetic.
// ------------------------------------------------------------------------------------------------
struct StereoLevels { const uint8_t* L[12]; const uint8_t* R[12]; int pitchL[12], pitchR[12], wR[12]; float sf[12], isf[12]; };

// LV supplies the pyramids: sf(o), isf(o), L(level), R(level), pitchL(level), pitchR(level), wR(level)
// rowStart / rowIdx (optional): the reference's vRowIndices table (Frame.cc:1064-1083) as CSR over image rows -- the right
// keypoints whose band [floor(y - r), ceil(y + r)] covers a row; with it a left keypoint only looks at the ~20 keypoints of its
// row instead of all of them.  The winner is min (distance, iR) either way, so the order inside a row list does not matter.
// GS = lanes per left keypoint (64: one per wave; 16: four per wave -- the kernel is bound by its chain of dependent memory round trips
// at full occupancy, so the batched form quarters the number of waves that wait: 0.33 -> 0.21 ms per 256 pairs; 8 lanes: no further gain)
template <int GS, class LV>
__device__ __forceinline__ void stereo_body(const KpIn* __restrict__ kl, const uint8_t* __restrict__ dl, int nl,
                                            const KpIn* __restrict__ kr, const uint8_t* __restrict__ dr, int nr,
                                            const LV& lv, float mb, float mbf, float* __restrict__ uright,
                                            float* __restrict__ depth, int* __restrict__ bestSad, int iL,
                                            const int* __restrict__ rowStart = nullptr, const unsigned short* __restrict__ rowIdx = nullptr, int nrows = 0) {
    const int lane = threadIdx.x & (GS - 1), grp = (threadIdx.x & 63) / GS;
    const KpIn kpL = kl[iL];
    const int levelL = kpL.octave;
    const float vL = kpL.y, uL = kpL.x;
    const int rowL = (int)vL;
    const float minD = 0, maxD = mbf / mb;
    const float minU = uL - maxD, maxU = uL - minD;
    float ur_out = -1.0f, depth_out = -1.0f;
    int sad_out = -1;
    if (!(maxU < 0)) {
        const uint4* qp = (const uint4*)(dl + (size_t)iL * 32);
        const uint4 qlo = qp[0], qhi = qp[1];
        const u64 a[4] = {(u64)qlo.x | ((u64)qlo.y << 32), (u64)qlo.z | ((u64)qlo.w << 32),
                          (u64)qhi.x | ((u64)qhi.y << 32), (u64)qhi.z | ((u64)qhi.w << 32)};
        unsigned int best = 0xFFFFFFFFu;                                     // (dist << 16) | iR, strict < keeps the first
        float bestx = 0.f;                                                   // x of this lane's best candidate
        int c0 = 0, c1 = nr;
        if (rowStart) { if (rowL >= 0 && rowL < nrows) { c0 = rowStart[rowL]; c1 = rowStart[rowL + 1]; } else c1 = 0; }
        for (int b0 = c0; b0 < c1; b0 += GS) {
            const int ci = b0 + lane;
            const int iR = rowStart ? (ci < c1 ? (int)rowIdx[ci] : nr) : ci;
            if (iR < nr) {
                // the candidate's descriptor is requested together with its keypoint, not after the gates (the kernel is bound by its
                // chain of dependent memory round trips; a pair's right descriptors are 38 KB that stay in L2)
                const float rx = kr[iR].x, ry = kr[iR].y;
                const int ro = kr[iR].octave;
                const uint4* tp = (const uint4*)(dr + (size_t)iR * 32);
                const uint4 lo = tp[0], hi = tp[1];
                const float r = 2.0f * lv.sf(ro);
                const int maxr = (int)ceilf(ry + r), minr = (int)floorf(ry - r);
                if (rowL >= minr && rowL <= maxr && ro >= levelL - 1 && ro <= levelL + 1 && rx >= minU && rx <= maxU) {
                    const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                                         (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
                    const unsigned key = ((unsigned)d << 16) | (unsigned)iR;
                    if (key < best) { best = key; bestx = rx; }
                }
            }
        }
        const unsigned mine = best;
#pragma unroll
        for (int o = GS / 2; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o));
        const int bestDist = best == 0xFFFFFFFFu ? 100 : (int)(best >> 16);
        if (best != 0xFFFFFFFFu && bestDist < 100 && bestDist < 75) {        // < TH_HIGH to replace the init, < thOrbDist to go on
            // the winner's x comes from the lane that holds it (keys are unique: they carry the index), not from memory again
            unsigned long long who = __ballot(mine == best);
            if (GS < 64) who = (who >> (GS * grp)) & ((1ull << GS) - 1ull);   // this keypoint's lanes
            const float uR0 = __shfl(bestx, (int)__builtin_ctzll(who) + GS * grp);
            const float scaleFactor = lv.isf(levelL);
            const float scaleduL = roundf(kpL.x * scaleFactor), scaledvL = roundf(kpL.y * scaleFactor);
            const float scaleduR0 = roundf(uR0 * scaleFactor);
            const int w = 5, Lh = 5;
            const float iniu = scaleduR0 + Lh - w, endu = scaleduR0 + Lh + w + 1;
            if (!(iniu < 0 || endu >= (float)lv.wR(levelL))) {
                const uint8_t* IL = lv.L(levelL);
                const uint8_t* IR = lv.R(levelL);
                const int pl = lv.pitchL(levelL), pr = lv.pitchR(levelL);
                const int cy = (int)scaledvL, cxl = (int)scaleduL, cxr = (int)scaleduR0;
                int sad[11];
#pragma unroll
                for (int k = 0; k < 11; ++k) sad[k] = 0;
                for (int p = lane; p < 121; p += GS) {
                    const int dy = p / 11 - w, dx = p % 11 - w;
                    const unsigned vl = IL[(size_t)(cy + dy) * pl + cxl + dx];
                    const uint8_t* rr = IR + (size_t)(cy + dy) * pr + cxr + dx;
                    // the 11 right pixels rr[-5..5] as three dword loads (global memory takes any alignment) instead of 11 byte loads;
                    // v_sad_u8 on single-byte operands is |a - b| + accumulator in one instruction
                    typedef unsigned int u32a __attribute__((aligned(1)));
                    const unsigned w0 = *(const u32a*)(rr - 5), w1 = *(const u32a*)(rr - 1), w2 = *(const u32a*)(rr + 3);
#pragma unroll
                    for (int k = 0; k < 11; ++k) {
                        const unsigned wk = k < 4 ? w0 : k < 8 ? w1 : w2;
                        sad[k] = (int)__builtin_amdgcn_sad_u8(vl, (wk >> (8 * (k & 3))) & 0xFFu, (unsigned)sad[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 11; ++k)
#pragma unroll
                    for (int o = GS / 2; o > 0; o >>= 1) sad[k] += __shfl_xor(sad[k], o);
                int bestD = 0x7FFFFFFF, bestinc = 0;
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const float dist = (float)sad[k];
                    if (dist < (float)bestD) { bestD = (int)dist; bestinc = k - Lh; }
                }
                if (!(bestinc == -Lh || bestinc == Lh)) {
                    float d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
                    for (int k = 1; k < 10; ++k) if (k - Lh == bestinc) { d1 = (float)sad[k - 1]; d2 = (float)sad[k]; d3 = (float)sad[k + 1]; }
                    const float deltaR = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2));
                    if (!(deltaR < -1 || deltaR > 1)) {
                        float bestuR = lv.sf(levelL) * ((float)scaleduR0 + (float)bestinc + deltaR);
                        float disparity = (uL - bestuR);
                        if (disparity >= minD && disparity < maxD) {
                            if (disparity <= 0) { disparity = 0.01; bestuR = (float)((double)uL - 0.01); }
                            depth_out = mbf / disparity;
                            ur_out = bestuR;
                            sad_out = bestD;
                        }
                    }
                }
            }
        }
    }
    if (lane == 0) { uright[iL] = ur_out; depth[iL] = depth_out; bestSad[iL] = sad_out; }
}

struct StereoLevelsView {                                  // accessor form of StereoLevels (one pair: orbm_stereo_matches)
    const StereoLevels& s;
    __device__ float sf(int o) const { return s.sf[o]; }
    __device__ float isf(int o) const { return s.isf[o]; }
    __device__ const uint8_t* L(int l) const { return s.L[l]; }
    __device__ const uint8_t* R(int l) const { return s.R[l]; }
    __device__ int pitchL(int l) const { return s.pitchL[l]; }
    __device__ int pitchR(int l) const { return s.pitchR[l]; }
    __device__ int wR(int l) const { return s.wR[l]; }
};
__global__ __launch_bounds__(256) void k_stereo(const KpIn* __restrict__ kl, const uint8_t* __restrict__ dl, int nl,
                                                const KpIn* __restrict__ kr, const uint8_t* __restrict__ dr, int nr,
                                                StereoLevels lv, float mb, float mbf, float* __restrict__ uright,
                                                float* __restrict__ depth, int* __restrict__ bestSad) {
    const int iL = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (iL >= nl) return;
    const StereoLevelsView v{lv};
    stereo_body<64>(kl, dl, nl, kr, dr, nr, v, mb, mbf, uright, depth, bestSad, iL);
}

// ------------------------------------------------------------------------------------------------
// Batched, device-resident stereo (config C3): pair p = frames (first_l + p, first_r + p) of ONE extractor batch whose
// result block (kps / desc / counts, [frames][cap]) and pyramids sit in HBM.  k_stereo_batch = k_stereo per pair;
// k_stereo_cut = the median cut of Frame.cc:1261-1275 on the device: sort the SAD of the pair's stereo points, take the
// element at size/2, drop every point with SAD >= 1.5f*1.4f*median.
// ------------------------------------------------------------------------------------------------
struct StereoBatchLayout {                                  // where an extractor keeps a batch's pyramids (orbx_internal_batch_layout)
    const uint8_t* const* l0; int l0pitch; const uint8_t* pyr; size_t frameBytes;
    int off[12], pitch[12], w[12]; float sf[12], isf[12];
};
struct StereoBatchView {
    const StereoBatchLayout& b; int fl, fr;
    __device__ float sf(int o) const { return b.sf[o]; }
    __device__ float isf(int o) const { return b.isf[o]; }
    __device__ const uint8_t* L(int l) const { return l == 0 ? b.l0[fl] : b.pyr + (size_t)fl * b.frameBytes + b.off[l]; }
    __device__ const uint8_t* R(int l) const { return l == 0 ? b.l0[fr] : b.pyr + (size_t)fr * b.frameBytes + b.off[l]; }
    __device__ int pitchL(int l) const { return l == 0 ? b.l0pitch : b.pitch[l]; }
    __device__ int pitchR(int l) const { return l == 0 ? b.l0pitch : b.pitch[l]; }
    __device__ int wR(int l) const { return b.w[l]; }
};
// k_stereo_rows: vRowIndices of every pair's right image as CSR (Frame.cc:1064-1083): rowStart [npairs][nrows + 1],
// rowIdx [npairs][rowCap] (right keypoint indices; a keypoint enters the rows of its band).  One workgroup per pair: band
// histogram in LDS -> exclusive scan -> scatter.  Entries beyond rowCap are dropped and flagged (never with rowCap = 16 * cap).
__global__ __launch_bounds__(256) void k_stereo_rows(const KpIn* __restrict__ kps, const int* __restrict__ counts, int cap, int first_r,
                                                     StereoBatchLayout B, int nrows, int rowCap, int* __restrict__ rowStart,
                                                     unsigned short* __restrict__ rowIdx, int* __restrict__ err) {
    extern __shared__ int srow[];                                        // [nrows + 1] counts -> starts, then fill cursors [nrows]
    const int pair = blockIdx.x, tid = threadIdx.x, fr = first_r + pair;
    const int nr = min(counts[fr], cap);
    const KpIn* kr = kps + (size_t)fr * cap;
    int* cur = srow + nrows + 1;
    for (int i = tid; i <= nrows; i += 256) srow[i] = 0;
    __syncthreads();
    for (int i = tid; i < nr; i += 256) {
        const float r = 2.0f * B.sf[kr[i].octave];
        const int maxr = min((int)ceilf(kr[i].y + r), nrows - 1), minr = max((int)floorf(kr[i].y - r), 0);
        for (int y = minr; y <= maxr; ++y) atomicAdd(&srow[y], 1);
    }
    __syncthreads();
    if (tid < 64) {                                                      // exclusive scan of the row counts by one wave
        int carry = 0;
        for (int b0 = 0; b0 <= nrows; b0 += 64) {
            const int i = b0 + tid;
            const int v = i < nrows ? srow[i] : 0;
            int sc_ = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(sc_, o); if (tid >= o) sc_ += t; }
            if (i <= nrows) srow[i] = carry + sc_ - v;
            carry += __shfl(sc_, 63);
        }
    }
    __syncthreads();
    int* rs = rowStart + (size_t)pair * (nrows + 1);
    for (int i = tid; i <= nrows; i += 256) { rs[i] = min(srow[i], rowCap); if (i < nrows) cur[i] = srow[i]; }
    __syncthreads();
    unsigned short* ri = rowIdx + (size_t)pair * rowCap;
    for (int i = tid; i < nr; i += 256) {
        const float r = 2.0f * B.sf[kr[i].octave];
        const int maxr = min((int)ceilf(kr[i].y + r), nrows - 1), minr = max((int)floorf(kr[i].y - r), 0);
        for (int y = minr; y <= maxr; ++y) {
            const int pos = atomicAdd(&cur[y], 1);
            if (pos < rowCap) ri[pos] = (unsigned short)i; else *err = 1;
        }
    }
}

__global__ __launch_bounds__(256) void k_stereo_batch(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ counts,
                                                      int cap, int first_l, int first_r, StereoBatchLayout B, float mb, float mbf,
                                                      float* __restrict__ uright, float* __restrict__ depth, int* __restrict__ bestSad,
                                                      const int* __restrict__ rowStart, const unsigned short* __restrict__ rowIdx, int nrows, int rowCap) {
    const int pair = blockIdx.y, fl = first_l + pair, fr = first_r + pair;
    const int nl = min(counts[fl], cap), nr = min(counts[fr], cap);
#ifndef ST_GS
#define ST_GS 16
#endif
    const int iL = blockIdx.x * (256 / ST_GS) + (threadIdx.x / ST_GS);   // 64 / ST_GS left keypoints per wave (ST_GS lanes each)
    if (iL >= nl) return;
    const StereoBatchView v{B, fl, fr};
    const size_t o = (size_t)pair * cap;
    if (nr == 0) { if ((threadIdx.x & (ST_GS - 1)) == 0) { uright[o + iL] = -1.0f; depth[o + iL] = -1.0f; bestSad[o + iL] = -1; } return; }
    stereo_body<ST_GS>(kps + (size_t)fl * cap, desc + (size_t)fl * cap * 32, nl, kps + (size_t)fr * cap, desc + (size_t)fr * cap * 32, nr, v, mb, mbf,
                uright + o, depth + o, bestSad + o, iL, rowStart ? rowStart + (size_t)pair * (nrows + 1) : nullptr,
                rowIdx ? rowIdx + (size_t)pair * rowCap : nullptr, nrows);
}

// the element of rank m/2 of the pair's SAD values (< 2^15: 121 pixels x 255) by a two-level histogram -- 256 bins of sad >> 7,
// then 128 bins of the low 7 bits inside the bin that holds the rank -- instead of sorting them
__global__ __launch_bounds__(256) void k_stereo_cut(const int* __restrict__ counts, int cap, int first_l, int n2, const int* __restrict__ bestSad,
                                                    float* __restrict__ uright, float* __restrict__ depth, int* __restrict__ kept) {
    __shared__ int hist[256];
    __shared__ int s_m, s_bin, s_before, s_med, s_kept;
    (void)n2;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int nl = min(counts[first_l + pair], cap);
    const size_t o = (size_t)pair * cap;
    hist[tid] = 0;
    if (tid == 0) { s_m = 0; s_kept = 0; }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < nl; i += 256) { const int v = bestSad[o + i]; if (v >= 0) { atomicAdd(&hist[min(v >> 7, 255)], 1); ++mine; } }
    atomicAdd(&s_m, mine);
    __syncthreads();
    const int m = s_m;
    if (m == 0) { if (tid == 0) kept[pair] = 0; return; }
    const int rank = m / 2;                                                  // vDistIdx[size / 2] of the sorted list (Frame.cc:1263)
    auto locate = [&](int r, int nb) {                                       // bin whose cumulative count first exceeds r; s_before = count below it
        if (tid < 64) {
            int carry = 0;
            for (int b0 = 0; b0 < nb; b0 += 64) {
                const int v = hist[b0 + tid];
                int inc = v;
#pragma unroll
                for (int s_ = 1; s_ < 64; s_ <<= 1) { const int t = __shfl_up(inc, s_); if (tid >= s_) inc += t; }
                const unsigned long long hit = __ballot(carry + inc > r);
                if (hit) {
                    const int l = __builtin_ctzll(hit);
                    if (tid == l) { s_bin = b0 + l; s_before = carry + inc - v; }
                    break;
                }
                carry += __shfl(inc, 63);
            }
        }
    };
    locate(rank, 256);
    __syncthreads();
    const int hb = s_bin, before = s_before;
    __syncthreads();
    if (tid < 128) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < nl; i += 256) { const int v = bestSad[o + i]; if (v >= 0 && min(v >> 7, 255) == hb) atomicAdd(&hist[hb == 255 ? min(v - (255 << 7), 127) : (v & 127)], 1); }
    __syncthreads();
    locate(rank - before, 128);
    __syncthreads();
    if (tid == 0) s_med = (hb << 7) + s_bin;
    __syncthreads();
    const float median = (float)s_med;
    const float thDist = 1.5f * 1.4f * median;
    mine = 0;
    for (int i = tid; i < nl; i += 256) {
        const int sdv = bestSad[o + i];
        if (sdv < 0) continue;
        if ((float)sdv < thDist) ++mine;
        else { uright[o + i] = -1.0f; depth[o + i] = -1.0f; }
    }
    atomicAdd(&s_kept, mine);
    __syncthreads();
    if (tid == 0) kept[pair] = s_kept;
}

// ------------------------------------------------------------------------------------------------
// k_triangulate_batch: ORBmatcher::SearchForTriangulation_ (ORBmatcher.cc:1388-1629, pinhole, orientation check off as
// LocalMapping calls it) for a batch of KeyFrame pairs held in extractor result blocks.  One wavefront per feature of
// KeyFrame 1.  Its bucket = the features of KeyFrame 2 with the same vocabulary node (FeatureVector order = ascending
// index).  The reference walks the bucket keeping `dist <= TH_LOW && dist <= bestDist` candidates that pass the epipole /
// epipolar gates, so the survivor is the smallest distance among the gate-passing candidates and, on ties, the LAST one:
// a min-reduction over keys (dist << 16 | 0xFFFF - idx2).  vbMatched2 is not kept by this overload (:1567), so the
// features of KeyFrame 1 are independent.
// ------------------------------------------------------------------------------------------------
struct TriParams { float F12[9]; float epx, epy; float sf2[12], sigma2[12]; int onlyStereo, coarse; };
// k_tri_buckets: the features of every KeyFrame 2 grouped by (vocabulary node & 255): bStart [npairs][257], bIdx [npairs][cap].
// A FeatureVector bucket is then one short list (plus the few features of other nodes that share the low byte, filtered by
// the exact node id in the search); the order inside a list does not matter to k_triangulate_batch's min-key reduction.
__global__ __launch_bounds__(256) void k_tri_buckets(const int* __restrict__ counts2, const int* __restrict__ node2, int cap,
                                                     int* __restrict__ bStart, unsigned short* __restrict__ bIdx) {
    __shared__ int hist[257], cur[256];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n2 = min(counts2[pair], cap);
    const int* nd = node2 + (size_t)pair * cap;
    hist[tid] = 0; if (tid == 0) hist[256] = 0;
    __syncthreads();
    for (int i = tid; i < n2; i += 256) atomicAdd(&hist[nd[i] & 255], 1);
    __syncthreads();
    if (tid < 64) {
        int carry = 0;
        for (int b0 = 0; b0 < 256; b0 += 64) {
            const int v = hist[b0 + tid];
            int sc_ = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(sc_, o); if (tid >= o) sc_ += t; }
            hist[b0 + tid] = carry + sc_ - v;
            carry += __shfl(sc_, 63);
        }
        if (tid == 0) hist[256] = carry;
    }
    __syncthreads();
    bStart[(size_t)pair * 257 + tid] = hist[tid]; if (tid == 0) bStart[(size_t)pair * 257 + 256] = hist[256];
    cur[tid] = hist[tid];
    __syncthreads();
    for (int i = tid; i < n2; i += 256) bIdx[(size_t)pair * cap + atomicAdd(&cur[nd[i] & 255], 1)] = (unsigned short)i;
}

__global__ __launch_bounds__(256) void k_triangulate_batch(const KpIn* __restrict__ kps1, const uint8_t* __restrict__ desc1, const int* __restrict__ counts1,
                                                           const int* __restrict__ node1, const float* __restrict__ ur1,
                                                           const KpIn* __restrict__ kps2, const uint8_t* __restrict__ desc2, const int* __restrict__ counts2,
                                                           const int* __restrict__ node2, const float* __restrict__ ur2,
                                                           int cap, TriParams P, int* __restrict__ matches12, int* __restrict__ nmatches,
                                                           const int* __restrict__ bStart, const unsigned short* __restrict__ bIdx) {
    // one THREAD per feature of KeyFrame 1 (a bucket holds a dozen candidates: a wave per feature spent its time on the chain of
    // dependent loads, not on the distances); the bucket is walked serially, the survivor is the min of (dist << 16 | 0xFFFF - idx2)
    const int pair = blockIdx.y;
    const int n1 = min(counts1[pair], cap);
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    const size_t o = (size_t)pair * cap;
    int res = -1;
    if (i1 < n1) {
        const KpIn kp1 = kps1[o + i1];
        const int nd = node1[o + i1];
        const bool bStereo1 = ur1 && ur1[o + i1] >= 0;
        unsigned int best = 0xFFFFFFFFu;
        if (!(P.onlyStereo && !bStereo1)) {
            const uint4* qp = (const uint4*)(desc1 + (o + i1) * 32);
            const uint4 qlo = qp[0], qhi = qp[1];
            const u64 a[4] = {(u64)qlo.x | ((u64)qlo.y << 32), (u64)qlo.z | ((u64)qlo.w << 32),
                              (u64)qhi.x | ((u64)qhi.y << 32), (u64)qhi.z | ((u64)qhi.w << 32)};
            // the epipolar line of kp1 in image 2 (Pinhole::epipolarConstrain_, Pinhole.cpp:281-287)
            const float la = kp1.x * P.F12[0] + kp1.y * P.F12[3] + P.F12[6];
            const float lb = kp1.x * P.F12[1] + kp1.y * P.F12[4] + P.F12[7];
            const float lc = kp1.x * P.F12[2] + kp1.y * P.F12[5] + P.F12[8];
            const float den = la * la + lb * lb;
            const int c0 = bStart[(size_t)pair * 257 + (nd & 255)], c1 = bStart[(size_t)pair * 257 + (nd & 255) + 1];
            for (int ci = c0; ci < c1; ++ci) {
                const int i2 = (int)bIdx[o + ci];
                if (node2[o + i2] != nd) continue;
                const bool bStereo2 = ur2 && ur2[o + i2] >= 0;
                if (P.onlyStereo && !bStereo2) continue;
                const uint4* tp = (const uint4*)(desc2 + (o + i2) * 32);
                const uint4 lo = tp[0], hi = tp[1];
                const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                                     (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
                if (d > 50) continue;                                                // TH_LOW
                const KpIn kp2 = kps2[o + i2];
                if (!bStereo1 && !bStereo2) {
                    const float distex = P.epx - kp2.x, distey = P.epy - kp2.y;
                    if (distex * distex + distey * distey < 100 * P.sf2[kp2.octave]) continue;
                }
                bool epi = false;
                if (den != 0) {
                    const float num = la * kp2.x + lb * kp2.y + lc;
                    const float dsqr = num * num / den;
                    epi = (double)dsqr < 3.84 * (double)P.sigma2[kp2.octave];         // float compared with the double product, as written (Pinhole.cpp:295)
                }
                if (epi || P.coarse) best = min(best, ((unsigned)d << 16) | (0xFFFFu - (unsigned)i2));
            }
        }
        res = best == 0xFFFFFFFFu ? -1 : (int)(0xFFFFu - (best & 0xFFFFu));
        matches12[o + i1] = res;
    }
    const unsigned long long found = __ballot(res >= 0);
    if ((threadIdx.x & 63) == 0 && found) atomicAdd(&nmatches[pair], __popcll(found));
}

// ------------------------------------------------------------------------------------------------
// Batched, device-resident forms (frame-to-frame tracking with no host round trip).
// k_grid_build_batch: one workgroup per frame of an extractor result block [nframes][cap].
// k_track_window: wave per keypoint of the query frame; window = (x+dx, y+dy) +- th*scale[octave], levels
// [octave-1, octave+1] in the train frame's grid (the mono SearchByProjection window, ORBmatcher.cc:2543-2549);
// writes the first-minimum best and the runner-up (strict <, candidate order) -- the claim-free part of the search.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_grid_build_batch(const KpIn* __restrict__ kps, const int* __restrict__ counts, int cap, int n2,
                                                          float min_x, float min_y, float inv_w, float inv_h,
                                                          int* __restrict__ grid_start, int* __restrict__ grid_idx) {
    extern __shared__ unsigned int keys[];
    const int frame = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts[frame], cap);
    const KpIn* kp = kps + (size_t)frame * cap;
    __shared__ int s_placed;
    if (tid == 0) s_placed = 0;
    __syncthreads();
    for (int i = tid; i < n2; i += 256) {
        unsigned int key = 0xFFFFFFFFu;
        if (i < n) {
            const int px = (int)roundf((kp[i].x - min_x) * inv_w);
            const int py = (int)roundf((kp[i].y - min_y) * inv_h);
            if (px >= 0 && px < 64 && py >= 0 && py < 48) { key = ((unsigned)(px * 48 + py) << 16) | (unsigned)i; atomicAdd(&s_placed, 1); }
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned int a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    const int np = s_placed;
    int* gi = grid_idx + (size_t)frame * cap;
    int* gs = grid_start + (size_t)frame * (64 * 48 + 1);
    for (int i = tid; i < np; i += 256) gi[i] = (int)(keys[i] & 0xFFFFu);
    for (int c = tid; c <= 64 * 48; c += 256) {
        const unsigned int target = (unsigned)c << 16;
        int lo = 0, hi = np;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < target) lo = mid + 1; else hi = mid; }
        gs[c] = lo;
    }
}

struct ScaleTab { float sf[12]; };

// What every batched search is handed.  Pool: the searched rows of cap keypoint slots each (counts NULL where a search reads none) with
// their 64 x 48 grids in CSR form over the cell geometry (min_x, min_y, inv_w, inv_h).  PoolRow: one row of it (row()).  TopList: the
// candidate lists a *_topk kernel leaves for its claim replay, per query row the window population, its TK_K best candidates as
// words and the radius a rescan reads back (r NULL for the track kernels, whose replay derives it).
// The candidate kernels take Pool and TopList by value.  The one-wave claim replays (k_mm_claim apart) and k_track_topk16 keep loose __restrict__
// parameters and build the Pool in their first line: a by-value struct carries no noalias to the compiler, and these kernels'
// time follows their register allocation and code placement (profiles/NOTES.md).
struct PoolRow {
    const KpIn* kt; const uint8_t* dt; const int* gs; const int* gi;
    float min_x, min_y, inv_w, inv_h;
};
struct Pool {
    const KpIn* kps; const uint8_t* desc; const int* counts; int cap;
    const int* grid_start; const int* grid_idx;
    float min_x, min_y, inv_w, inv_h;
    __device__ __forceinline__ PoolRow row(size_t r) const {
        return PoolRow{kps + r * cap, desc + r * cap * 32, grid_start + r * (GRID_CELLS + 1), grid_idx + r * cap, min_x, min_y, inv_w, inv_h};
    }
};
struct TopList { int* cnt; unsigned int* keys; float* r; };
// the track kernels' pairing and window: query row q_first + pair against row t_first + pair, th * scale[octave] around (x + dx, y + dy);
// factor: the rotation histogram's bins per degree
struct TrackArgs { int q_first, t_first; float th, dx, dy, factor; };

__global__ __launch_bounds__(256) void k_track_window(Pool pool, TrackArgs A, ScaleTab st, int* __restrict__ best_idx, int* __restrict__ best_dist,
                                                      int* __restrict__ second_dist) {
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.y;
    const int qf = A.q_first + pair, tf = A.t_first + pair;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int cap = pool.cap;
    if (q >= min(pool.counts[qf], cap)) return;
    const KpIn kq = pool.kps[(size_t)qf * cap + q];
    const PoolRow T = pool.row(tf);
    const float x = kq.x + A.dx, y = kq.y + A.dy, r = A.th * st.sf[kq.octave];
    const int minLevel = kq.octave - 1, maxLevel = kq.octave + 1;
    unsigned int best = 0xFFFFFFFFu;                                        // (dist << 16 | order): first minimum in candidate order
    int second = 256, bestk = -1;
    const int nMinCellX = max(0, (int)floorf((x - T.min_x - r) * T.inv_w));
    const int nMaxCellX = min(63, (int)ceilf((x - T.min_x + r) * T.inv_w));
    const int nMinCellY = max(0, (int)floorf((y - T.min_y - r) * T.inv_h));
    const int nMaxCellY = min(47, (int)ceilf((y - T.min_y + r) * T.inv_h));
    int ord0 = 0;
    int bd = 256, bk = -1, sd = 256;                                        // per-lane partials
    unsigned int bo = 0xFFFFFFFFu;
    if (nMinCellX < 64 && nMaxCellX >= 0 && nMinCellY < 48 && nMaxCellY >= 0) {
        const uint4* qp = (const uint4*)(pool.desc + ((size_t)qf * cap + q) * 32);
        const uint4 qlo = qp[0], qhi = qp[1];
        const u64 a[4] = {(u64)qlo.x | ((u64)qlo.y << 32), (u64)qlo.z | ((u64)qlo.w << 32),
                          (u64)qhi.x | ((u64)qhi.y << 32), (u64)qhi.z | ((u64)qhi.w << 32)};
        for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
            const int j0 = T.gs[ix * 48 + nMinCellY], j1 = T.gs[ix * 48 + nMaxCellY + 1];
            for (int jb = j0; jb < j1; jb += 64) {
                const int j = jb + lane;
                if (j < j1) {
                    const int k = T.gi[j];
                    const KpIn kp = T.kt[k];
                    bool ok = !(kp.octave < minLevel) && !(kp.octave > maxLevel);   // bCheckLevels is true here (maxLevel >= 0)
                    if (!(fabsf(kp.x - x) < r && fabsf(kp.y - y) < r)) ok = false;
                    if (ok) {
                        const uint4* tp = (const uint4*)(T.dt + (size_t)k * 32);
                        const uint4 lo = tp[0], hi = tp[1];
                        const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                                             (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
                        const unsigned int key = ((unsigned)d << 20) | (unsigned)(ord0 + (j - j0));   // order within the whole sweep
                        if (key < bo) { sd = bd; bo = key; bd = d; bk = k; }
                        else if (d < sd) sd = d;
                    }
                }
            }
            ord0 += j1 - j0;
        }
    }
    // wave merge of (best key, runner-up distance): runner-up = min over all candidates except the winner
    unsigned int wbest = bo;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wbest = min(wbest, (unsigned)__shfl_xor((int)wbest, o));
    int cand2 = (bo == wbest) ? sd : bd;                                     // lanes that lost contribute their own best
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand2 = min(cand2, __shfl_xor(cand2, o));
    best = wbest; second = cand2;
    const unsigned long long who = __ballot(bo == wbest && wbest != 0xFFFFFFFFu);
    if (who) bestk = __shfl(bk, __ffsll((long long)who) - 1);
    if (lane == 0) {
        const size_t o = (size_t)pair * cap + q;
        best_idx[o] = bestk;
        best_dist[o] = bestk < 0 ? 256 : (int)(best >> 20);
        second_dist[o] = second;
    }
}

// ------------------------------------------------------------------------------------------------
// Batched SearchByProjection(Frame, Frame), final matches on the device (ORBmatcher.cc:2469-2711, mono branch).
// k_track_topk: wave per query keypoint (same window as k_track_window).  What the sequential claim replay can ever look at:
//   the window's candidate count and its TK_K best candidates in (distance, visiting order) rank -- the order in which the
//   reference's `dist < bestDist` scan would prefer them -- each as ONE word: dist << 21 | rotation bin << 16 | keypoint index
//   (bin = round((angle_q - angle_t [+360]) * 30/360), 30 -> 0, ORBmatcher.cc:2596-2603; the replay needs no second gather).
// k_track_claim: ONE wave per frame pair replays the claims in query order (:2555-2593): a query takes its first candidate that is
//   not blocked (a MapPoint with observations already sits there: cur_blocked, or an earlier query with observations claimed it,
//   :2565-2567), bestDist <= TH_HIGH assigns the slot (:2589-2592), the rotation histogram keeps (slot, bin) of every assignment
//   and the three-maxima cull clears the others (:2690-2708).  Eight queries' lists (8 x 8 keys) are fetched per round trip and the
//   next eight are requested before the current ones are resolved; the blocked set is a bit array in LDS, claims inside a group
//   travel by register compare.  A query whose TK_K listed candidates are all blocked although its window holds more is rescanned
//   in place, blocked set applied (rare; the single-frame host replay falls back to full lists in the same case).
// ------------------------------------------------------------------------------------------------
#define TK_K 8                                                              // candidates listed per query, every batched search (track, M3, M4)
#define TK_NOBIN 31
// wave-wide minimum of a 32-bit key by DPP (six v_min_u32 with data movement folded in; the result of a full reduction sits in lane 63)
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// minimum over the 16 lanes of a DPP row, in every lane of the row (four rotations)
__device__ __forceinline__ unsigned row16_min_u32(unsigned v) {
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xf, 0xf, false));   // row_ror:8
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124, 0xf, 0xf, false));   // row_ror:4
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x122, 0xf, 0xf, false));   // row_ror:2
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x121, 0xf, 0xf, false));   // row_ror:1
    return v;
}
__device__ __forceinline__ int wave_excl_scan(int v, int* total) {           // exclusive prefix sum over the 64 lanes
    int s = v;
    s += __builtin_amdgcn_update_dpp(0, s, 0x111, 0xf, 0xf, true);
    s += __builtin_amdgcn_update_dpp(0, s, 0x112, 0xf, 0xf, true);
    s += __builtin_amdgcn_update_dpp(0, s, 0x114, 0xf, 0xf, true);
    s += __builtin_amdgcn_update_dpp(0, s, 0x118, 0xf, 0xf, true);
    s += __builtin_amdgcn_update_dpp(0, s, 0x142, 0xa, 0xf, false);
    s += __builtin_amdgcn_update_dpp(0, s, 0x143, 0xc, 0xf, false);
    *total = __builtin_amdgcn_readlane(s, 63);
    return s - v;
}

// ---- shared by the batched SearchByProjection kernels (track M4, M3 k_lp_*, motion-model M4 k_mm_*) ----
__device__ __forceinline__ void load_desc(const uint8_t* p, u64 (&a)[4]) {    // one 32-byte descriptor as four 64-bit words
    const uint4* qp = (const uint4*)p;
    const uint4 qlo = qp[0], qhi = qp[1];
    a[0] = (u64)qlo.x | ((u64)qlo.y << 32); a[1] = (u64)qlo.z | ((u64)qlo.w << 32);
    a[2] = (u64)qhi.x | ((u64)qhi.y << 32); a[3] = (u64)qhi.z | ((u64)qhi.w << 32);
}

// A GetFeaturesInArea window (Frame.cc:784-871): levels by the generic rule (bCheckLevels = minLevel > 0 || maxLevel >= 0, maxLevel < 0
// leaves the top open) and, with an mvuRight array, the stereo gate |ur - uR[k]| <= r of the right-projecting searches.
struct Win { float x, y, r, ur; int minLevel, maxLevel; };

// The 5-bit payload a candidate word carries: the candidate's octave + 1 (M3: the ratio test compares levels) or its rotation bin
// (M4: angle_q - angle_t as ORBmatcher.cc:2596-2603, TK_NOBIN outside [0, 30)).
struct OctavePay { __device__ unsigned operator()(const KpIn& kp) const { return (unsigned)(kp.octave + 1); } };
struct RotBinPay {
    float qangle, factor;
    __device__ unsigned operator()(const KpIn& kp) const {
        float rot = qangle - kp.angle;
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == 30) bin = 0;
        if (bin < 0 || bin >= 30) bin = TK_NOBIN;
        return (unsigned)bin;
    }
};

// One sweep of window w over a frame's grid (w wave-uniform, all 64 lanes).  The window's grid columns are flattened into one list
// (column ranges one per lane, prefix sum across the wave) and taken in passes of 64.  Grid positions j are monotone in the reference's
// visiting order (cell = ix * 48 + iy, cells ascending in the CSR), so (distance, j) ranks the candidates as the scan meets them.
// key = dist << 40 | j << 21 | payload << 16 | keypoint (j, keypoint < 65536).
// TOPK: cnt = window population, top[0..TK_K) = its TK_K smallest keys (wave-uniform).
// !TOPK: only candidates not blocked in blk; top[0], top[1] = the two smallest.
// Gate: a further candidate test after the window, level and stereo tests (Fuse's chi2 test, FuseGate); NoGate compiles to nothing.
struct NoGate {
    static constexpr bool on = false;
    __device__ bool operator()(const KpIn&, int) const { return true; }
};
template <bool TOPK, class Pay, class Gate = NoGate>
__device__ __forceinline__ void win_sweep(const Win& w, const Pay& pay, const PoolRow& T, const float* __restrict__ urt, const u64 (&a)[4],
                                          const unsigned int* blk, int lane, int& cnt, u64 (&top)[TK_K], const Gate& gate = Gate{}) {
    const u64 INV = ~0ull;
#pragma unroll
    for (int i = 0; i < TK_K; ++i) top[i] = INV;
    cnt = 0;
    const int nMinCellX = max(0, (int)floorf((w.x - T.min_x - w.r) * T.inv_w));
    const int nMaxCellX = min(63, (int)ceilf((w.x - T.min_x + w.r) * T.inv_w));
    const int nMinCellY = max(0, (int)floorf((w.y - T.min_y - w.r) * T.inv_h));
    const int nMaxCellY = min(47, (int)ceilf((w.y - T.min_y + w.r) * T.inv_h));
    if (!(w.r >= 0 && nMinCellX < 64 && nMaxCellX >= 0 && nMinCellY < 48 && nMaxCellY >= 0 && nMinCellX <= nMaxCellX && nMinCellY <= nMaxCellY)) return;
    const bool bCheckLevels = (w.minLevel > 0) || (w.maxLevel >= 0);
    const int loLevel = bCheckLevels ? w.minLevel : INT_MIN, hiLevel = bCheckLevels && w.maxLevel >= 0 ? w.maxLevel : INT_MAX;
    const int ncols = nMaxCellX - nMinCellX + 1;                             // 1 .. 64: one column per lane
    int cj0 = 0, clen = 0;
    if (lane < ncols) {
        const int ix = nMinCellX + lane;
        cj0 = T.gs[ix * 48 + nMinCellY];
        clen = T.gs[ix * 48 + nMaxCellY + 1] - cj0;
    }
    int total;
    const int excl = wave_excl_scan(clen, &total);
    u64 b1 = INV, b2 = INV;                                                  // !TOPK: the lane's two smallest
    for (int base = 0; base < total; base += 64) {
        const int t = base + lane;
        int cs = 0, c0 = 0;
        for (int c = 0; c < ncols; ++c) {                                    // t's column: the last one starting at or before t
            const int e = __builtin_amdgcn_readlane(excl, c), s = __builtin_amdgcn_readlane(cj0, c);
            if (t >= e) { cs = e; c0 = s; }
        }
        bool ok = false;
        u64 key = INV;
        if (t < total) {
            const int j = c0 + (t - cs);
            const int k = T.gi[j];
            const KpIn kp = T.kt[k];
            ok = (kp.octave >= loLevel) & (kp.octave <= hiLevel) & (fabsf(kp.x - w.x) < w.r) & (fabsf(kp.y - w.y) < w.r);   // (no short cut: one x, y load)
            if (ok && urt) {
                const float urk = urt[k];
                if (urk > 0 && fabsf(w.ur - urk) > w.r) ok = false;            // ORBmatcher.cc:107-117, :2569-2576
            }
            if (Gate::on && ok && !gate(kp, k)) ok = false;
            if (!TOPK && ok && ((blk[k >> 5] >> (k & 31)) & 1u)) ok = false;
            if (ok) {
                const uint4* tp = (const uint4*)(T.dt + (size_t)k * 32);
                const uint4 lo = tp[0], hi = tp[1];
                const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                                     (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
                key = ((u64)d << 40) | ((u64)j << 21) | ((u64)pay(kp) << 16) | (u64)k;
            }
        }
        if (TOPK) {
            const unsigned long long bal = __ballot(ok);
            cnt += __popcll(bal);
            if (bal == 0) continue;
            for (int rnd = 0; rnd < TK_K; ++rnd) {                           // merge: pull the chunk's minima until one no longer beats the K-th
                const u64 m = wave_min_u64(key);
                if (m >= top[TK_K - 1]) break;
                if (key == m) key = INV;                                     // keys are unique (grid position)
                u64 c = m;
#pragma unroll
                for (int i = 0; i < TK_K; ++i) { const u64 tt = top[i]; const bool sw = c < tt; top[i] = sw ? c : tt; c = sw ? tt : c; }
            }
        } else {
            if (key < b1) { b2 = b1; b1 = key; }
            else if (key < b2) b2 = key;
        }
    }
    if (!TOPK) {
        const u64 m1 = wave_min_u64(b1);
        top[0] = m1;
        top[1] = wave_min_u64(b1 == m1 ? b2 : b1);                          // the winner's lane offers its runner-up
    }
}

__device__ __forceinline__ unsigned int cand_word(u64 key) {                 // dist << 21 | payload << 16 | keypoint, or 0xFFFFFFFF
    return key == ~0ull ? 0xFFFFFFFFu : ((unsigned)(key >> 40) << 21) | (unsigned)(key & 0x1FFFFFu);
}

// word w of an LDS bit array over a byte array: bit b = src[32 w + b] != 0 for 32 w + b < n.  src NULL: dflt (0 for a blocked set:
// nothing blocked; ~0 for "observed": every query counts).  32 byte loads in flight (clamped, not predicated), then the bits.
__device__ __forceinline__ unsigned int bits_word(const uint8_t* __restrict__ src, int n, int w, unsigned int dflt) {
    if (!src) return dflt;
    const int last = max(n - 1, 0);
    unsigned v[32];
#pragma unroll
    for (int b = 0; b < 32; ++b) v[b] = src[min(w * 32 + b, last)];
    unsigned int bits = 0;
#pragma unroll
    for (int b = 0; b < 32; ++b) if (w * 32 + b < n && v[b]) bits |= 1u << b;
    return bits;
}

// ComputeThreeMaxima (ORBmatcher.cc:2870-2909) on the 30 bin counts: the kept bins, -1 where the 0.1 rule drops one
struct Max3 { int i1, i2, i3; };
__device__ __forceinline__ Max3 three_maxima(const unsigned int* hist) {
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < 30; ++i) {
        const int sz = (int)hist[i];
        if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; i3 = i2; i2 = i1; i1 = i; }
        else if (sz > max2) { max3 = max2; max2 = sz; i3 = i2; i2 = i; }
        else if (sz > max3) { max3 = sz; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) i3 = -1;
    return Max3{i1, i2, i3};
}

// three_maxima on the bin counts, then every assignment acc[0..nacc) (slot | bin << 16) of another bin is cleared (:2696-2707) as
// ORBM_MATCH_PRUNED.  Returns the number of pruned entries (wave-uniform).
__device__ __forceinline__ int rot_cull(const unsigned int* hist, const unsigned int* acc, int nacc, int* mrow, int lane) {
    const Max3 m3 = three_maxima(hist);
    const int i1 = m3.i1, i2 = m3.i2, i3 = m3.i3;
    int pruned = 0;
    for (int e = lane; e < nacc; e += 64) {
        const unsigned int v = acc[e];
        const int bin = (int)(v >> 16), k = (int)(v & 0xFFFFu);
        if (bin != i1 && bin != i2 && bin != i3) { mrow[k] = -2; ++pruned; }      // ORBM_MATCH_PRUNED
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pruned += __shfl_xor(pruned, o);
    return pruned;
}

// row o of a TopList
__device__ __forceinline__ void put_topk(const TopList& out, size_t o, int cnt, float r, const u64 (&top)[TK_K]) {
    out.cnt[o] = cnt;
    out.r[o] = r;
    uint4* ok = (uint4*)(out.keys + o * TK_K);
    ok[0] = make_uint4(cand_word(top[0]), cand_word(top[1]), cand_word(top[2]), cand_word(top[3]));
    ok[1] = make_uint4(cand_word(top[4]), cand_word(top[5]), cand_word(top[6]), cand_word(top[7]));
}

#ifdef ORBX_AB   /* A/B reference (a wave per query), not in the product library */
// The window's grid columns are flattened into ONE candidate list (column starts / lengths loaded by one lane each, prefix sum across
// lanes), so that a window of up to 64 candidates costs four dependent round trips (cell ranges, indices, keypoints, descriptors)
// whatever its shape -- the per-column loop of k_track_window pays them per column -- and the eight best come out of eight DPP
// minimum reductions of a 32-bit key (distance << 16 | position), already in rank order.
__global__ __launch_bounds__(256) void k_track_topk(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                    const int* __restrict__ counts, int cap, const int* __restrict__ grid_start,
                                                    const int* __restrict__ grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                                                    int q_first, int t_first, float th, ScaleTab st, float dx, float dy, float factor,
                                                    int* __restrict__ out_cnt, unsigned int* __restrict__ out_keys) {
    const Pool pool{kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h};
    const TrackArgs A{q_first, t_first, th, dx, dy, factor};
    const TopList out{out_cnt, out_keys, nullptr};
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.y;
    const int qf = A.q_first + pair, tf = A.t_first + pair;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= min(pool.counts[qf], cap)) return;
    const KpIn kq = pool.kps[(size_t)qf * cap + q];
    const PoolRow T = pool.row(tf);
    const float x = kq.x + A.dx, y = kq.y + A.dy, r = A.th * st.sf[kq.octave];
    const int minLevel = kq.octave - 1, maxLevel = kq.octave + 1;
    const unsigned INV = 0xFFFFFFFFu;
    unsigned topKey[TK_K], topPay[TK_K];                                   // (distance << 16 | position) ascending; payload = bin << 16 | keypoint
#pragma unroll
    for (int i = 0; i < TK_K; ++i) { topKey[i] = INV; topPay[i] = INV; }
    int cnt = 0;
    const int nMinCellX = max(0, (int)floorf((x - T.min_x - r) * T.inv_w));
    const int nMaxCellX = min(63, (int)ceilf((x - T.min_x + r) * T.inv_w));
    const int nMinCellY = max(0, (int)floorf((y - T.min_y - r) * T.inv_h));
    const int nMaxCellY = min(47, (int)ceilf((y - T.min_y + r) * T.inv_h));
    if (nMinCellX < 64 && nMaxCellX >= 0 && nMinCellY < 48 && nMaxCellY >= 0) {
        const uint4* qp = (const uint4*)(pool.desc + ((size_t)qf * cap + q) * 32);
        const uint4 qlo = qp[0], qhi = qp[1];
        const u64 a[4] = {(u64)qlo.x | ((u64)qlo.y << 32), (u64)qlo.z | ((u64)qlo.w << 32),
                          (u64)qhi.x | ((u64)qhi.y << 32), (u64)qhi.z | ((u64)qhi.w << 32)};
        const unsigned long long lt = (1ull << lane) - 1ull;
        const int ncols = nMaxCellX - nMinCellX + 1;                       // <= 64 (the grid has 64 columns)
        int cj0 = 0, clen = 0;
        if (lane < ncols) {
            const int ix = nMinCellX + lane;
            cj0 = T.gs[ix * 48 + nMinCellY];
            clen = T.gs[ix * 48 + nMaxCellY + 1] - cj0;
        }
        int total;
        const int coff = wave_excl_scan(clen, &total);
        bool first = true;
        for (int base = 0; base < total; base += 64) {
            const int t = base + lane;
            // the lane's column: the last one whose offset is <= t (columns in ascending order, empty ones share an offset)
            int myj0 = 0, myoff = 0;
            for (int c = 0; c < ncols; ++c) {
                const int oc = __builtin_amdgcn_readlane(coff, c), jc = __builtin_amdgcn_readlane(cj0, c);
                if (t >= oc) { myoff = oc; myj0 = jc; }
            }
            bool ok = false;
            int k = 0;
            float ang = 0.f;
            if (t < total) {
                k = T.gi[myj0 + (t - myoff)];
                const KpIn kp = T.kt[k];
                ok = !(kp.octave < minLevel) && !(kp.octave > maxLevel);   // bCheckLevels is true here (maxLevel >= 0)
                if (!(fabsf(kp.x - x) < r && fabsf(kp.y - y) < r)) ok = false;
                ang = kp.angle;
            }
            const unsigned long long bal = __ballot(ok);
            if (bal == 0) continue;
            unsigned key = INV, pay = INV;
            if (ok) {
                const int pos = cnt + __popcll(bal & lt);
                const uint4* tp = (const uint4*)(T.dt + (size_t)k * 32);
                const uint4 lo = tp[0], hi = tp[1];
                const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                                     (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
                float rot = kq.angle - ang;
                if (rot < 0.0f) rot += 360.0f;
                int bin = (int)roundf(rot * A.factor);
                if (bin == 30) bin = 0;
                if (bin < 0 || bin >= 30) bin = TK_NOBIN;
                key = ((unsigned)d << 16) | (unsigned)pos;                   // positions < 65536 (cap)
                pay = ((unsigned)bin << 16) | (unsigned)k;
            }
            cnt += __popcll(bal);
            if (first) {
                // first chunk: the minima come out in rank order
#pragma unroll
                for (int i = 0; i < TK_K; ++i) {
                    const unsigned m = wave_min_u32(key);
                    if (m == INV) break;
                    const int src = __ffsll((long long)__ballot(key == m)) - 1;     // keys are unique (position)
                    topKey[i] = m; topPay[i] = (unsigned)__builtin_amdgcn_readlane((int)pay, src);
                    if (lane == src) key = INV;
                }
                first = false;
            } else {
                for (int rnd = 0; rnd < TK_K; ++rnd) {                     // later chunks (windows of more than 64 grid entries): insertion
                    const unsigned m = wave_min_u32(key);
                    if (m >= topKey[TK_K - 1]) break;                      // INV included
                    const int src = __ffsll((long long)__ballot(key == m)) - 1;
                    unsigned ck = m, cp = (unsigned)__builtin_amdgcn_readlane((int)pay, src);
                    if (lane == src) key = INV;
#pragma unroll
                    for (int i = 0; i < TK_K; ++i) {
                        const bool sw = ck < topKey[i];
                        const unsigned tk = topKey[i], tp2 = topPay[i];
                        topKey[i] = sw ? ck : tk; topPay[i] = sw ? cp : tp2;
                        ck = sw ? tk : ck; cp = sw ? tp2 : cp;
                    }
                }
            }
        }
    }
    if (lane == 0) {
        const size_t o = (size_t)pair * cap + q;
        out.cnt[o] = cnt;
#pragma unroll
        for (int i = 0; i < TK_K; ++i)
            out.keys[o * TK_K + i] = topKey[i] == INV ? 0xFFFFFFFFu : ((topKey[i] >> 16) << 21) | (topPay[i] & 0x1FFFFFu);
    }
}

#endif  /* ORBX_AB */

// k_track_topk16: the same lists with SIXTEEN lanes per query (four queries per wave).  A mono window (th = 15) holds 6 grid entries at
// level 0 and ~40 at level 7 (14 on average over a 1000-feature frame), so a wave per query keeps most lanes idle and the kernel is bound
// by the number of waves it can keep in flight across five dependent round trips.  A lane owns entries t = base + 16 j + l (j < NJ <= 4:
// up to 64 entries per query and pass); column ranges sit in LDS (row-local prefix sums by DPP row_shr); the entries that pass the
// level and window tests are packed to one per lane before their descriptors are read (tk16_pass); the eight best come from each
// lane counting the smaller keys of its row (DPP row_ror), and later passes (windows of more than 64 grid entries) and further
// rounds (rows of more than 16 candidates) merge into the LDS list by row-wide minimum reductions whose winner writes its own word,
// the list competing as one more key per lane.  The record loads are BRANCH-FREE per NJ (inactive entries read row 0 instead of
// being predicated off), so that the NJ loads of a pass are in flight together; consecutive queries sit on the same pyramid level
// (similar windows), so NJ is chosen per wave.
struct Tk16 {
    const uint4* ent; const uint8_t* dt; int cap;
    float x, y, r, qangle, factor; int minLevel, maxLevel;
    int total, ncols, qr, l16, wr;
};
// one candidate of a lane: the distance, the rotation bin (ORBmatcher.cc:2596-2603), the key (distance << 16 | position) and the word
__device__ __forceinline__ void tk16_cand(const Tk16& c, const u64 (&a)[4], const uint4& lo, const uint4& hi, float ang, int k, int pos, bool ok,
                                          unsigned& key, unsigned& word) {
    const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32), (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
    float rot = c.qangle - ang;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * c.factor);
    if (bin == 30) bin = 0;
    if (bin < 0 || bin >= 30) bin = TK_NOBIN;
    key = ok ? ((unsigned)d << 16) | (unsigned)pos : 0xFFFFFFFFu;            // positions < 65536 (cap)
    word = ((unsigned)d << 21) | ((unsigned)bin << 16) | (unsigned)k;
}

// the row's list so far (one entry in each of its first TK_K lanes: pk, pw) merged with one more candidate per lane (k1, w1): TK_K row-wide
// minimum reductions, in rank order, whose winner writes its own word to the list
__device__ __forceinline__ void tk16_merge(const Tk16& c, unsigned k1, unsigned w1, unsigned pk, unsigned pw, uint2 (*sTop)[TK_K]) {
    const unsigned INV = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < TK_K; ++i) {
        const unsigned mine = min(k1, pk);
        const unsigned m = row16_min_u32(mine);
        if (!__any(m != INV)) break;
        if (mine == m && m != INV) {                                        // keys are unique (position): exactly one lane of the row
            sTop[c.qr][i] = make_uint2(m, pk == m ? pw : w1);
            if (pk == m) pk = INV; else k1 = INV;
        }
    }
}

// A pass FILTERS before it fetches: the level band and the window test need only an entry's 16-byte record, and of a window's entries
// about a quarter pass them.  So the records are loaded and tested first, the row positions taken from the ballots, and the survivors
// (keypoint, angle, position) packed through LDS to one per lane -- in visiting order -- before any descriptor is read: one descriptor
// load, one distance, one rotation bin and one key per LANE instead of one per ENTRY, and no descriptor held in registers per entry.
template <int NJ, bool FB>
__device__ __forceinline__ void tk16_pass(const Tk16& c, const u64 (&a)[4], int base, int& cnt, const int2 (*sCol)[64], const int (*sAdj)[64], uint2 (*sK)[16], uint2 (*sTop)[TK_K]) {
    const unsigned INV = 0xFFFFFFFFu;
    int t[NJ], eidx[NJ];
    const int cnt0 = cnt;
#pragma unroll
    for (int j = 0; j < NJ; ++j) t[j] = base + 16 * j + c.l16;
    if (!FB) {
        // first 64 entries of a window: the prologue left (grid position - list position) of every entry in LDS
#pragma unroll
        for (int j = 0; j < NJ; ++j) eidx[j] = t[j] < c.total ? t[j] + sAdj[c.qr][t[j]] : 0;
    } else {
        // later passes: each entry's column is the last one whose offset is <= t (columns ascending, empty ones share an offset)
        int off[NJ], j0[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) { off[j] = 0; j0[j] = 0; }
        for (int col = 0; __any(col < c.ncols); ++col) {
            const int2 e = sCol[c.qr][col];
            const bool in = col < c.ncols;
#pragma unroll
            for (int j = 0; j < NJ; ++j) if (in && t[j] >= e.x) { off[j] = e.x; j0[j] = e.y; }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) eidx[j] = t[j] < c.total ? j0[j] + (t[j] - off[j]) : 0;
    }
    // one 16-byte record per grid entry, in the grid's own order (k_track_pack): (x, y, angle, octave << 16 | keypoint) -- the entry and
    // its keypoint in ONE load from consecutive addresses instead of an index and three dependent scattered ones
    int k[NJ];
    float kx[NJ], ky[NJ], ang[NJ];
    int oct[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const uint4 e = c.ent[eidx[j]];
        kx[j] = __uint_as_float(e.x); ky[j] = __uint_as_float(e.y); ang[j] = __uint_as_float(e.z);
        oct[j] = (int)(e.w >> 16); k[j] = (int)(e.w & 0xFFFFu);
    }
    const unsigned below = (1u << c.l16) - 1u;
    bool ok[NJ];
    int posj[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        ok[j] = t[j] < c.total && !(oct[j] < c.minLevel) && !(oct[j] > c.maxLevel) && (fabsf(kx[j] - c.x) < c.r && fabsf(ky[j] - c.y) < c.r);   // bCheckLevels is true here
        const unsigned rowbits = (unsigned)(__ballot(ok[j]) >> (16 * c.wr)) & 0xFFFFu;
        posj[j] = cnt + __popc(rowbits & below);
        cnt += __popc(rowbits);
    }
    // rounds of 16 survivors per row, one per lane.  The rule is ONE round; a wave in which some row has more than 16 survivors (many
    // same-level keypoints inside one window) takes more, and every round after a window's first merges into the list like a later pass
    const int nv = cnt - cnt0;
#pragma unroll
    for (int r = 0; r < NJ; ++r) {
        if (r > 0 && !__any(nv > 16 * r)) break;
        bool ok1 = ok[0];
        int k1 = k[0], pos1 = posj[0];
        float ang1 = ang[0];
        if (NJ > 1) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int rel = posj[j] - cnt0 - 16 * r;
                if (ok[j] && (unsigned)rel < 16u) sK[c.qr][rel] = make_uint2(((unsigned)posj[j] << 16) | (unsigned)k[j], __float_as_uint(ang[j]));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint2 e = sK[c.qr][c.l16];
            ok1 = 16 * r + c.l16 < nv; k1 = (int)(e.x & 0xFFFFu); pos1 = (int)(e.x >> 16); ang1 = __uint_as_float(e.y);
        }
        const uint4* tp = (const uint4*)(c.dt + (size_t)(ok1 ? k1 : 0) * 32);   // unconditional: a lane without a survivor reads row 0
        const uint4 lo = tp[0], hi = tp[1];
        unsigned key, word;
        tk16_cand(c, a, lo, hi, ang1, k1, pos1, ok1, key, word);
        if (!FB && r == 0) {
            // the list is empty: each lane's rank is the number of smaller keys in its row (15 rotations; keys are unique by position)
            int rank = 0;
            unsigned rk = key;
#pragma unroll
            for (int i = 0; i < 15; ++i) {
                rk = (unsigned)__builtin_amdgcn_update_dpp((int)rk, (int)rk, 0x121, 0xf, 0xf, false);   // row_ror:1
                rank += rk < key ? 1 : 0;
            }
            if (key != INV && rank < TK_K) sTop[c.qr][rank] = make_uint2(key, word);
        } else {
            unsigned pk = INV, pw = INV;
            if (c.l16 < TK_K) { const uint2 pv = sTop[c.qr][c.l16]; pk = pv.x; pw = pv.y; }   // the list so far competes again
            tk16_merge(c, key, word, pk, pw, sTop);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");              // (the next round or pass reads the list and writes sK)
        __builtin_amdgcn_wave_barrier();
    }
}
struct Tk16Filter {
    template <int NJ, bool FB>
    static __device__ __forceinline__ void run(const Tk16& c, const u64 (&a)[4], int base, int& cnt, const int2 (*sCol)[64], const int (*sAdj)[64], uint2 (*sK)[16], uint2 (*sTop)[TK_K]) {
        tk16_pass<NJ, FB>(c, a, base, cnt, sCol, sAdj, sK, sTop);
    }
};

#ifdef ORBX_AB   /* A/B reference (descriptors and distances for every grid entry of the window), not in the product library */
template <int NJ, bool FB>
__device__ __forceinline__ void tk16_pass_v1(const Tk16& c, const u64 (&a)[4], int base, int& cnt, const int2 (*sCol)[64], const int (*sAdj)[64], uint2 (*sK)[16], uint2 (*sTop)[TK_K]) {
    const unsigned INV = 0xFFFFFFFFu;
    int t[NJ], eidx[NJ];
    const int cnt0 = cnt;
#pragma unroll
    for (int j = 0; j < NJ; ++j) t[j] = base + 16 * j + c.l16;
    if (!FB) {
        // first 64 entries of a window: the prologue left (grid position - list position) of every entry in LDS
#pragma unroll
        for (int j = 0; j < NJ; ++j) eidx[j] = t[j] < c.total ? t[j] + sAdj[c.qr][t[j]] : 0;
    } else {
        // later passes: each entry's column is the last one whose offset is <= t (columns ascending, empty ones share an offset)
        int off[NJ], j0[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) { off[j] = 0; j0[j] = 0; }
        for (int col = 0; __any(col < c.ncols); ++col) {
            const int2 e = sCol[c.qr][col];
            const bool in = col < c.ncols;
#pragma unroll
            for (int j = 0; j < NJ; ++j) if (in && t[j] >= e.x) { off[j] = e.x; j0[j] = e.y; }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) eidx[j] = t[j] < c.total ? j0[j] + (t[j] - off[j]) : 0;
    }
    // one 16-byte record per grid entry, in the grid's own order (k_track_pack): (x, y, angle, octave << 16 | keypoint) -- the entry and
    // its keypoint in ONE load from consecutive addresses instead of an index and three dependent scattered ones
    int k[NJ];
    float kx[NJ], ky[NJ], ang[NJ];
    int oct[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const uint4 e = c.ent[eidx[j]];
        kx[j] = __uint_as_float(e.x); ky[j] = __uint_as_float(e.y); ang[j] = __uint_as_float(e.z);
        oct[j] = (int)(e.w >> 16); k[j] = (int)(e.w & 0xFFFFu);
    }
    bool ok[NJ];
    uint4 lo[NJ], hi[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        ok[j] = t[j] < c.total && !(oct[j] < c.minLevel) && !(oct[j] > c.maxLevel) && (fabsf(kx[j] - c.x) < c.r && fabsf(ky[j] - c.y) < c.r);   // bCheckLevels is true here
        const uint4* tp = (const uint4*)(c.dt + (size_t)(ok[j] ? k[j] : 0) * 32);
        lo[j] = tp[0]; hi[j] = tp[1];
    }
    const unsigned below = (1u << c.l16) - 1u;
    unsigned key[NJ + 1], word[NJ + 1];
    int posj[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const unsigned rowbits = (unsigned)(__ballot(ok[j]) >> (16 * c.wr)) & 0xFFFFu;
        const int pos = cnt + __popc(rowbits & below);
        posj[j] = pos;
        const int d = ham256(a, (u64)lo[j].x | ((u64)lo[j].y << 32), (u64)lo[j].z | ((u64)lo[j].w << 32),
                             (u64)hi[j].x | ((u64)hi[j].y << 32), (u64)hi[j].z | ((u64)hi[j].w << 32));
        float rot = c.qangle - ang[j];
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * c.factor);
        if (bin == 30) bin = 0;
        if (bin < 0 || bin >= 30) bin = TK_NOBIN;
        key[j] = ok[j] ? ((unsigned)d << 16) | (unsigned)pos : INV;          // positions < 65536 (cap)
        word[j] = ((unsigned)d << 21) | ((unsigned)bin << 16) | (unsigned)k[j];
        cnt += __popc(rowbits);
    }
    key[NJ] = INV; word[NJ] = INV;
    if (FB && c.l16 < TK_K) { const uint2 pv = sTop[c.qr][c.l16]; key[NJ] = pv.x; word[NJ] = pv.y; }   // the list so far competes again
    // !FB: at most 16 candidates of a row passed the tests (the rule: 14 grid entries per window, a quarter of them on the right levels
    // and inside the window): they are packed to one per lane -- in visiting order -- and each lane's rank is the number of smaller
    // keys in its row (15 rotations; keys are unique by position).  Otherwise eight row-wide minimum reductions.
    const int nv = cnt - cnt0;
    if (!FB && (NJ == 1 || !__any(nv > 16))) {
        unsigned k1 = key[0], w1 = word[0];
        if (NJ > 1) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) if (key[j] != INV) sK[c.qr][posj[j] - cnt0] = make_uint2(key[j], word[j]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint2 e = sK[c.qr][c.l16];
            k1 = c.l16 < nv ? e.x : INV; w1 = e.y;
        }
        int rank = 0;
        unsigned rk = k1;
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            rk = (unsigned)__builtin_amdgcn_update_dpp((int)rk, (int)rk, 0x121, 0xf, 0xf, false);   // row_ror:1
            rank += rk < k1 ? 1 : 0;
        }
        if (k1 != INV && rank < TK_K) sTop[c.qr][rank] = make_uint2(k1, w1);
    } else {
#pragma unroll
        for (int i = 0; i < TK_K; ++i) {
            unsigned mine = key[0];
#pragma unroll
            for (int j = 1; j <= (FB ? NJ : NJ - 1); ++j) mine = min(mine, key[j]);
            const unsigned m = row16_min_u32(mine);
            if (!__any(m != INV)) break;
            if (mine == m && m != INV) {                                    // keys are unique (position): exactly one lane of the row
                unsigned w = word[0];
#pragma unroll
                for (int j = 1; j <= (FB ? NJ : NJ - 1); ++j) if (key[j] == m) w = word[j];
                sTop[c.qr][i] = make_uint2(m, w);
#pragma unroll
                for (int j = 0; j <= (FB ? NJ : NJ - 1); ++j) if (key[j] == m) key[j] = INV;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
struct Tk16FetchAll {
    template <int NJ, bool FB>
    static __device__ __forceinline__ void run(const Tk16& c, const u64 (&a)[4], int base, int& cnt, const int2 (*sCol)[64], const int (*sAdj)[64], uint2 (*sK)[16], uint2 (*sTop)[TK_K]) {
        tk16_pass_v1<NJ, FB>(c, a, base, cnt, sCol, sAdj, sK, sTop);
    }
};
#endif  /* ORBX_AB */

// k_track_pack: the searched frames' grid entries as 16-byte records in grid order (see tk16_pass)
__global__ __launch_bounds__(256) void k_track_pack(Pool pool, int t_first, uint4* __restrict__ ent) {
    const int pair = blockIdx.y;
    const PoolRow T = pool.row(t_first + pair);
    const int pos = blockIdx.x * 256 + threadIdx.x;
    const int n = min(T.gs[GRID_CELLS], pool.cap);
    if (pos >= n) return;
    const int k = T.gi[pos];
    const KpIn kp = T.kt[k];
    ent[(size_t)pair * pool.cap + pos] = make_uint4(__float_as_uint(kp.x), __float_as_uint(kp.y), __float_as_uint(kp.angle), ((unsigned)kp.octave << 16) | (unsigned)k);
}

// the kernel's body; Pass: how a pass of up to 64 entries per query turns into candidates (Tk16Filter; the A/B build also has Tk16FetchAll)
template <class Pass>
__device__ __forceinline__ void tk16_body(const Pool& pool, const uint4* __restrict__ ent, const TrackArgs& A, const ScaleTab& st, const TopList& out) {
    __shared__ int2 sCol[16][64];                                           // per query: (offset in the flattened list, first grid entry) of each window column
    __shared__ uint2 sTop[16][TK_K];                                        // per query: (distance << 16 | position, output word), ascending
    __shared__ int sAdj[16][64];                                            // per query: grid position - list position of the first 64 window entries
    __shared__ uint2 sK[16][16];                                            // per query: the candidates that passed, one per lane
    const int lane = threadIdx.x & 63, l16 = threadIdx.x & 15, wr = lane >> 4, qr = threadIdx.x >> 4;
    const int pair = blockIdx.y;
    const int qf = A.q_first + pair, cap = pool.cap;
    const int nq = min(pool.counts[qf], cap);
    if ((int)blockIdx.x * 16 >= nq) return;
    const int q = blockIdx.x * 16 + qr;
    const bool live = q < nq;
    const KpIn kq = pool.kps[(size_t)qf * cap + (live ? q : 0)];
    const PoolRow T = pool.row(A.t_first + pair);
    const float x = kq.x + A.dx, y = kq.y + A.dy, r = A.th * st.sf[kq.octave];
    const unsigned INV = 0xFFFFFFFFu;
    const int nMinCellX = max(0, (int)floorf((x - T.min_x - r) * T.inv_w));
    const int nMaxCellX = min(63, (int)ceilf((x - T.min_x + r) * T.inv_w));
    const int nMinCellY = max(0, (int)floorf((y - T.min_y - r) * T.inv_h));
    const int nMaxCellY = min(47, (int)ceilf((y - T.min_y + r) * T.inv_h));
    const bool hit = live && nMinCellX < 64 && nMaxCellX >= 0 && nMinCellY < 48 && nMaxCellY >= 0;
    const int ncols = hit ? nMaxCellX - nMinCellX + 1 : 0;                  // <= 64
    u64 a[4];
    load_desc(pool.desc + ((size_t)qf * cap + (live ? q : 0)) * 32, a);
    if (l16 < TK_K) sTop[qr][l16] = make_uint2(INV, INV);
    int total = 0;
    for (int cb = 0; __any(cb < ncols); cb += 16) {
        const int c = cb + l16;
        int cj0 = 0, clen = 0;
        if (c < ncols) {
            const int ix = nMinCellX + c;
            cj0 = T.gs[ix * 48 + nMinCellY];
            clen = T.gs[ix * 48 + nMaxCellY + 1] - cj0;
        }
        int sc = clen;                                                      // inclusive prefix sum inside the 16-lane row
        sc += __builtin_amdgcn_update_dpp(0, sc, 0x111, 0xf, 0xf, true);
        sc += __builtin_amdgcn_update_dpp(0, sc, 0x112, 0xf, 0xf, true);
        sc += __builtin_amdgcn_update_dpp(0, sc, 0x114, 0xf, 0xf, true);
        sc += __builtin_amdgcn_update_dpp(0, sc, 0x118, 0xf, 0xf, true);
        const int excl = total + sc - clen;
        if (c < ncols) sCol[qr][c] = make_int2(excl, cj0);
        for (int e = 0; __any(e < clen && excl + e < 64); ++e)              // (a cell column of a window holds one or two entries as a rule)
            if (e < clen && excl + e < 64) sAdj[qr][excl + e] = cj0 - excl;
        const int s0 = __builtin_amdgcn_readlane(sc, 15), s1 = __builtin_amdgcn_readlane(sc, 31),
                  s2 = __builtin_amdgcn_readlane(sc, 47), s3 = __builtin_amdgcn_readlane(sc, 63);
        total += wr == 0 ? s0 : wr == 1 ? s1 : wr == 2 ? s2 : s3;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                  // a row lives inside one wave: LDS traffic of the same wave is ordered
    __builtin_amdgcn_wave_barrier();
    Tk16 c;
    c.ent = ent + (size_t)pair * cap; c.dt = T.dt; c.cap = cap;
    c.x = x; c.y = y; c.r = r; c.qangle = kq.angle; c.factor = A.factor; c.minLevel = kq.octave - 1; c.maxLevel = kq.octave + 1;
    c.total = total; c.ncols = ncols; c.qr = qr; c.l16 = l16; c.wr = wr;
    const int maxTotal = max(max(__builtin_amdgcn_readlane(total, 0), __builtin_amdgcn_readlane(total, 16)),
                             max(__builtin_amdgcn_readlane(total, 32), __builtin_amdgcn_readlane(total, 48)));
    int cnt = 0;
    for (int base = 0; base < maxTotal; base += 64) {
        const int nj = min(4, (maxTotal - base + 15) >> 4);                 // wave-uniform
        if (base == 0) {
            if (nj == 1) Pass::template run<1, false>(c, a, base, cnt, sCol, sAdj, sK, sTop);
            else if (nj == 2) Pass::template run<2, false>(c, a, base, cnt, sCol, sAdj, sK, sTop);
            else if (nj == 3) Pass::template run<3, false>(c, a, base, cnt, sCol, sAdj, sK, sTop);
            else Pass::template run<4, false>(c, a, base, cnt, sCol, sAdj, sK, sTop);
        } else {
            if (nj <= 2) Pass::template run<2, true>(c, a, base, cnt, sCol, sAdj, sK, sTop);
            else Pass::template run<4, true>(c, a, base, cnt, sCol, sAdj, sK, sTop);
        }
    }
    if (live) {
        const size_t o = (size_t)pair * cap + q;
        if (l16 == 0) out.cnt[o] = cnt;
        if (l16 < TK_K) { const uint2 e = sTop[qr][l16]; out.keys[o * TK_K + l16] = e.x == INV ? INV : e.y; }
    }
}

// (the kernels keep the loose parameters their generated code was tuned with; the body takes the views)
#define TK16_PARAMS const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ counts, int cap,                 \
                    const int* __restrict__ grid_start, const uint4* __restrict__ ent, float min_x, float min_y, float inv_w, float inv_h,    \
                    int q_first, int t_first, float th, ScaleTab st, float dx, float dy, float factor, int* __restrict__ out_cnt,             \
                    unsigned int* __restrict__ out_keys
#define TK16_BODY(Pass) tk16_body<Pass>(Pool{kps, desc, counts, cap, grid_start, nullptr, min_x, min_y, inv_w, inv_h}, ent,                 \
                                        TrackArgs{q_first, t_first, th, dx, dy, factor}, st, TopList{out_cnt, out_keys, nullptr})
__global__ __launch_bounds__(256) void k_track_topk16(TK16_PARAMS) { TK16_BODY(Tk16Filter); }
#ifdef ORBX_AB   /* A/B reference, not in the product library */
__global__ __launch_bounds__(256) void k_track_topk16_v1(TK16_PARAMS) { TK16_BODY(Tk16FetchAll); }
#endif
#undef TK16_PARAMS
#undef TK16_BODY

#ifdef ORBX_AB   /* A/B reference (eight queries per step), not in the product library */
__global__ __launch_bounds__(64) void k_track_claim(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ counts, int cap,
                                                    const int* __restrict__ grid_start, const int* __restrict__ grid_idx,
                                                    float min_x, float min_y, float inv_w, float inv_h, int q_first, int t_first, float th, ScaleTab st, float dx, float dy, float factor,
                                                    const int* __restrict__ topCnt, const unsigned int* __restrict__ topKeys,
                                                    const uint8_t* __restrict__ t_blocked, const uint8_t* __restrict__ q_obs, int check_ori,
                                                    unsigned int* __restrict__ accepted, int* __restrict__ match, int* __restrict__ nmatches) {
    extern __shared__ unsigned int tk_lds[];                                // blocked bit array [ceil(cap / 32)], hist[32], "query has observations" bits [ceil(cap / 32)]
    const int lane = threadIdx.x, pair = blockIdx.x;
    const Pool pool{kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h};
    const TrackArgs A{q_first, t_first, th, dx, dy, factor};
    const int qf = q_first + pair, tf = t_first + pair;
    const int nq = min(pool.counts[qf], cap), nt = min(pool.counts[tf], cap);
    const int nwords = (cap + 31) >> 5;
    unsigned int* blk = tk_lds;
    unsigned int* hist = tk_lds + nwords;
    unsigned int* obsb = hist + 32;
    int* mrow = match + (size_t)pair * cap;
    unsigned int* acc = accepted + (size_t)pair * cap;
    const uint8_t* tb = t_blocked ? t_blocked + (size_t)tf * cap : nullptr;
    const uint8_t* qo = q_obs ? q_obs + (size_t)qf * cap : nullptr;
    for (int w = lane; w < nwords; w += 64) { blk[w] = bits_word(tb, nt, w, 0u); obsb[w] = bits_word(qo, nq, w, 0xFFFFFFFFu); }
    if (lane < 32) hist[lane] = 0;
    for (int k = lane; k < cap; k += 64) mrow[k] = -1;                        // ORBM_NO_MATCH
    __syncthreads();
    const size_t rowBase = (size_t)pair * cap;
    const int sub = lane >> 3;                                              // the lane's query inside a group of eight
    int nm = 0, nacc = 0;
    // Two register sets of four groups (32 queries) each: set A is resolved while set B's lists are in flight (a list comes from another
    // XCD's writes, i.e. from memory: ~1.6 us per round trip, against ~0.3 us to resolve a group).  The loaded values are touched only
    // when their set becomes current -- a move or a select behind the load would make the wave wait for it there -- and the loads are
    // UNCONDITIONAL (clamped index): a load under a branch turns every later s_waitcnt into a full drain.
    const int qLast = max(nq - 1, 0);
    unsigned int ak0, ak1, ak2, ak3;
    int ac0, ac1, ac2, ac3;
    auto fetch = [&](int qi, unsigned int& k_, int& c_) {
        const int qc = min(qi, qLast);
        k_ = topKeys[(rowBase + qc) * TK_K + (lane & 7)];
        c_ = topCnt[rowBase + qc];
    };
    fetch(sub, ak0, ac0); fetch(8 + sub, ak1, ac1); fetch(16 + sub, ak2, ac2); fetch(24 + sub, ak3, ac3);
    for (int G = 0; G < nq; G += 32) {
      unsigned int bk0, bk1, bk2, bk3;
      int bc0, bc1, bc2, bc3;
      fetch(G + 32 + sub, bk0, bc0); fetch(G + 40 + sub, bk1, bc1); fetch(G + 48 + sub, bk2, bc2); fetch(G + 56 + sub, bk3, bc3);
#pragma clang loop unroll(disable)
      for (int s4 = 0; s4 < 4; ++s4) {
        const int g0 = G + 8 * s4;
        if (g0 >= nq) break;
        const bool ql = g0 + sub < nq;
        const unsigned int kraw = s4 == 0 ? ak0 : s4 == 1 ? ak1 : s4 == 2 ? ak2 : ak3;
        const int craw = s4 == 0 ? ac0 : s4 == 1 ? ac1 : s4 == 2 ? ac2 : ac3;
        const unsigned int key = ql ? kraw : 0xFFFFFFFFu;
        const int cnt = ql ? craw : 0;
        const int qme = min(g0 + sub, qLast);
        const unsigned ob = (obsb[qme >> 5] >> (qme & 31)) & 1u;               // != 0: the lane's query has observations (:2565: only those block a slot)
        const unsigned long long obsMask = __ballot(ob != 0);
        const bool valid = key != 0xFFFFFFFFu;
        const unsigned int myk = key & 0xFFFFu;
        bool blocked = valid && ((blk[myk >> 5] >> (myk & 31)) & 1u);       // as of the start of the group; claims inside it: below
        const int gend = min(8, nq - g0);
        {   // all eight queries at once: each takes the first of its listed candidates that was free when the group started.  That IS the
            // sequential outcome unless two accepted queries of the group want the same slot (the later one must then see the claim, or
            // overwrite it) or a query has run out of listed candidates with more in its window -- such a group is replayed one by one.
            const unsigned long long fr = __ballot(valid && !blocked);
            const unsigned m8 = (unsigned)(fr >> (8 * sub)) & 0xFFu;
            const unsigned pick = (unsigned)__shfl((int)key, (sub << 3) + (m8 ? __ffs((int)m8) - 1 : 0));
            const bool qlive = g0 + sub < nq;
            const bool take = qlive && m8 != 0 && (pick >> 21) <= 100u;    // TH_HIGH (:2589)
            const unsigned pk = pick & 0xFFFFu;
            bool clash = qlive && m8 == 0 && cnt > TK_K;
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                const unsigned ke = (unsigned)__builtin_amdgcn_readlane((int)pk, 8 * e);
                const int te = __builtin_amdgcn_readlane((int)take, 8 * e);
                if (te && take && sub > e && ke == pk) clash = true;
            }
            if (!__any(clash)) {
                const bool lead = (lane & 7) == 0 && take;
                const unsigned bin = (pick >> 16) & 31u;
                const bool withBin = lead && check_ori && bin != TK_NOBIN;
                const unsigned long long tb = __ballot(lead), bb = __ballot(withBin);
                if (lead) {
                    mrow[pk] = g0 + sub;
                    if (ob != 0) atomicOr(&blk[pk >> 5], 1u << (pk & 31));
                }
                if (withBin) {
                    acc[nacc + __popcll(bb & ((1ull << lane) - 1ull))] = pk | (bin << 16);
                    atomicAdd(&hist[bin], 1u);
                }
                nm += __popcll(tb);
                nacc += __popcll(bb);
                continue;
            }
        }
        for (int s = 0; s < gend; ++s) {
            const int qi = g0 + s;
            const unsigned long long sel = 0xFFull << (8 * s);
            const unsigned long long bal = __ballot(valid && !blocked) & sel;
            unsigned int best = 0xFFFFFFFFu;
            if (bal) best = (unsigned int)__builtin_amdgcn_readlane((int)key, __ffsll((long long)bal) - 1);   // (wave-uniform lane: no LDS crossbar round trip)
            else {
                const int c = __builtin_amdgcn_readlane(cnt, 8 * s);
                if (c > TK_K) {                                             // the list ran dry, the window holds more: rescan it, blocked set applied
                    const KpIn kq = pool.kps[(size_t)qf * cap + qi];                // the window k_track_topk16 swept
                    const Win w = {kq.x + A.dx, kq.y + A.dy, A.th * st.sf[kq.octave], 0.f, kq.octave - 1, kq.octave + 1};
                    u64 a[4], top[TK_K];
                    load_desc(pool.desc + ((size_t)qf * cap + qi) * 32, a);
                    int c2;
                    win_sweep<false>(w, RotBinPay{kq.angle, A.factor}, pool.row(tf), nullptr, a, blk, lane, c2, top);
                    best = cand_word(top[0]);
                }
            }
            if (best == 0xFFFFFFFFu) continue;
            const int d = (int)(best >> 21);
            if (d > 100) continue;                                          // TH_HIGH (:2589)
            const unsigned int k = best & 0xFFFFu, bin = (best >> 16) & 31u;
            const bool obs = (obsMask >> (8 * s)) & 1ull;
            if (obs && valid && myk == k) blocked = true;                  // later queries of this group see the claim
            if (lane == 0) {
                // LDS updates as returnless atomics: nothing in the chain of the next query waits for them
                mrow[k] = qi;
                if (obs) atomicOr(&blk[k >> 5], 1u << (k & 31));
                if (check_ori && bin != TK_NOBIN) { acc[nacc] = k | (bin << 16); atomicAdd(&hist[bin], 1u); }
            }
            ++nm;
            if (check_ori && bin != TK_NOBIN) ++nacc;
        }
      }
      ak0 = bk0; ak1 = bk1; ak2 = bk2; ak3 = bk3; ac0 = bc0; ac1 = bc1; ac2 = bc2; ac3 = bc3;
    }
    __syncthreads();
    if (check_ori) nm -= rot_cull(hist, acc, nacc, mrow, lane);
    if (lane == 0) nmatches[pair] = nm;
}

#endif  /* ORBX_AB */

__global__ __launch_bounds__(64) void k_track_claim64(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ counts, int cap,
                                                    const int* __restrict__ grid_start, const int* __restrict__ grid_idx,
                                                    float min_x, float min_y, float inv_w, float inv_h, int q_first, int t_first, float th, ScaleTab st, float dx, float dy, float factor,
                                                    const int* __restrict__ topCnt, const unsigned int* __restrict__ topKeys,
                                                    const uint8_t* __restrict__ t_blocked, const uint8_t* __restrict__ q_obs, int check_ori,
                                                    unsigned int* __restrict__ accepted, int* __restrict__ match, int* __restrict__ nmatches) {
    extern __shared__ unsigned int tk_lds[];                                // blocked bit array [ceil(cap / 32)], hist[32], "query has observations" bits [ceil(cap / 32)]
    const int lane = threadIdx.x, pair = blockIdx.x;
    const Pool pool{kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h};
    const TrackArgs A{q_first, t_first, th, dx, dy, factor};
    const int qf = q_first + pair, tf = t_first + pair;
    const int nq = min(pool.counts[qf], cap), nt = min(pool.counts[tf], cap);
    const int nwords = (cap + 31) >> 5;
    unsigned int* blk = tk_lds;
    unsigned int* hist = tk_lds + nwords;
    unsigned int* obsb = hist + 32;
    unsigned int* tag = obsb + nwords;                                      // [cap]: per slot the latest proposal (round << 6 | 63 - lane), see below
    int* mrow = match + (size_t)pair * cap;
    unsigned int* acc = accepted + (size_t)pair * cap;
    const uint8_t* tb = t_blocked ? t_blocked + (size_t)tf * cap : nullptr;
    const uint8_t* qo = q_obs ? q_obs + (size_t)qf * cap : nullptr;
    for (int w = lane; w < nwords; w += 64) { blk[w] = bits_word(tb, nt, w, 0u); obsb[w] = bits_word(qo, nq, w, 0xFFFFFFFFu); }
    if (lane < 32) hist[lane] = 0;
    for (int k = lane; k < cap; k += 64) { mrow[k] = -1; tag[k] = 0; }       // ORBM_NO_MATCH
    __syncthreads();
    const size_t rowBase = (size_t)pair * cap;
    int nm = 0, nacc = 0;
    // SIXTY-FOUR queries per step, one per lane with its eight listed candidates in registers.  Every lane proposes its first candidate
    // that is free right now; per slot the lowest lane wins (LDS atomicMax of round << 6 | 63 - lane, then a read-back).  The queries
    // below the first loser f take their proposals at once -- none of them wanted a slot a lower query took, and everything listed before
    // a proposal was blocked already, so this IS what the one-by-one replay (:2555-2593) does for them -- query f is resolved alone with
    // those claims applied (its proposal is gone, or its list ran dry with more in the window: win_sweep), and the rest of the 64 propose
    // again.  Lists come from another XCD's writes, i.e. from memory: the next 64 queries' loads are in flight while these are resolved;
    // the loaded values are touched only when their window becomes current, and the loads are unconditional (clamped index).
    const int qLast = max(nq - 1, 0);
    uint4 alo, ahi, blo, bhi;
    int ac, bc;
    auto fetch = [&](int qi, uint4& lo_, uint4& hi_, int& c_) {
        const int qc = min(qi, qLast);
        const uint4* kp = (const uint4*)(topKeys + (rowBase + qc) * TK_K);
        lo_ = kp[0]; hi_ = kp[1];
        c_ = topCnt[rowBase + qc];
    };
    fetch(lane, alo, ahi, ac);
    unsigned int round = 1;
    for (int W0 = 0; W0 < nq; W0 += 64) {
        fetch(W0 + 64 + lane, blo, bhi, bc);
        const int q = W0 + lane;
        const bool ql = q < nq;
        unsigned int key[TK_K] = {alo.x, alo.y, alo.z, alo.w, ahi.x, ahi.y, ahi.z, ahi.w};
#pragma unroll
        for (int i = 0; i < TK_K; ++i) if (!ql) key[i] = 0xFFFFFFFFu;
        const int cnt = ql ? ac : 0;
        const int qme = min(q, qLast);
        const bool ob = (obsb[qme >> 5] >> (qme & 31)) & 1u;                // the lane's query has observations (:2565: only those block a slot)
        int start = 0;
        while (start < 64 && W0 + start < nq) {
            unsigned int pick = 0xFFFFFFFFu;
#pragma unroll
            for (int i = TK_K - 1; i >= 0; --i) {
                const unsigned int k = key[i] & 0xFFFFu;
                const bool fr = key[i] != 0xFFFFFFFFu && !((blk[k >> 5] >> (k & 31)) & 1u);
                pick = fr ? key[i] : pick;
            }
            const bool active = ql && lane >= start;
            const bool take = active && pick != 0xFFFFFFFFu && (pick >> 21) <= 100u;   // TH_HIGH (:2589)
            const bool resc = active && pick == 0xFFFFFFFFu && cnt > TK_K;
            const unsigned int pk = pick & 0xFFFFu;
            const unsigned int tv = (round << 6) | (unsigned)(63 - lane);
            if (take) atomicMax(&tag[pk], tv);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const bool lose = take && tag[pk] != tv;
            const unsigned long long bad = __ballot(lose || resc);
            const int f = bad ? __ffsll((long long)bad) - 1 : 64;          // >= start
            {
                const bool com = take && lane < f;
                const unsigned bin = (pick >> 16) & 31u;
                const bool withBin = com && check_ori && bin != TK_NOBIN;
                const unsigned long long tb = __ballot(com), bb = __ballot(withBin);
                if (com) {
                    mrow[pk] = q;
                    if (ob) atomicOr(&blk[pk >> 5], 1u << (pk & 31));
                }
                if (withBin) {
                    acc[nacc + __popcll(bb & ((1ull << lane) - 1ull))] = pk | (bin << 16);
                    atomicAdd(&hist[bin], 1u);
                }
                nm += __popcll(tb);
                nacc += __popcll(bb);
            }
            if (f < 64) {
                // query W0 + f alone (wave-uniform), the claims above applied
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int qi = W0 + f;
                unsigned int best = 0xFFFFFFFFu;
#pragma unroll
                for (int i = TK_K - 1; i >= 0; --i) {
                    const unsigned int ki = (unsigned int)__builtin_amdgcn_readlane((int)key[i], f);
                    const unsigned int k = ki & 0xFFFFu;
                    const bool fr = ki != 0xFFFFFFFFu && !((blk[k >> 5] >> (k & 31)) & 1u);
                    best = fr ? ki : best;
                }
                if (best == 0xFFFFFFFFu && __builtin_amdgcn_readlane(cnt, f) > TK_K) {   // the list ran dry, the window holds more: rescan it, blocked set applied
                    const KpIn kq = pool.kps[(size_t)qf * cap + qi];                // the window k_track_topk16 swept
                    const Win w = {kq.x + A.dx, kq.y + A.dy, A.th * st.sf[kq.octave], 0.f, kq.octave - 1, kq.octave + 1};
                    u64 a[4], top[TK_K];
                    load_desc(pool.desc + ((size_t)qf * cap + qi) * 32, a);
                    int c2;
                    win_sweep<false>(w, RotBinPay{kq.angle, A.factor}, pool.row(tf), nullptr, a, blk, lane, c2, top);
                    best = cand_word(top[0]);
                }
                if (best != 0xFFFFFFFFu && (best >> 21) <= 100u) {
                    const unsigned int k = best & 0xFFFFu, bin = (best >> 16) & 31u;
                    const bool obs = (obsb[qi >> 5] >> (qi & 31)) & 1u;
                    if (lane == 0) {
                        mrow[k] = qi;
                        if (obs) atomicOr(&blk[k >> 5], 1u << (k & 31));
                        if (check_ori && bin != TK_NOBIN) { acc[nacc] = k | (bin << 16); atomicAdd(&hist[bin], 1u); }
                    }
                    ++nm;
                    if (check_ori && bin != TK_NOBIN) ++nacc;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            start = f + 1;
            ++round;
        }
        alo = blo; ahi = bhi; ac = bc;
    }
    __syncthreads();
    if (check_ori) nm -= rot_cull(hist, acc, nacc, mrow, lane);
    if (lane == 0) nmatches[pair] = nm;
}

// ------------------------------------------------------------------------------------------------
// Batched SearchByProjection(Frame, local MapPoints) -- M3, the left-camera part of ORBmatcher.cc:45-166 -- final matches on the device.
// The queries are a tracker's local map points as k_frustum left them: one row of q_stride entries per searched frame of an extractor
// result block.  Per query the window is derived on the device (RadiusByViewingCos [* th] * scale[level], levels [level-1, level],
// the mvuRight gate, :66-117); a query that is not in view, lies beyond th_far (bFarPoints) or has a level outside the table reads
// nothing else of its row (k_frustum leaves those fields unwritten for rejected points).
// k_lp_topk: wave per query, one win_sweep: a window of up to 64 grid entries costs one pass whatever its column count and larger
//   ones (th = 10, high levels: r up to 4 * th * scale) take more passes of 64.  Out: the window population and its TK_K best
//   candidates in (distance, visiting order) rank, each as ONE word dist << 21 | (octave + 1) << 16 | keypoint (the replay reads the
//   level of best and second from it; no second gather).
// k_lp_claim: one wave per frame replays the claims in query order (:119-164).  A query's list sits in LDS, one candidate per lane;
//   one ballot over the blocked bit array gives its first two unblocked candidates -- best and second, as `dist < bestDist` /
//   `else if dist < bestDist2` would have met them.  A truncated list with fewer than two unblocked entries is rescanned in full,
//   blocked set applied (win_sweep<false>).
// ------------------------------------------------------------------------------------------------
struct LpRows {                                            // the per-query arrays of one call, [nframes][q_stride] unless q_shared
    const int* nq; int q_stride;
    const uint8_t* in_view; const float* px; const float* py; const float* pxr; const float* view_cos; const int* level;
    const float* depth; float th_far;
    const uint8_t* qdesc; const uint8_t* mp_obs; int q_shared;
    float th; int nlevels;
};

// the window of query row o (wave-uniform), or false: the query is skipped
__device__ __forceinline__ bool lp_query(const LpRows& R, const float* sf, bool stereo, size_t o, Win& w) {
    if (!R.in_view[o]) return false;
    if (R.depth && R.depth[o] > R.th_far) return false;                      // bFarPoints (:57-58)
    const int lvl = R.level[o];
    if (lvl < 0 || lvl >= R.nlevels) return false;
    float r = (double)R.view_cos[o] > 0.998 ? 2.5f : 4.0f;                   // RadiusByViewingCos (:242-249): float against a double literal
    if (R.th != 1.0f) r *= R.th;
    w.r = r * sf[lvl];                                                     // one float multiply, as GetFeaturesInArea's argument
    w.x = R.px[o]; w.y = R.py[o]; w.minLevel = lvl - 1; w.maxLevel = lvl;
    w.ur = stereo ? R.pxr[o] : 0.f;
    return true;
}

__global__ __launch_bounds__(256) void k_lp_topk(Pool pool, int t_first, const float* __restrict__ uright, LpRows R, ScaleTab st, TopList out) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.y, tf = t_first + f;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nq = min(max(R.nq[f], 0), R.q_stride);
    if (q >= nq) return;
    const size_t o = (size_t)f * R.q_stride + q;
    Win w;
    int cnt = 0;
    u64 top[TK_K];
    if (lp_query(R, st.sf, uright != nullptr, o, w)) {
        u64 a[4];
        load_desc(R.qdesc + (R.q_shared ? (size_t)q : o) * 32, a);
        win_sweep<true>(w, OctavePay{}, pool.row(tf), uright ? uright + (size_t)f * pool.cap : nullptr, a, nullptr, lane, cnt, top);
    } else {
#pragma unroll
        for (int i = 0; i < TK_K; ++i) top[i] = ~0ull;
    }
    if (lane == 0) put_topk(out, o, cnt, w.r, top);    // (the radius is read back only by a rescan: count > TK_K)
}

__global__ __launch_bounds__(64) void k_lp_claim(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ counts, int cap,
                                                 const int* __restrict__ grid_start, const int* __restrict__ grid_idx,
                                                 float min_x, float min_y, float inv_w, float inv_h, int t_first, const float* __restrict__ uright, const uint8_t* __restrict__ t_blocked,
                                                 LpRows R, float nnratio, TopList L, int* __restrict__ match, int* __restrict__ nmatches) {
    extern __shared__ unsigned int lp_lds[];                                 // blocked bit array [ceil(cap / 32)], the current 64 queries' lists [64][TK_K]
    const unsigned INV = 0xFFFFFFFFu;
    const Pool pool{kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h};
    const int lane = threadIdx.x, f = blockIdx.x, tf = t_first + f;
    const int nt = min(max(pool.counts[tf], 0), cap);
    const int nq = min(max(R.nq[f], 0), R.q_stride);
    const int nwords = (cap + 31) >> 5;
    unsigned int* blk = lp_lds;
    unsigned int* sk = lp_lds + nwords;
    int* mrow = match + (size_t)f * cap;
    for (int wd = lane; wd < nwords; wd += 64) blk[wd] = bits_word(t_blocked ? t_blocked + (size_t)f * cap : nullptr, nt, wd, 0u);
    for (int k = lane; k < cap; k += 64) mrow[k] = -1;                      // ORBM_NO_MATCH
    __syncthreads();
    const PoolRow T = pool.row(tf);
    const float* urt = uright ? uright + (size_t)f * cap : nullptr;
    const size_t rowBase = (size_t)f * R.q_stride;
    int nm = 0;
    // the next 64 queries' lists, counts and observation flags are in flight while the current ones are replayed (clamped, unconditional loads)
    unsigned int pk[TK_K];
    int pc = 0;
    uint8_t pob = 0;
    auto fetch = [&](int W0) {
        const int last = nq * TK_K - 1;
#pragma unroll
        for (int r = 0; r < TK_K; ++r) pk[r] = L.keys[rowBase * TK_K + min(W0 * TK_K + r * 64 + lane, last)];
        const int qc = min(W0 + lane, nq - 1);
        pc = L.cnt[rowBase + qc];
        pob = R.mp_obs[R.q_shared ? (size_t)qc : rowBase + qc];
    };
    if (nq > 0) fetch(0);
    for (int W0 = 0; W0 < nq; W0 += 64) {
#pragma unroll
        for (int r = 0; r < TK_K; ++r) sk[r * 64 + lane] = pk[r];             // query i's list: sk[i * TK_K .. + TK_K)
        const int cnt = W0 + lane < nq ? pc : 0;
        const int ob = pob != 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (W0 + 64 < nq) fetch(W0 + 64);
        unsigned long long todo = __ballot(cnt > 0);                        // skipped queries and empty windows have count 0
        while (todo) {
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            unsigned int key = INV;
            bool fr = false;
            if (lane < TK_K) {
                key = sk[i * TK_K + lane];
                const unsigned int k = key == INV ? 0u : key & 0xFFFFu;
                fr = key != INV && !((blk[k >> 5] >> (k & 31)) & 1u);
            }
            unsigned long long fb = __ballot(fr);
            unsigned int w1 = INV, w2 = INV;
            if (fb) {
                w1 = (unsigned)__builtin_amdgcn_readlane((int)key, __ffsll((long long)fb) - 1);
                fb &= fb - 1;
                if (fb) w2 = (unsigned)__builtin_amdgcn_readlane((int)key, __ffsll((long long)fb) - 1);
            }
            if (w2 == INV && __builtin_amdgcn_readlane(cnt, i) > TK_K) {
                // best AND second must come from the unblocked candidates: the listed ones ran dry, the window holds more
                const size_t o = rowBase + W0 + i;
                const Win w = {R.px[o], R.py[o], L.r[o], uright ? R.pxr[o] : 0.f, R.level[o] - 1, R.level[o]};   // the window k_lp_topk swept
                u64 a[4], top[TK_K];                                         // (its radius from there: no scale table here)
                load_desc(R.qdesc + (R.q_shared ? (size_t)(W0 + i) : o) * 32, a);
                int c2;
                win_sweep<false>(w, OctavePay{}, T, urt, a, blk, lane, c2, top);
                w1 = cand_word(top[0]); w2 = cand_word(top[1]);
            }
            if (w1 == INV) continue;
            const int bestDist = (int)(w1 >> 21), bestLevel = (int)((w1 >> 16) & 31u) - 1;
            const int bestDist2 = w2 == INV ? 256 : (int)(w2 >> 21), bestLevel2 = w2 == INV ? -1 : (int)((w2 >> 16) & 31u) - 1;
            if (bestDist <= 100) {                                           // TH_HIGH (:119)
                if (bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2) continue;
                if (bestLevel != bestLevel2 || (float)bestDist <= nnratio * (float)bestDist2) {
                    const unsigned int k = w1 & 0xFFFFu;
                    const int obi = __builtin_amdgcn_readlane(ob, i);
                    if (lane == 0) {
                        mrow[k] = W0 + i;                                    // may overwrite a claim of a query without observations
                        if (obi) blk[k >> 5] |= 1u << (k & 31);
                    }
                    ++nm;                                                    // overwrites count, as the reference's nmatches++ does
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");              // the next chunk's lists overwrite sk
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) nmatches[f] = nm;
}

// ------------------------------------------------------------------------------------------------
// Batched SearchByProjection(Frame, Frame) on the caller's projections -- M4, Tracking::TrackWithMotionModel -- final matches on the
// device: ORBmatcher.cc:2469-2612 (the left-camera part, Nleft == -1) with the rotation check :2686-2708, and Tracking's wider-window
// retry (Tracking.cc:3213-3221).  The queries are the LastFrame MapPoints as k_mm_project (or the caller) left them: one row of
// q_stride entries per pair.  Per query the window is th * scale[octave], levels by the pair's direction (:2543-2549: o-1..o+1,
// bForward o.., bBackward 0..o, GetFeaturesInArea's bCheckLevels rule, Frame.cc:784-871) and the mvuRight gate (:2569-2576: ur =
// u - mbf * invzc, a multiply then a subtract: this file is compiled without contraction).  A query that is not valid or whose
// octave lies outside the scale table reads nothing else of its row.
// k_mm_topk: ONE WAVE PER QUERY.  Mono windows at th 15 hold about 14 grid entries, so one pass leaves most lanes idle; but a query
//   costs four dependent round trips (cell ranges, grid indices, keypoints, descriptors) whatever its lane count, 64 pairs x 1000
//   queries are 64 k waves -- enough to fill the machine by waves rather than by lanes --, and the windows the same call must also
//   take (th 30 on level 7: 30 * 1.2^7 = 107 px, a few hundred entries; the retry doubles th again) then need a few passes of 64
//   instead of many passes of 16 with the per-pass merge each time: one win_sweep, as in k_lp_topk.  Out: the window population and
//   its TK_K best candidates in (distance, visiting order) rank as ONE word each, dist << 21 | rotation bin << 16 | keypoint (bin of
//   angle_q - angle_t as :2596-2603, TK_NOBIN outside [0, 30)), so the claim needs no second gather.
// k_mm_claim: one wave per pair replays the claims in query order (:2553-2612).  A query's list sits in LDS, one candidate per lane;
//   one ballot over the blocked bit array gives its first unblocked candidate, which is its `dist < bestDist` winner.  A truncated
//   list whose candidates are all blocked is rescanned in full with the blocked set applied (win_sweep<false>).  Each assignment with
//   a rotation bin is appended to a per-pair list and counted in an LDS histogram; the three-maxima cull then marks every slot of a
//   culled bin ORBM_MATCH_PRUNED once per entry, so a slot claimed twice is culled (and uncounted) as often as the reference does.
// RETRY: the same two kernels at 2 * th for the pairs whose count is below retry_below, from an empty frame (mvpMapPoints filled
//   with NULL: no blocked slots); every other pair returns at once, so the retry needs no host round trip.
// ------------------------------------------------------------------------------------------------
struct MmRows {                                            // the per-query arrays of one call, [npairs][q_stride]
    const int* nq; int q_stride;
    const uint8_t* valid; const float* u; const float* v; const float* invzc; const int* octave; const float* angle;
    const uint8_t* qdesc; const uint8_t* mp_obs; const uint8_t* dir;
    float mbf, factor; int nlevels, retry_below, check_ori;
};

// the window of valid query row o of pair p with octave oc, all but its radius
__device__ __forceinline__ void mm_levels(const MmRows& R, int p, int oc, size_t o, bool stereo, Win& w) {
    const int d = R.dir ? R.dir[p] : 0;
    if (d == 1) { w.minLevel = oc; w.maxLevel = -1; }                        // bForward: GetFeaturesInArea(.., nLastOctave)
    else if (d == 2) { w.minLevel = 0; w.maxLevel = oc; }                    // bBackward
    else { w.minLevel = oc - 1; w.maxLevel = oc + 1; }
    w.x = R.u[o]; w.y = R.v[o];
    w.ur = stereo ? R.u[o] - R.mbf * R.invzc[o] : 0.f;                       // :2571
}

// the window of query row o of pair p (wave-uniform), or false: the query is skipped
__device__ __forceinline__ bool mm_query(const MmRows& R, const float* sf, float th, bool stereo, int p, size_t o, Win& w) {
    if (!R.valid[o]) return false;
    const int oc = R.octave[o];
    if (oc < 0 || oc >= R.nlevels) return false;
    w.r = th * sf[oc];                                                       // :2536, one float multiply
    mm_levels(R, p, oc, o, stereo, w);
    return true;
}

template <bool RETRY>
__global__ __launch_bounds__(256) void k_mm_topk(Pool pool, int t_first, const float* __restrict__ uright, MmRows R, ScaleTab st, float th,
                                                 const int* __restrict__ nmatches, TopList out) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.y, tf = t_first + p;
    if (RETRY && !(nmatches[p] < R.retry_below)) return;                    // the first search of this pair stands
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nq = min(max(R.nq[p], 0), R.q_stride);
    if (q >= nq) return;
    const size_t o = (size_t)p * R.q_stride + q;
    Win w;
    w.r = 0.f;                                                               // (a skipped query's out_r is written but never read)
    int cnt = 0;
    u64 top[TK_K];
    if (mm_query(R, st.sf, th, uright != nullptr, p, o, w)) {
        u64 a[4];
        load_desc(R.qdesc + o * 32, a);
        win_sweep<true>(w, RotBinPay{R.angle[o], R.factor}, pool.row(tf), uright ? uright + (size_t)p * pool.cap : nullptr, a, nullptr, lane, cnt, top);
    } else {
#pragma unroll
        for (int i = 0; i < TK_K; ++i) top[i] = ~0ull;
    }
    if (lane == 0) put_topk(out, o, cnt, w.r, top);    // (the radius is read back only by a rescan: count > TK_K)
}

template <bool RETRY>
__global__ __launch_bounds__(64) void k_mm_claim(Pool pool, int t_first, const float* __restrict__ uright, const uint8_t* __restrict__ t_blocked,
                                                 MmRows R, TopList L, unsigned int* __restrict__ accepted,
                                                 int* __restrict__ match, int* __restrict__ nmatches, uint8_t* __restrict__ retried) {
    extern __shared__ unsigned int mm_lds[];                                 // blocked bits [ceil(cap / 32)], hist[32], the current 64 queries' lists [64][TK_K]
    const unsigned INV = 0xFFFFFFFFu;
    const int lane = threadIdx.x, p = blockIdx.x, tf = t_first + p, cap = pool.cap;
    if (RETRY && !(nmatches[p] < R.retry_below)) return;                    // (wave-uniform) the first search of this pair stands
    const int nt = min(max(pool.counts[tf], 0), cap);
    const int nq = min(max(R.nq[p], 0), R.q_stride);
    const int nwords = (cap + 31) >> 5;
    unsigned int* blk = mm_lds;
    unsigned int* hist = mm_lds + nwords;
    unsigned int* sk = hist + 32;
    int* mrow = match + (size_t)p * cap;
    const uint8_t* tb = !RETRY && t_blocked ? t_blocked + (size_t)p * cap : nullptr;   // the retry starts from an empty frame (Tracking.cc:3217)
    for (int wd = lane; wd < nwords; wd += 64) blk[wd] = bits_word(tb, nt, wd, 0u);
    if (lane < 32) hist[lane] = 0;
    for (int k = lane; k < cap; k += 64) mrow[k] = -1;                      // ORBM_NO_MATCH
    __syncthreads();
    const PoolRow T = pool.row(tf);
    const float* urt = uright ? uright + (size_t)p * cap : nullptr;
    const size_t rowBase = (size_t)p * R.q_stride;
    unsigned int* acc = accepted + rowBase;                                  // (slot | bin << 16) of every assignment with a bin, in order
    int nm = 0, nacc = 0;
    // the next 64 queries' lists and counts are in flight while the current ones are replayed (clamped, unconditional loads);
    // mp_obs is read only for a query with candidates (a skipped row reads nothing else)
    const unsigned int* keyRow = L.keys + rowBase * TK_K;
    const int* cntRow = L.cnt + rowBase;
    const uint8_t* obRow = R.mp_obs + rowBase;
    unsigned int pk[TK_K];
    int pc = 0;
    uint8_t pob = 0;
    auto fetch = [&](int W0) {
        const int last = nq * TK_K - 1;
#pragma unroll
        for (int r = 0; r < TK_K; ++r) pk[r] = keyRow[min(W0 * TK_K + r * 64 + lane, last)];
        const int qc = min(W0 + lane, nq - 1);
        pc = cntRow[qc];
        pob = (W0 + lane < nq && pc > 0) ? obRow[qc] : 0;
    };
    if (nq > 0) fetch(0);
    for (int W0 = 0; W0 < nq; W0 += 64) {
#pragma unroll
        for (int r = 0; r < TK_K; ++r) sk[r * 64 + lane] = pk[r];             // query i's list: sk[i * TK_K .. + TK_K)
        const int cnt = W0 + lane < nq ? pc : 0;
        const int ob = pob != 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (W0 + 64 < nq) fetch(W0 + 64);
        unsigned long long todo = __ballot(cnt > 0);                        // skipped queries and empty windows have count 0
        while (todo) {
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            unsigned int key = INV;
            bool fr = false;
            if (lane < TK_K) {
                key = sk[i * TK_K + lane];
                const unsigned int k = key == INV ? 0u : key & 0xFFFFu;
                fr = key != INV && !((blk[k >> 5] >> (k & 31)) & 1u);
            }
            const unsigned long long fb = __ballot(fr);
            unsigned int best = fb ? (unsigned)__builtin_amdgcn_readlane((int)key, __ffsll((long long)fb) - 1) : INV;
            if (best == INV && __builtin_amdgcn_readlane(cnt, i) > TK_K) {
                // every listed candidate is blocked and the window holds more: the window again, blocked set applied
                const size_t o = rowBase + W0 + i;
                Win w;                                                       // the window k_mm_topk swept (its radius from there: no scale table here)
                w.r = L.r[o];
                mm_levels(R, p, R.octave[o], o, urt != nullptr, w);
                u64 a[4], top[TK_K];
                load_desc(R.qdesc + o * 32, a);
                int c2;
                win_sweep<false>(w, RotBinPay{R.angle[o], R.factor}, T, urt, a, blk, lane, c2, top);
                best = cand_word(top[0]);
            }
            if (best == INV || (best >> 21) > 100u) continue;                // TH_HIGH (:2589)
            const unsigned int k = best & 0xFFFFu, bin = (best >> 16) & 31u;
            const int obi = __builtin_amdgcn_readlane(ob, i);
            const bool withBin = R.check_ori && bin != TK_NOBIN;
            if (lane == 0) {
                mrow[k] = W0 + i;                                            // may overwrite a claim of a query without observations
                if (obi) blk[k >> 5] |= 1u << (k & 31);
                if (withBin) { acc[nacc] = k | (bin << 16); hist[bin] += 1u; }
            }
            ++nm;                                                            // overwrites count, as the reference's nmatches++ does
            if (withBin) ++nacc;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");              // the next chunk's lists overwrite sk
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (R.check_ori) nm -= rot_cull(hist, acc, nacc, mrow, lane);
    if (lane == 0) {
        nmatches[p] = nm;
        if (retried) retried[p] = RETRY ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------
// M4 with Nleft != -1 (a fisheye rig: ORBmatcher.cc:2469-2711 with the right-camera block :2615-2680), final rows on the device.  A pair
// is a left row (mvKeys, mGrid) and a right row (mvKeysRight, mGridRight) of one pool; there is no stereo gate (:2569).  The candidate
// pass is k_mm_topk once per camera -- (u, v) over the left rows, (ur, vr) over the right rows, each with its own count / key / radius
// lists -- so the radius th * sf[octave] and the rotation bin are mm_query's and RotBinPay's, the bin against the angle of the row
// that was searched (:2602-2604, :2668).
// k_mmf_claim: one wave per pair replays the queries in order.  A query whose LEFT window is empty is finished: the `continue` of
//   :2551 skips the right block too, and the window population is counted before blocked slots are looked at.  Otherwise it claims
//   its first unblocked candidate of least distance in the left row (:2556-2593) and then, independently, in the right row
//   (:2637-2661), each camera with its own blocked bit array in LDS (mvpMapPoints[i2] and [i2 + Nleft]); a listed-all-blocked window
//   that holds more than TK_K is rescanned per camera (win_sweep<false>).  Both cameras' assignments go into ONE histogram and one
//   accepted list (slot | bin << 16 | camera << 21, :2612 / :2677); the three-maxima cull (:2688-2708) writes ORBM_MATCH_PRUNED to
//   the row the entry names and counts down once per entry.
// RETRY: as k_mm_*: 2 * th, both blocked sets empty, only the pairs whose count is below retry_below (Tracking.cc:3213-3221).
// ------------------------------------------------------------------------------------------------
// one camera's row of a pair and its projections
struct MmfCam { PoolRow T; const float* px; const float* py; };             // px, py [npairs][q_stride]

// query i of the current 64 (row o) in one camera: the first listed candidate that is not blocked, or, when every listed one is
// blocked and the window holds more, the window again with the blocked set applied.  0xFFFFFFFF: nothing to claim.
__device__ __forceinline__ unsigned int mmf_best(const unsigned int* sk, int i, const unsigned int* blk, int cnt, float r, const MmfCam& cam,
                                                 const MmRows& R, int p, size_t o, int lane) {
    const unsigned INV = 0xFFFFFFFFu;
    unsigned int key = INV;
    bool fr = false;
    if (lane < TK_K) {
        key = sk[i * TK_K + lane];
        const unsigned int k = key == INV ? 0u : key & 0xFFFFu;
        fr = key != INV && !((blk[k >> 5] >> (k & 31)) & 1u);
    }
    const unsigned long long fb = __ballot(fr);
    unsigned int best = fb ? (unsigned)__builtin_amdgcn_readlane((int)key, __ffsll((long long)fb) - 1) : INV;
    if (best == INV && cnt > TK_K) {
        Win w;                                                               // the window k_mm_topk swept for this camera
        w.r = r;
        mm_levels(R, p, R.octave[o], o, false, w);
        w.x = cam.px[o]; w.y = cam.py[o];
        u64 a[4], top[TK_K];
        load_desc(R.qdesc + o * 32, a);
        int c2;
        win_sweep<false>(w, RotBinPay{R.angle[o], R.factor}, cam.T, nullptr, a, blk, lane, c2, top);
        best = cand_word(top[0]);
    }
    return best;
}

// rot_cull over two rows: entry = slot | bin << 16 | camera << 21
__device__ __forceinline__ int rot_cull_lr(const unsigned int* hist, const unsigned int* acc, int nacc, int* mrow_l, int* mrow_r, int lane) {
    const Max3 m3 = three_maxima(hist);
    const int i1 = m3.i1, i2 = m3.i2, i3 = m3.i3;
    int pruned = 0;
    for (int e = lane; e < nacc; e += 64) {
        const unsigned int v = acc[e];
        const int bin = (int)((v >> 16) & 31u), k = (int)(v & 0xFFFFu);
        if (bin != i1 && bin != i2 && bin != i3) { ((v >> 21) & 1u ? mrow_r : mrow_l)[k] = -2; ++pruned; }   // ORBM_MATCH_PRUNED
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pruned += __shfl_xor(pruned, o);
    return pruned;
}

template <bool RETRY>
__global__ __launch_bounds__(64) void k_mmf_claim(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ counts, int cap,
                                                 const int* __restrict__ grid_start, const int* __restrict__ grid_idx,
                                                 float min_x, float min_y, float inv_w, float inv_h, int first_l, int first_r,
                                                  const uint8_t* __restrict__ blocked_l, const uint8_t* __restrict__ blocked_r, MmRows R,
                                                  const float* __restrict__ ur, const float* __restrict__ vr, TopList LL, TopList LR,
                                                  unsigned int* __restrict__ accepted,
                                                  int* __restrict__ match_l, int* __restrict__ match_r, int* __restrict__ nmatches,
                                                  uint8_t* __restrict__ retried) {
    extern __shared__ unsigned int mmf_lds[];                                // blocked bits left, right [ceil(cap / 32)] each, hist[32], the current 64 queries' lists [64][TK_K] per camera
    const unsigned INV = 0xFFFFFFFFu;
    const Pool pool{kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h};
    const int lane = threadIdx.x, p = blockIdx.x, fl = first_l + p, fr = first_r + p;
    if (RETRY && !(nmatches[p] < R.retry_below)) return;                    // (wave-uniform) the first search of this pair stands
    const int ntl = min(max(pool.counts[fl], 0), cap), ntr = min(max(pool.counts[fr], 0), cap);
    const int nq = min(max(R.nq[p], 0), R.q_stride);
    const int nwords = (cap + 31) >> 5;
    unsigned int* blkL = mmf_lds;
    unsigned int* blkR = blkL + nwords;
    unsigned int* hist = blkR + nwords;
    unsigned int* skL = hist + 32;
    unsigned int* skR = skL + 64 * TK_K;
    int* mrowL = match_l + (size_t)p * cap;
    int* mrowR = match_r + (size_t)p * cap;
    const uint8_t* tbl = !RETRY && blocked_l ? blocked_l + (size_t)p * cap : nullptr;   // the retry starts from an empty frame (Tracking.cc:3217)
    const uint8_t* tbr = !RETRY && blocked_r ? blocked_r + (size_t)p * cap : nullptr;
    for (int wd = lane; wd < nwords; wd += 64) { blkL[wd] = bits_word(tbl, ntl, wd, 0u); blkR[wd] = bits_word(tbr, ntr, wd, 0u); }
    if (lane < 32) hist[lane] = 0;
    for (int k = lane; k < cap; k += 64) { mrowL[k] = -1; mrowR[k] = -1; }  // ORBM_NO_MATCH
    __syncthreads();
    const size_t rowBase = (size_t)p * R.q_stride;
    const MmfCam camL{pool.row(fl), R.u, R.v}, camR{pool.row(fr), ur, vr};
    unsigned int* acc = accepted + rowBase * 2;                              // at most one entry per query and camera, in order
    int nm = 0, nacc = 0;
    // the next 64 queries' lists and counts of both cameras are in flight while the current ones are replayed (clamped, unconditional
    // loads); mp_obs is read only for a query with left candidates (any other row reads nothing else)
    const unsigned int* keyRowL = LL.keys + rowBase * TK_K;
    const unsigned int* keyRowR = LR.keys + rowBase * TK_K;
    const int* cntRowL = LL.cnt + rowBase;
    const int* cntRowR = LR.cnt + rowBase;
    const uint8_t* obRow = R.mp_obs + rowBase;
    unsigned int pkL[TK_K], pkR[TK_K];
    int pcL = 0, pcR = 0;
    uint8_t pob = 0;
    auto fetch = [&](int W0) {
        const int last = nq * TK_K - 1;
#pragma unroll
        for (int r = 0; r < TK_K; ++r) {
            const int e = min(W0 * TK_K + r * 64 + lane, last);
            pkL[r] = keyRowL[e]; pkR[r] = keyRowR[e];
        }
        const int qc = min(W0 + lane, nq - 1);
        pcL = cntRowL[qc]; pcR = cntRowR[qc];
        pob = (W0 + lane < nq && pcL > 0) ? obRow[qc] : 0;
    };
    if (nq > 0) fetch(0);
    for (int W0 = 0; W0 < nq; W0 += 64) {
#pragma unroll
        for (int r = 0; r < TK_K; ++r) { skL[r * 64 + lane] = pkL[r]; skR[r * 64 + lane] = pkR[r]; }   // query i's lists: sk?[i * TK_K .. + TK_K)
        const int cntL = W0 + lane < nq ? pcL : 0;
        const int cntR = pcR;                                                // read only where cntL > 0
        const int ob = pob != 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (W0 + 64 < nq) fetch(W0 + 64);
        unsigned long long todo = __ballot(cntL > 0);                       // skipped queries and empty LEFT windows: the right block is skipped too (:2551)
        while (todo) {
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const size_t o = rowBase + W0 + i;
            const int obi = __builtin_amdgcn_readlane(ob, i);
#pragma unroll
            for (int c = 0; c < 2; ++c) {                                    // the left claim (:2556-2613), then the right one (:2637-2679)
                const int cn = __builtin_amdgcn_readlane(c ? cntR : cntL, i);
                if (cn <= 0) continue;                                       // (right) an empty window claims nothing
                unsigned int* blk = c ? blkR : blkL;
                const unsigned int best = mmf_best(c ? skR : skL, i, blk, cn, cn > TK_K ? (c ? LR.r : LL.r)[o] : 0.f, c ? camR : camL, R, p, o, lane);
                if (best == INV || (best >> 21) > 100u) continue;            // TH_HIGH (:2590, :2658)
                const unsigned int k = best & 0xFFFFu, bin = (best >> 16) & 31u;
                const bool withBin = R.check_ori && bin != TK_NOBIN;
                if (lane == 0) {
                    (c ? mrowR : mrowL)[k] = W0 + i;                         // may overwrite a claim of a query without observations
                    if (obi) blk[k >> 5] |= 1u << (k & 31);
                    if (withBin) { acc[nacc] = k | (bin << 16) | ((unsigned)c << 21); hist[bin] += 1u; }
                }
                ++nm;                                                        // overwrites count, as the reference's nmatches++ does
                if (withBin) ++nacc;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");              // the next chunk's lists overwrite sk
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (R.check_ori) nm -= rot_cull_lr(hist, acc, nacc, mrowL, mrowR, lane);
    if (lane == 0) {
        nmatches[p] = nm;
        if (retried) retried[p] = RETRY ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------
// M3 with Nleft != -1 (a fisheye rig: ORBmatcher.cc:45-239 with the right-camera block :170-236), final rows on the device.  A pair is
// a left row and a right row of one pool as for k_mmf_claim; there is no stereo gate (:107).  The candidate pass is k_lp_topk once per
// camera -- an LpRows over the left fields with th over the left rows, an LpRows over the right fields with th = 1 (:173-176 apply no
// factor) over the right rows -- so lp_query's skips (not in view, bFarPoints, a level outside the table; -1 is the reference's own
// skip of :172) arrive here as a zero count.
// k_lpf_claim: one wave per pair replays the queries in order.  Per query the left list gives best and second among the slots not in
//   the left blocked set (one ballot; a truncated list with fewer than two is rescanned, win_sweep<false>); TH_HIGH and the same-level
//   ratio rule decide (:147-154).  A ratio rejection is the `continue` of :151-152: the query is finished, right block included.  A
//   claim writes match_l[best] and, if mvLeftToRightMatch[best] names a right slot, match_r of that slot as well (:157-161, no look at
//   the blocked set), each counted; with mp_obs every written slot is blocked in its camera's bit array, which the right block of the
//   same query already sees.  The right block (:170-236) is the mirror over the right list: mvRightToLeftMatch[best] into match_l,
//   then match_r[best].  Partner slots are read at claim time (wave-uniform) and honoured only inside the other row's count.
// ------------------------------------------------------------------------------------------------
// query i of the current 64 (row o, index q of its pair) in one camera: the first two listed candidates that are not blocked, or,
// when the truncated list holds fewer than two, the window again with the blocked set applied.  0xFFFFFFFF: none.
__device__ __forceinline__ void lpf_top2(const unsigned int* sk, int i, const unsigned int* blk, int cnt, const float* topR, const PoolRow& T,
                                         const LpRows& R, size_t o, int q, int lane, unsigned int& w1, unsigned int& w2) {
    const unsigned INV = 0xFFFFFFFFu;
    unsigned int key = INV;
    bool fr = false;
    if (lane < TK_K) {
        key = sk[i * TK_K + lane];
        const unsigned int k = key == INV ? 0u : key & 0xFFFFu;
        fr = key != INV && !((blk[k >> 5] >> (k & 31)) & 1u);
    }
    unsigned long long fb = __ballot(fr);
    w1 = INV; w2 = INV;
    if (fb) {
        w1 = (unsigned)__builtin_amdgcn_readlane((int)key, __ffsll((long long)fb) - 1);
        fb &= fb - 1;
        if (fb) w2 = (unsigned)__builtin_amdgcn_readlane((int)key, __ffsll((long long)fb) - 1);
    }
    if (w2 == INV && cnt > TK_K) {
        const Win w = {R.px[o], R.py[o], topR[o], 0.f, R.level[o] - 1, R.level[o]};   // the window k_lp_topk swept for this camera
        u64 a[4], top[TK_K];
        load_desc(R.qdesc + (R.q_shared ? (size_t)q : o) * 32, a);
        int c2;
        win_sweep<false>(w, OctavePay{}, T, nullptr, a, blk, lane, c2, top);
        w1 = cand_word(top[0]); w2 = cand_word(top[1]);
    }
}

__global__ __launch_bounds__(64) void k_lpf_claim(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ counts, int cap,
                                                 const int* __restrict__ grid_start, const int* __restrict__ grid_idx,
                                                 float min_x, float min_y, float inv_w, float inv_h, int first_l, int first_r,
                                                  const uint8_t* __restrict__ blocked_l, const uint8_t* __restrict__ blocked_r,
                                                  const int* __restrict__ l2r, const int* __restrict__ r2l, LpRows RL, LpRows RR, float nnratio,
                                                  TopList LL, TopList LR, int* __restrict__ match_l, int* __restrict__ match_r, int* __restrict__ nmatches) {
    extern __shared__ unsigned int lpf_lds[];                                // blocked bits left, right [ceil(cap / 32)] each, the current 64 queries' lists [64][TK_K] per camera
    const unsigned INV = 0xFFFFFFFFu;
    const Pool pool{kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h};
    const int lane = threadIdx.x, p = blockIdx.x, fl = first_l + p, fr = first_r + p;
    const int ntl = min(max(pool.counts[fl], 0), cap), ntr = min(max(pool.counts[fr], 0), cap);
    const int nq = min(max(RL.nq[p], 0), RL.q_stride);
    const int nwords = (cap + 31) >> 5;
    unsigned int* blkL = lpf_lds;
    unsigned int* blkR = blkL + nwords;
    unsigned int* skL = blkR + nwords;
    unsigned int* skR = skL + 64 * TK_K;
    int* mrowL = match_l + (size_t)p * cap;
    int* mrowR = match_r + (size_t)p * cap;
    const uint8_t* tbl = blocked_l ? blocked_l + (size_t)p * cap : nullptr;
    const uint8_t* tbr = blocked_r ? blocked_r + (size_t)p * cap : nullptr;
    for (int wd = lane; wd < nwords; wd += 64) { blkL[wd] = bits_word(tbl, ntl, wd, 0u); blkR[wd] = bits_word(tbr, ntr, wd, 0u); }
    for (int k = lane; k < cap; k += 64) { mrowL[k] = -1; mrowR[k] = -1; }  // ORBM_NO_MATCH
    __syncthreads();
    const size_t rowBase = (size_t)p * RL.q_stride;
    const PoolRow camL = pool.row(fl), camR = pool.row(fr);
    const int* l2rRow = l2r ? l2r + (size_t)p * cap : nullptr;               // mvLeftToRightMatch / mvRightToLeftMatch of the pair
    const int* r2lRow = r2l ? r2l + (size_t)p * cap : nullptr;
    int nm = 0;
    // the next 64 queries' lists and counts of both cameras are in flight while the current ones are replayed (clamped, unconditional
    // loads); mp_obs is read only for a query with candidates in either camera (any other row reads nothing else)
    const unsigned int* keyRowL = LL.keys + rowBase * TK_K;
    const unsigned int* keyRowR = LR.keys + rowBase * TK_K;
    const int* cntRowL = LL.cnt + rowBase;
    const int* cntRowR = LR.cnt + rowBase;
    const uint8_t* obRow = RL.mp_obs + (RL.q_shared ? (size_t)0 : rowBase);
    unsigned int pkL[TK_K], pkR[TK_K];
    int pcL = 0, pcR = 0;
    uint8_t pob = 0;
    auto fetch = [&](int W0) {
        const int last = nq * TK_K - 1;
#pragma unroll
        for (int r = 0; r < TK_K; ++r) {
            const int e = min(W0 * TK_K + r * 64 + lane, last);
            pkL[r] = keyRowL[e]; pkR[r] = keyRowR[e];
        }
        const int qc = min(W0 + lane, nq - 1);
        pcL = cntRowL[qc]; pcR = cntRowR[qc];
        pob = (W0 + lane < nq && (pcL > 0 || pcR > 0)) ? obRow[qc] : 0;
    };
    if (nq > 0) fetch(0);
    for (int W0 = 0; W0 < nq; W0 += 64) {
#pragma unroll
        for (int r = 0; r < TK_K; ++r) { skL[r * 64 + lane] = pkL[r]; skR[r * 64 + lane] = pkR[r]; }   // query i's lists: sk?[i * TK_K .. + TK_K)
        const int cntL = W0 + lane < nq ? pcL : 0;
        const int cntR = W0 + lane < nq ? pcR : 0;
        const int ob = pob != 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (W0 + 64 < nq) fetch(W0 + 64);
        unsigned long long todo = __ballot(cntL > 0 || cntR > 0);           // skipped queries and two empty windows claim nothing; an empty LEFT window alone does not end the query
        while (todo) {
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const size_t o = rowBase + W0 + i;
            const int obi = __builtin_amdgcn_readlane(ob, i);
#pragma unroll
            for (int c = 0; c < 2; ++c) {                                    // the left block (:65-168), then the right one (:170-236)
                const int cn = __builtin_amdgcn_readlane(c ? cntR : cntL, i);
                if (cn <= 0) continue;                                       // block skipped, or an empty window (:85, :178)
                unsigned int* blk = c ? blkR : blkL;
                unsigned int* oblk = c ? blkL : blkR;
                unsigned int w1, w2;
                lpf_top2(c ? skR : skL, i, blk, cn, c ? LR.r : LL.r, c ? camR : camL, c ? RR : RL, o, W0 + i, lane, w1, w2);
                if (w1 == INV) continue;                                     // every candidate blocked: bestDist stays 256
                const int bestDist = (int)(w1 >> 21), bestLevel = (int)((w1 >> 16) & 31u) - 1;
                const int bestDist2 = w2 == INV ? 256 : (int)(w2 >> 21), bestLevel2 = w2 == INV ? -1 : (int)((w2 >> 16) & 31u) - 1;
                if (bestDist > 100) continue;                                // TH_HIGH (:147, :219)
                if (bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2) break;   // :151-152, :221-222: the query is finished
                if (c == 0 && !(bestLevel != bestLevel2 || (float)bestDist <= nnratio * (float)bestDist2)) continue;   // :154
                const unsigned int k = w1 & 0xFFFFu;
                const int* prow = c ? r2lRow : l2rRow;
                int partner = prow ? prow[k] : -1;                           // :157, :224 (wave-uniform)
                if (partner < 0 || partner >= (c ? ntl : ntr)) partner = -1;
                if (lane == 0) {
                    (c ? mrowR : mrowL)[k] = W0 + i;                         // may overwrite a claim of a query without observations
                    if (obi) blk[k >> 5] |= 1u << (k & 31);
                    if (partner >= 0) {
                        (c ? mrowL : mrowR)[partner] = W0 + i;               // :158, :225: whatever the slot holds
                        if (obi) oblk[partner >> 5] |= 1u << (partner & 31);
                    }
                }
                nm += partner >= 0 ? 2 : 1;                                  // overwrites count, as the reference's nmatches++ does
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");              // the next chunk's lists overwrite sk
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) nmatches[p] = nm;
}

// k_mm_project: the LastFrame MapPoints of every pair through the current pose (ORBmatcher.cc:2481-2527 as facade/ORBmatcher.h
// evaluates it against cvcompat.h): a 3x3 * 3x1 product accumulates in double and rounds once to float, the translation is a float
// add; invzc = (float)(1.0 / (double)z); pinhole u = fx * xc / zc + cx (Pinhole.cpp:33-37).  A rejected point (no MapPoint or an
// outlier, invzc < 0, outside the bounds) gets valid = 0 and u = v = invzc = 0.  Thread 0 of each pair also writes its direction
// (0, 1 = bForward, 2 = bBackward) from tlc = Rlw * (-Rcw^T * tcw) + tlw.
struct MmProj { float k[4], bounds[4], mb; int mono, q_stride; };
__device__ __forceinline__ float mm_dot3(float r0, float r1, float r2, float x0, float x1, float x2) {
    double s = 0;
    s += (double)r0 * (double)x0;
    s += (double)r1 * (double)x1;
    s += (double)r2 * (double)x2;
    return (float)s;
}
__global__ __launch_bounds__(256) void k_mm_project(const float* __restrict__ tcw_cur, const float* __restrict__ tcw_last, const int* __restrict__ nq,
                                                    const float* __restrict__ x3dw, const uint8_t* __restrict__ has_mp, MmProj P,
                                                    uint8_t* __restrict__ valid, float* __restrict__ u, float* __restrict__ v,
                                                    float* __restrict__ invzc, uint8_t* __restrict__ dir) {
    const int p = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const float* T = tcw_cur + (size_t)p * 12;                              // row-major 3x4 [R | t]
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float twc[3];
        for (int r = 0; r < 3; ++r) twc[r] = mm_dot3(-T[0 * 4 + r], -T[1 * 4 + r], -T[2 * 4 + r], T[3], T[7], T[11]);   // -Rcw.t() * tcw
        const float* Tl = tcw_last + (size_t)p * 12;
        const float tlcz = mm_dot3(Tl[8], Tl[9], Tl[10], twc[0], twc[1], twc[2]) + Tl[11];                              // (Rlw * twc + tlw)(2)
        dir[p] = (!P.mono && tlcz > P.mb) ? 1 : (!P.mono && -tlcz > P.mb) ? 2 : 0;
    }
    const int n = min(max(nq[p], 0), P.q_stride);
    if (q >= n) return;
    const size_t o = (size_t)p * P.q_stride + q;
    uint8_t ok = 0;
    float pu = 0.f, pv = 0.f, iz = 0.f;
    if (has_mp[o]) {
        const float* X = x3dw + o * 3;
        const float x0 = X[0], x1 = X[1], x2 = X[2];
        const float xc = mm_dot3(T[0], T[1], T[2], x0, x1, x2) + T[3];
        const float yc = mm_dot3(T[4], T[5], T[6], x0, x1, x2) + T[7];
        const float zc = mm_dot3(T[8], T[9], T[10], x0, x1, x2) + T[11];
        const float izc = (float)(1.0 / (double)zc);
        if (!(izc < 0)) {
            const float uu = P.k[0] * xc / zc + P.k[2], vv = P.k[1] * yc / zc + P.k[3];
            if (!(uu < P.bounds[0] || uu > P.bounds[1]) && !(vv < P.bounds[2] || vv > P.bounds[3])) { ok = 1; pu = uu; pv = vv; iz = izc; }
        }
    }
    valid[o] = ok; u[o] = pu; v[o] = pv; invzc[o] = iz;
}

// ------------------------------------------------------------------------------------------------
// Batched Fuse -- M13, the search core of ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:1823-2049, chi2 = 1) and of its Sim3
// twin (:2051-2199, chi2 = 0) -- for (KeyFrame row, query row) pairs, pinhole, Nleft == -1.  No claims: a MapPoint's best slot depends on
// no other MapPoint, so every (pair, query) is independent.
// k_fuse_topk: a wave per (pair, query), as k_lp_topk.  The projection and the gates run wave-uniformly in the facade's numerics against
//   cvcompat.h (fuse_project); the window KeyFrame::GetFeaturesInArea (KeyFrame.cc:916-962: no level or stereo gate) is one win_sweep
//   with the level band [level-1, level] (:1959) and FuseGate.  The smallest key is the `dist < bestDist` first minimum in visiting order.
// k_fuse_count: one block per pair counts the row's fused entries (deterministic, nothing to zero before a replay).
// ------------------------------------------------------------------------------------------------
struct FuseRows {                                          // the per-query arrays of one call, [npairs][q_stride] unless q_shared
    const int* nq; const uint8_t* valid;
    const float* pw; const float* normal; const float* min_dist; const float* max_dist; const uint8_t* qdesc;
};
struct FuseParams { float k[4], bounds[4], bf, th, logSF; int nlevels, q_stride, q_shared, chi2, nkf_rows; float sf[12], isg[12]; };

// Fuse's candidate test (ORBmatcher.cc:1963-1992): the reprojection error against the keypoint's level sigma, with the right-image term
// where the slot has an mvuRight >= 0 (urt NULL: none has).  Float expressions in the reference's order, compared with the double literal.
struct FuseGate {
    static constexpr bool on = true;
    float u, v, ur;
    const float* __restrict__ urt;
    const float* isg;
    bool chi2;                                                               // 0: the Sim3 variant, no test
    __device__ bool operator()(const KpIn& kp, int k) const {
        if (!chi2) return true;
        const float ex = u - kp.x, ey = v - kp.y;
        if (urt && urt[k] >= 0) {
            const float er = ur - urt[k];
            const float e2 = ex * ex + ey * ey + er * er;
            return !(e2 * isg[kp.octave] > 7.8);
        }
        const float e2 = ex * ex + ey * ey;
        return !(e2 * isg[kp.octave] > 5.99);
    }
};

// The projection and geometric gates of Fuse (ORBmatcher.cc:1878-1930 as facade/ORBmatcher.h evaluates them against cvcompat.h): x3Dc
// through mm_dot3 + t, z < 0 rejects, invz = 1 / z, pinhole u = fx * x / z + cx, KeyFrame::IsInImage (half-open, KeyFrame.cc:965-968),
// ur = u - bf * invz, dist3D the float of a double norm against [0.8 min, 1.2 max], PO . Pn (double) >= 0.5 dist3D, then PredictScale as
// k_frustum computes it.  Returns the predicted level, or -1.
// FORM 1 is the projection of SearchByProjection's vpPointsKFs overload (:724-729): x * invz first, then fx * x + cx; it rounds differently.
template <int FORM = 0>
__device__ __forceinline__ int fuse_project(const float* T, const float* O, const float* X, const float* N, float minDist, float maxDist,
                                            const FuseParams& P, float& u, float& v, float& ur) {
    const float x0 = X[0], x1 = X[1], x2 = X[2];
    const float xc = mm_dot3(T[0], T[1], T[2], x0, x1, x2) + T[3];
    const float yc = mm_dot3(T[4], T[5], T[6], x0, x1, x2) + T[7];
    const float zc = mm_dot3(T[8], T[9], T[10], x0, x1, x2) + T[11];
    if (zc < 0.0f) return -1;
    const float invz = 1.0f / zc;
    if (FORM == 1) {
        const float x = xc * invz, y = yc * invz;
        u = P.k[0] * x + P.k[2];
        v = P.k[1] * y + P.k[3];
    } else {
        u = P.k[0] * xc / zc + P.k[2];
        v = P.k[1] * yc / zc + P.k[3];
    }
    if (!(u >= P.bounds[0] && u < P.bounds[1] && v >= P.bounds[2] && v < P.bounds[3])) return -1;
    ur = u - P.bf * invz;
    const float maxD = 1.2f * maxDist, minD = 0.8f * minDist;
    const float o0 = x0 - O[0], o1 = x1 - O[1], o2 = x2 - O[2];
    double d2 = 0.0;
    d2 += (double)o0 * (double)o0; d2 += (double)o1 * (double)o1; d2 += (double)o2 * (double)o2;
    const float dist = (float)sqrt(d2);
    if (dist < minD || dist > maxD) return -1;
    double dot = 0.0;
    dot += (double)o0 * (double)N[0]; dot += (double)o1 * (double)N[1]; dot += (double)o2 * (double)N[2];
    if (dot < 0.5 * (double)dist) return -1;
    const float ratio = maxDist / dist;
    const float lg = (float)log((double)ratio);
    int ns = (int)ceilf(lg / P.logSF);
    if (ns < 0) ns = 0; else if (ns >= P.nlevels) ns = P.nlevels - 1;
    return ns;
}

__global__ __launch_bounds__(256) void k_fuse_topk(Pool pool, const float* __restrict__ uright, const int* __restrict__ kf_row, const float* __restrict__ tcw, const float* __restrict__ ow,
                                                   FuseRows R, FuseParams P, int* __restrict__ best_idx, int* __restrict__ level_out) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.y;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= P.q_stride) return;
    const size_t o = (size_t)p * P.q_stride + q;
    const int row = kf_row ? kf_row[p] : p;
    const int nq = min(max(R.nq[p], 0), P.q_stride);
    int lvl = -1, best = -1;
    float u = 0.f, v = 0.f, ur = 0.f;
    const size_t qo = P.q_shared ? (size_t)q : o;
    if (row >= 0 && row < P.nkf_rows && q < nq && R.valid[o])
        lvl = fuse_project(tcw + (size_t)p * 12, ow + (size_t)p * 3, R.pw + qo * 3, R.normal + qo * 3, R.min_dist[qo], R.max_dist[qo], P, u, v, ur);
    if (lvl >= 0) {
        u64 a[4];
        load_desc(R.qdesc + qo * 32, a);
        const Win w = {u, v, P.th * P.sf[lvl], 0.f, lvl - 1, lvl};               // radius = th * mvScaleFactors[nPredictedLevel]
        const FuseGate g = {u, v, ur, uright ? uright + (size_t)row * pool.cap : nullptr, P.isg, P.chi2 != 0};
        int cnt;
        u64 top[TK_K];
        win_sweep<true>(w, OctavePay{}, pool.row(row), nullptr, a, nullptr, lane, cnt, top, g);
        if (top[0] != ~0ull && (int)(top[0] >> 40) <= 50) best = (int)(top[0] & 0xFFFFu);   // bestDist <= TH_LOW
    }
    if (lane == 0) {
        best_idx[o] = best;
        if (level_out) level_out[o] = lvl;
    }
}

__global__ __launch_bounds__(256) void k_fuse_count(const int* __restrict__ best_idx, int q_stride, int* __restrict__ nfused) {
    __shared__ int part[4];
    const int p = blockIdx.x;
    int c = 0;
    for (int i = threadIdx.x; i < q_stride; i += 256) c += best_idx[(size_t)p * q_stride + i] >= 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) nfused[p] = part[0] + part[1] + part[2] + part[3];
}

// ------------------------------------------------------------------------------------------------
// Batched relocalisation SearchByProjection -- M5, SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:
// 2723-2852) of Tracking::Relocalization -- for (frame row, candidate KeyFrame, pose) pairs, pinhole, Nleft == -1.  Query i of a pair
// is KeyFrame slot i; the frame is a row of a Frame pool with its grid.
// k_rl_topk: a wave per (pair, query), as k_fuse_topk.  The projection and gates run wave-uniformly (rl_project); the window
//   Frame::GetFeaturesInArea(u, v, th * scale[level], level - 1, level + 1) (:2778) is one win_sweep with the rotation-bin payload of
//   angle_kf - angle_f (:2829-2833).  Out, as k_mm_topk: the window population, its TK_K best candidate words, the radius, and the
//   window centre and level a rescan needs.
// k_claim<RlPol> (k_rl_claim until the replay was shared with M6): one wave per pair replays the claims in query order, as k_mm_claim: the first unblocked listed candidate is the query's
//   `dist < bestDist` winner among the free slots; a truncated list whose candidates are all blocked is rescanned with the blocked set
//   applied.  Unlike M4, EVERY claim blocks its slot (:2793, mvpMapPoints[i2] is set for every match), so a slot is assigned at most once
//   and the rotation cull prunes each assignment once.  bestDist <= ORBdist accepts.
// ------------------------------------------------------------------------------------------------
struct RlRows {                                            // the per-query arrays of one call, [npairs][q_stride]
    const int* nq; const uint8_t* valid;
    const float* pw; const float* min_dist; const float* max_dist; const float* angle; const uint8_t* qdesc;
};
struct RlParams { float k[4], bounds[4], th, logSF, factor; int nlevels, q_stride, nf_rows, orb_dist, check_ori; float sf[12]; };

// The projection and gates of M5 (ORBmatcher.cc:2756-2776 as facade/ORBmatcher.h evaluates them against cvcompat.h): x3Dc through
// mm_dot3 + t, pinhole u = fx * x / z + cx with NO depth test, the closed bounds test (u < minX || u > maxX, v < minY || v > maxY
// reject), dist3D the float of a double norm against [0.8 min, 1.2 max], then PredictScale with the frame's log scale factor as
// k_frustum computes it.  Returns the predicted level, or -1.
__device__ __forceinline__ int rl_project(const float* T, const float* O, const float* X, float minDist, float maxDist, const RlParams& P,
                                          float& u, float& v) {
    const float x0 = X[0], x1 = X[1], x2 = X[2];
    const float xc = mm_dot3(T[0], T[1], T[2], x0, x1, x2) + T[3];
    const float yc = mm_dot3(T[4], T[5], T[6], x0, x1, x2) + T[7];
    const float zc = mm_dot3(T[8], T[9], T[10], x0, x1, x2) + T[11];
    u = P.k[0] * xc / zc + P.k[2];
    v = P.k[1] * yc / zc + P.k[3];
    if (u < P.bounds[0] || u > P.bounds[1]) return -1;
    if (v < P.bounds[2] || v > P.bounds[3]) return -1;
    const float maxD = 1.2f * maxDist, minD = 0.8f * minDist;
    const float o0 = x0 - O[0], o1 = x1 - O[1], o2 = x2 - O[2];
    double d2 = 0.0;
    d2 += (double)o0 * (double)o0; d2 += (double)o1 * (double)o1; d2 += (double)o2 * (double)o2;
    const float dist = (float)sqrt(d2);
    if (dist < minD || dist > maxD) return -1;
    const float ratio = maxDist / dist;
    const float lg = (float)log((double)ratio);
    int ns = (int)ceilf(lg / P.logSF);
    if (ns < 0) ns = 0; else if (ns >= P.nlevels) ns = P.nlevels - 1;
    return ns;
}

__global__ __launch_bounds__(256) void k_rl_topk(Pool pool, const int* __restrict__ f_row, const float* __restrict__ tcw, const float* __restrict__ ow,
                                                 RlRows R, RlParams P, TopList out, float4* __restrict__ out_win) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.y;
    const int row = f_row ? f_row[p] : p;
    if (row < 0 || row >= P.nf_rows) return;                                 // the claim replay reads nothing of this pair
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nq = min(max(R.nq[p], 0), P.q_stride);
    if (q >= nq) return;
    const size_t o = (size_t)p * P.q_stride + q;
    int lvl = -1, cnt = 0;
    float u = 0.f, v = 0.f, r = 0.f;
    u64 top[TK_K];
    if (R.valid[o]) lvl = rl_project(tcw + (size_t)p * 12, ow + (size_t)p * 3, R.pw + o * 3, R.min_dist[o], R.max_dist[o], P, u, v);
    if (lvl >= 0) {
        u64 a[4];
        load_desc(R.qdesc + o * 32, a);
        r = P.th * P.sf[lvl];                                                // radius = th * mvScaleFactors[nPredictedLevel], :2775
        const Win w = {u, v, r, 0.f, lvl - 1, lvl + 1};
        win_sweep<true>(w, RotBinPay{R.angle[o], P.factor}, pool.row(row), nullptr, a, nullptr, lane, cnt, top);
    } else {
#pragma unroll
        for (int i = 0; i < TK_K; ++i) top[i] = ~0ull;
    }
    if (lane == 0) {
        put_topk(out, o, cnt, r, top);
        out_win[o] = make_float4(u, v, 0.f, __int_as_float(lvl));            // read back only by a rescan (count > TK_K)
    }
}

// The replay is k_claim<Pol>; Pol carries what differs between the searches that share it: the per-query rows and parameters, the upper
// end of the level band, the sweep's payload, the acceptance test and whether a rotation histogram is kept.  RlPol is M5 (k_rl_claim).
struct RlPol {
    using Rows = RlRows;
    using Params = RlParams;
    __device__ static int hi(int lvl) { return lvl + 1; }
    __device__ static RotBinPay pay(const Rows& R, size_t o, const Params& P) { return RotBinPay{R.angle[o], P.factor}; }
    __device__ static bool accept(unsigned int best, const Params& P) { return (int)(best >> 21) <= P.orb_dist; }   // bestDist <= ORBdist (:2789)
    __device__ static bool ori(const Params& P) { return P.check_ori; }
};

template <class Pol>
__global__ __launch_bounds__(64) void k_claim(const KpIn* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ counts, int cap,
                                                 const int* __restrict__ grid_start, const int* __restrict__ grid_idx,
                                                 float min_x, float min_y, float inv_w, float inv_h, const int* __restrict__ f_row, const uint8_t* __restrict__ f_blocked,
                                              typename Pol::Rows R, typename Pol::Params P,
                                              const int* __restrict__ topCnt, const unsigned int* __restrict__ topKeys, const float* __restrict__ topR,
                                              const float4* __restrict__ topWin,
                                              unsigned int* __restrict__ accepted, int* __restrict__ match, int* __restrict__ nmatches) {
    extern __shared__ unsigned int rl_lds[];                                 // blocked bits [ceil(cap / 32)], hist[32], the current 64 queries' lists [64][TK_K]
    const unsigned INV = 0xFFFFFFFFu;
    const Pool pool{kps, desc, counts, cap, grid_start, grid_idx, min_x, min_y, inv_w, inv_h};
    const int lane = threadIdx.x, p = blockIdx.x;
    const int row = f_row ? f_row[p] : p;
    const bool live = row >= 0 && row < P.nf_rows;                           // (wave-uniform) an out-of-range row: all NO_MATCH and 0
    const int nt = live ? min(max(pool.counts[row], 0), cap) : 0;
    const int nq = live ? min(max(R.nq[p], 0), P.q_stride) : 0;
    const int nwords = (cap + 31) >> 5;
    unsigned int* blk = rl_lds;
    unsigned int* hist = rl_lds + nwords;
    unsigned int* sk = hist + 32;
    int* mrow = match + (size_t)p * cap;
    for (int wd = lane; wd < nwords; wd += 64) blk[wd] = bits_word(f_blocked ? f_blocked + (size_t)p * cap : nullptr, nt, wd, 0u);
    if (lane < 32) hist[lane] = 0;
    for (int k = lane; k < cap; k += 64) mrow[k] = -1;                      // ORBM_NO_MATCH
    __syncthreads();
    const PoolRow T = pool.row(live ? (size_t)row : 0);
    const size_t rowBase = (size_t)p * P.q_stride;
    unsigned int* acc = accepted + rowBase;                                  // (slot | bin << 16) of every assignment with a bin, in order
    int nm = 0, nacc = 0;
    // the next 64 queries' lists and counts are in flight while the current ones are replayed (clamped, unconditional loads)
    const unsigned int* keyRow = topKeys + rowBase * TK_K;
    const int* cntRow = topCnt + rowBase;
    unsigned int pk[TK_K];
    int pc = 0;
    auto fetch = [&](int W0) {
        const int last = nq * TK_K - 1;
#pragma unroll
        for (int r = 0; r < TK_K; ++r) pk[r] = keyRow[min(W0 * TK_K + r * 64 + lane, last)];
        pc = cntRow[min(W0 + lane, nq - 1)];
    };
    if (nq > 0) fetch(0);
    for (int W0 = 0; W0 < nq; W0 += 64) {
#pragma unroll
        for (int r = 0; r < TK_K; ++r) sk[r * 64 + lane] = pk[r];             // query i's list: sk[i * TK_K .. + TK_K)
        const int cnt = W0 + lane < nq ? pc : 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (W0 + 64 < nq) fetch(W0 + 64);
        unsigned long long todo = __ballot(cnt > 0);                        // skipped queries and empty windows have count 0
        while (todo) {
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            unsigned int key = INV;
            bool fr = false;
            if (lane < TK_K) {
                key = sk[i * TK_K + lane];
                const unsigned int k = key == INV ? 0u : key & 0xFFFFu;
                fr = key != INV && !((blk[k >> 5] >> (k & 31)) & 1u);
            }
            const unsigned long long fb = __ballot(fr);
            unsigned int best = fb ? (unsigned)__builtin_amdgcn_readlane((int)key, __ffsll((long long)fb) - 1) : INV;
            if (best == INV && __builtin_amdgcn_readlane(cnt, i) > TK_K) {
                // every listed candidate is blocked and the window holds more: the window k_rl_topk swept again, blocked set applied
                const size_t o = rowBase + W0 + i;
                const float4 cw = topWin[o];
                const int lvl = __float_as_int(cw.w);
                const Win w = {cw.x, cw.y, topR[o], 0.f, lvl - 1, Pol::hi(lvl)};
                u64 a[4], top[TK_K];
                load_desc(R.qdesc + o * 32, a);
                int c2;
                win_sweep<false>(w, Pol::pay(R, o, P), T, nullptr, a, blk, lane, c2, top);
                best = cand_word(top[0]);
            }
            if (best == INV || !Pol::accept(best, P)) continue;
            const unsigned int k = best & 0xFFFFu, bin = (best >> 16) & 31u;
            const bool withBin = Pol::ori(P) && bin != TK_NOBIN;
            if (lane == 0) {
                mrow[k] = W0 + i;
                blk[k >> 5] |= 1u << (k & 31);                               // every claim blocks its slot (:2791-2793)
                if (withBin) { acc[nacc] = k | (bin << 16); hist[bin] += 1u; }
            }
            ++nm;
            if (withBin) ++nacc;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");              // the next chunk's lists overwrite sk
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (Pol::ori(P)) nm -= rot_cull(hist, acc, nacc, mrow, lane);
    if (lane == 0) nmatches[p] = nm;
}

// ------------------------------------------------------------------------------------------------
// Batched Sim3 SearchByProjection -- M6, SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (ORBmatcher.cc:549-679) and its
// vpPointsKFs overload (:681-797) of LoopClosing::DetectCommonRegionsFromBoW / FindMatchesByProjection -- for (KeyFrame row, Sim3 pose,
// MapPoint row) triples, pinhole, Nleft == -1.  The shape of M5 on the inputs of M13:
// k_s3_topk: a wave per (pair, query).  fuse_project<FORM> is the projection with every gate (FORM 0: mpCamera->project, :602; FORM 1:
//   x * invz, :724-729); the window KeyFrame::GetFeaturesInArea(u, v, th * scale[level]) is one win_sweep with the level band
//   [level-1, level] (:637, :759).  Out, as k_rl_topk: the window population, its TK_K best candidate words, the radius, centre and level.
// k_claim<S3Pol>: the claim replay M5 uses (k_claim<RlPol>), one wave per pair in query order.  The blocked set starts as matched_in (vpMatched[idx],
//   :633, :755) and EVERY claim adds its slot (:653, :775: vpMatched[bestIdx] = pMP); (float)bestDist <= TH_LOW * ratioHamming accepts
//   (max_dist is that float product, below 256 by the entry point's check); no rotation check.
// ------------------------------------------------------------------------------------------------
struct S3Claim { int q_stride, nf_rows; float max_dist; };

template <int FORM>
__global__ __launch_bounds__(256) void k_s3_topk(Pool pool, const int* __restrict__ kf_row, const float* __restrict__ tcw, const float* __restrict__ ow,
                                                 FuseRows R, FuseParams P, TopList out, float4* __restrict__ out_win) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.y;
    const int row = kf_row ? kf_row[p] : p;
    if (row < 0 || row >= P.nkf_rows) return;                                // the claim replay reads nothing of this pair
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nq = min(max(R.nq[p], 0), P.q_stride);
    if (q >= nq) return;
    const size_t o = (size_t)p * P.q_stride + q;
    int lvl = -1, cnt = 0;
    float u = 0.f, v = 0.f, ur = 0.f, r = 0.f;
    u64 top[TK_K];
    if (R.valid[o])
        lvl = fuse_project<FORM>(tcw + (size_t)p * 12, ow + (size_t)p * 3, R.pw + o * 3, R.normal + o * 3, R.min_dist[o], R.max_dist[o], P, u, v, ur);
    if (lvl >= 0) {
        u64 a[4];
        load_desc(R.qdesc + o * 32, a);
        r = P.th * P.sf[lvl];                                                // radius = th * mvScaleFactors[nPredictedLevel], :622, :744
        const Win w = {u, v, r, 0.f, lvl - 1, lvl};
        win_sweep<true>(w, OctavePay{}, pool.row(row), nullptr, a, nullptr, lane, cnt, top);
    } else {
#pragma unroll
        for (int i = 0; i < TK_K; ++i) top[i] = ~0ull;
    }
    if (lane == 0) {
        put_topk(out, o, cnt, r, top);
        out_win[o] = make_float4(u, v, 0.f, __int_as_float(lvl));            // read back only by a rescan (count > TK_K)
    }
}

// the claim replay of M6 (k_claim<S3Pol>): blocked bits from matched_in, band [level-1, level], no rotation bin, the float bound
struct S3Rows { const int* nq; const uint8_t* qdesc; };
struct S3Pol {
    using Rows = S3Rows;
    using Params = S3Claim;
    __device__ static int hi(int lvl) { return lvl; }
    __device__ static OctavePay pay(const Rows&, size_t, const Params&) { return OctavePay{}; }
    __device__ static bool accept(unsigned int best, const Params& P) { return (float)(int)(best >> 21) <= P.max_dist; }   // bestDist <= TH_LOW * ratioHamming (:651, :773)
    __device__ static bool ori(const Params&) { return false; }
};

// ------------------------------------------------------------------------------------------------
// k_bow_transform2: DBoW2 TemplatedVocabulary::transform (TemplatedVocabulary.h:1196-1262) for a batch of descriptors: at every level the
// child with the smallest Hamming distance (first minimum, strict <) is taken; the node reached at level L - levelsup is recorded.
// The tree is in the level-major layout the host builds (orbm_vocab_create): nodes renumbered breadth-first so
// that the children of a node are CONTIGUOUS rows in its own child order; info[n] = first child << 5 | child count; orig[n] = the
// vocabulary's node id.  16 lanes per descriptor (4 descriptors per wave): lane c takes child c, the 16-lane minimum of
// (distance << 5 | c) by four DPP row rotations picks the first-minimum child (strict `d < best_d` in child order,
// TemplatedVocabulary.h:1239-1250).  A wave instruction then touches the 3 lines of each of its 4 child blocks instead of 64 scattered
// rows -- at ORBvoc's size (35.6 MB of node descriptors) the L1 line rate, not the arithmetic, bounds the thread-per-descriptor kernel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bow_transform2(const uint8_t* __restrict__ desc, int n, const unsigned* __restrict__ info,
                                                        const uint8_t* __restrict__ ndesc, const int* __restrict__ orig,
                                                        const int* __restrict__ nword, const double* __restrict__ nweight,
                                                        int L, int levelsup, int* __restrict__ word_id, int* __restrict__ node_id,
                                                        double* __restrict__ weight) {
    const int c = threadIdx.x & 15;
    const int i = (blockIdx.x * 256 + threadIdx.x) >> 4;
    const bool live = i < n;
    const uint4* qp = (const uint4*)(desc + (size_t)(live ? i : 0) * 32);
    const uint4 qlo = qp[0], qhi = qp[1];
    const u64 a[4] = {(u64)qlo.x | ((u64)qlo.y << 32), (u64)qlo.z | ((u64)qlo.w << 32),
                      (u64)qhi.x | ((u64)qhi.y << 32), (u64)qhi.z | ((u64)qhi.w << 32)};
    const int nid_level = L - levelsup;
    int cur = 0, nid = 0, level = 0;
    for (;;) {
        const unsigned inf = info[cur];
        const int cnt = (int)(inf & 31u), first = (int)(inf >> 5);
        // (uniform inside a 16-lane group; groups of a wave may leave at different levels: the DPP rotations stay inside a row)
        if (cnt == 0) break;
        ++level;
        unsigned best = 0xFFFFFFFFu;
        for (int c0 = 0; c0 < cnt; c0 += 16) {                             // k <= 16 in one step (DBoW2 allows k up to 20)
            unsigned key = 0xFFFFFFFFu;
            if (c0 + c < cnt) {
                const uint4* tp = (const uint4*)(ndesc + (size_t)(first + c0 + c) * 32);
                const uint4 lo = tp[0], hi = tp[1];
                const int d = ham256(a, (u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                                     (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32));
                key = ((unsigned)d << 5) | (unsigned)(c0 + c);
            }
            best = min(best, row16_min_u32(key));
        }
        cur = first + (int)(best & 31u);
        if (level == nid_level) nid = cur;
    }
    if (live && c == 0) {
        if (word_id) word_id[i] = nword[cur];
        if (weight) weight[i] = nweight[cur];
        node_id[i] = nid ? orig[nid] : 0;
    }
}

// ------------------------------------------------------------------------------------------------
// k_bow_search: M7 ORBmatcher::SearchByBoW(KeyFrame*, Frame&) (ORBmatcher.cc:314-547, Nleft == -1) for a batch of (KF row, frame row)
// pairs, one workgroup of BOW_WAVES waves per pair, everything in LDS.
// 1. Both rows are bucketed by (node & 255) with a STABLE counting sort (bow_buckets): each wave owns a contiguous run of indices,
//    per-wave histograms give every (bucket, wave) its first slot, and inside a 64-chunk a lane's rank among the lanes of its bucket
//    comes from eight ballots (v_mbcnt).  Each list is in ascending feature index, as a FeatureVector bucket is walked.  Stopped words
//    (weight <= 0), KF features without a good MapPoint and slots >= count are left out here.
// 2. Claims: wave w takes the hash buckets w, w + BOW_WAVES, ...  Features of different nodes never meet, so a hash list that holds
//    several nodes is still walked correctly in index order, and hash buckets are independent.  Per KF feature (in order) the lanes
//    take the frame list in passes of 64 (the first 64 stay in registers for the whole bucket), key = dist << 16 | list position for
//    an unmatched frame feature of the same node; the wave minimum is bestDist1 (first minimum in frame index order) and the minimum
//    of the other keys is the if / else-if chain's bestDist2.  An accepted claim writes KF index + 1 into the pair's LDS row.
// 3. check_orientation: the 30-bin histogram is rebuilt from the finished row (rot = angle_kf - angle_f, :451-459; a bin outside
//    [0, 30) is neither counted nor culled, as the host RotHist), three_maxima, and the matches of the other bins are cleared (-1).
// LDS: cur [BOW_WAVES][256] + kstart [257] + fstart [257] + hist [32] + red [8] ints, klist [cap_kf] + flist [cap_f] + row [cap_f]
// ushorts (bow_search_lds).
// ------------------------------------------------------------------------------------------------
#define BOW_WAVES 8
struct BowSide {                                           // one pool: rows of cap slots
    const KpIn* kps; const uint8_t* desc; const int* counts; const int* node; const double* weight; const uint8_t* good;
    int nrows, cap;
};
__host__ __device__ inline size_t bow_search_lds(int cap_kf, int cap_f) {
    return (size_t)(BOW_WAVES * 256 + 2 * 257 + 32 + 8) * sizeof(int) + (size_t)(cap_kf + 2 * cap_f) * sizeof(unsigned short);
}

__device__ __forceinline__ unsigned bow_rank(u64 m) {                       // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
__device__ __forceinline__ u64 readlane64(u64 v, int l) {
    return (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l) | ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l) << 32);
}
__device__ __forceinline__ bool bow_live(const BowSide& s, size_t o, int i, int n) {
    return i < n && (!s.weight || s.weight[o + i] > 0) && (!s.good || s.good[o + i]);
}

// One row of a pool as a bucket source: index i is slot i of row `o`.
struct BowRow {
    const BowSide& s; size_t o; int n;
    __device__ __forceinline__ bool live(int i) const { return bow_live(s, o, i, n); }
    __device__ __forceinline__ int node(int i) const { return s.node[o + i]; }
};
// Two rows of one pool as ONE index space [0, nl + nr): the reference's realIdxF of a two-camera Frame (left slot j is j, right slot j
// is Nleft + j, ORBmatcher.cc:406).  at(i) is the pool offset of combined index i.
struct BowRowPair {
    const BowSide& s; size_t ol, orr; int nl, n;
    __device__ __forceinline__ size_t at(int i) const { return i < nl ? ol + i : orr + (i - nl); }
    __device__ __forceinline__ bool live(int i) const {
        if (i >= n) return false;
        const size_t g = at(i);
        return !s.weight || s.weight[g] > 0;
    }
    __device__ __forceinline__ int node(int i) const { return s.node[at(i)]; }
};

// the stable (node & 255) buckets of the n indices of src: start [257], list [n live entries] (whole workgroup)
template <class Src>
__device__ void bow_buckets_of(const Src& src, int n, int* cur, int* start, int* red, unsigned short* list) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (int e = tid; e < BOW_WAVES * 256; e += BOW_WAVES * 64) cur[e] = 0;
    __syncthreads();
    const int per = ((n + BOW_WAVES * 64 - 1) / (BOW_WAVES * 64)) * 64;     // whole 64-chunks per wave, in index order
    const int lo = min(w * per, n), hi = min(lo + per, n);
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        if (i < hi && src.live(i)) atomicAdd(&cur[w * 256 + (src.node(i) & 255)], 1);
    }
    __syncthreads();
    int c[BOW_WAVES], tot = 0, ex = 0;
    if (tid < 256) {                                                         // bucket h = tid: (h, wave) order
#pragma unroll
        for (int v = 0; v < BOW_WAVES; ++v) { c[v] = cur[v * 256 + tid]; tot += c[v]; }
        int wt;
        ex = wave_excl_scan(tot, &wt);
        if (lane == 0) red[w] = wt;
    }
    __syncthreads();
    if (tid < 256) {
        int base = ex;
        for (int v = 0; v < w; ++v) base += red[v];
        start[tid] = base;
        if (tid == 255) start[256] = base + tot;
#pragma unroll
        for (int v = 0; v < BOW_WAVES; ++v) { cur[v * 256 + tid] = base; base += c[v]; }
    }
    __syncthreads();
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const bool ok = i < hi && src.live(i);
        const int h = ok ? (src.node(i) & 255) : 0;
        u64 eq = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 bb = __ballot((h >> b) & 1);
            eq &= ((h >> b) & 1) ? bb : ~bb;
        }
        if (ok) {
            const unsigned r = bow_rank(eq), nb = (unsigned)__popcll(eq);
            list[cur[w * 256 + h] + r] = (unsigned short)i;
            if (r == nb - 1) cur[w * 256 + h] += nb;                        // the bucket's last lane moves the cursor
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
}
__device__ void bow_buckets(const BowSide& s, size_t o, int n, int* cur, int* start, int* red, unsigned short* list) {
    bow_buckets_of(BowRow{s, o, n}, n, cur, start, red, list);
}

// KF = true is M8, ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (ORBmatcher.cc:955-1105, NLeft == -1): K is pKF1 (the outer
// loop), F is pKF2 (the claimed side, vbMatched2), both sides drop features without a good MapPoint (F.good), bestDist1 < TH_LOW is
// strict (:1054) and the result is indexed by idx1: the claimed-side LDS row is transposed into matches12 [npairs][K.cap] at the end
// (the output row is filled with -1 first), so no third LDS row is needed.  The fill and the scatter are global stores of different
// threads of one workgroup: what orders them is that __syncthreads() is a workgroup-scope release / acquire FENCE on global memory as well
// as a barrier (bow_buckets and the claim phase hold several).  A bare s_barrier builtin in their place would not order them.
template <bool KF>
__global__ __launch_bounds__(BOW_WAVES * 64) void k_bow_search(int npairs, BowSide K, BowSide F, const int* __restrict__ kf_row,
                                                               const int* __restrict__ f_row, float nnratio, int check_ori,
                                                               int* __restrict__ f_match, int* __restrict__ nmatches) {
    extern __shared__ int bow_lds[];
    int* cur = bow_lds;
    int* kstart = cur + BOW_WAVES * 256;
    int* fstart = kstart + 257;
    unsigned int* hist = (unsigned int*)(fstart + 257);
    int* red = (int*)(hist + 32);
    unsigned short* klist = (unsigned short*)(red + 8);
    unsigned short* flist = klist + K.cap;
    unsigned short* row = flist + F.cap;
    const int p = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int ocap = KF ? K.cap : F.cap;
    int* out = f_match + (size_t)p * ocap;
    const int kr = kf_row ? kf_row[p] : p, fr = f_row ? f_row[p] : p;
    if (KF || kr < 0 || kr >= K.nrows || fr < 0 || fr >= F.nrows) {        // (block-uniform) an empty row; M8 scatters into it below
        for (int j = tid; j < ocap; j += BOW_WAVES * 64) out[j] = -1;
        if (kr < 0 || kr >= K.nrows || fr < 0 || fr >= F.nrows) {
            if (tid == 0) nmatches[p] = 0;
            return;
        }
    }
    const size_t ko = (size_t)kr * K.cap, fo = (size_t)fr * F.cap;
    const int nk = min(max(K.counts[kr], 0), K.cap), nf = min(max(F.counts[fr], 0), F.cap);
    for (int j = tid; j < F.cap; j += BOW_WAVES * 64) row[j] = 0;
    bow_buckets(K, ko, nk, cur, kstart, red, klist);
    bow_buckets(F, fo, nf, cur, fstart, red, flist);
    const unsigned INV = 0xFFFFFFFFu;
    for (int h = w; h < 256; h += BOW_WAVES) {
        const int ks = kstart[h], ke = kstart[h + 1], fs = fstart[h], fe = fstart[h + 1];
        if (ks == ke || fs == fe) continue;
        int fj0 = -1, fn0 = 0;                                               // the first 64 frame candidates, for the whole bucket
        u64 fd0[4] = {0, 0, 0, 0};
        if (fs + lane < fe) { fj0 = flist[fs + lane]; fn0 = F.node[fo + fj0]; load_desc(F.desc + (fo + fj0) * 32, fd0); }
        for (int kb = ks; kb < ke; kb += 64) {
            int ki = -1, kn = 0;
            u64 kd[4] = {0, 0, 0, 0};
            if (kb + lane < ke) { ki = klist[kb + lane]; kn = K.node[ko + ki]; load_desc(K.desc + (ko + ki) * 32, kd); }
            const int kcnt = min(64, ke - kb);
            for (int t = 0; t < kcnt; ++t) {
                const int i = __builtin_amdgcn_readlane(ki, t), nd = __builtin_amdgcn_readlane(kn, t);
                u64 a[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = readlane64(kd[q], t);
                unsigned b1 = INV, b2 = INV;                                 // the lane's two smallest keys
                if (fj0 >= 0 && fn0 == nd && row[fj0] == 0) b1 = ((unsigned)ham256(a, fd0[0], fd0[1], fd0[2], fd0[3]) << 16) | (unsigned)lane;
                for (int fb = fs + 64; fb < fe; fb += 64) {                  // buckets longer than 64
                    const int pos = fb + lane;
                    if (pos < fe) {
                        const int j = flist[pos];
                        if (F.node[fo + j] == nd && row[j] == 0) {
                            u64 d4[4];
                            load_desc(F.desc + (fo + j) * 32, d4);
                            const unsigned key = ((unsigned)ham256(a, d4[0], d4[1], d4[2], d4[3]) << 16) | (unsigned)(pos - fs);
                            if (key < b1) { b2 = b1; b1 = key; }
                            else if (key < b2) b2 = key;
                        }
                    }
                }
                const unsigned m1 = wave_min_u32(b1);
                if (m1 == INV) continue;
                const unsigned m2 = wave_min_u32(b1 == m1 ? b2 : b1);       // the winner's lane offers its runner-up
                const int d1 = (int)(m1 >> 16), d2 = m2 == INV ? 256 : (int)(m2 >> 16);
                if ((KF ? d1 < 50 : d1 <= 50) && (float)d1 < nnratio * (float)d2) {   // TH_LOW, :436-442; strict for M8, :1054
                    if (lane == 0) row[flist[fs + (m1 & 0xFFFFu)]] = (unsigned short)(i + 1);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
    }
    __syncthreads();
    const float factor = 30 / 360.0f;                                        // HISTO_LENGTH / 360.0f, :334
    auto bin_of = [&](int j, int v) {
        float rot = K.kps[ko + v - 1].angle - F.kps[fo + j].angle;
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == 30) bin = 0;
        return bin;
    };
    if (check_ori) {
        if (tid < 32) hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < nf; j += BOW_WAVES * 64) {
            const int v = row[j];
            if (v) { const int bin = bin_of(j, v); if (bin >= 0 && bin < 30) atomicAdd(&hist[bin], 1u); }
        }
        __syncthreads();
        const Max3 m3 = three_maxima(hist);
        const int i1 = m3.i1, i2 = m3.i2, i3 = m3.i3;
        for (int j = tid; j < nf; j += BOW_WAVES * 64) {
            const int v = row[j];
            if (v) { const int bin = bin_of(j, v); if (bin >= 0 && bin < 30 && bin != i1 && bin != i2 && bin != i3) row[j] = 0; }
        }
        __syncthreads();
    }
    if (tid == 0) red[0] = 0;
    __syncthreads();
    int nm = 0;
    for (int j0 = w * 64; j0 < F.cap; j0 += BOW_WAVES * 64) {
        const int j = j0 + lane;
        const int v = j < F.cap ? (int)row[j] : 0;
        if (KF) { if (v) out[v - 1] = j; }                                   // vpMatches12[idx1] = idx2
        else if (j < F.cap) out[j] = v - 1;
        nm += __popcll(__ballot(v != 0));
    }
    if (lane == 0 && nm) atomicAdd(&red[0], nm);
    __syncthreads();
    if (tid == 0) nmatches[p] = red[0];
}

// k_bow_search_fisheye: M7 with F.Nleft != -1 (the else branch of ORBmatcher.cc:406-433 and the nested acceptance of :438-500) for a
// batch of (KF row, left frame row, right frame row) triples; k_bow_search<false> with these differences.
//  - The frame side is the COMBINED index space of BowRowPair, nl = count of the left row: one stable counting sort over [0, nl + nr)
//    leaves every hash list in ascending realIdxF, left entries before right ones, as the reference walks a bucket.  flist and the
//    claimed row hold combined indices (at most 2 * cap_f each; the caller sizes the LDS with bow_search_lds(cap_kf, 2 * cap_f)).
//  - A lane keeps the two smallest keys of its LEFT candidates (bestDist1 / bestIdxF / bestDist2) and the smallest key of its RIGHT ones
//    (bestDist1R / bestIdxFR).  bestDist2R feeds only a ratio test that `|| true` switches off (:473), so it is not computed.
//  - bestDist1 <= TH_LOW opens both claims (:438): the left slot under the ratio test, the right slot under bestDist1R <= TH_LOW alone.
//    A node without an unclaimed left candidate leaves bestDist1 at 256 and claims nothing in either camera.
//  - One histogram over both cameras' claims, rebuilt from the finished row (a slot is claimed at most once, so the row holds one
//    entry per rotHist entry); the tail splits the row into the two output rows, each padded with -1 to F.cap.
__global__ __launch_bounds__(BOW_WAVES * 64) void k_bow_search_fisheye(int npairs, BowSide K, BowSide F, const int* __restrict__ kf_row,
                                                                       const int* __restrict__ fl_row, const int* __restrict__ fr_row,
                                                                       float nnratio, int check_ori, int* __restrict__ f_match_l,
                                                                       int* __restrict__ f_match_r, int* __restrict__ nmatches) {
    extern __shared__ int bow_lds[];
    int* cur = bow_lds;
    int* kstart = cur + BOW_WAVES * 256;
    int* fstart = kstart + 257;
    unsigned int* hist = (unsigned int*)(fstart + 257);
    int* red = (int*)(hist + 32);
    unsigned short* klist = (unsigned short*)(red + 8);
    unsigned short* flist = klist + K.cap;
    unsigned short* row = flist + 2 * F.cap;
    const int p = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int* out_l = f_match_l + (size_t)p * F.cap;
    int* out_r = f_match_r + (size_t)p * F.cap;
    const int kr = kf_row ? kf_row[p] : p, fl = fl_row[p], fr = fr_row[p];
    if (kr < 0 || kr >= K.nrows || fl < 0 || fl >= F.nrows || fr < 0 || fr >= F.nrows) {   // (block-uniform) two empty rows
        for (int j = tid; j < F.cap; j += BOW_WAVES * 64) { out_l[j] = -1; out_r[j] = -1; }
        if (tid == 0) nmatches[p] = 0;
        return;
    }
    const size_t ko = (size_t)kr * K.cap;
    const int nk = min(max(K.counts[kr], 0), K.cap);
    const int nl = min(max(F.counts[fl], 0), F.cap), nr = min(max(F.counts[fr], 0), F.cap), nf = nl + nr;
    const BowRowPair FP{F, (size_t)fl * F.cap, (size_t)fr * F.cap, nl, nf};
    for (int j = tid; j < 2 * F.cap; j += BOW_WAVES * 64) row[j] = 0;
    bow_buckets(K, ko, nk, cur, kstart, red, klist);
    bow_buckets_of(FP, nf, cur, fstart, red, flist);
    const unsigned INV = 0xFFFFFFFFu;
    for (int h = w; h < 256; h += BOW_WAVES) {
        const int ks = kstart[h], ke = kstart[h + 1], fs = fstart[h], fe = fstart[h + 1];
        if (ks == ke || fs == fe) continue;
        int fj0 = -1, fn0 = 0;                                               // the first 64 frame candidates, for the whole bucket
        u64 fd0[4] = {0, 0, 0, 0};
        if (fs + lane < fe) { fj0 = flist[fs + lane]; const size_t g = FP.at(fj0); fn0 = F.node[g]; load_desc(F.desc + g * 32, fd0); }
        for (int kb = ks; kb < ke; kb += 64) {
            int ki = -1, kn = 0;
            u64 kd[4] = {0, 0, 0, 0};
            if (kb + lane < ke) { ki = klist[kb + lane]; kn = K.node[ko + ki]; load_desc(K.desc + (ko + ki) * 32, kd); }
            const int kcnt = min(64, ke - kb);
            for (int t = 0; t < kcnt; ++t) {
                const int i = __builtin_amdgcn_readlane(ki, t), nd = __builtin_amdgcn_readlane(kn, t);
                u64 a[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = readlane64(kd[q], t);
                unsigned l1 = INV, l2 = INV, r1 = INV;                       // left: the lane's two smallest keys; right: its smallest
                if (fj0 >= 0 && fn0 == nd && row[fj0] == 0) {
                    const unsigned key = ((unsigned)ham256(a, fd0[0], fd0[1], fd0[2], fd0[3]) << 16) | (unsigned)lane;
                    if (fj0 < nl) l1 = key; else r1 = key;
                }
                for (int fb = fs + 64; fb < fe; fb += 64) {                  // buckets longer than 64
                    const int pos = fb + lane;
                    if (pos < fe) {
                        const int j = flist[pos];
                        const size_t g = FP.at(j);
                        if (F.node[g] == nd && row[j] == 0) {
                            u64 d4[4];
                            load_desc(F.desc + g * 32, d4);
                            const unsigned key = ((unsigned)ham256(a, d4[0], d4[1], d4[2], d4[3]) << 16) | (unsigned)(pos - fs);
                            if (j >= nl) r1 = min(r1, key);
                            else if (key < l1) { l2 = l1; l1 = key; }
                            else if (key < l2) l2 = key;
                        }
                    }
                }
                const unsigned m1 = wave_min_u32(l1);
                if (m1 == INV || (int)(m1 >> 16) > 50) continue;             // TH_LOW on the LEFT distance gates both cameras, :438
                const unsigned m2 = wave_min_u32(l1 == m1 ? l2 : l1);       // the winner's lane offers its runner-up
                const unsigned mr = wave_min_u32(r1);
                const int d1 = (int)(m1 >> 16), d2 = m2 == INV ? 256 : (int)(m2 >> 16);
                const bool takeL = (float)d1 < nnratio * (float)d2;         // :441
                const bool takeR = mr != INV && (int)(mr >> 16) <= 50;      // :471; the ratio test of :473 is `|| true`
                if (takeL || takeR) {
                    if (lane == 0) {
                        if (takeL) row[flist[fs + (m1 & 0xFFFFu)]] = (unsigned short)(i + 1);
                        if (takeR) row[flist[fs + (mr & 0xFFFFu)]] = (unsigned short)(i + 1);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
    }
    __syncthreads();
    const float factor = 30 / 360.0f;                                        // HISTO_LENGTH / 360.0f, :334
    auto bin_of = [&](int j, int v) {                                        // :459-464 and :490-495: mvKeys / mvKeysRight by camera
        float rot = K.kps[ko + v - 1].angle - F.kps[FP.at(j)].angle;
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == 30) bin = 0;
        return bin;
    };
    if (check_ori) {
        if (tid < 32) hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < nf; j += BOW_WAVES * 64) {
            const int v = row[j];
            if (v) { const int bin = bin_of(j, v); if (bin >= 0 && bin < 30) atomicAdd(&hist[bin], 1u); }
        }
        __syncthreads();
        const Max3 m3 = three_maxima(hist);
        const int i1 = m3.i1, i2 = m3.i2, i3 = m3.i3;
        for (int j = tid; j < nf; j += BOW_WAVES * 64) {
            const int v = row[j];
            if (v) { const int bin = bin_of(j, v); if (bin >= 0 && bin < 30 && bin != i1 && bin != i2 && bin != i3) row[j] = 0; }
        }
        __syncthreads();
    }
    if (tid == 0) red[0] = 0;
    __syncthreads();
    int nm = 0;
    for (int j0 = w * 64; j0 < F.cap; j0 += BOW_WAVES * 64) {                // every output slot is written once, by this thread alone
        const int j = j0 + lane;
        const int vl = j < nl ? (int)row[j] : 0, vr = j < nr ? (int)row[nl + j] : 0;
        if (j < F.cap) { out_l[j] = vl - 1; out_r[j] = vr - 1; }
        nm += __popcll(__ballot(vl != 0)) + __popcll(__ballot(vr != 0));
    }
    if (lane == 0 && nm) atomicAdd(&red[0], nm);
    __syncthreads();
    if (tid == 0) nmatches[p] = red[0];
}

// ------------------------------------------------------------------------------------------------
// M10 SearchForTriangulation_ (ORBmatcher.cc:1388-1629; pinhole, Nleft == -1) for a batch of (pKF1 row, pKF2 row, F12, epipole) pairs:
// orbm_search_for_triangulation_batch_async.  LocalMapping::CreateNewMapPoints is one pKF1 row against 10-20 neighbour rows, each with
// its own geometry, and most features of a real KeyFrame already hold a MapPoint and are skipped on both sides (:1456-1462, :1487-1491).
//  - k_trib_buckets, one workgroup per pool-2 ROW that some pair names: the (node & 255) lists of k_tri_buckets with every per-feature
//    filter folded in -- slots >= count, stopped words, features with a MapPoint, non-stereo features under only_stereo and octaves
//    outside [0, nlevels) are not listed, so the search reads none of those arrays and never indexes the level tables out of range.
//    An entry is (idx2 | stereo2 << 16, node id): the search needs nothing else of a candidate before its descriptor.
//  - k_trib_search: LPF lanes per pKF1 feature (16: profiles/NOTES.md; one thread per feature spends its time on the chain of dependent
//    loads, and compacting the features that search at all first gained nothing) walk its bucket LPF candidates at a time; a feature
//    beyond the count, with a stopped word, with a MapPoint or, under only_stereo, without a stereo match leaves at once; the survivor is the minimum of
//    (dist << 16 | 0xFFFF - idx2) over the gate-passing candidates -- the smallest distance and, on ties, the LAST idx2, which is what
//    the reference's `dist > TH_LOW || dist > bestDist` walk keeps.  F12 and the epipole are read per pair from memory.  The output
//    rows are -1 beforehand (a memset node); only matches are written.
//  - k_trib_tail, one workgroup per pair: the orientation check (rot = angle1 - angle2, factor 1.0f / HISTO_LENGTH as written at
//    :1441, so only bins 0..12 occur; three_maxima; the other bins' matches become -1) and the count, computed from the finished row:
//    nothing accumulates across launches.
// ------------------------------------------------------------------------------------------------
struct TriSide {                                           // one pool: rows of cap slots
    const KpIn* kps; const uint8_t* desc; const int* counts; const int* node; const double* weight; const uint8_t* has_mp; const float* ur;
    int nrows, cap;
};
struct TriBatchParams { float sf2[12], sigma2[12]; int nlevels, onlyStereo, coarse, npairs; };

// does some pair name row r? (whole workgroup; rows == NULL: pair p names row p)
__device__ __forceinline__ bool trib_named(const int* __restrict__ rows, int npairs, int r) {
    if (!rows) return r < npairs;
    int hit = 0;
    for (int p = threadIdx.x; p < npairs; p += 256) hit |= rows[p] == r;
    return __syncthreads_or(hit) != 0;
}
__device__ __forceinline__ bool trib_searches(const TriSide& s, size_t o, int i, int onlyStereo) {
    return (!s.weight || s.weight[o + i] > 0) && !s.has_mp[o + i] && !(onlyStereo && !(s.ur && s.ur[o + i] >= 0));
}

__global__ __launch_bounds__(256) void k_trib_buckets(TriSide S, const int* __restrict__ row2, TriBatchParams P,
                                                      int* __restrict__ bStart, uint2* __restrict__ bEnt) {
    __shared__ int hist[257], cur[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (!trib_named(row2, P.npairs, r)) return;
    const size_t o = (size_t)r * S.cap;
    const int n = min(max(S.counts[r], 0), S.cap);
    auto listed = [&](int i) { return trib_searches(S, o, i, P.onlyStereo) && (unsigned)S.kps[o + i].octave < (unsigned)P.nlevels; };
    hist[tid] = 0; if (tid == 0) hist[256] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) if (listed(i)) atomicAdd(&hist[S.node[o + i] & 255], 1);
    __syncthreads();
    if (tid < 64) {
        int carry = 0;
        for (int b0 = 0; b0 < 256; b0 += 64) {
            const int v = hist[b0 + tid];
            int tot;
            const int ex = wave_excl_scan(v, &tot);
            hist[b0 + tid] = carry + ex;
            carry += tot;
        }
        if (tid == 0) hist[256] = carry;
    }
    __syncthreads();
    bStart[(size_t)r * 257 + tid] = hist[tid]; if (tid == 0) bStart[(size_t)r * 257 + 256] = hist[256];
    cur[tid] = hist[tid];
    __syncthreads();
    for (int i = tid; i < n; i += 256)
        if (listed(i)) {
            const int nd = S.node[o + i];
            const unsigned st = S.ur && S.ur[o + i] >= 0 ? 0x10000u : 0u;
            bEnt[o + atomicAdd(&cur[nd & 255], 1)] = make_uint2((unsigned)i | st, (unsigned)nd);
        }
}

template <int LPF>
__global__ __launch_bounds__(256) void k_trib_search(TriSide A, TriSide B, const int* __restrict__ row1, const int* __restrict__ row2,
                                                     const float* __restrict__ F12, const float* __restrict__ ep, TriBatchParams P,
                                                     const int* __restrict__ bStart, const uint2* __restrict__ bEnt,
                                                     int* __restrict__ matches12) {
    const int p = blockIdx.y;
    const int r1 = row1 ? row1[p] : p, r2 = row2 ? row2[p] : p;
    if (r1 < 0 || r1 >= A.nrows || r2 < 0 || r2 >= B.nrows) return;          // (block-uniform) the row stays -1
    const int i1 = (blockIdx.x * 256 + threadIdx.x) / LPF, sub = threadIdx.x % LPF;
    const size_t o1 = (size_t)r1 * A.cap, o2 = (size_t)r2 * B.cap;
    if (i1 >= min(A.counts[r1], A.cap) || !trib_searches(A, o1, i1, P.onlyStereo)) return;   // uniform over the LPF lanes of a feature
    const KpIn kp1 = A.kps[o1 + i1];
    const int nd = A.node[o1 + i1];
    const bool bStereo1 = A.ur && A.ur[o1 + i1] >= 0;
    u64 a[4];
    load_desc(A.desc + (o1 + i1) * 32, a);
    const float* F = F12 + (size_t)p * 9;
    const float epx = ep[2 * p], epy = ep[2 * p + 1];
    // the epipolar line of kp1 in image 2 (Pinhole::epipolarConstrain_, Pinhole.cpp:281-287)
    const float la = kp1.x * F[0] + kp1.y * F[3] + F[6];
    const float lb = kp1.x * F[1] + kp1.y * F[4] + F[7];
    const float lc = kp1.x * F[2] + kp1.y * F[5] + F[8];
    const float den = la * la + lb * lb;
    const int c0 = bStart[(size_t)r2 * 257 + (nd & 255)], c1 = bStart[(size_t)r2 * 257 + (nd & 255) + 1];
    unsigned int best = 0xFFFFFFFFu;
    for (int ci = c0 + sub; ci < c1; ci += LPF) {
        const uint2 e = bEnt[o2 + ci];
        if ((int)e.y != nd) continue;
        const int i2 = (int)(e.x & 0xFFFFu);
        u64 b[4];
        load_desc(B.desc + (o2 + i2) * 32, b);
        const int d = ham256(a, b[0], b[1], b[2], b[3]);
        if (d > 50) continue;                                                // TH_LOW, inclusive
        const KpIn kp2 = B.kps[o2 + i2];                                     // its octave is inside [0, nlevels): k_trib_buckets
        if (!bStereo1 && !(e.x >> 16)) {
            const float distex = epx - kp2.x, distey = epy - kp2.y;          // a non-finite epipole compares as IEEE does: never closer
            if (distex * distex + distey * distey < 100 * P.sf2[kp2.octave]) continue;
        }
        bool epi = false;
        if (den != 0) {
            const float num = la * kp2.x + lb * kp2.y + lc;
            const float dsqr = num * num / den;
            epi = (double)dsqr < 3.84 * (double)P.sigma2[kp2.octave];         // float compared with the double product, as written (Pinhole.cpp:295)
        }
        if (epi || P.coarse) best = min(best, ((unsigned)d << 16) | (0xFFFFu - (unsigned)i2));
    }
#pragma unroll
    for (int s = LPF >> 1; s > 0; s >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, s));
    if (sub == 0 && best != 0xFFFFFFFFu) matches12[(size_t)p * A.cap + i1] = (int)(0xFFFFu - (best & 0xFFFFu));
}

__global__ __launch_bounds__(256) void k_trib_tail(TriSide A, TriSide B, const int* __restrict__ row1, const int* __restrict__ row2,
                                                   int check_ori, int* __restrict__ matches12, int* __restrict__ nmatches) {
    __shared__ unsigned int hist[32];
    __shared__ int total;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int r1 = row1 ? row1[p] : p, r2 = row2 ? row2[p] : p;
    if (r1 < 0 || r1 >= A.nrows || r2 < 0 || r2 >= B.nrows) { if (tid == 0) nmatches[p] = 0; return; }
    const size_t o1 = (size_t)r1 * A.cap, o2 = (size_t)r2 * B.cap;
    const int n1 = min(max(A.counts[r1], 0), A.cap);
    int* row = matches12 + (size_t)p * A.cap;
    if (tid < 32) hist[tid] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    // rot_cull wants the assignments as a list of (slot | bin << 16) words, which the claim kernels keep in LDS; here the row over cap1
    // is the only record, so the histogram and the cull are two passes over it around three_maxima.  A bin outside [0, 30) (a NaN
    // angle; the reference asserts) enters no histogram bin and is never culled: the match stays and is counted, as on the host.
    const float factor = 1.0f / 30;                                          // 1.0f / HISTO_LENGTH, :1441 (sic)
    auto bin_of = [&](int i, int j) {
        float rot = A.kps[o1 + i].angle - B.kps[o2 + j].angle;
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == 30) bin = 0;
        return bin;
    };
    int mine = 0;
    if (check_ori) {
        for (int i = tid; i < n1; i += 256) {
            const int j = row[i];
            if (j >= 0) { const int bin = bin_of(i, j); if (bin >= 0 && bin < 30) atomicAdd(&hist[bin], 1u); }
        }
        __syncthreads();
        const Max3 m3 = three_maxima(hist);
        for (int i = tid; i < n1; i += 256) {
            const int j = row[i];
            if (j < 0) continue;
            const int bin = bin_of(i, j);
            if (bin >= 0 && bin < 30 && bin != m3.i1 && bin != m3.i2 && bin != m3.i3) row[i] = -1;
            else ++mine;
        }
    } else {
        for (int i = tid; i < n1; i += 256) mine += row[i] >= 0;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_xor(mine, s);
    if ((tid & 63) == 0 && mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) nmatches[p] = total;
}

// ------------------------------------------------------------------------------------------------
// k_init_search: M9 ORBmatcher::SearchForInitialization (ORBmatcher.cc:799-943) END TO END, one workgroup of INIT_WAVES waves per
// pair (a persistent grid walks the pairs when there are more pairs than workgroups).
// The claim loop is sequential in i1 -- which slots earlier queries hold, and at what distance, decides a later query's best and
// second (:853) -- but the distances are not, so the pair's queries are taken in CHUNKS of up to INIT_CHUNK consecutive i1:
// 1. candidate pass (all waves, a wave per query): the window's grid columns are flattened as in win_sweep (one column per lane, prefix
//    sum), every entry is tested (slot < n2, level, strict box) BEFORE its descriptor is fetched, and the survivors are written in grid
//    order -- the reference's visiting order -- as words dist << 21 | rotation bin << 16 | slot.  There is no cap per query: a query
//    reserves the population of its window's cells (an upper bound of its list) from the workgroup's scratch, the first query of a chunk
//    owns a region of cap2 words of its own (a list cannot be longer), and a query that finds the scratch full ends the chunk in front
//    of itself (sStop) and is searched again by the next chunk.
// 2. replay (wave 0, queries in order): the lanes share a query's list; a candidate whose slot is held at a lower-or-equal distance is
//    skipped (:853); the smallest (distance, visiting position) key is "the first of least distance", the smallest key of the others
//    (the winner's lane offers its runner-up) is bestDist2 of the if / else-if chain.  bestDist <= TH_LOW and bestDist < (float)bestDist2
//    * nnratio (INT_MAX where there is no second) accept; lane 0 writes vMatchedDistance << 16 | vnMatches21 of the slot into the LDS row
//    over cap2 -- overwriting the owner IS the steal of :876-880 -- and counts the rotation bin.  The bin counts are taken at claim time
//    and never reduced: the reference's rotHist keeps a query that was robbed later (:902 is not undone), so ComputeThreeMaxima sees it.
// 3. tail (all waves): matches12 is the transposed LDS row (filled with -1 before, scattered after); three_maxima on the claim-time
//    counts; a live entry of another bin is culled, a robbed one has no entry left to cull (:926); the survivors are counted and carry
//    the matched keypoint's position into prev_out, every other entry below the row's count carries prev_in.
// Everything is recomputed per launch: nothing accumulates across graph replays.
// LDS: the row over cap2 (4 B per slot, dynamic) + sQ [INIT_CHUNK] (offset, count) + the histogram.
// ------------------------------------------------------------------------------------------------
#define INIT_WAVES 16
#define INIT_CHUNK 1024
struct InitSide { const KpIn* kps; const uint8_t* desc; const int* counts; int nrows, cap; };
struct InitParams { float min_x, min_y, inv_w, inv_h, r, nnratio, factor; int check_ori, npairs; unsigned int budget; };

__global__ __launch_bounds__(INIT_WAVES * 64) void k_init_search(InitSide A, InitSide B, const int* __restrict__ grid_start,
                                                                const int* __restrict__ grid_idx, const int* __restrict__ row1,
                                                                const int* __restrict__ row2, const float* prev_in, float* prev_out,
                                                                InitParams P, unsigned int* scratch, int* matches12, int* __restrict__ nmatches) {
    extern __shared__ unsigned int sState[];                                 // per slot: vMatchedDistance << 16 | vnMatches21; 0xFFFF = INT_MAX / -1
    __shared__ int2 sQ[INIT_CHUNK];
    __shared__ unsigned int sHist[32];
    __shared__ int sUsed, sStop, sTotal;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NT = INIT_WAVES * 64;
    unsigned int* scr = scratch + (size_t)blockIdx.x * P.budget;
    for (int p = blockIdx.x; p < P.npairs; p += gridDim.x) {
        const int r1 = row1 ? row1[p] : p, r2 = row2 ? row2[p] : p;
        const bool ok1 = r1 >= 0 && r1 < A.nrows, ok2 = r2 >= 0 && r2 < B.nrows;
        const int n1 = ok1 ? min(max(A.counts[r1], 0), A.cap) : 0, n2 = ok2 ? min(max(B.counts[r2], 0), B.cap) : 0;
        const size_t o1 = (size_t)(ok1 ? r1 : 0) * A.cap, o2 = (size_t)(ok2 ? r2 : 0) * B.cap, op = (size_t)p * A.cap;
        int* row = matches12 + op;
        const float* pin = prev_in + 2 * op;
        float* pout = prev_out + 2 * op;
        for (int i = tid; i < A.cap; i += NT) row[i] = -1;
        for (int i = tid; i < 2 * n1; i += NT) pout[i] = pin[i];             // (in place: the same value)
        if (n1 == 0 || n2 == 0) {                                           // (workgroup-uniform)
            if (tid == 0) nmatches[p] = 0;
            continue;
        }
        for (int i = tid; i < n2; i += NT) sState[i] = 0xFFFFFFFFu;
        if (tid < 32) sHist[tid] = 0;
        if (tid == 0) sTotal = 0;
        const KpIn* kt = B.kps + o2;
        const uint8_t* dt = B.desc + o2 * 32;
        const int* gs = grid_start + (size_t)r2 * (GRID_CELLS + 1);
        const int* gi = grid_idx + o2;
        for (int c0 = 0; c0 < n1;) {
            const int cend = min(c0 + INIT_CHUNK, n1);
            __syncthreads();                                                // the row is initialised / the last chunk's replay is over
            if (tid == 0) { sUsed = n2; sStop = cend; }
            __syncthreads();
            // ---- 1. candidate pass ----
            for (int q = c0 + wave; q < cend; q += INIT_WAVES) {
                if (q >= *(volatile int*)&sStop) break;                     // the chunk already ends in front of this query
                int2 rec = make_int2(0, 0);
                const KpIn kq = A.kps[o1 + q];
                const int lvl = kq.octave;                                  // GetFeaturesInArea(x, y, r, level1, level1)
                const float x = pin[2 * q], y = pin[2 * q + 1];
                const int nMinCellX = max(0, (int)floorf((x - P.min_x - P.r) * P.inv_w));
                const int nMaxCellX = min(63, (int)ceilf((x - P.min_x + P.r) * P.inv_w));
                const int nMinCellY = max(0, (int)floorf((y - P.min_y - P.r) * P.inv_h));
                const int nMaxCellY = min(47, (int)ceilf((y - P.min_y + P.r) * P.inv_h));
                const bool window = lvl <= 0 && nMinCellX < 64 && nMaxCellX >= 0 && nMinCellY < 48 && nMaxCellY >= 0 && nMinCellX <= nMaxCellX &&
                                    nMinCellY <= nMaxCellY;                 // :825 level1 > 0 does not search
                int total = 0, excl = 0, cj0 = 0;
                const int ncols = nMaxCellX - nMinCellX + 1;
                if (window) {
                    int clen = 0;
                    if (lane < ncols) {
                        const int ix = nMinCellX + lane;
                        cj0 = min(max(gs[ix * 48 + nMinCellY], 0), n2);     // (clamped: a foreign grid must not lead outside the row)
                        clen = min(max(gs[ix * 48 + nMaxCellY + 1], cj0), n2) - cj0;
                    }
                    excl = wave_excl_scan(clen, &total);
                    total = min(total, n2);                                 // columns of a grid built over this row are disjoint: only a foreign grid is cut
                }
                bool mine = total > 0;
                unsigned int off = 0;
                if (mine && q != c0) {                                      // the chunk's first query owns [0, n2)
                    if (lane == 0) off = (unsigned)atomicAdd(&sUsed, total);
                    off = (unsigned)__builtin_amdgcn_readfirstlane((int)off);
                    if (off + (unsigned)total > P.budget) {
                        if (lane == 0) atomicMin(&sStop, q);
                        mine = false;
                    }
                }
                if (mine) {
                    const bool bCheckLevels = lvl >= 0;                     // (minLevel > 0) || (maxLevel >= 0) with both = level1 <= 0
                    u64 a[4];
                    load_desc(A.desc + (o1 + q) * 32, a);
                    const RotBinPay pay{kq.angle, P.factor};
                    int cnt = 0;
                    for (int base = 0; base < total; base += 64) {
                        const int t = base + lane;
                        int cs = 0, cb = 0;
                        for (int c = 0; c < ncols; ++c) {                   // t's column: the last one starting at or before t
                            const int e = __builtin_amdgcn_readlane(excl, c), s = __builtin_amdgcn_readlane(cj0, c);
                            if (t >= e) { cs = e; cb = s; }
                        }
                        bool ok = false;
                        unsigned int word = 0;
                        if (t < total) {
                            const int k = gi[cb + (t - cs)];
                            if ((unsigned)k < (unsigned)n2) {
                                const KpIn kp = kt[k];
                                ok = (!bCheckLevels || kp.octave == lvl) && fabsf(kp.x - x) < P.r && fabsf(kp.y - y) < P.r;
                                if (ok) {
                                    u64 b[4];
                                    load_desc(dt + (size_t)k * 32, b);
                                    word = ((unsigned)ham256(a, b[0], b[1], b[2], b[3]) << 21) | (pay(kp) << 16) | (unsigned)k;
                                }
                            }
                        }
                        const u64 bal = __ballot(ok);
                        if (ok) scr[off + cnt + bow_rank(bal)] = word;
                        cnt += __popcll(bal);
                    }
                    rec = make_int2((int)off, cnt);
                }
                if (lane == 0) sQ[q - c0] = rec;
            }
            __syncthreads();
            const int stop = sStop;                                         // > c0: the first query never waits for room
            // ---- 2. replay ----
            if (wave == 0) {
                for (int qb = c0; qb < stop; qb += 64) {
                    const int2 oc = qb + lane < stop ? sQ[qb + lane - c0] : make_int2(0, 0);
                    u64 live = __ballot(oc.y > 0);
                    while (live) {
                        const int l = __builtin_ctzll(live);
                        live &= live - 1;
                        const unsigned int off = (unsigned)__builtin_amdgcn_readlane(oc.x, l);
                        const int cnt = __builtin_amdgcn_readlane(oc.y, l), i1 = qb + l;
                        unsigned int b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu, e1 = 0;
                        for (int pos = lane; pos < cnt; pos += 64) {
                            const unsigned int e = scr[off + pos];
                            const unsigned int d = e >> 21;
                            if ((sState[e & 0xFFFFu] >> 16) <= d) continue;  // :853 vMatchedDistance[i2] <= dist
                            const unsigned int key = (d << 16) | (unsigned)pos;
                            if (key < b1) { b2 = b1; b1 = key; e1 = e; }
                            else if (key < b2) b2 = key;
                        }
                        const unsigned int m1 = wave_min_u32(b1);
                        if (m1 == 0xFFFFFFFFu) continue;                    // every candidate skipped
                        const unsigned int m2 = wave_min_u32(b1 == m1 ? b2 : b1);
                        const int bestDist = (int)(m1 >> 16), bestDist2 = m2 == 0xFFFFFFFFu ? INT_MAX : (int)(m2 >> 16);
                        if (bestDist <= 50 && (float)bestDist < (float)bestDist2 * P.nnratio) {      // :870, :873
                            const unsigned int e = (unsigned)__builtin_amdgcn_readlane((int)e1, __builtin_ctzll(__ballot(b1 == m1)));
                            const unsigned int bin = (e >> 16) & 31u;
                            if (lane == 0) {
                                sState[e & 0xFFFFu] = ((unsigned)bestDist << 16) | (unsigned)i1;
                                if (P.check_ori && bin < 30u) sHist[bin] += 1;
                            }
                        }
                    }
                }
            }
            c0 = stop;
        }
        __syncthreads();
        // ---- 3. tail ----
        const Max3 m3 = three_maxima(sHist);
        int kept = 0;
        for (int k = tid; k < n2; k += NT) {
            const unsigned int i1 = sState[k] & 0xFFFFu;
            if (i1 == 0xFFFFu) continue;
            const KpIn kp2 = kt[k];
            if (P.check_ori) {
                const int bin = (int)RotBinPay{A.kps[o1 + i1].angle, P.factor}(kp2);
                if (bin < 30 && bin != m3.i1 && bin != m3.i2 && bin != m3.i3) continue;   // culled (:926-930)
            }
            row[i1] = k;
            pout[2 * i1] = kp2.x; pout[2 * i1 + 1] = kp2.y;                  // :938-940
            ++kept;
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) kept += __shfl_xor(kept, s);
        if (lane == 0 && kept) atomicAdd(&sTotal, kept);
        __syncthreads();
        if (tid == 0) nmatches[p] = sTotal;
        __syncthreads();                                                    // sTotal and the row are reused by the next pair
    }
}

// ------------------------------------------------------------------------------------------------
// k_undistort: Frame::UndistortKeyPoints (Frame.cc:924-970) = cv::undistortPoints(K, D, R = I, P = newK), one thread per
// keypoint, double arithmetic in OpenCV's operation order (5 fixed-point iterations; compiled without contraction).
// ------------------------------------------------------------------------------------------------
struct UndistParams { double k[14]; double fx, fy, cx, cy, nfx, nfy, ncx, ncy; };

__device__ __forceinline__ void undistort_point(const UndistParams& P, double u, double v, float* ox, float* oy) {
    const double ifx = 1.0 / P.fx, ify = 1.0 / P.fy;
    double x = (u - P.cx) * ifx, y = (v - P.cy) * ify;
    const double x0 = x, y0 = y;
    const double* k = P.k;
    for (int j = 0; j < 5; ++j) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0) { x = (u - P.cx) * ifx; y = (v - P.cy) * ify; break; }
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = P.nfx * x + 0.0 * y + P.ncx, yy = 0.0 * x + P.nfy * y + P.ncy, ww = 1.0 / (0.0 * x + 0.0 * y + 1.0);
    *ox = (float)(xx * ww); *oy = (float)(yy * ww);
}

__global__ __launch_bounds__(256) void k_undistort(const KpIn* __restrict__ in, int n, UndistParams P, int passthrough,
                                                   KpIn* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    KpIn kp = in[i];
    if (!passthrough) undistort_point(P, (double)kp.x, (double)kp.y, &kp.x, &kp.y);
    out[i] = kp;
}

// ------------------------------------------------------------------------------------------------
// k_frustum: Frame::isInFrustum (Nleft == -1, Frame.cc:603-671) + MapPoint::PredictScale (MapPoint.cc:725-740), one
// thread per map point.  Float expressions in the reference's order (Matx products accumulate from 0 in float, cv::norm
// accumulates in double); log(ratio) is evaluated in double and rounded to float (the host libm's logf is within 1 ulp of
// that; the predicted level can differ only when log(ratio)/logScaleFactor is within an ulp of an integer).  The per-point body is
// frustum_point, shared with k_frustum_batch: both forms give the same bits.
// ------------------------------------------------------------------------------------------------
struct FrustumParams { float rcw[9], tcw[3], ow[3], k[4], bounds[4], bf, cosLimit, logSF; int nLevels; };

// One map point: reads entry q of the MapPoint rows, writes entry o of the seven output rows; true where the point is in view.
__device__ __forceinline__ bool frustum_point(const FrustumParams& F, const float* __restrict__ pw, const float* __restrict__ normal,
                                              const float* __restrict__ minDist, const float* __restrict__ maxDist, size_t q, size_t o,
                                              uint8_t* inView, float* projX, float* projY, float* projXR, float* depth, int* level,
                                              float* viewCos) {
    inView[o] = 0; projX[o] = -1.f; projY[o] = -1.f;
    const float P0 = pw[3 * q], P1 = pw[3 * q + 1], P2 = pw[3 * q + 2];
    float Pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float s = 0.f;
        s += F.rcw[3 * r] * P0; s += F.rcw[3 * r + 1] * P1; s += F.rcw[3 * r + 2] * P2;
        Pc[r] = s + F.tcw[r];
    }
    double n2 = 0.0;
    n2 += (double)Pc[0] * (double)Pc[0]; n2 += (double)Pc[1] * (double)Pc[1]; n2 += (double)Pc[2] * (double)Pc[2];
    const float PcDist = (float)sqrt(n2);
    const float PcZ = Pc[2];
    const float invz = 1.0f / PcZ;
    if (PcZ < 0.0f) return false;
    const float u = F.k[0] * Pc[0] / Pc[2] + F.k[2], v = F.k[1] * Pc[1] / Pc[2] + F.k[3];
    if (u < F.bounds[0] || u > F.bounds[1]) return false;
    if (v < F.bounds[2] || v > F.bounds[3]) return false;
    projX[o] = u; projY[o] = v;
    const float maxD = 1.2f * maxDist[q], minD = 0.8f * minDist[q];
    const float O0 = P0 - F.ow[0], O1 = P1 - F.ow[1], O2 = P2 - F.ow[2];
    double d2 = 0.0;
    d2 += (double)O0 * (double)O0; d2 += (double)O1 * (double)O1; d2 += (double)O2 * (double)O2;
    const float dist = (float)sqrt(d2);
    if (dist < minD || dist > maxD) return false;
    float dot = 0.f;
    dot += O0 * normal[3 * q]; dot += O1 * normal[3 * q + 1]; dot += O2 * normal[3 * q + 2];
    const float vc = dot / dist;
    if (vc < F.cosLimit) return false;
    const float ratio = maxDist[q] / dist;
    const float lg = (float)log((double)ratio);
    int ns = (int)ceilf(lg / F.logSF);
    if (ns < 0) ns = 0; else if (ns >= F.nLevels) ns = F.nLevels - 1;
    inView[o] = 1; projXR[o] = u - F.bf * invz; depth[o] = PcDist; level[o] = ns; viewCos[o] = vc;
    return true;
}

__global__ __launch_bounds__(256) void k_frustum(int n, const float* __restrict__ pw, const float* __restrict__ normal,
                                                 const float* __restrict__ minDist, const float* __restrict__ maxDist, FrustumParams F,
                                                 uint8_t* inView, float* projX, float* projY, float* projXR, float* depth, int* level,
                                                 float* viewCos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    frustum_point(F, pw, normal, minDist, maxDist, (size_t)i, (size_t)i, inView, projX, projY, projXR, depth, level, viewCos);
}

// k_frustum_batch: frustum_point for every (frame, point) of a batch in one launch, grid = (point blocks, frames).  Frame f's pose comes
// from device rows -- tcw [nframes][12] row-major 3x4 [Rcw | tcw], ow [nframes][3]; f is blockIdx.y, so the fifteen loads are uniform --
// and its count from nq[f], clamped to [0, qStride]: a replayed graph follows the rows.  C carries k, bounds, bf, cosLimit, logSF and
// nLevels; its pose fields are not read.  The MapPoint rows are [nframes][qStride], or one row for all frames when qShared.  Entry i of
// row f: i >= n or skip[f][i] != 0 -> inView = 0 and nothing else written; otherwise exactly what k_frustum writes.  nInView[f] (NULL =
// not counted) += the popcount of each wave's in-view ballot: an integer sum into a row the caller's memset zeroes ahead of the launch
// in the same stream, so it is exact, independent of the order and the same on every replay.  No LDS; every lane reaches the ballot.
__global__ __launch_bounds__(256) void k_frustum_batch(const float* __restrict__ tcw, const float* __restrict__ ow, const int* __restrict__ nq,
                                                       int qStride, const uint8_t* __restrict__ skip, const float* __restrict__ pw,
                                                       const float* __restrict__ normal, const float* __restrict__ minDist,
                                                       const float* __restrict__ maxDist, int qShared, FrustumParams C, uint8_t* inView,
                                                       float* projX, float* projY, float* projXR, float* depth, int* level, float* viewCos,
                                                       int* nInView) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(max(nq[f], 0), qStride);
    FrustumParams F = C;
    const float* T = tcw + 12 * (size_t)f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        F.rcw[3 * r] = T[4 * r]; F.rcw[3 * r + 1] = T[4 * r + 1]; F.rcw[3 * r + 2] = T[4 * r + 2]; F.tcw[r] = T[4 * r + 3];
        F.ow[r] = ow[3 * (size_t)f + r];
    }
    const size_t o = (size_t)f * qStride + i, q = qShared ? (size_t)i : o;
    bool iv = false;
    if (i < qStride) {
        if (i >= n || (skip && skip[o])) inView[o] = 0;
        else iv = frustum_point(F, pw, normal, minDist, maxDist, q, o, inView, projX, projY, projXR, depth, level, viewCos);
    }
    const u64 bal = __ballot(iv);
    if (nInView && bal && (threadIdx.x & 63) == 0) atomicAdd(&nInView[f], __popcll(bal));
}

// ------------------------------------------------------------------------------------------------
// RGB-D frames.  k_rgbd_stereo: Frame::ComputeStereoFromRGBD (Frame.cc:1279-1309) with GrabImageRGBD's convertTo
// (Tracking.cc:1353-1354) folded into the sample: only the pixels under keypoints are read, and converting one pixel gives what
// converting the image gives.  One workgroup per frame of the call strides over the row's `cap` slots, so that the count of valid
// depths is a reduction over the finished row (ballot + popcount per wave, LDS across the waves, one plain store): nothing
// accumulates across graph replays and nothing has to be cleared.
//   pixel   row = (int)kp.y, col = (int)kp.x of the RAW keypoint (the truncation of Mat::at<float>(float, float)); a coordinate whose
//           truncation lies outside the image, or a NaN, reads nothing and gives -1 / -1 (the reference reads out of bounds there)
//   d       scale ? (float)raw * factor : raw  -- one float32 multiply (convertTo's alpha in float, beta == 0)
//   d > 0   depth = d, uright = kpU.x - mbf / d (IEEE float division, float subtraction); else -1 / -1 (0, negatives, NaN)
// Slots at or beyond the frame's count get -1 / -1 too.
// ------------------------------------------------------------------------------------------------
struct RgbdParams { int first, cap, w, h, stride_bytes, f32, scale; float factor, mbf; };

__global__ __launch_bounds__(256) void k_rgbd_stereo(const KpIn* __restrict__ kps, const KpIn* __restrict__ kps_un, const int* __restrict__ counts,
                                                     const void* const* __restrict__ depth_imgs, RgbdParams P,
                                                     float* __restrict__ uright, float* __restrict__ depth, int* __restrict__ nvalid) {
    __shared__ int sCnt[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const size_t in0 = (size_t)(P.first + f) * P.cap, out0 = (size_t)f * P.cap;
    const int n = min(max(counts[P.first + f], 0), P.cap);
    const uint8_t* img = (const uint8_t*)depth_imgs[f];
    const float fw = (float)P.w, fh = (float)P.h;
    int cnt = 0;
    for (int base = 0; base < P.cap; base += 256) {                          // uniform trip count: every lane reaches the ballot
        const int i = base + tid;
        float ur = -1.0f, dp = -1.0f;
        if (i < n) {
            const float x = kps[in0 + i].x, y = kps[in0 + i].y;
            if (x > -1.0f && x < fw && y > -1.0f && y < fh) {                // (int) truncates towards zero: (-1, 0) reads index 0; NaN fails
                const uint8_t* p = img + (size_t)(int)y * P.stride_bytes;
                const float raw = P.f32 ? ((const float*)p)[(int)x] : (float)((const uint16_t*)p)[(int)x];
                const float d = P.scale ? raw * P.factor : raw;
                if (d > 0) { dp = d; ur = kps_un[in0 + i].x - P.mbf / d; }
            }
        }
        if (i < P.cap) { uright[out0 + i] = ur; depth[out0 + i] = dp; }
        cnt += __popcll(__ballot(dp > 0));                                   // wave-uniform: -1 marks every slot without depth
    }
    if ((tid & 63) == 0) sCnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) nvalid[f] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
}

// k_unproject_stereo: Frame::UnprojectStereo (Frame.cc:1312-1326) for every slot of every row.  z = depth > 0: x = (u - cx) * z * invfx
// and y likewise, left to right in float; x3Dw = mRwc * x3Dc + mOw by the cv::Mat product rule (double sum rounded once to float, then
// a float add: mm_dot3, as k_mm_project) -- not the Matx rule of k_frustum.  Any other slot, and slots at or beyond the count, get
// has_depth = 0 and (0, 0, 0).  twc: [nrows][12] row-major 3x4 [Rwc | Ow].
struct UnprojParams { int first, cap; float cx, cy, invfx, invfy; };

__global__ __launch_bounds__(256) void k_unproject_stereo(const KpIn* __restrict__ kps_un, const int* __restrict__ counts, const float* __restrict__ depth,
                                                          const float* __restrict__ twc, UnprojParams P, float* __restrict__ x3dw,
                                                          uint8_t* __restrict__ has_depth) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.cap) return;
    const size_t o = (size_t)r * P.cap + i;
    const int n = min(max(counts[P.first + r], 0), P.cap);
    float X = 0.f, Y = 0.f, Z = 0.f;
    uint8_t ok = 0;
    if (i < n) {
        const float z = depth[o];
        if (z > 0) {
            const KpIn& kp = kps_un[(size_t)(P.first + r) * P.cap + i];
            const float x = (kp.x - P.cx) * z * P.invfx;
            const float y = (kp.y - P.cy) * z * P.invfy;
            const float* T = twc + (size_t)r * 12;
            X = mm_dot3(T[0], T[1], T[2], x, y, z) + T[3];
            Y = mm_dot3(T[4], T[5], T[6], x, y, z) + T[7];
            Z = mm_dot3(T[8], T[9], T[10], x, y, z) + T[11];
            ok = 1;
        }
    }
    x3dw[o * 3] = X; x3dw[o * 3 + 1] = Y; x3dw[o * 3 + 2] = Z;
    has_depth[o] = ok;
}

// ------------------------------------------------------------------------------------------------
// k_depth_select: the sorted walk over a frame's depth points that Tracking::UpdateLastFrame (Tracking.cc:3094-3163) and
// Tracking::CreateNewKeyFrame (:3694-3783) run, and NeedNewKeyFrame's close counts (:3524-3546).  One workgroup per row of the call.
//   keys    one 64-bit key per slot i < n with depth > 0: (depth bits) << 32 | i.  Positive IEEE floats, +inf included, order as their
//           bit patterns, and the slot in the low word breaks ties, so an ascending sort of the keys IS std::sort of pair<float,int>.
//           Depth tests run on the bits (zbits - 1 < 0x7F800000 is z > 0 without NaN; the thresholds arrive as bit patterns from
//           the host, DepthSelParams): no compare that could flush a denormal.  The row is padded to n2 = a power of two with all-ones
//           keys, which no point can equal (a NaN pattern in the high word).
//   sort    bitonic network in LDS over n2 keys (n2 * 8 B of dynamic LDS: sized from the padded cap).  One thread per PAIR
//           (i, i | j) with i = 2p - (p & (j - 1)), so every lane of every step works.  For j >= 32 the 32 lanes of a ds_read_b64
//           group read 32 consecutive keys = 64 banks: conflict-free.  For j < 32 the group's pairs span 64 keys and both reads go
//           2-way; those are the last five steps of each stage.  Steps with j > 64 end in a workgroup barrier; the steps with j <= 64
//           stay inside the 128 keys one wave owns and run back to back under a wave barrier (56 of the 66 steps at 2048 keys).
//   bound   c = points with !(depth > th) (ballot + popcount while the keys are built), nd = |D|;
//           nvisit = min(nd, max(c, max_points) + 1): the walk stops AFTER visiting the first far point past max_points.
//   output  order[j] = slot at position j < nvisit, -1 beyond.  A slot was visited iff its key <= the key at position nvisit - 1
//           (keys are unique), so create_new and the counts are one pass over the slots, every value written once from the finished
//           row with plain stores: nothing accumulates across graph replays.
// ------------------------------------------------------------------------------------------------
struct DepthSelParams { int first, cap, n2, max_points; unsigned int far_above, close_below; };

__global__ __launch_bounds__(1024) void k_depth_select(const int* __restrict__ counts, const float* __restrict__ depth,
                                                       const uint8_t* __restrict__ keeps_mp, const uint8_t* __restrict__ tracked,
                                                       DepthSelParams P, int* __restrict__ order, uint8_t* __restrict__ create_new,
                                                       int* __restrict__ nvisit, int* __restrict__ ncreate,
                                                       int* __restrict__ nclose_tracked, int* __restrict__ nclose_untracked) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long dsel_keys[];
    __shared__ int sA[16], sB[16], sC[16];
    const int r = blockIdx.x, tid = threadIdx.x, T = blockDim.x, wave = tid >> 6, nwaves = T >> 6;
    const size_t o0 = (size_t)r * P.cap;
    const int n = min(max(counts[P.first + r], 0), P.cap);
    const unsigned int* zb = (const unsigned int*)depth + o0;
    int cntD = 0, cntC = 0;
    for (int base = 0; base < P.n2; base += T) {                             // uniform trip count: every lane reaches the ballots
        const int i = base + tid;
        unsigned long long key = ~0ull;
        bool has = false, nr = false;
        if (i < n) {
            const unsigned int z = zb[i];
            has = z - 1u < 0x7F800000u;                                      // z > 0: not 0, not negative, not NaN; +inf and denormals pass
            nr = has && !(z > P.far_above);
            if (has) key = ((unsigned long long)z << 32) | (unsigned)i;
        }
        if (i < P.n2) dsel_keys[i] = key;
        cntD += __popcll(__ballot(has)); cntC += __popcll(__ballot(nr));
    }
    if ((tid & 63) == 0) { sA[wave] = cntD; sB[wave] = cntC; }
    __syncthreads();
    const int half = P.n2 >> 1;
    for (int k = 2; k <= P.n2; k <<= 1) {
        int j = k >> 1;
        for (; j > 64; j >>= 1) {                                            // steps that cross waves: a workgroup barrier each
            for (int p = tid; p < half; p += T) {
                const int i = 2 * p - (p & (j - 1)), q = i | j;
                const unsigned long long a = dsel_keys[i], b = dsel_keys[q];
                if ((a > b) == ((i & k) == 0)) { dsel_keys[i] = b; dsel_keys[q] = a; }
            }
            __syncthreads();
        }
        // j <= 64: the 64 pairs [64 w, 64 w + 64) of a wave are exactly the keys [128 w, 128 w + 128) at every remaining step, so the
        // rest of the stage runs back to back on the wave's own keys (LDS accesses of one wave complete in order)
        for (int p0 = tid & ~63; p0 < half; p0 += T) {                       // wave-uniform trip count
            const int p = p0 + (tid & 63);
            for (int jj = j; jj > 0; jj >>= 1) {
                if (p < half) {
                    const int i = 2 * p - (p & (jj - 1)), q = i | jj;
                    const unsigned long long a = dsel_keys[i], b = dsel_keys[q];
                    if ((a > b) == ((i & k) == 0)) { dsel_keys[i] = b; dsel_keys[q] = a; }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
    int nd = 0, c = 0;
    for (int w = 0; w < nwaves; ++w) { nd += sA[w]; c += sB[w]; }
    const int nv = min(nd, max(c, min(P.max_points, nd)) + 1);
    const unsigned long long kmax = nv > 0 ? dsel_keys[nv - 1] : 0ull;       // no key is 0: depth bits are >= 1
    int* ord = order + o0;
    for (int j = tid; j < P.cap; j += T) ord[j] = j < nv ? (int)(unsigned)dsel_keys[j] : -1;
    int cntN = 0, cntT = 0, cntU = 0;
    for (int base = 0; base < P.cap; base += T) {
        const int i = base + tid;
        bool cn = false, ct = false, cu = false;
        if (i < n) {
            const unsigned int z = zb[i];
            const bool has = z - 1u < 0x7F800000u;
            const unsigned long long key = ((unsigned long long)z << 32) | (unsigned)i;
            cn = has && key <= kmax && !(keeps_mp && keeps_mp[o0 + i]);
            const bool close = has && z < P.close_below;                    // depth > 0 && depth < th (Tracking.cc:3533)
            const bool trk = tracked && tracked[o0 + i];
            ct = close && trk; cu = close && !trk;
        }
        if (i < P.cap) create_new[o0 + i] = cn ? 1 : 0;
        cntN += __popcll(__ballot(cn)); cntT += __popcll(__ballot(ct)); cntU += __popcll(__ballot(cu));
    }
    __syncthreads();                                                         // sA / sB have been read by every thread
    if ((tid & 63) == 0) { sA[wave] = cntN; sB[wave] = cntT; sC[wave] = cntU; }
    __syncthreads();
    if (tid == 0) {
        int a = 0, b = 0, u = 0;
        for (int w = 0; w < nwaves; ++w) { a += sA[w]; b += sB[w]; u += sC[w]; }
        nvisit[r] = nv; ncreate[r] = a;
        if (nclose_tracked) nclose_tracked[r] = b;
        if (nclose_untracked) nclose_untracked[r] = u;
    }
}

// k_adopt_new_points: `new MapPoint(x3D, pMap, &mLastFrame, i)` (Tracking.cc:3139-3143) as far as M4 reads it, thread per slot.  Where
// create_new is set: x3dw = x3d_new, has_mp = !outlier (M4 tests pMP && !mvbOutlier[i], ORBmatcher.cc:2505-2509), mp_obs = 0 (nObs(0),
// MapPoint.cc:92), qdesc = the frame's descriptor row of that slot (MapPoint.cc:127).  Every other slot is untouched.
__global__ __launch_bounds__(256) void k_adopt_new_points(const int* __restrict__ counts, int first, int cap, const uint8_t* __restrict__ create_new,
                                                          const float* __restrict__ x3d_new, const uint8_t* __restrict__ desc,
                                                          const uint8_t* __restrict__ outlier, float* __restrict__ x3dw,
                                                          uint8_t* __restrict__ has_mp, uint8_t* __restrict__ mp_obs, uint8_t* __restrict__ qdesc) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(max(counts[first + r], 0), cap)) return;
    const size_t o = (size_t)r * cap + i;
    if (!create_new[o]) return;
    x3dw[o * 3] = x3d_new[o * 3]; x3dw[o * 3 + 1] = x3d_new[o * 3 + 1]; x3dw[o * 3 + 2] = x3d_new[o * 3 + 2];
    has_mp[o] = outlier ? (outlier[o] ? 0 : 1) : 1;
    mp_obs[o] = 0;
    const uint32_t* s = (const uint32_t*)(desc + ((size_t)(first + r) * cap + i) * 32);
    uint32_t* d = (uint32_t*)(qdesc + o * 32);
    for (int w = 0; w < 8; ++w) d[w] = s[w];
}

// ------------------------------------------------------------------------------------------------
// MapPoint refresh: the producer of the qdesc / normal / min_dist / max_dist rows the batched searches read.
// k_mp_distinctive: MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:450-538); k_mp_normal_depth: MapPoint::UpdateNormalAndDepth
// (MapPoint.cc:578-652).  Both walk a CSR of observation entries (KeyFrame pool row, slot, flags) over the MapPoints of the call.
// An entry is skipped when its row lies outside [0, nkf_rows) or its slot outside [0, min(counts_kf[row], cap)); a list is empty when
// its offset pair does not increase, leaves [0, nobs] or is longer than MP_MAX_OBS entries: nothing is read out of bounds.
// ------------------------------------------------------------------------------------------------
#define MP_MAX_OBS 65535                                                    // the winner key holds the entry's position in 16 bits
struct MpObs { const int* off; const int* row; const int* slot; const uint8_t* flags; const uint8_t* valid; int nobs, nmp, nkf_rows, cap; };

// the entry list of MapPoint mp: [o0, o0 + return value)
__device__ __forceinline__ int mp_obs_range(const MpObs& O, int mp, int& o0) {
    o0 = 0;
    if (O.valid && !O.valid[mp]) return 0;
    const int a = O.off[mp], b = O.off[mp + 1];
    if (a < 0 || b > O.nobs || b <= a || b - a > MP_MAX_OBS) return 0;
    o0 = a;
    return b - a;
}
// the pool slot (row * cap + slot) entry e of the arrays names, or -1 when the entry is skipped
__device__ __forceinline__ long long mp_obs_slot(const MpObs& O, const int* __restrict__ counts_kf, int e) {
    const int r = O.row[e], s = O.slot[e];
    if ((unsigned)r >= (unsigned)O.nkf_rows) return -1;
    if (s < 0 || s >= min(counts_kf[r], O.cap)) return -1;
    return (long long)r * O.cap + s;
}

// k_mp_distinctive: ONE wave per MapPoint, four MapPoints per workgroup; a list of more than 64 entries is shared by the workgroup's
// four waves.  Lane i holds the descriptor of entry i in eight registers;
// entries of a bad KeyFrame (flag bit 1, :477) and skipped entries are masked out of the rows and out of the columns, so that N is the
// number of live entries and the position reported is the entry's position in the MapPoint's own list.  Column j reaches every lane by
// v_readlane (no memory traffic inside the N x N table).  The median of row i -- element (int)(0.5 * (N - 1)) = (N - 1) >> 1 of the
// sorted row, the 0 to itself included (:518-521) -- is the least v with count(d <= v) >= k + 1:
//   E <= 64   the row's distances go to LDS once (16 bits: 256 is a legal distance) and nine bisection steps over 0..256 count them;
//   E  > 64   the waves walk the rows in chunks of 64 (wave w: chunks w, w + 4, ...) and the columns in chunks of 64; per row chunk two sweeps recompute the
//             distances into a per-lane histogram in LDS: 17 bins of d >> 4 find the bin of the k-th, 16 bins of d & 15 inside it
//             find the value (counts fit 16 bits: N <= 65535).
// The winner is one wave_min_u32 over median << 16 | position (and, for a shared list, one LDS atomic minimum per wave): the FIRST row of least median (strict <, :524).  N == 0 (an empty list,
// every entry skipped, a MapPoint that is not valid) writes best_obs = best_median = -1 and leaves mp_desc alone.
__device__ __forceinline__ bool mpd_load(const MpObs& O, const int* __restrict__ counts_kf, const uint8_t* __restrict__ desc_kf, int o0, int E, int e,
                                         unsigned (&a)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = 0;
    if (e >= E || (O.flags[o0 + e] & 2)) return false;
    const long long p = mp_obs_slot(O, counts_kf, o0 + e);
    if (p < 0) return false;
    const uint4* q = (const uint4*)(desc_kf + p * 32);
    const uint4 x = q[0], y = q[1];
    a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w; a[4] = y.x; a[5] = y.y; a[6] = y.z; a[7] = y.w;
    return true;
}
// distance of the lane's descriptor a to lane j's descriptor b (j wave-uniform)
__device__ __forceinline__ unsigned mpd_dist(const unsigned (&a)[8], const unsigned (&b)[8], int j) {
    unsigned d = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) d = bcnt_acc(a[t] ^ (unsigned)__builtin_amdgcn_readlane((int)b[t], j), d);
    return d;
}

// the outputs of one MapPoint from the reduced key median << 16 | position (all ones: no live entry)
__device__ __forceinline__ void mpd_write(const MpObs& O, const int* __restrict__ counts_kf, const uint8_t* __restrict__ desc_kf, int mp, int o0,
                                          unsigned best, int lane, uint8_t* __restrict__ mp_desc, int* __restrict__ best_obs,
                                          int* __restrict__ best_median) {
    if (best == 0xFFFFFFFFu) {
        if (lane == 0) { best_obs[mp] = -1; if (best_median) best_median[mp] = -1; }
        return;
    }
    const int win = (int)(best & 0xFFFFu);
    if (lane < 8) {                                                         // the winner's 32 bytes, one dword per lane
        const long long p = mp_obs_slot(O, counts_kf, o0 + win);
        ((unsigned*)(mp_desc + (size_t)mp * 32))[lane] = ((const unsigned*)(desc_kf + p * 32))[lane];
    }
    if (lane == 0) { best_obs[mp] = win; if (best_median) best_median[mp] = (int)(best >> 16); }
}

// the workgroup's work: phase 1, every wave takes its own MapPoint when the list has at most 64 entries (no barrier); phase 2, the four
// waves share the row chunks of each longer list of the workgroup (wave w takes rows 64 w, 64 w + 256, ...) and meet in one LDS word.
// The tests around the barriers read the same global words in every thread, so they are uniform over the workgroup.
// SKIP_UPTO > 0 (A/B build only) leaves lists of at most that many entries to the packed kernel.
template <int SKIP_UPTO>
__device__ __forceinline__ void mp_distinctive_block(const uint8_t* __restrict__ desc_kf, const int* __restrict__ counts_kf, const MpObs& O,
                                                     uint8_t* __restrict__ mp_desc, int* __restrict__ best_obs, int* __restrict__ best_median,
                                                     unsigned short (&sD)[4][64][64], unsigned& sBest) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mp0 = blockIdx.x * 4;
    unsigned a[8], b[8];
    if (mp0 + wv < O.nmp) {                                                 // phase 1
        const int mp = mp0 + wv;
        int o0;
        const int E = mp_obs_range(O, mp, o0);
        if (E <= 64 && !(SKIP_UPTO > 0 && E <= SKIP_UPTO)) {
            unsigned best = 0xFFFFFFFFu;
            const bool ok = mpd_load(O, counts_kf, desc_kf, o0, E, lane, a);
            const u64 mask = __ballot(ok);
            if (mask) {
                const int k = (__popcll(mask) - 1) >> 1;
                for (u64 m = mask; m; m &= m - 1) {
                    const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
                    sD[wv][j][lane] = (unsigned short)mpd_dist(a, a, j);
                }
                int lo = 0, hi = 256;                                       // the answer stays in [lo, hi]: count(d <= 256) = N > k
                for (int it = 0; it < 9; ++it) {
                    const int mid = (lo + hi) >> 1;
                    int cnt = 0;
                    for (u64 m = mask; m; m &= m - 1) cnt += sD[wv][__builtin_amdgcn_readfirstlane(__builtin_ctzll(m))][lane] <= mid;
                    if (cnt > k) hi = mid; else lo = mid + 1;
                }
                best = wave_min_u32(ok ? ((unsigned)lo << 16 | (unsigned)lane) : 0xFFFFFFFFu);
            }
            mpd_write(O, counts_kf, desc_kf, mp, o0, best, lane, mp_desc, best_obs, best_median);
        }
    }
    for (int q = 0; q < 4; ++q) {                                           // phase 2
        const int mp = mp0 + q;
        if (mp >= O.nmp) break;
        int o0;
        const int E = mp_obs_range(O, mp, o0);
        if (E <= 64) continue;
        if (threadIdx.x == 0) sBest = 0xFFFFFFFFu;
        __syncthreads();
        int N = 0;
        for (int jb = 0; jb < E; jb += 64) {
            const int e = jb + lane;
            N += __popcll(__ballot(e < E && !(O.flags[o0 + e] & 2) && mp_obs_slot(O, counts_kf, o0 + e) >= 0));
        }
        const int k = (N - 1) >> 1;
        unsigned best = 0xFFFFFFFFu;
        for (int ib = wv * 64; ib < E && N > 0; ib += 256) {
            const bool okA = mpd_load(O, counts_kf, desc_kf, o0, E, ib + lane, a);
            if (!__ballot(okA)) continue;
            for (int c = 0; c < 33; ++c) sD[wv][c][lane] = 0;
            for (int jb = 0; jb < E; jb += 64) {                            // sweep 1: bins of d >> 4 (0..16)
                const u64 mB = __ballot(mpd_load(O, counts_kf, desc_kf, o0, E, jb + lane, b));
                for (u64 m = mB; m; m &= m - 1) {
                    const unsigned d = mpd_dist(a, b, __builtin_amdgcn_readfirstlane(__builtin_ctzll(m)));
                    sD[wv][d >> 4][lane] += 1;
                }
            }
            int cum = 0, bin = 16, kk = k;
            bool found = false;
            for (int c = 0; c < 17; ++c) {                                  // the lowest bin whose running count passes k
                const int h = sD[wv][c][lane];
                if (!found && cum + h > k) { bin = c; kk = k - cum; found = true; }
                cum += h;
            }
            for (int jb = 0; jb < E; jb += 64) {                            // sweep 2: bins of d & 15 inside that bin
                const u64 mB = __ballot(mpd_load(O, counts_kf, desc_kf, o0, E, jb + lane, b));
                for (u64 m = mB; m; m &= m - 1) {
                    const unsigned d = mpd_dist(a, b, __builtin_amdgcn_readfirstlane(__builtin_ctzll(m)));
                    if ((int)(d >> 4) == bin) sD[wv][17 + (d & 15)][lane] += 1;
                }
            }
            int fine = 15;
            cum = 0; found = false;
            for (int t = 0; t < 16; ++t) {
                const int h = sD[wv][17 + t][lane];
                if (!found && cum + h > kk) { fine = t; found = true; }
                cum += h;
            }
            const unsigned med = (unsigned)(bin * 16 + fine);
            best = min(best, wave_min_u32(okA ? (med << 16 | (unsigned)(ib + lane)) : 0xFFFFFFFFu));
        }
        if (lane == 0 && best != 0xFFFFFFFFu) atomicMin(&sBest, best);
        __syncthreads();
        if (wv == 0) mpd_write(O, counts_kf, desc_kf, mp, o0, sBest, lane, mp_desc, best_obs, best_median);
        __syncthreads();                                                    // the word is free for the next long list
    }
}

__global__ __launch_bounds__(256) void k_mp_distinctive(const uint8_t* __restrict__ desc_kf, const int* __restrict__ counts_kf, MpObs O,
                                                        uint8_t* __restrict__ mp_desc, int* __restrict__ best_obs, int* __restrict__ best_median) {
    __shared__ __attribute__((aligned(16))) unsigned short sD[4][64][64];   // [wave][column j | histogram bin][lane]: a lane reads what it wrote
    // the meeting word of phase 2 lives in wave 0's last column: thread 0 writes it after its own phase 1, and phase 2 uses bins 0..32 only
    mp_distinctive_block<0>(desc_kf, counts_kf, O, mp_desc, best_obs, best_median, sD, reinterpret_cast<unsigned&>(sD[0][63][0]));
}

#ifdef ORBX_AB   /* A/B: several MapPoints per wave in groups of G lanes (ORBM_MP_PACKED = 8 | 16 | 32), not in the product library */
// k_mp_distinctive_packed<G>: a group of G lanes takes one MapPoint whose list has at most G entries; lane l holds entry l, column j
// reaches the group by ds_bpermute, the G distances of a row stay in registers (0xFFFF for a masked column), nine bisection steps
// count them, and log2(G) xor-shuffles reduce median << 16 | position inside the group.  Lists of more than G entries are left
// alone: k_mp_distinctive_long<G>, the product wave with the short lists skipped, takes them in a second launch.
template <int G>
__global__ __launch_bounds__(256) void k_mp_distinctive_packed(const uint8_t* __restrict__ desc_kf, const int* __restrict__ counts_kf, MpObs O,
                                                               uint8_t* __restrict__ mp_desc, int* __restrict__ best_obs, int* __restrict__ best_median) {
    const int lane = threadIdx.x & 63, l = lane & (G - 1), gbase = lane & ~(G - 1);
    const int mp = (int)((blockIdx.x * 256u + threadIdx.x) / G);
    int o0 = 0, E = 0;
    bool mine = false;
    if (mp < O.nmp) { E = mp_obs_range(O, mp, o0); mine = E <= G; }
    unsigned a[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = 0;
    bool ok = false;
    if (mine) ok = mpd_load(O, counts_kf, desc_kf, o0, E, l, a);
    const u64 bal = __ballot(ok);
    const unsigned gmask = (unsigned)((bal >> gbase) & (G == 32 ? 0xFFFFFFFFull : ((1ull << G) - 1)));
    const int k = (__popc(gmask) - 1) >> 1;
    unsigned d[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        unsigned dd = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) dd = bcnt_acc(a[t] ^ (unsigned)__shfl((int)a[t], gbase + j), dd);
        d[j] = ((gmask >> j) & 1u) ? dd : 0xFFFFu;
    }
    int lo = 0, hi = 256;
    for (int it = 0; it < 9; ++it) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < G; ++j) cnt += d[j] <= (unsigned)mid;
        if (cnt > k) hi = mid; else lo = mid + 1;
    }
    unsigned key = ok ? ((unsigned)lo << 16 | (unsigned)l) : 0xFFFFFFFFu;
#pragma unroll
    for (int sft = G / 2; sft > 0; sft >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, sft));
    if (!mine) return;                                                      // every shuffle is behind us
    if (key == 0xFFFFFFFFu) {
        if (l == 0) { best_obs[mp] = -1; if (best_median) best_median[mp] = -1; }
        return;
    }
    const int win = (int)(key & 0xFFFFu);
    if (l < 8) {
        const long long p = mp_obs_slot(O, counts_kf, o0 + win);
        ((unsigned*)(mp_desc + (size_t)mp * 32))[l] = ((const unsigned*)(desc_kf + p * 32))[l];
    }
    if (l == 0) { best_obs[mp] = win; if (best_median) best_median[mp] = (int)(key >> 16); }
}

template <int G>
__global__ __launch_bounds__(256) void k_mp_distinctive_long(const uint8_t* __restrict__ desc_kf, const int* __restrict__ counts_kf, MpObs O,
                                                             uint8_t* __restrict__ mp_desc, int* __restrict__ best_obs, int* __restrict__ best_median) {
    __shared__ __attribute__((aligned(16))) unsigned short sD[4][64][64];
    mp_distinctive_block<G>(desc_kf, counts_kf, O, mp_desc, best_obs, best_median, sD, reinterpret_cast<unsigned&>(sD[0][63][0]));
}
#endif  /* ORBX_AB */

// k_mp_normal_depth: one thread per MapPoint, a sequential loop over its entries in the order given (float addition order is part of
// the result).  Entries of bad KeyFrames count here: the reference does not test them.  Per entry d = pw - Ow in float (Ow from ow_l or,
// flag bit 0, ow_r), s = (float)(1.0 / sqrt(double sum of d^2)) -- cv::norm and Mat / s of facade/cvcompat.h --, normal += d * s as a
// float multiply and a float add.  An entry that names the right camera while ow_r is NULL is skipped like an out-of-range one.
struct MpNdParams { int nlevels; ScaleTab sf; };

__device__ __forceinline__ double mp_norm3(float x, float y, float z) { return sqrt((double)x * (double)x + (double)y * (double)y + (double)z * (double)z); }

__global__ __launch_bounds__(256) void k_mp_normal_depth(const KpIn* __restrict__ kps_kf, const int* __restrict__ counts_kf, const float* __restrict__ ow_l,
                                                         const float* __restrict__ ow_r, MpObs O, const float* __restrict__ pw,
                                                         const int* __restrict__ ref_row, const int* __restrict__ ref_slot, MpNdParams P,
                                                         float* __restrict__ normal, float* __restrict__ min_dist, float* __restrict__ max_dist,
                                                         uint8_t* __restrict__ updated) {
    const int mp = blockIdx.x * 256 + threadIdx.x;
    if (mp >= O.nmp) return;
    int o0;
    const int E = mp_obs_range(O, mp, o0);
    if (E == 0) { updated[mp] = 0; return; }                                // not valid or an empty list: nothing else is read
    const float px = pw[(size_t)mp * 3], py = pw[(size_t)mp * 3 + 1], pz = pw[(size_t)mp * 3 + 2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    int n = 0;
    for (int e = o0; e < o0 + E; ++e) {
        const int r = O.row[e], s = O.slot[e];
        if ((unsigned)r >= (unsigned)O.nkf_rows || s < 0 || s >= min(counts_kf[r], O.cap)) continue;
        const bool right = O.flags[e] & 1;
        if (right && !ow_r) continue;
        const float* ow = (right ? ow_r : ow_l) + (size_t)r * 3;
        const float dx = px - ow[0], dy = py - ow[1], dz = pz - ow[2];
        const float sc = (float)(1.0 / mp_norm3(dx, dy, dz));
        nx = nx + dx * sc; ny = ny + dy * sc; nz = nz + dz * sc;
        ++n;
    }
    uint8_t ok = 0;
    if (n > 0) {
        const int rr = ref_row[mp], rs = ref_slot[mp];
        if ((unsigned)rr < (unsigned)O.nkf_rows && rs >= 0 && rs < min(counts_kf[rr], O.cap)) {
            const int level = kps_kf[(size_t)rr * O.cap + rs].octave;
            if (level >= 0 && level < P.nlevels) {
                const float* ow = ow_l + (size_t)rr * 3;
                const float dist = (float)mp_norm3(px - ow[0], py - ow[1], pz - ow[2]);
                const float mx = dist * P.sf.sf[level];
                const float inv = (float)(1.0 / (double)n);
                max_dist[mp] = mx;
                min_dist[mp] = mx / P.sf.sf[P.nlevels - 1];
                normal[(size_t)mp * 3] = nx * inv; normal[(size_t)mp * 3 + 1] = ny * inv; normal[(size_t)mp * 3 + 2] = nz * inv;
                ok = 1;
            }
        }
    }
    updated[mp] = ok;
}

// ------------------------------------------------------------------------------------------------
// k_bow_vector: the BowVector of one row of (word, weight) features -- TemplatedVocabulary::transform for the header `0 0`
// (TemplatedVocabulary.h:1145-1161, :1193) with BowVector::addWeight and BowVector::normalize(L1) (BowVector.cpp:34-46, :62-84).
// One workgroup per row.
//   keys    one 64-bit key per feature i < n with weight > 0 and word >= 0: word << 32 | i; every other slot and the padding to
//           n2 = a power of two hold all ones.  k_depth_select's bitonic network sorts them in LDS, so that the features of one word are
//           neighbours in feature order and the words ascend: std::map's order.
//   sums    the lane at the head of a run adds the run's weights one after the other in feature order (v = w0; v = v + w1; ...):
//           double addition is not associative and nothing is reassociated.  The head's output position is the number of heads before
//           it (ballot prefix inside the wave, wave totals through LDS).  bow_word / bow_val receive the word and the raw sum.
//   norm    wave 0 reads the raw sums back 64 at a time and adds fabs of lane 0, 1, 2, ... into one wave-uniform double: ONE serial
//           chain in ascending word id.  Every value is then divided by it, only if norm > 0.0.
// Only positions below nbow[r] are written; every value is recomputed per launch, so nothing accumulates across graph replays.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_bow_vector(const int* __restrict__ word_id, const double* __restrict__ weight,
                                                     const int* __restrict__ counts, int cap, int n2, int* __restrict__ bow_word,
                                                     double* __restrict__ bow_val, int* __restrict__ nbow) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long bv_keys[];
    __shared__ int sCnt[16];
    __shared__ double sNorm;
    const int r = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
    const size_t o0 = (size_t)r * cap;
    const int n = min(max(counts[r], 0), cap);
    const int* wid = word_id + o0;
    const double* wgt = weight + o0;
    for (int i = tid; i < n2; i += T) {
        unsigned long long key = ~0ull;
        if (i < n) {
            const int w = wid[i];
            if (wgt[i] > 0 && w >= 0) key = ((unsigned long long)(unsigned)w << 32) | (unsigned)i;     // !(w > 0) is left out (:1157)
        }
        bv_keys[i] = key;
    }
    __syncthreads();
    const int half = n2 >> 1;
    for (int k = 2; k <= n2; k <<= 1) {                                      // k_depth_select's network, step for step
        int j = k >> 1;
        for (; j > 64; j >>= 1) {
            for (int p = tid; p < half; p += T) {
                const int i = 2 * p - (p & (j - 1)), q = i | j;
                const unsigned long long a = bv_keys[i], b = bv_keys[q];
                if ((a > b) == ((i & k) == 0)) { bv_keys[i] = b; bv_keys[q] = a; }
            }
            __syncthreads();
        }
        for (int p0 = tid & ~63; p0 < half; p0 += T) {
            const int p = p0 + lane;
            for (int jj = j; jj > 0; jj >>= 1) {
                if (p < half) {
                    const int i = 2 * p - (p & (jj - 1)), q = i | jj;
                    const unsigned long long a = bv_keys[i], b = bv_keys[q];
                    if ((a > b) == ((i & k) == 0)) { bv_keys[i] = b; bv_keys[q] = a; }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
    int* ow = bow_word + o0;
    double* ov = bow_val + o0;
    int base = 0;                                                            // heads before this chunk of T positions
    for (int p0 = 0; p0 < n2; p0 += T) {                                     // uniform trip count: every lane reaches the barriers
        const int p = p0 + tid;
        const unsigned long long key = p < n2 ? bv_keys[p] : ~0ull;
        const int w = (int)(key >> 32);
        const bool head = key != ~0ull && (p == 0 || (int)(bv_keys[p - 1] >> 32) != w);
        const u64 bal = __ballot(head);
        if (lane == 0) sCnt[wave] = __popcll(bal);
        __syncthreads();
        int before = base, total = 0;
        for (int v = 0; v < nwaves; ++v) { const int c = sCnt[v]; total += c; if (v < wave) before += c; }
        if (head) {
            double v = wgt[(unsigned)key];
            for (int e = p + 1; e < n2; ++e) {
                const unsigned long long ke = bv_keys[e];
                if (ke == ~0ull || (int)(ke >> 32) != w) break;
                v = v + wgt[(unsigned)ke];
            }
            const int jo = before + __popcll(bal & ((1ull << lane) - 1));
            ow[jo] = w; ov[jo] = v;
        }
        base += total;
        __syncthreads();                                                     // sCnt is free for the next chunk
    }
    const int nb = base;
    if (wave == 0) {
        double norm = 0.0;
        for (int c0 = 0; c0 < nb; c0 += 64) {
            const int cnt = min(64, nb - c0);
            const double mine = lane < cnt ? ov[c0 + lane] : 0.0;
            for (int l = 0; l < cnt; ++l) norm = norm + fabs(__shfl(mine, l));
        }
        if (lane == 0) { sNorm = norm; nbow[r] = nb; }
    }
    __syncthreads();
    const double norm = sNorm;
    if (norm > 0.0)
        for (int jo = tid; jo < nb; jo += T) ov[jo] = ov[jo] / norm;
}

// ------------------------------------------------------------------------------------------------
// KeyFrameDatabase queries: DetectRelocalizationCandidates (KeyFrameDatabase.cc:869-981) and DetectNBestCandidates (:660-866) as far as
// the inverted file, the 0.8 rule and L1Scoring::score go.  ONE wave per (query q, database row r), four per workgroup; lanes over the
// row's entries in chunks of 64, each lane looking its word up in the query's ascending words by binary search.
// k_kfdb_common: common = sum of the ballot popcounts, first_word = the word of the first hit (the row ascends); one atomicMax and one
//   atomicAdd per sharing row into max_common / nsharing, which a memset ahead of the kernel in the same stream zeroes: integer maximum
//   and sum do not depend on their order, and a replayed graph starts from the memset.
// k_kfdb_score: min_common = (int)((float)max_common * 0.8f), scored = common > min_common; a scored row repeats the lookup and adds
//   fabs(vi - wi) - fabs(vi) - fabs(wi) (ScoringObject.cpp:41) for the set bits of each chunk's ballot in ascending lane = ascending
//   word, every term broadcast from its lane into one wave-uniform double: L1Scoring::score's chain, in its order, without LDS.
// Row lengths are min(max(n, 0), cap); a q_row outside [0, nq_rows) is an empty query.  Nothing is read out of bounds.
// ------------------------------------------------------------------------------------------------
struct KfdbParams {
    int nq, nq_rows, q_cap, ndb_rows, db_cap;
    const int* q_row; const int* q_word; const double* q_val; const int* q_n;
    const int* db_word; const double* db_val; const int* db_n; const uint8_t* db_active; const uint8_t* exclude;
};

// the query's row: its length (0 for a q_row out of range) and the start of its arrays
__device__ __forceinline__ int kfdb_query(const KfdbParams& P, int q, size_t& qo) {
    const int qr = P.q_row[q];
    qo = 0;
    if ((unsigned)qr >= (unsigned)P.nq_rows) return 0;
    qo = (size_t)qr * P.q_cap;
    return min(max(P.q_n[qr], 0), P.q_cap);
}
// the database row's length as this query sees it: 0 when the row is inactive or excluded
__device__ __forceinline__ int kfdb_row(const KfdbParams& P, int q, int r) {
    if (P.db_active && !P.db_active[r]) return 0;
    if (P.exclude && P.exclude[(size_t)q * P.ndb_rows + r]) return 0;
    return min(max(P.db_n[r], 0), P.db_cap);
}
// position of word w in qw[0, nq), or -1
__device__ __forceinline__ int kfdb_find(const int* __restrict__ qw, int nq, int w) {
    int lo = 0, hi = nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qw[mid] < w) lo = mid + 1; else hi = mid;
    }
    return (lo < nq && qw[lo] == w) ? lo : -1;
}

__global__ __launch_bounds__(256) void k_kfdb_common(KfdbParams P, int* __restrict__ common, int* __restrict__ first_word,
                                                     int* __restrict__ max_common, int* __restrict__ nsharing) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), q = blockIdx.y;
    if (r >= P.ndb_rows) return;                                             // wave-uniform
    size_t qo;
    const int nqw = kfdb_query(P, q, qo);
    const int nr = nqw > 0 ? kfdb_row(P, q, r) : 0;
    const int* qw = P.q_word + qo;
    const int* rw = P.db_word + (size_t)r * P.db_cap;
    int cnt = 0, first = -1;
    for (int c0 = 0; c0 < nr; c0 += 64) {
        const int i = c0 + lane;
        const int w = i < nr ? rw[i] : 0;
        const bool hit = i < nr && kfdb_find(qw, nqw, w) >= 0;
        const u64 bal = __ballot(hit);
        if (bal && first < 0) first = __shfl(w, __builtin_ctzll(bal));
        cnt += __popcll(bal);
    }
    if (lane == 0) {
        const size_t o = (size_t)q * P.ndb_rows + r;
        common[o] = cnt; first_word[o] = first;
        if (cnt > 0) { atomicMax(&max_common[q], cnt); atomicAdd(&nsharing[q], 1); }
    }
}

__global__ __launch_bounds__(256) void k_kfdb_score(KfdbParams P, const int* __restrict__ common, const int* __restrict__ max_common,
                                                    float* __restrict__ score, uint8_t* __restrict__ scored,
                                                    int* __restrict__ min_common, int* __restrict__ nscored) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), q = blockIdx.y;
    if (r >= P.ndb_rows) return;
    const int minc = (int)__fmul_rn((float)max_common[q], 0.8f);             // KeyFrameDatabase.cc:905: a float product, truncated
    if (r == 0 && lane == 0) min_common[q] = minc;
    const size_t o = (size_t)q * P.ndb_rows + r;
    const bool sc = common[o] > minc;                                        // strict (:916); common is 0 wherever the row is not searched
    double s = 0.0;
    if (sc) {
        size_t qo;
        const int nqw = kfdb_query(P, q, qo);
        const int nr = kfdb_row(P, q, r);
        const int* qw = P.q_word + qo;
        const double* qv = P.q_val + qo;
        const int* rw = P.db_word + (size_t)r * P.db_cap;
        const double* rv = P.db_val + (size_t)r * P.db_cap;
        for (int c0 = 0; c0 < nr; c0 += 64) {
            const int i = c0 + lane;
            const int pos = i < nr ? kfdb_find(qw, nqw, rw[i]) : -1;
            double term = 0.0;
            if (pos >= 0) {
                const double vi = qv[pos], wi = rv[i];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
            for (u64 m = __ballot(pos >= 0); m; m &= m - 1) s = s + __shfl(term, __builtin_ctzll(m));
        }
    }
    if (lane == 0) {
        score[o] = sc ? (float)(-s / 2.0) : 0.0f;
        scored[o] = sc ? 1 : 0;
        if (sc) atomicAdd(&nscored[q], 1);
    }
}

// k_gather_rows: packs the used prefix of every row of the two [nq][cap] candidate arrays into [nq][maxc] (one contiguous
// device-to-host copy instead of nq*cap entries or a strided copy).
__global__ __launch_bounds__(256) void k_gather_rows(const int* __restrict__ idx, const int* __restrict__ dist, int nq, int cap, int maxc,
                                                     int* __restrict__ oidx, int* __restrict__ odist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq * maxc) return;
    const int q = i / maxc, k = i - q * maxc;
    oidx[i] = idx[(size_t)q * cap + k];
    odist[i] = dist[(size_t)q * cap + k];
}

// ------------------------------------------------------------------------------------------------
// KeyFrameCulling: LocalMapping::KeyFrameCulling's redundancy counts (LocalMapping.cc:1218-1400) for every candidate KeyFrame of a call,
// over the KeyFrame pool and the observation CSR of the MapPoint refresh (MpObs, mp_obs_range, mp_obs_slot: the same skip rules).
// k_kfcull, grid = (ceil(cap / 16), ncand), 256 threads:
//   Work split.  The unit is one (candidate, slot) item with a ragged entry list; per entry the work is one 4-byte octave out of a
//   28-byte keypoint at a scattered pool address (a pool of 100 rows x 1000 slots is 2.8 MB: it stays in one XCD's 4 MiB L2).  One
//   thread per slot would walk lists of 3..30 entries in divergent loops with one gather in flight per lane.  Instead a group of 16
//   lanes takes a slot -- four slots per wave, sixteen per workgroup -- and walks the list 16 entries at a time: the typical list is
//   one or two rounds, every round is 16 independent gathers, and the group's sums are popcounts of wave ballots masked to the group
//   (no shuffles, no LDS).  A list of more than 64 entries is left out of the group rounds and taken afterwards by the WHOLE wave, 64
//   entries a round, so the longest legal list (65535) costs its own wave 1024 rounds and the other three waves of the workgroup
//   nothing.  16 rather than 8 lanes: at a mean of 8 entries half of the lists are longer than 8 and would need a second round.
//   Early exit.  With erased == NULL nobs_eff is mp_nobs[j]: a slot with mp_nobs <= th_obs is not walked at all and a walk stops after
//   the round in which its count passed th_obs (the reference's break, :1335; counts only grow, so the answer is the same).  With an
//   erased row every list is walked to its end, because nobs_eff needs all of it.
//   Pairs.  A right entry that passes re-reads its predecessor: when that is a live left entry of the same row which passes too, the
//   KeyFrame was counted there (the scaleLeveli minimum of :1316-1328).  No state crosses a round.
//   Counts.  Per workgroup two LDS counters take the wave ballots' popcounts, then one integer atomicAdd each into n_mps[k] /
//   n_redundant[k], rows that a memset in the same stream has zeroed: exact, and the same on every replay.
// k_kfcull_finish, one workgroup behind it in the stream: cull[k] = (float)n_redundant > redundant_th * (float)n_mps (one float
// multiply, one compare, :1349) and first_cull by a minimum over the workgroup, with plain stores: nothing to reset between replays.
// Nothing reads out of bounds whatever cand_row, kf_mp and the CSR hold.
// ------------------------------------------------------------------------------------------------
struct KfcullParams {
    int ncand, th_obs;
    float th_depth;
    const int* cand_row; const KpIn* kps_kf; const int* counts_kf; const int* kf_mp; const float* depth; const int* mp_nobs; const uint8_t* erased;
};

// entry a of the CSR against candidate row r at level L: er = a live entry of an erased row (w = its weight in nObs), ps = it adds one
// to the count of observing KeyFrames
__device__ __forceinline__ void kfc_entry(const KfcullParams& P, const MpObs& O, int r, int L, int a, bool first, bool& er, int& w, bool& ps) {
    er = false; ps = false; w = 0;
    const long long p = mp_obs_slot(O, P.counts_kf, a);
    if (p < 0) return;                                                      // skipped: neither erased nor observing
    const int row = O.row[a];
    const unsigned fl = O.flags[a];
    if (P.erased && P.erased[row]) { er = true; w = (fl & 4) ? 2 : 1; return; }
    if (row == r) return;                                                   // pKFi == pKF (:1312)
    const long long top = (long long)L + 1;
    if ((long long)P.kps_kf[p].octave > top) return;
    ps = true;
    if ((fl & 1) && !first && O.row[a - 1] == row && !(O.flags[a - 1] & 1)) {   // the right entry of a pair: counted at the left entry if that passes
        const long long q = mp_obs_slot(O, P.counts_kf, a - 1);
        if (q >= 0 && (long long)P.kps_kf[q].octave <= top) ps = false;
    }
}

__global__ __launch_bounds__(256) void k_kfcull(KfcullParams P, MpObs O, int* __restrict__ n_mps, int* __restrict__ n_redundant,
                                                uint8_t* __restrict__ slot_state) {
    __shared__ int sCnt[2];
    const int k = blockIdx.y, lane = threadIdx.x & 63, l = lane & 15;
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4);                     // the group's slot
    const u64 gm = 0xFFFFull << (lane & 48);                                // the group's lanes in a wave ballot
    if (threadIdx.x < 2) sCnt[threadIdx.x] = 0;
    __syncthreads();
    const int r = P.cand_row[k];
    const bool full = P.erased != nullptr;
    int n = 0;
    if ((unsigned)r < (unsigned)O.nkf_rows && !(full && P.erased[r])) n = min(P.counts_kf[r], O.cap);
    bool counted = false;
    long long nobs = 0;
    int L = 0, o0 = 0, E = 0;
    if (i < n) {
        const size_t at = (size_t)k * O.cap + i;
        const int j = P.kf_mp[at];
        if ((unsigned)j < (unsigned)O.nmp && !(O.valid && !O.valid[j])) {
            bool inDepth = true;
            if (P.depth) { const float d = P.depth[at]; inDepth = !(d > P.th_depth || d < 0); }   // :1295 as written: NaN and -0.0 pass
            if (inDepth) {
                counted = true;
                nobs = P.mp_nobs[j];
                E = mp_obs_range(O, j, o0);
                L = P.kps_kf[(size_t)r * O.cap + i].octave;
            }
        }
    }
    const bool walk = counted && E > 0 && (full || nobs > P.th_obs);
    int cnt = 0, wsum = 0;
    bool anyE = false;
    // lists of at most 64 entries: the group's 16 lanes, 16 entries a round
    const int Es = (walk && E <= 64) ? E : 0;
    for (int base = 0; __any(base < Es && (full || cnt <= P.th_obs)); base += 16) {
        bool er = false, ps = false;
        int w = 0;
        const int e = base + l;
        if (e < Es && (full || cnt <= P.th_obs)) kfc_entry(P, O, r, L, o0 + e, e == 0, er, w, ps);
        const u64 bp = __ballot(ps) & gm, be = __ballot(er) & gm, b2 = __ballot(er && w == 2) & gm;
        cnt += __popcll(bp); wsum += __popcll(be) + __popcll(b2); anyE |= be != 0;
    }
    // longer lists: the whole wave, 64 entries a round, one list after the other
    for (u64 m = __ballot(walk && E > 64 && l == 0); m; m &= m - 1) {
        const int src = __ffsll((long long)m) - 1;                           // the first lane of the list's group
        const int o0w = __shfl(o0, src), Ew = __shfl(E, src), Lw = __shfl(L, src);
        int c = 0, ws = 0;
        bool ae = false;
        for (int base = 0; base < Ew && (full || c <= P.th_obs); base += 64) {
            bool er = false, ps = false;
            int w = 0;
            const int e = base + lane;
            if (e < Ew) kfc_entry(P, O, r, Lw, o0w + e, e == 0, er, w, ps);
            const u64 be = __ballot(er);
            c += __popcll(__ballot(ps)); ws += __popcll(be) + __popcll(__ballot(er && w == 2)); ae |= be != 0;
        }
        if ((lane & 48) == src) { cnt = c; wsum = ws; anyE = ae; }
    }
    const long long eff = nobs - wsum;                                       // nObs after every erase; it only falls (MapPoint.cc:231-250)
    if (anyE && eff <= 2) counted = false;                                  // bad by erasure: gone from this KeyFrame too (:280-305)
    const bool red = counted && eff > P.th_obs && cnt > P.th_obs;
    if (slot_state && l == 0 && i < O.cap) slot_state[(size_t)k * O.cap + i] = counted ? (red ? 2 : 1) : 0;
    const int nc = __popcll(__ballot(counted && l == 0)), nr = __popcll(__ballot(red && l == 0));
    if (lane == 0) { if (nc) atomicAdd(&sCnt[0], nc); if (nr) atomicAdd(&sCnt[1], nr); }
    __syncthreads();
    if (threadIdx.x == 0) { if (sCnt[0]) atomicAdd(&n_mps[k], sCnt[0]); if (sCnt[1]) atomicAdd(&n_redundant[k], sCnt[1]); }
}

__global__ __launch_bounds__(1024) void k_kfcull_finish(int ncand, const int* __restrict__ n_mps, const int* __restrict__ n_redundant, float redundant_th,
                                                        uint8_t* __restrict__ cull, int* __restrict__ first_cull) {
    __shared__ int sFirst;
    if (threadIdx.x == 0) sFirst = INT_MAX;
    __syncthreads();
    int mine = INT_MAX;
    for (int k = threadIdx.x; k < ncand; k += 1024) {
        const float bound = redundant_th * (float)n_mps[k];                 // -ffp-contract=off: one multiply, then one compare
        const bool c = (float)n_redundant[k] > bound;
        cull[k] = c ? 1 : 0;
        if (c) mine = min(mine, k);
    }
    if (mine != INT_MAX) atomicMin(&sFirst, mine);
    __syncthreads();
    if (threadIdx.x == 0 && first_cull) *first_cull = sFirst == INT_MAX ? -1 : sFirst;
}

// ------------------------------------------------------------------------------------------------
// Covisibility votes: KeyFrame::UpdateConnections step 1 (KeyFrame.cc:474-512) and Tracking::UpdateLocalKeyFrames' keyframeCounter
// (Tracking.cc:3964-4013): every MapPoint of a query votes for the KeyFrames that observe it, over the observation CSR of the MapPoint
// refresh (MpObs, mp_obs_range, mp_obs_slot: the same skip rules).
// k_covis_votes, grid = (ceil(q_stride / COVIS_WG_SLOTS), nq), 256 threads:
//   Work split.  k_kfcull's (see its header comment): a group of 16 lanes per (query, slot), 16 entries of the MapPoint's list a round,
//   a list of more than 64 entries taken afterwards by the whole wave, 64 a round.  A workgroup takes COVIS_WG_SLOTS = 64 slots in four
//   passes of 16, so that its LDS table sees a few hundred votes.
//   Pairs.  A right entry (bit 0) directly preceded by a live, non-skipped left entry of the same row adds nothing: the KeyFrame voted
//   at the left entry (mObservations holds one entry per KeyFrame).  No state crosses a round: the right entry re-reads its predecessor.
//   Counts.  The votes of a query pile onto a few tens of rows.  LDS = true: a direct-mapped table of COVIS_TBL (row tag, count)
//   pairs takes them; the tag is claimed by an LDS compare-and-swap, a vote whose entry holds another row goes straight to a global
//   atomicAdd, and at the end of the workgroup every occupied entry is flushed with one global atomicAdd.  LDS = false (A/B build only):
//   one global atomicAdd per vote.  Integer atomics into a row that a memset in the same stream has zeroed: exact, the same on every
//   replay.
// k_covis_finish, one workgroup per query behind it: n_voted, max_votes, n_over and the rows with votes > 0 in ascending row order, by a
// workgroup prefix scan over the dense row in chunks of 1024, with plain stores.
// Nothing reads out of bounds whatever q_mp, self_row and the CSR hold.
// ------------------------------------------------------------------------------------------------
#define COVIS_WG_SLOTS 64
#define COVIS_TBL 256
struct CovisParams {
    int q_stride, skip_bad;
    const int* q_mp; const int* q_n; const int* self_row; const int* counts_kf; const uint8_t* kf_skip;
};

// the row entry a of the CSR votes for, or -1: skipped, the query's own row, a kf_skip row, a bad KeyFrame under skip_bad
__device__ __forceinline__ int covis_live(const CovisParams& P, const MpObs& O, int self, int a) {
    if (mp_obs_slot(O, P.counts_kf, a) < 0) return -1;
    const int row = O.row[a];
    if (row == self) return -1;                                             // mnId == mnId (KeyFrame.cc:503)
    if (P.kf_skip && P.kf_skip[row]) return -1;
    if (P.skip_bad && (O.flags[a] & 2)) return -1;
    return row;
}
__device__ __forceinline__ int covis_entry(const CovisParams& P, const MpObs& O, int self, int a, bool first) {
    const int row = covis_live(P, O, self, a);
    if (row < 0) return -1;
    if ((O.flags[a] & 1) && !first && O.row[a - 1] == row && !(O.flags[a - 1] & 1) && covis_live(P, O, self, a - 1) == row) return -1;   // voted at the left entry
    return row;
}

template <bool LDS>
__device__ __forceinline__ void covis_vote(int row, int* __restrict__ vq, int* sTag, int* sCnt) {
    if (row < 0) return;
    if (LDS) {
        const int h = row & (COVIS_TBL - 1);
        const int was = atomicCAS(&sTag[h], -1, row);
        if (was == -1 || was == row) { atomicAdd(&sCnt[h], 1); return; }
    }
    atomicAdd(&vq[row], 1);
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_covis_votes(CovisParams P, MpObs O, int* __restrict__ votes) {
    __shared__ int sTag[COVIS_TBL], sCnt[COVIS_TBL];
    const int q = blockIdx.y, lane = threadIdx.x & 63, l = lane & 15;
    if (LDS) {
        for (int t = threadIdx.x; t < COVIS_TBL; t += 256) { sTag[t] = -1; sCnt[t] = 0; }
        __syncthreads();
    }
    const int n = min(max(P.q_n[q], 0), P.q_stride);
    const int self = P.self_row ? P.self_row[q] : -1;
    int* vq = votes + (size_t)q * O.nkf_rows;
    for (int pass = 0; pass < COVIS_WG_SLOTS / 16; ++pass) {
        const int i = blockIdx.x * COVIS_WG_SLOTS + pass * 16 + (threadIdx.x >> 4);   // the group's slot
        int o0 = 0, E = 0;
        if (i < n) {
            const int j = P.q_mp[(size_t)q * P.q_stride + i];
            if ((unsigned)j < (unsigned)O.nmp) E = mp_obs_range(O, j, o0);  // an invalid MapPoint has an empty list
        }
        // lists of at most 64 entries: the group's 16 lanes, 16 entries a round
        const int Es = E <= 64 ? E : 0;
        for (int e = l; e < Es; e += 16) covis_vote<LDS>(covis_entry(P, O, self, o0 + e, e == 0), vq, sTag, sCnt);
        // longer lists: the whole wave, 64 entries a round, one list after the other
        for (u64 m = __ballot(E > 64 && l == 0); m; m &= m - 1) {
            const int src = __ffsll((long long)m) - 1;                       // the first lane of the list's group
            const int o0w = __shfl(o0, src), Ew = __shfl(E, src);
            for (int e = lane; e < Ew; e += 64) covis_vote<LDS>(covis_entry(P, O, self, o0w + e, e == 0), vq, sTag, sCnt);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int t = threadIdx.x; t < COVIS_TBL; t += 256)
            if (sCnt[t] > 0) atomicAdd(&vq[sTag[t]], sCnt[t]);
    }
}

// exclusive position of this thread's flag among the workgroup's 1024 threads, and the workgroup's total; sWave holds 16 ints
__device__ __forceinline__ int wg_scan_flag(bool flag, int* sWave, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const u64 b = __ballot(flag);
    __syncthreads();                                                        // the previous round's readers are done
    if (lane == 0) sWave[w] = __popcll(b);
    __syncthreads();
    int before = 0; total = 0;
    for (int k = 0; k < nw; ++k) { const int c = sWave[k]; if (k < w) before += c; total += c; }
    return before + __popcll(b & ((1ull << lane) - 1));
}

__global__ __launch_bounds__(1024) void k_covis_finish(int nkf_rows, int th, int list_cap, const int* __restrict__ votes, int* __restrict__ n_voted,
                                                       int* __restrict__ max_votes, int* __restrict__ n_over, int* __restrict__ list_row,
                                                       int* __restrict__ list_votes) {
    __shared__ int sWave[16], sMax, sOver;
    const int q = blockIdx.x;
    const int* vq = votes + (size_t)q * nkf_rows;
    if (threadIdx.x == 0) { sMax = 0; sOver = 0; }
    int base = 0, mx = 0, over = 0;
    for (int r0 = 0; r0 < nkf_rows; r0 += 1024) {
        const int r = r0 + threadIdx.x;
        const int v = r < nkf_rows ? vq[r] : 0;
        int total;
        const int pos = base + wg_scan_flag(v > 0, sWave, total);
        if (v > 0) {
            mx = max(mx, v); over += v >= th ? 1 : 0;
            if (pos < list_cap) { list_row[(size_t)q * list_cap + pos] = r; list_votes[(size_t)q * list_cap + pos] = v; }
        }
        base += total;
    }
    __syncthreads();
    if (mx > 0) atomicMax(&sMax, mx);
    if (over) atomicAdd(&sOver, over);
    __syncthreads();
    if (threadIdx.x == 0) { n_voted[q] = base; max_votes[q] = sMax; n_over[q] = sOver; }
}

// ------------------------------------------------------------------------------------------------
// Local map points: Tracking::UpdateLocalPoints (Tracking.cc:3917-3948).  Position (k, i) of a frame holds MapPoint j =
// kf_mp[lkf_row[k]][i]; j is emitted at its FIRST position in (k, i) order (the mnTrackReferenceForFrame test of :3938-3944), and the
// emitted indices stand in position order.  The 32-bit key of a position is k * cap + i; a chunk is LP_CHUNK consecutive keys.
//   k_lp_mark   thread per position: atomicMin of the key into first_pos [T][nmp], which a memset in the same stream set to 0xFF.
//   k_lp_count  workgroup per (chunk, frame), four consecutive keys per thread: the number of positions whose key equals first_pos[j].
//   k_lp_scan   workgroup per frame: the chunk counts become exclusive offsets in place, 1024 a round; n_total and nq.
//   k_lp_write  workgroup per (chunk, frame): the chunk's own scan again, then local_mp with plain stores; emissions at and beyond
//               q_stride are dropped.
// No thread walks more than four positions or 1 / 1024 of the chunk counts.  Nothing reads out of bounds whatever lkf_row and kf_mp hold.
// ------------------------------------------------------------------------------------------------
#define LP_CHUNK 1024
struct LpParams {
    int lkf_stride, nkf_rows, cap, nmp, nchunks;
    const int* lkf_row; const int* n_lkf; const int* counts_kf; const int* kf_mp; const uint8_t* mp_valid;
};
// the MapPoint at position `key` of frame f, or -1
__device__ __forceinline__ int lp_at(const LpParams& P, int f, unsigned key) {
    const unsigned k = key / (unsigned)P.cap, i = key - k * (unsigned)P.cap;
    if ((int)k >= min(max(P.n_lkf[f], 0), P.lkf_stride)) return -1;
    const int row = P.lkf_row[(size_t)f * P.lkf_stride + k];
    if ((unsigned)row >= (unsigned)P.nkf_rows) return -1;
    if ((int)i >= min(P.counts_kf[row], P.cap)) return -1;
    const int j = P.kf_mp[(size_t)row * P.cap + i];
    if ((unsigned)j >= (unsigned)P.nmp) return -1;
    if (P.mp_valid && !P.mp_valid[j]) return -1;
    return j;
}

__global__ __launch_bounds__(256) void k_lp_mark(LpParams P, unsigned npos, unsigned* __restrict__ first_pos) {
    const int f = blockIdx.y;
    const unsigned key = blockIdx.x * 256u + threadIdx.x;
    if (key >= npos) return;
    const int j = lp_at(P, f, key);
    if (j >= 0) atomicMin(&first_pos[(size_t)f * P.nmp + j], key);
}

// the flags of the thread's four keys (bit b = key0 + b is a first position)
__device__ __forceinline__ unsigned lp_flags(const LpParams& P, int f, unsigned npos, const unsigned* __restrict__ first_pos, int* js) {
    const unsigned key0 = blockIdx.x * (unsigned)LP_CHUNK + threadIdx.x * 4u;
    unsigned fl = 0;
    for (int b = 0; b < 4; ++b) {
        js[b] = -1;
        if (key0 + b >= npos || key0 + b < key0) continue;
        const int j = lp_at(P, f, key0 + b);
        if (j >= 0 && first_pos[(size_t)f * P.nmp + j] == key0 + b) { fl |= 1u << b; js[b] = j; }
    }
    return fl;
}

__global__ __launch_bounds__(256) void k_lp_count(LpParams P, unsigned npos, const unsigned* __restrict__ first_pos, int* __restrict__ chunk_cnt) {
    __shared__ int sSum;
    const int f = blockIdx.y;
    if (threadIdx.x == 0) sSum = 0;
    __syncthreads();
    int js[4];
    int c = __popc(lp_flags(P, f, npos, first_pos, js));
    for (int o = 32; o; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sSum, c);
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[(size_t)f * P.nchunks + blockIdx.x] = sSum;
}

// inclusive scan of v over the workgroup; sWave holds blockDim.x / 64 ints; total = the workgroup's sum
__device__ __forceinline__ int wg_scan_incl(int v, int* sWave, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int s = v;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(s, o); if (lane >= o) s += t; }
    __syncthreads();
    if (lane == 63) sWave[w] = s;
    __syncthreads();
    int before = 0; total = 0;
    for (int k = 0; k < nw; ++k) { const int c = sWave[k]; if (k < w) before += c; total += c; }
    return before + s;
}

__global__ __launch_bounds__(1024) void k_lp_scan(int nchunks, int q_stride, int* __restrict__ chunk_cnt, int* __restrict__ n_total, int* __restrict__ nq) {
    __shared__ int sWave[16];
    const int f = blockIdx.x;
    int* c = chunk_cnt + (size_t)f * nchunks;
    int base = 0;
    for (int c0 = 0; c0 < nchunks; c0 += 1024) {
        const int at = c0 + threadIdx.x;
        const int v = at < nchunks ? c[at] : 0;
        int total;
        const int incl = wg_scan_incl(v, sWave, total);
        if (at < nchunks) c[at] = base + incl - v;
        base += total;
    }
    if (threadIdx.x == 0) { n_total[f] = base; nq[f] = min(base, q_stride); }
}

__global__ __launch_bounds__(256) void k_lp_write(LpParams P, unsigned npos, const unsigned* __restrict__ first_pos, const int* __restrict__ chunk_off,
                                                  int q_stride, int* __restrict__ local_mp) {
    __shared__ int sWave[4];
    const int f = blockIdx.y;
    int js[4];
    const unsigned fl = lp_flags(P, f, npos, first_pos, js);
    const int c = __popc(fl);
    int total;
    int pos = chunk_off[(size_t)f * P.nchunks + blockIdx.x] + wg_scan_incl(c, sWave, total) - c;
    for (int b = 0; b < 4; ++b)
        if (fl & (1u << b)) { if (pos < q_stride) local_mp[(size_t)f * q_stride + pos] = js[b]; ++pos; }
}

// ------------------------------------------------------------------------------------------------
// k_gather_map_points: the rows SearchLocalPoints reads, gathered from the MapPoint pool by local_mp.  Thread per (frame, entry); a
// descriptor moves as two 128-bit words.  Entries at and beyond nq[f] are not touched; an index outside [0, nmp) gets skip = 1 only.
// ------------------------------------------------------------------------------------------------
struct GatherMpParams {
    int q_stride, nmp;
    const int* local_mp; const int* nq;
    const float* mp_pw; const float* mp_normal; const float* mp_min_dist; const float* mp_max_dist; const uint8_t* mp_desc; const int* mp_nobs;
    const uint8_t* mp_skip;
    float* pw; float* normal; float* min_dist; float* max_dist; uint8_t* qdesc; uint8_t* mp_obs; uint8_t* skip;
};
__global__ __launch_bounds__(256) void k_gather_map_points(GatherMpParams P) {
    const int f = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= min(max(P.nq[f], 0), P.q_stride)) return;
    const size_t o = (size_t)f * P.q_stride + e;
    const int j = P.local_mp[o];
    if ((unsigned)j >= (unsigned)P.nmp) { if (P.skip) P.skip[o] = 1; return; }
    if (P.pw && P.mp_pw) { P.pw[o * 3] = P.mp_pw[(size_t)j * 3]; P.pw[o * 3 + 1] = P.mp_pw[(size_t)j * 3 + 1]; P.pw[o * 3 + 2] = P.mp_pw[(size_t)j * 3 + 2]; }
    if (P.normal && P.mp_normal) {
        P.normal[o * 3] = P.mp_normal[(size_t)j * 3]; P.normal[o * 3 + 1] = P.mp_normal[(size_t)j * 3 + 1]; P.normal[o * 3 + 2] = P.mp_normal[(size_t)j * 3 + 2];
    }
    if (P.min_dist && P.mp_min_dist) P.min_dist[o] = P.mp_min_dist[j];
    if (P.max_dist && P.mp_max_dist) P.max_dist[o] = P.mp_max_dist[j];
    if (P.qdesc && P.mp_desc) {
        const uint4* s = (const uint4*)(P.mp_desc + (size_t)j * 32);
        uint4* d = (uint4*)(P.qdesc + o * 32);
        const uint4 a = s[0], b = s[1];
        d[0] = a; d[1] = b;
    }
    if (P.mp_obs && P.mp_nobs) P.mp_obs[o] = P.mp_nobs[j] > 0 ? 1 : 0;
    if (P.skip) P.skip[o] = P.mp_skip ? (P.mp_skip[(size_t)f * P.nmp + j] ? 1 : 0) : 0;
}

// ------------------------------------------------------------------------------------------------
// k_pose_opt: Optimizer::PoseOptimization(Frame*) (Optimizer.cc:943-1286, !mpCamera2) for one frame per workgroup of 256 threads.  The
// arithmetic, the LM state machine, the four rounds and the REDUCTION ORDER are those of orbm_poseopt.h, which the host tests compile
// too; this file only supplies the context: where a thread's edges live and how 256 partial sums become one.
//   edges    slot s belongs to thread s % 256.  With cap <= PO_LDS_CAP (LDS = true) a slot's observation, point, weight, kind and state
//            are gathered once through q_mp into LDS (seven float planes and two byte planes, lane-consecutive: no bank conflicts) and
//            every later pass reads them there.  Past PO_LDS_CAP (LDS = false) every pass gathers the slot again from the global rows
//            (L2 hits after the first pass) and the state lives in the `outlier` row itself, which only the owning thread touches.
//            Registers were not used for the edges: the solve path already holds the 28 partial sums, three poses, H, b and x as doubles.
//   sums     po_dev_reduce: xor butterfly over the wave by __shfl_xor (a double moves as two 32-bit halves), lane 0 of each wave stores
//            to LDS, every thread adds the four wave sums in wave order.  Every thread therefore holds the same bits, the 6x6 solve and
//            every LM decision are computed redundantly by all 256 threads, and each data-dependent loop is uniform over the
//            workgroup: no broadcast, no divergence, and the barriers inside the loops are reached by everyone.
//   results  plain vector stores by the owning thread (flags) and by thread 0 (pose, counts).  One launch, no scratch, no atomics.
// A slot holds an edge when i < min(counts, cap), q_mp is inside [0, nmp) and the octave inside [0, nlevels).
// ------------------------------------------------------------------------------------------------
#define PO_LDS_CAP 1536
#define PO_MAX_LEVELS 32
struct PoseOptParams {
    int first, cap, nmp, nlevels;
    float k[4], bf, ils2[PO_MAX_LEVELS];
    const KpIn* kps_un; const int* counts; const float* uright; const int* q_mp; const float* mp_pw; const float* tcw_in;
    float* tcw_out; uint8_t* outlier; int* n_corr; int* n_good;
};

template <int NACC>
__device__ __forceinline__ void po_dev_reduce(double* v, double* sRed) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        double x = v[a];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, 64);
        v[a] = x;
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < NACC; ++a) sRed[wv * PO_NACC + a] = v[a];
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NACC; ++a) v[a] = ((sRed[a] + sRed[PO_NACC + a]) + sRed[2 * PO_NACC + a]) + sRed[3 * PO_NACC + a];
    __syncthreads();
}

__device__ __forceinline__ int po_dev_count(int c, int* sCnt) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
    if ((threadIdx.x & 63) == 0) sCnt[threadIdx.x >> 6] = c;
    __syncthreads();
    const int t = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
    __syncthreads();
    return t;
}

template <bool LDS>
struct PoDevCtx {
    PoCam C;
    int n, nmp, nlevels;
    float* sE; uint8_t* sState; uint8_t* sStereo; const float* sIls2; double* sRed; int* sCnt;    // LDS
    const KpIn* kp; const float* ur; const int* qmp; const float* pw; uint8_t* gState;           // the frame's global rows

    // the slot's edge from the global rows; false = no edge
    __device__ __forceinline__ bool gather(int s, PoEdge& e) const {
        const int j = qmp[s];
        if ((unsigned)j >= (unsigned)nmp) return false;
        const KpIn& k = kp[s];
        return po_make_edge(k.x, k.y, k.octave, ur ? ur + s : nullptr, pw + 3 * (size_t)j, sIls2, nlevels, e);
    }
    // the slot's edge and state for a pass; PO_NONE = no edge
    __device__ __forceinline__ int fetch(int s, PoEdge& e) const {
        if (LDS) {
            const int st = sState[s];
            if (st == PO_NONE) return st;
            e.u = (double)sE[s]; e.v = (double)sE[PO_LDS_CAP + s]; e.ur = (double)sE[2 * PO_LDS_CAP + s];
            e.X = (double)sE[3 * PO_LDS_CAP + s]; e.Y = (double)sE[4 * PO_LDS_CAP + s]; e.Z = (double)sE[5 * PO_LDS_CAP + s];
            e.w = (double)sE[6 * PO_LDS_CAP + s]; e.stereo = sStereo[s] != 0;
            return st;
        }
        if (!gather(s, e)) return PO_NONE;
        return gState[s] ? PO_OUTLIER : PO_INLIER;
    }
    __device__ __forceinline__ void system(const double T[12], bool kernel, double acc[PO_NACC]) const {
#pragma unroll
        for (int a = 0; a < PO_NACC; ++a) acc[a] = 0.0;
        for (int s = threadIdx.x; s < n; s += PO_THREADS) {
            PoEdge e;
            if (fetch(s, e) == PO_INLIER) po_edge_system(C, T, e, kernel, acc);
        }
        po_dev_reduce<PO_NACC>(acc, sRed);
    }
    __device__ __forceinline__ double chi(const double T[12], bool kernel) const {
        double c = 0.0;
        for (int s = threadIdx.x; s < n; s += PO_THREADS) {
            PoEdge e;
            if (fetch(s, e) == PO_INLIER) c = c + po_edge_chi(C, T, e, kernel);
        }
        po_dev_reduce<1>(&c, sRed);
        return c;
    }
    __device__ __forceinline__ int classify(const double Terr[12], const double T[12]) const {
        int nBad = 0;
        for (int s = threadIdx.x; s < n; s += PO_THREADS) {
            PoEdge e;
            const int st = fetch(s, e);
            if (st == PO_NONE) continue;
            const int ns = po_edge_classify(C, Terr, T, e, st);
            if (LDS) sState[s] = (uint8_t)ns; else gState[s] = (uint8_t)ns;
            nBad += ns == PO_OUTLIER;
        }
        return po_dev_count(nBad, sCnt);
    }
};

template <bool LDS>
__global__ __launch_bounds__(256) void k_pose_opt(PoseOptParams P) {
    __shared__ float sE[LDS ? 7 * PO_LDS_CAP : 1];
    __shared__ uint8_t sState[LDS ? PO_LDS_CAP : 1], sStereo[LDS ? PO_LDS_CAP : 1];
    __shared__ float sIls2[PO_MAX_LEVELS];
    __shared__ double sRed[4 * PO_NACC];
    __shared__ int sCnt[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const size_t in0 = (size_t)(P.first + f) * P.cap, out0 = (size_t)f * P.cap;
    int n = min(max(P.counts[P.first + f], 0), P.cap);
    if (LDS) n = min(n, PO_LDS_CAP);                                       // the host picks LDS = true only for cap <= PO_LDS_CAP
    float tin[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) tin[i] = P.tcw_in[12 * (size_t)f + i];
#pragma unroll
    for (int i = 0; i < PO_MAX_LEVELS; ++i) if (tid == i) sIls2[i] = P.ils2[i];
    __syncthreads();
    PoDevCtx<LDS> ctx;
    ctx.C = PoCam{(double)P.k[0], (double)P.k[1], (double)P.k[2], (double)P.k[3], (double)P.bf};
    ctx.n = n; ctx.nmp = P.nmp; ctx.nlevels = min(P.nlevels, PO_MAX_LEVELS);
    ctx.sE = sE; ctx.sState = sState; ctx.sStereo = sStereo; ctx.sIls2 = sIls2; ctx.sRed = sRed; ctx.sCnt = sCnt;
    ctx.kp = P.kps_un + in0; ctx.ur = P.uright ? P.uright + out0 : nullptr; ctx.qmp = P.q_mp + out0; ctx.pw = P.mp_pw; ctx.gState = P.outlier + out0;
    // the edges: every slot with a MapPoint starts as an inlier, mvbOutlier[i] = false (Optimizer.cc:1011, :1046)
    int cnt = 0;
    for (int s = tid; s < n; s += PO_THREADS) {
        PoEdge e;
        const bool has = ctx.gather(s, e);
        if (LDS) {
            sState[s] = has ? PO_INLIER : PO_NONE;
            if (has) {
                sE[s] = (float)e.u; sE[PO_LDS_CAP + s] = (float)e.v; sE[2 * PO_LDS_CAP + s] = (float)e.ur;
                sE[3 * PO_LDS_CAP + s] = (float)e.X; sE[4 * PO_LDS_CAP + s] = (float)e.Y; sE[5 * PO_LDS_CAP + s] = (float)e.Z;
                sE[6 * PO_LDS_CAP + s] = (float)e.w; sStereo[s] = e.stereo ? 1 : 0;
            }
        } else if (has) {
            ctx.gState[s] = 0;
        }
        cnt += has ? 1 : 0;
    }
    const int nCorr = po_dev_count(cnt, sCnt);                             // its barriers also publish the LDS planes (each slot stays with one thread anyway)
    double T[12];
    int nGood = 0;
    if (nCorr >= 3) {
        double T0[12];
        po_pose_from_float(tin, T0);
        nGood = po_four_rounds(ctx, nCorr, T0, T);
    }
    if (LDS)
        for (int s = tid; s < n; s += PO_THREADS)
            if (sState[s] != PO_NONE) P.outlier[out0 + s] = sState[s] == PO_OUTLIER ? 1 : 0;
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) P.tcw_out[12 * (size_t)f + i] = nCorr >= 3 ? (float)T[i] : tin[i];
        P.n_corr[f] = nCorr; P.n_good[f] = nGood;
    }
}

// k_discard_outliers: the loops around PoseOptimization for one (frame, slot) per thread.  With discard and the slot's outlier flag
// set (Tracking.cc:3038-3054, :3246-3262): q_mp = -1, outlier = 0, mp_seen = 1, counted in n_discarded.  Otherwise the slot counts in
// n_matches_map when it is no outlier and mp_nobs > 0 (:3055-3057; mnMatchesInliers of :3388-3410 with discard == 0), and step 1 of
// SearchLocalPoints (:3812-3832) follows: a bad MapPoint leaves the slot when clear_bad is set, any other is marked seen.  mp_seen takes
// plain byte stores of 1 (several slots may hit one MapPoint); the counts go by ballot popcount and one integer atomic per wave into
// rows a memset in the same stream zeroed, as k_frustum_batch.
struct DiscardParams {
    int cap, nmp, discard, clear_bad;
    const int* counts; int* q_mp; uint8_t* outlier; const int* mp_nobs; const uint8_t* mp_valid;
    uint8_t* mp_seen; int* n_matches_map; int* n_discarded;
};
__global__ __launch_bounds__(256) void k_discard_outliers(DiscardParams P) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(max(P.counts[f], 0), P.cap);
    bool match = false, gone = false;
    if (i < n) {
        const size_t o = (size_t)f * P.cap + i;
        const int j = P.q_mp[o];
        if ((unsigned)j < (unsigned)P.nmp) {
            const bool out = P.outlier[o] != 0;
            if (P.discard && out) {
                P.q_mp[o] = -1; P.outlier[o] = 0;
                if (P.mp_seen) P.mp_seen[(size_t)f * P.nmp + j] = 1;
                gone = true;
            } else {
                match = !out && P.mp_nobs[j] > 0;
                if (P.clear_bad && P.mp_valid && !P.mp_valid[j]) P.q_mp[o] = -1;
                else if (P.mp_seen) P.mp_seen[(size_t)f * P.nmp + j] = 1;
            }
        }
    }
    const u64 bm = __ballot(match), bg = __ballot(gone);
    if ((threadIdx.x & 63) == 0) {
        if (P.n_matches_map && bm) atomicAdd(&P.n_matches_map[f], __popcll(bm));
        if (P.n_discarded && bg) atomicAdd(&P.n_discarded[f], __popcll(bg));
    }
}

// ------------------------------------------------------------------------------------------------
// k_triangulate_new / k_triangulate_order: step 6 of LocalMapping::CreateNewMapPoints (LocalMapping.cc:609-892) behind M10's matches12.
// The per-match arithmetic is tri_one_match of orbm_triangulate.h, which the host tests compile too; this file supplies the walk.
//   k_triangulate_new    one lane per idx1 of the group's current KeyFrame (row1 of its pairs), 256 lanes per workgroup, grid.y = group.
//            The lane walks the group's pairs IN ORDER, reads matches12[p][idx1] (lane-consecutive) and stops trying at the first pair
//            whose match passes every gate: that loop IS the cross-pair rule -- a later pair's match for this idx1 is
//            dropped (TRI_TAKEN) exactly where the reference's search would have skipped a feature that holds a MapPoint.  No flag array,
//            no atomics.  The pair's pose, row and count are the same for every lane (uniform addresses); the level tables are copied to
//            LDS once because the octave indexes them per lane.  The 4x4, its V and the rotations live in registers (four named columns
//            each, constant indices after inlining).
//   k_triangulate_order  ONE wave per group.  The reference creates MapPoints pair by pair and inside a pair in ascending idx1
//            (ORBmatcher.cc, end of SearchForTriangulation_).  Lane L keeps the count of the group's pair L in a register (at most 64
//            pairs per group); the wave walks won_pair in chunks of 64 idx1, and per distinct pair of the chunk a ballot gives the count
//            and the rank of each lane among the lanes of the same pair.  Pass 1 counts, a wave scan over the lanes gives each pair's base,
//            pass 2 stores idx1 at base + running count + rank.  Every count starts from zero in the kernel, nothing is atomic: a replay
//            repeats its result.  The tail of `order` past ntotal is filled with -1.
// group_start travels in the kernel arguments (TRI_GROUPS_PER_LAUNCH groups per launch): the host checked it, the kernels trust it.
// ------------------------------------------------------------------------------------------------
#define TRI_GROUPS_PER_LAUNCH 128
#define TRI_MAX_GROUP_PAIRS 64
struct TriPool {
    int nrows, cap;
    const KpIn* kps_un; const KpIn* kps; const int* counts; const float* uright; const float* depth; const float* tcw; const float* ow;
};
struct TriNewParams {
    int g0, npairs, nlevels;                                  // first group of this launch
    float mb1, mbf1, mb2, ratio_factor, th_far;
    TriCam k1, k2;
    float sf1[TRI_MAX_LEVELS], ls1[TRI_MAX_LEVELS], sf2[TRI_MAX_LEVELS], ls2[TRI_MAX_LEVELS];
    int gstart[TRI_GROUPS_PER_LAUNCH + 1];
    TriPool p1, p2;
    const int* row1; const int* row2; const int* matches12;
    int* won_pair; int* won_idx2; float* x3d; uint8_t* reason; int* ncreated; int* order; int* ntotal;
};

__device__ __forceinline__ void tri_load_pose(const TriPool& pool, int row, TriPose& P) {
#pragma unroll
    for (int i = 0; i < 12; ++i) P.T[i] = pool.tcw[12 * (size_t)row + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) P.ow[i] = pool.ow[3 * (size_t)row + i];
}
__device__ __forceinline__ void tri_load_obs(const TriPool& pool, int row, int i, TriObs& o) {
    const size_t s = (size_t)row * pool.cap + i;
    const KpIn& ku = pool.kps_un[s];
    o.ux = ku.x; o.uy = ku.y; o.octave = ku.octave;
    if (pool.kps != pool.kps_un) { const KpIn& k = pool.kps[s]; o.kx = k.x; o.ky = k.y; } else { o.kx = o.ux; o.ky = o.uy; }
    o.uright = pool.uright ? pool.uright[s] : -1.f;
    o.depth = pool.depth ? pool.depth[s] : -1.f;
}

__global__ __launch_bounds__(256) void k_triangulate_new(TriNewParams P) {
    __shared__ float sTab[4 * TRI_MAX_LEVELS];
    const int tid = threadIdx.x, g = blockIdx.y;
    if (tid < TRI_MAX_LEVELS) {
        sTab[tid] = P.sf1[tid]; sTab[TRI_MAX_LEVELS + tid] = P.ls1[tid];
        sTab[2 * TRI_MAX_LEVELS + tid] = P.sf2[tid]; sTab[3 * TRI_MAX_LEVELS + tid] = P.ls2[tid];
    }
    __syncthreads();
    const int pBeg = P.gstart[g], pEnd = P.gstart[g + 1];
    const int cap1 = P.p1.cap, idx1 = blockIdx.x * 256 + tid;
    if (idx1 >= cap1) return;                                 // no barrier below
    const size_t gout = (size_t)(P.g0 + g) * cap1 + idx1;
    int won = -1, wonIdx2 = -1;
    float wx = 0.f, wy = 0.f, wz = 0.f;
    if (pBeg < pEnd) {
        const int r1 = P.row1[pBeg];
        bool mixed = false;
        for (int p = pBeg + 1; p < pEnd; ++p) mixed = mixed || P.row1[p] != r1;
        const bool ok1 = (unsigned)r1 < (unsigned)P.p1.nrows && !mixed;
        const int n1 = ok1 ? min(max(P.p1.counts[r1], 0), cap1) : 0;
        TriPose pose1; TriObs o1;
        if (ok1) tri_load_pose(P.p1, r1, pose1);
        const bool live = idx1 < n1;
        if (live) tri_load_obs(P.p1, r1, idx1, o1);
        for (int p = pBeg; p < pEnd; ++p) {
            const int r2 = P.row2[p];
            const bool ok2 = (unsigned)r2 < (unsigned)P.p2.nrows;
            const int n2 = ok2 ? min(max(P.p2.counts[r2], 0), P.p2.cap) : 0;
            const int m = live ? P.matches12[(size_t)p * cap1 + idx1] : -1;
            int r = mixed ? TRI_MIXED_ROW1 : TRI_NO_MATCH;
            if ((unsigned)m < (unsigned)n2) {                 // garbage (< -1, >= the row's count) reads as no match and is never dereferenced
                if (won >= 0) r = TRI_TAKEN;
                else {
                    TriPose pose2; TriObs o2;
                    tri_load_pose(P.p2, r2, pose2);
                    tri_load_obs(P.p2, r2, m, o2);
                    float x[3];
                    r = tri_one_match(P.k1, P.k2, P.mb1, P.mbf1, P.mb2, pose1, pose2, o1, o2, sTab, sTab + TRI_MAX_LEVELS, sTab + 2 * TRI_MAX_LEVELS,
                                      sTab + 3 * TRI_MAX_LEVELS, P.nlevels, P.ratio_factor, P.th_far, x);
                    if (tri_ok(r)) { won = p; wonIdx2 = m; wx = x[0]; wy = x[1]; wz = x[2]; }
                }
            }
            if (P.reason) P.reason[(size_t)p * cap1 + idx1] = (uint8_t)r;
        }
    }
    P.won_pair[gout] = won; P.won_idx2[gout] = wonIdx2;
    P.x3d[3 * gout] = wx; P.x3d[3 * gout + 1] = wy; P.x3d[3 * gout + 2] = wz;
}

__global__ __launch_bounds__(64) void k_triangulate_order(TriNewParams P) {
    const int lane = threadIdx.x, g = blockIdx.x;
    const int pBeg = P.gstart[g], np = min(P.gstart[g + 1] - pBeg, TRI_MAX_GROUP_PAIRS);
    const int cap1 = P.p1.cap;
    const size_t gout = (size_t)(P.g0 + g) * cap1;
    const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int cnt = 0;
    for (int c0 = 0; c0 < cap1; c0 += 64) {
        const int idx = c0 + lane;
        const int lp = (idx < cap1 ? P.won_pair[gout + idx] : -1) - pBeg;
        const bool has = (unsigned)lp < (unsigned)np;
        u64 rem = __ballot(has);
        while (rem) {
            const int pl = __shfl(lp, __ffsll(rem) - 1, 64);
            const u64 mask = __ballot(has && lp == pl);
            if (lane == pl) cnt += __popcll(mask);
            rem &= ~mask;
        }
    }
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
    const int total = __shfl(incl, 63, 64);
    if (lane < np) P.ncreated[pBeg + lane] = cnt;
    if (lane == 0) P.ntotal[P.g0 + g] = total;
    int run = incl - cnt;                                     // the pair's first position in `order`
    for (int c0 = 0; c0 < cap1; c0 += 64) {
        const int idx = c0 + lane;
        const int lp = (idx < cap1 ? P.won_pair[gout + idx] : -1) - pBeg;
        const bool has = (unsigned)lp < (unsigned)np;
        u64 rem = __ballot(has);
        while (rem) {
            const int pl = __shfl(lp, __ffsll(rem) - 1, 64);
            const bool mine = has && lp == pl;
            const u64 mask = __ballot(mine);
            const int at = __shfl(run, pl, 64) + __popcll(mask & below);
            if (mine && at < cap1) P.order[gout + at] = idx;
            if (lane == pl) run += __popcll(mask);
            rem &= ~mask;
        }
    }
    for (int i = total + lane; i < cap1; i += 64) P.order[gout + i] = -1;
}

}  // namespace orbmk
