// orbx_plan.h -- the extractor's host planner: everything the kernels are told about an image size, worked out in plain C++.
//
// HIP-free (C++17, the standard headers and the ABI's error codes only), so the library (orbx_api.hip) and a stand-alone CPU program
// (tests/plan_dump.cpp, driven by tests/test_plan_cpu.py) compile the same text.  It owns
//   * the records the host fills and the kernels read (orbx_kernels.hip.h includes this header), with the constants both sides share;
//   * plan_tables(): the reference constructor's tables (ORBextractor.cc:468-571) and the IC_Angle byte weights, in its float arithmetic;
//   * plan_geometry(): per image size the level sizes and slab offsets, the FAST cell grid, k_fast4's strips, launch groups and tables,
//     k_resize2's taps and task records, k_blur3's / k_blur2's task lists and weights, the quadtree's capacities and LDS sizes
//     (replays ORBextractor.cc:1669, 1053-1106, 695-699 in the reference's float arithmetic);
//   * rz_launch(), blur_walks(), qt_wide(): what a launch decides from the plan and the batch size.
// The limits that the kernels' comments call "host checks" are checked here.  Nothing here allocates device memory or reads the environment.
#pragma once
#include "../../include/orbx.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

namespace orbxk {

typedef uint32_t u32;
typedef uint16_t u16;
typedef uint8_t u8;

// ---- records and constants shared with the kernels (orbx_kernels.hip.h says at each kernel what they mean to it)
struct RzTab { int s; short a0, a1; };                     // source index + two Q11 taps (8 bytes)

struct LevelDesc {                                         // one pyramid level of the current geometry
    int w, h, pitch;
    int off;                                               // byte offset inside a frame's pyramid slab (levels >= 1)
    int boff, btpr;                                        // blurred copy: byte offset inside a frame's blurred slab; tiles per tile row (tiled layout)
    int rzx, rzy;                                          // offsets into the resize tap tables
    int cellBase, nCells;                                  // active FAST cells of this level in the cell table
    int slotBase, slotCap;                                 // candidate slots: slotBase + cell*slotCap + k
    int N, nIni, qtW, qtH;                                 // quadtree target, roots, extent (maxX-minX, maxY-minY)
    float hX;
    int selBase, selCap;                                   // quadtree output slots inside a frame
    float sf;                                              // mvScaleFactor[level]
    float patch;                                           // (float)(int)(31*sf)
};

struct CellInfo {                                          // one FAST cell (sub-image handed to cv::FAST)
    short level, x0, y0, cw, ch, addx, addy, pad;
    int slot;                                              // index of slot 0 of this cell within the frame
    int cnt;                                               // index of the count word within the frame
};

struct Geom {                                              // kernel argument block (passed by value)
    int nlevels, w0, h0;
    int iniTh, minTh, lowTh;
    int totalCells, totalSlots, totalSel, kpCap;
    int nodeCap, sortCap;
    size_t pyrFrameBytes;                                  // per-frame slab holding levels 1..L-1 (and a copy slot for 0)
    size_t blrFrameBytes;                                  // per-frame slab of the blurred levels
    int blurTiled;                                         // blurred levels are stored as 16 x 8-px tiles (one 128-byte line each), see k_blur3
    LevelDesc lv[12];
};

// k_resize2
#define RZ_R 8
#define RZ_SRC 12                                          // source rows one task may touch: what RZ_R rows need at scale factors up to 1.5 (host checks)
struct RzX4 { int bs; u8 o[4]; u32 a[4]; };                // per destination dword: byte offset of the first tap, tap offsets from it (<= 6), (2*a0 | 2*a1<<16): DOUBLED Q11 taps
struct alignas(64) RzTask {                                // 32 words
    int g0, y0;                                            // first destination dword and row
    int pack, gw, gmul;                                    // frames per wave, lanes per frame (64: full tile), ceil(65536 / gw)
    int sFirst, nsrc;                                      // first source row, source rows (2 .. RZ_SRC)
    u32 emit;                                              // bit j: source row sFirst + j completes a destination row (bit 0 is never set)
    int dpitch, doff, x4base;                              // destination level: pitch, offset in the slab, first entry of the x4 table
    int spitch, soff;                                      // source level (levels >= 1; level 0 is the caller's)
    int pad[3];
    u32 taps[16];                                          // [j]: a0 | a1 << 16 of the destination row that source row j completes
};
static_assert(sizeof(RzTask) == 128 && RZ_SRC == 12, "RzTask is read as 32 scalar words, of which 13 + 11 are pinned");
struct RzLaunch { u32 nFull, nPack, nimg, nFullW, nWaves, mFull, mPack; };   // mX = floor(2^32 / nX) + 1: n / nX = umulhi(n, mX) while n * nX < 2^32 (host checks)
#ifdef ORBX_AB   /* k_resize2p: A/B reference (8-row tasks of one frame, row taps reloaded per row), not in the product library */
#define RZP_R 8
#define RZP_SRC 12                                         // source rows one task may touch (host checks)
struct RzTaskP { short level, g0, y0, pad; };
#endif

// FAST
#define ORBX_FAST_TILE 6400
struct StripInfo { short level, ncell, x0, y0, w, h, xal, lp; int cell0; };   // lp = LDS tile pitch in bytes
#define F3_NT 256
struct CellAux {                                            // 32 bytes, read with one scalar load
    u32 tab;                                                // first F4Item of the cell's shape table: [nit][64]
    int slot, cnt;                                          // as CellInfo
    u16 base;                                               // tile byte offset of (row 0, xs 0): 3 * pitch + s4
    u16 nit;                                                // quick-pass iterations (0: empty window)
    short outx, outy;                                       // packed output coordinates of (row 0, xs 0)
    u16 xlo, xhi;                                           // xs of the window's first / last column
    u32 pad[2];
};
struct F4Item { u32 mask; u32 offq; };                      // mask: pixel k of the lane's 8 inside the window -> bit 4k+3; offq: lo16 = row * pitch + 8 * col, hi16 = row << 9 | col << 5

// k_blur3 / k_blur2
#define B3_ROWS 26
#ifndef B3_CHUNK
#define B3_CHUNK 8
#endif
struct Blur3Task { short level, x0, t0, nt; int th, tv; };   // th / tv: entries of the weight tables (tv: of tile t0)
#define BL_R 32
struct BlurTask { short level, g0, y0, pad; };            // g0 = first dword column of the strip, y0 = first output row
struct BlurSel { u32 selB[12], selC[12]; };               // per level: right-edge fix-up selectors

// k_orient_desc / k_orient_desc2
struct Umax { int v[16]; };
#define OD_WTAB (17 * 8)                                   // IC_Angle weight table: [|v| (16 = zero row)][dword of the 32-byte patch row]

// weight of source position p in output position `out` of an n-long line: sum_i [reflect101(out + i - 3) == p] * K[i]
// (host side: the weight fragments are tabulated per column strip and per tile row when the geometry is built)
static inline int b3_toep(int p, int out, int n) {
    const int K[7] = {18, 34, 48, 56, 48, 34, 18};
    int wsum = 0;
    for (int i = 0; i < 7; ++i) {
        int q = out + i - 3;
        q = q < 0 ? -q : q;
        q = q >= n ? 2 * n - 2 - q : q;
        wsum += q == p ? K[i] : 0;
    }
    return wsum;
}
// pass-1 weights (B operand) of the strip at x0: [k-step s][lane] uint4; lane (r, hh) holds column x0 + r, element j of
// k-step s <-> pixel x0 - 16 + 32 s + 16 hh + j
static inline void b3_build_th(int x0, int w, u32* out /* [2][64][4] */) {
    for (int s = 0; s < 2; ++s)
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 4; ++e) {
                const int r = lane & 31, hh = lane >> 5;
                u32 v = 0;
                for (int b = 0; b < 4; ++b) v |= (u32)b3_toep(x0 - 16 + 32 * s + 16 * hh + 4 * e + b, x0 + r, w) << (8 * b);
                out[(s * 64 + lane) * 4 + e] = v;
            }
}
// pass-2 weights (A operand) of the tile at y0: [lane] uint4; lane (r, hh) holds output row y0 + r (26 valid), element j <->
// H row (j&3) + 8 (j>>2) + 4 hh of the tile = image row y0 - 3 + that (the register order of the pass-1 accumulator)
static inline void b3_build_tv(int y0, int h, u32* out /* [64][4] */) {
    for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 4; ++e) {
            const int r = lane & 31, hh = lane >> 5;
            u32 v = 0;
            for (int b = 0; b < 4; ++b) {
                const int j = 4 * e + b, krow = (j & 3) + 8 * (j >> 2) + 4 * hh;
                v |= (r < B3_ROWS ? (u32)b3_toep(y0 - 3 + krow, y0 + r, h) : 0u) << (8 * b);
            }
            out[lane * 4 + e] = v;
        }
}

// ---- what the planner is given, and what it leaves behind
struct PlanConfig {                                        // orbx_create's arguments and the A/B knobs the planner reads (read from the environment there, never here)
    int nfeatures = 0, nlevels = 0, iniTh = 0, minTh = 0, maxW = 0, maxH = 0, maxBatch = 0;
    double scaleFactor = 0;                                // double member initialised from float (ORBextractor.h:96)
    bool blurTiled = true;                                 // k_blur3 writes / k_orient_desc2 reads the blurred levels as 16 x 8-px tiles (ORBX_BLUR_ROWMAJOR: A/B)
    bool fastV3 = false;                                   // ORBX_FAST_V3: A/B, k_fast3 instead of k_fast4
    bool f3NoFixedPitch = false;                           // ORBX_FAST_PITCH0: A/B, every group on the per-strip-pitch kernel
    int f3QcapForce = 0;                                   // ORBX_FAST_QCAP: test knob, forces a small queue
    int qtWideForce = -1;                                  // ORBX_QT_WIDE=0/1: A/B switch
    int fastWgs = 7;                                       // ORBX_FAST_WGS: A/B, workgroups per CU that the fine groups' queue is bounded for
    int fastLdsPad = 0;                                    // ORBX_FAST_LDSPAD: experiment, occupancy sensitivity
#ifdef ORBX_AB
    bool rzNoPack = false;                                 // ORBX_RESIZE_NOPACK: A/B, one frame per wave everywhere (the form of a slab too large for 32-bit lane offsets)
#endif
};

struct ExtractorTables {                                   // constructor tables of the reference, per level
    std::vector<float> sf, invsf, sig2, invsig2;
    std::vector<int> nfeat;
    Umax umax;
    std::array<u32, OD_WTAB> odW;                          // IC_Angle byte weights (k_orient_desc2)
};

// k_fast3 launch groups: level 0 (needs no resize), the fine levels, the coarse levels.  Each group sizes its own LDS
// (tile of its tallest cell row + survivor queues), because occupancy -- 20 vs 28 waves per CU -- is worth ~15 %.
struct F3Group { int strip0 = 0, nstrips = 0, tile = 0, qcap = 0, lastLevel = 0, pitch = 0; size_t lds = 0; bool v4 = false; };   // pitch: 176 / 208 = compile-time tile pitch of the group, 0 = per strip

struct Plan {                                              // geometry of one image size
    Geom g = {};
    std::vector<CellInfo> cells;
    std::vector<StripInfo> strips;
    std::vector<int> stripTile, stripQ;                       // per strip: tile bytes, worst-case queue entries
    std::vector<F3Group> f3g;
    size_t fastLds = 0;                                       // largest LDS size of any FAST group
    std::vector<CellAux> aux; std::vector<F4Item> f4items;    // k_fast4: per-cell scalars and per-shape item tables
    std::vector<RzTab> xt, yt;
    std::vector<RzX4> x4;
    std::vector<RzTask> rzTasks[12];                          // per level: the full-tile tasks, then the packed remainder tasks
    int rzTaskOff[12] = {}; bool rzStream[12] = {};           // first record of a level in the concatenated list; the level is resized by k_resize2
    int rzNFull[12] = {}, rzNPack[12] = {}, rzPack[12] = {};  // task counts of the two kinds; frames per wave of the packed kind
#ifdef ORBX_AB
    std::vector<RzTaskP> rzTasksP[12];
    int rzTaskOffP[12] = {}; bool rzStreamP[12] = {};
#endif
    std::vector<BlurTask> tiles;
    std::vector<Blur3Task> tiles3;                            // k_blur3 (matrix-core blur) tasks: B3_CHUNK-tile walks, then one-tile tasks
    size_t nTiles3Walk = 0;                                   // (small batches take the one-tile list: more, shorter workgroups)
    std::vector<u32> b3Th, b3Tv;                              // its weight fragments: [strip][2][64][4], [tile row][64][4]
    BlurSel blurSel = {};
    int64_t algBytes = 0, fusedBytes = 0;
    size_t qtLds = 0, qt2Lds = 0;
    int qtFuseD = 3;
    int qtHistD = 3;                                           // depth of k_quadtree2's deepest path histogram (>= qtFuseD)
    int maxIni = 1;                                            // most quadtree roots of any level
    int qt2Cap = 0, qt2Sort = 0;
    int maxCells = 0;
    bool qtWide = false;                                       // 1024-thread quadtree workgroups (large frames / feature counts)
    int l0pitch = 0;
};

static inline int cv_round_f(float v) { return (int)lrintf(v); }
static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

// The reference's constructor tables (ORBextractor.cc:468-571) and the byte weights made from umax.  The float / double mix is the reference's.
static inline ExtractorTables plan_tables(const PlanConfig& cfg) {
    ExtractorTables t;
    const int L = cfg.nlevels, nfeatures = cfg.nfeatures;
    t.sf.resize(L); t.sig2.resize(L); t.invsf.resize(L); t.invsig2.resize(L); t.nfeat.resize(L);
    t.sf[0] = 1.0f; t.sig2[0] = 1.0f;
    for (int i = 1; i < L; ++i) { t.sf[i] = (float)(t.sf[i - 1] * cfg.scaleFactor); t.sig2[i] = t.sf[i] * t.sf[i]; }
    for (int i = 0; i < L; ++i) { t.invsf[i] = 1.0f / t.sf[i]; t.invsig2[i] = 1.0f / t.sig2[i]; }
    float factor = (float)(1.0f / cfg.scaleFactor);
    float nDesired = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; ++l) { t.nfeat[l] = cv_round_f(nDesired); sum += t.nfeat[l]; nDesired *= factor; }
    t.nfeat[L - 1] = std::max(nfeatures - sum, 0);
    {   // umax (ORBextractor.cc:542-570)
        int* um = t.umax.v;
        int v, v0, vmax = (int)floorf(15 * sqrtf(2.f) / 2 + 1), vmin = (int)ceilf(15 * sqrtf(2.f) / 2);
        for (v = 0; v <= vmax; ++v) um[v] = (int)lrint(std::sqrt(225.0 - v * v));
        for (v = 15, v0 = 0; v >= vmin; --v) { while (um[v0] == um[v0 + 1]) ++v0; um[v] = v0; ++v0; }
    }
    {   // IC_Angle weights for v_dot4: entry [|v|][j] packs, for the 4 bytes of dword j of a 32-byte patch row (it starts at
        // cx-15) at distance |v| from the centre, (u + 16) where the pixel lies inside the disc (|u| <= umax[|v|]) and 0
        // elsewhere; u = 4j + b - 15.  Row 16 is all zero (lanes past the 31st row).
        t.odW.fill(0u);
        for (int va = 0; va < 16; ++va)
            for (int j = 0; j < 8; ++j) {
                u32 wv = 0;
                for (int b = 0; b < 4; ++b) {
                    const int u = 4 * j + b - 15;
                    if (std::abs(u) <= t.umax.v[va]) wv |= (u32)(u + 16) << (8 * b);
                }
                t.odW[va * 8 + j] = wv;
            }
    }
    return t;
}

// ---- plan_geometry and its parts, one per concern.  A part that can refuse returns 0 or an ORBX_E_* code, its text written by fail().
struct Planner {                                           // what the parts share while one plan is built
    const PlanConfig& cfg;
    const ExtractorTables& tab;
    Plan& p;
    char* err; size_t errlen;
    size_t off = 0, boff = 0;                              // bytes of a frame's pyramid / blurred slab so far
    int totalSlots = 0, totalSel = 0, maxN = 0;
    int64_t sumAll = 0, sumSrc = 0, sumDst = 0;
    std::vector<Blur3Task> tiles3one;                      // one-tile k_blur3 tasks, appended behind the walks

    int fail(int code, const char* fmt, ...) const {
        va_list ap; va_start(ap, fmt);
        if (err && errlen) vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
        return code;
    }
};

// size of level l, its place in the pyramid and blurred slabs, its scale and feature budget
static inline int plan_level(Planner& P, int l) {
    Geom& g = P.p.g;
    LevelDesc& D = g.lv[l];
    const int L = g.nlevels;
    const float scale = P.tab.invsf[l];
    D.w = cv_round_f((float)g.w0 * scale); D.h = cv_round_f((float)g.h0 * scale);
    if (D.w > 4095 || D.h > 4095) return P.fail(ORBX_E_UNSUPPORTED, "level %d is %dx%d: packed candidates hold 12-bit coordinates", l, D.w, D.h);
    D.pitch = align_up(D.w, 64);
    D.off = (int)P.off;
    P.off += (size_t)align_up(D.pitch * D.h, 256);
    // blurred copy: row-major twin of the level, or 16 x 8-px tiles (one more tile per tile row than the pitch needs: the
    // descriptor kernel's 48-byte patch rows may start up to 10 bytes before the right edge)
    D.btpr = D.pitch / 16 + 1;
    D.boff = P.cfg.blurTiled ? (int)P.boff : D.off;
    P.boff += (size_t)align_up(D.btpr * ((D.h + 7) / 8) * 128, 256);
    D.sf = P.tab.sf[l];
    D.patch = (float)(int)(31 * P.tab.sf[l]);
    D.N = P.tab.nfeat[l];
    P.sumAll += (int64_t)D.w * D.h;
    if (l < L - 1) P.sumSrc += (int64_t)D.w * D.h;
    if (l > 0) P.sumDst += (int64_t)D.w * D.h;
    return 0;
}

// FAST cell grid of level l and its strips
static inline int plan_cells(Planner& P, int l) {
    Plan& p = P.p;
    LevelDesc& D = p.g.lv[l];
    const int minB = 16, maxBX = D.w - 16, maxBY = D.h - 16;
    const float width = (float)(maxBX - minB), height = (float)(maxBY - minB);
    const float W = 35;
    const int nCols = (int)(width / W), nRows = (int)(height / W);
    if (nCols < 1 || nRows < 1) return P.fail(ORBX_E_TOO_SMALL, "level %d (%dx%d) is smaller than one FAST cell", l, D.w, D.h);
    const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
    D.cellBase = (int)p.cells.size();
    D.slotBase = P.totalSlots;
    D.slotCap = ((wCell + 1) / 2) * ((hCell + 1) / 2);
    for (int i = 0; i < nRows; ++i) {
        const float iniY = (float)(minB + i * hCell);
        float maxY = iniY + hCell + 6;
        if (iniY >= maxBY - 3) continue;
        if (maxY > maxBY) maxY = (float)maxBY;
        for (int j = 0; j < nCols; ++j) {
            const float iniX = (float)(minB + j * wCell);
            float maxX = iniX + wCell + 6;
            if (iniX >= maxBX - 6) continue;
            if (maxX > maxBX) maxX = (float)maxBX;
            CellInfo c;
            c.level = (short)l; c.x0 = (short)iniX; c.y0 = (short)iniY;
            c.cw = (short)((int)maxX - (int)iniX); c.ch = (short)((int)maxY - (int)iniY);
            c.addx = (short)(j * wCell); c.addy = (short)(i * hCell); c.pad = 0;
            c.cnt = (int)p.cells.size();
            c.slot = P.totalSlots;
            if ((int)c.cw * c.ch > ORBX_FAST_TILE) return P.fail(ORBX_E_UNSUPPORTED, "FAST cell %dx%d exceeds the LDS tile", c.cw, c.ch);
            P.totalSlots += D.slotCap;
            p.cells.push_back(c);
        }
    }
    D.nCells = (int)p.cells.size() - D.cellBase;
    // strips for k_fast3: runs of <= 8 cells of one cell-row (one wavefront per cell); the tile pitch is a
    // multiple of 16 bytes (<= 512) and starts >= 4 bytes left of the strip at a 16-byte aligned column
    for (int ci = D.cellBase; ci < (int)p.cells.size();) {
        const CellInfo& f = p.cells[ci];
        const int Hs = f.ch;
        if (Hs > 127) return P.fail(ORBX_E_UNSUPPORTED, "FAST cell of %d rows exceeds the strip kernel's 127", Hs);
        const int xal = (f.x0 - 4) & ~15;
        int n = 0, needed = 0;
        while (ci + n < (int)p.cells.size() && n < F3_NT / 64) {
            const CellInfo& c = p.cells[ci + n];
            if (c.y0 != f.y0) break;
            const int nd = c.x0 + c.cw - 3 - xal + 8;
            if (nd > 512) break;
            needed = nd; ++n;
        }
        if (n == 0) return P.fail(ORBX_E_UNSUPPORTED, "FAST cell %dx%d does not fit the strip tile", f.cw, f.ch);
        const CellInfo& last = p.cells[ci + n - 1];
        StripInfo st;
        st.level = (short)l; st.ncell = (short)n; st.x0 = f.x0; st.y0 = f.y0;
        st.w = (short)(last.x0 + last.cw - f.x0); st.h = (short)Hs; st.xal = (short)xal;
        st.lp = (short)align_up(needed, 16); st.cell0 = ci;
        int qworst = 64;
        for (int k = 0; k < n; ++k) {
            const CellInfo& c = p.cells[ci + k];
            qworst = std::max(qworst, align_up(std::max(0, c.cw - 6) * std::max(0, c.ch - 6), 64));
        }
        p.stripTile.push_back((int)st.lp * Hs); p.stripQ.push_back(qworst);
        p.strips.push_back(st);
        ci += n;
    }
    if (P.totalSlots - D.slotBase >= (1 << 24)) return P.fail(ORBX_E_UNSUPPORTED, "level %d has too many candidate slots", l);
    return 0;
}

// quadtree roots of level l (ORBextractor.cc:695-699) and its output slots
static inline int plan_quadtree_level(Planner& P, int l) {
    LevelDesc& D = P.p.g.lv[l];
    const int minB = 16, maxBX = D.w - 16, maxBY = D.h - 16;
    D.qtW = maxBX - minB; D.qtH = maxBY - minB;
    D.nIni = (int)std::round(static_cast<float>(D.qtW) / D.qtH);
    if (D.nIni < 1 || D.nIni > 16) return P.fail(ORBX_E_UNSUPPORTED, "aspect ratio of level %d unsupported (nIni=%d; the reference divides by zero for nIni=0)", l, D.nIni);
    D.hX = static_cast<float>(D.qtW) / D.nIni;
    D.selBase = P.totalSel;
    D.selCap = std::max(D.N + 3, 4 * D.nIni) + 1;
    P.totalSel += D.selCap;
    P.maxN = std::max(P.maxN, std::max(D.N, 4 * D.nIni));
    return 0;
}

// bytes of the quadrant histograms of depths fuseD + 1 .. D (u32, maxIni * 4^d entries at depth d)
static inline size_t qt_hist_bytes(int maxIni, int fuseD, int D) {
    size_t words = 0;
    for (int d = fuseD + 1; d <= D; ++d) words += (size_t)maxIni << (2 * d);
    return words * 4;
}

// the quadtree kernels' capacities, LDS sizes and fused depth, once every level is known
static inline int plan_quadtree(Planner& P) {
    Plan& p = P.p;
    Geom& g = p.g;
    const int L = g.nlevels, maxN = P.maxN;
    // maxN = max over the levels of max(N, 4 * nIni) (above): the first pass of DistributeOctTree splits every root before it looks at
    // N, so a level ends with up to 4 * nIni nodes whatever its budget.  k_quadtree (the A/B kernel) keeps the parents of a pass until
    // its end: at most nIni + 4 * nIni nodes in the first pass and N + (N + 3) later, both within 2 * maxN + 64 for every nIni
    g.nodeCap = 2 * maxN + 64;
    int sc = 1; while (sc < maxN + 8) sc <<= 1;
    g.sortCap = sc;
    if (g.nodeCap > 65000) return P.fail(ORBX_E_UNSUPPORTED, "nfeatures per level %d too large for 16-bit node ids", maxN);
    p.qtLds = (size_t)g.sortCap * 8 + (size_t)g.nodeCap * 56 + 64;
    {   // k_quadtree2: list capacity max(N+3, 4*nIni) (+slack), power-of-two sort buffer.  The 4 * nIni term is inside maxN, so a
        // wide frame with a small budget (six roots, N = 11: 24 nodes after the first pass) fits: tests/test_gpu_extract_second_reading.py
        p.qt2Cap = maxN + 8;
        int sc2 = 1; while (sc2 < p.qt2Cap) sc2 <<= 1;
        p.qt2Sort = sc2;
        p.maxCells = 0;
        for (int l = 0; l < L; ++l) p.maxCells = std::max(p.maxCells, g.lv[l].nCells);
        p.qtWide = P.cfg.qtWideForce >= 0 ? P.cfg.qtWideForce != 0 : maxN >= 512;   // many features per level: 1024-thread workgroups
        p.maxIni = 1;
        for (int l = 0; l < L; ++l) p.maxIni = std::max(p.maxIni, g.lv[l].nIni);
        // + the fused first iterations' histograms (4 + 16 + 64 (+ 256) words per root), path table and per-node paths.  A fourth fused
        // iteration only happens when some level wants more than ~512 nodes (128 + 3 * 128 <= N), and 12 path bits hold 16 roots * 4^4 / 16
        p.qtFuseD = (maxN >= 512 && p.maxIni <= 4) ? 4 : 3;
        const size_t hw = p.qtFuseD == 4 ? 340 : 84, tw = p.qtFuseD == 4 ? 256 : 64;
        p.qt2Lds = (size_t)sc2 * 8 + (size_t)p.qt2Cap * (16 * 2 + 16 + 4 + 4 + 8 + 2 + 1 + 1) + (size_t)(p.maxCells + 1) * 4 + 64 +
                   (size_t)p.maxIni * (hw * 4 + tw * 2) + (size_t)p.qt2Cap * 4 + 8;
        if (p.qt2Lds > 160 * 1024 - 512) return P.fail(ORBX_E_UNSUPPORTED, "quadtree for %d features/level needs %zu B of LDS (> 160 KiB)", maxN, p.qt2Lds);
        // depth of the deepest path histogram (table mode of k_quadtree2): the largest of fuseD .. fuseD + 2 that costs no LDS, so that
        // as many workgroups stay resident per CU as before.  The levels beyond fuseD overlay childPos / newPos (10 B per node), the
        // path table [maxIni * 4^D] of u16 overlays the sort keys, and a node's path | depth << 12 leaves the path 12 bits
        p.qtHistD = p.qtFuseD;
        for (int D = p.qtFuseD + 2; D > p.qtFuseD; --D) {
            const size_t paths = (size_t)p.maxIni << (2 * D);
            if (paths <= 4096 && qt_hist_bytes(p.maxIni, p.qtFuseD, D) <= (size_t)p.qt2Cap * 10 && paths * 2 <= (size_t)sc2 * 8) { p.qtHistD = D; break; }
        }
    }
    if (p.qtLds > 160 * 1024 - 512) return P.fail(ORBX_E_UNSUPPORTED, "quadtree for %d features/level needs %zu B of LDS (> 160 KiB)", maxN, p.qtLds);
    return 0;
}

// blur task lists and weights of level l
static inline void plan_blur(Planner& P, int l) {
    Plan& p = P.p;
    const LevelDesc& D = p.g.lv[l];
    // blur tasks: one wavefront per (248-px column strip, BL_R-row block); right-edge reflect-101 selectors
    {   // strips of output dwords: the first stores from lane 0 (63 dwords), the others from lane 1 (62), and a strip whose
        // lane 63 is the image's last dword stores that one too (k_blur2's doStore)
        const int gl = (D.w - 1) >> 2;
        for (int ty = 0; ty < D.h; ty += BL_R)
            for (int g0 = 0; g0 <= gl;) {
                p.tiles.push_back(BlurTask{(short)l, (short)g0, (short)ty, 0});
                const int lead = g0 > 0 ? 1 : 0;
                int lastOut = g0 - lead + 62;
                if (g0 - lead + 63 == gl) lastOut = gl;
                g0 = lastOut + 1;
            }
    }
    {   // k_blur3: one wavefront per 32-px column strip and chunk of up to B3_CHUNK 26-row tiles; weight fragments per
        // strip (pass 1, reflect-101 folded at the left / right edge) and per tile row (pass 2, folded at top / bottom)
        const int ntile = (D.h + B3_ROWS - 1) / B3_ROWS, nstrip = (D.w + 31) / 32;
        const int th0 = (int)(p.b3Th.size() / 512), tv0 = (int)(p.b3Tv.size() / 256);
        p.b3Th.resize(p.b3Th.size() + (size_t)nstrip * 512);
        p.b3Tv.resize(p.b3Tv.size() + (size_t)ntile * 256);
        for (int sx = 0; sx < nstrip; ++sx) b3_build_th(sx * 32, D.w, p.b3Th.data() + (size_t)(th0 + sx) * 512);
        for (int t = 0; t < ntile; ++t) b3_build_tv(t * B3_ROWS, D.h, p.b3Tv.data() + (size_t)(tv0 + t) * 256);
        for (int t0 = 0; t0 < ntile; t0 += B3_CHUNK)
            for (int sx = 0; sx < nstrip; sx += 4)                  // a workgroup = four adjacent strips
                p.tiles3.push_back(Blur3Task{(short)l, (short)(sx * 32), (short)t0, (short)std::min(B3_CHUNK, ntile - t0), th0 + sx, tv0 + t0});
        for (int t0 = 0; t0 < ntile; ++t0)
            for (int sx = 0; sx < nstrip; sx += 4)
                P.tiles3one.push_back(Blur3Task{(short)l, (short)(sx * 32), (short)t0, 1, th0 + sx, tv0 + t0});
    }
    {
        static const u32 kSelB[4] = {0x05060700u, 0x07000100u, 0x01020100u, 0x03020100u};   // k = (w-1)&3 valid bytes-1
        static const u32 kSelC[4] = {0x04040404u, 0x04040506u, 0x05060700u, 0x07000102u};
        const int k = (D.w - 1) & 3;
        p.blurSel.selB[l] = kSelB[k]; p.blurSel.selC[l] = kSelC[k];
    }
}

// resize taps from level l-1, the streaming kernel's x4 table, and whether the level can stream
static inline void plan_resize_taps(Planner& P, int l) {
    Plan& p = P.p;
    Geom& g = p.g;
    LevelDesc& D = g.lv[l];
    D.rzx = (int)p.xt.size(); D.rzy = (int)p.yt.size();
    if (l > 0) {
        const LevelDesc& S = g.lv[l - 1];
        const double scale_x = 1.0 / ((double)D.w / S.w), scale_y = 1.0 / ((double)D.h / S.h);
        auto sat = [](float v) { int r = (int)lrintf(v); return (short)std::min(32767, std::max(-32768, r)); };
        for (int dx = 0; dx < D.w; ++dx) {
            float fx = (float)((dx + 0.5) * scale_x - 0.5);
            int sx = (int)floorf(fx);
            fx -= sx;
            if (sx < 0) { fx = 0; sx = 0; }
            if (sx >= S.w - 1) { fx = 0; sx = S.w - 1; }
            p.xt.push_back(RzTab{sx, sat((1.f - fx) * 2048.f), sat(fx * 2048.f)});
        }
        for (int dy = 0; dy < D.h; ++dy) {
            float fy = (float)((dy + 0.5) * scale_y - 0.5);
            int sy = (int)floorf(fy);
            fy -= sy;
            p.yt.push_back(RzTab{sy, sat((1.f - fy) * 2048.f), sat(fy * 2048.f)});
        }
        // per-dword tables of the streaming kernel: it loads 8 bytes from the first tap, so every tap pair must start
        // within 6 bytes of it (true for scale factors up to 1.5; otherwise the level uses k_resize)
        while (p.x4.size() * 4 < (size_t)D.rzx) p.x4.push_back(RzX4{});
        bool ok = (D.rzx % 4) == 0 && S.w >= 8;
        for (int gx = 0; gx * 4 < D.w && ok; ++gx) {
            RzX4 e{};
            int sx[4];
            for (int i = 0; i < 4; ++i) {
                const int dx = std::min(gx * 4 + i, D.w - 1);
                const RzTab& tb = p.xt[D.rzx + dx];
                if (tb.s < 0 || tb.a0 < 0 || tb.a1 < 0) { ok = false; break; }
                if (tb.s + 1 < S.w) {
                    sx[i] = tb.s;
                    e.a[i] = (u32)(unsigned short)(2 * tb.a0) | ((u32)(unsigned short)(2 * tb.a1) << 16);   // doubled taps (<= 4096): k_resize2 keeps (H >> 4) << 5
                } else {                                           // clamped last column (a1 == 0): pair (w-2, w-1), weight on the second
                    sx[i] = tb.s - 1;
                    e.a[i] = (u32)(unsigned short)(2 * tb.a0) << 16;
                }
            }
            if (!ok) break;
            e.bs = *std::min_element(sx, sx + 4);
            for (int i = 0; i < 4; ++i) {
                const int off = sx[i] - e.bs;
                if (off < 0 || off > 6) { ok = false; break; }
                e.o[i] = (u8)off;
            }
            p.x4.push_back(e);
        }
        // rows: strictly increasing source rows without clamping, and a bounded source span per task
        for (int dy = 0; dy < D.h && ok; ++dy) {
            const int sy = p.yt[D.rzy + dy].s;
            if (sy < 0 || sy + 1 >= S.h || (dy > 0 && sy <= p.yt[D.rzy + dy - 1].s)) ok = false;
        }
        auto span_ok = [&](int R, int nsrcMax) {
            for (int ty = 0; ty < D.h; ty += R)
                if (p.yt[D.rzy + std::min(ty + R, D.h) - 1].s + 2 - p.yt[D.rzy + ty].s > nsrcMax) return false;
            return true;
        };
#ifdef ORBX_AB
        p.rzStreamP[l] = ok && span_ok(RZP_R, RZP_SRC);
        if (p.rzStreamP[l])
            for (int ty = 0; ty < D.h; ty += RZP_R)
                for (int gx = 0; gx * 4 < D.w; gx += 64) p.rzTasksP[l].push_back(RzTaskP{(short)l, (short)gx, (short)ty, 0});
#endif
        p.rzStream[l] = ok && span_ok(RZ_R, RZ_SRC);        // (its task records need the slab size: plan_resize_tasks)
    }
    while (p.xt.size() % 4) p.xt.push_back(RzTab{0, 0, 0});      // keep every level's tap offset a multiple of 4
}

// k_resize2's task records.  A level of ndw dwords has ndw / 64 full column tiles (a wave per tile and frame) and, for the
// remainder r = ndw % 64, one packed tile whose wave serves 64 / r consecutive frames.  The lanes of a packed wave reach their
// frames' slabs by 32-bit offsets from the first one's, so packing needs 64 slabs within 4 GiB; otherwise the tile keeps a frame per wave.
static inline void plan_resize_tasks(Planner& P) {
    Plan& p = P.p;
    const Geom& g = p.g;
    const int L = g.nlevels;
    for (int l = 1; l < L; ++l) {
        p.rzNFull[l] = p.rzNPack[l] = 0; p.rzPack[l] = 1;
        if (!p.rzStream[l]) continue;
        const LevelDesc &D = g.lv[l], &S = g.lv[l - 1];
        const int ndw = (D.w + 3) / 4, nfullTiles = ndw / 64, r = ndw % 64;
        bool canPack = (uint64_t)P.off * 64 <= (1ull << 32);
#ifdef ORBX_AB
        if (P.cfg.rzNoPack) canPack = false;
#endif
        const int pack = r && canPack ? 64 / r : 1;
        std::vector<RzTask> packed;
        for (int ty = 0; ty < D.h; ty += RZ_R) {
            RzTask t{};
            const int ye = std::min(ty + RZ_R, D.h);
            t.y0 = ty; t.sFirst = p.yt[D.rzy + ty].s; t.nsrc = p.yt[D.rzy + ye - 1].s + 2 - t.sFirst;
            for (int dy = ty; dy < ye; ++dy) {
                const RzTab& e = p.yt[D.rzy + dy];
                const int j = e.s + 1 - t.sFirst;                 // >= 1, distinct per dy (source rows strictly increase), < nsrc <= RZ_SRC
                t.emit |= 1u << j;
                t.taps[j] = (u32)(unsigned short)e.a0 | ((u32)(unsigned short)e.a1 << 16);
            }
            t.dpitch = D.pitch; t.doff = D.off; t.x4base = D.rzx / 4; t.spitch = S.pitch; t.soff = S.off;
            for (int tile = 0; tile < nfullTiles; ++tile) { t.g0 = tile * 64; t.pack = 1; t.gw = 64; t.gmul = 1024; p.rzTasks[l].push_back(t); }
            if (r) { t.g0 = nfullTiles * 64; t.pack = pack; t.gw = r; t.gmul = (65536 + r - 1) / r; packed.push_back(t); }
        }
        p.rzNFull[l] = (int)p.rzTasks[l].size(); p.rzNPack[l] = (int)packed.size(); p.rzPack[l] = pack;
        p.rzTasks[l].insert(p.rzTasks[l].end(), packed.begin(), packed.end());
        // the kernel divides a wave's index by a task count with one high multiply, exact while index * count < 2^32
        const uint64_t nmax = (uint64_t)p.rzTasks[l].size() * (uint64_t)P.cfg.maxBatch;
        if (nmax * (uint64_t)std::max(p.rzNFull[l], p.rzNPack[l]) >= (1ull << 32)) { p.rzStream[l] = false; p.rzTasks[l].clear(); }
    }
    for (int l = 0, n = 0; l < L; ++l) { p.rzTaskOff[l] = n; n += (int)p.rzTasks[l].size(); }   // the levels' records are uploaded as one list
#ifdef ORBX_AB
    for (int l = 0, n = 0; l < L; ++l) { p.rzTaskOffP[l] = n; n += (int)p.rzTasksP[l].size(); }
#endif
}

// FAST launch groups.  Boundaries: [level 0] [levels 1..k] [levels k+1..], k = the smallest level after which at most
// 15 % of the cells remain: the coarse levels have few cells, but the tallest cell rows (an image 102 rows high is
// cut into 2 cell rows of 51) and the densest corners, so they keep the worst-case queue.  The other groups bound the
// queue so that 7 workgroups fit a CU; a cell that overflows it is redone by k_fast_fix.
static inline int plan_fast_groups(Planner& P) {
    Plan& p = P.p;
    const Geom& g = p.g;
    const int nS = (int)p.strips.size();
    std::vector<int> cellsAfter(g.nlevels + 1, 0);
    for (int l = g.nlevels - 1; l >= 0; --l) cellsAfter[l] = cellsAfter[l + 1] + g.lv[l].nCells;
    int k = g.nlevels - 1;
    while (k > 0 && cellsAfter[k] * 100 <= 15 * g.totalCells) --k;      // levels > k hold <= 15 % of the cells
    int b0 = 0, b1 = 0;
    for (const StripInfo& stp : p.strips) { if (stp.level == 0) ++b0; if (stp.level <= k) ++b1; }
    const int bounds[4] = {0, b0, std::max(b0, b1), nS};
    size_t maxLds = 0;
    for (int gi = 0; gi < 3; ++gi) {
        F3Group G;
        G.strip0 = bounds[gi]; G.nstrips = bounds[gi + 1] - bounds[gi];
        if (G.nstrips <= 0) continue;
        int qworst = 64, maxLp = 0, maxH = 0;
        for (int si = G.strip0; si < G.strip0 + G.nstrips; ++si) {
            G.tile = std::max(G.tile, p.stripTile[si]); qworst = std::max(qworst, p.stripQ[si]);
            maxLp = std::max(maxLp, (int)p.strips[si].lp); maxH = std::max(maxH, (int)p.strips[si].h);
        }
        // one compile-time tile pitch for the whole group when its strips allow it (35..40-px cells, 4 per strip: <= 208 bytes)
        G.pitch = P.cfg.f3NoFixedPitch ? 0 : maxLp <= 176 ? 176 : maxLp <= 208 ? 208 : 0;
        // (>= 1 KiB: k_fast4 writes a fixed-pitch tile in wave-instructions of 64 x 16 bytes, a shorter strip as one of them)
        if (G.pitch) G.tile = std::max(G.pitch * maxH, 1024);
        G.tile = align_up(G.tile, 16);
        G.lastLevel = p.strips[G.strip0 + G.nstrips - 1].level;
        G.qcap = qworst;
        if (gi < 2) {
            const int wgs = P.cfg.fastWgs;
            const int budget = (160 * 1024 / wgs - 2 * G.tile) / (2 * (F3_NT / 64));
            G.qcap = std::min(qworst, std::max(wgs > 7 ? 256 : 512, budget / 64 * 64));
        } else {
            // coarse levels: dense corners (over half of a cell's pixels survive on the synthetic stream), so only a mild
            // bound -- 5 workgroups per CU instead of 4 -- and only if the queue still holds >= 3/4 of the worst case
            const int budget = (160 * 1024 / 5 - 2 * G.tile) / (2 * (F3_NT / 64));
            const int q5 = budget / 64 * 64;
            if (q5 < qworst && q5 * 4 >= qworst * 3) G.qcap = q5;
        }
        if (P.cfg.f3QcapForce > 0) G.qcap = std::min(G.qcap, align_up(P.cfg.f3QcapForce, 64));
        G.lds = (size_t)2 * G.tile + (size_t)(F3_NT / 64) * G.qcap * 2;
        G.lds += (size_t)P.cfg.fastLdsPad;
        if (G.lds > 160 * 1024 - 256) return P.fail(ORBX_E_UNSUPPORTED, "FAST strip needs %zu B of LDS", G.lds);
        maxLds = std::max(maxLds, G.lds);
        p.f3g.push_back(G);
    }
    p.fastLds = maxLds;
    // k_fast4 tables: per cell the scalars a wave needs, per distinct cell shape (pitch, window width, window height, column
    // phase) the lane -> (tile bytes, valid pixels, queue-entry base) list of every quick-pass iteration
    p.aux.assign(p.cells.size(), CellAux{});
    p.f4items.clear();
    std::map<std::array<int, 4>, u32> shapes;
    for (F3Group& G : p.f3g) {
        G.v4 = !P.cfg.fastV3;
        for (int si = G.strip0; si < G.strip0 + G.nstrips && G.v4; ++si) {
            const StripInfo& stp = p.strips[si];
            const int Pb = G.pitch ? G.pitch : (int)stp.lp;
            for (int k = 0; k < stp.ncell && G.v4; ++k) {
                const CellInfo& c = p.cells[stp.cell0 + k];
                CellAux& A = p.aux[stp.cell0 + k];
                A.slot = c.slot; A.cnt = c.cnt;
                const int cx0 = c.x0 + 3 - stp.xal, vw = c.cw - 6, vh = stp.h - 6;
                if (vw <= 0 || vh <= 0) { A.nit = 0; continue; }
                const int a = cx0 & 3, s4 = cx0 - a, ncol = (a + vw + 7) / 8, nitems = vh * ncol, nit = (nitems + 63) / 64;
                // limits of the 16-bit fields (entry: 7-bit row, 7-bit xs; item: 16-bit tile offset); beyond them the group stays on k_fast3
                if (ncol > 16 || vh > 127 || (vh - 1) * Pb + 8 * (ncol - 1) > 65535 || 3 * Pb + s4 > 65535 || s4 < 4) { G.v4 = false; break; }
                const std::array<int, 4> key = {Pb, vw, vh, a};
                auto itS = shapes.find(key);
                if (itS == shapes.end()) {
                    const u32 t0 = (u32)p.f4items.size();
                    p.f4items.resize(t0 + (size_t)nit * 64);
                    for (int i = 0; i < nit * 64; ++i) {
                        F4Item& I = p.f4items[t0 + i];
                        I.mask = 0; I.offq = 0;
                        if (i >= nitems) continue;                  // idle lane of the last iteration: reads (row 0, column 0), keeps nothing
                        const int row = i / ncol, col = i % ncol;
                        for (int px = 0; px < 8; ++px) { const int xs = 8 * col + px; if (xs >= a && xs < a + vw) I.mask |= 1u << (4 * px + 3); }
                        I.offq = (u32)(row * Pb + 8 * col) | ((u32)((row << 9) | (col << 5)) << 16);
                    }
                    itS = shapes.emplace(key, t0).first;
                }
                A.tab = itS->second;
                A.base = (u16)(3 * Pb + s4); A.nit = (u16)nit;
                A.outx = (short)(c.x0 + 3 - 16 - a); A.outy = (short)(stp.y0 + 3 - 16);
                A.xlo = (u16)a; A.xhi = (u16)(a + vw - 1);
            }
        }
    }
    if (p.f4items.size() < 64) p.f4items.resize(64, F4Item{0, 0});    // (k_fast4's waves without a cell read one iteration of table 0)
    return 0;
}

// The plan of a w x h image.  Returns 0, or an ORBX_E_* code with its text in err; `out` is then incomplete and must not be used.
static inline int plan_geometry(const PlanConfig& cfg, const ExtractorTables& tab, int w, int h, Plan& out, char* err, size_t errlen) {
    out = Plan();
    Planner P{cfg, tab, out, err, errlen};
    Geom& g = out.g;
    memset(&g, 0, sizeof g);                               // (padding too: the block is passed to the kernels by value)
    const int L = cfg.nlevels;
    g.nlevels = L; g.w0 = w; g.h0 = h; g.iniTh = cfg.iniTh; g.minTh = cfg.minTh; g.lowTh = std::min(cfg.iniTh, cfg.minTh);
    for (int l = 0; l < L; ++l) {
        if (int rc = plan_level(P, l)) return rc;
        if (int rc = plan_cells(P, l)) return rc;
        if (int rc = plan_quadtree_level(P, l)) return rc;
        plan_blur(P, l);
        plan_resize_taps(P, l);
    }
    g.pyrFrameBytes = P.off;
    plan_resize_tasks(P);
    g.blurTiled = cfg.blurTiled ? 1 : 0;
    g.blrFrameBytes = cfg.blurTiled ? P.boff : P.off;
    g.totalCells = (int)out.cells.size();
    g.totalSlots = P.totalSlots;
    g.totalSel = P.totalSel;
    g.kpCap = P.totalSel;
    if (int rc = plan_quadtree(P)) return rc;
    out.algBytes = P.sumSrc + P.sumDst + P.sumAll;      // read L0..L6 + write L1..L7 + read L0..L7
    out.fusedBytes = P.sumSrc + P.sumDst;
    out.l0pitch = align_up(w, 64);
    out.nTiles3Walk = out.tiles3.size();
    out.tiles3.insert(out.tiles3.end(), P.tiles3one.begin(), P.tiles3one.end());
    return plan_fast_groups(P);
}

// ---- per launch: pure functions of the plan and the batch size
// k_resize2's launch record of level l: a flat list of waves, full tiles x frames, then packed remainder tiles x groups of `pack` frames
static inline RzLaunch rz_launch(const Plan& p, int l, int nimg) {
    RzLaunch R;
    R.nFull = (u32)p.rzNFull[l]; R.nPack = (u32)p.rzNPack[l]; R.nimg = (u32)nimg;
    R.nFullW = R.nFull * R.nimg;
    R.nWaves = R.nFullW + R.nPack * (u32)((nimg + p.rzPack[l] - 1) / p.rzPack[l]);
    R.mFull = R.nFull > 1 ? (u32)((1ull << 32) / R.nFull) + 1u : 0u;
    R.mPack = R.nPack > 1 ? (u32)((1ull << 32) / R.nPack) + 1u : 0u;
    return R;
}
// k_blur3's form.  Big batches: workgroups walk B3_CHUNK tiles (prologue amortised); small ones: one tile per workgroup (8x the
// workgroups, an eighth of the latency -- the single-frame path).  force: -1, or 0 / 1 for the one-tile / walking form
static inline bool blur_walks(const Plan& p, int nimg, int force) {
    return force >= 0 ? force != 0 : (size_t)nimg * p.nTiles3Walk >= 2048;
}
// k_quadtree2's form.  Few workgroups (small batches, the single-frame call): the kernel's time is one workgroup's latency, and 1024
// threads walk a level's candidates four times faster than 256 (one frame: 0.276 -> 0.237 ms end to end); many workgroups: 256 threads
// (shorter barriers, more workgroups per CU: 0.24 vs 0.56 ms per 512 frames).  force: PlanConfig::qtWideForce, already inside p.qtWide
static inline bool qt_wide(const Plan& p, int nimg, int nlevels, int force) {
    return force >= 0 ? p.qtWide : (p.qtWide || nimg * nlevels <= 512);
}

}  // namespace orbxk
