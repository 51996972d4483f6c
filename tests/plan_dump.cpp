// Runs the extractor's host planner (orb-slam3_amd/csrc/orbx_plan.h: plan_tables, plan_geometry, rz_launch, blur_walks, qt_wide) on the CPU,
// exactly as orbx_create / build_geometry call it, and prints what tests/test_plan_cpu.py asserts.  No HIP anywhere.
// Input (stdin), one configuration per line:
//   w h nfeatures scale_factor nlevels ini_th min_th max_batch  blurTiled fastV3 noFixedPitch qcapForce qtWideForce fastWgs fastLdsPad rzNoPack
// (scale_factor is read as a float, as the ABI takes it; rzNoPack is ignored without -DORBX_AB.)
// Output: one JSON line per configuration -- return code and error text; the constructor tables (floats as their bit patterns); Geom and
// its levels; cells, strips and FAST groups as flat integer lists; and, where the tables are large, what a walk over them finds:
// per k_fast4 shape the pixels its items' mask bits select, per streamed resize level the destination coverage of its task records and
// the exactness of the multiply-high division, per level the coverage of k_blur3's two task lists and the sums of its weights.
// "hash" is FNV-1a over Geom and every host table and scalar of the plan, in the order of plan_hash() below.
#include <cinttypes>
#include <cstdio>
#include <string>
#include "../orb-slam3_amd/csrc/orbx_plan.h"

using namespace orbxk;

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const void* p, size_t n) { const u8* b = (const u8*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } }
    template <class T> void val(const T& v) { add(&v, sizeof v); }
    template <class T> void vec(const std::vector<T>& v) { const uint64_t n = v.size(); val(n); if (n) add(v.data(), n * sizeof(T)); }
};
// S: anything that names the plan's members as Plan does
template <class S> static uint64_t plan_hash(const S& s, int L, size_t fastLds) {
    Fnv f;
    f.add(&s.g, sizeof(Geom));
    f.vec(s.cells); f.vec(s.strips); f.vec(s.stripTile); f.vec(s.stripQ);
    for (const auto& G : s.f3g) { f.val(G.strip0); f.val(G.nstrips); f.val(G.tile); f.val(G.qcap); f.val(G.lastLevel); f.val(G.pitch); f.val((uint64_t)G.lds); f.val((int)G.v4); }
    f.val((uint64_t)fastLds);
    f.vec(s.aux); f.vec(s.f4items); f.vec(s.xt); f.vec(s.yt); f.vec(s.x4);
    for (int l = 0; l < L; ++l) { f.vec(s.rzTasks[l]); f.val(s.rzTaskOff[l]); f.val((int)s.rzStream[l]); f.val(s.rzNFull[l]); f.val(s.rzNPack[l]); f.val(s.rzPack[l]); }
    f.vec(s.tiles); f.vec(s.tiles3); f.val((uint64_t)s.nTiles3Walk); f.vec(s.b3Th); f.vec(s.b3Tv);
    for (int l = 0; l < L; ++l) { f.val(s.blurSel.selB[l]); f.val(s.blurSel.selC[l]); }
    f.val((int64_t)s.algBytes); f.val((int64_t)s.fusedBytes); f.val((uint64_t)s.qtLds); f.val((uint64_t)s.qt2Lds);
    f.val(s.qtFuseD); f.val(s.maxIni); f.val(s.qt2Cap); f.val(s.qt2Sort); f.val(s.maxCells); f.val((int)s.qtWide); f.val(s.l0pitch);
    return f.h;
}

static std::string J;                                            // the line being written
static void jf(const char* fmt, ...) {
    char b[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    J += b;
}
static void key(const char* k) { if (J.back() != '{' && J.back() != '[') J += ','; jf("\"%s\":", k); }
template <class T> static void jnum(T v) { if (J.back() != '[' && J.back() != ':') J += ','; jf("%lld", (long long)v); }
template <class It> static void jarr(const char* k, It b, It e) { key(k); J += '['; for (; b != e; ++b) jnum(*b); J += ']'; }
static u32 bits(float v) { u32 u; memcpy(&u, &v, 4); return u; }
static void jbits(const char* k, const std::vector<float>& v) { key(k); J += '['; for (float x : v) jnum(bits(x)); J += ']'; }

static void dump(const PlanConfig& cfg, int w, int h) {
    const ExtractorTables tab = plan_tables(cfg);
    Plan p;
    char err[512] = "";
    const int rc = plan_geometry(cfg, tab, w, h, p, err, sizeof err);
    J = "{";
    key("rc"); jnum(rc);
    key("err"); J += '"'; for (const char* c = err; *c; ++c) { if (*c == '"' || *c == '\\') J += '\\'; J += *c; } J += '"';
    key("tab"); J += '{';
    jbits("sf", tab.sf); jbits("invsf", tab.invsf); jbits("sig2", tab.sig2); jbits("invsig2", tab.invsig2);
    jarr("nfeat", tab.nfeat.begin(), tab.nfeat.end()); jarr("umax", tab.umax.v, tab.umax.v + 16); jarr("odW", tab.odW.begin(), tab.odW.end());
    J += '}';
    if (rc) { J += '}'; puts(J.c_str()); return; }
    const Geom& g = p.g;
    const int L = g.nlevels;
    key("hash"); jf("\"%016" PRIx64 "\"", plan_hash(p, L, p.fastLds));
    {
        const long long v[] = {g.nlevels, g.w0, g.h0, g.iniTh, g.minTh, g.lowTh, g.totalCells, g.totalSlots, g.totalSel, g.kpCap, g.nodeCap, g.sortCap,
                               (long long)g.pyrFrameBytes, (long long)g.blrFrameBytes, g.blurTiled};
        jarr("g", v, v + 15);
    }
    key("lv"); J += '[';
    for (int l = 0; l < L; ++l) {
        const LevelDesc& D = g.lv[l];
        const long long v[] = {D.w, D.h, D.pitch, D.off, D.boff, D.btpr, D.rzx, D.rzy, D.cellBase, D.nCells, D.slotBase, D.slotCap, D.N, D.nIni, D.qtW, D.qtH,
                               bits(D.hX), D.selBase, D.selCap, bits(D.sf), bits(D.patch)};
        if (l) J += ',';
        J += '['; for (long long x : v) jnum(x); J += ']';
    }
    J += ']';
    // cells, and how often each pixel of a level is inside a cell's evaluated window [x0 + 3, x0 + cw - 3) x [y0 + 3, y0 + ch - 3)
    key("cells"); J += '[';
    for (const CellInfo& c : p.cells) { const int v[] = {c.level, c.x0, c.y0, c.cw, c.ch, c.addx, c.addy, c.pad, c.slot, c.cnt}; for (int x : v) jnum(x); }
    J += ']';
    {
        std::vector<long long> bad(L, 0);
        for (int l = 0; l < L; ++l) {
            const LevelDesc& D = g.lv[l];
            std::vector<u8> cov((size_t)D.w * D.h, 0);
            for (int ci = D.cellBase; ci < D.cellBase + D.nCells; ++ci) {
                const CellInfo& c = p.cells[ci];
                for (int y = c.y0 + 3; y < c.y0 + c.ch - 3; ++y)
                    for (int x = c.x0 + 3; x < c.x0 + c.cw - 3; ++x) {
                        if (x < 0 || y < 0 || x >= D.w || y >= D.h) { ++bad[l]; continue; }
                        ++cov[(size_t)y * D.w + x];
                    }
            }
            for (int y = 0; y < D.h; ++y)
                for (int x = 0; x < D.w; ++x) {
                    const bool in = x >= 19 && x < D.w - 19 && y >= 19 && y < D.h - 19;
                    if (cov[(size_t)y * D.w + x] != (in ? 1 : 0)) ++bad[l];
                }
        }
        jarr("cell_cover_bad", bad.begin(), bad.end());
    }
    key("strips"); J += '[';
    for (const StripInfo& s : p.strips) { const int v[] = {s.level, s.ncell, s.x0, s.y0, s.w, s.h, s.xal, s.lp, s.cell0}; for (int x : v) jnum(x); }
    J += ']';
    jarr("stripTile", p.stripTile.begin(), p.stripTile.end()); jarr("stripQ", p.stripQ.begin(), p.stripQ.end());
    key("f3g"); J += '[';
    for (const F3Group& G : p.f3g) { const long long v[] = {G.strip0, G.nstrips, G.tile, G.qcap, G.lastLevel, G.pitch, (long long)G.lds, G.v4}; for (long long x : v) jnum(x); }
    J += ']';
    key("fastLds"); jnum(p.fastLds);
    {   // k_fast4: per cell the scalars recomputed in plain ints against the record's 16-bit fields; per distinct table the decoded items
        long long cellBad = 0, cellsV4 = 0;
        std::map<u32, std::array<int, 5>> tabs;                  // first item -> (pitch, vw, vh, a, nit)
        for (const F3Group& G : p.f3g) {
            if (!G.v4) continue;
            for (int si = G.strip0; si < G.strip0 + G.nstrips; ++si) {
                const StripInfo& s = p.strips[si];
                const int Pb = G.pitch ? G.pitch : (int)s.lp;
                for (int k = 0; k < s.ncell; ++k) {
                    const CellInfo& c = p.cells[s.cell0 + k];
                    const CellAux& A = p.aux[s.cell0 + k];
                    ++cellsV4;
                    const int cx0 = c.x0 + 3 - s.xal, vw = c.cw - 6, vh = s.h - 6;
                    if (A.slot != c.slot || A.cnt != c.cnt) ++cellBad;
                    if (vw <= 0 || vh <= 0) { if (A.nit != 0) ++cellBad; continue; }
                    const int a = cx0 & 3, s4 = cx0 - a, ncol = (a + vw + 7) / 8;
                    const bool ok = (int)A.base == 3 * Pb + s4 && (int)A.xlo == a && (int)A.xhi == a + vw - 1 && a + vw - 1 < 128 && vh <= 127 &&
                                    (int)A.nit * 64 >= vh * ncol && (int)A.outx == c.x0 + 3 - 16 - a && (int)A.outy == s.y0 + 3 - 16 &&
                                    (size_t)A.tab + (size_t)A.nit * 64 <= p.f4items.size() && s4 >= 4;
                    if (!ok) ++cellBad;
                    const std::array<int, 5> shape = {Pb, vw, vh, a, (int)A.nit};
                    auto it = tabs.find(A.tab);
                    if (it == tabs.end()) tabs.emplace(A.tab, shape);
                    else if (it->second != shape) ++cellBad;   // two shapes on one table
                }
            }
        }
        key("f4_cells"); jnum(cellsV4); key("f4_cell_bad"); jnum(cellBad); key("f4_items"); jnum(p.f4items.size());
        key("f4_shapes"); J += '[';                              // pitch, vw, vh, a, nit, pixels selected, selected twice, outside the window, offq halves that disagree
        for (const auto& kv : tabs) {
            const int Pb = kv.second[0], vw = kv.second[1], vh = kv.second[2], a = kv.second[3], nit = kv.second[4];
            std::vector<u8> cov((size_t)vw * vh, 0);
            long long npix = 0, dup = 0, outside = 0, offqBad = 0;
            for (int i = 0; i < nit * 64; ++i) {
                const F4Item& I = p.f4items[kv.first + i];
                const u32 lo = I.offq & 0xffffu, hi = I.offq >> 16;
                const int row = (int)(hi >> 9), col = (int)((hi >> 5) & 15);
                if ((hi & 31u) != 0 || (long long)lo != (long long)row * Pb + 8 * col) ++offqBad;
                if (I.mask & ~0x88888888u) ++offqBad;
                for (int px = 0; px < 8; ++px) {
                    if (!(I.mask >> (4 * px + 3) & 1u)) continue;
                    const int xs = 8 * col + px;
                    if (xs < a || xs >= a + vw || row >= vh) { ++outside; continue; }
                    ++npix;
                    if (cov[(size_t)row * vw + xs - a]++) ++dup;
                }
            }
            const long long v[] = {Pb, vw, vh, a, nit, npix, dup, outside, offqBad};
            for (long long x : v) jnum(x);
        }
        J += ']';
    }
    // resize: per destination level
    key("rz"); J += '[';
    for (int l = 1; l < L; ++l) {
        const LevelDesc& D = g.lv[l];
        const int ndw = (D.w + 3) / 4;
        long long coverBad = 0, ytBad = 0, fieldBad = 0, mulhiBad = 0, x4max = 0;
        int nsrcMin = 1 << 30, nsrcMax = 0, rr = 0;
        const RzLaunch R = rz_launch(p, l, cfg.maxBatch);
        if (p.rzStream[l]) {
            std::vector<u8> cov((size_t)D.h * ndw, 0);
            const std::vector<RzTask>& T = p.rzTasks[l];
            for (size_t ti = 0; ti < T.size(); ++ti) {
                const RzTask& t = T[ti];
                const bool full = (int)ti < p.rzNFull[l];
                if (full ? (t.pack != 1 || t.gw != 64 || t.gmul != 1024) : (t.pack != p.rzPack[l] || t.gw != ndw % 64 || t.gmul != (65536 + t.gw - 1) / t.gw)) ++fieldBad;
                if (!full) rr = t.gw;
                if (t.pack * t.gw > 64 || t.dpitch != D.pitch || t.doff != D.off || t.x4base != D.rzx / 4 || t.spitch != g.lv[l - 1].pitch || t.soff != g.lv[l - 1].off || (t.emit & 1u)) ++fieldBad;
                for (int lane = 0; lane < 64; ++lane) if ((int)(((u32)lane * (u32)t.gmul) >> 16) != lane / t.gw) ++fieldBad;
                nsrcMin = std::min(nsrcMin, t.nsrc); nsrcMax = std::max(nsrcMax, t.nsrc);
                int dy = t.y0;
                for (int j = 0; j < 32; ++j) {
                    if (!(t.emit >> j & 1u)) continue;
                    if (j >= t.nsrc || j >= 16 || dy >= D.h) { ++ytBad; continue; }
                    const RzTab& e = p.yt[D.rzy + dy];
                    if (e.s != t.sFirst + j - 1 || t.taps[j] != ((u32)(unsigned short)e.a0 | ((u32)(unsigned short)e.a1 << 16))) ++ytBad;
                    for (int gx = t.g0; gx < t.g0 + t.gw; ++gx) {
                        if (gx >= ndw) { ++coverBad; continue; }
                        ++cov[(size_t)dy * ndw + gx];
                    }
                    ++dy;
                }
            }
            for (u8 c : cov) if (c != 1) ++coverBad;
            for (int gx = 0; gx < ndw; ++gx) for (int i = 0; i < 4; ++i) x4max = std::max<long long>(x4max, p.x4[D.rzx / 4 + gx].o[i]);
            // the kernel's division of a wave's index by the task count (k_resize2: fq = umulhi(wq, m)), for every wave of the largest batch
            for (u32 wq = 0; wq < R.nFullW; ++wq) if (R.nFull > 1 && (u32)(((uint64_t)wq * R.mFull) >> 32) != wq / R.nFull) ++mulhiBad;
            for (u32 wq = 0; wq < R.nWaves - R.nFullW; ++wq) if (R.nPack > 1 && (u32)(((uint64_t)wq * R.mPack) >> 32) != wq / R.nPack) ++mulhiBad;
        }
        const long long v[] = {p.rzStream[l], p.rzNFull[l], p.rzNPack[l], p.rzPack[l], rr, nsrcMin, nsrcMax, x4max, coverBad, ytBad, fieldBad, mulhiBad,
                               R.nWaves, p.rzTaskOff[l], (long long)p.rzTasks[l].size(),
#ifdef ORBX_AB
                               p.rzStreamP[l], p.rzTaskOffP[l], (long long)p.rzTasksP[l].size()
#else
                               -1, -1, -1
#endif
        };
        if (l > 1) J += ',';
        J += '['; for (long long x : v) jnum(x); J += ']';
    }
    J += ']';
    {   // k_blur3: both task lists against the (column group, tile) grid of every level; weight sums of both passes
        long long walkBad = 0, oneBad = 0, rangeBad = 0, sumBad = 0;
        int th0 = 0, tv0 = 0;
        std::vector<int> lvTh(L), lvTv(L);
        for (int l = 0; l < L; ++l) { lvTh[l] = th0; lvTv[l] = tv0; th0 += (g.lv[l].w + 31) / 32; tv0 += (g.lv[l].h + B3_ROWS - 1) / B3_ROWS; }
        if ((size_t)th0 * 512 != p.b3Th.size() || (size_t)tv0 * 256 != p.b3Tv.size()) ++rangeBad;
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<std::vector<u8>> cov(L);
            for (int l = 0; l < L; ++l) cov[l].assign((size_t)((g.lv[l].w + 127) / 128) * ((g.lv[l].h + B3_ROWS - 1) / B3_ROWS), 0);
            const size_t b = pass ? p.nTiles3Walk : 0, e = pass ? p.tiles3.size() : p.nTiles3Walk;
            long long& bad = pass ? oneBad : walkBad;
            for (size_t i = b; i < e; ++i) {
                const Blur3Task& t = p.tiles3[i];
                if (t.level < 0 || t.level >= L) { ++bad; continue; }
                const LevelDesc& D = g.lv[t.level];
                const int ntile = (D.h + B3_ROWS - 1) / B3_ROWS, nstrip = (D.w + 31) / 32, ngrp = (D.w + 127) / 128;
                if (t.x0 % 128 || t.x0 / 128 >= ngrp || t.nt < 1 || t.nt > (pass ? 1 : B3_CHUNK) || t.t0 < 0 || t.t0 + t.nt > ntile) { ++bad; continue; }
                if (t.th != lvTh[t.level] + t.x0 / 32 || t.th >= lvTh[t.level] + nstrip || t.tv != lvTv[t.level] + t.t0) ++rangeBad;
                for (int k = 0; k < t.nt; ++k) ++cov[t.level][(size_t)(t.t0 + k) * ngrp + t.x0 / 128];
            }
            for (int l = 0; l < L; ++l) for (u8 c : cov[l]) if (c != 1) ++bad;
        }
        for (int l = 0; l < L; ++l) {
            const LevelDesc& D = g.lv[l];
            for (int sx = 0; sx * 32 < D.w; ++sx) {
                const u32* T = p.b3Th.data() + (size_t)(lvTh[l] + sx) * 512;
                for (int r = 0; r < 32 && sx * 32 + r < D.w; ++r) {
                    int sum = 0;
                    for (int s = 0; s < 2; ++s) for (int hh = 0; hh < 2; ++hh) for (int e = 0; e < 4; ++e) for (int b = 0; b < 4; ++b) sum += (T[(s * 64 + hh * 32 + r) * 4 + e] >> (8 * b)) & 255u;
                    if (sum != 256) ++sumBad;
                }
            }
            for (int t = 0; t * B3_ROWS < D.h; ++t) {
                const u32* T = p.b3Tv.data() + (size_t)(lvTv[l] + t) * 256;
                for (int r = 0; r < B3_ROWS && t * B3_ROWS + r < D.h; ++r) {
                    int sum = 0;
                    for (int hh = 0; hh < 2; ++hh) for (int e = 0; e < 4; ++e) for (int b = 0; b < 4; ++b) sum += (T[(hh * 32 + r) * 4 + e] >> (8 * b)) & 255u;
                    if (sum != 256) ++sumBad;
                }
            }
        }
        const long long v[] = {(long long)p.nTiles3Walk, (long long)(p.tiles3.size() - p.nTiles3Walk), walkBad, oneBad, rangeBad, sumBad, (long long)p.tiles.size()};
        jarr("blur", v, v + 7);
        jarr("selB", p.blurSel.selB, p.blurSel.selB + L); jarr("selC", p.blurSel.selC, p.blurSel.selC + L);
    }
    {
        const long long v[] = {(long long)p.qtLds, (long long)p.qt2Lds, p.qtFuseD, p.maxIni, p.qt2Cap, p.qt2Sort, p.maxCells, p.qtWide, p.l0pitch, p.algBytes, p.fusedBytes};
        jarr("qt", v, v + 11);
        const long long d[] = {qt_wide(p, 1, L, cfg.qtWideForce), qt_wide(p, cfg.maxBatch, L, cfg.qtWideForce), qt_wide(p, 512 / L + 1, L, cfg.qtWideForce),
                               blur_walks(p, 1, -1), blur_walks(p, cfg.maxBatch, -1), blur_walks(p, 1, 1), blur_walks(p, cfg.maxBatch, 0)};
        jarr("launch", d, d + 7);
    }
    J += '}';
    puts(J.c_str());
}

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        PlanConfig c;
        int w, h, blurTiled, fastV3, noFixed, rzNoPack;
        float sf;
        if (sscanf(line, "%d %d %d %f %d %d %d %d %d %d %d %d %d %d %d %d", &w, &h, &c.nfeatures, &sf, &c.nlevels, &c.iniTh, &c.minTh, &c.maxBatch,
                   &blurTiled, &fastV3, &noFixed, &c.f3QcapForce, &c.qtWideForce, &c.fastWgs, &c.fastLdsPad, &rzNoPack) != 16) continue;
        c.scaleFactor = sf; c.maxW = w; c.maxH = h;
        c.blurTiled = blurTiled != 0; c.fastV3 = fastV3 != 0; c.f3NoFixedPitch = noFixed != 0;
#ifdef ORBX_AB
        c.rzNoPack = rzNoPack != 0;
#endif
        dump(c, w, h);
    }
    return 0;
}
