// The binary form of a CreateNewMapPoints case (tests/triangulate_io.py: write_case) as the C++ test programs read it.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

struct Pool {
    int rows = 0, cap = 0;
    std::vector<float> ux, uy, kx, ky, uright, depth, tcw, ow;
    std::vector<int32_t> octave, counts;
};
template <class T> static inline bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static inline void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }
static inline bool read_pool(FILE* f, Pool& p) {
    const size_t s = (size_t)p.rows * p.cap;
    return rd(f, p.ux, s) && rd(f, p.uy, s) && rd(f, p.octave, s) && rd(f, p.kx, s) && rd(f, p.ky, s) && rd(f, p.counts, p.rows) &&
           rd(f, p.uright, s) && rd(f, p.depth, s) && rd(f, p.tcw, (size_t)12 * p.rows) && rd(f, p.ow, (size_t)3 * p.rows);
}
struct TriCase {
    int ng = 0, npairs = 0, nl = 0;
    Pool a, b;
    std::vector<int32_t> gs, row1, row2, m12;
    std::vector<float> fl, sf1, ls1, sf2, ls2;      // fl: k1 [6], k2 [6], mb1, mbf1, mb2, ratio_factor, th_far
};
static inline bool read_case(const char* path, TriCase& c) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int32_t h[8];
    bool ok = fread(h, sizeof(int32_t), 8, f) == 8;
    if (ok) {
        c.ng = h[0]; c.npairs = h[1]; c.nl = h[6];
        c.a.rows = h[2]; c.a.cap = h[3]; c.b.rows = h[4]; c.b.cap = h[5];
        ok = c.ng >= 0 && c.npairs >= 0 && c.a.rows >= 0 && c.b.rows >= 0 && c.a.cap >= 1 && c.b.cap >= 1 && c.nl >= 1 && c.nl <= 32;
    }
    ok = ok && rd(f, c.gs, c.ng + 1) && rd(f, c.row1, c.npairs) && rd(f, c.row2, c.npairs) && rd(f, c.m12, (size_t)c.npairs * c.a.cap) && read_pool(f, c.a) &&
         read_pool(f, c.b) && rd(f, c.fl, 17) && rd(f, c.sf1, c.nl) && rd(f, c.ls1, c.nl) && rd(f, c.sf2, c.nl) && rd(f, c.ls2, c.nl);
    fclose(f);
    return ok;
}
