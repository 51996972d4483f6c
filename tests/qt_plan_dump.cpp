// The quadtree part of the extractor's host planner (orb-slam3_amd/csrc/orbx_plan.h: plan_quadtree) on the CPU, for
// tests/test_quadtree_table_cases_cpu.py.  No HIP anywhere.
// Input (stdin), one configuration per line:  w h nfeatures scale_factor nlevels max_batch   (iniTh 20, minTh 7, no A/B knob)
// Output, one line per configuration:  rc qtFuseD qtHistD qt2Lds qt2Cap qt2Sort maxIni maxCells
// and, for D = qtFuseD .. qtFuseD + 2, the bytes k_quadtree2 would lay over other arrays:  hist(D) td(D)
// (hist: histogram levels beyond qtFuseD, on childPos / newPos = 10 * qt2Cap bytes; td: the path table, on the sort keys = 8 * qt2Sort).
#include <cstdio>
#include "../orb-slam3_amd/csrc/orbx_plan.h"

using namespace orbxk;

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        PlanConfig c;
        int w, h;
        float sf;
        if (sscanf(line, "%d %d %d %f %d %d", &w, &h, &c.nfeatures, &sf, &c.nlevels, &c.maxBatch) != 6) continue;
        c.scaleFactor = sf; c.maxW = w; c.maxH = h; c.iniTh = 20; c.minTh = 7;
        const ExtractorTables tab = plan_tables(c);
        Plan p;
        char err[512] = "";
        const int rc = plan_geometry(c, tab, w, h, p, err, sizeof err);
        printf("%d %d %d %zu %d %d %d %d", rc, p.qtFuseD, p.qtHistD, p.qt2Lds, p.qt2Cap, p.qt2Sort, p.maxIni, p.maxCells);
        for (int D = p.qtFuseD; D <= p.qtFuseD + 2; ++D)
            printf(" %zu %zu", qt_hist_bytes(p.maxIni, p.qtFuseD, D), ((size_t)p.maxIni << (2 * D)) * 2);
        printf("\n");
    }
    return 0;
}
