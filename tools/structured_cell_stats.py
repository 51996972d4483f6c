#!/usr/bin/env python3
"""Which FAST routes the structured test images (tests/structured_images.py) walk, counted with the CPU oracle and numpy alone:
per kind at 752x480 / 1000 features / default parameters, over the cells of the 8 levels,
  overflow: cells whose quick-test survivors outnumber the queue a wave of k_fast4 has for them (redone by k_fast_fix), per level;
            the capacity is restated from the host code that sizes it (structured_images.fast_queue_caps: 960 entries on levels 0-3
            at this size, the cells' worst case on levels 4-7) -- derived from the code, not read from the device,
  retry:    cells without a corner at iniTh, run again at minTh (ORBextractor.cc:1118-1125).
    tools/structured_cell_stats.py > profiles/rNN_structured_cell_stats.txt"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import orbref
import structured_images as si

first = True
for kind, params in [("textured", {}), ("sparse", {}), ("lowcontrast", {})] + si.STRUCTURED:
    ref = orbref.Extractor(1000)
    n = ref(si.gen(kind, 752, 480, 7, **params), (0, 0))[0]
    r = si.cell_routes(ref)
    if first:
        print("cells per level      %s" % " ".join("%4d" % x[0] for x in r))
        print("queue entries        %s" % " ".join("%4d" % x[3] for x in r))
        print("%-42s %5s %8s %5s %9s   %s" % ("kind", "cells", "overflow", "retry", "keypoints", "overflow cells on levels 0..7"))
        first = False
    name = kind + "".join(" %s=%s" % kv for kv in sorted(params.items()))
    print("%-42s %5d %8d %5d %9d   %s" % (name, sum(x[0] for x in r), sum(x[1] for x in r), sum(x[2] for x in r), n, " ".join("%3d" % x[1] for x in r)))
