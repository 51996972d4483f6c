"""Timing of the batched SearchForInitialization (M9 orbm_search_for_initialization_batch_async) against the loop of host calls
(orbm_search_for_initialization) it replaces, on the same inputs, medians (host clock round enqueue + sync; the batch also by the
handle's device events): each side alone, then interleaved on one handle and on two handles.

    python tools/init_batch.py [--reps 15] [--out profiles/init_batch.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/init_batch.py --batch-only --pairs 8

Shapes: 752 x 480 / 5 000 features for P = 1, 8, 64 pairs and 376 x 240 / 2 500 features for P = 8.  The P pairs of a shape are the
same (initial, current) frame pair in P rows, so the host loop and the batch do the same work per pair; the rows and counts of the
two are compared before anything is timed."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true", help="only the batch calls (for a kernel trace of its own)")
    ap.add_argument("--pairs", type=int, default=0, help="only the 752 x 480 shape with this many pairs")
    a = ap.parse_args()
    pkg = importlib.import_module("orb-slam3_amd")
    synth = importlib.import_module("orb-slam3_amd.synth")
    import orbref
    L = pkg.lib()
    mt = pkg.ORBmatcher(0.9)                      # the batch's handle
    mh = pkg.ORBmatcher(0.9)                      # the host calls' handle in the "two handles" columns
    out = []
    shapes = ((752, 480, 5000, (a.pairs,)),) if a.pairs else ((752, 480, 5000, (1, 8, 64)), (376, 240, 2500, (8,)))
    for (w, h, nf, plist) in shapes:
        l, r = synth.gen_stereo_pair(w, h, 321)
        ex = orbref.Extractor(nf)
        _, k1, d1, _ = ex(l, (0, 1000)); _, k2, d2, _ = ex(r, (0, 1000))
        inv_w, inv_h = np.float32(64) / np.float32(w), np.float32(48) / np.float32(h)
        prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
        v1 = pkg.FrameView(k1, d1, w, h, backend=mt); v2 = pkg.FrameView(k2, d2, w, h, backend=mt)
        n_h, m_h, p_h = mt.SearchForInitialization(v1, v2, prev, 100, 0.9, True)
        cap1, cap2 = len(k1) + 16, len(k2) + 16
        for P in plist:
            K1 = np.zeros((P, cap1), pkg.KP_DTYPE); D1 = np.zeros((P, cap1, 32), np.uint8); K1[:, :len(k1)] = k1; D1[:, :len(k1)] = d1
            K2 = np.zeros((P, cap2), pkg.KP_DTYPE); D2 = np.zeros((P, cap2, 32), np.uint8); K2[:, :len(k2)] = k2; D2[:, :len(k2)] = d2
            PV = np.zeros((P, cap1, 2), np.float32); PV[:, :len(k1)] = prev
            dev = lambda x: pkg.DeviceBuffer(x.nbytes).upload(x)
            dk1, dd1, dc1 = dev(K1), dev(D1), dev(np.full(P, len(k1), np.int32))
            dk2, dd2, dc2 = dev(K2), dev(D2), dev(np.full(P, len(k2), np.int32))
            dpi = dev(PV); dpo = pkg.DeviceBuffer(PV.nbytes)
            gs, gi = pkg.DeviceBuffer(4 * 3073 * P), pkg.DeviceBuffer(4 * cap2 * P)
            mm, nm = pkg.DeviceBuffer(4 * P * cap1), pkg.DeviceBuffer(4 * P)
            assert L.orbm_grid_build_batch_async(mt.h, dk2.ptr, dc2.ptr, P, cap2, 0.0, 0.0, float(inv_w), float(inv_h), gs.ptr, gi.ptr) == 0

            def batch():
                rc = L.orbm_search_for_initialization_batch_async(mt.h, P, P, cap1, dk1.ptr, dd1.ptr, dc1.ptr, P, cap2, dk2.ptr, dd2.ptr, dc2.ptr,
                                                                  gs.ptr, gi.ptr, 0.0, 0.0, float(inv_w), float(inv_h), None, None, dpi.ptr,
                                                                  100, 0.9, 1, mm.ptr, nm.ptr, dpo.ptr)
                assert rc == 0, L.orbm_last_error()
                mt.sync()

            def host_loop(m=mt):
                for _ in range(P):
                    m.SearchForInitialization(v1, v2, prev, 100, 0.9, True)
            batch()
            rows = mm.download(np.int32, P * cap1).reshape(P, cap1); cnt = nm.download(np.int32, P)
            assert np.all(cnt == n_h) and all(np.array_equal(rows[p, :len(m_h)], m_h) for p in range(P)), "batch differs from the host entry"

            def clock(f):
                t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3

            def stats(v):
                return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
            rec = dict(shape="%dx%d" % (w, h), nfeatures=nf, n1=len(k1), n2=len(k2), level0_queries=int((k1["octave"] == 0).sum()), pairs=P,
                       matches=int(n_h), reps=a.reps)
            ev = []
            alone = []
            for _ in range(a.reps):                                          # the batch alone, host clock and device events
                alone.append(clock(batch))
                kernel_ms = C.c_float(0); L.orbm_last_timing(mt.h, C.byref(kernel_ms)); ev.append(kernel_ms.value)
            rec["batch_alone_ms"] = stats(alone); rec["batch_event_ms"] = stats(ev)
            if not a.batch_only:
                rec["host_alone_ms"] = stats([clock(host_loop) for _ in range(a.reps)])
                for name, m in (("same_handle", mt), ("two_handles", mh)):   # interleaved
                    tb, th = [], []
                    for _ in range(a.reps):
                        tb.append(clock(batch)); th.append(clock(lambda: host_loop(m)))
                    rec["interleaved_%s_batch_ms" % name] = stats(tb); rec["interleaved_%s_host_ms" % name] = stats(th)
                rec["host_per_call_ms"] = rec["host_alone_ms"]["median"] / P
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in out:
                f.write(json.dumps(rec) + "\n")
    mt.close(); mh.close()


if __name__ == "__main__":
    main()
