"""CreateNewMapPoints behind M10 on the device (orbm_triangulate_new_points_batch_async: one lane per feature of a current KeyFrame, one wave
per KeyFrame for the creation order) for --keyframes (1, 16) current KeyFrames x --neighbours (20) at --features (1000), 30 % of the
features stereo, the scenes of tests/triangulate_cases.py.

Per shape --reps (30) samples after a warm-up, each the device-event time around --inner back-to-back calls divided by --inner; median
and interquartile range in ms:
  eager   the call enqueued directly
  graph   the call captured once into a HIP graph and replayed
  host_path   what the caller did before this call existed, for the same inputs: matches12 copied to the host (d2h_ms), the g++ build of
              csrc/orbm_triangulate.h looped over the rows on one thread (tests/triangulate_header.cpp, compiled when the tool starts;
              host_header_ms), the results copied up again for the device stages that follow (h2d_ms); host_path_ms is their sum.
The device result must equal the host program's bits.  Prints one JSON line per shape.  A record, not a threshold."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("orb-slam3_amd")
import triangulate_cases as tc      # noqa: E402
import triangulate_io as io         # noqa: E402


def stats(x):
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    return dict(median=float(med), iqr=float(q3 - q1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    exe = io.build_program(tmp)
    L = pkg.lib()
    hip = C.CDLL("libamdhip64.so")
    m = pkg.ORBmatcher(0.6)
    stream = C.c_void_p(L.orbm_stream(m.h))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    up = lambda x: pkg.DeviceBuffer(max(x.nbytes, 4)).upload(np.ascontiguousarray(x))

    def timed(step):
        m.sync()
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(a.inner):
            step()
        assert hip.hipEventRecord(e1, stream) == 0
        m.sync()
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value / a.inner

    def captured(step):
        graph, ge = C.c_void_p(), C.c_void_p()
        assert hip.hipStreamBeginCapture(stream, 1) == 0                     # hipStreamCaptureModeThreadLocal
        step()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and graph.value
        assert hip.hipGraphInstantiate(C.byref(ge), graph, None, None, C.c_size_t(0)) == 0
        return lambda: hip.hipGraphLaunch(ge, stream)

    def sample(step):
        for _ in range(3):
            timed(step)
        return stats([timed(step) for _ in range(a.reps)])

    def wall(fn):
        t = []
        for _ in range(a.reps):
            m.sync(); t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))

    nf, nn = a.features, a.neighbours
    for G in a.keyframes:
        c = tc.case(7000 + G, n1=nf, cap=nf, nneigh=nn, groups=G, stereo1=0.3, stereo2=0.3)
        npairs, cap1 = c["matches12"].shape
        pools = []
        for p in (c["pool1"], c["pool2"]):
            b = [up(p[k]) for k in ("kps_un", "kps", "counts", "uright", "depth", "tcw", "ow")]
            pools.append((b, (p["kps_un"].shape[0], p["kps_un"].shape[1]) + tuple(x.ptr for x in b)))
        d1, d2, dm = up(c["row1"]), up(c["row2"]), up(c["matches12"])
        out = {"won_pair": np.zeros((G, cap1), np.int32), "won_idx2": np.zeros((G, cap1), np.int32), "x3d": np.zeros((G, cap1, 3), np.float32),
               "reason": np.zeros((npairs, cap1), np.uint8), "ncreated": np.zeros(npairs, np.int32), "order": np.zeros((G, cap1), np.int32),
               "ntotal": np.zeros(G, np.int32)}
        dout = {k: up(v) for k, v in out.items()}

        def step():
            m.TriangulateNewPointsBatchAsync(c["group_start"], npairs, pools[0][1], pools[1][1], d1.ptr, d2.ptr, dm.ptr, c["k1"], c["k2"], c["mb1"], c["mbf1"],
                                             c["mb2"], c["sf1"], c["ls1"], c["sf2"], c["ls2"], c["ratio_factor"], c["th_far"],
                                             *(dout[k].ptr for k in ("won_pair", "won_idx2", "x3d", "reason", "ncreated", "order", "ntotal")))

        step(); m.sync()
        host = io.run_program(exe, c, tmp, "shape_%d" % G, reps=a.host_reps)
        for k, v in out.items():
            got = dout[k].download(v.dtype, v.size)
            assert got.tobytes() == np.ascontiguousarray(host[k]).astype(v.dtype).tobytes(), "the device %s differs from the host build of the header" % k
        d2h = wall(lambda: dm.download(np.int32, npairs * cap1))
        res_up = [np.ascontiguousarray(host[k]) for k in ("won_pair", "won_idx2", "x3d", "order", "ntotal")]
        h2d = wall(lambda: [dout[k].upload(v) for k, v in zip(("won_pair", "won_idx2", "x3d", "order", "ntotal"), res_up)])
        rec = dict(tool="triangulate_new_points_batch", keyframes=G, neighbours=nn, features=nf, pairs=npairs, matches=int((c["matches12"] >= 0).sum()),
                   created=int(host["ntotal"].sum()), reps=a.reps, inner=a.inner, library=os.path.basename(pkg.LIB_PATH), eager=sample(step),
                   graph=sample(captured(step)), d2h_ms=d2h, host_header_ms=host["time_ms"], h2d_ms=h2d, host_path_ms=d2h + host["time_ms"] + h2d,
                   host_header_is="csrc/orbm_triangulate.h, g++ -O2, one thread")
        print(json.dumps(rec), flush=True)
    m.close()


if __name__ == "__main__":
    main()
