"""Optimizer::PoseOptimization on the device (orbm_pose_optimization_batch_async: one workgroup per frame, all four rounds in one launch)
for T = --frames (1, 8, 64) frames of --edges (300, 1000) edges with 15 % gross outliers, 40 % of the edges stereo.

Per shape --reps (30) samples after a warm-up, each the device-event time around --inner back-to-back calls divided by --inner; median
and interquartile range in ms:
  eager   the call enqueued directly
  graph   the call captured once into a HIP graph and replayed
  host_header_ms   as context, NOT a host solver: the library's own arithmetic (csrc/orbm_poseopt.h with the reduction order replayed by
                   loops, tests/poseopt_header.cpp, g++ -O2 -ffp-contract=off, compiled when the tool starts) on one host thread, per
                   frame.  g2o itself cannot be built here (no Eigen), so this stands in for the host step the call removes.
The device result of frame 0 must equal the host program's bits.  Prints one JSON line per shape.  A record, not a threshold."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("orb-slam3_amd")
import poseopt_cases as pc          # noqa: E402
import poseopt_io as io             # noqa: E402


def stats(x):
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    return dict(median=float(med), iqr=float(q3 - q1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--edges", type=int, nargs="+", default=[300, 1000])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    exe = io.build_program(tmp)
    L = pkg.lib()
    hip = C.CDLL("libamdhip64.so")
    m = pkg.ORBmatcher(0.9)
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

    for ne in a.edges:
        cap = ne + ne // 5
        for T in a.frames:
            scenes = [pc.scene(5000 + 100 * ne + f, cap, ne, stereo_share=0.4, outlier_share=0.15) for f in range(T)]
            kps = np.stack([s["kps"] for s in scenes]); counts = np.full(T, cap, np.int32)
            ur = np.stack([s["uright"] for s in scenes])
            base = np.cumsum([0] + [len(s["mp_pw"]) for s in scenes])
            q_mp = np.stack([np.where(s["q_mp"] >= 0, s["q_mp"] + base[f], -1) for f, s in enumerate(scenes)]).astype(np.int32)
            pw = np.concatenate([s["mp_pw"] for s in scenes]); tcw = np.stack([s["tcw_in"].reshape(12) for s in scenes])
            d = [up(x) for x in (kps, counts, ur, q_mp, pw, tcw)]
            tout, out, nc, ng = pkg.DeviceBuffer(T * 48), pkg.DeviceBuffer(T * cap), pkg.DeviceBuffer(T * 4), pkg.DeviceBuffer(T * 4)

            def step():
                m.PoseOptimizationBatchAsync(T, 0, cap, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, len(pw), d[4].ptr, d[5].ptr, pc.K, float(pc.BF), pc.ILS2,
                                             tout.ptr, out.ptr, nc.ptr, ng.ptr)

            step(); m.sync()
            path = os.path.join(tmp, "case_%d_%d.txt" % (ne, T))
            io.write_cases(path, {"frame0": scenes[0]})
            host = io.run_program(exe, path, reps=a.host_reps)["frame0"]
            assert tout.download(np.float32, 12).tobytes() == host["tcw"].tobytes(), "the device pose differs from the host build of the header"
            good = ng.download(np.int32, T)
            assert good[0] == host["n_good"]
            rec = dict(tool="pose_optimization_batch", frames=T, edges=ne, cap=cap, outlier_share=0.15, stereo_share=0.4, reps=a.reps, inner=a.inner,
                       library=os.path.basename(pkg.LIB_PATH), n_good_mean=float(good.mean()), eager=sample(step), graph=sample(captured(step)),
                       host_header_ms=host["time_ms"], host_header_is="csrc/orbm_poseopt.h, g++ -O2, one thread, one frame: not g2o")
            print(json.dumps(rec), flush=True)
    m.close()


if __name__ == "__main__":
    main()
