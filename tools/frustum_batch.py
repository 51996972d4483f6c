"""Frame::isInFrustum for T frames that share one local map: ONE orbm_is_in_frustum_batch_async call (q_shared, poses from device rows)
against a loop of T orbm_is_in_frustum(ORBM_DEVICE) calls with the output pointers offset to row f -- the single-frame form is the path a
device-resident caller had before the batched call, unchanged by it.

T in --frames (1, 8, 64) x --points (4000) local points, every point of the row live.  Both forms run in the same process on the same
matcher and stream, alternating, after a warm-up.  Each is timed three ways, --reps times, and reported as median / min / max (the run-to-run
spread) in ms per step of T frames:
  event_ms   device events on the matcher's stream around --inner back-to-back eager steps, divided by --inner: what the stream is
             busy or waiting for, host enqueue gaps included (the loop enqueues T launches per step through ctypes)
  wall_ms    host clock round the same --inner steps plus the synchronise
  graph_ms   the step captured once into a HIP graph on the matcher's stream and replayed --inner times between two events: the
             device-side cost without the host's enqueue work
The two forms must write the same seven rows, bit for bit.  Prints one JSON line per T.  A record of what the call costs, not a threshold."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("orb-slam3_amd")

F = np.float32
K = np.array([458.654, 457.296, 367.215, 248.375], F)
BOUNDS = np.array([0.0, 752.0, 0.0, 480.0], F)
BF, COS_LIMIT, LSF, NLEV = 47.90639384423901, 0.5, float(np.log(F(1.2))), 8
ROWS = (("in_view", np.uint8), ("proj_x", F), ("proj_y", F), ("proj_xr", F), ("depth", F), ("level", np.int32), ("view_cos", F))


def local_map(rng, n):
    """Points in front of a camera at the origin, most of them inside the image; normals near the viewing ray; distance ranges around them."""
    z = rng.uniform(1.0, 14.0, n)
    pw = np.stack([rng.uniform(-0.9, 0.9, n) * z, rng.uniform(-0.6, 0.6, n) * z, z], 1).astype(F)
    dist = np.linalg.norm(pw, axis=1)
    nm = pw / dist[:, None] + rng.normal(0, 0.2, (n, 3))
    nm = (nm / np.linalg.norm(nm, axis=1, keepdims=True)).astype(F)
    mx = (dist * rng.uniform(1.0, 3.0, n)).astype(F)
    return pw, nm, (mx / 1.2 ** 7).astype(F), mx


def pose(rng):
    a = rng.uniform(-0.05, 0.05, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).astype(F)
    t = rng.uniform(-0.2, 0.2, 3).astype(F)
    return R, t, (-R.T @ t).astype(F)


def stats(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    L = pkg.lib()
    hip = C.CDLL("libamdhip64.so")
    m = pkg.ORBmatcher(0.9)
    stream = C.c_void_p(L.orbm_stream(m.h))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    up = lambda x: pkg.DeviceBuffer(x.nbytes).upload(np.ascontiguousarray(x))
    n = a.points
    rng = np.random.default_rng(4)
    pw, nm, mn, mx = local_map(rng, n)
    dpw, dnm, dmn, dmx = up(pw), up(nm), up(mn), up(mx)

    def timed(step):
        """(event ms, wall ms) per step over a.inner back-to-back steps."""
        m.sync()
        t0 = time.perf_counter()
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(a.inner):
            step()
        assert hip.hipEventRecord(e1, stream) == 0
        m.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value / a.inner, wall / a.inner

    for T in a.frames:
        poses = [pose(rng) for _ in range(T)]
        tcw = np.stack([np.concatenate([R, t[:, None]], 1).reshape(12) for R, t, _ in poses]).astype(F)
        ow = np.stack([o for _, _, o in poses]).astype(F)
        dtcw, dow, dnq = up(tcw), up(ow), up(np.full(T, n, np.int32))
        outs = {form: [pkg.DeviceBuffer(T * n * np.dtype(dt).itemsize) for _, dt in ROWS] for form in ("batch", "loop")}
        dcnt = pkg.DeviceBuffer(4 * T)
        host = [(np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(t), np.ascontiguousarray(o)) for R, t, o in poses]

        def batch():
            rc = L.orbm_is_in_frustum_batch_async(m.h, T, dtcw.ptr, dow.ptr, dnq.ptr, n, None, dpw.ptr, dnm.ptr, dmn.ptr, dmx.ptr, 1, vp(K), vp(BOUNDS),
                                                  BF, COS_LIMIT, LSF, NLEV, *[b.ptr for b in outs["batch"]], dcnt.ptr)
            assert rc == 0, L.orbm_last_error()

        def loop():
            for f in range(T):
                R, t, o = host[f]
                rc = L.orbm_is_in_frustum(m.h, pkg.DEVICE, n, dpw.ptr, dnm.ptr, dmn.ptr, dmx.ptr, vp(R), vp(t), vp(o), vp(K), vp(BOUNDS), BF, COS_LIMIT, LSF,
                                          NLEV, *[b.ptr + f * n * np.dtype(dt).itemsize for b, (_, dt) in zip(outs["loop"], ROWS)])
                assert rc == 0, L.orbm_last_error()

        forms = {"batch": batch, "loop": loop}
        for form in forms:                                                   # fresh rows, one step each: the outputs must agree
            for b, (_, dt) in zip(outs[form], ROWS):
                b.upload(np.full(T * n, 77, dt))
            forms[form]()
        m.sync()
        same = all(a_.download(np.uint8, a_.nbytes).tobytes() == b_.download(np.uint8, b_.nbytes).tobytes() for a_, b_ in zip(outs["batch"], outs["loop"]))
        in_view = outs["batch"][0].download(np.uint8, T * n).reshape(T, n).sum(1)
        assert np.array_equal(dcnt.download(np.int32, T), in_view)
        replay = {}
        for form in forms:                                                   # one graph per form
            graph, ge = C.c_void_p(), C.c_void_p()
            assert hip.hipStreamBeginCapture(stream, 1) == 0                 # hipStreamCaptureModeThreadLocal
            forms[form]()
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and graph.value
            assert hip.hipGraphInstantiate(C.byref(ge), graph, None, None, C.c_size_t(0)) == 0
            replay[form] = (lambda ge=ge: hip.hipGraphLaunch(ge, stream))
        for _ in range(3):                                                   # warm-up: every timed shape, every path
            for form in forms:
                timed(forms[form]); timed(replay[form])
        res = {form: dict(event_ms=[], wall_ms=[], graph_ms=[]) for form in forms}
        for _ in range(a.reps):                                              # alternate the forms within every repeat
            for form in forms:
                ev, wall = timed(forms[form])
                res[form]["event_ms"].append(ev); res[form]["wall_ms"].append(wall)
                res[form]["graph_ms"].append(timed(replay[form])[0])
        rec = dict(tool="frustum_batch", frames=T, points=n, reps=a.reps, inner=a.inner, in_view_per_frame=float(in_view.mean()), rows_equal=bool(same))
        for form in forms:
            for key, v in res[form].items():
                rec[form + "_" + key] = stats(v)
        print(json.dumps(rec), flush=True)
        assert same, "the batched rows differ from the loop's rows"
    m.close()


if __name__ == "__main__":
    main()
