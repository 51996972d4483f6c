"""KeyFrameCulling's redundancy counts on the device (orbm_keyframe_culling_batch_async, one call for all candidates) against a
single-thread C++ loop over the same flattened arrays (tools/keyframe_culling_host.cpp, g++ -O2, compiled when the tool starts; a host
loop over arrays, NOT the reference, which chases std::map nodes).

Shapes: --cands (30, 100) candidates of --slots (1000) slots; entry lists of mean length 8 and 25, and one skewed set (mean 8 with a few
lists of thousands of entries).  About 80 % of the slots hold a MapPoint.  Per shape, --reps times each after a warm-up, median [min -
max] in ms:
  event_ms      device events on the matcher's stream around --inner back-to-back eager calls, divided by --inner
  graph_ms      the call captured once into a HIP graph and replayed --inner times between the same events
  erased_ms     event_ms with an erased row set (no early exit: every list is walked to its end)
  host_form_ms  orbm_keyframe_culling on host arrays: staging, one upload of every array, the call, the download (host clock)
  upload_ms     the uploads alone, every input array to the device (host clock): what a caller with resident arrays does not pay
  host_loop_ms  the C++ loop, median of --reps runs
The device counts must equal the host loop's.  Prints one JSON line per shape.  A record of what the call costs, not a threshold."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("orb-slam3_amd")


def make(rng, ncand, slots, mean_len, skew):
    nrows = ncand + 40                                                      # the candidates and forty KeyFrames that only observe
    nmp = int(ncand * slots * 0.8 / 4)                                      # a MapPoint sits in about four candidates
    lens = np.clip(rng.poisson(mean_len, nmp), 1, None)
    if skew:
        lens[rng.choice(nmp, 12, replace=False)] = rng.integers(2000, 8000, 12)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nobs = int(off[-1])
    row = rng.integers(0, nrows, nobs).astype(np.int32); slot = rng.integers(0, slots, nobs).astype(np.int32)
    flags = np.where(rng.random(nobs) < 0.3, 4, 0).astype(np.uint8)
    kps = np.zeros((nrows, slots), pkg.KP_DTYPE)
    kps["octave"] = rng.choice([0, 1, 1, 2, 2, 2, 3, 4, 5], (nrows, slots))
    kf_mp = np.where(rng.random((ncand, slots)) < 0.8, rng.integers(0, nmp, (ncand, slots)), -1).astype(np.int32)
    depth = rng.choice(np.array([1.0, 5.0, 20.0, 40.0], np.float32), (ncand, slots))
    return dict(cand_row=np.arange(ncand, dtype=np.int32), kps=kps, counts=np.full(nrows, slots, np.int32), kf_mp=kf_mp, depth=depth, off=off, row=row,
                slot=slot, flags=flags, valid=np.ones(nmp, np.uint8), mp_nobs=lens.astype(np.int32), nrows=nrows, nmp=nmp, nobs=nobs)


def stats(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cands", type=int, nargs="+", default=[30, 100])
    ap.add_argument("--slots", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    so = os.path.join(tmp, "keyframe_culling_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "keyframe_culling_host.cpp")])
    host = C.CDLL(so)
    host.kfcull_host.restype = C.c_double
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    host.kfcull_host.argtypes = [ci, vp, ci, ci, vp, vp, vp, vp, cf, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, cf, vp, vp, vp, ci]
    L = pkg.lib()
    hip = C.CDLL("libamdhip64.so")
    m = pkg.ORBmatcher(0.9)
    stream = C.c_void_p(L.orbm_stream(m.h))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    up = lambda x: pkg.DeviceBuffer(x.nbytes).upload(np.ascontiguousarray(x))

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

    for ncand in a.cands:
        for mean_len, skew in ((8, False), (25, False), (8, True)):
            rng = np.random.default_rng(ncand * 100 + mean_len + skew)
            S = make(rng, ncand, a.slots, mean_len, skew)
            names = ("cand_row", "kps", "counts", "kf_mp", "depth", "off", "row", "slot", "flags", "valid", "mp_nobs")
            d = {k: up(S[k]) for k in names}
            erased = np.zeros(S["nrows"], np.uint8); erased[ncand:ncand + 4] = 1            # four of the observing KeyFrames are gone
            d_er = up(erased)
            out = [pkg.DeviceBuffer(4 * ncand), pkg.DeviceBuffer(4 * ncand), pkg.DeviceBuffer(ncand), pkg.DeviceBuffer(ncand * a.slots), pkg.DeviceBuffer(4)]

            def call(er=None):
                m.KeyframeCullingBatchAsync(ncand, d["cand_row"].ptr, S["nrows"], a.slots, d["kps"].ptr, d["counts"].ptr, d["kf_mp"].ptr, d["depth"].ptr, 35.0,
                                            S["nmp"], S["nobs"], d["off"].ptr, d["row"].ptr, d["slot"].ptr, d["flags"].ptr, d["valid"].ptr, d["mp_nobs"].ptr,
                                            er, 3, 0.9, *[o.ptr for o in out])

            hn, hr, hc = np.zeros(ncand, np.int32), np.zeros(ncand, np.int32), np.zeros(ncand, np.uint8)
            hargs = [ncand, p(S["cand_row"]), S["nrows"], a.slots, p(S["kps"]), p(S["counts"]), p(S["kf_mp"]), p(S["depth"]), 35.0, S["nmp"], S["nobs"], p(S["off"]),
                     p(S["row"]), p(S["slot"]), p(S["flags"]), p(S["valid"]), p(S["mp_nobs"])]
            host_er_ms = host.kfcull_host(*hargs, p(erased), 3, 0.9, p(hn), p(hr), p(hc), a.reps)
            call(d_er.ptr); m.sync()
            assert np.array_equal(out[0].download(np.int32, ncand), hn) and np.array_equal(out[1].download(np.int32, ncand), hr)
            host_ms = host.kfcull_host(*hargs, None, 3, 0.9, p(hn), p(hr), p(hc), a.reps)
            call(); m.sync()
            assert np.array_equal(out[0].download(np.int32, ncand), hn) and np.array_equal(out[1].download(np.int32, ncand), hr)
            assert np.array_equal(out[2].download(np.uint8, ncand), hc)
            graph, ge = C.c_void_p(), C.c_void_p()
            assert hip.hipStreamBeginCapture(stream, 1) == 0                 # hipStreamCaptureModeThreadLocal
            call()
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and graph.value
            assert hip.hipGraphInstantiate(C.byref(ge), graph, None, None, C.c_size_t(0)) == 0
            replay = lambda: hip.hipGraphLaunch(ge, stream)

            def uploads():
                for k in names:
                    d[k].upload(S[k])

            def host_form():
                m.KeyframeCulling(S["cand_row"], S["kps"], S["counts"], S["kf_mp"], S["depth"], 35.0, S["off"], S["row"], S["slot"], S["flags"], S["valid"],
                                  S["mp_nobs"], None, 3, 0.9, slot_state=False)

            def wall(fn):
                m.sync(); t0 = time.perf_counter(); fn(); m.sync()
                return (time.perf_counter() - t0) * 1e3

            for _ in range(3):                                               # warm-up: every timed path
                timed(call); timed(replay); timed(lambda: call(d_er.ptr)); wall(uploads); wall(host_form)
            res = dict(event_ms=[], graph_ms=[], erased_ms=[], upload_ms=[], host_form_ms=[])
            for _ in range(a.reps):
                res["event_ms"].append(timed(call)); res["graph_ms"].append(timed(replay)); res["erased_ms"].append(timed(lambda: call(d_er.ptr)))
                res["upload_ms"].append(wall(uploads)); res["host_form_ms"].append(wall(host_form))
            rec = dict(tool="keyframe_culling", cands=ncand, slots=a.slots, mean_len=mean_len, skewed=bool(skew), nmp=S["nmp"], nobs=S["nobs"],
                       longest=int(S["mp_nobs"].max()), input_mb=round(sum(S[k].nbytes for k in names) / 1e6, 2), reps=a.reps, inner=a.inner,
                       n_mps_mean=float(hn.mean()), n_redundant_mean=float(hr.mean()), culled=int(hc.sum()), host_loop_ms=float(host_ms),
                       host_loop_erased_ms=float(host_er_ms))
            for k, v in res.items():
                rec[k] = stats(v)
            print(json.dumps(rec), flush=True)
    m.close()


if __name__ == "__main__":
    main()
