"""MapPoint refresh for a KeyFrame insertion kept on the device: orbm_distinctive_descriptors_batch_async and
orbm_update_normal_and_depth_batch_async over a pool of --rows KeyFrame rows of --cap slots, for --mappoints MapPoints (default 1 000 and
4 000) whose observation counts follow a long-tailed distribution (log-normal, mean about 15, clipped to [2, 300]).  Medians of --reps
calls with the host clock round enqueue + sync: each device call, the pair, (a) the host forms on the same inputs and (b) the two loops
as a caller runs them today -- single-threaded plain C++ (tools/mappoint_refresh_host.cpp, built here with g++) followed by the upload
of the four rows.  The results of all three are compared before anything is timed.  Prints one JSON line per size; the kernels alone
come from running the tool under rocprofv3 --kernel-trace --stats (k_mp_distinctive, k_mp_normal_depth).  --clip N draws lists of at
most N observations (--clip 30: a call without the long tail).  With ORB_LIB pointing at liborbslam3_amd_ab.so the descriptor call is
also timed with the packed A/B kernels (ORBM_MP_PACKED = 8, 16, 32: groups of that many lanes per MapPoint, longer lists in a second
launch of the wave kernel), after their rows are seen to equal the product's.  A record, not a threshold."""
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
F = np.float32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_lib(tmp):
    so = os.path.join(tmp, "mappoint_refresh_host.so")
    subprocess.check_call(["g++", "-O2", "-mpopcnt", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "mappoint_refresh_host.cpp")])
    lib = C.CDLL(so)
    lib.mp_refresh_host.argtypes = [C.c_int] * 3 + [C.c_void_p] * 13 + [C.c_int] + [C.c_void_p] * 4
    return lib


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run(m, host, nmp, nrows, cap, reps, rng, clip):
    L = m.L
    nlev = 8
    sf = (F(1.2) ** np.arange(nlev)).astype(F)
    desc = rng.integers(0, 256, (nrows, cap, 32)).astype(np.uint8)
    kps = np.zeros((nrows, cap), pkg.KP_DTYPE); kps["octave"] = rng.integers(0, nlev, (nrows, cap))
    counts = np.full(nrows, cap, np.int32)
    ow_l = rng.uniform(-3, 3, (nrows, 3)).astype(F); ow_r = (ow_l + F(0.1)).astype(F)
    n = np.clip(np.round(rng.lognormal(2.2, 1.0, nmp)), 2, clip).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    nobs = int(off[-1])
    row = rng.integers(0, nrows, nobs).astype(np.int32); slot = rng.integers(0, cap, nobs).astype(np.int32)
    flags = (rng.random(nobs) < 0.02).astype(np.uint8) * 2                  # a few bad KeyFrames
    pw = rng.uniform(-8, 8, (nmp, 3)).astype(F)
    ref_row = row[off[:-1]].copy(); ref_slot = slot[off[:-1]].copy()
    up = lambda a: pkg.DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a))
    d_desc, d_kps, d_counts, d_owl, d_owr = up(desc), up(kps), up(counts), up(ow_l), up(ow_r)
    d_off, d_row, d_slot, d_fl, d_pw, d_rr, d_rs = up(off), up(row), up(slot), up(flags), up(pw), up(ref_row), up(ref_slot)
    o_desc, o_best, o_med = pkg.DeviceBuffer(nmp * 32), pkg.DeviceBuffer(nmp * 4), pkg.DeviceBuffer(nmp * 4)
    o_n, o_mn, o_mx, o_up = pkg.DeviceBuffer(nmp * 12), pkg.DeviceBuffer(nmp * 4), pkg.DeviceBuffer(nmp * 4), pkg.DeviceBuffer(nmp)

    def dev_desc():
        m.ComputeDistinctiveDescriptorsBatchAsync(nmp, nrows, cap, d_desc.ptr, d_counts.ptr, nobs, d_off.ptr, d_row.ptr, d_slot.ptr, d_fl.ptr, None,
                                                  o_desc.ptr, o_best.ptr, o_med.ptr)

    def dev_normal():
        m.UpdateNormalAndDepthBatchAsync(nmp, nrows, cap, d_kps.ptr, d_counts.ptr, d_owl.ptr, d_owr.ptr, nobs, d_off.ptr, d_row.ptr, d_slot.ptr, d_fl.ptr, None,
                                         d_pw.ptr, d_rr.ptr, d_rs.ptr, sf, o_n.ptr, o_mn.ptr, o_mx.ptr, o_up.ptr)

    def host_forms():
        a = m.ComputeDistinctiveDescriptors(desc, counts, off, row, slot, flags)
        b = m.UpdateNormalAndDepth(kps, counts, ow_l, ow_r, off, row, slot, flags, None, pw, ref_row, ref_slot, sf)
        return a, b

    octave = np.ascontiguousarray(kps["octave"], np.int32)
    h_desc = np.zeros((nmp, 32), np.uint8); h_n = np.zeros((nmp, 3), F); h_mn = np.zeros(nmp, F); h_mx = np.zeros(nmp, F)

    def cpp_loops():
        host.mp_refresh_host(nmp, nrows, cap, _p(desc), _p(octave), _p(counts), _p(ow_l), _p(ow_r), _p(off), _p(row), _p(slot), _p(flags), _p(pw),
                             _p(ref_row), _p(ref_slot), _p(sf), nlev, _p(h_desc), _p(h_n), _p(h_mn), _p(h_mx))
        o_desc.upload(h_desc); o_n.upload(h_n); o_mn.upload(h_mn); o_mx.upload(h_mx)   # the rows go back for the next device search

    # the three agree before anything is timed
    cpp_loops()
    dev_desc(); dev_normal(); m.sync()
    g_desc = o_desc.download(np.uint8, nmp * 32).reshape(nmp, 32); g_n = o_n.download(F, nmp * 3).reshape(nmp, 3)
    g_mx = o_mx.download(F, nmp); g_up = o_up.download(np.uint8, nmp)
    (_, a_desc, _, _), (_, a_n, _, a_mx, a_up) = host_forms()
    assert g_up.all() and np.array_equal(g_desc, h_desc) and np.array_equal(g_n.view(np.uint32), h_n.view(np.uint32)) and np.array_equal(g_mx, h_mx)
    assert np.array_equal(a_desc, g_desc) and np.array_equal(a_n.view(np.uint32), g_n.view(np.uint32)) and np.array_equal(a_mx, g_mx) and a_up.all()
    res = dict(tool="mappoint_refresh_batch", mappoints=nmp, observations=nobs, n_mean=float(n.mean()), n_max=int(n.max()), rows=nrows, cap=cap, reps=reps, clip=clip)
    res["device_descriptors_ms"] = _median_ms(lambda: (dev_desc(), m.sync()), reps)
    res["device_normals_ms"] = _median_ms(lambda: (dev_normal(), m.sync()), reps)
    res["device_pair_ms"] = _median_ms(lambda: (dev_desc(), dev_normal(), m.sync()), reps)
    res["host_forms_pair_ms"] = _median_ms(host_forms, reps)
    res["cpp_single_thread_pair_ms"] = _median_ms(cpp_loops, reps)
    if AB:                                                                  # the packed A/B kernels against the wave per MapPoint, same call
        res["ab_wave_descriptors_ms"] = res["device_descriptors_ms"]
        for g in (8, 16, 32):
            os.environ["ORBM_MP_PACKED"] = str(g)
            try:
                o_desc.upload(np.zeros(nmp * 32, np.uint8)); o_best.upload(np.full(nmp, -9, np.int32))
                dev_desc(); m.sync()
                assert np.array_equal(o_desc.download(np.uint8, nmp * 32).reshape(nmp, 32), g_desc), "packed %d differs" % g
                res["ab_packed%d_descriptors_ms" % g] = _median_ms(lambda: (dev_desc(), m.sync()), reps)
                res["ab_packed%d_share_of_mappoints" % g] = float((n <= g).mean())
            finally:
                del os.environ["ORBM_MP_PACKED"]
    return res


AB = os.environ.get("ORB_LIB", "").endswith("_ab.so")                       # ORB_LIB=.../liborbslam3_amd_ab.so: the -DORBX_AB build


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mappoints", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--cap", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--clip", type=int, default=300, help="longest observation list of the draw")
    a = ap.parse_args()
    m = pkg.ORBmatcher(0.9)
    with tempfile.TemporaryDirectory() as tmp:
        host = _host_lib(tmp)
        for nmp in a.mappoints:
            print(json.dumps(run(m, host, nmp, a.rows, a.cap, a.reps, np.random.default_rng(nmp), a.clip)), flush=True)


if __name__ == "__main__":
    main()
