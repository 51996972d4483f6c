"""The covisibility votes and the local map points on the device (orbm_covisibility_votes_batch_async, orbm_local_points_batch_async +
orbm_gather_map_points_batch_async) against the reference's own loops on one host thread (tests/covis_facade.cpp `bench`, g++ -O2,
compiled when the tool starts: std::map counters and pointer chasing on mock objects, maps drawn from the same distribution).

Shapes: votes for --queries (1, 64) queries of --slots (1200) slots, MapPoints with a mean of --mean-obs (8) entries, nine votes in ten
on --hot (30) rows of a --rows (2000) row pool; local points + gather for T = --queries frames of --lkf (80) KeyFrames x --slots slots.
Per shape --reps (30) samples after a warm-up, each the device-event time around --inner back-to-back calls divided by --inner; median
and interquartile range in ms:
  votes_lds / votes_plain   eager calls; the plain form (one global atomicAdd per vote) exists in the A/B library only: run the tool
                            with ORB_LIB=orb-slam3_amd/liborbslam3_amd_ab.so to get both (the switch is ORBM_COVIS_PLAIN)
  *_graph                   the call captured once into a HIP graph and replayed
  local_gather              local points + gather, eager and replayed
  ref_*_ms                  the reference's loops, mean of --host-reps runs
The device results must equal a numpy count of the same arrays.  Prints one JSON line per shape.  A record, not a threshold."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("orb-slam3_amd")


def make_votes(rng, nq, slots, rows, mean_obs, hot):
    nmp = nq * slots
    lens = rng.integers(1, 2 * mean_obs, nmp)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nobs = int(off[-1])
    row = np.where(rng.random(nobs) < 0.9, rng.integers(0, hot, nobs), rng.integers(0, rows, nobs)).astype(np.int32)
    return dict(q_mp=rng.permutation(nmp).astype(np.int32).reshape(nq, slots), q_n=np.full(nq, slots, np.int32), counts=np.full(rows, slots, np.int32),
                off=off, row=row, slot=rng.integers(0, slots, nobs).astype(np.int32), flags=np.zeros(nobs, np.uint8), nmp=nmp, nobs=nobs)


def stats(x):
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    return dict(median=float(med), iqr=float(q3 - q1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--slots", type=int, default=1200)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--mean-obs", type=int, default=8)
    ap.add_argument("--hot", type=int, default=30)
    ap.add_argument("--lkf", type=int, default=80)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    exe = os.path.join(tempfile.mkdtemp(), "covis_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "covis_facade.cpp")])
    L = pkg.lib()
    ab = os.path.basename(pkg.LIB_PATH).endswith("_ab.so")
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

    for nq in a.queries:
        rng = np.random.default_rng(nq)
        S = make_votes(rng, nq, a.slots, a.rows, a.mean_obs, a.hot)
        d = {k: up(S[k]) for k in ("q_mp", "q_n", "counts", "off", "row", "slot", "flags")}
        votes, cnt = pkg.DeviceBuffer(nq * a.rows * 4), [pkg.DeviceBuffer(nq * 4) for _ in range(3)]
        lcap = 64
        lists = [pkg.DeviceBuffer(nq * lcap * 4), pkg.DeviceBuffer(nq * lcap * 4)]

        def vote():
            m.CovisibilityVotesBatchAsync(nq, a.slots, d["q_mp"].ptr, d["q_n"].ptr, None, a.rows, a.slots, d["counts"].ptr, None, 0, S["nmp"], S["nobs"],
                                          d["off"].ptr, d["row"].ptr, d["slot"].ptr, d["flags"].ptr, None, 15, lcap, votes.ptr, cnt[0].ptr, cnt[1].ptr, cnt[2].ptr,
                                          lists[0].ptr, lists[1].ptr)

        want = np.zeros((nq, a.rows), np.int32)
        per_entry_q = np.repeat(np.argsort(S["q_mp"].reshape(-1)) // a.slots, np.diff(S["off"]))   # the query that holds each entry's MapPoint
        np.add.at(want, (per_entry_q, S["row"]), 1)
        rec = dict(tool="covisibility_batch", queries=nq, slots=a.slots, rows=a.rows, mean_obs=a.mean_obs, hot=a.hot, nobs=S["nobs"], reps=a.reps,
                   inner=a.inner, library=os.path.basename(pkg.LIB_PATH), max_votes=int(want.max()), n_voted_mean=float((want > 0).sum(1).mean()))
        for name, env in (("votes_lds", None),) + ((("votes_plain", "1"),) if ab else ()):
            os.environ.pop("ORBM_COVIS_PLAIN", None)
            if env:
                os.environ["ORBM_COVIS_PLAIN"] = env
            vote(); m.sync()
            assert np.array_equal(votes.download(np.int32, nq * a.rows).reshape(nq, a.rows), want), name
            rec[name] = sample(vote)
            rec[name + "_graph"] = sample(captured(vote))
        os.environ.pop("ORBM_COVIS_PLAIN", None)

        # local points + gather: T = nq frames over one pool of lkf KeyFrames x slots, a MapPoint in about four of them
        T, nl = nq, a.lkf
        nmp = nl * a.slots // 4 + 1
        kf_mp = rng.integers(0, nmp, (nl, a.slots)).astype(np.int32)
        lkf = np.stack([rng.permutation(nl) for _ in range(T)]).astype(np.int32)
        qs = nmp
        pool = dict(pw=rng.random((nmp, 3), np.float32), normal=rng.random((nmp, 3), np.float32), mn=rng.random(nmp, np.float32), mx=rng.random(nmp, np.float32),
                    desc=rng.integers(0, 256, (nmp, 32), np.uint8), nobs=rng.integers(0, 5, nmp).astype(np.int32))
        dp = {k: up(v) for k, v in pool.items()}
        dl, dn, dc, dk = up(lkf), up(np.full(T, nl, np.int32)), up(np.full(nl, a.slots, np.int32)), up(kf_mp)
        local_mp, n_total, dnq = pkg.DeviceBuffer(T * qs * 4), pkg.DeviceBuffer(T * 4), pkg.DeviceBuffer(T * 4)
        dst = [pkg.DeviceBuffer(T * qs * w) for w in (12, 12, 4, 4, 32, 1, 1)]

        def local():
            m.LocalPointsBatchAsync(T, nl, dl.ptr, dn.ptr, nl, a.slots, dc.ptr, dk.ptr, nmp, None, qs, local_mp.ptr, n_total.ptr, dnq.ptr)
            m.GatherMapPointsBatchAsync(T, qs, local_mp.ptr, dnq.ptr, nmp, dp["pw"].ptr, dp["normal"].ptr, dp["mn"].ptr, dp["mx"].ptr, dp["desc"].ptr,
                                        dp["nobs"].ptr, None, *[b.ptr for b in dst])

        local(); m.sync()
        got = local_mp.download(np.int32, T * qs).reshape(T, qs)
        nt = n_total.download(np.int32, T)
        for f in (0, T - 1):
            flat = kf_mp[lkf[f]].reshape(-1)
            first = flat[np.sort(np.unique(flat, return_index=True)[1])]
            assert nt[f] == len(first) and np.array_equal(got[f, :nt[f]], first)
        rec.update(frames=T, lkf=nl, local_nmp=nmp, n_total_mean=float(nt.mean()), local_gather=sample(local), local_gather_graph=sample(captured(local)))
        ref = json.loads(subprocess.check_output([exe, "bench", str(nq), str(a.slots), str(a.rows), str(a.mean_obs), str(a.hot), str(T), str(nl), str(a.slots),
                                                  str(a.host_reps)]))
        rec.update(ref_votes_frame_ms=ref["votes_frame_us"] / 1e3, ref_votes_keyframe_ms=ref["votes_keyframe_us"] / 1e3,
                   ref_local_points_ms=ref["local_points_us"] / 1e3)
        print(json.dumps(rec), flush=True)
    m.close()


if __name__ == "__main__":
    main()
