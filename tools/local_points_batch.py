"""SearchLocalPoints (M3) for a batch of frames: orbm_search_by_projection_points_batch_async against a loop of
orbm_search_by_projection_points_resident over the same frames and queries.

64 frames of 752 x 480 / 1000 features are extracted in one batch; every frame gets ~2 400 local map points (jittered
keypoints of the frame, descriptors with a few flipped bits), ~85 % of them in view.  The batched call is timed with its
own device events (orbm_last_timing: the candidate and the claim kernel, after warm-up) and with the host clock around
enqueue + sync; the resident path is a host-clock loop of one call per frame (it returns host rows, so its host round
trip is the cost a tracker pays).  Both must produce the same rows.  Prints one JSON line per measurement."""
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
synth = importlib.import_module("orb-slam3_amd.synth")

W, H, NB, NQ, REPS = 752, 480, 64, 2400, 20
INV_W, INV_H = float(np.float32(64) / np.float32(W)), float(np.float32(48) / np.float32(H))


def queries(rng, kps, desc, nq):
    src = rng.integers(0, len(kps), nq)
    px = (kps["x"][src] + rng.normal(0, 1.5, nq)).astype(np.float32); py = (kps["y"][src] + rng.normal(0, 1.5, nq)).astype(np.float32)
    d = desc[src].copy()
    for j in range(6):
        sel = np.flatnonzero(rng.integers(0, 7, nq) > j); b = rng.integers(0, 256, len(sel))
        d[sel, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return dict(in_view=(rng.random(nq) < 0.85).astype(np.uint8), px=px, py=py, pxr=(px - rng.uniform(2, 40, nq)).astype(np.float32),
                view_cos=rng.uniform(0.994, 1.0, nq).astype(np.float32), level=kps["octave"][src].astype(np.int32), qdesc=d,
                mp_obs=(rng.random(nq) < 0.9).astype(np.uint8))


def main():
    th, nnratio = float(os.environ.get("LP_TH", "1.0")), 0.8
    imgs = [synth.gen_image(W, H, 300 + i) for i in range(NB)]
    ex = pkg.ORBextractor(1000, max_size=(W, H), max_batch=NB)
    res = ex.extract_batch(imgs, [(0, 1000)] * NB)
    r = ex.result_device(); cap = r["cap"]
    L = pkg.lib()
    mg, m = pkg.ORBmatcher(0.8), pkg.ORBmatcher(0.8)          # grid on its own handle: m's event span is the search alone
    gs = pkg.DeviceBuffer(NB * 3073 * 4); gi = pkg.DeviceBuffer(NB * cap * 4)
    assert L.orbm_grid_build_batch_async(mg.h, r["kps"], r["counts"], NB, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr) == 0
    mg.sync()
    rng = np.random.default_rng(1)
    Q = [queries(rng, res[f][1], res[f][2], NQ) for f in range(NB)]
    blocked = (rng.random((NB, cap)) < 0.05).astype(np.uint8)
    dev = {}
    for name, dt in (("in_view", np.uint8), ("px", np.float32), ("py", np.float32), ("pxr", np.float32), ("view_cos", np.float32),
                     ("level", np.int32), ("mp_obs", np.uint8)):
        dev[name] = pkg.DeviceBuffer(NB * NQ * np.dtype(dt).itemsize).upload(np.stack([q[name] for q in Q]).astype(dt))
    dev["qdesc"] = pkg.DeviceBuffer(NB * NQ * 32).upload(np.stack([q["qdesc"] for q in Q]))
    dnq = pkg.DeviceBuffer(NB * 4).upload(np.full(NB, NQ, np.int32))
    dblk = pkg.DeviceBuffer(NB * cap).upload(blocked)
    sf = ex.GetScaleFactors()
    dm = pkg.DeviceBuffer(NB * cap * 4); dn = pkg.DeviceBuffer(NB * 4)

    def call():
        rc = L.orbm_search_by_projection_points_batch_async(
            m.h, r["kps"], r["desc"], r["counts"], cap, gs.ptr, gi.ptr, 0.0, 0.0, INV_W, INV_H, 0, NB, None, dblk.ptr, dnq.ptr, NQ,
            dev["in_view"].ptr, dev["px"].ptr, dev["py"].ptr, dev["pxr"].ptr, dev["view_cos"].ptr, dev["level"].ptr, None, 0.0,
            dev["qdesc"].ptr, dev["mp_obs"].ptr, 0, th, nnratio, sf.ctypes.data_as(C.c_void_p), 8, dm.ptr, dn.ptr)
        assert rc == 0, L.orbm_last_error()

    for _ in range(3):
        call()
    m.sync()
    dev_ms, wall_ms = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        m.sync()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(m.timing_ms())
    match = dm.download(np.int32, NB * cap).reshape(NB, cap); nm = dn.download(np.int32, NB)
    in_view = int(sum(int(q["in_view"].sum()) for q in Q))
    print(json.dumps(dict(path="batch", frames=NB, queries_per_frame=NQ, in_view_per_frame=in_view / NB, th=th,
                          device_ms_per_call=float(np.median(dev_ms)), device_ms_min=float(np.min(dev_ms)),
                          device_ms_per_frame=float(np.median(dev_ms)) / NB, wall_ms_per_call=float(np.median(wall_ms)),
                          matches=int(nm.sum()))), flush=True)
    # the same frames through the resident single-frame path (host rows, one call per frame)
    frames = [pkg.ResidentFrame(m, device=dict(kps=r["kps"] + f * cap * 28, desc=r["desc"] + f * cap * 32, n=len(res[f][1])), width=W, height=H)
              for f in range(NB)]
    args = lambda f: dict(blocked=blocked[f, :len(res[f][1])], scale_factors=sf, th=th, nnratio=nnratio, **Q[f])
    rows = [m.SearchByProjectionPointsResident(frames[f], **args(f)) for f in range(NB)]        # warm-up pass
    same = all(int(nm[f]) == rows[f][0] and np.array_equal(match[f, :len(res[f][1])], rows[f][1]) for f in range(NB))
    t0 = time.perf_counter()
    for _ in range(3):
        for f in range(NB):
            m.SearchByProjectionPointsResident(frames[f], **args(f))
    per_call = (time.perf_counter() - t0) * 1e3 / (3 * NB)
    print(json.dumps(dict(path="resident_loop", frames=NB, queries_per_frame=NQ, th=th, wall_ms_per_call=per_call,
                          wall_ms_per_batch=per_call * NB, rows_equal_batch=bool(same))), flush=True)
    for fr in frames:
        fr.close()
    assert same, "batched rows differ from the resident rows"


if __name__ == "__main__":
    main()
