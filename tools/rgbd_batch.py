"""RGB-D frame steps for a batch kept on the device: orbm_stereo_from_rgbd_batch_async (ComputeStereoFromRGBD with the depth conversion
folded in) and orbm_unproject_stereo_batch_async (UnprojectStereo) on a hand-laid block of --frames frames x --keypoints keypoints over
--width x --height 16-bit depth images (default 256 x 1000 on 640 x 480: TUM RGB-D's size), --reps eager calls of each.  Prints one JSON
line with the host clock round the enqueues + sync; the kernels alone come from running the tool under rocprofv3 --kernel-trace --stats
(k_rgbd_stereo, k_unproject_stereo).  A record of what the two calls cost, not a threshold."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("orb-slam3_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    nf, cap, w, h = a.frames, a.keypoints, a.width, a.height
    m = pkg.ORBmatcher(0.9)
    L = m.L
    kps = np.zeros((nf, cap), pkg.KP_DTYPE)
    kps["x"] = rng.uniform(0, w, kps.shape); kps["y"] = rng.uniform(0, h, kps.shape)
    counts = np.full(nf, cap, np.int32)
    img = rng.integers(0, 40000, (nf, h, w)).astype(np.uint16)
    img[rng.random(img.shape) < 0.1] = 0
    dk = pkg.DeviceBuffer(kps.nbytes).upload(kps); dc = pkg.DeviceBuffer(counts.nbytes).upload(counts); di = pkg.DeviceBuffer(img.nbytes).upload(img)
    tab = pkg.DeviceBuffer(8 * nf).upload(np.array([di.ptr + f * h * w * 2 for f in range(nf)], np.uint64))
    ur = pkg.DeviceBuffer(nf * cap * 4); dp = pkg.DeviceBuffer(nf * cap * 4); nv = pkg.DeviceBuffer(nf * 4)
    twc = np.tile(np.array([1, 0, 0, 0.1, 0, 1, 0, 0.2, 0, 0, 1, 0.3], np.float32), (nf, 1))
    dT = pkg.DeviceBuffer(twc.nbytes).upload(twc)
    x3 = pkg.DeviceBuffer(nf * cap * 12); has = pkg.DeviceBuffer(nf * cap)
    K = np.array([517.3, 516.5, 318.6, 255.3], np.float32)

    def step():
        m.ComputeStereoFromRGBDBatchAsync(nf, 0, cap, dk.ptr, dk.ptr, dc.ptr, tab.ptr, pkg.DEPTH_U16, w, h, w * 2, 1.0 / 5000.0, 40.0, ur.ptr, dp.ptr, nv.ptr)
        m.UnprojectStereoBatchAsync(nf, 0, cap, dk.ptr, dc.ptr, dp.ptr, dT.ptr, K, x3.ptr, has.ptr)

    step(); m.sync()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter(); step(); m.sync(); ts.append((time.perf_counter() - t0) * 1e3)
    n_valid = int(nv.download(np.int32, nf).sum()); n_pts = int(has.download(np.uint8, nf * cap).sum())
    assert n_valid == n_pts > 0
    print(json.dumps(dict(tool="rgbd_batch", frames=nf, keypoints=cap, width=w, height=h, depth="u16", reps=a.reps, depth_points=n_valid,
                          both_calls_ms_median=float(np.median(ts)), both_calls_ms_min=float(min(ts)), both_calls_ms_max=float(max(ts)))), flush=True)


if __name__ == "__main__":
    main()
