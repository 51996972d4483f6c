"""facade/PoseOptimization.h compiled with plain g++ against cvcompat.h on the mock Frame / MapPoint types of tests/poseopt_mock.h as a
stand-alone program (tests/poseopt_facade.cpp, which supplies orbm_pose_optimization as the host run of csrc/orbm_poseopt.h): for every
case the facade's flatten equals the case arrays, the frame ends with the flags and the pose the header program computes, and a frame
with a second camera is refused before any call.  No GPU, no library."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseopt_io as io            # noqa: E402
import poseopt_results as res      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("poseopt_facade")
    exe, path = str(d / "poseopt_facade"), str(d / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "poseopt_facade.cpp")])
    io.write_cases(path, res.cases())
    got, cur = {}, None
    for line in subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines():
        name, n, *vals = line.split()
        if name == "case":
            cur = got.setdefault(n, {})
            continue
        assert int(n) == len(vals), line
        cur[name] = np.array([int(v) for v in vals], np.int64)
    refused = subprocess.run([exe, path, "second-camera"], check=True, capture_output=True, text=True).stdout.split()
    return got, io.run_program(io.build_program(d), path), refused


def _f32(a):
    return a.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("name", sorted(res.cases()))
def test_flatten_and_results(outputs, name):
    got, hdr = outputs[0][name], outputs[1][name]
    c = res.cases()[name]
    n = len(c["q_mp"])
    calls, nframes, first, cap, nmp, nlevels, count, have_ur, ret, n_set = [int(v) for v in got["shape"]]
    has = c["q_mp"] >= 0
    assert (calls, nframes, first, cap, nlevels, count) == (1, 1, 0, max(n, 1), len(c["ils2"]), n)
    assert nmp == max(int(has.sum()), 1) and have_ur == (0 if c["uright"] is None else 1)
    assert np.array_equal(_f32(got["x"])[:n], c["kps"]["x"]) and np.array_equal(_f32(got["y"])[:n], c["kps"]["y"])
    assert np.array_equal(got["octave"][:n], c["kps"]["octave"])
    if c["uright"] is not None:
        assert np.array_equal(_f32(got["uright"])[:n], c["uright"])
    q = got["q_mp"][:n]
    assert np.array_equal(q >= 0, has) and np.array_equal(q[has], np.arange(has.sum()))       # one pool row per slot, in slot order
    if has.any():
        assert np.array_equal(_f32(got["pw"]).reshape(-1, 3), c["mp_pw"][c["q_mp"][has]])
    assert np.array_equal(_f32(got["ils2"]), c["ils2"]) and np.array_equal(_f32(got["tcw"]), c["tcw_in"].reshape(-1))
    assert np.array_equal(_f32(got["k"]), c["K"]) and _f32(got["bf"])[0] == c["bf"]
    # what the facade left in the frame: flags only where a MapPoint sits (the mock starts them all true), SetPose unless n_corr < 3
    assert np.array_equal(got["outlier"], np.where(hdr["outlier"] < 0, 1, hdr["outlier"]))
    assert ret == hdr["n_good"] and n_set == (1 if hdr["n_corr"] >= 3 else 0)
    pose = _f32(got["pose"]).reshape(4, 4)
    assert np.array_equal(pose[:3], hdr["tcw"] if hdr["n_corr"] >= 3 else c["tcw_in"]) and np.array_equal(pose[3], [0, 0, 0, 1])


def test_second_camera_is_refused(outputs):
    assert outputs[2] == ["refused", "1", "1", "calls", "1", "0"]
