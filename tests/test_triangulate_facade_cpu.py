"""facade/CreateNewMapPoints.h on mock KeyFrames, built with g++ on cvcompat.h (tests/triangulate_facade.cpp), no GPU: the flatten of
the KeyFrames of a case equals the case's own arrays byte for byte (pools, poses, camera centres, matches12, intrinsics, level tables,
ratio factor); the baseline and median-depth tests drop the neighbours the reference drops; F12 equals K1^-T [t12]x R12 K2^-1; a second
camera, NLeft != -1, another camera model or another camera are refused."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulate_io as io        # noqa: E402
import triangulate_results as res  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ["short_baseline_is_skipped", "monocular_uses_the_median_depth", "monocular_ratio_below_0.01_is_skipped", "second_camera_of_a_neighbour_is_refused",
          "second_camera_is_refused", "nleft_is_refused", "fisheye_is_refused", "another_camera_is_refused"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("triangulate_facade")
    path = str(d / "triangulate_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-o", path, os.path.join(ROOT, "tests", "triangulate_facade.cpp")])
    return d, path


def tight(c):
    """The case as the facade lays it out: pool 1 = the current KeyFrame's row alone with cap1 = its count, pool 2 = one row per pair
    with cap2 = the largest neighbour count; slots past a count hold zeros and -1."""
    p1, p2 = c["pool1"], c["pool2"]
    r1 = int(c["row1"][0]); n1 = int(p1["counts"][r1]); rows2 = [int(r) for r in c["row2"]]
    cap2 = max(int(p2["counts"][r]) for r in rows2)

    def rows(p, rr, cap):
        out = {"counts": np.array([p["counts"][r] for r in rr], np.int32), "tcw": np.stack([p["tcw"][r] for r in rr]), "ow": np.stack([p["ow"][r] for r in rr])}
        for key, fill in (("kps_un", None), ("kps", None), ("uright", -1), ("depth", -1)):
            a = np.zeros((len(rr), cap), p[key].dtype)
            if fill is not None:
                a[:] = fill
            for j, r in enumerate(rr):
                n = int(p["counts"][r]); a[j, :n] = p[key][r, :n]
            out[key] = a
        for key in ("kps_un", "kps"):                     # the program's mock KeyPoints carry x, y and octave only
            z = np.zeros_like(out[key]); z["x"], z["y"], z["octave"] = out[key]["x"], out[key]["y"], out[key]["octave"]; out[key] = z
        return out
    m = np.full((len(rows2), n1), -1, np.int32)
    for p, r in enumerate(rows2):
        row = c["matches12"][p, :n1]
        ok = (row >= 0) & (row < int(p2["counts"][r]))
        m[p, ok] = row[ok]
    return dict(c, pool1=rows(p1, [r1], n1), pool2=rows(p2, rows2, cap2), row1=np.zeros(len(rows2), np.int32), row2=np.arange(len(rows2), dtype=np.int32), matches12=m)


@pytest.mark.parametrize("name", ["mono_3", "both_stereo_3", "close_stereo"])
def test_the_flatten_equals_the_case_arrays(exe, name):
    d, path = exe
    c = res.cases()[name]
    src, want, out = str(d / (name + ".bin")), str(d / (name + ".want")), str(d / (name + ".flat"))
    io.write_case(src, c); io.write_case(want, tight(c))
    r = subprocess.run([path, src, out], check=True, capture_output=True, text=True).stdout
    assert ("pairs %d of %d" % (len(c["row1"]), len(c["row1"]))) in r and ("searches %d" % len(c["row1"])) in r
    assert open(out, "rb").read() == open(want, "rb").read()
    checks = {t[1]: t[2] == "1" for t in (line.split() for line in r.splitlines()) if len(t) == 3 and t[0] == "check"}
    assert sorted(checks) == sorted(CHECKS) and all(checks.values()), checks
    # F12 = K1^-T [t12]x R12 K2^-1 in float64, to float32 rounding of a handful of products
    k = c["k1"].astype(np.float64); Ki = np.array([[1 / k[0], 0, -k[2] / k[0]], [0, 1 / k[1], -k[3] / k[1]], [0, 0, 1]])
    T1 = c["pool1"]["tcw"][int(c["row1"][0])].reshape(3, 4).astype(np.float64)
    for line in r.splitlines():
        t = line.split()
        if t and t[0] == "F12":
            T2 = c["pool2"]["tcw"][int(c["row2"][int(t[1])])].reshape(3, 4).astype(np.float64)
            R12 = T1[:, :3] @ T2[:, :3].T; t12 = -R12 @ T2[:, 3] + T1[:, 3]
            tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
            F = Ki.T @ tx @ R12 @ Ki
            got = np.array([float.fromhex(v) for v in t[2:]]).reshape(3, 3)
            assert np.abs(got - F).max() <= 1e-5 * np.abs(F).max()
