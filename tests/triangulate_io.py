"""Helpers shared by the CreateNewMapPoints tests: the binary form of a case that tests/triangulate_header.cpp reads, the g++ build of that
program and its parsed output."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "triangulate_header.cpp")
OUT_KEYS = ("won_pair", "won_idx2", "x3d", "reason", "ncreated", "order", "ntotal")


def _pool_bytes(p):
    kp = p["kps_un"]; k = kp if p.get("kps") is None else p["kps"]
    full = lambda key: np.full(kp.shape, -1, np.float32) if p.get(key) is None else np.asarray(p[key], np.float32)
    parts = [kp["x"], kp["y"], kp["octave"].astype(np.int32), k["x"], k["y"], np.asarray(p["counts"], np.int32), full("uright"), full("depth"),
             np.asarray(p["tcw"], np.float32), np.asarray(p["ow"], np.float32)]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def write_case(path, c):
    m12 = np.ascontiguousarray(c["matches12"], np.int32); npairs, cap1 = m12.shape
    p1, p2 = c["pool1"], c["pool2"]
    head = np.array([len(c["group_start"]) - 1, npairs, p1["kps_un"].shape[0], cap1, p2["kps_un"].shape[0], p2["kps_un"].shape[1], len(c["sf1"]), 0], np.int32)
    fl = np.concatenate([np.asarray(c["k1"], np.float32), np.asarray(c["k2"], np.float32),
                         np.array([c["mb1"], c["mbf1"], c["mb2"], c["ratio_factor"], c["th_far"]], np.float32)])
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for key in ("group_start", "row1", "row2"):
            f.write(np.ascontiguousarray(c[key], np.int32).tobytes())
        f.write(m12.tobytes()); f.write(_pool_bytes(p1)); f.write(_pool_bytes(p2)); f.write(fl.tobytes())
        for key in ("sf1", "ls1", "sf2", "ls2"):
            f.write(np.ascontiguousarray(c[key], np.float32).tobytes())


def build_program(outdir, extra=()):
    exe = os.path.join(str(outdir), "triangulate_header" + ("_san" if extra else ""))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", *extra, "-o", exe, SRC])
    return exe


def run_program(exe, c, workdir, tag="case", reps=0):
    """-> the outputs of orbm_triangulate_new_points as the header computes them, plus xh [npairs][cap1][4] and, with reps, time_ms."""
    path, out = os.path.join(str(workdir), tag + ".bin"), os.path.join(str(workdir), tag + ".out")
    write_case(path, c)
    r = subprocess.run([exe, path, out] + ([str(reps)] if reps else []), check=True, capture_output=True, text=True)
    npairs, cap1 = np.asarray(c["matches12"]).shape; ng = len(c["group_start"]) - 1
    raw = open(out, "rb").read()
    shapes = [("won_pair", np.int32, (ng, cap1)), ("won_idx2", np.int32, (ng, cap1)), ("x3d", np.float32, (ng, cap1, 3)), ("reason", np.int32, (npairs, cap1)),
              ("ncreated", np.int32, (npairs,)), ("order", np.int32, (ng, cap1)), ("ntotal", np.int32, (ng,)), ("xh", np.float32, (npairs, cap1, 4))]
    res, off = {}, 0
    for key, dt, shp in shapes:
        n = int(np.prod(shp)) * 4
        res[key] = np.frombuffer(raw[off:off + n], dt).reshape(shp).copy(); off += n
    assert off == len(raw)
    res["reason"] = res["reason"].astype(np.uint8)
    for line in r.stdout.splitlines():
        if line.startswith("time_ms"):
            res["time_ms"] = float(line.split()[1])
    return res
