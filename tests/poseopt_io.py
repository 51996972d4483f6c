"""Helpers shared by the pose-optimisation tests: the text form of a case that tests/poseopt_header.cpp reads, the g++ build of that
program, its parsed output, and the tolerance rule."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "poseopt_header.cpp")
HDR = os.path.join(ROOT, "orb-slam3_amd", "csrc", "orbm_poseopt.h")


def write_cases(path, cases):
    """cases: {name: case dict of tests/poseopt_cases.py}."""
    g = lambda v: "%.9g" % float(v)
    with open(path, "w") as f:
        for name, c in cases.items():
            n = len(c["q_mp"])
            f.write("%s %d %d %d\n" % (name, n, len(c["ils2"]), 0 if c["uright"] is None else 1))
            f.write(" ".join(g(v) for v in c["K"]) + " " + g(c["bf"]) + "\n")
            f.write(" ".join(g(v) for v in c["ils2"]) + "\n")
            f.write(" ".join(g(v) for v in np.asarray(c["tcw_in"], np.float32).reshape(-1)) + "\n")
            nmp = len(c["mp_pw"])
            for i in range(n):
                j = int(c["q_mp"][i])
                has = 0 <= j < nmp
                pw = c["mp_pw"][j] if has else (0.0, 0.0, 0.0)
                ur = -1.0 if c["uright"] is None else c["uright"][i]
                f.write("%s %s %d %s %d %s %s %s\n" % (g(c["kps"]["x"][i]), g(c["kps"]["y"][i]), int(c["kps"]["octave"][i]), g(ur), int(has),
                                                   g(pw[0]), g(pw[1]), g(pw[2])))


def build_program(outdir, extra=()):
    exe = os.path.join(str(outdir), "poseopt_header" + ("_san" if extra else ""))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", *extra, "-o", exe, SRC])
    return exe


def run_program(exe, path, reps=0):
    out = subprocess.run([exe, path] + ([str(reps)] if reps else []), check=True, capture_output=True, text=True).stdout.split("\n")
    res, cur = {}, None
    for line in out:
        t = line.split()
        if not t:
            continue
        if t[0] == "case":
            cur = res.setdefault(t[1], {"n_corr": int(t[3]), "n_good": int(t[5])})
        elif t[0] == "pose":
            cur["pose"] = np.array([float.fromhex(v) for v in t[1:]]).reshape(3, 4)
        elif t[0] == "tcw":
            cur["tcw"] = np.array([float.fromhex(v) for v in t[1:]], np.float32).reshape(3, 4)
        elif t[0] == "flags":
            cur["outlier"] = np.array([-1 if ch == "-" else int(ch) for ch in (t[1] if len(t) > 1 else "")], np.int8)
        elif t[0] == "time_ms":
            cur["time_ms"] = float(t[1])
    return res


def pose_spread(a, b):
    """The largest difference of a pose entry, the translation column relative to max(1, |t|)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    d[:, 3] = d[:, 3] / np.maximum(1.0, np.abs(np.asarray(b, np.float64)[:, 3]))
    return float(d.max())


def run_selftest(exe):
    """`poseopt_header selftest`: {check name: bool}; the program's exit code says whether all held."""
    out = subprocess.run([exe, "selftest"], capture_output=True, text=True)
    checks = {t[1]: t[2] == "1" for t in (line.split() for line in out.stdout.splitlines()) if len(t) == 3 and t[0] == "check"}
    return out.returncode, checks
