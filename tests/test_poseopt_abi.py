"""CPU-side checks of the pose-optimisation entry points (orbm_pose_optimization, orbm_pose_optimization_batch_async,
orbm_discard_outliers_batch_async): each is declared in include/orbm.h, exported by the library, listed in the package's EXPORTS and bound
with argument types that match the declaration one for one; the host and the device form share their parameter list; the limits; the
header contract names its rules; without a device the calls fail with ORBM_E_HIP.  No GPU; the refused-argument cases need a handle and
live in tests/test_gpu_poseopt.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_HIP = -2, -5
POSE = ["nframes", "first", "cap", "kps_un", "counts", "uright", "q_mp", "nmp", "mp_pw", "tcw_in", "k_host", "bf", "inv_level_sigma2_host", "nlevels",
        "tcw_out", "outlier", "n_corr", "n_good"]
DISCARD = ["nframes", "cap", "counts", "q_mp", "outlier", "nmp", "mp_nobs", "mp_valid", "discard", "clear_bad", "mp_seen", "n_matches_map", "n_discarded"]
SYMBOLS = {"orbm_pose_optimization": POSE, "orbm_pose_optimization_batch_async": POSE, "orbm_discard_outliers_batch_async": DISCARD}
INTS = {"nframes", "first", "cap", "nmp", "nlevels", "discard", "clear_bad"}


def _header():
    return open(os.path.join(ROOT, "include", "orbm.h")).read()


def _params(name):
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert decl, name + " is not declared in orbm.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",") if a.strip()]


def _ctype(decl):
    return C.c_void_p if "*" in decl else (C.c_float if decl.startswith("float") else C.c_int)


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_declared_exported_and_bound(pkg, name):
    params = _params(name)
    assert [a.split()[-1].lstrip("*") for a in params[1:]] == SYMBOLS[name]
    assert name in pkg.EXPORTS
    pkg.build()
    assert hasattr(C.CDLL(pkg.LIB_PATH), name)
    at = getattr(pkg.lib(), name).argtypes
    assert at is not None and list(at) == [_ctype(a) for a in params]
    for i, p in enumerate(SYMBOLS[name], 1):
        assert at[i] is (C.c_int if p in INTS else C.c_float if p == "bf" else C.c_void_p), p


def test_host_and_device_forms_share_their_parameter_list():
    assert _params("orbm_pose_optimization") == _params("orbm_pose_optimization_batch_async")


def test_declared_after_the_covisibility_block():
    txt = _header()
    order = [txt.index(s) for s in ("int orbm_gather_map_points_batch_async(", "/* ---- Pose optimisation on the device", "int orbm_pose_optimization(",
                                    "int orbm_pose_optimization_batch_async(", "int orbm_discard_outliers_batch_async(",
                                    "/* M15 Frame::ComputeStereoMatches")]
    assert order == sorted(order)


def test_limit_constants(pkg):
    assert re.search(r"enum\s*\{\s*ORBM_POSEOPT_MAX_FRAMES\s*=\s*65535\s*,\s*ORBM_POSEOPT_MAX_CAP\s*=\s*65535\s*,\s*ORBM_POSEOPT_MAX_LEVELS\s*=\s*32\s*\}", _header())
    assert (pkg.POSEOPT_MAX_FRAMES, pkg.POSEOPT_MAX_CAP, pkg.POSEOPT_MAX_LEVELS) == (65535, 65535, 32)
    kernels = open(os.path.join(ROOT, "orb-slam3_amd", "csrc", "orbm_kernels.hip.h")).read()
    assert re.search(r"#define\s+PO_MAX_LEVELS\s+32\b", kernels) and re.search(r"#define\s+PO_LDS_CAP\s+1536\b", kernels)


def test_wrappers_exist(pkg):
    pkg.lib()
    for name in ("PoseOptimization", "PoseOptimizationBatchAsync", "DiscardOutliersBatchAsync"):
        assert callable(getattr(pkg.ORBmatcher, name))


def test_contract_comment_names_the_rules():
    """The header carries the contract where callers read it."""
    txt = _header()
    c = txt[txt.index("/* ---- Pose optimisation on the device"):txt.index("enum { ORBM_POSEOPT_MAX_FRAMES")]
    c = re.sub(r"\s*\n \*\s*", " ", c)                                       # phrases may run over a line break of the comment
    for phrase in ("Optimizer.cc:943-1286", "!pFrame->mpCamera2", "Tracking.cc:3029-3059", ":3239-3266", ":3812-3832", "held to a TOLERANCE",
                   "one parameter list, one kernel", "orbm_unproject_stereo_batch_async", "or NULL: every edge is mono",
                   "an index outside [0, nmp) is NULL", "tcw_out == tcw_in is allowed", "octave is outside [0, nlevels) is treated as NULL",
                   "the < 3 rule", "n_good = 0", "tcw_out[f] = tcw_in[f]", "the float invz", "const float invz = 1.0f / z",
                   "the round-restart rule", "EVERY round starts from the input pose", "(float)chi2 > 5.991f / 7.815f, strictly",
                   "The stale-error rule", "the error at the REJECTED pose", "the < 10 rule", "only the first round runs",
                   "empty active set", "the reduction order", "slot s belongs to thread s % 256", "xor butterfly", "in wave order",
                   "written ONLY for slots that hold a MapPoint", "nInitialCorrespondences - nBad of the last round run", "ONE launch",
                   "no scratch, no atomics", "from the first call", "cap <= 1536", "ORBM_E_INVALID, with nothing enqueued",
                   "No CPU fallback: ORBM_E_HIP without a device",
                   "there is no host form", "Tracking.cc:3038-3054", "q_mp = -1, outlier = 0, mp_seen[f][j] = 1", ":3055-3057", ":3388-3410",
                   ":3817-3819", ":3826", "plain byte stores of the value 1", "one integer atomic per wave", "nframes * nmp > 2^28"):
        assert phrase in c, phrase


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_without_a_device_the_call_fails_with_e_hip(pkg, name):
    """Without a device no handle exists; handed the NULL handle such a caller is left with, every form answers ORBM_E_HIP and "no CPU
    fallback", not a complaint about the arguments.  With a device a NULL handle is an invalid argument."""
    L = pkg.lib()
    one = np.zeros(64, np.int32)
    p = one.ctypes.data_as(C.c_void_p)                                       # never read: the handle is tested first
    args = [1 if q in INTS else 1.0 if q == "bf" else p for q in SYMBOLS[name]]
    rc = getattr(L, name)(None, *args)
    msg = L.orbm_last_error()
    if L.orbx_device_count() > 0:
        assert rc == E_INVALID and b"handle" in msg
    else:
        assert rc == E_HIP and b"no CPU fallback" in msg
    assert np.all(one == 0)
