"""CPU-side checks of the CreateNewMapPoints entry points (orbm_triangulate_new_points, orbm_triangulate_new_points_batch_async): each is
declared in include/orbm.h, exported by the library, listed in the package's EXPORTS and bound with argument types that match the
declaration one for one; the host form is the device form's parameter list behind `space`; the limits; the header contract names the
tolerance, the cross-pair rule and the mbf1 rule; without a device the calls fail with ORBM_E_HIP.  No GPU; the refused-argument cases
need a handle and live in tests/test_gpu_triangulate.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_HIP = -2, -5
POOL = ["nrows%d", "cap%d", "kps_un%d", "kps%d", "counts%d", "uright%d", "depth%d", "tcw%d", "ow%d"]
LIST = (["ngroups", "group_start_host", "npairs"] + [p % 1 for p in POOL] + [p % 2 for p in POOL] +
        ["row1", "row2", "matches12", "k1_host", "k2_host", "mb1", "mbf1", "mb2", "scale_factors1_host", "level_sigma2_1_host",
         "scale_factors2_host", "level_sigma2_2_host", "nlevels", "ratio_factor", "th_far",
         "won_pair", "won_idx2", "x3d", "reason", "ncreated", "order", "ntotal"])
SYMBOLS = {"orbm_triangulate_new_points": ["space"] + LIST, "orbm_triangulate_new_points_batch_async": LIST}
INTS = {"space", "ngroups", "npairs", "nrows1", "cap1", "nrows2", "cap2", "nlevels"}
FLOATS = {"mb1", "mbf1", "mb2", "ratio_factor", "th_far"}


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
        assert at[i] is (C.c_int if p in INTS else C.c_float if p in FLOATS else C.c_void_p), p


def test_one_parameter_list():
    host, dev = _params("orbm_triangulate_new_points"), _params("orbm_triangulate_new_points_batch_async")
    assert host[1] == "int space" and host[:1] + host[2:] == dev


def test_declared_after_the_pose_optimisation_block():
    txt = _header()
    order = [txt.index(s) for s in ("int orbm_discard_outliers_batch_async(", "/* ---- CreateNewMapPoints behind M10", "int orbm_triangulate_new_points_batch_async(",
                                    "int orbm_triangulate_new_points(", "/* M15 Frame::ComputeStereoMatches")]
    assert order == sorted(order)


def test_limit_constants(pkg):
    assert re.search(r"enum\s*\{\s*ORBM_TRI_MAX_CAP\s*=\s*65535\s*,\s*ORBM_TRI_MAX_PAIRS\s*=\s*65535\s*,\s*ORBM_TRI_MAX_GROUP_PAIRS\s*=\s*64\s*,"
                     r"\s*ORBM_TRI_MAX_LEVELS\s*=\s*32\s*\}", _header())
    assert (pkg.TRI_MAX_CAP, pkg.TRI_MAX_PAIRS, pkg.TRI_MAX_GROUP_PAIRS, pkg.TRI_MAX_LEVELS) == (65535, 65535, 64, 32)
    kernels = open(os.path.join(ROOT, "orb-slam3_amd", "csrc", "orbm_kernels.hip.h")).read()
    shared = open(os.path.join(ROOT, "orb-slam3_amd", "csrc", "orbm_triangulate.h")).read()
    assert re.search(r"#define\s+TRI_MAX_GROUP_PAIRS\s+64\b", kernels) and re.search(r"#define\s+TRI_MAX_LEVELS\s+32\b", shared)


def test_reason_codes_are_one_list():
    """The exits are numbered once: the shared header's enum, the numbers the contract comment quotes and the second reading's names."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import second_reading_triangulate as sr
    shared = open(os.path.join(ROOT, "orb-slam3_amd", "csrc", "orbm_triangulate.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(TRI_[A-Z0-9_]+)\s*=\s*(\d+)", shared[shared.index("enum TriReason"):shared.index("TRI_FN bool tri_ok")]))
    want = {"TRI_OK_TRIANGULATED": sr.OK_TRI, "TRI_OK_STEREO1": sr.OK_ST1, "TRI_OK_STEREO2": sr.OK_ST2, "TRI_NO_MATCH": sr.NO_MATCH, "TRI_TAKEN": sr.TAKEN,
            "TRI_BAD_OCTAVE": sr.BAD_OCTAVE, "TRI_LOW_PARALLAX": sr.LOW_PARALLAX, "TRI_W_ZERO": sr.W_ZERO, "TRI_BEHIND_1": sr.BEHIND_1,
            "TRI_BEHIND_2": sr.BEHIND_2, "TRI_CHI2_1": sr.CHI2_1, "TRI_CHI2_2": sr.CHI2_2, "TRI_DIST_ZERO": sr.DIST_ZERO, "TRI_FAR": sr.FAR,
            "TRI_SCALE": sr.SCALE, "TRI_MIXED_ROW1": sr.MIXED}
    assert enum == want


def test_wrappers_exist(pkg):
    pkg.lib()
    for name in ("TriangulateNewPoints", "TriangulateNewPointsBatchAsync"):
        assert callable(getattr(pkg.ORBmatcher, name))


def test_contract_comment_names_the_rules():
    txt = _header()
    c = txt[txt.index("/* ---- CreateNewMapPoints behind M10"):txt.index("enum { ORBM_TRI_MAX_CAP")]
    c = re.sub(r"\s*\n \*\s*", " ", c)
    for phrase in ("LocalMapping.cc:609-892", "!mpCamera2", "(:552-578) stay with the caller", "held to a TOLERANCE", "NOT bit-identical to cv::SVD",
                   "C * eps32 * sigma1 / (sigma3 - sigma4)", "tests/triangulate_results.py", "there is no SVD", "bit-identical, x3d included",
                   "one parameter list", "share one row1", "is a HOST array in both forms", "is refused", "NULL = kps_un1", "one pool may be passed twice",
                   "never dereferenced", "`if (bStereo1) ... else if (bStereo2)` as written", "in double, stored to float", "< 0.9998",
                   "zeros for depth <= 0", "x3D_h(3) == 0 rejects", "invz = 1.0 / z stored to float", "The mbf1 rule", "KeyFrame 1's mbf",
                   "5.991 * sigma2", "7.8 * sigma2", "against the double product", "dist == 0 rejects", "dist >= th_far rejects",
                   "indexes no table", "the cross-pair rule", "the FIRST pair whose match passes every gate wins", "is dropped (reason 4)",
                   "leaves idx1 free for the next pair", "pair by pair, ascending idx1 inside a pair", "-1 past ntotal", "counts start from zero",
                   "nothing is atomic", "No scratch, no allocation", "from the first call", "ORBM_E_INVALID, with nothing enqueued",
                   "a ratio_factor that is not finite", "ORBM_TRI_MAX_GROUP_PAIRS", "No CPU fallback: ORBM_E_HIP without a device"):
        assert phrase in c, phrase


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_without_a_device_the_call_fails_with_e_hip(pkg, name):
    """Without a device no handle exists; handed the NULL handle such a caller is left with, both forms answer ORBM_E_HIP and "no CPU
    fallback", not a complaint about the arguments.  With a device a NULL handle is an invalid argument."""
    L = pkg.lib()
    one = np.zeros(64, np.int32)
    p = one.ctypes.data_as(C.c_void_p)                                       # never read: the handle is tested first
    args = [(0 if q == "space" else 1) if q in INTS else 1.0 if q in FLOATS else p for q in SYMBOLS[name]]
    rc = getattr(L, name)(None, *args)
    msg = L.orbm_last_error()
    if L.orbx_device_count() > 0:
        assert rc == E_INVALID and b"handle" in msg
    else:
        assert rc == E_HIP and b"no CPU fallback" in msg
    assert np.all(one == 0)
