"""CPU-side checks of the RGB-D entry points (orbm_stereo_from_rgbd, orbm_stereo_from_rgbd_batch_async, orbm_unproject_stereo,
orbm_unproject_stereo_batch_async): each is declared in include/orbm.h, exported by the library, listed in the package's EXPORTS and
bound with argument types that match the declaration one for one (pointer -> c_void_p, int -> c_int, float -> c_float).  No GPU; the
refused-argument cases need a handle and live in tests/test_gpu_rgbd.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (number of parameters, positions of the ints, positions of the floats)
NAMES = {
    "orbm_stereo_from_rgbd": (13, {1, 5, 6, 7, 8}, {9, 10}),                    # n; depth_type, w, h, stride_bytes; depth_factor, mbf
    "orbm_stereo_from_rgbd_batch_async": (17, {1, 2, 3, 8, 9, 10, 11}, {12, 13}),   # nframes, first, cap; depth_type, w, h, stride_bytes
    "orbm_unproject_stereo": (8, {1}, set()),                                  # n
    "orbm_unproject_stereo_batch_async": (11, {1, 2, 3}, set()),               # nrows, first, cap
}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_exported_and_bound(pkg, name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert decl, name + " is not declared in orbm.h"
    params = [a.strip() for a in decl.group(1).split(",") if a.strip()]
    want = [C.c_void_p if "*" in a else C.c_float if re.match(r"(const\s+)?float\b", a) else C.c_int for a in params]
    assert name in pkg.EXPORTS
    pkg.build()
    assert hasattr(C.CDLL(pkg.LIB_PATH), name)
    at = getattr(pkg.lib(), name).argtypes
    assert at is not None and list(at) == want
    nparams, ints, floats = NAMES[name]
    assert len(at) == nparams
    assert all((at[i] is C.c_int) == (i in ints) and (at[i] is C.c_float) == (i in floats) for i in range(nparams))


def test_depth_type_constants(pkg):
    txt = open(os.path.join(ROOT, "include", "orbm.h")).read()
    assert re.search(r"enum\s*\{\s*ORBM_DEPTH_U16\s*=\s*0\s*,\s*ORBM_DEPTH_F32\s*=\s*1\s*\}", txt)
    assert (pkg.DEPTH_U16, pkg.DEPTH_F32) == (0, 1)


def test_contract_comments_name_the_rules():
    """The header carries the contract where callers read it."""
    txt = open(os.path.join(ROOT, "include", "orbm.h")).read()
    c = txt[txt.index("/* ---- RGB-D frames"):txt.index("int orbm_stereo_from_rgbd(")]
    for phrase in ("Frame.cc:1279-1309", "Tracking.cc:1353-1354", "truncation", "reads out of bounds", "fabs(depth_factor - 1.0f) > 1e-5",
                   "one float32 multiply", "+inf passes", "DEVICE array of nframes device pointers", "at or beyond the frame's count",
                   "nothing accumulates across graph replays", "orbx_capture_begin", "ORBM_E_INVALID", "non-finite depth_factor"):
        assert phrase in c, phrase
    c = txt[txt.index("/* orbm_unproject_stereo /"):txt.index("int orbm_unproject_stereo(")]
    for phrase in ("Frame.cc:1312-1326", "invfx", "left to right", "cv::Mat product rule", "not the Matx rule", "has_depth = 0",
                   "orbm_project_last_frame_batch_async", "ANDs its own selection", "orbx_capture_begin"):
        assert phrase in c, phrase
