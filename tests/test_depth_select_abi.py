"""CPU-side checks of the depth point selection entry points (orbm_select_depth_points, orbm_select_depth_points_batch_async,
orbm_adopt_new_points_batch_async): each is declared in include/orbm.h, exported by the library, listed in the package's EXPORTS and
bound with argument types that match the declaration one for one (pointer -> c_void_p, int -> c_int, float -> c_float).  No GPU; the
refused-argument cases need a handle and live in tests/test_gpu_depth_select.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (number of parameters, positions of the ints, positions of the floats)
NAMES = {
    "orbm_select_depth_points": (12, {1, 6}, {5}),                             # n; th_depth; max_points
    "orbm_select_depth_points_batch_async": (16, {1, 2, 3, 9}, {8}),           # nrows, first, cap; th_depth; max_points
    "orbm_adopt_new_points_batch_async": (13, {1, 2, 3}, set()),               # nrows, first, cap
}


def _header():
    return open(os.path.join(ROOT, "include", "orbm.h")).read()


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_exported_and_bound(pkg, name):
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
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


def test_declared_in_the_rgbd_section_after_unproject():
    txt = _header()
    assert txt.index("/* ---- RGB-D frames") < txt.index("int orbm_unproject_stereo_batch_async(") < txt.index("int orbm_select_depth_points(") \
        < txt.index("int orbm_adopt_new_points_batch_async(") < txt.index("/* ---- MapPoint refresh")


def test_limit_constant(pkg):
    assert re.search(r"enum\s*\{\s*ORBM_DEPTH_SELECT_MAX_CAP\s*=\s*16384\s*\}", _header())
    assert pkg.DEPTH_SELECT_MAX_CAP == 16384


def test_wrappers_exist(pkg):
    pkg.lib()
    for name in ("SelectDepthPoints", "SelectDepthPointsBatchAsync", "AdoptNewPointsBatchAsync"):
        assert callable(getattr(pkg.ORBmatcher, name))


def test_contract_comments_name_the_rules():
    """The header carries the contract where callers read it."""
    txt = _header()
    c = txt[txt.index("/* orbm_select_depth_points /"):txt.index("int orbm_select_depth_points(")]
    for phrase in ("Tracking.cc:3094-3163", "Tracking.cc:3694-3783", "Tracking.cc:3524-3546", "max(c, max_points) + 1", "one extra point",
                   "101 visited slots", "ties by slot", "+inf is in", "positive denormal", "NaN th_depth never stops the walk", "strict <",
                   "in neither", "Observations() < 1", "ORBM_DEPTH_SELECT_MAX_CAP = 16384", "nothing accumulates across graph replays",
                   "orbx_capture_begin", "ORBM_E_INVALID", "ORBM_E_CAPACITY", "at or beyond the count",
                   "Tracking.cc:3139-3143", "ORBmatcher.cc:2505-2509", "MapPoint.cc:92", "MapPoint.cc:127", "Every other slot is", "q_stride == cap",
                   "UnprojectStereoFishEye", "mvLeftToRightMatch"):
        assert phrase in c, phrase
    u = txt[txt.index("/* orbm_unproject_stereo /"):txt.index("int orbm_unproject_stereo(")]
    assert "ANDs its own selection" in u and "orbm_select_depth_points_batch_async" in u and "orbm_adopt_new_points_batch_async" in u
