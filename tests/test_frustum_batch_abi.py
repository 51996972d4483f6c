"""CPU-side checks of the batched isInFrustum entry point: orbm_is_in_frustum_batch_async is declared in include/orbm.h, exported by the
library, listed in the package's EXPORTS and bound with argument types that match the declaration one for one; the header contract names
its rules; without a device the call fails with ORBM_E_HIP.  No GPU; the refused-argument cases need a handle and live in
tests/test_gpu_frustum_batch.py."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "orbm_is_in_frustum_batch_async"
E_INVALID, E_HIP = -2, -5
PARAMS = ["nframes", "tcw", "ow", "nq", "q_stride", "skip", "pw", "normal", "min_dist", "max_dist", "q_shared", "k_host", "bounds_host", "bf",
          "viewing_cos_limit", "log_scale_factor", "n_scale_levels", "in_view", "proj_x", "proj_y", "proj_xr", "depth", "level", "view_cos", "n_in_view"]
INTS = {"nframes", "q_stride", "q_shared", "n_scale_levels"}
FLOATS = {"bf", "viewing_cos_limit", "log_scale_factor"}


def _header():
    return open(os.path.join(ROOT, "include", "orbm.h")).read()


def _params(name):
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert decl, name + " is not declared in orbm.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",") if a.strip()]


def test_declared_exported_and_bound(pkg):
    params = _params(NAME)
    assert [a.split()[-1].lstrip("*") for a in params[1:]] == PARAMS
    want = [C.c_void_p if "*" in a else (C.c_float if a.startswith("float ") else C.c_int) for a in params]
    assert NAME in pkg.EXPORTS
    pkg.build()
    assert hasattr(C.CDLL(pkg.LIB_PATH), NAME)
    at = getattr(pkg.lib(), NAME).argtypes
    assert at is not None and list(at) == want
    assert len(at) == 1 + len(PARAMS)
    for i, p in enumerate(PARAMS, 1):
        assert at[i] is (C.c_int if p in INTS else C.c_float if p in FLOATS else C.c_void_p), p
    assert callable(pkg.ORBmatcher.isInFrustumBatch)


def test_the_output_rows_are_the_rows_m3_takes():
    """The seven rows go straight into orbm_search_by_projection_points_batch_async: the same names, depth as its th_far row."""
    m3 = [a.split()[-1].lstrip("*") for a in _params("orbm_search_by_projection_points_batch_async")]
    for row in ("in_view", "proj_x", "proj_y", "proj_xr", "view_cos", "level", "depth", "nq", "q_stride", "q_shared"):
        assert row in m3 and row in PARAMS, row
    assert m3.index("th_far") == m3.index("depth") + 1


def test_declared_after_the_single_frame_form():
    txt = _header()
    assert txt.index("int orbm_is_in_frustum(") < txt.index("/* orbm_is_in_frustum_batch_async:") < txt.index("int " + NAME + "(")


def test_contract_comment_names_the_rules():
    """The header carries the contract where callers read it: the row layouts, the skip rule, the tail rule, which fields a rejected point
    keeps, the count."""
    txt = _header()
    c = txt[txt.index("/* orbm_is_in_frustum_batch_async:"):txt.index("int " + NAME + "(")]
    c = re.sub(r"\s*\n \*\s*", " ", c)                                       # phrases may run over a line break of the comment
    for phrase in ("Tracking.cc:3808-3862", "ONE launch", "tcw [nframes][12]", "row-major 3x4 [Rcw | tcw]", "ow [nframes][3]",
                   "min(max(nq[f], 0), q_stride)", "q_shared != 0", "host pointers", "the same bits",
                   "Skip rule", "skip [nframes][q_stride]", "NULL = none", "mnLastFrameSeen == frame.mnId || pMP->isBad()", ":3844", ":3847",
                   "in_view = 0 and NOTHING ELSE of it is written", "leaves mTrackProjX/Y alone", "ORBmatcher.cc:45-80",
                   "Tail rule", "nq[f] <= i < q_stride get in_view = 0", "other six fields are not written",
                   "-1 unless the point passed the image-bounds test", "stay set when a later gate rejects it",
                   "written only where in_view == 1", "keeps the caller's bytes",
                   "Count", "n_in_view [nframes]", "NULL = not wanted", "nToMatch (:3856)", "integer atomics", "the same on every replay",
                   "no scratch and no work buffer", "from the first call", "follows new poses, counts and skip flags",
                   "KannalaBrandt8::project", "stays with the caller", "ORBM_E_INVALID", "ORBM_E_CAPACITY", "nframes > 65535",
                   "q_stride > ORBM_LP_MAX_QUERIES", "not finite", "Nothing is enqueued on either error", "orbm_last_error names the argument",
                   "ORBM_E_HIP where there is no device (no CPU fallback)"):
        assert phrase in c, phrase


def test_without_a_device_the_call_fails_with_e_hip(pkg):
    """tests/test_abi.py pins that without a device no handle exists: orbm_create fails first, loudly, with "no CPU fallback".  The call
    keeps that order -- the device before the arguments: handed the NULL handle such a caller is left with, it answers ORBM_E_HIP and the
    same words, not a complaint about the arguments.  With a device a NULL handle is an invalid argument."""
    L = pkg.lib()
    one = np.zeros(16, np.float32)
    p = one.ctypes.data_as(C.c_void_p)                                       # never read: the handle is tested first
    rc = L.orbm_is_in_frustum_batch_async(None, 1, p, p, p, 1, None, p, p, p, p, 0, p, p, 1.0, 0.5, 0.18, 8, p, p, p, p, p, p, p, None)
    msg = L.orbm_last_error()
    if L.orbx_device_count() > 0:
        assert rc == E_INVALID and b"handle" in msg
    else:
        assert rc == E_HIP and b"no CPU fallback" in msg and b"isInFrustum batch" in msg
        h = C.c_void_p()
        assert L.orbm_create(C.byref(h), 0) == E_HIP and not h.value
    assert np.all(one == 0)
