"""CPU-side checks of the batched two-camera SearchLocalPoints entry point (M3 with Nleft != -1,
orbm_search_by_projection_points_fisheye_batch_async): declared in include/orbm.h, exported by both builds of the library (the product
one and the -DORBX_AB one), listed in the package's EXPORTS, bound with argument types that match the declaration one for one, and a
NULL handle is refused with ORBM_E_INVALID before anything touches a device.  No GPU; the other refusals need a handle and live in
tests/test_gpu_local_points_fisheye_batch.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "orbm_search_by_projection_points_fisheye_batch_async"
AB_LIB = os.path.join(ROOT, "orb-slam3_amd", "liborbslam3_amd_ab.so")
SF_ARG = 37                                                                    # scale_factors_host, the one host pointer


def _declared_types():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", txt)
    assert decl, NAME + " is not declared in orbm.h"
    params = [a.strip() for a in decl.group(1).split(",") if a.strip()]
    assert params[SF_ARG].endswith("scale_factors_host")
    return [C.c_void_p if "*" in a else C.c_float if re.match(r"(const\s+)?float\b", a) else C.c_int for a in params]


def test_declared_exported_and_bound(pkg):
    want = _declared_types()
    assert len(want) == 42
    assert NAME in pkg.EXPORTS
    pkg.build()
    assert os.path.exists(AB_LIB), "the -DORBX_AB build of the library is missing"
    for path in (pkg.LIB_PATH, AB_LIB):
        assert hasattr(C.CDLL(path), NAME), path
    at = getattr(pkg.lib(), NAME).argtypes
    assert at is not None and list(at) == want


def test_null_handle_is_invalid(pkg):
    """ORBM_E_INVALID for a NULL handle, from both builds; nothing is dereferenced."""
    want = _declared_types()
    pkg.build()
    for path in (pkg.LIB_PATH, AB_LIB):
        fn = getattr(C.CDLL(path), NAME)
        fn.argtypes = want
        fn.restype = C.c_int
        buf = (C.c_uint8 * 4096)()
        p = C.addressof(buf)
        sf = (C.c_float * 8)(*[1.0] * 8)
        args = [None if i == 0 else (C.addressof(sf) if i == SF_ARG else p) if t is C.c_void_p else 1.0 if t is C.c_float else 4 for i, t in enumerate(want)]
        assert want[SF_ARG] is C.c_void_p
        assert fn(*args) == -2


def test_contract_comment_names_the_rules():
    """The header carries the contract where callers read it: every rule with its reference lines."""
    txt = open(os.path.join(ROOT, "include", "orbm.h")).read()
    c = txt[txt.index("/* " + NAME):txt.index("int " + NAME)]
    for phrase in ("ORBmatcher.cc:45-239", ":56-60", ":65-168", ":107", ":125-141", ":147", ":151-152", ":154", ":157-161", ":170-236", ":172",
                   ":173-176", ":224-233", ":2551", "NO th factor", "mvLeftToRightMatch", "mvRightToLeftMatch", "mvpMapPoints[Nleft + k]",
                   "0 <= l2r[k] < counts[right row]", "0 <= r2l[k] < counts[left row]", "ORBM_NO_MATCH", "orbx_capture_begin", "ORBM_E_INVALID",
                   "ORBM_E_CAPACITY", "KannalaBrandt8", "q_shared", "reads nothing else of its row", "orbm_search_by_projection_points_fisheye"):
        assert phrase in c, phrase
