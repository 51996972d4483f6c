"""CPU-side checks of the MapPoint refresh entry points (orbm_distinctive_descriptors, orbm_update_normal_and_depth and their
_batch_async forms): each is declared in include/orbm.h, exported by the library, listed in the package's EXPORTS and bound with
argument types that match the declaration one for one (pointer -> c_void_p, int -> c_int, float -> c_float).  No GPU; the
refused-argument cases need a handle and live in tests/test_gpu_mappoint.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (number of parameters, positions of the ints)
NAMES = {
    "orbm_distinctive_descriptors": (15, {1, 2, 3, 6}),                     # nmp, nkf_rows, cap; nobs
    "orbm_distinctive_descriptors_batch_async": (15, {1, 2, 3, 6}),
    "orbm_update_normal_and_depth": (23, {1, 2, 3, 8, 18}),                 # nmp, nkf_rows, cap; nobs; nlevels
    "orbm_update_normal_and_depth_batch_async": (23, {1, 2, 3, 8, 18}),
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
    nparams, ints = NAMES[name]
    assert len(at) == nparams
    assert all((at[i] is C.c_int) == (i in ints) and at[i] is not C.c_float for i in range(nparams))


def test_host_and_device_forms_share_their_parameter_lists():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    for name in ("orbm_distinctive_descriptors", "orbm_update_normal_and_depth"):
        a = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt).group(1)
        b = re.search(r"\bint\s+" + name + r"_batch_async\s*\(([^;]*)\)\s*;", txt).group(1)
        norm = lambda s: re.sub(r"\s+", " ", s).replace("scale_factors_host", "scale_factors").strip()
        assert norm(a) == norm(b)


def test_limits_and_wrappers(pkg):
    txt = open(os.path.join(ROOT, "include", "orbm.h")).read()
    assert re.search(r"enum\s*\{\s*ORBM_MP_MAX_OBS\s*=\s*65535\s*,\s*ORBM_MP_MAX_BATCH\s*=\s*1\s*<<\s*20\s*\}", txt)
    pkg.lib()
    for name in ("ComputeDistinctiveDescriptors", "ComputeDistinctiveDescriptorsBatchAsync", "UpdateNormalAndDepth", "UpdateNormalAndDepthBatchAsync"):
        assert callable(getattr(pkg.ORBmatcher, name))
    assert os.path.exists(os.path.join(ROOT, "orb-slam3_amd", "facade", "MapPointRefresh.h"))


def test_contract_comment_names_the_rules():
    """The header carries the contract where callers read it."""
    txt = open(os.path.join(ROOT, "include", "orbm.h")).read()
    c = txt[txt.index("/* ---- MapPoint refresh"):txt.index("int orbm_distinctive_descriptors(")]
    for phrase in ("MapPoint.cc:450-538", "MapPoint.cc:578-652", "orbm_fuse_batch_async convention", "ONE stacked row", "GetRightCameraCenter",
                   "obs_off[0] may be non-zero", "bit 0 = a right-camera observation", "bit 1 = the", "in\n * the order given",
                   # the skip rules
                   "outside [0, nkf_rows)", "min(counts_kf[row], cap)", "16-byte aligned", "4-byte aligned", "non-increasing obs_off pair", "Nothing reads out of bounds",
                   # the median, the tie rule and the 256 case
                   "(int)(0.5 * (N - 1))", "lower median", "FIRST row of least median", "strict <", "256 is a legal value", "never wraps",
                   "skipped entries counted", "keeps the\n * caller's bytes", "nothing is truncated and nothing falls back to the host",
                   # the normal
                   "NOT skipped here", "facade/cvcompat.h", "(float)(1.0 / sqrt(double sum of d^2))", "without contraction", "float addition order",
                   "scale[nlevels - 1]", "(float)(1.0 / n)", "updated = 0", "bits of a NaN are not pinned",
                   # the enqueue rules
                   "orbx_capture_begin", "nothing accumulates across graph replays", "ORBM_E_INVALID", "ORBM_E_CAPACITY", "nlevels > 12",
                   "ORBM_MP_MAX_BATCH"):
        assert phrase in c, phrase
