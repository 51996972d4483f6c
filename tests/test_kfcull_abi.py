"""CPU-side checks of the KeyFrameCulling entry points (orbm_keyframe_culling, orbm_keyframe_culling_batch_async): each is declared in
include/orbm.h, exported by the library, listed in the package's EXPORTS and bound with argument types that match the declaration one for
one; the host and the device form share their parameter list; the two limits; the header contract names its rules; without a device the
calls fail with ORBM_E_HIP.  No GPU; the refused-argument cases need a handle and live in tests/test_gpu_kfcull.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbm_keyframe_culling", "orbm_keyframe_culling_batch_async")
E_INVALID, E_HIP = -2, -5
PARAMS = ["ncand", "cand_row", "nkf_rows", "cap", "kps_kf", "counts_kf", "kf_mp", "depth", "th_depth", "nmp", "nobs", "obs_off", "obs_row",
          "obs_slot", "obs_flags", "mp_valid", "mp_nobs", "erased", "th_obs", "redundant_th", "n_mps", "n_redundant", "cull", "slot_state",
          "first_cull"]
INTS = {"ncand", "nkf_rows", "cap", "nmp", "nobs", "th_obs"}
FLOATS = {"th_depth", "redundant_th"}


def _header():
    return open(os.path.join(ROOT, "include", "orbm.h")).read()


def _params(name):
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert decl, name + " is not declared in orbm.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(pkg, name):
    params = _params(name)
    assert [a.split()[-1].lstrip("*") for a in params[1:]] == PARAMS
    want = [C.c_void_p if "*" in a else (C.c_float if a.startswith("float ") else C.c_int) for a in params]
    assert name in pkg.EXPORTS
    pkg.build()
    assert hasattr(C.CDLL(pkg.LIB_PATH), name)
    at = getattr(pkg.lib(), name).argtypes
    assert at is not None and list(at) == want
    assert len(at) == 1 + len(PARAMS)
    for i, p in enumerate(PARAMS, 1):
        assert at[i] is (C.c_int if p in INTS else C.c_float if p in FLOATS else C.c_void_p), p


def test_host_and_device_form_share_their_parameter_list():
    assert _params(NAMES[0]) == _params(NAMES[1])


def test_declared_after_the_keyframe_database():
    txt = _header()
    assert txt.index("int orbm_kfdb_query_batch_async(") < txt.index("/* ---- KeyFrameCulling") < txt.index("int orbm_keyframe_culling(") \
        < txt.index("int orbm_keyframe_culling_batch_async(")


def test_limit_constants(pkg):
    assert re.search(r"enum\s*\{\s*ORBM_KFCULL_MAX_CAND\s*=\s*65535\s*,\s*ORBM_KFCULL_MAX_CAP\s*=\s*65535\s*\}", _header())
    assert pkg.KFCULL_MAX_CAND == 65535 and pkg.KFCULL_MAX_CAP == 65535


def test_wrappers_exist(pkg):
    pkg.lib()
    for name in ("KeyframeCulling", "KeyframeCullingBatchAsync"):
        assert callable(getattr(pkg.ORBmatcher, name))


def test_contract_comment_names_the_rules():
    """The header carries the contract where callers read it."""
    txt = _header()
    c = txt[txt.index("/* ---- KeyFrameCulling"):txt.index("enum { ORBM_KFCULL_MAX_CAND")]
    c = re.sub(r"\s*\n \*\s*", " ", c)                                       # phrases may run over a line break of the comment
    for phrase in ("LocalMapping.cc:1218-1400", "one parameter list", "MapPoint refresh convention exactly", "one stacked row", "ORBM_MP_MAX_OBS",
                   "in the order of GetVectorCovisibleKeyFrames()", "mnId == GetInitKFid() || isBad()", ":1272",
                   "an index outside [0, nmp) means NULL", "NULL means mbMonocular", "NULL = all valid", "mp_nobs [nmp] = Observations()",
                   "NULL = none", "th_obs is 3", "0.9f or 0.5f", ":1238-1245",
                   "Bit 2 of obs_flags: the entry weighs 2 in nObs", "MapPoint.cc:212, :232", "The two refresh calls ignore bit 2",
                   "Bit 1 (the KeyFrame isBad()) is ignored here",
                   "r out of range or erased[r] set gives zeros", "mp_valid[j] == 0: the slot is not counted",
                   "nobs_eff = mp_nobs[j] - the sum of the weights of E", "E is not empty and nobs_eff <= 2", "bad by erasure",
                   "MapPoint.cc:220-257", ":280-305", "nObs only falls",
                   "depth[k][i] > th_depth || depth[k][i] < 0", ":1295", "A NaN depth is counted, -0.0 is counted, depth == th_depth is counted",
                   "If nobs_eff > th_obs", "is not erased and is not r", "octave <= L + 1", "directly preceded in the list by a left entry of the same row",
                   "counts once if either entry passes", ":1316-1328", "defined here, not by the reference", "break at :1335",
                   "(float)n_redundant > redundant_th * (float)n_mps", "no contraction", ":1349", "9 of 10 is not culled and 10 of 11 is",
                   "the least k with cull[k] set, or -1", "0 = not counted, 1 = counted, 2 = redundant", "Every slot below cap is written",
                   "Deviation", "mvKeysRight[i].octave with the stacked index i", ":1303-1305", "reads slot i of the stacked row",
                   "The sequential rule", "KeyFrame.cc:746-887", "exact for candidates 0 .. first_cull", ":1352-1387", "stay with the caller",
                   "mbNotErase leaves it alive", "sets erased[row] = 1 and calls again for the remaining candidates",
                   "No CSR, pool or kf_mp row is rebuilt", "Only while erased is all zero or NULL",
                   "exists exactly where X's mvpMapPoints holds that MapPoint",
                   "returns the number of candidates with cull set", "no scratch that survives a call", "integer atomics",
                   "nothing accumulates across graph replays", "from the first call",
                   "follows rewritten erased, kf_mp, mp_valid, mp_nobs and cand_row rows", "the outputs are the same",
                   "Nothing reads out of bounds", "ORBM_E_INVALID, with nothing enqueued", "th_obs < 0", "ORBM_E_CAPACITY",
                   "ORBM_KFCULL_MAX_CAND", "ORBM_KFCULL_MAX_CAP", "nkf_rows * cap > 2^31 - 1", "No CPU fallback: ORBM_E_HIP without a device"):
        assert phrase in c, phrase


def test_facade_states_the_deviation_and_the_invariant():
    txt = open(os.path.join(ROOT, "orb-slam3_amd", "facade", "KeyFrameCulling.h")).read()
    txt = re.sub(r"\s*\n//\s*", " ", txt)
    for phrase in ("mvKeysRight[i].octave", ":1303-1305", "slot i of the stacked row", "exists exactly where X's mvpMapPoints holds that MapPoint",
                   "UpdateBestCovisibles", ":1272", ":1395", "onRedundant", "SetBadFlag", "erased"):
        assert phrase in txt, phrase


@pytest.mark.parametrize("name", NAMES)
def test_without_a_device_the_call_fails_with_e_hip(pkg, name):
    """Without a device no handle exists (orbm_create fails with "no CPU fallback"); handed the NULL handle such a caller is left with,
    both forms answer ORBM_E_HIP and the same words, not a complaint about the arguments.  With a device a NULL handle is an invalid
    argument."""
    L = pkg.lib()
    one = np.zeros(16, np.int32)
    p = one.ctypes.data_as(C.c_void_p)                                       # never read: the handle is tested first
    rc = getattr(L, name)(None, 1, p, 1, 1, p, p, p, None, 35.0, 1, 1, p, p, p, p, None, p, None, 3, 0.9, p, p, p, None, None)
    msg = L.orbm_last_error()
    if L.orbx_device_count() > 0:
        assert rc == E_INVALID and b"handle" in msg
    else:
        assert rc == E_HIP and b"no CPU fallback" in msg and b"KeyFrameCulling" in msg
    assert np.all(one == 0)
