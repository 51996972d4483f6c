"""CPU-side checks of the covisibility entry points (orbm_covisibility_votes, orbm_local_points and their _batch_async forms,
orbm_gather_map_points_batch_async): each is declared in include/orbm.h, exported by the library, listed in the package's EXPORTS and
bound with argument types that match the declaration one for one; host and device forms share their parameter lists; the limits; the
header contract names its rules; without a device the calls fail with ORBM_E_HIP.  No GPU; the refused-argument cases need a handle and
live in tests/test_gpu_covis.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_HIP = -2, -5
VOTES = ["nq", "q_stride", "q_mp", "q_n", "self_row", "nkf_rows", "cap", "counts_kf", "kf_skip", "skip_bad", "nmp", "nobs", "obs_off", "obs_row",
         "obs_slot", "obs_flags", "mp_valid", "th", "list_cap", "votes", "n_voted", "max_votes", "n_over", "list_row", "list_votes"]
LOCAL = ["T", "lkf_stride", "lkf_row", "n_lkf", "nkf_rows", "cap", "counts_kf", "kf_mp", "nmp", "mp_valid", "q_stride", "local_mp", "n_total", "nq"]
GATHER = ["T", "q_stride", "local_mp", "nq", "nmp", "mp_pw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc", "mp_nobs", "mp_skip",
          "pw", "normal", "min_dist", "max_dist", "qdesc", "mp_obs", "skip"]
SYMBOLS = {"orbm_covisibility_votes": VOTES, "orbm_covisibility_votes_batch_async": VOTES, "orbm_local_points": LOCAL,
           "orbm_local_points_batch_async": LOCAL, "orbm_gather_map_points_batch_async": GATHER}
INTS = {"nq", "q_stride", "nkf_rows", "cap", "skip_bad", "nmp", "nobs", "th", "list_cap", "T", "lkf_stride"}


def _header():
    return open(os.path.join(ROOT, "include", "orbm.h")).read()


def _params(name):
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert decl, name + " is not declared in orbm.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_declared_exported_and_bound(pkg, name):
    params = _params(name)
    assert [a.split()[-1].lstrip("*") for a in params[1:]] == SYMBOLS[name]
    want = [C.c_void_p if "*" in a else C.c_int for a in params]
    assert name in pkg.EXPORTS
    pkg.build()
    assert hasattr(C.CDLL(pkg.LIB_PATH), name)
    at = getattr(pkg.lib(), name).argtypes
    assert at is not None and list(at) == want
    for i, p in enumerate(SYMBOLS[name], 1):
        is_int = p in INTS and not (name.startswith("orbm_local_points") and p == "nq") and not (name.startswith("orbm_gather") and p == "nq")
        assert at[i] is (C.c_int if is_int else C.c_void_p), p


def test_host_and_device_forms_share_their_parameter_lists():
    assert _params("orbm_covisibility_votes") == _params("orbm_covisibility_votes_batch_async")
    assert _params("orbm_local_points") == _params("orbm_local_points_batch_async")


def test_declared_after_keyframe_culling():
    txt = _header()
    order = [txt.index(s) for s in ("int orbm_keyframe_culling_batch_async(", "/* ---- Covisibility votes and the local map", "int orbm_covisibility_votes(",
                                    "int orbm_covisibility_votes_batch_async(", "int orbm_local_points(", "int orbm_local_points_batch_async(",
                                    "int orbm_gather_map_points_batch_async(", "/* M15 Frame::ComputeStereoMatches")]
    assert order == sorted(order)


def test_limit_constants(pkg):
    h = _header()
    assert re.search(r"enum\s*\{\s*ORBM_COVIS_MAX_QUERIES\s*=\s*65535\s*,\s*ORBM_COVIS_MAX_SLOTS\s*=\s*65535\s*,\s*ORBM_COVIS_MAX_ROWS\s*=\s*1\s*<<\s*20\s*,"
                     r"\s*ORBM_COVIS_MAX_VOTES\s*=\s*1\s*<<\s*28\s*\}", h)
    assert re.search(r"enum\s*\{\s*ORBM_LOCALPTS_MAX_FRAMES\s*=\s*65535\s*,\s*ORBM_LOCALPTS_MAX_KFS\s*=\s*65535\s*,\s*ORBM_LOCALPTS_MAX_CAP\s*=\s*65535\s*\}", h)
    assert (pkg.COVIS_MAX_QUERIES, pkg.COVIS_MAX_SLOTS, pkg.COVIS_MAX_ROWS, pkg.COVIS_MAX_VOTES) == (65535, 65535, 1 << 20, 1 << 28)
    assert (pkg.LOCALPTS_MAX_FRAMES, pkg.LOCALPTS_MAX_KFS, pkg.LOCALPTS_MAX_CAP) == (65535, 65535, 65535)


def test_wrappers_exist(pkg):
    pkg.lib()
    for name in ("CovisibilityVotes", "CovisibilityVotesBatchAsync", "LocalPoints", "LocalPointsBatchAsync", "GatherMapPointsBatchAsync"):
        assert callable(getattr(pkg.ORBmatcher, name))


def test_contract_comment_names_the_rules():
    """The header carries the contract where callers read it."""
    txt = _header()
    c = txt[txt.index("/* ---- Covisibility votes and the local map"):txt.index("enum { ORBM_COVIS_MAX_QUERIES")]
    c = re.sub(r"\s*\n \*\s*", " ", c)                                       # phrases may run over a line break of the comment
    for phrase in ("KeyFrame.cc:474-512", "Tracking.cc:3964-4013", "Tracking.cc:3917-3948", "one parameter list", "MapPoint refresh convention exactly",
                   "ORBM_MP_MAX_OBS", "used only for the slot skip rule", "a negative count reads as 0", "an index outside [0, nmp) means NULL",
                   "mnId == mnId, KeyFrame.cc:503", "-1, or a NULL array, means no self row", "GetMap() != mpMap", "NULL = all valid",
                   "th is 15 for UpdateConnections", "Bit 1 = the KeyFrame isBad()", "UpdateConnections passes 1", ":4033", "Bit 2 is ignored here",
                   "in any order", "one entry per KeyFrame", "directly preceded in the list by a live, non-skipped left entry of the same row",
                   "the pair rule of KeyFrameCulling", "defined here, not by the reference", "votes twice", "the rows with votes > 0 in ascending row order",
                   "the first min(n_voted, list_cap) entries are written", "keeps the caller's bytes", "list_cap may be 0 with both pointers NULL",
                   "first maximum in pointer order with strict >", "(weight, pointer) pairs", "the library reports only counts", "uses no scratch",
                   "zeroed by memsets inside the enqueued work", "integer atomics", "nothing accumulates across graph replays", "from the first call",
                   "follows rewritten q_mp, q_n, self_row and kf_skip rows", "Nothing reads out of bounds", "ORBM_E_INVALID, with nothing enqueued",
                   "nq * nkf_rows > ORBM_COVIS_MAX_VOTES", "No CPU fallback: ORBM_E_HIP without a device",
                   "IN THE ORDER WALKED", "reverse iterator", "lays the list out reversed", "a row outside [0, nkf_rows) contributes nothing",
                   "kf_mp [nkf_rows][cap] is pool-wide", "FIRST position in (k, i) lexicographic order", "mnTrackReferenceForFrame", ":3938-3944",
                   "A KeyFrame listed twice emits nothing the second time", "the order of mvpLocalMapPoints", "nq [T] = min(n_total, q_stride)",
                   "Emissions beyond q_stride are dropped", "slots at and beyond nq keep the caller's bytes", "handle-owned", "grown by an eager call",
                   "with no allocation and can be captured", "lkf_stride * cap > 2^31 - 1", "T * nmp > ORBM_COVIS_MAX_VOTES",
                   "there is no host form", "mp_nobs > 0", "mnLastFrameSeen == mnId", "Every source / destination pair is optional",
                   "Entries at and beyond nq[f] keep the caller's bytes", "gets skip = 1 and nothing else", "16-byte aligned", "two 128-bit words",
                   "No scratch; capturable from the first call"):
        assert phrase in c, phrase


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_without_a_device_the_call_fails_with_e_hip(pkg, name):
    """Without a device no handle exists; handed the NULL handle such a caller is left with, every form answers ORBM_E_HIP and "no CPU
    fallback", not a complaint about the arguments.  With a device a NULL handle is an invalid argument."""
    L = pkg.lib()
    one = np.zeros(64, np.int32)
    p = one.ctypes.data_as(C.c_void_p)                                       # never read: the handle is tested first
    args = [1 if q in INTS else p for q in SYMBOLS[name]]
    if not name.startswith("orbm_covisibility"):
        args = [p if q == "nq" else a for q, a in zip(SYMBOLS[name], args)]
    rc = getattr(L, name)(None, *args)
    msg = L.orbm_last_error()
    if L.orbx_device_count() > 0:
        assert rc == E_INVALID and b"handle" in msg
    else:
        assert rc == E_HIP and b"no CPU fallback" in msg
    assert np.all(one == 0)
