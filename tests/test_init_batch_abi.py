"""CPU-side checks of the batched SearchForInitialization entry point (M9 orbm_search_for_initialization_batch_async): it is declared in
include/orbm.h, exported by the library, listed in the package's EXPORTS and bound with argument types that match the declaration one
for one (pointer -> c_void_p, int -> c_int, float -> c_float).  No GPU; the refused-argument cases need a handle and live in
tests/test_gpu_init_batch.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "orbm_search_for_initialization_batch_async"


def test_declared_exported_and_bound(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", txt)
    assert decl, NAME + " is not declared in orbm.h"
    params = [a.strip() for a in decl.group(1).split(",") if a.strip()]
    want = [C.c_void_p if "*" in a else C.c_float if re.match(r"(const\s+)?float\b", a) else C.c_int for a in params]
    assert NAME in pkg.EXPORTS
    pkg.build()
    assert hasattr(C.CDLL(pkg.LIB_PATH), NAME)
    at = getattr(pkg.lib(), NAME).argtypes
    assert at is not None and list(at) == want
    ints = {1, 2, 3, 7, 8, 21, 23}                                           # npairs, nrows1, cap1, nrows2, cap2, window_size, check_orientation
    floats = {14, 15, 16, 17, 22}                                            # min_x, min_y, inv_w, inv_h, nnratio
    assert len(at) == 27
    assert all((at[i] is C.c_int) == (i in ints) and (at[i] is C.c_float) == (i in floats) for i in range(27))


def test_contract_comment_names_the_rules():
    """The header carries the contract where callers read it."""
    txt = open(os.path.join(ROOT, "include", "orbm.h")).read()
    c = txt[txt.index("/* " + NAME):txt.index("int " + NAME)]
    for phrase in ("level-0 rule", "vMatchedDistance skip", "robbed-entry histogram rule", "In-place prev", "NOT idempotent", "two buffers",
                   "orbx_capture_begin", "ORBM_E_CAPACITY", "ORBM_INIT_MAX_CAP", "no cap on"):
        assert phrase in c, phrase
