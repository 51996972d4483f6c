"""CPU-side checks of the batched place-recognition entry points (M8 orbm_search_by_bow_kf_batch_async, M6
orbm_search_by_projection_sim3_batch_async): each is declared in include/orbm.h, exported by the library, listed in the package's EXPORTS
and bound with argument types that match the declaration one for one (pointer -> c_void_p, int -> c_int, float -> c_float).  No GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,nargs,spots", [
    ("orbm_search_by_bow_kf_batch_async", 24, {20: C.c_float, 21: C.c_int}),                       # nnratio, check_orientation
    ("orbm_search_by_projection_sim3_batch_async", 35, {27: C.c_int, 28: C.c_float, 29: C.c_int}),  # th, ratio_hamming, proj_form
])
def test_declared_exported_and_bound(pkg, name, nargs, spots):
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
    assert len(at) == nargs and all(at[i] is t for i, t in spots.items())
