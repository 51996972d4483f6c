"""CPU-side checks of the batched relocalisation SearchByProjection entry point (M5): orbm_search_by_projection_kf_batch_async is declared
in include/orbm.h, exported by the library, listed in the package's EXPORTS and bound with argument types that match the declaration
one for one (pointer -> c_void_p, int -> c_int, float -> c_float).  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "orbm_search_by_projection_kf_batch_async"


def test_reloc_batch_is_declared_exported_and_bound(pkg):
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
    assert len(at) == 35 and at[27] is C.c_float and at[28] is C.c_int            # th, orb_dist
