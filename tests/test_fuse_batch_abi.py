"""CPU-side checks of the batched Fuse entry point (M13): orbm_fuse_batch_async is declared in include/orbm.h, exported by the library,
listed in the package's EXPORTS and bound with its argument types.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuse_batch_is_declared_exported_and_bound(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbm.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+orbm_fuse_batch_async\s*\(([^;]*)\)\s*;", txt)
    assert decl, "orbm_fuse_batch_async is not declared in orbm.h"
    nparams = len([a for a in decl.group(1).split(",") if a.strip()])
    assert "orbm_fuse_batch_async" in pkg.EXPORTS
    pkg.build()
    assert hasattr(C.CDLL(pkg.LIB_PATH), "orbm_fuse_batch_async")
    L = pkg.lib()
    at = L.orbm_fuse_batch_async.argtypes
    assert at is not None and len(at) == nparams
    assert at[28] is C.c_float and at[29] is C.c_int                                # th, chi2_gate
    assert at.count(C.c_float) == 7 and at.count(C.c_int) == 7
