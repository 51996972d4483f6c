"""The chunk boundaries of the batched SearchForInitialization (k_init_search): ORBM_INIT_ROOM (a knob of the -DORBX_AB build only) sets
the room a chunk's queries share beside the first query's own region.  At 0 no second searching query fits, so every chunk holds one
searching query and every query is deferred once; at a few thousand words chunks end at data-dependent places.  Same rows, counts and
prev_out as the oracle whatever the room is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import init_cases as ic
from test_gpu_init_batch import frames, OM, mt, Pool, run, check, own_xy   # noqa: F401  (fixtures + helpers)


@pytest.mark.parametrize("room", ["0", "3000", "70000"])
def test_chunks_end_where_the_scratch_is_full(pkg, OM, mt, frames, monkeypatch, room):
    f0, f1, f2 = frames
    A = Pool(pkg, [f0, f1], 9); B = Pool(pkg, [f1, f2], 11).build_grid(pkg.lib(), mt)
    prevs = [own_xy(f0[0]), own_xy(f1[0]), own_xy(f0[0])]
    monkeypatch.setenv("ORBM_INIT_ROOM", room)
    got = run(pkg, mt, A, B, [0, 1, 0], [0, 1, 1], prevs, 100, 0.9, 1)
    refs = check(pkg, OM, A, B, [0, 1, 0], [0, 1, 1], prevs, 100, 0.9, 1, got)
    assert min(r[0] for r in refs) >= 200
