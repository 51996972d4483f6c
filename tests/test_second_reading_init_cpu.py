"""The CPU oracle's SearchForInitialization (M9, oracle/orbref_match.cpp) against the second reading of ORBmatcher.cc:799-943
(tests/second_reading_init.py): entry for entry -- vnMatches12, the count, vbPrevMatched -- on the suite's 376 x 240 / 2 500-feature
scene with orientation on and off, on a three-frame chain that carries vbPrevMatched over, and on constructed pairs that each prove
from the second reading's branch counters that they reached the branch they were built for.  No GPU."""
import os
import re

import numpy as np
import pytest

import init_cases as ic
import second_reading as sr
import second_reading_init as sri

HERE = os.path.dirname(os.path.abspath(__file__))


def test_second_reading_imports_neither_oracle_nor_product():
    src = open(os.path.join(HERE, "second_reading_init.py")).read()
    mods = set(re.findall(r"^\s*(?:from|import)\s+([\w\.]+)", src, flags=re.M))
    assert mods == {"collections", "numpy", "second_reading"}, mods
    for word in ("orbref", "orb-slam3_amd", "importlib", "ctypes", "__import__", "liborb"):
        assert word not in src, word
    helper = open(os.path.join(HERE, "init_cases.py")).read()
    assert set(re.findall(r"^\s*(?:from|import)\s+([\w\.]+)", helper, flags=re.M)) == {"numpy"}


@pytest.fixture(scope="module")
def frames(synth, oracle):
    return ic.scene_frames(synth, oracle)


@pytest.fixture(scope="module")
def OM(oracle):
    return oracle._oracle_matcher_class()()


def _grid_frame(k, d):
    return sr.GridFrame(k, d, 0.0, 0.0, ic.INV_W, ic.INV_H)


def _both(pkg, OM, k1, d1, k2, d2, prev, window, nnratio, ori):
    f1 = pkg.FrameView(k1, d1, ic.W, ic.H, backend=OM); f2 = pkg.FrameView(k2, d2, ic.W, ic.H, backend=OM)
    n_o, m_o, p_o = OM.SearchForInitialization(f1, f2, prev, window, nnratio, ori)
    n_s, m_s, p_s, t = sri.search_for_initialization(_grid_frame(k1, d1), _grid_frame(k2, d2), prev, window, nnratio, ori)
    assert n_o == n_s, (n_o, n_s)
    assert np.array_equal(m_o, m_s), np.nonzero(m_o != m_s)[0][:10]
    assert np.array_equal(p_o.view(np.uint32), p_s.view(np.uint32))
    return n_s, m_s, p_s, t


@pytest.mark.parametrize("ori", [True, False])
def test_scene_oracle_equals_second_reading(pkg, OM, frames, ori):
    (k1, d1), (k2, d2), _ = frames
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    n, m, p, t = _both(pkg, OM, k1, d1, k2, d2, prev, 100, 0.9, ori)
    print({k: v for k, v in t.items() if not isinstance(v, tuple)})
    # not vacuous: the scene reaches the order-dependent branches
    assert t["matches_before_cull"] >= 300
    assert t["steal"] >= 1
    assert t["query_outcome_changed_by_skip"] >= 1
    assert t["level_skip"] > 0 and t["skipped_by_matched_distance"] > 0 and t["ratio_fail"] > 0 and t["over_th_low"] > 0
    if ori:
        assert t["cull_live"] >= 1 and n == t["matches_before_cull"] - t["cull_live"]
    moved = m >= 0
    assert np.array_equal(p[~moved], prev[~moved]) and np.array_equal(p[moved, 0], k2["x"][m[moved]])


def test_three_frame_chain_carries_prev(pkg, OM, frames):
    (k1, d1), (k2, d2), (k3, d3) = frames
    prev0 = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    _, m1, prev1, _ = _both(pkg, OM, k1, d1, k2, d2, prev0, 100, 0.9, True)
    assert not np.array_equal(prev0, prev1)
    n2, m2, prev2, t2 = _both(pkg, OM, k1, d1, k3, d3, prev1, ic.CHAIN_WINDOW, 0.9, True)
    assert n2 > 100
    # the carried positions matter (in a window smaller than the motion): the same step from the initial positions gives another row
    _, m2b, _, _ = sri.search_for_initialization(_grid_frame(k1, d1), _grid_frame(k3, d3), prev0, ic.CHAIN_WINDOW, 0.9, True)
    assert not np.array_equal(m2, m2b)


CASES = ic.constructed_pairs()


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_pair(pkg, OM, name):
    pair, expect = CASES[name]
    k1, d1, k2, d2, prev = pair.arrays()
    n, m, p, t = _both(pkg, OM, k1, d1, k2, d2, prev, pair.window, pair.nnratio, pair.check_ori)
    for key, want in expect.items():
        if key == "m12":
            for q, s in want.items():
                assert m[q] == s, (name, q, int(m[q]), s)
        elif key == "nmatches":
            assert n == want
        elif key == "differs_from_finished_row_cull":
            n_f, m_f = sri.cull_from_finished_row(_grid_frame(k1, d1), _grid_frame(k2, d2), np.array(t["row_before_cull"]))
            assert not np.array_equal(m_f, m)
        elif want == 0:
            assert t[key] == 0, (name, key, t[key])
        else:
            assert t[key] >= want, (name, key, t[key])
    assert n == int((m >= 0).sum())


def test_tie_winner_is_the_higher_index():
    pair, expect = CASES["tie"]
    (q, s), = expect["m12"].items()
    assert s == 1                                     # slot 1 wins over slot 0: grid order, not index order


def test_ratio_product_is_float32():
    assert not (np.float32(45) < np.float32(50) * np.float32(0.9)) and 45 < 50 * 0.9000000001
    assert np.float32(44) < np.float32(50) * np.float32(0.9)
