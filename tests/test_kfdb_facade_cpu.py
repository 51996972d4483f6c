"""facade/KeyFrameDatabase.h's accumulation and selection functions, compiled with g++ -ffp-contract=off on mock types as a stand-alone
program (tests/kfdb_facade.cpp), against the second reading end to end: the candidate lists and the members of every KeyFrame afterwards,
on every constructed case and on 200 seeded random databases, in both forms.  The three result rows the functions take come from the
second reading here; tests/test_gpu_kfdb.py feeds them from the device.  No GPU."""
import os
import subprocess
from collections import Counter

import pytest

import kfdb_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kfdb") / "kfdb_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-o", out, os.path.join(ROOT, "tests", "kfdb_facade.cpp")])
    return out


def _run(exe, tmp_path, items):
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write(kc.facade_text(items))
    res = subprocess.run([exe, "select", path], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return kc.parse_facade_output(res.stdout, items)


def test_constructed_cases(exe, tmp_path):
    items = [(kc.case(n), place, kc.expected(kc.case(n), place)) for n in kc.CASE_NAMES for place in (False, True)]
    for got, (c, place, _) in zip(_run(exe, tmp_path, items), items):
        kc.check_facade(got, c, place)


def test_200_random_databases(exe, tmp_path):
    cases = [kc.random_case(s) for s in range(200)]
    items = [(c, place, kc.expected(c, place)) for c in cases for place in (False, True)]
    t, nonempty = Counter(), 0
    for got, (c, place, _) in zip(_run(exe, tmp_path, items), items):
        t.update(kc.check_facade(got, c, place))
        nonempty += any(len(v) for v in got[0].values())
    assert nonempty > 200                                                    # of 400: the lists are not trivially empty
    for key in ("neighbour_stale_score", "neighbour_is_best", "cut_by_075", "other_map", "duplicate", "not_taken", "excluded_connected"):
        assert t[key] > 0, key


def test_a_bad_keyframe_is_passed_over(exe, tmp_path):
    """The reference spins forever at KeyFrameDatabase.cc:815-816 (the second reading raises); the facade advances.  A list takes a group's
    KeyFrame whenever it is not full and the loop ends only when both are, so each list is the first n_candidates of what the second
    reading lists with room for every row, the bad KeyFrame taken out."""
    import copy
    import second_reading_kfdb as srk
    checked = 0
    for seed in range(40):
        c = copy.copy(kc.random_case(seed))
        rows = kc.expected(c, True)
        n = c.n_candidates
        c.n_candidates = len(c.rows)
        full, _, _ = kc.facade_expected(c, True)
        c.n_candidates = n
        if len(full["L"]) < 2:
            continue
        victim = full["L"][0]
        c.bad = list(c.bad); c.bad[victim] = True
        with pytest.raises(srk.BadKeyFrameSpin):
            kc.facade_expected(c, True)
        got = _run(exe, tmp_path, [(c, True, rows)])[0][0]
        assert got == {"L": [r for r in full["L"] if r != victim][:n], "M": [r for r in full["M"] if r != victim][:n]}, seed
        checked += 1
    assert checked >= 10
