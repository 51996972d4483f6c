"""facade/KeyFrameCulling.h's flatten (kfcull::Flat), compiled with plain g++ against cvcompat.h on the mock types of tests/kfcull_mock.h
as a stand-alone program (tests/kfcull_facade.cpp): for every constructed case and for seeded random maps its arrays equal the flatten of
tests/second_reading_kfcull.py, bit for bit.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import kfcull_cases as kc
import second_reading_kfcull as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kfcull") / "kfcull_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-o", out, os.path.join(ROOT, "tests", "kfcull_facade.cpp")])
    return out


def _bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def write_map(path, builder, covisible):
    kfs, mps = builder.kfs, builder.mps
    index = {id(mp): i for i, mp in enumerate(mps)}
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (builder.map.init_id, len(kfs), len(mps)))
        for kf in kfs:
            f.write("%d %d %d %d %d %d %d\n" % (kf.mnId, kf.N, kf.NLeft, kf.mpCamera2, kf.mbNotErase, kf.mbBad, _bits(kf.mThDepth)))
            f.write(" ".join(str(o) for o in kf.octaves) + "\n")
            f.write(" ".join(str(_bits(v)) for v in kf.mvuRight) + "\n")
            f.write(" ".join(str(_bits(v)) for v in kf.mvDepth) + "\n")
            f.write(" ".join(str(-1 if mp is None else index[id(mp)]) for mp in kf.mvpMapPoints) + "\n")
        for mp in mps:
            obs = mp.GetObservations()
            f.write("%d %d %d " % (mp.mbBad, mp.nObs, len(obs)) + " ".join("%d %d %d" % (kf.addr, l, r) for kf, (l, r) in obs) + "\n")
        f.write("%d " % len(covisible) + " ".join(str(kf.addr) for kf in covisible) + "\n")


def run(exe, path, monocular):
    res = subprocess.run([exe, path, "1" if monocular else "0"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = {}
    for line in res.stdout.splitlines():
        name, n, *vals = line.split()
        assert int(n) == len(vals)
        out[name] = np.array([int(v) for v in vals], np.int64)
    return out


def compare(exe, tmp_path, builder, covisible, monocular):
    path = str(tmp_path / "map.txt")
    write_map(path, builder, covisible)
    got = run(exe, path, monocular)
    cands = sr.candidates(covisible)
    F = sr.flatten(cands, monocular)
    assert int(got["cap"][0]) == F["cap"] and [int(r) for r in got["rows"]] == [kf.addr for kf in F["rows"]]
    for key in ("cand_row", "counts_kf", "kf_mp", "octave", "obs_off", "obs_row", "obs_slot", "obs_flags", "mp_valid", "mp_nobs"):
        assert np.array_equal(got[key], np.asarray(F[key]).reshape(-1)), key
    if monocular:
        assert len(got["depth"]) == 0
    else:
        assert np.array_equal(got["depth"].astype(np.uint32), F["depth"].reshape(-1).view(np.uint32))
    if cands:
        assert int(got["th_depth"][0]) == _bits(F["th_depth"])
    return F


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_flatten_of_the_constructed_cases(exe, tmp_path, name):
    c = kc.case(name)
    compare(exe, tmp_path, c.builder, c.covisible, c.monocular)


def test_flatten_of_random_maps(exe, tmp_path):
    flags = set()
    for seed in range(12):
        b, cov, monocular, _ = kc.random_map(seed)
        flags.update(compare(exe, tmp_path, b, cov, monocular)["obs_flags"].tolist())
    assert {0, 1, 4} <= flags                                               # left, right and weight-2 entries all occur


def test_flatten_after_an_erasure(exe, tmp_path):
    """A map in which a KeyFrame is already bad and MapPoints went bad with it: the bad KeyFrame is passed over as a candidate and keeps
    flag bit 1 where a MapPoint still lists it."""
    c = kc.case("erasure_to_3_and_to_2")
    c.covisible[0].mbBad = True                                             # marked bad without the surgery: its entries stay
    F = compare(exe, tmp_path, c.builder, c.covisible, True)
    assert len(F["cand_row"]) == 1 and (F["obs_flags"] & 2).any()
