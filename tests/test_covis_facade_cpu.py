"""facade/Covisibility.h compiled with plain g++ against cvcompat.h on the mock types of tests/kfcull_mock.h as a stand-alone program
(tests/covis_facade.cpp, which supplies the two host entry points as plain loops over the header's contract): for every constructed case
and for seeded random maps the facade's flatten equals the flatten of tests/second_reading_covis.py array for array, and its three
results -- ConnectionCountsBatch, LocalKeyFrameVotes with the cleared slots, LocalMapPoints -- equal the second reading and the reference's
loops restated in the program.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import covis_cases as cc
import second_reading_covis as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("covis") / "covis_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", out, os.path.join(ROOT, "tests", "covis_facade.cpp")])
    return out


def _bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def write_map(path, kfs, frame, local):
    """The KeyFrames in pointer order (the program keeps them in one vector, so index order is pointer order there)."""
    order = sorted(kfs, key=lambda k: k.addr)
    kidx = {id(k): i for i, k in enumerate(order)}
    mps, midx = [], {}
    for mp in [mp for kf in order for mp in kf.mvpMapPoints] + list(frame.mvpMapPoints):
        if mp is not None and id(mp) not in midx:
            midx[id(mp)] = len(mps); mps.append(mp)
    main = order[0].map if order else None
    for kf in order:                                                        # the first map is the one most KeyFrames lie in
        if sum(k.map is kf.map for k in order) > sum(k.map is main for k in order):
            main = kf.map
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (10 ** 6, len(order), len(mps)))
        for kf in order:
            f.write("%d %d %d %d %d %d %d\n" % (kf.mnId, kf.N, kf.NLeft, kf.mpCamera2, 0, kf.mbBad, _bits(kf.mThDepth)))
            f.write(" ".join(str(o) for o in kf.octaves) + "\n")
            f.write(" ".join(str(_bits(v)) for v in kf.mvuRight) + "\n")
            f.write(" ".join(str(_bits(v)) for v in kf.mvDepth) + "\n")
            f.write(" ".join(str(-1 if mp is None else midx[id(mp)]) for mp in kf.mvpMapPoints) + "\n")
        for mp in mps:
            obs = mp.GetObservations()
            f.write("%d %d %d " % (mp.mbBad, mp.nObs, len(obs)) + " ".join("%d %d %d" % (kidx[id(kf)], l, r) for kf, (l, r) in obs) + "\n")
        f.write("0\n")
        others = [kidx[id(k)] for k in order if k.map is not main]
        f.write("%d " % len(others) + " ".join(map(str, others)) + "\n")
        f.write("%d " % frame.N + " ".join(str(-1 if mp is None else midx[id(mp)]) for mp in frame.mvpMapPoints) + "\n")
        f.write("%d " % len(local) + " ".join(str(kidx[id(k)]) for k in local) + "\n")
    return order, mps, main


def run(exe, path):
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = {}
    for line in res.stdout.splitlines():
        name, n, *vals = line.split()
        assert int(n) == len(vals), line
        out[name] = np.array([int(v) for v in vals], np.int64)
    return out


def compare(exe, tmp_path, kfs, frame, local):
    path = str(tmp_path / "map.txt")
    order, mps, main = write_map(path, kfs, frame, local)
    got = run(exe, path)
    assert got["same_as_reference_loops"][0] == 1
    queries = [kf for kf in order if not kf.isBad() and kf.map is main]
    if queries:
        F = sr.flatten_votes([kf.GetMapPointMatches() for kf in queries], queries, main)
        assert int(got["cap"][0]) == F["cap"] and int(got["q_stride"][0]) == F["q_mp"].shape[1]
        assert [int(r) for r in got["rows"]] == [order.index(kf) for kf in F["rows"]]
        for key in ("q_mp", "q_n", "self_row", "counts_kf", "kf_skip", "obs_off", "obs_row", "obs_slot", "obs_flags", "mp_valid"):
            if key in ("obs_off", "mp_valid") and not F["mps"]:
                continue                                                    # no MapPoint: the reading pads one, the facade makes no call
            assert np.array_equal(got[key], np.asarray(F[key]).reshape(-1)), key
        for q, kf in enumerate(queries):
            pairs = got["conn%d" % q].reshape(-1, 2)
            assert {order[int(k)]: int(v) for k, v in pairs} == sr.ConnectionCounts(kf), q
            assert list(pairs[:, 0]) == sorted(pairs[:, 0])                 # the map is in pointer order
    want_frame = sr.LocalKeyFrameVotes(frame)                               # clears the bad slots of `frame`
    assert {order[int(k)]: int(v) for k, v in got["frame0"].reshape(-1, 2)} == want_frame
    assert [int(j) for j in got["frame_slots"]] == [-1 if mp is None else mps.index(mp) for mp in frame.mvpMapPoints]
    assert [mps[int(j)] if int(j) < len(mps) else None for j in got["local"]] == sr.LocalMapPoints(local, 4242)
    return got


@pytest.mark.parametrize("name", sorted(cc.VOTE_CASES))
def test_vote_cases(exe, tmp_path, name):
    kfs, who, _ = cc.VOTE_CASES[name]()
    frame = who if isinstance(who, sr.Frame) else sr.Frame(1, kfs[0].GetMapPointMatches())
    compare(exe, tmp_path, kfs, frame, kfs[::-1])


@pytest.mark.parametrize("name", sorted(cc.LOCAL_CASES))
def test_local_point_cases(exe, tmp_path, name):
    local, want = cc.LOCAL_CASES[name]()
    kfs = sorted(set(local), key=lambda k: k.addr)
    if not kfs:
        _, kfs = cc.world(1)
    got = compare(exe, tmp_path, kfs, sr.Frame(1, []), local)
    assert len(got["local"]) == len(want)


def test_random_maps(exe, tmp_path):
    flags = set()
    for seed in range(25):
        kfs, frame, local = cc.random_map(seed)
        got = compare(exe, tmp_path, kfs, frame, local)
        flags.update(got.get("obs_flags", np.zeros(0)).tolist())
    assert {0, 1, 2, 3} <= flags                                            # left, right and bad-KeyFrame entries all occur
