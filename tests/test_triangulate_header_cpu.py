"""orb-slam3_amd/csrc/orbm_triangulate.h -- the arithmetic k_triangulate_new executes -- built with g++ as the stand-alone program
tests/triangulate_header.cpp (-ffp-contract=off) and run on every case of tests/triangulate_cases.py against the second reading: reason,
won_pair, won_idx2, ncreated, order and ntotal equal the reading exactly, with no match excluded; on the UnprojectStereo_ branches x3D
equals the reading bit for bit; on the triangulated branch the sign-aligned unit x3D_h lies within C eps32 sigma1 / (sigma3 - sigma4) of
the reading's float64 null vector.  C = 4 x the ratio an independent float32 SVD shows on the same matches, measured here again
(tests/triangulate_results.py).  The program is also built with -fsanitize=address,undefined and run directly on the same cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_reading_triangulate as sr            # noqa: E402
import triangulate_io as io                        # noqa: E402
import triangulate_results as res                  # noqa: E402
import test_second_reading_triangulate_cpu as hand  # noqa: E402

SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("triangulate_header")
    return d, io.build_program(d)


@pytest.fixture(scope="module")
def header_results(built):
    d, exe = built
    return {name: io.run_program(exe, c, d, name) for name, c in res.cases().items()}


def test_c_is_four_times_the_measured_float32_svd():
    m = res.measure_float32_svd()
    print("np.linalg.svd on the float32 A: largest ratio %.4f; committed %.4f, C = %.4f" % (m, res.MEASURED_RATIO, res.C))
    assert res.C == 4 * res.MEASURED_RATIO and 0.5 * res.MEASURED_RATIO < m <= res.MEASURED_RATIO


@pytest.mark.parametrize("name", sorted(res.tc.CASES) + sorted(res.tc.GPU_CASES))
def test_header_against_the_reading(header_results, name):
    h = header_results[name]
    worst = res.check_against_reading(res.cases()[name], res.reading(name), h, "header", xh=h["xh"])
    print("%s: largest x3D_h distance / bound = %.3f (bound = C eps32 s1 / (s3 - s4), C = %.4f)" % (name, worst, res.C))


def test_sanitized_build_agrees(built, header_results):
    d, _ = built
    exe = io.build_program(d, extra=SAN)
    for name, c in res.cases().items():
        s = io.run_program(exe, c, d, name + "_san")
        for key in io.OUT_KEYS + ("xh",):
            assert s[key].tobytes() == header_results[name][key].tobytes(), (name, key)


@pytest.mark.parametrize("name", sorted(hand.GATES))
def test_hand_placed_gates(built, name):
    """Every exit on the hand-placed inputs of the second reading's own test, x3D_h(3) == 0 and dist == 0 among them."""
    d, exe = built
    make, want = hand.GATES[name]
    c = make()
    h = io.run_program(exe, c, d, "gate_" + name)
    assert h["reason"][0, 0] == want, (sr.NAMES[h["reason"][0, 0]], sr.NAMES[want])
    assert h["ntotal"][0] == (1 if want <= sr.OK_ST2 else 0) and h["won_pair"][0, 0] == (0 if want <= sr.OK_ST2 else -1)


def test_rules_where_the_other_reading_differs(built):
    d, exe = built
    X, T1, T2 = hand.X, hand.T1, hand.T2
    mbf2 = np.float32(0.2) * hand.tc.K[0]
    a = hand.tc.single(hand.feature(T1, X), hand.feature(T2, X, stereo=True, mbf=hand.tc.MBF), T1, T2, mb2=0.2)
    b = hand.tc.single(hand.feature(T1, X), hand.feature(T2, X, stereo=True, mbf=mbf2), T1, T2, mb2=0.2)
    assert io.run_program(exe, a, d, "mbf_a")["reason"][0, 0] == sr.OK_TRI and io.run_program(exe, b, d, "mbf_b")["reason"][0, 0] == sr.CHI2_2
    e = hand.tc.single(hand.feature(T1, X, stereo=True, depth=200.0), hand.feature(T2, X, stereo=True, depth=0.4), T1, T2)
    assert io.run_program(exe, e, d, "elseif")["reason"][0, 0] == sr.OK_TRI


def test_garbage_matches_and_rows_read_as_no_match(built):
    d, exe = built
    c = dict(res.cases()["mono_3"])
    m = c["matches12"].copy(); n2 = int(c["pool2"]["counts"][1])
    m[1, :6] = [-2, -(2 ** 31), 2 ** 31 - 1, n2, c["pool2"]["kps_un"].shape[1], 10 ** 6]
    c["matches12"] = m; c["row2"] = c["row2"].copy(); c["row2"][2] = 99
    h = io.run_program(exe, c, d, "garbage")
    r = sr.read_case(c)
    assert np.all(h["reason"][1, :6] == sr.NO_MATCH) and np.all(h["reason"][2] == sr.NO_MATCH) and h["ncreated"][2] == 0
    res.check_against_reading(c, r, h, "header", xh=h["xh"])
