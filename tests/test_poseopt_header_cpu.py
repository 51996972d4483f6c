"""orb-slam3_amd/csrc/orbm_poseopt.h -- the arithmetic k_pose_opt executes -- built with g++ as the stand-alone program
tests/poseopt_header.cpp (-ffp-contract=off) and run on every case of tests/poseopt_cases.py against the second reading: on a decisive
case flags, n_corr and n_good equal the reading exactly and the pose lies within 4 s of it before the final rounding (one float32 ulp
plus 4 s after it); on a named knife-edge or rounding-floor case flags and counts are equal too and the pose lies within 4 max(s, the
case's own spread between the reading's summation orders).  `poseopt_header selftest` pins the strict > of the classification and
the stale-error rule on hand-built inputs.  s is measured by the test, on the CPU, between
the reading's three summation orders (tests/poseopt_results.py).  The program is also built with -fsanitize=address,undefined and run
directly on the same cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseopt_io as io            # noqa: E402
import poseopt_results as res      # noqa: E402


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("poseopt_header")
    path = str(d / "cases.txt")
    io.write_cases(path, res.cases())
    return d, path


@pytest.fixture(scope="module")
def header_results(built):
    d, path = built
    return io.run_program(io.build_program(d), path)


@pytest.mark.parametrize("name", sorted(res.cases()))
def test_header_against_the_reading(header_results, name):
    h = header_results[name]
    print("%s: pose off by %.3g before rounding, s = %.3g" % (name, io.pose_spread(h["pose"], res.reading(name)["pose"]), res.family_spread()["all"]))
    assert np.array_equal(h["tcw"], h["pose"].astype(np.float32))
    res.check_against_reading(name, h["pose"], h["tcw"], h["outlier"], h["n_corr"], h["n_good"], "header")


def test_sanitized_build_agrees(built, header_results):
    d, path = built
    san = io.run_program(io.build_program(d, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")), path)
    assert sorted(san) == sorted(header_results)
    for name, h in header_results.items():
        assert san[name]["pose"].tobytes() == h["pose"].tobytes() and np.array_equal(san[name]["outlier"], h["outlier"]), name
        assert (san[name]["n_corr"], san[name]["n_good"]) == (h["n_corr"], h["n_good"])


def test_octave_outside_the_levels_is_null(built):
    """A slot whose octave is outside [0, nlevels) holds no edge: it is not counted and its flag is not written."""
    d, _ = built
    c = dict(res.cases()["ncorr_10"])
    c["kps"] = c["kps"].copy()
    s = np.nonzero(c["q_mp"] >= 0)[0]
    c["kps"]["octave"][s[0]] = len(c["ils2"]); c["kps"]["octave"][s[1]] = -1
    path = str(d / "octave.txt")
    io.write_cases(path, {"octave": c})
    h = io.run_program(io.build_program(d), path)["octave"]
    assert h["n_corr"] == 8 and h["outlier"][s[0]] == -1 and h["outlier"][s[1]] == -1 and np.all(h["outlier"][s[2:]] >= 0)


RULE_CHECKS = [tag + "_" + c for tag in ("mono", "stereo") for c in ("chi2_is_w", "on_threshold_is_inlier", "one_float_ulp_above_is_outlier",
                                                                     "double_above_rounds_down_to_inlier", "one_float_ulp_below_is_inlier")] + [
    "chi2_here_4_there_16", "inlier_is_read_at_Terr_above", "inlier_is_read_at_Terr_below", "outlier_is_recomputed_at_T_below",
    "outlier_is_recomputed_at_T_above", "ten_rejected_trials_end_the_round", "estimate_is_restored", "errors_stay_at_the_rejected_pose",
    "the_rejected_pose_is_the_damped_step", "a_failed_solve_applies_the_previous_x", "a_failed_solve_is_never_accepted"]


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_rules_on_hand_built_inputs(built, san):
    """The shipped po_edge_classify and po_optimize10 on inputs whose answers are known by hand: an edge whose chi2 is exactly the float
    threshold stays in, one float ulp above it goes out, a double just above that rounds down to it stays in (mono 5.991f, stereo
    7.815f); an inlier is classified with the error at the pose of the last trial and an outlier at the estimate, with the threshold
    between the two chi2; after ten rejected trials the estimate is restored and the errors' pose is the rejected one."""
    d, _ = built
    extra = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g") if san else ()
    rc, checks = io.run_selftest(io.build_program(d, extra=extra))
    assert sorted(checks) == sorted(RULE_CHECKS)
    assert rc == 0 and all(checks.values()), [k for k, v in checks.items() if not v]
