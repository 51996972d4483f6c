"""The second reading's results on every case of tests/poseopt_cases.py, computed once per process and shared by the tests (read-only)."""
import functools

import numpy as np

import poseopt_cases as pc
import poseopt_io as io
import second_reading_poseopt as sr

ORDERS = ("asc", "desc", "tree")
FAMILY = {"seeded": pc.SEEDED, "constructed": tuple(n for n in ("readmit", "empty_round1", "behind_camera", "stereo_invz", "noise_free",
                                                                   "rejected_last_trial", "restart_matters", "start_at_optimum"))}


@functools.lru_cache(maxsize=None)
def cases():
    return pc.build_cases()


@functools.lru_cache(maxsize=None)
def reading(name, order="asc"):
    r = sr.pose_optimization(*pc.reading_args(cases()[name]), sum_order=order)
    for a in (r["pose"], r["pose_f32"], r["outlier"]):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def spread(name):
    """s of one case: the largest spread of a final pose entry between the three summation orders."""
    return max(io.pose_spread(reading(name, o)["pose"], reading(name, "asc")["pose"]) for o in ORDERS)


@functools.lru_cache(maxsize=None)
def family_spread():
    """s per case family, measured on the DECISIVE cases as the tolerance rule says (the figures profiles/NOTES.md records); "all" is the
    s of the tolerance.  "floor" is recorded for information only: the spread on the cases where LM reaches the rounding floor."""
    s = {fam: max([spread(n) for n in names if n in pc.DECISIVE] or [0.0]) for fam, names in FAMILY.items()}
    s["all"] = max(s.values())
    s["floor"] = max(spread(n) for n in pc.FLOOR + pc.KNIFE_EDGE)
    return s


def check_against_reading(name, got_pose64, got_tcw32, got_outlier, got_n_corr, got_n_good, what):
    """The header test's rule.  On EVERY case flags, n_corr and n_good equal the reading exactly and the pose lies within one float32
    ulp plus 4 s of it after the final rounding.  Before the final rounding (got_pose64, where the implementation exposes it): a decisive
    case lies within 4 s of the ascending-order reading, s being measured on the decisive cases; a named knife-edge or rounding-floor
    case, where rho's sign in the last trials is noise and the reading's own summation orders part ways, lies within 4 max(s, that
    case's own spread between the three orders) -- the same factor on the reading's own error for that scene."""
    r = reading(name)
    s = family_spread()["all"]
    assert np.array_equal(np.asarray(got_outlier, np.int8), r["outlier"]), "%s: %s: flags differ from the reading" % (what, name)
    assert got_n_corr == r["n_corr"], (what, name, got_n_corr, r["n_corr"])
    assert got_n_good == r["n_good"], (what, name, got_n_good, r["n_good"])
    ref32 = r["pose_f32"].astype(np.float64)
    scale = np.ones((3, 4)); scale[:, 3] = np.maximum(1.0, np.abs(r["pose"][:, 3]))
    ulp = np.spacing(np.abs(r["pose_f32"])).astype(np.float64)
    d32 = np.abs(np.asarray(got_tcw32, np.float64).reshape(3, 4) - ref32)
    assert np.all(d32 <= ulp + 4 * s * scale), "%s: %s: pose after rounding off by %g" % (what, name, float(d32.max()))
    if got_pose64 is not None:
        bound = 4 * s if name in pc.DECISIVE else 4 * max(s, spread(name))
        d = io.pose_spread(got_pose64, r["pose"])
        assert d <= bound, "%s: %s: pose off by %g before the final rounding, bound %g" % (what, name, d, bound)
