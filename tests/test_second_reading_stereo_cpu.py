"""The CPU oracle's ComputeStereoMatches (oracle/orbref_frame.cpp) against the second reading of Frame.cc:1027-1276
(tests/second_reading_stereo.py): entry for entry -- the count and the bytes of mvuRight and mvDepth -- on two rendered pairs, on the
self pair and on the constructed pairs of tests/stereo_cases.py, each of which proves from the second reading's branch counters that it
reached the branch it was built for.  Over the module every branch the reading names is reached, except the deltaR gate (:1231), which is
dead: the strict minimum gives dist1 > dist2 <= dist3, hence |deltaR| <= 0.5.  No GPU."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import second_reading_stereo as srs
import stereo_cases as sc
import structured_images as si

HERE = os.path.dirname(os.path.abspath(__file__))
NF = 500
SEEN = Counter()                                  # branch counts of every comparison this module ran


def rendered_pairs(synth, oracle):
    """name -> (left image, right image, kl, dl, kr, dr, mb, mbf) with the oracle extractor's rows: a synthetic pair, a lattice pair whose
    rows tie all along the band, and the synthetic left image against itself (every SAD 0: the median is 0 and the cut takes them all)."""
    l, r = synth.gen_stereo_pair(sc.W, sc.H, 321)
    dl_, dr_ = si.shifted_pair("dots", sc.W, sc.H, 51, 12, pitch=8)
    out = {}
    for name, a, b in (("synth", l, r), ("dots", dl_, dr_), ("self", l, l)):
        ex = oracle.Extractor(NF)
        _, ka, da, _ = ex(a, (0, 0)); _, kb, db, _ = ex(b, (0, 0))
        out[name] = (a, b, ka, da, kb, db, si.MB, si.MBF)
    return out


def oracle_and_reading(oracle, OM, img_l, img_r, kl, dl, kr, dr, mb, mbf):
    """Runs both on one pair, asserts that they agree and returns the reading's (kept, uright, depth, sad, branches)."""
    ol, orr = oracle.Extractor(NF), oracle.Extractor(NF)
    ol(img_l, (0, 0)); orr(img_r, (0, 0))                                    # the pyramids the oracle's SAD slide reads
    t = ol.tables()
    assert np.array_equal(t["sf"], sc.SF) and np.array_equal(t["inv_sf"], sc.ISF)
    lv_l = [ol.level_image(i) for i in range(sc.NLEVELS)]; lv_r = [orr.level_image(i) for i in range(sc.NLEVELS)]
    assert [a.shape for a in lv_l] == list(zip(sc.LEVEL_H, sc.LEVEL_W))
    assert np.array_equal(lv_l[0], img_l) and np.array_equal(lv_r[0], img_r)
    kept, ur, dp, sad, br = srs.compute_stereo_matches(kl, dl, kr, dr, lv_l, lv_r, t["sf"], t["inv_sf"], mb, mbf)
    n_o, ur_o, dp_o = OM.ComputeStereoMatches(ol, orr, kl, dl, kr, dr, mb, mbf)
    assert n_o == kept, (n_o, kept)
    assert ur_o.tobytes() == ur.tobytes(), np.nonzero(ur_o.view(np.uint32) != ur.view(np.uint32))[0][:10]
    assert dp_o.tobytes() == dp.tobytes(), np.nonzero(dp_o.view(np.uint32) != dp.view(np.uint32))[0][:10]
    assert kept == int((ur >= 0).sum()) == int((dp > 0).sum()) and np.all(sad[ur >= 0] >= 0)
    SEEN.update(br)
    return kept, ur, dp, sad, br


def check_expectations(case, kl, ur, dp, sad, br):
    for key, want in case.expect.items():
        if isinstance(want, tuple):
            assert br[key] == want[1], (case.name, key, br[key], want)
        else:
            assert br[key] >= want, (case.name, key, br[key], want)
    for il, v in case.valid.items():
        assert bool(ur[il] >= 0) == v, (case.name, il, float(ur[il]), int(sad[il]))
    for il, s in case.sad.items():
        assert sad[il] == s, (case.name, il, int(sad[il]), s)
    for il in case.clamped:                                                  # :1245-1246: a double difference and the double literal, narrowed
        assert ur[il] == np.float32(np.float64(kl[il]["x"]) - 0.01) and dp[il] == np.float32(case.mbf) / np.float32(0.01), (case.name, il)
    assert br["deltaR_gate"] == 0


def test_second_reading_imports_neither_oracle_nor_product():
    src = open(os.path.join(HERE, "second_reading_stereo.py")).read()
    mods = set(re.findall(r"^\s*(?:from|import)\s+([\w\.]+)", src, flags=re.M))
    assert mods == {"math", "collections", "numpy", "second_reading"}, mods
    for word in ("orbref", "orb-slam3_amd", "importlib", "ctypes", "__import__", "liborb"):
        assert word not in src, word
    helper = open(os.path.join(HERE, "stereo_cases.py")).read()
    assert set(re.findall(r"^\s*(?:from|import)\s+([\w\.]+)", helper, flags=re.M)) == {"numpy"}


@pytest.fixture(scope="module")
def OM(oracle):
    return oracle._oracle_matcher_class()()


@pytest.fixture(scope="module")
def rendered(synth, oracle):
    return rendered_pairs(synth, oracle)


CASES = sc.constructed_cases()


@pytest.mark.parametrize("name", ["synth", "dots", "self"])
def test_rendered_pair_oracle_equals_second_reading(oracle, OM, rendered, name):
    kept, ur, dp, sad, br = oracle_and_reading(oracle, OM, *rendered[name])
    print(name, kept, dict(br))
    assert br["deltaR_gate"] == 0
    if name == "synth":                                                      # not vacuous
        assert kept > 100 and br["cut"] > 0 and br["octave_band_reject"] > 0 and br["u_range_reject"] > 0 and br["bestDist_ge_thOrbDist"] > 0
    if name == "dots":
        assert br["distance_tie"] > 0 and br["bestincR_at_minus_L"] + br["bestincR_at_plus_L"] > 0
    if name == "self":                                                       # SAD 0 at shift 0 for every match: median 0, threshold 0, all cut
        assert kept == 0 and br["cut"] > 100 and np.all(sad[sad >= 0] == 0)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_constructed_case(oracle, OM, case):
    kl, dl, kr, dr = case.arrays()
    kept, ur, dp, sad, br = oracle_and_reading(oracle, OM, case.img_l, case.img_r, kl, dl, kr, dr, case.mb, case.mbf)
    print(case.name, kept, dict(br))
    check_expectations(case, kl, ur, dp, sad, br)


def test_every_branch_was_reached_and_the_deltaR_gate_never():
    """Runs after the comparisons above (file order): SEEN holds the reading's counters over the rendered pairs and every constructed case."""
    assert SEEN["kept"] > 0, "run the whole module"
    missing = [b for b in srs.BRANCHES if b != "deltaR_gate" and SEEN[b] == 0]
    assert not missing, missing
    assert SEEN["deltaR_gate"] == 0
    for edge in ("row_outside_image_dropped", "empty_vDistIdx", "iniu_zero", "endu_cols_minus_1", "deltaR_half", "uR_on_minU", "uR_on_maxU",
                 "row_on_minr", "row_on_maxr", "bestDist_on_thOrbDist_minus_1", "candidates_over_64", "slide_left_of_level"):
        assert SEEN[edge] > 0, edge


def test_width_of_the_two_float_lines_cannot_be_observed():
    """Two places where the product must follow the reference's types, and where no input can show it: the cut's threshold in float
    against double (:1263) and the clamp's subtraction in double against float (:1246).  Both lists are empty over every SAD below
    121 * 255 and every uL below 512; the constructed cases pin the values (cut_threshold_edge, disparity), not the widths."""
    assert sc.float_and_double_thresholds_differ() == []
    assert sc.clamp_in_float_differs() == []
    assert sc.survives(20, 10) and not sc.survives(21, 10)


def test_camera_width_is_no_multiple_of_the_device_pitch():
    """The device pyramids pad every row to a multiple of 64 bytes: at this width every level's width differs from its pitch, so a window
    bound taken against the pitch (sad_window) reads on where the reference stops."""
    assert all(w % 64 for w in sc.LEVEL_W)
