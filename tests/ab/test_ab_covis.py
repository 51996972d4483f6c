"""The plain form of the covisibility vote (k_covis_votes<false>: one global atomicAdd per vote, -DORBX_AB build only, switch
ORBM_COVIS_PLAIN): the same votes, counts and lists as the second reading's contract and as the shipped form that aggregates per workgroup
in LDS, on the array-level data of tests/test_gpu_covis.py (lists of every length, aliasing rows, garbage indices) and on the constructed
maps."""
import pytest

pytestmark = pytest.mark.gpu
import covis_cases as cc
import second_reading_covis as sr
from test_gpu_covis import _three_ways, m, synthetic_votes   # noqa: F401  (m: the matcher fixture)


@pytest.mark.parametrize("garbage", [False, True], ids=["clean", "garbage"])
@pytest.mark.parametrize("nq,cap", [(1, 16), (9, 40)])
def test_plain_atomics_equal_the_second_reading(pkg, m, monkeypatch, nq, cap, garbage):
    args = synthetic_votes(10 * nq + cap, nq, cap, garbage)
    shipped = _three_ways(pkg, m, args)
    monkeypatch.setenv("ORBM_COVIS_PLAIN", "1")
    plain = _three_ways(pkg, m, args)                                       # host form == device form == contract under the switch
    assert all((shipped[k] == plain[k]).all() for k in ("votes", "n_voted", "max_votes", "n_over"))


def test_plain_atomics_on_the_constructed_maps(pkg, m, monkeypatch):
    monkeypatch.setenv("ORBM_COVIS_PLAIN", "1")
    for name in sorted(cc.VOTE_CASES):
        kfs, who, _ = cc.VOTE_CASES[name]()
        if isinstance(who, sr.Frame):
            F = sr.flatten_votes([who.mvpMapPoints], None, None); seq = sr.LocalKeyFrameVotes(who); skip_bad = 0
        else:
            F = sr.flatten_votes([kfs[who].GetMapPointMatches()], [kfs[who]], kfs[who].map); seq = sr.ConnectionCounts(kfs[who]); skip_bad = 1
        assert sr.counter_of(F, _three_ways(pkg, m, sr.vote_args(F, skip_bad, 15, 3))["votes"][0]) == seq, name


def test_the_switch_is_in_this_library_only(pkg):
    import os
    ab = open(pkg.LIB_PATH, "rb").read()
    prod = open(os.path.join(os.path.dirname(pkg.LIB_PATH), "liborbslam3_amd.so"), "rb").read()
    assert b"ORBM_COVIS_PLAIN" in ab and b"ORBM_COVIS_PLAIN" not in prod
