"""Hand-worked answers for the second reading of the covisibility votes and the local map points (tests/second_reading_covis.py) on the
constructed maps of tests/covis_cases.py, and the sequential reading against the numpy call contracts through the flatten, on every case
and on 300 seeded maps.  No GPU."""
import copy

import numpy as np
import pytest

import covis_cases as cc
import second_reading_covis as sr


def _votes_of(kfs, who):
    """The sequential reading and the contract through the flatten, for one query."""
    if isinstance(who, sr.Frame):
        twin = copy.copy(who); twin.mvpMapPoints = list(who.mvpMapPoints)
        F = sr.flatten_votes([who.mvpMapPoints], None, None)
        seq = sr.LocalKeyFrameVotes(twin)
        skip_bad = 0
    else:
        kf = kfs[who]
        F = sr.flatten_votes([kf.GetMapPointMatches()], [kf], kf.map)
        seq = sr.ConnectionCounts(kf)
        skip_bad = 1
    con = sr.votes_contract(*sr.vote_args(F, skip_bad, 15, 4))
    return seq, con, F


@pytest.mark.parametrize("name", sorted(cc.VOTE_CASES))
def test_vote_cases_by_hand(name):
    kfs, who, want = cc.VOTE_CASES[name]()
    seq, con, F = _votes_of(kfs, who)
    assert {kfs.index(kf): n for kf, n in seq.items()} == want
    assert sr.counter_of(F, con["votes"][0]) == seq
    assert con["n_voted"][0] == len(want) and con["max_votes"][0] == max([0] + list(want.values()))
    assert con["n_over"][0] == sum(v >= 15 for v in want.values())


def test_skip_bad_zero_and_one():
    """The same KeyFrame query with skip_bad 0 counts the bad KeyFrame, with 1 it does not (obs_flags bit 1)."""
    kfs, _, _ = cc.bad_keyframe()
    F = sr.flatten_votes([kfs[0].GetMapPointMatches()], [kfs[0]], kfs[0].map)
    on = sr.votes_contract(*sr.vote_args(F, 1))["votes"][0]
    off = sr.votes_contract(*sr.vote_args(F, 0))["votes"][0]
    r1, r2 = F["rows"].index(kfs[1]), F["rows"].index(kfs[2])
    assert (on[r1], on[r2], off[r1], off[r2]) == (3, 0, 3, 2) and on[0] == off[0] == 0


def test_pair_and_lone_right_entries_in_the_flatten():
    kfs, _, _ = cc.left_right_pair()
    F = sr.flatten_votes([kfs[0].GetMapPointMatches()], [kfs[0]], kfs[0].map)
    assert F["obs_flags"].tolist() == [0, 0, 1, 0, 0] and F["obs_row"].tolist() == [0, 1, 1, 0, 1] and F["obs_slot"].tolist() == [0, 1, 5, 1, 2]
    kfs, _, _ = cc.lone_right()
    F = sr.flatten_votes([kfs[0].GetMapPointMatches()], [kfs[0]], kfs[0].map)
    assert F["obs_flags"].tolist() == [0, 1] and sr.votes_contract(*sr.vote_args(F, 1))["votes"][0].tolist() == [0, 1]


def test_pair_rule_needs_a_live_left_entry():
    """A right entry whose left neighbour is skipped (slot out of range) or belongs to another row votes itself: defined by the call."""
    base = dict(q_mp=np.array([[0]], np.int32), q_n=[1], self_row=None, counts_kf=np.array([4, 4], np.int32), cap=4, kf_skip=None)
    obs = lambda row, slot, fl: [np.array([0, len(row)], np.int32), np.array(row, np.int32), np.array(slot, np.int32), np.array(fl, np.uint8), None]
    v = lambda row, slot, fl: sr.votes_contract(*[base[k] for k in sr.VOTE_ORDER], 0, *obs(row, slot, fl))["votes"][0].tolist()
    assert v([1, 1], [0, 2], [0, 1]) == [0, 1]                              # a pair
    assert v([1, 1], [9, 2], [0, 1]) == [0, 1]                              # the left entry is skipped: the right one votes
    assert v([0, 1], [0, 2], [0, 1]) == [1, 1]                              # another row before it
    assert v([1, 1], [0, 2], [1, 1]) == [0, 2]                              # two right entries: per entry
    assert v([1, 1, 1], [0, 1, 2], [0, 1, 1]) == [0, 2]                     # left, right, right: the second right entry votes


def test_frame_reading_clears_bad_points():
    kfs, frame, _ = cc.bad_point_frame()
    assert sum(mp is not None for mp in frame.mvpMapPoints) == 2
    sr.LocalKeyFrameVotes(frame)
    assert sum(mp is not None for mp in frame.mvpMapPoints) == 1


def test_tie_rules_stay_with_the_caller():
    kfs, who, _ = cc.tie_in_pointer_order()
    nmax, kfmax, pairs = sr.connection_summary(sr.ConnectionCounts(kfs[who]), th=2)
    assert nmax == 2 and kfmax is kfs[2] and [kf for _, kf in pairs] == [kfs[2], kfs[1]]


def test_list_is_in_ascending_row_order_and_cut_at_list_cap():
    kfs, who, want = cc.fourteen_fifteen()
    F = sr.flatten_votes([kfs[0].GetMapPointMatches()], [kfs[0]], kfs[0].map)
    con = sr.votes_contract(*sr.vote_args(F, 1, 15, 3), list_fill=-7)
    assert con["list_row"][0].tolist() == [1, 2, -7] and con["list_votes"][0].tolist() == [14, 15, -7]
    con = sr.votes_contract(*sr.vote_args(F, 1, 15, 1), list_fill=-7)
    assert con["list_row"][0].tolist() == [1] and con["n_voted"][0] == 2 and con["n_over"][0] == 1


@pytest.mark.parametrize("name", sorted(cc.LOCAL_CASES))
def test_local_point_cases_by_hand(name):
    local, want = cc.LOCAL_CASES[name]()
    F = sr.flatten_local([local])
    seq = sr.LocalMapPoints(local, 77)
    assert [mp.addr for mp in seq] == want
    out, nt, nq = sr.local_points_contract(*[F[k] for k in sr.LOCAL_ORDER])
    assert nt[0] == nq[0] == len(want) and [F["mps"][j].addr for j in out[0, :nq[0]]] == want


def test_q_stride_overflow_drops_the_tail():
    local, want = cc.dedupe()
    F = sr.flatten_local([local])
    out, nt, nq = sr.local_points_contract(*[F[k] for k in sr.LOCAL_ORDER], q_stride=2, fill=-9)
    assert nt[0] == 3 and nq[0] == 2 and [F["mps"][j].addr for j in out[0]] == want[:2]
    out, nt, nq = sr.local_points_contract(*[F[k] for k in sr.LOCAL_ORDER], q_stride=5, fill=-9)
    assert out[0, 3:].tolist() == [-9, -9]


def test_out_of_range_rows_and_indices_contribute_nothing():
    kf_mp = np.array([[0, 5, -1, 1], [1, 2, 0, 3]], np.int32)
    out, nt, _ = sr.local_points_contract(np.array([[1, 7, -1, 0]], np.int32), [4], np.array([3, 9], np.int32), kf_mp, 3, np.array([1, 1, 0], np.uint8))
    assert nt[0] == 2 and out[0, :2].tolist() == [1, 0]                      # row 1: 1, (2 invalid), 0, (3 NULL); rows 7, -1 skipped; row 0: 0 seen, 5 NULL


def test_sequential_reading_equals_the_contract_on_300_seeded_maps():
    voted = over = emitted = 0
    for seed in range(300):
        kfs, frame, local = cc.random_map(seed)
        queries = [kf for kf in kfs if not kf.isBad()]
        if queries:
            F = sr.flatten_votes([kf.GetMapPointMatches() for kf in queries], queries, queries[0].map)
            for q, kf in enumerate(queries):                                # one call per map: kf_skip is one row per call
                Fq = dict(F, kf_skip=np.array([0 if r.map is kf.map else 1 for r in F["rows"]], np.uint8))
                con = sr.votes_contract(*sr.vote_args(Fq, 1, 3, len(F["rows"])))
                seq = sr.ConnectionCounts(kf)
                assert sr.counter_of(F, con["votes"][q]) == seq, (seed, q)
                nmax, _, pairs = sr.connection_summary(seq, 3)
                assert (con["n_voted"][q], con["max_votes"][q], con["n_over"][q]) == (len(seq), nmax, len(pairs))
                n = con["n_voted"][q]
                assert con["list_row"][q, :n].tolist() == sorted(F["rows"].index(k) for k in seq)
                voted += len(seq); over += len(pairs)
        Ff = sr.flatten_votes([frame.mvpMapPoints], None, None)
        seq = sr.LocalKeyFrameVotes(frame)
        assert sr.counter_of(Ff, sr.votes_contract(*sr.vote_args(Ff, 0))["votes"][0]) == seq, seed
        assert all(mp is None or not mp.isBad() for mp in frame.mvpMapPoints)
        Fl = sr.flatten_local([local, local[::-1]])
        out, nt, nq = sr.local_points_contract(*[Fl[k] for k in sr.LOCAL_ORDER])
        for f, lst in enumerate((local, local[::-1])):
            want = sr.LocalMapPoints(lst, 9000 + 2 * seed + f)
            assert [Fl["mps"][j] for j in out[f, :nq[f]]] == want and nt[f] == len(want), (seed, f)
            emitted += len(want)
    assert voted > 1000 and over > 200 and emitted > 3000
