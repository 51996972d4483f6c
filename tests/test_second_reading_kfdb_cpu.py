"""Hand-worked answers for tests/second_reading_kfdb.py (the 0.8 rule, the strict >, the list order, the stale-score neighbour, the 0.75f
cut, the duplicate set, the selection loop of DetectNBestCandidates), and proof through its branch counters that tests/kfdb_cases.py
reaches every situation it names.  No GPU and no product code."""
from collections import Counter

import numpy as np
import pytest

import kfdb_cases as kc
import second_reading_kfdb as srk

F = np.float32
# (int)(m * 0.8f) by hand: 0.8f = 0.800000011920929.  4 -> 3.2, 6 -> 4.8, 99 -> 79.2, 101 -> 80.8 truncate; 5, 10, 15, 100 give
# 4.00000006, 8.0000001, 12.0000002, 80.0000012, which round to the whole float below them (the spacing there is 4.8e-7 .. 7.6e-6)
MIN_COMMON = {1: 0, 4: 3, 5: 4, 6: 4, 10: 8, 15: 12, 99: 79, 100: 80, 101: 80}


@pytest.mark.parametrize("m", kc.MAX_COMMONS)
def test_point_eight_rule_and_strict_greater(m):
    c = kc.case("max_common_%d" % m)
    for place in (False, True):
        e = kc.expected(c, place)
        assert e["max_common"] == m and e["min_common"] == MIN_COMMON[m]
        mn = MIN_COMMON[m]
        assert e["common"][1] == m and e["scored"][1] == 1
        assert e["common"][2] == mn and e["scored"][2] == 0                  # exactly min_common: `>` is strict
        assert e["first_word"][2] == (-1 if mn == 0 else 12) and e["score"][2] == 0
        if mn + 1 <= m:
            assert e["common"][3] == mn + 1 and e["scored"][3] == 1 and e["score"][3] > 0
        assert e["nscored"] == int(e["scored"].sum()) and e["nsharing"] == int((e["common"] > 0).sum())


def test_list_order_is_first_word_then_row():
    e = kc.expected(kc.case("same_first_word"), False)
    assert e["order"] == [2, 1, 3, 0]
    assert list(e["first_word"]) == [49, 44, 41, 44]
    for name in kc.CASE_NAMES:                                               # the derivation include/orbm.h states, on every case
        for place in (False, True):
            e = kc.expected(kc.case(name), place)
            sharing = [r for r in range(len(e["common"])) if e["common"][r] > 0]
            assert e["order"] == sorted(sharing, key=lambda r: (e["first_word"][r], r)), name


def test_masked_rows_do_not_hold_the_maximum():
    c = kc.case("masked_maximum")
    reloc, place = kc.expected(c, False), kc.expected(c, True)
    assert reloc["max_common"] == 45 and reloc["common"][0] == 0 and reloc["first_word"][0] == -1      # the erased row shared 50
    assert place["max_common"] == 10 and place["common"][1] == 0 and place["min_common"] == 8
    assert list(place["scored"]) == [0, 0, 1, 1, 0, 0] and place["branches"]["excluded_connected"] == 45


def test_row_lengths_and_counts_are_laid():
    c = kc.case("row_lengths")
    assert sorted({len(ids) for ids, _ in c.rows}) == list(kc.ROW_LENGTHS)
    e = kc.expected(c, False)
    last = kc.PRIVATE - 1
    assert [int(w) for w in e["first_word"][6:11]] == [last] * 5             # rows that share the query's last word only
    for r in range(11, 16):                                                  # the shared word is the row's last entry
        assert e["common"][r] == 1 and c.rows[r][0][-1] == e["first_word"][r] == 1007
    assert e["common"][0] == 0 and len(c.rows[0][0]) == 0
    assert [len(kc.case("rows_%d" % n).rows) for n in kc.ROW_COUNTS] == list(kc.ROW_COUNTS)
    assert kc.expected(kc.case("no_sharing"), False)["nsharing"] == 0


def test_l1_of_a_vector_with_itself():
    """s = sum of -2 v_i, every term exact, so the score is the in-order sum of the values: (float)1.0 wherever they sum to exactly 1."""
    ids = [3, 9, 10, 400]
    assert srk.l1_score(ids, [0.5, 0.25, 0.125, 0.125], ids, [0.5, 0.25, 0.125, 0.125]) == 1.0
    n_exact = 0
    for name in kc.CASE_NAMES:
        c = kc.case(name)
        for ids, vals in c.rows + [c.query]:
            if len(ids) == 0:
                continue
            run = 0.0
            for v in vals:
                run += float(v)
            s = srk.l1_score(list(ids), list(vals), list(ids), list(vals))
            assert s == run
            if run == 1.0:
                n_exact += 1
                assert F(s) == F(1.0)
    assert n_exact > 100
    e = kc.expected(kc.case("identical_row"), False)
    assert e["scored"][1] == 1 and abs(float(e["score"][1]) - 1.0) < 1e-6


def test_l1_walks_with_lower_bound():
    t = Counter()
    s = srk.l1_score([1, 2, 3, 50], [0.25] * 4, [3, 4, 5, 50, 60], [0.5, 0.125, 0.125, 0.125, 0.125], t)
    # word 3: |.25 - .5| - .25 - .5 = -.5; word 50: |.25 - .125| - .25 - .125 = -.25; -(-.75) / 2
    assert s == 0.375 and t["l1_equal"] == 2 and t["l1_advance_v1"] == 1 and t["l1_advance_v2"] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# a database worked by hand: the query holds words 1..4 at 0.25 each
#   A = the query                     common 4, score 1.0
#   B = words 1, 2, 3, 9              common 3 = min_common (4 * 0.8f = 3.2): listed, NOT scored, keeps its stale score 0.5
#   C = (.5, .25, .125, .125)         common 4, s = -.5 - .5 - .25 - .25, score .75
#   D = (.125, .125, .25, .5)         common 4, score .75
#   E = words 7, 8                    shares nothing
#   G = the query, in the other map   common 4, score 1.0
# covisibility: A: [B, E]   C: [A]   D: []   G: [B]
#   groups: A 1.0 + 0.5 (B's stale score) = 1.5, best A;  C .75 + 1.0 = 1.75, best A;  D .75, best D;  G 1.0 + 0.5 = 1.5, best G
#   bestAccScore 1.75, 0.75f * 1.75 = 1.3125:  A passes -> A;  C passes -> A again (duplicate);  D is cut;  G passes, other map
# ---------------------------------------------------------------------------------------------------------------------------
def _hand(place, other_map_bad=False, a_bad=False):
    maps = [srk.Map(), srk.Map(other_map_bad)]
    q4 = [0.25] * 4
    A = srk.KeyFrame([1, 2, 3, 4], q4, maps[0], a_bad)
    B = srk.KeyFrame([1, 2, 3, 9], q4, maps[0])
    C = srk.KeyFrame([1, 2, 3, 4], [0.5, 0.25, 0.125, 0.125], maps[0])
    D = srk.KeyFrame([1, 2, 3, 4], [0.125, 0.125, 0.25, 0.5], maps[0])
    E = srk.KeyFrame([7, 8], [0.5, 0.5], maps[0])
    G = srk.KeyFrame([1, 2, 3, 4], q4, maps[1])
    A.covisible, C.covisible, G.covisible = [B, E], [A], [B]
    B.mRelocScore = B.mPlaceRecognitionScore = F(0.5)
    db = srk.KeyFrameDatabase(16)
    for kf in (A, B, C, D, E, G):
        db.add(kf)
    query = srk.KeyFrame([1, 2, 3, 4], q4, maps[0]) if place else srk.Frame([1, 2, 3, 4], q4, 41)
    return db, (A, B, C, D, E, G), query, maps


def test_relocalization_by_hand():
    db, (A, B, C, D, E, G), frame, maps = _hand(False)
    out = db.detect_relocalization_candidates(frame, maps[0])
    assert out == [A]
    assert db.last["sharing"] == [A, B, C, D, G] and db.last["max_common"] == 4 and db.last["min_common"] == 3
    assert [(float(s), k) for s, k in db.last["scores"]] == [(1.0, A), (0.75, C), (0.75, D), (1.0, G)]
    assert B.mnRelocQuery == 41 and B.mnRelocWords == 3 and B.mRelocScore == F(0.5)       # listed, its score is not written
    assert E.mnRelocQuery == -1
    t = db.t
    assert t["neighbour_stale_score"] == 2 and t["neighbour_not_sharing"] == 1 and t["neighbour_is_best"] == 1
    assert t["duplicate"] == 1 and t["cut_by_075"] == 1 and t["other_map"] == 1 and t["at_or_below_min_common"] == 1


def test_n_best_by_hand():
    # sorted groups (stable): C 1.75 -> A, A 1.5 -> A, G 1.5 -> G, D .75 -> D
    db, (A, B, C, D, E, G), kf, maps = _hand(True)
    assert db.detect_n_best_candidates(kf, 2) == ([A, D], [G])
    assert db.t["duplicate"] == 1
    db, (A, B, C, D, E, G), kf, maps = _hand(True)
    assert db.detect_n_best_candidates(kf, 1) == ([A], [G])                  # the loop ends once both hold one
    db, (A, B, C, D, E, G), kf, maps = _hand(True, other_map_bad=True)
    assert db.detect_n_best_candidates(kf, 2) == ([A, D], []) and db.t["not_taken"] == 1
    db, (A, B, C, D, E, G), kf, maps = _hand(True)
    kf.connected = {A}                                                       # A is connected: it leaves the list, C's neighbour no longer counts
    assert db.detect_n_best_candidates(kf, 2) == ([C, D], [G])
    assert A.mnPlaceRecognitionQuery == -1 and A.mnPlaceRecognitionWords == 1 and db.t["excluded_connected"] == 4
    db, (A, B, C, D, E, G), kf, maps = _hand(True, a_bad=True)
    with pytest.raises(srk.BadKeyFrameSpin):
        db.detect_n_best_candidates(kf, 2)


def test_stable_sort_keeps_equal_scores_in_list_order():
    pairs = [(F(0.5), "a"), (F(0.75), "b"), (F(0.5), "c"), (F(0.75), "d"), (F(0.25), "e")]
    assert [k for _, k in srk.stable_sort_comp_first(pairs)] == ["b", "d", "a", "c", "e"]


def test_erase_and_clear_map():
    db, (A, B, C, D, E, G), frame, maps = _hand(False)
    db.erase(A)
    db.clear_map(maps[1])
    db.detect_relocalization_candidates(frame, maps[0])
    assert db.last["sharing"] == [B, C, D] and db.last["min_common"] == 3 and [k for _, k in db.last["scores"]] == [C, D]


def test_every_situation_of_the_cases_is_reached():
    t = Counter()
    for c in [kc.case(n) for n in kc.CASE_NAMES] + [kc.random_case(s) for s in range(40)]:
        for place in (False, True):
            db, rows, query, maps = kc.build(c, place)
            if place:
                db.detect_n_best_candidates(query, c.n_candidates)
            else:
                db.detect_relocalization_candidates(query, maps[c.query_map])
            t.update(db.t)
    for m in kc.MAX_COMMONS:
        assert t[("max_common", m)] >= 2, m
    for key in ("no_sharing", "scored", "at_or_below_min_common", "below_min_common", "excluded_connected", "neighbour_stale_score",
                "neighbour_not_sharing", "neighbour_is_best", "cut_by_075", "other_map", "duplicate", "not_taken", "l1_equal", "l1_advance_v1",
                "l1_advance_v2"):
        assert t[key] > 0, key
