"""The sequential rule of orbm_keyframe_culling (include/orbm.h): repeated contract calls with `erased` flags, on arrays flattened ONCE,
equal the sequential reading of the reference, which erases a KeyFrame the moment it is voted out (tests/second_reading_kfcull.py).  On
every constructed case and on 400 seeded random maps, mono and stereo weights.  No GPU, no library."""
import copy

import pytest

import kfcull_cases as kc
import second_reading_kfcull as sr

NMAPS = 400


def through_the_rule(covisible, monocular, th, call=sr.contract):
    """The rule on a copy of the map: flatten once, then calls with erased flags; the non-inertial branch (:1391) decides."""
    twin = copy.deepcopy(covisible)
    cands = sr.candidates(twin)
    if not cands:
        return []
    F = sr.flatten(cands, monocular)

    def decide(kf):
        kf.SetBadFlag()
        return kf.isBad()
    return sr.sequential_by_contract(F, cands, decide, call=call, redundant_th=th)


def sequential(covisible, monocular, th, abort=False):
    """The sequential reading, with what it met on the way: -> (records, number of real erases, number of votes against a KeyFrame that
    stayed, number of MapPoints that an erasure turned bad and that sat in the slots of a KeyFrame counted later)."""
    held_before = {kf.addr: [mp for mp in kf.mvpMapPoints if mp is not None] for kf in covisible}
    all_mps = {mp.addr: mp for mps in held_before.values() for mp in mps}
    bad = {a for a, mp in all_mps.items() if mp.isBad()}
    turned = set()                                                          # MapPoints that an erasure of this loop turned bad

    def on_redundant(kf):                                                   # the non-inertial branch, :1391
        kf.SetBadFlag()
        turned.update(a for a, mp in all_mps.items() if mp.isBad() and a not in bad)
        return True
    log = sr.KeyFrameCulling(covisible, monocular, th, abort_ba=lambda: abort, on_redundant=on_redundant)
    order = [r["kf"].addr for r in log]
    met = 0
    for a in turned:                                                        # it left with an erased KeyFrame and sat in a KeyFrame counted after that one
        gone_with = [i for i, r in enumerate(log) if r["erased"] and all_mps[a] in held_before[r["kf"].addr]]
        if gone_with and any(all_mps[a] in held_before[k] for k in order[gone_with[0] + 1:]):
            met += 1
    return log, sum(r["erased"] for r in log), sum(1 for r in log if r["cull"] and not r["erased"]), met


def same(log, rule):
    assert len(rule) >= len(log)                                            # the count rule ends the reference's loop; the rule's caller stops there
    for r, (n_mps, n_red, cull, state) in zip(log, rule):
        assert (r["n_mps"], r["n_redundant"], int(r["cull"])) == (n_mps, n_red, cull), r["kf"].addr
        assert list(state[:len(r["state"])]) == r["state"] and not state[len(r["state"]):].any()


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_rule_on_the_constructed_cases(name):
    c = kc.case(name)
    rule = through_the_rule(c.covisible, c.monocular, c.th)
    log = sequential(c.covisible, c.monocular, c.th, c.abort)[0]
    assert [(r["n_mps"], r["n_redundant"], int(r["cull"]), r["erased"]) for r in log] == c.seq
    same(log, rule)


def test_rule_on_random_maps():
    multi = held = bad_met = culls = mono = 0
    for seed in range(NMAPS):
        _, cov, monocular, th = kc.random_map(seed)
        rule = through_the_rule(cov, monocular, th)
        log, erases, stayed, met = sequential(cov, monocular, th)
        assert len(log) == len(rule)
        same(log, rule)
        multi += erases > 1; held += stayed > 0; bad_met += met > 0; culls += erases + stayed; mono += monocular
    # the generator is chosen so that the sequential reading alone meets these
    assert multi >= 50, multi
    assert held >= 20, held
    assert bad_met >= 20, bad_met
    assert 100 <= mono <= 300 and culls >= 400, (mono, culls)
