"""Hand-worked answers for the constructed KeyFrameCulling maps of tests/kfcull_cases.py: the sequential reading of the reference
(tests/second_reading_kfcull.py: KeyFrameCulling with the map surgery) and the numpy statement of the call contract both give what each
case's docstring works out.  No GPU, no library."""
import numpy as np
import pytest

import kfcull_cases as kc
import second_reading_kfcull as sr


def _contract(F, th, erased=None):
    return sr.contract(F["cand_row"], F["octave"], F["counts_kf"], F["kf_mp"], F["depth"], F["th_depth"], F["obs_off"], F["obs_row"], F["obs_slot"],
                       F["obs_flags"], F["mp_valid"], F["mp_nobs"], erased, 3, th)


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_hand_worked(name):
    c = kc.case(name)
    cands = sr.candidates(c.covisible)
    F = sr.flatten(cands, c.monocular)                                      # before the sequential reading changes the map
    if c.tweak:
        c.tweak(F)
    con = _contract(F, c.th)
    got = list(zip(con["n_mps"].tolist(), con["n_redundant"].tolist(), con["cull"].tolist()))
    log = sr.KeyFrameCulling(c.covisible, c.monocular, c.th, abort_ba=lambda: c.abort)
    assert [(r["n_mps"], r["n_redundant"], int(r["cull"]), r["erased"]) for r in log] == c.seq
    if c.con is not None:
        assert got == c.con
    else:                                                                   # one call is the reference up to and including the first cull
        upto = len(got) if con["first_cull"] < 0 else con["first_cull"] + 1
        upto = min(upto, len(c.seq))                                        # the count rule of :1395 may end the reference's loop before the list does
        assert got[:upto] == [s[:3] for s in c.seq][:upto]
    hit = [k for k, g in enumerate(got) if g[2]]
    assert con["first_cull"] == (hit[0] if hit else -1)
    for k, kf in enumerate(cands):                                          # slot_state agrees with the two counts and is 0 beyond the row
        row = con["slot_state"][k]
        assert (row != 0).sum() == got[k][0] and (row == 2).sum() == got[k][1]
        assert not row[min(int(F["counts_kf"][F["cand_row"][k]]), F["cap"]):].any()


def test_float32_bound():
    """:1349 in float: 0.9f * 10 rounds to 9.0f, so 9 of 10 is not culled; 0.9f * 11 is below 10."""
    assert np.float32(0.9) * np.float32(10) == np.float32(9.0)
    assert not sr.voted_out(9, 10, 0.9) and sr.voted_out(10, 11, 0.9) and not sr.voted_out(0, 0, 0.9)
    assert sr.voted_out(6, 11, 0.5) and not sr.voted_out(5, 10, 0.5)


def test_weights_and_the_two_rule():
    """AddObservation / EraseObservation: a stereo keypoint weighs 2, a two-camera KeyFrame's entries 1 each; at nObs <= 2 the MapPoint
    goes bad and leaves every observer."""
    b = kc.Builder()
    st = b.kf([0, 0], uRight=[3.0, -1.0]); two = b.kf([0, 0, 0, 0], NLeft=2, camera2=True, uRight=[3.0] * 4); mono = b.kf([0])
    mp = b.mp((st, 0), (two, 0), (two, 2), (mono, 0))
    assert mp.Observations() == 2 + 1 + 1 + 1 and mp.mObservations[two] == (0, 2)
    mp.EraseObservation(two)
    assert mp.Observations() == 3 and not mp.isBad()
    mp.EraseObservation(two)                                                # not an observer any more: nothing happens
    assert mp.Observations() == 3
    mp.EraseObservation(mono)
    assert mp.Observations() == 2 and mp.isBad() and st.mvpMapPoints[0] is None and not mp.mObservations
    assert two.mvpMapPoints[0] is mp                                        # EraseObservation alone does not touch the KeyFrame's slot


def test_keyframe_set_bad_flag():
    b = kc.Builder(init_id=1)
    first = b.kf([0]); held = b.kf([0], notErase=True); kf = b.kf([0]); other = b.kf([0, 0]); third = b.kf([0])
    mp = b.mp((first, 0), (held, 0), (kf, 0), (other, 0)); mp2 = b.mp((kf, 0), (other, 1), (third, 0))
    kf.mvpMapPoints[0] = mp                                                  # (the second link took the slot over; keep the first MapPoint there)
    first.SetBadFlag(); held.SetBadFlag()
    assert not first.isBad() and not held.isBad() and held.mbToBeErased and mp.Observations() == 4
    kf.SetBadFlag()
    assert kf.isBad() and mp.Observations() == 3 and kf not in mp.mObservations and not mp.isBad()
    assert mp2.Observations() == 3                                          # not in kf's slots: its entry stays (the invariant is the caller's)
