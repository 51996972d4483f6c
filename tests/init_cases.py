"""Inputs shared by the SearchForInitialization (M9) tests: the suite's 376 x 240 / 2 500-feature scene and a set of constructed frame
pairs, each built to reach one branch of ORBmatcher.cc:799-943.  A constructed pair places its keypoints on a lattice of sites 40 px
apart and searches with an 8-px window, so that a query sees only the slots put at its own site; descriptors are bit patterns whose
Hamming distances are chosen by hand.  No oracle, product or second-reading import: this file only makes arrays."""
import numpy as np

W, H, NF = 376, 240, 500
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
INV_W, INV_H = np.float32(64) / np.float32(W), np.float32(48) / np.float32(H)
CHAIN_WINDOW = 20                               # second step of the three-frame chain: smaller than the motion, so the carried positions decide
WINDOW = 8                                      # of the constructed pairs; the scene uses the reference's 100


def bits(*ranges):
    """A 32-byte descriptor with the bits of the given [lo, hi) ranges set."""
    b = np.zeros(256, np.uint8)
    for lo, hi in ranges:
        b[lo:hi] = 1
    return np.packbits(b, bitorder="little")


def site(i):
    """Centre of lattice site i (9 columns x 6 rows, 40 px apart)."""
    return 20.0 + 40.0 * (i % 9), 20.0 + 40.0 * (i // 9)


class Pair:
    """One constructed (F1, F2, vbPrevMatched) triple."""

    def __init__(self, name, nnratio=0.9, check_ori=True):
        self.name, self.nnratio, self.check_ori, self.window = name, nnratio, check_ori, WINDOW
        self._k1, self._d1, self._prev, self._k2, self._d2 = [], [], [], [], []

    def q(self, x, y, desc, angle=0.0, octave=0, prev=None):
        self._k1.append((x, y, 31.0, angle, 1.0, octave, -1)); self._d1.append(desc)
        self._prev.append((x, y) if prev is None else prev)
        return len(self._k1) - 1

    def s(self, x, y, desc, angle=0.0, octave=0):
        self._k2.append((x, y, 31.0, angle, 1.0, octave, -1)); self._d2.append(desc)
        return len(self._k2) - 1

    def arrays(self):
        return (np.array(self._k1, KP_DTYPE), np.array(self._d1, np.uint8).reshape(-1, 32), np.array(self._k2, KP_DTYPE),
                np.array(self._d2, np.uint8).reshape(-1, 32), np.array(self._prev, np.float32).reshape(-1, 2))


def _simple_match(p, i, angle, d=10):
    """A query and a slot at site i, `d` bits apart, rotation difference `angle` degrees."""
    x, y = site(i)
    return p.q(x, y, bits(), angle=angle), p.s(x + 1.0, y, bits((0, d)))


def constructed_pairs():
    """name -> (Pair, expect): expect maps a trace counter of the second reading to the least value that proves the branch was reached,
    plus "m12" -> {query: slot or -1} entries that must hold."""
    out = {}
    # a distance of exactly TH_LOW is accepted, TH_LOW + 1 is not
    p = Pair("th_low")
    x, y = site(0); a = p.q(x, y, bits()); sa = p.s(x, y, bits((0, 50)))
    x, y = site(1); b = p.q(x, y, bits()); p.s(x, y, bits((0, 51)))
    out[p.name] = (p, {"dist_on_th_low": 1, "dist_on_th_low_plus_1": 1, "m12": {a: sa, b: -1}})
    # the ratio on the float32 product: 50 * 0.9f rounds to 45.0f, so (45, 50) fails and (44, 50) passes
    p = Pair("ratio")
    x, y = site(0); a = p.q(x, y, bits()); p.s(x, y, bits((0, 45))); p.s(x + 2, y, bits((100, 150)))
    x, y = site(1); b = p.q(x, y, bits()); sb = p.s(x, y, bits((0, 44))); p.s(x + 2, y, bits((100, 150)))
    out[p.name] = (p, {"ratio_fail": 1, "ratio_pass": 1, "m12": {a: -1, b: sb}})
    # a tie is won by the first slot in grid order: slot 1 sits one grid column to the left of slot 0
    p = Pair("tie", nnratio=1.2)
    x, y = site(10); a = p.q(x, y, bits()); p.s(x + 6, y, bits((0, 30))); s1 = p.s(x - 6, y, bits((50, 80)))
    out[p.name] = (p, {"ratio_pass": 1, "m12": {a: s1}})
    # |dx| == window_size is outside (strict <), just inside is inside
    p = Pair("window_edge")
    x, y = site(0); a = p.q(x, y, bits()); p.s(x + WINDOW, y, bits((0, 10)))
    x, y = site(1); b = p.q(x, y, bits()); sb = p.s(x + WINDOW - 0.5, y, bits((0, 10)))
    x, y = site(2); c = p.q(x, y, bits()); p.s(x, y - WINDOW, bits((0, 10)))
    out[p.name] = (p, {"exactly_r_away": 2, "empty_window": 2, "m12": {a: -1, b: sb, c: -1}})
    # octave-1 keypoints on both sides are ignored
    p = Pair("octave_1")
    x, y = site(0); a = p.q(x, y, bits(), octave=1); p.s(x, y, bits((0, 5)))
    x, y = site(1); b = p.q(x, y, bits()); p.s(x, y, bits((0, 5)), octave=1); sb = p.s(x + 2, y, bits((0, 40)))
    x, y = site(2); c = p.q(x, y, bits()); p.s(x, y, bits((0, 5)), octave=1)
    out[p.name] = (p, {"level_skip": 1, "empty_window": 1, "m12": {a: -1, b: sb, c: -1}})
    # vbPrevMatched, not the keypoint's own position, centres the window
    p = Pair("prev_elsewhere")
    x, y = site(0); x2, y2 = site(30)
    a = p.q(x, y, bits(), prev=(x2, y2)); p.s(x, y, bits((0, 3))); sa = p.s(x2, y2, bits((0, 20)))
    out[p.name] = (p, {"ratio_pass": 1, "m12": {a: sa}})
    # an empty window
    p = Pair("empty_window")
    x, y = site(0); a = p.q(x, y, bits()); x, y = site(5); p.s(x, y, bits((0, 3)))
    out[p.name] = (p, {"empty_window": 1, "m12": {a: -1}})
    # the best slot is held by an earlier claim at a lower distance: it is skipped and the second-nearest slot is accepted
    p = Pair("skip_to_second")
    x, y = site(0)
    a = p.q(x, y, bits()); b = p.q(x + 1, y, bits((0, 10), (100, 112)))
    s0 = p.s(x, y, bits((0, 10))); s1 = p.s(x + 2, y, bits((0, 10), (100, 112), (200, 220)))
    out[p.name] = (p, {"skipped_by_matched_distance": 1, "query_outcome_changed_by_skip": 1, "m12": {a: s0, b: s1}})
    # ... and at an EQUAL distance too (<=)
    p = Pair("skip_on_equal")
    x, y = site(0)
    a = p.q(x, y, bits()); b = p.q(x + 1, y, bits((0, 10), (100, 110)))
    s0 = p.s(x, y, bits((0, 10)))
    out[p.name] = (p, {"skipped_by_matched_distance": 1, "all_candidates_skipped": 1, "m12": {a: s0, b: -1}})
    # a steal whose victim's bin is culled: the robbed entry is not counted down a second time
    p = Pair("steal_then_cull")
    n = 0
    for bin_, cnt in ((0, 4), (1, 4), (2, 3)):
        for _ in range(cnt):
            _simple_match(p, n, 12.0 * bin_); n += 1
    x, y = site(n)
    v = p.q(x, y, bits(), angle=60.0)                                        # bin 5, alone: culled
    t = p.q(x + 1, y, bits((0, 20), (100, 110)), angle=0.0)                  # bin 0, 10 bits from the slot: steals it from v (20 bits)
    sv = p.s(x, y, bits((0, 20)))
    out[p.name] = (p, {"steal": 1, "cull_robbed": 1, "nmatches": 12, "m12": {v: -1, t: sv}})
    # robbed entries decide the three maxima: bin 2 holds 3 claims of which 2 are robbed later, bin 3 holds 2 live ones
    p = Pair("robbed_in_maxima")
    n = 0
    for bin_, cnt in ((0, 8), (1, 10)):
        for _ in range(cnt):
            _simple_match(p, n, 12.0 * bin_); n += 1
    live2, s2 = _simple_match(p, n, 24.0); n += 1
    victims = []
    for _ in range(2):
        x, y = site(n); n += 1
        victims.append((p.q(x, y, bits(), angle=24.0), p.s(x, y, bits((0, 20))), x, y))
    live3 = [_simple_match(p, n + i, 36.0)[0] for i in range(2)]; n += 2
    thieves = [p.q(x + 1, y, bits((0, 20), (100, 110)), angle=0.0) for (_, _, x, y) in victims]
    m = {live2: s2, live3[0]: -1, live3[1]: -1}
    for (vq, vs, _, _), tq in zip(victims, thieves):
        m[vq] = -1; m[tq] = vs
    out[p.name] = (p, {"steal": 2, "cull_live": 2, "cull_robbed": 0, "nmatches": 21, "m12": m, "differs_from_finished_row_cull": True})
    return out


def scene_frames(synth, oracle):
    """The 376 x 240 pair of tests/test_oracle_searches_cpu.py's M9 case (seed 321, Extractor(5 x 500)) and a third view for the chain."""
    l, r = synth.gen_stereo_pair(W, H, 321)
    r2 = synth.gen_stereo_pair(W, H, 321, dmin=6, dmax=55)[1]
    ex = oracle.Extractor(5 * NF)
    frames = []
    for img in (l, r, r2):
        _, k, d, _ = ex(img, (0, 1000))
        frames.append((k, d))
    return frames


def make_pool(rows, cap, filler):
    """rows: list of (kps, desc); returns (kps [nrows][cap], desc [nrows][cap][32], counts).  Slots at or beyond a row's count hold
    `filler` = (keypoint record, descriptor): data that would match if it were read."""
    n = len(rows)
    kps = np.zeros((n, cap), KP_DTYPE); desc = np.zeros((n, cap, 32), np.uint8); counts = np.zeros(n, np.int32)
    kps[:] = filler[0]; desc[:] = filler[1]
    for i, (k, d) in enumerate(rows):
        counts[i] = len(k)
        kps[i, :len(k)] = k.view(KP_DTYPE) if k.dtype != KP_DTYPE else k
        desc[i, :len(k)] = d
    return kps, desc, counts
