"""The HIP extractor held to the second reading of ORBextractor.cc's cell loop, quadtree and epilogue (tests/second_reading_extract.py)
directly -- the oracle is not consulted: per level the FAST candidates in vToDistributeKeys order (k_fast4 / k_fast_fix), the quadtree's
selection in its output order (k_quadtree2), and the final keypoints' six non-angle fields, their order and the mono count (k_slots),
on every hand-laid frame of tests/extract_cases.py, singly, batched, and with both workgroup widths of k_quadtree2.  The reading takes
the product's own un-blurred level images as data (the resize has its numpy statement in tests/test_oracle_params_cpu.py)."""
import numpy as np
import pytest

import extract_cases as ec
import second_reading_extract as sr

pytestmark = pytest.mark.gpu

CASES = ec.all_cases()
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(ec.key(_c), []).append(_c)
_READ = {}                                                   # case name -> (level images, the reading's result): computed once


def group_id(k):
    return "%dx%d-nf%d-nl%d-sf%s" % k[:5]


def make_extractor(pkg, k, max_batch=1):
    w, h, nf, nl, sf, ini, mn = k
    return pkg.ORBextractor(nf, sf, nl, ini, mn, max_size=(w, h), max_batch=max_batch)


def reading_of(c, levels):
    """The reading's result for a case on these level images (the same images every time: asserted)."""
    if c["name"] not in _READ:
        _READ[c["name"]] = (levels, sr.extract(levels, c["nf"], c["sf"], c["ini"], c["mn"], c["lap"]))
    kept, rd = _READ[c["name"]]
    assert len(kept) == len(levels) and all(np.array_equal(a, b) for a, b in zip(kept, levels)), c["name"]
    return rd


def check_frame(ex, c, result, frame=0):
    """One frame of the last call on `ex` against the reading: stages per level, then the final output."""
    mono, kps, desc = result
    levels = [ex.level_image(l, frame=frame) for l in range(c["nl"])]
    assert np.array_equal(levels[0], c["img"]), c["name"]
    rd = reading_of(c, levels)
    for k in c["want"]:
        assert rd["counters"][k] > 0, (c["name"], k)
    for l in range(c["nl"]):
        assert np.array_equal(ex.level_candidates(l, frame=frame), rd["candidates"][l]), (c["name"], "candidates", l)
        assert np.array_equal(ex.level_selected(l, frame=frame), rd["level_keypoints"][l]), (c["name"], "selection", l)
    f = sr.fields_array(rd["fields"])
    assert len(kps) == len(f) and mono == rd["mono"], (c["name"], len(kps), len(f), mono, rd["mono"])
    for name in sr.KEY_FIELDS:
        assert kps[name].tobytes() == f[name].tobytes(), (c["name"], name)
    assert desc.shape == (len(f), 32)
    if c["n_out"] is not None:
        assert len(kps) == c["n_out"], c["name"]


@pytest.mark.parametrize("k", list(GROUPS), ids=group_id)
def test_single_and_batched_frames_equal_the_reading(pkg, k):
    """Each frame alone, then all frames of the group through one extract_batch call (side by side in k_quadtree2's grid), each with
    its own lapping area: the batch equals the reading frame by frame, and the single calls byte for byte (angle and descriptors too)."""
    group = GROUPS[k]
    ex = make_extractor(pkg, k, max_batch=len(group))
    try:
        single = []
        for c in group:
            single.append(ex(c["img"], c["lap"]))
            assert ex.quadtree_threads() == 1024                  # one frame: the wide form
            check_frame(ex, c, single[-1])
        batch = ex.extract_batch([c["img"] for c in group], [c["lap"] for c in group])
        for i, c in enumerate(group):
            check_frame(ex, c, batch[i], frame=i)
            assert batch[i][0] == single[i][0] and batch[i][1].tobytes() == single[i][1].tobytes() and np.array_equal(batch[i][2], single[i][2]), c["name"]
    finally:
        ex.close()


def test_wide_frames_with_small_budgets_return_four_nodes_per_root(pkg):
    """1241 x 376 (four roots) and 2400 x 420 (six) with budgets below 4 * nIni: the first pass of DistributeOctTree splits every root
    before it looks at N, so a level returns 16 / 24 keypoints -- k_quadtree2's list must hold them (orbx_plan.h: qt2Cap)."""
    for name, n in (("wide_1241_nl1_N4", 16), ("wide_1241_nl1_N7", 16), ("wide_2400_nl1_N11", 24), ("wide_2400_nl1_N15", 24)):
        c = next(c for c in CASES if c["name"] == name)
        ex = make_extractor(pkg, ec.key(c))
        try:
            res = ex(c["img"], c["lap"])
            assert len(res[1]) == n <= ex.cap
            check_frame(ex, c, res)
        finally:
            ex.close()


# k_quadtree2 runs 1024 threads per (frame, level) when some level wants >= 512 nodes or the grid is small (frames * levels <= 512),
# 256 otherwise (orbx_plan.h, qt_wide).  One frame takes the wide form; 520 one-level / 260 two-level frames the narrow one.
def _max_n(k):
    """maxN of orbx_plan.h: the largest max(N, 4 * nIni) of any level; the wide form is chosen from 512 on."""
    w, h, nf, nl, sf = k[:5]
    budget = sr.features_per_level(nf, sf, nl)
    return max(max(n, 4 * sr.c_round(np.float32(lw - 32) / np.float32(lh - 32))) for n, (lw, lh) in zip(budget, sr.level_sizes(w, h, sf, nl)))


# (frames up to 180 x 180 only: a batch of 520 of them stays small)
NARROW = [k for k in GROUPS if k[0] * k[1] <= 180 * 180 and _max_n(k) < 512]


@pytest.mark.parametrize("size", sorted({(k[0], k[1], k[3], k[4]) for k in NARROW}), ids=lambda s: "%dx%d-nl%d-sf%s" % s)
def test_narrow_workgroups_equal_the_reading(pkg, size):
    """All groups of one frame size, each repeated into a batch of more than 512 (frame, level) pairs: the 256-thread form of
    k_quadtree2.  Every distinct frame of the batch is held to the reading at its first and at its last position."""
    for k in [k for k in NARROW if (k[0], k[1], k[3], k[4]) == size]:
        group = GROUPS[k]
        nl = k[3]
        nframes = 512 // nl + 8
        assert nframes * nl > 512
        order = [group[i % len(group)] for i in range(nframes)]
        ex = make_extractor(pkg, k, max_batch=nframes)
        try:
            res = ex.extract_batch([c["img"] for c in order], [c["lap"] for c in order])
            assert ex.quadtree_threads() == 256
            first = {}
            for i, c in enumerate(order):
                if c["name"] not in first:
                    first[c["name"]] = i
                    check_frame(ex, c, res[i], frame=i)
                else:
                    j = first[c["name"]]
                    assert res[i][0] == res[j][0] and res[i][1].tobytes() == res[j][1].tobytes() and np.array_equal(res[i][2], res[j][2]), (c["name"], i)
            for c in group:
                i = max(i for i, o in enumerate(order) if o is c)
                check_frame(ex, c, res[i], frame=i)
        finally:
            ex.close()
