"""k_quadtree2's table mode and its fallback on the hand-laid frames of tests/quadtree_table_cases.py: candidates, the quadtree's
selection in its output order and the final keypoints against the second reading (check_frame of
tests/test_gpu_extract_second_reading.py), singly (1024-thread workgroups) and in batches of more than 512 (frame, level) pairs
(256-thread workgroups) in which frames that fall back and frames that do not alternate.  orbx_quadtree_fallbacks tells which path
ran: over every frame it must move by exactly the number of levels that, by the second reading with DivideNode watched, run a pass
after one that made a several-key node at the table depth (tests/test_quadtree_table_cases_cpu.py shows on the reading alone which
frames those are, and that the levels a case declares deep by the reference's halving are among them)."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as ec
import quadtree_table_cases as qc
from test_gpu_extract_second_reading import _max_n, check_frame, make_extractor, reading_of

pytestmark = pytest.mark.gpu

CASES = qc.all_cases()
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(ec.key(_c), []).append(_c)


def group_id(k):
    return "%dx%d-nf%d-nl%d-sf%s" % k[:5]


def falls(ex, c, frame=0):
    """How many levels of this frame leave table mode: the reading of the frame's own level images, DivideNode watched
    (quadtree_table_cases.levels_that_fall_back); the levels a case declares deep by construction are among them."""
    levels = [ex.level_image(l, frame=frame) for l in range(c["nl"])]
    out = qc.levels_that_fall_back(c, reading_of(c, levels))
    assert set(c["deep"]) <= set(out), c["name"]
    return len(out)


@pytest.mark.parametrize("k", list(GROUPS), ids=group_id)
def test_single_frames(pkg, k):
    ex = make_extractor(pkg, k)
    try:
        for c in GROUPS[k]:
            before = ex.quadtree_fallbacks()
            res = ex(c["img"], c["lap"])
            assert ex.quadtree_threads() == 1024
            moved = ex.quadtree_fallbacks() - before
            check_frame(ex, c, res)
            assert moved == falls(ex, c), c["name"]
    finally:
        ex.close()


@pytest.mark.parametrize("k", list(GROUPS), ids=group_id)
def test_interleaved_batches(pkg, k):
    """The group's frames in turn (deep, shallow, deep, ...) until the grid has more than 512 workgroups."""
    group = GROUPS[k]
    nl = k[3]
    nframes = 512 // nl + 8
    order = [group[i % len(group)] for i in range(nframes)]
    ex = make_extractor(pkg, k, max_batch=nframes)
    try:
        before = ex.quadtree_fallbacks()
        res = ex.extract_batch([c["img"] for c in order], [c["lap"] for c in order])
        assert ex.quadtree_threads() == (256 if _max_n(k) < 512 else 1024)
        moved = ex.quadtree_fallbacks() - before
        first, want = {}, 0
        for i, c in enumerate(order):
            if c["name"] not in first:
                first[c["name"]] = (i, falls(ex, c, frame=i))
                check_frame(ex, c, res[i], frame=i)
            else:
                j = first[c["name"]][0]
                assert res[i][0] == res[j][0] and res[i][1].tobytes() == res[j][1].tobytes() and np.array_equal(res[i][2], res[j][2]), (c["name"], i)
            want += first[c["name"]][1]
        for c in group:                                                          # and at its last position
            i = max(i for i, o in enumerate(order) if o is c)
            check_frame(ex, c, res[i], frame=i)
        assert moved == want, (moved, want)
    finally:
        ex.close()


def test_ladders_move_the_counter_exactly(pkg):
    """The ladders and triples alone, held to what the reference's halving says of them (not to the watched reading): the counter moves by
    the number of deep frames, singly and batched."""
    seen_deep = seen_shallow = 0
    for k, whole in GROUPS.items():
        group = [c for c in whole if c["name"].startswith(("ladder", "triple"))]
        if not group:
            continue
        order = (group * 3)[:max(6, len(group))]
        ex = make_extractor(pkg, k, max_batch=len(order))
        try:
            for c in group:
                before = ex.quadtree_fallbacks()
                ex(c["img"], c["lap"])
                assert ex.quadtree_fallbacks() - before == len(c["deep"]), c["name"]
            before = ex.quadtree_fallbacks()
            ex.extract_batch([c["img"] for c in order], [c["lap"] for c in order])
            assert ex.quadtree_fallbacks() - before == sum(len(c["deep"]) for c in order), group_id(k)
            seen_deep += sum(len(c["deep"]) > 0 for c in group); seen_shallow += sum(len(c["deep"]) == 0 for c in group)
        finally:
            ex.close()
    assert seen_deep >= 8 and seen_shallow >= 14


def test_graph_replays_give_identical_bytes(pkg):
    """A captured step of six frames (three fall back) replayed twice: the same bytes as the eager batch each time, and the counter --
    never reset inside the step -- moves by three per replay."""
    k = next(k for k in GROUPS if k[2] == 60 and any(c["deep"] for c in GROUPS[k]))
    group = [c for c in GROUPS[k] if c["name"].startswith(("ladder", "triple"))]
    deep, shallow = [c for c in group if c["deep"]], [c for c in group if not c["deep"]]
    order = [deep[0], shallow[0], deep[1 % len(deep)], shallow[1 % len(shallow)], deep[0], shallow[0]]
    ex = make_extractor(pkg, k, max_batch=len(order))
    L = pkg.lib()
    try:
        eager = ex.extract_batch([c["img"] for c in order], [c["lap"] for c in order])
        h, w = order[0]["img"].shape
        stride = (w + 63) // 64 * 64
        buf = pkg.DeviceBuffer(stride * h * len(order))
        for i, c in enumerate(order):
            pad = np.zeros((h, stride), np.uint8)
            pad[:, :w] = c["img"]
            buf.upload(pad.reshape(-1), offset=i * stride * h)
        ptrs = (C.c_void_p * len(order))(*[buf.ptr + i * stride * h for i in range(len(order))])
        lap = np.zeros(2 * len(order), np.int32)
        ex.enqueue_device(ptrs, w, h, stride, lap)                               # (a capture wants the same batch enqueued once before it)
        ex.sync()
        assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
        ex.enqueue_device(ptrs, w, h, stride, lap)
        assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
        for _ in range(2):
            before = ex.quadtree_fallbacks()
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            ex.sync()
            got = ex.fetch_all()
            assert ex.quadtree_fallbacks() - before == 3
            for i, c in enumerate(order):
                assert got[i][0] == eager[i][0] and got[i][1].tobytes() == eager[i][1].tobytes() and np.array_equal(got[i][2], eager[i][2]), c["name"]
    finally:
        ex.close()
