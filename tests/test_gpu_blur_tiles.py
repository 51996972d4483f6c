"""k_blur3's strip, tile and walk geometry, held byte for byte to the exact integer statement of the blur (tests/blur_cases.py).

The frames of a geometry (value noise, random 0 / 255 pixels, all 0, all 255, two impulse frames) run as one batch: as device
pointers in permuted slots under a pitch wider than the image with 255 in the padding, and as host images.  For every frame and every
level -- whether or not a keypoint was selected there: the oracle blurs no other level, and an all-black frame has none at all -- the
blurred level must equal gauss7_exact of the device's own un-blurred level, the un-blurred level the oracle's, and the key points,
descriptors and mono counts the oracle's (k_orient_desc2 reads the tiled layout that k_blur3 writes, at the same edges).
`blur_form()` is asserted wherever a form is claimed: 0 = one tile per workgroup, 1 = the walk with double-buffered LDS (a batch with
frames x walk tasks >= 2048), 2 = k_blur2.  tests/ab/test_ab_blur_tiles.py forces the forms on the A/B library with the helpers below."""
import ctypes as C

import numpy as np
import pytest

import blur_cases as bc
from blur_cases import GEOMS, gauss7_exact

_refs, _exact = {}, {}


def _ref(oracle, synth, name, i):
    """(levels, n, kps bytes, desc, mono) of image i of a geometry from the oracle, computed once."""
    if (name, i) not in _refs:
        _, _, nl, sf, _ = GEOMS[name]
        ref = oracle.Extractor(bc.NFEATURES, sf, nl, bc.INI_TH, bc.MIN_TH)
        n, kps, desc, mono = ref(bc.image(synth, name, i), (0, 0))
        _refs[(name, i)] = ([ref.level_image(l).copy() for l in range(nl)], n, kps.tobytes(), desc.copy(), mono)
    return _refs[(name, i)]


def _statement(level):
    """gauss7_exact of an un-blurred level, computed once per distinct level."""
    key = (level.shape, level.tobytes())
    if key not in _exact:
        _exact[key] = gauss7_exact(level).tobytes()
    return _exact[key]


class DeviceFrames:
    """The frames of a batch in one device buffer, in permuted slots with a gap between them, 255 in the row padding and the gaps.
    stride None: a pitch wider than the image; otherwise the given one (a multiple of 16)."""

    def __init__(self, pkg, imgs, stride=None):
        h, w = imgs[0].shape
        self.w, self.h, self.stride = w, h, stride or (w + 63) // 64 * 64 + 64
        assert self.stride >= w and self.stride % 16 == 0
        slot = (self.stride * h + 192 + 255) // 256 * 256
        n = len(imgs)
        order = [(7 * i + 3) % n for i in range(n)] if n % 7 else list(range(n))[::-1]
        assert sorted(order) == list(range(n))
        self.buf = pkg.DeviceBuffer(slot * n)
        flat = np.full(slot, 255, np.uint8)
        pad = flat[:self.stride * h].reshape(h, self.stride)
        for i, im in enumerate(imgs):
            pad[:, :w] = im
            self.buf.upload(flat, offset=order[i] * slot)
        self.ptrs = (C.c_void_p * n)(*[self.buf.ptr + order[i] * slot for i in range(n)])


def compare(ex, res, oracle, synth, name, which, tag, level_frames=None, form=0):
    """which[f] = the image of frame f.  Both copies of every level of the frames in level_frames (default: all) against the oracle and
    the statement (first: a wrong blurred byte is reported as such, not as the descriptor it changes), then the results of every frame
    against the oracle."""
    nl = GEOMS[name][2]
    assert ex.blur_form() == form, (name, tag, ex.blur_form())
    assert len(res) == len(which)
    for f in (range(len(which)) if level_frames is None else level_frames):
        levels = _ref(oracle, synth, name, which[f])[0]
        for l in range(nl):
            if l or not tag.startswith("device"):
                own = ex.level_image(l, f)
                assert own.tobytes() == levels[l].tobytes(), (name, tag, "frame %d level %d" % (f, l))
            else:                                                                            # level 0 of a device-resident input is the caller's buffer:
                own = bc.image(synth, name, which[f])                                        # the handle keeps no copy of it to fetch
            got = ex.level_image(l, f, blurred=True)
            if got.tobytes() != _statement(own):
                bad = np.argwhere(got != np.frombuffer(_statement(own), np.uint8).reshape(own.shape))
                raise AssertionError((name, tag, "blurred frame %d level %d: %d bytes differ, first (y, x) %s, rows %d..%d, columns %d..%d"
                                      % (f, l, len(bad), tuple(int(v) for v in bad[0]), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())))
    for f, i in enumerate(which):
        _, n, kps, desc, mono = _ref(oracle, synth, name, i)
        m, k, d = res[f]
        assert len(k) == n and m == mono, (name, tag, f)
        assert k.tobytes() == kps and np.array_equal(d, desc), (name, tag, f)


def make(pkg, name, max_batch):
    w, h, nl, sf, _ = GEOMS[name]
    ex = pkg.ORBextractor(bc.NFEATURES, sf, nl, bc.INI_TH, bc.MIN_TH, max_size=(w, h), max_batch=max_batch)
    assert ex.blur_form() == -1
    return ex


def run_device(pkg, oracle, synth, name, which, max_batch=None, graph=False, form=0, level_frames=None, stride=None):
    w, h = GEOMS[name][:2]
    ex = make(pkg, name, max_batch or len(which))
    try:
        dev = DeviceFrames(pkg, [bc.image(synth, name, i) for i in which], stride)
        lap = np.zeros(2 * len(which), np.int32)
        ex.enqueue_device(dev.ptrs, w, h, dev.stride, lap)
        ex.sync()
        res = ex.fetch_all()
        compare(ex, res, oracle, synth, name, which, "device", level_frames, form)
        if graph:
            L = pkg.lib()
            assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
            ex.enqueue_device(dev.ptrs, w, h, dev.stride, lap)
            assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            ex.sync()
            again = ex.fetch_all()
            for (m0, k0, d0), (m1, k1, d1) in zip(res, again):
                assert m0 == m1 and k0.tobytes() == k1.tobytes() and np.array_equal(d0, d1)
            compare(ex, again, oracle, synth, name, which, "device replay", level_frames, form)
        return [[ex.level_image(l, f, blurred=True) for l in range(GEOMS[name][2])] for f in (level_frames or range(len(which)))]
    finally:
        ex.close()


def run_host(pkg, oracle, synth, name, which, form=0, level_frames=None):
    ex = make(pkg, name, len(which))
    try:
        imgs = [bc.image(synth, name, i) for i in which]
        res = ex.extract_batch(imgs, [(0, 0)] * len(imgs)) if len(imgs) > 1 else [ex(imgs[0], (0, 0))]
        compare(ex, res, oracle, synth, name, which, "host", level_frames, form)
    finally:
        ex.close()


def all_images(name):
    return list(range(GEOMS[name][4]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMS))
def test_blurred_levels_of_a_batch_equal_the_statement(pkg, oracle, synth, name):
    run_device(pkg, oracle, synth, name, all_images(name))
    run_host(pkg, oracle, synth, name, all_images(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMS))
def test_single_frame_call(pkg, oracle, synth, name):
    """The single-frame entry point with the impulse frame and with value noise, and a device batch of one."""
    run_host(pkg, oracle, synth, name, [4])
    run_host(pkg, oracle, synth, name, [0])
    run_device(pkg, oracle, synth, name, [5])


@pytest.mark.gpu
def test_batch_smaller_than_the_handle(pkg, oracle, synth):
    run_device(pkg, oracle, synth, "fold1", [1, 4, 0], max_batch=16)
    run_device(pkg, oracle, synth, "tall16", [5, 3, 1, 0], max_batch=9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fold32", "tall16"])
def test_graph_replay_equals_eager(pkg, oracle, synth, name):
    run_device(pkg, oracle, synth, name, all_images(name), graph=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMS))
def test_source_clamp_tight_and_wide_pitch(pkg, oracle, synth, name):
    """Under a level-0 pitch of exactly align16(w) the staging pieces right of it are clamped to column 0 (and where w is a multiple of
    16 there is no padding at all: every piece past the edge is); under the wide pitch they read the 255 padding.  Either way they
    meet zero weights only: the same blurred bytes, and both the statement's (compare)."""
    w = GEOMS[name][0]
    tight = run_device(pkg, oracle, synth, name, all_images(name), stride=(w + 15) // 16 * 16)
    wide = run_device(pkg, oracle, synth, name, all_images(name))
    for a, b in zip(tight, wide):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


@pytest.mark.gpu
def test_the_walk_on_the_product_library(pkg, oracle, synth):
    """The geometry with the most walk tasks per frame, with as many frames as the walking form needs (frames x walk tasks >= 2048) and
    one fewer (the one-tile form) on the same handle and the same device frames: six images in turn, one frame the odd one out.
    Results of every frame; every level of the first, the last, the odd and ten seeded other frames."""
    name = bc.MOST_WALK_TASKS
    tasks = bc.walk_tasks(bc.level_sizes(oracle, name))
    frames = (2048 + tasks - 1) // tasks
    assert 100 < frames < 200 and (frames - 1) * tasks < 2048 <= frames * tasks
    w, h = GEOMS[name][:2]
    odd = 101
    which = [i % len(bc.IMAGE_KINDS) for i in range(frames)]
    which[odd] = len(bc.IMAGE_KINDS)                                                          # value noise with a seed of its own
    assert len(set(which)) >= 6 and which.count(which[odd]) == 1
    rng = np.random.default_rng(11)
    picked = sorted({0, frames - 1, odd} | set(int(v) for v in rng.choice(np.arange(1, frames - 1), 10, replace=False)))
    ex = make(pkg, name, frames)
    try:
        dev = DeviceFrames(pkg, [bc.image(synth, name, i) for i in which])
        for n, form in ((frames - 1, 0), (frames, 1)):
            ptrs = (C.c_void_p * n)(*dev.ptrs[:n])
            ex.enqueue_device(ptrs, w, h, dev.stride, np.zeros(2 * n, np.int32))
            ex.sync()
            assert ex.blur_form() == form
            compare(ex, ex.fetch_all(), oracle, synth, name, which[:n], "device walk %d" % form, [f for f in picked if f < n] + [n - 1], form)
    finally:
        ex.close()
