"""k_orient_desc2's patch, lane-group and frame geometry, held bit for bit to the numpy statement of IC_Angle and computeOrbDescriptor
(tests/orient_cases.py: fast_atan2_np; umax_table, moments and descriptors of tests/test_oracle_structured_cpu.py).

For every frame, level and keypoint the statement is applied to the device's own un-blurred level (the caller's image for a
device-resident level 0), its own blurred level and its own level_selected points, and the `angle` field and the 32 descriptor bytes of
the final output -- mapped onto the levels by the epilogue of tests/second_reading_extract.py -- must equal it; the first differing
keypoint is reported with its level, position, column phase and angle.  The whole result is then compared with the oracle.  The frames
(tests/test_orient_cases_cpu.py holds them to their classes) run as host images, as device pointers under a tight and a wide pitch with
255 in the padding, singly, on a handle larger than the frame needs, in batches around the 8-frame XCD deal, and through one graph
replay with refilled inputs.  `orient_form()` is asserted in every comparison: 0 = k_orient_desc2 on tiles;
tests/ab/test_ab_orient_geometry.py runs the same helpers on the row-major layout (1) and with k_orient_desc (2)."""
import ctypes as C

import numpy as np
import pytest

import orient_cases as oc
import second_reading_extract as sr
from orient_cases import FRAMES

_oracle = {}


def spec(name):
    f = FRAMES[name]
    return dict(img=f["img"], nf=f["nf"], sf=f["sf"], nl=f["nl"], name=name)


def batch_specs(size):
    return [dict(img=im, name="batch%d[%d]" % (size, i), **oc.BATCH_PARAMS) for i, im in enumerate(oc.batch_images(size))]


def oracle_result(oracle, s):
    """(n, keypoint bytes, descriptors, mono) of a frame from the oracle, computed once per distinct image and parameters."""
    key = (s["img"].shape, s["img"].tobytes(), s["nf"], s["sf"], s["nl"])
    if key not in _oracle:
        n, kps, desc, mono = oracle.Extractor(s["nf"], s["sf"], s["nl"], oc.INI_TH, oc.MIN_TH)(s["img"], (0, 0))
        assert n >= 0, s["name"]
        _oracle[key] = (n, kps.tobytes(), desc.copy(), mono)
    return _oracle[key]


def check_frame(ex, oracle, s, result, frame, tag, device_level0):
    """One frame of the last call on `ex`: the statement on the device's own levels and selection, then the oracle."""
    mono, kps, desc = result
    nl = s["nl"]
    sf = sr.scale_factors(s["sf"], nl)[0]
    pattern = oracle.pattern()
    records, want_angle, want_desc, where = [], [], [], []
    for l in range(nl):
        sel = ex.level_selected(l, frame=frame)
        size = int(np.float32(np.float32(31) * np.float32(sf[l])))
        records.append([(np.float32(x), np.float32(y), np.float32(size), np.float32(r), l, -1) for x, y, r in sel])
        if len(sel) == 0:
            continue
        level = s["img"] if l == 0 and device_level0 else ex.level_image(l, frame=frame)
        if l == 0:
            assert np.array_equal(level, s["img"]), (s["name"], tag)
        blurred = ex.level_image(l, frame=frame, blurred=True)
        xs, ys = sel[:, 0].astype(np.int64), sel[:, 1].astype(np.int64)
        assert xs.min() >= 19 and ys.min() >= 19 and xs.max() <= level.shape[1] - 20 and ys.max() <= level.shape[0] - 20
        a, d, m01, m10 = oc.statement(level, blurred, xs, ys, pattern)
        want_angle.append(a); want_desc.append(d)
        where += [(l, int(x), int(y)) for x, y in zip(xs, ys)]
    perm, fields, want_mono = sr.assemble(records, (0, 0), sf)
    f = sr.fields_array(fields)
    assert len(kps) == len(f) and mono == want_mono and desc.shape == (len(f), 32), (s["name"], tag, frame, len(kps), len(f))
    for name in sr.KEY_FIELDS:
        assert kps[name].tobytes() == f[name].tobytes(), (s["name"], tag, frame, name)
    if len(f):
        perm = np.array(perm, np.int64)
        want_angle = np.concatenate(want_angle)[perm]; want_desc = np.concatenate(want_desc)[perm]
        bad = np.flatnonzero((kps["angle"].view(np.uint32) != want_angle.view(np.uint32)) | (desc != want_desc).any(1))
        if len(bad):
            i = int(bad[0])
            l, x, y = where[perm[i]]
            raise AssertionError("%s, %s, frame %d: %d of %d keypoints differ from the statement; first: slot %d, level %d, (x, y) = (%d, %d), "
                                 "column phase %d, row phase %d, angle %r (statement %r), %d descriptor bits differ"
                                 % (s["name"], tag, frame, len(bad), len(f), i, l, x, y, (x - 18) & 7, (y - 18) & 7, float(kps["angle"][i]),
                                    float(want_angle[i]), int(np.unpackbits(desc[i] ^ want_desc[i]).sum())))
    n, okps, odesc, omono = oracle_result(oracle, s)
    assert len(kps) == n and mono == omono, (s["name"], tag, frame, len(kps), n)
    assert kps.tobytes() == okps and np.array_equal(desc, odesc), (s["name"], tag, frame, "oracle")


def compare(ex, oracle, specs, res, tag, form, device_level0=False):
    assert ex.orient_form() == form, (tag, ex.orient_form())
    assert len(res) == len(specs)
    for f, s in enumerate(specs):
        check_frame(ex, oracle, s, res[f], f, tag, device_level0)


def make(pkg, s, max_batch=1, max_size=None, nf=None):
    h, w = s["img"].shape
    ex = pkg.ORBextractor(nf or s["nf"], s["sf"], s["nl"], oc.INI_TH, oc.MIN_TH, max_size=max_size or (w, h), max_batch=max_batch)
    assert ex.orient_form() == -1
    return ex


class DeviceFrames:
    """The frames of a batch in one device buffer, in permuted slots with a gap between them, 255 in the row padding and the gaps.
    tight: a pitch of align16(w); otherwise one wider than the image.  fill() uploads other images into the same slots."""

    def __init__(self, pkg, imgs, tight=False):
        h, w = imgs[0].shape
        self.w, self.h = w, h
        self.stride = (w + 15) // 16 * 16 if tight else (w + 63) // 64 * 64 + 64
        self.slot = (self.stride * h + 192 + 255) // 256 * 256
        n = len(imgs)
        self.order = [(7 * i + 3) % n for i in range(n)] if n % 7 else list(range(n))[::-1]
        assert sorted(self.order) == list(range(n))
        self.buf = pkg.DeviceBuffer(self.slot * n)
        self.ptrs = (C.c_void_p * n)(*[self.buf.ptr + self.order[i] * self.slot for i in range(n)])
        self.fill(imgs)

    def fill(self, imgs):
        assert len(imgs) == len(self.order)
        flat = np.full(self.slot, 255, np.uint8)
        pad = flat[:self.stride * self.h].reshape(self.h, self.stride)
        for i, im in enumerate(imgs):
            assert im.shape == (self.h, self.w)
            pad[:, :self.w] = im
            self.buf.upload(flat, offset=self.order[i] * self.slot)


def run_host(pkg, oracle, specs, form=0, singly=True, **handle):
    """The frames one by one through the single-frame call, then all of them through one extract_batch call."""
    ex = make(pkg, specs[0], max_batch=handle.pop("max_batch", len(specs)), **handle)
    try:
        if singly:
            for s in specs:
                compare(ex, oracle, [s], [ex(s["img"], (0, 0))], "host single", form)
        if len(specs) > 1 or not singly:
            res = ex.extract_batch([s["img"] for s in specs], [(0, 0)] * len(specs))
            compare(ex, oracle, specs, res, "host batch", form)
    finally:
        ex.close()


def run_device(pkg, oracle, specs, form=0, tight=False, refill=None, **handle):
    """The frames as device pointers; refill: capture the step, upload these other frames into the same buffers, replay once."""
    ex = make(pkg, specs[0], max_batch=handle.pop("max_batch", len(specs)), **handle)
    try:
        dev = DeviceFrames(pkg, [s["img"] for s in specs], tight)
        lap = np.zeros(2 * len(specs), np.int32)
        ex.enqueue_device(dev.ptrs, dev.w, dev.h, dev.stride, lap)
        ex.sync()
        res = ex.fetch_all()
        compare(ex, oracle, specs, res, "device tight" if tight else "device wide", form, device_level0=True)
        if refill is not None:
            L = pkg.lib()
            assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
            ex.enqueue_device(dev.ptrs, dev.w, dev.h, dev.stride, lap)
            assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
            dev.fill([s["img"] for s in refill])
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            ex.sync()
            compare(ex, oracle, refill, ex.fetch_all(), "device replay", form, device_level0=True)
        return res
    finally:
        ex.close()


GROUPS = {name: [name] for name in oc.BORDER + oc.DOUBLED}
GROUPS["compass_and_saturated"] = ["compass_240x200"] + oc.SATURATED
GROUPS["counts"] = oc.COUNT


def group(name):
    return [spec(n) for n in GROUPS[name]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GROUPS))
def test_host_images_singly_and_batched(pkg, oracle, name):
    run_host(pkg, oracle, group(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GROUPS))
def test_device_pointers_tight_and_wide_pitch(pkg, oracle, name):
    """IC_Angle reads level 0 of a device-resident frame from the caller's buffer at the caller's pitch: 32-byte rows from cx - 15, which
    at x = w - 20 end 4 px inside the image.  The 255 in the padding and between the frames must never show, and a pitch of exactly
    align16(w) (no padding at all where w is a multiple of 16) and a wide one give the same result."""
    tight = run_device(pkg, oracle, group(name), tight=True)
    wide = run_device(pkg, oracle, group(name))
    for (m0, k0, d0), (m1, k1, d1) in zip(tight, wide):
        assert m0 == m1 and k0.tobytes() == k1.tobytes() and np.array_equal(d0, d1)


@pytest.mark.gpu
def test_single_frames_as_device_batches_of_one(pkg, oracle):
    for name in (oc.BORDER[0], oc.DOUBLED[0], "sat_bright_dots", "count_0", "count_1", "count_17"):
        run_device(pkg, oracle, [spec(name)])


@pytest.mark.gpu
def test_handle_larger_than_the_frame_needs(pkg, oracle):
    """max_batch, max_size and nfeatures above what the frames need: the grid has workgroups beyond every frame's n, and frames beyond
    the batch.  (nfeatures is part of the result: the oracle runs with the same 1000.)"""
    specs = [dict(s, nf=1000) for s in group("counts")]
    run_host(pkg, oracle, specs, max_size=(752, 480), max_batch=12, nf=1000)
    run_device(pkg, oracle, specs[:5], max_size=(752, 480), max_batch=12, nf=1000)
    specs = [dict(spec(oc.BORDER[0]), nf=1000)]
    run_host(pkg, oracle, specs, max_size=(640, 400), max_batch=3, nf=1000)


@pytest.mark.gpu
@pytest.mark.parametrize("size", oc.BATCH_SIZES)
def test_batches_around_the_xcd_deal(pkg, oracle, size):
    """1, 7, 8, 9, 16 and 17 frames whose images all differ, with very different n: the workgroups of the first 8 * (size / 8) frames
    are dealt over the XCDs, the others keep their grid position.  Every frame of every batch is checked.  The host batch takes the
    frames one place on: a wrong (frame, chunk) of the deal shows only where the frame it skips has keypoints in that chunk, and
    in one order that frame may be an empty one."""
    specs = batch_specs(size)
    run_device(pkg, oracle, specs)
    run_host(pkg, oracle, specs[1:] + specs[:1], singly=False)


@pytest.mark.gpu
def test_graph_replay_with_refilled_inputs(pkg, oracle):
    """The captured step of a batch of 9 replayed once after other frames went into the same device buffers: the frames one place
    on, so that every slot holds another image and another n than at capture."""
    specs = batch_specs(9)
    refill = specs[1:] + specs[:1]
    run_device(pkg, oracle, specs, refill=refill)
