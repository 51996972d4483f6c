"""k_resize2's task lists: full column tiles of one frame, packed remainder tiles of several frames, one row record per task.

A level of ndw = ceil(w / 4) dwords has ndw // 64 full tiles and, for r = ndw % 64, one packed tile whose wave serves pack = 64 // r
consecutive frames.  What decides which lanes of which wave touch which frame is the level's width (r, pack), the number of frames
against pack, and the level's height against the rows of a task -- so the frames below are small ones chosen for those numbers.
`test_geometries_contain_the_classes` derives every level's dword count, remainder and pack from the oracle's level_size and fails if a
geometry stops containing the class it is listed for.  The frames of a batch are all different images, handed over as device pointers
in permuted, non-contiguous order under a level-0 pitch wider than the image (or as host images: the staged level 0); every unblurred
level of every frame is compared byte for byte with the oracle's, and so are the key points and descriptors.

A level shorter than 16 rows does not exist: the extractor needs a 35-px FAST cell inside a 16-px border on every level (h >= 67)."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_LIB = os.path.join(ROOT, "orb-slam3_amd", "liborbslam3_amd_ab.so")

# name -> (w, h, nlevels, scale factor, frames)
GEOMS = {
    # level 1: 260 x 80 = 65 dwords, one full tile + remainder 1 (pack 64), h % 16 == 0; level 2: 217 x 67 = 55 dwords, narrower than a wave
    "pack64": (312, 96, 3, 1.2, 65),
    # level 1: 256 x 96 = 64 dwords, remainder 0 (no packed tile)
    "aligned": (307, 115, 3, 1.2, 3),
    # level 1: 512 x 81, two full tiles, h % 16 == 1; level 2: 426 x 67 = 107 dwords, a full tile + remainder 43 (pack 1)
    "wide": (614, 97, 3, 1.2, 3),
    # level 1: 275 x 95 = 69 dwords, remainder 5 (pack 12), the last dword holds 3 pixels, h % 16 == 15; 13 frames = one full wave + one group
    "pack12": (330, 114, 3, 1.2, 13),
    # level 1: 351 x 106 = 88 dwords, remainder 24 (pack 2), the last dword holds 3 pixels; level 2: 292 x 88, remainder 9 (pack 7)
    "pack2": (421, 127, 3, 1.2, 5),
    # level 1: 320 x 83 = 80 dwords, remainder 16 (pack 4)
    "pack4": (384, 100, 2, 1.2, 6),
    # scale factor 1.5, the streaming limit (8-byte tap window, every task spans the 12 source rows a task may touch); level 1: 267 x 102,
    # remainder 3 (pack 21); level 2: 178 x 68
    "scale15": (400, 153, 3, 1.5, 4),
    # scale factor 1.7: the general kernel (k_resize) makes the pyramid, as before
    "scale17": (400, 140, 2, 1.7, 3),
}
LARGEST_PACK = "pack64"


def classes_of(oracle, name):
    """[(level, w, h, dwords, remainder, pack)] of the destination levels (1 .. L-1), from the oracle's level_size."""
    w, h, nl, sf, _ = GEOMS[name]
    ref = oracle.Extractor(200, sf, nl, 20, 7)
    ref(np.zeros((h, w), np.uint8), (0, 0))
    out = []
    for l in range(1, nl):
        lw, lh = ref.level_size(l)
        ndw = (lw + 3) // 4
        r = ndw % 64
        out.append((l, lw, lh, ndw, r, 64 // r if r else 0))
    return out


def test_geometries_contain_the_classes(oracle):
    c = {k: classes_of(oracle, k) for k in GEOMS if k != "scale17"}
    lv = [x for k in c for x in c[k]]
    assert any(r == 0 for _, _, _, _, r, _ in lv)                                            # no packed tile
    assert c["aligned"][0][3] == 64 and c["wide"][0][3] == 128
    assert any(ndw < 64 and p == 1 for _, _, _, ndw, _, p in lv)                             # packed kind only, pack 1
    assert any(r == 1 and p == 64 and ndw > 64 for _, _, _, ndw, r, p in lv)                 # pack 64 beside a full tile
    assert any(2 <= r <= 12 and p >= 5 for _, _, _, _, r, p in lv)
    assert any(13 <= r <= 21 and 3 <= p <= 4 for _, _, _, _, r, p in lv)
    assert any(22 <= r <= 32 and p == 2 for _, _, _, _, r, p in lv)
    assert any(33 <= r <= 63 and p == 1 and ndw > 64 for _, _, _, ndw, r, p in lv)           # pack 1 beside a full tile
    assert max(p for _, _, _, _, _, p in lv) == max(p for _, _, _, _, _, p in c[LARGEST_PACK]) == 64
    assert any(lw % 4 and p >= 2 for _, lw, _, _, _, p in lv)                                # partial last dword inside a packed group
    assert {0, 1, 15} <= {lh % 16 for _, _, lh, _, _, _ in lv}
    for k, v in c.items():                                                                   # frames against pack: a last wave that is not full
        packs = [p for _, _, _, _, _, p in v if p > 1]
        assert not packs or any(GEOMS[k][4] % p for p in packs), k
    assert GEOMS["scale15"][3] == 1.5 and GEOMS["scale17"][3] > 1.5
    # scale factor 1.5: some 8-row task of level 1 (which has a full tile and a packed one) spans 12 source rows, the most a task may
    # touch, and none spans more (cv::resize: sy = floor((dy + 0.5) * src_h / dst_h - 0.5); a task reads rows sy(first) .. sy(last) + 1)
    src_h = GEOMS["scale15"][1]
    for _, lw, lh, ndw, r, _ in c["scale15"]:                                                # (a level with a longer span would go to k_resize)
        sy = [int(np.floor(np.float32((dy + 0.5) * (1.0 / (lh / src_h)) - 0.5))) for dy in range(lh)]
        assert max(sy[min(t + 8, lh) - 1] + 2 - sy[t] for t in range(0, lh, 8)) == 12
        src_h = lh
    assert c["scale15"][0][3] > 64 and c["scale15"][0][4]                                    # level 1: a full tile and a packed one


_images, _refs = {}, {}


def _image(synth, name, i):
    w, h = GEOMS[name][:2]
    if (name, i) not in _images:
        seed = 700 + 131 * sorted(GEOMS).index(name) + i
        if name == "scale15" and i % 2:                        # black / white frames: horizontal sums with every high bit set, in the registers
            import structured_images                           # that the packing of a destination dword must not pick up
            _images[(name, i)] = structured_images.gen("binary", w, h, seed)
        else:
            _images[(name, i)] = synth.gen_image(w, h, seed)
    return _images[(name, i)]


def _ref(oracle, synth, name, i):
    """(levels, n, kps bytes, desc, mono) of frame i from the oracle, computed once."""
    if (name, i) not in _refs:
        _, _, nl, sf, _ = GEOMS[name]
        ref = oracle.Extractor(200, sf, nl, 20, 7)
        n, kps, desc, mono = ref(_image(synth, name, i), (0, 0))
        _refs[(name, i)] = ([ref.level_image(l).copy() for l in range(nl)], n, kps.tobytes(), desc.copy(), mono)
    return _refs[(name, i)]


class _DeviceFrames:
    """The frames of a batch in one device buffer, in permuted slots with a gap between them, under a pitch wider than the image."""

    def __init__(self, pkg, imgs):
        h, w = imgs[0].shape
        self.w, self.h, self.stride = w, h, (w + 63) // 64 * 64 + 64
        slot = self.stride * h + 192
        n = len(imgs)
        order = [(7 * i + 3) % n for i in range(n)] if n % 7 else list(range(n))[::-1]
        assert sorted(order) == list(range(n))
        self.buf = pkg.DeviceBuffer(slot * n)
        pad = np.full((h, self.stride), 255, np.uint8)
        for i, im in enumerate(imgs):
            pad[:, :w] = im
            self.buf.upload(pad, offset=order[i] * slot)
        self.ptrs = (C.c_void_p * n)(*[self.buf.ptr + order[i] * slot for i in range(n)])


def _compare(ex, res, oracle, synth, name, frames, tag):
    nl = GEOMS[name][2]
    assert len(res) == frames
    for i in range(frames):
        levels, n, kps, desc, mono = _ref(oracle, synth, name, i)
        for l in range(0 if tag == "host" else 1, nl):                                       # (level 0 of a device-resident input is the caller's buffer)
            assert ex.level_image(l, i).tobytes() == levels[l].tobytes(), (name, tag, "frame %d level %d" % (i, l))
        m, k, d = res[i]
        assert len(k) == n and m == mono, (name, tag, i)
        assert k.tobytes() == kps and np.array_equal(d, desc), (name, tag, i)


def _run_device(pkg, oracle, synth, name, frames, max_batch=None, graph=False):
    w, h, nl, sf, _ = GEOMS[name]
    imgs = [_image(synth, name, i) for i in range(frames)]
    ex = pkg.ORBextractor(200, sf, nl, 20, 7, max_size=(w, h), max_batch=max_batch or frames)
    try:
        dev = _DeviceFrames(pkg, imgs)
        ex.enqueue_device(dev.ptrs, w, h, dev.stride, np.zeros(2 * frames, np.int32))
        ex.sync()
        res = ex.fetch_all()
        _compare(ex, res, oracle, synth, name, frames, "device")
        if graph:
            L = pkg.lib()
            assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
            ex.enqueue_device(dev.ptrs, w, h, dev.stride, np.zeros(2 * frames, np.int32))
            assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            ex.sync()
            again = ex.fetch_all()
            for (m0, k0, d0), (m1, k1, d1) in zip(res, again):
                assert m0 == m1 and k0.tobytes() == k1.tobytes() and np.array_equal(d0, d1)
            _compare(ex, again, oracle, synth, name, frames, "replay")
    finally:
        ex.close()


def _run_host(pkg, oracle, synth, name, frames):
    w, h, nl, sf, _ = GEOMS[name]
    imgs = [_image(synth, name, i) for i in range(frames)]
    ex = pkg.ORBextractor(200, sf, nl, 20, 7, max_size=(w, h), max_batch=frames)
    try:
        res = ex.extract_batch(imgs, [(0, 0)] * frames) if frames > 1 else [ex(imgs[0], (0, 0))]
        _compare(ex, res, oracle, synth, name, frames, "host")
    finally:
        ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMS))
def test_pyramids_of_a_batch_bit_exact(pkg, oracle, synth, name):
    _run_device(pkg, oracle, synth, name, GEOMS[name][4])


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [1, 63, 64, 129])                                         # pack - 1, pack, 2 * pack + 1 (pack + 1: above) and a batch of one
def test_batch_sizes_around_the_largest_pack(pkg, oracle, synth, frames):
    _run_device(pkg, oracle, synth, LARGEST_PACK, frames)


@pytest.mark.gpu
def test_batch_smaller_than_the_handle(pkg, oracle, synth):
    """Five frames on a handle made for sixteen: the last packed wave has lanes whose frame is past the batch but inside the allocation."""
    _run_device(pkg, oracle, synth, "pack12", 5, max_batch=16)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pack12", "pack2", "pack64"])
def test_host_images_bit_exact(pkg, oracle, synth, name):
    _run_host(pkg, oracle, synth, name, min(GEOMS[name][4], 13))


@pytest.mark.gpu
def test_single_frame_call(pkg, oracle, synth):
    _run_host(pkg, oracle, synth, "pack2", 1)


@pytest.mark.gpu
def test_graph_replay_equals_eager(pkg, oracle, synth):
    _run_device(pkg, oracle, synth, "pack2", 5, graph=True)


def _ab_child():
    """In a process on the -DORBX_AB library: the kept parent kernel (k_resize2p) and the unpacked task lists (a frame per wave
    everywhere: the form of a handle whose slabs are too large for 32-bit lane offsets) give the same bytes."""
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    pkg = importlib.import_module("orb-slam3_amd")
    synth = importlib.import_module("orb-slam3_amd.synth")
    import orbref
    orbref.lib()
    for env in ({"ORBX_RESIZE_V2P": "1"}, {"ORBX_RESIZE_NOPACK": "1"}):
        os.environ.update(env)
        try:
            for name in ("pack12", "pack2", "scale15", "wide"):
                _run_device(pkg, orbref, synth, name, GEOMS[name][4])
            _run_host(pkg, orbref, synth, "pack12", 3)
        finally:
            for k in env:
                del os.environ[k]
    print("ab child ok")


@pytest.mark.gpu
def test_parent_kernel_and_unpacked_lists_on_the_ab_library():
    assert os.path.exists(AB_LIB), "build it: make -C orb-slam3_amd/csrc"
    env = dict(os.environ, ORB_LIB=AB_LIB)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "ab-child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ab child ok" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])


if __name__ == "__main__" and sys.argv[1:] == ["ab-child"]:
    _ab_child()
