"""k_blur3's byte fix-up.  Pass 2 of the kernel starts both products from zero, so every byte it parks in its LDS output tile is the
blurred byte minus 0x81 modulo 256; the 0x81 goes back on, four bytes to a dword and without a carry between them, where a thread
reads its 16-byte piece of that tile for the global store.  Two frames of geometry `tall` (256 x 442, three levels) are built for it:

  (a)  16 x 16-px flat blocks of value (16 by + bx) mod 256: every value 0..255 has a flat interior that blurs to itself, and
       horizontal neighbours differ by one, across 0x7E / 0x7F / 0x80 / 0x81 as well;
  (b)  the same blocks with value (37 v + 0xFF) mod 256: neighbours are 37 apart, so the blurred edges between them run through
       dwords whose bytes lie on both sides of 0x80 (958 of them on level 0, against 12 in (a)), next to flat dwords of 0xFF, 0x00
       and 0x80.

Every level of every frame must equal gauss7_exact (tests/blur_cases.py) of the oracle's level byte for byte: as a batch on the
product library in both forms of the kernel (the batch sizes tests/test_gpu_blur_tiles.py uses to reach the walk), as a single-frame
call and as a replayed graph; and, in a child process on the A/B library (this file run as a script), under ORBX_BLUR_ROWMAJOR in
both forms.  The same child holds k_blur3p (ORBX_BLUR_V3P, the kernel as it was before the fix-up) to k_blur3 byte for byte on
geometry `fold1` with the frames of blur_cases.image."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_LIB = os.path.join(ROOT, "orb-slam3_amd", "liborbslam3_amd_ab.so")
if __name__ == "__main__":                                      # the child process: what conftest.py does for pytest
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

import blur_cases as bc
from blur_cases import GEOMS, gauss7_exact
from test_gpu_blur_tiles import DeviceFrames, all_images, make

NAME = "tall"
_frames, _expected = {}, {}


def frame(i):
    """Frame (a) for i == 0, frame (b) for i == 1."""
    if i not in _frames:
        w, h = GEOMS[NAME][:2]
        by, bx = np.mgrid[0:h, 0:w] // 16
        v = (16 * by + bx) % 256
        img = (v if i == 0 else (37 * v + 0xFF) % 256).astype(np.uint8)
        img.setflags(write=False)
        _frames[i] = img
    return _frames[i]


def expected(oracle, i):
    """gauss7_exact of every level of frame i as the oracle builds it, computed once."""
    if i not in _expected:
        _, _, nl, sf, _ = GEOMS[NAME]
        ref = oracle.Extractor(bc.NFEATURES, sf, nl, bc.INI_TH, bc.MIN_TH)
        ref(frame(i), (0, 0))
        _expected[i] = [gauss7_exact(ref.level_image(l)) for l in range(nl)]
    return _expected[i]


def test_the_frames_hold_what_they_are_built_for():
    a, b = frame(0), frame(1)
    assert a.shape == b.shape == (442, 256)
    for img in (a, b):
        assert np.array_equal(np.unique(img[:256]), np.arange(256))
        blurred = gauss7_exact(img)
        for by in range(16):                                                                 # every value has an interior that blurs to itself:
            for bx in range(16):                                                             # whole dwords of it, 0x00, 0x7F, 0x80 and 0xFF among them
                box = slice(16 * by + 3, 16 * by + 13), slice(16 * bx + 4, 16 * bx + 12)
                assert np.array_equal(blurred[box], img[box])
        d = blurred.reshape(442, 64, 4)                                                      # and dwords whose bytes lie on both sides of 0x80
        assert np.any((d.max(axis=2) >= 0x80) & (d.min(axis=2) < 0x80))
    assert a[7 * 16 + 8, 14 * 16] == 0x7E and a[7 * 16 + 8, 15 * 16] == 0x7F and a[8 * 16 + 8, 0] == 0x80 and a[8 * 16 + 8, 16] == 0x81
    assert np.array_equal(b, ((37 * a.astype(int) + 0xFF) % 256).astype(np.uint8))
    assert b[0, 0] == 0xFF and b[10 * 16 + 8, 13 * 16] == 0x00 and 0x80 in b                    # v = 0 -> 0xFF, v = 173 -> 0x00 (37 * 173 = 25 * 256 + 1)


def test_the_switch_is_in_the_ab_library_only():
    prod = open(os.path.join(ROOT, "orb-slam3_amd", "liborbslam3_amd.so"), "rb").read()
    ab = open(AB_LIB, "rb").read()
    for n in (b"ORBX_BLUR_V3P", b"8k_blur3pE"):
        assert n not in prod and n in ab, n
    assert b"7k_blur3E" in prod and b"7k_blur3E" in ab


def check(ex, oracle, which, form, tag, frames=None):
    assert ex.blur_form() == form, (tag, ex.blur_form())
    nl = GEOMS[NAME][2]
    for f in (range(len(which)) if frames is None else frames):
        want = expected(oracle, which[f])
        for l in range(nl):
            got = ex.level_image(l, f, blurred=True)
            if got.tobytes() != want[l].tobytes():
                bad = np.argwhere(got != want[l])
                y, x = (int(v) for v in bad[0])
                raise AssertionError((tag, "frame %d (image %s) level %d: %d bytes differ, first (y, x) = (%d, %d): got 0x%02X, want 0x%02X"
                                      % (f, "ab"[which[f]], l, len(bad), y, x, int(got[y, x]), int(want[l][y, x]))))


def run_device(pkg, oracle, which, form, tag, graph=False, counts=None):
    """The frames of `which` from a device buffer; counts: batch sizes to enqueue in turn on the one handle with the form each must take."""
    w, h = GEOMS[NAME][:2]
    ex = make(pkg, NAME, len(which))
    try:
        dev = DeviceFrames(pkg, [frame(i) for i in which])
        for n, fm in (counts or [(len(which), form)]):
            ptrs = (C.c_void_p * n)(*dev.ptrs[:n])
            lap = np.zeros(2 * n, np.int32)
            ex.enqueue_device(ptrs, w, h, dev.stride, lap)
            ex.sync()
            check(ex, oracle, which[:n], fm, "%s, %d frames" % (tag, n))
        if graph:
            L = pkg.lib()
            assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
            ex.enqueue_device(ptrs, w, h, dev.stride, lap)
            assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
            for _ in range(2):
                assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
                ex.sync()
                check(ex, oracle, which, form, tag + ", replay")
    finally:
        ex.close()


def run_host(pkg, oracle, which, form, tag):
    ex = make(pkg, NAME, len(which))
    try:
        imgs = [frame(i) for i in which]
        if len(imgs) > 1:
            ex.extract_batch(imgs, [(0, 0)] * len(imgs))
        else:
            ex(imgs[0], (0, 0))
        check(ex, oracle, which, form, tag)
    finally:
        ex.close()


@pytest.mark.gpu
def test_batch_in_both_forms(pkg, oracle):
    """frames x walk tasks >= 2048 is the walk, one frame fewer the one-tile form: the same handle and device frames, (a) and (b) in turn."""
    tasks = bc.walk_tasks(bc.level_sizes(oracle, NAME))
    frames = (2048 + tasks - 1) // tasks
    assert (frames - 1) * tasks < 2048 <= frames * tasks
    run_device(pkg, oracle, [i % 2 for i in range(frames)], None, "device batch", counts=[(frames - 1, 0), (frames, 1)])


@pytest.mark.gpu
def test_small_batch(pkg, oracle):
    run_device(pkg, oracle, [0, 1, 1, 0, 1], 0, "device batch")
    run_host(pkg, oracle, [1, 0, 0], 0, "host batch")


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 1])
def test_single_frame_call(pkg, oracle, i):
    run_host(pkg, oracle, [i], 0, "single frame")
    run_device(pkg, oracle, [i], 0, "device batch of one")


@pytest.mark.gpu
def test_replayed_graph(pkg, oracle):
    run_device(pkg, oracle, [0, 1], 0, "graph", graph=True)


@pytest.mark.gpu
def test_row_major_and_the_parent_kernel_on_the_ab_library():
    assert os.path.exists(AB_LIB), "build it: make -C orb-slam3_amd/csrc"
    env = dict(os.environ, ORB_LIB=AB_LIB)
    for k in ("ORBX_BLUR_ROWMAJOR", "ORBX_BLUR_WALK", "ORBX_BLUR_V3P"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "blur bytes child ok" in p.stdout


def _child():
    """On the A/B library: the row-major branch of the store address in both forms with frames (a) and (b), then k_blur3p against
    k_blur3 on fold1.  The switches are read when a handle is created."""
    import importlib
    pkg = importlib.import_module("orb-slam3_amd")
    synth = importlib.import_module("orb-slam3_amd.synth")
    import orbref as oracle
    oracle.lib()
    assert os.path.samefile(pkg.LIB_PATH, AB_LIB)

    def setenv(**kw):
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    for walk, form in ((None, 0), ("1", 1)):
        setenv(ORBX_BLUR_ROWMAJOR="1", ORBX_BLUR_WALK=walk)
        run_device(pkg, oracle, [0, 1, 1], form, "row-major device batch, form %d" % form)
        run_host(pkg, oracle, [1, 0], form, "row-major host batch, form %d" % form)
        run_host(pkg, oracle, [1], form, "row-major single frame, form %d" % form)
    setenv(ORBX_BLUR_ROWMAJOR=None, ORBX_BLUR_WALK=None)

    name = "fold1"
    w, h, nl = GEOMS[name][:3]
    imgs = [bc.image(synth, name, i) for i in all_images(name)]
    for walk in ("0", "1"):
        got = {}
        for v3p in (None, "1"):
            setenv(ORBX_BLUR_WALK=walk, ORBX_BLUR_V3P=v3p)
            ex = make(pkg, name, len(imgs))
            try:
                ex.extract_batch(imgs, [(0, 0)] * len(imgs))
                assert ex.blur_form() == int(walk)
                got[v3p] = [[ex.level_image(l, f, blurred=True) for l in range(nl)] for f in range(len(imgs))]
                own = [[ex.level_image(l, f) for l in range(nl)] for f in range(len(imgs))]
            finally:
                ex.close()
            for f in range(len(imgs)):
                for l in range(nl):
                    assert got[v3p][f][l].tobytes() == gauss7_exact(own[f][l]).tobytes(), ("k_blur3p" if v3p else "k_blur3", walk, f, l)
        for f in range(len(imgs)):
            for l in range(nl):
                assert got[None][f][l].tobytes() == got["1"][f][l].tobytes(), ("k_blur3p differs from k_blur3", walk, f, l)
    setenv(ORBX_BLUR_WALK=None, ORBX_BLUR_V3P=None)
    print("blur bytes child ok")


if __name__ == "__main__":
    _child()
