"""k_fast4's tile staging, scalar prologue and fused suppression + store on the strip shapes where they can go wrong.

The kernel fetches a fixed-pitch tile as a linear list of 16-byte chunks, 64 per wave-instruction, the last instruction of a tile moved
back so that it ends at the tile's end; a wave takes its cell record before the barrier (an idle wave of a short strip the last cell's);
the suppression loop stores the keypoints it finds.  What decides which of these paths run is the SHAPE of a strip -- its number of
cells, its number of rows -- and the level's width against its pitch, so the frames below are small ones chosen for their shapes:
`test_geometries_contain_the_shapes` derives the shapes from the reference's cell arithmetic (ORBextractor.cc:1083-1100) and fails if
a geometry stops containing the shape it is listed for.  Every frame is bit-exact against the CPU oracle: key points (all fields,
the response among them), descriptors, and per level the FAST candidates in order."""
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_LIB = os.path.join(ROOT, "orb-slam3_amd", "liborbslam3_amd_ab.so")

# name -> (w, h, nfeatures, nlevels, ini_th, min_th, kind, frames)
GEOMS = {
    # one level of 210 x 134: two cell rows of 57 tile rows (> 48: three fetches per wave), five cells a row = strips of 4 and 1;
    # 210 is no multiple of 16 and the level-0 pitch is 256: the clamped right edge
    "tall": (210, 134, 300, 1, 20, 7, "textured", 1),
    # one level of 560 x 1083: 30 cell rows of 36, the last one cut to 7 tile rows (fewer than the 8 of a register-staged pass; FAST on a
    # single image row)
    "short7": (560, 1083, 1000, 1, 20, 7, "textured", 1),
    # one level of 600 x 1153: the last of 32 cell rows is cut to 5 tile rows = 55 chunks, fewer than one wave-instruction; its cells
    # have no pixel to test
    "short5": (600, 1153, 1000, 1, 20, 7, "textured", 1),
    # eight levels of 421 x 307, five frames (no multiple of 8): strips of 1, 2, 3 and 4 cells, odd widths on every level
    "pyramid": (421, 307, 500, 8, 20, 7, "textured", 5),
    # thresholds 40 / 5 on a low-contrast frame: most cells find nothing at 40 and run again at 5 (nothing may have been stored by then)
    "retry": (421, 307, 500, 8, 40, 5, "lowcontrast", 3),
}


def strips_of(w, h, nlevels, scale_factor=1.2):
    """[(level, cells, tile rows, level width)] from the reference's cell grid; a strip is a run of up to four cells of one cell row."""
    out = []
    sf = np.float32(1.0)
    for l in range(nlevels):
        if l:
            sf = np.float32(sf * np.float32(scale_factor))
        inv = np.float32(1.0) / sf
        lw, lh = int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))
        min_b, max_bx, max_by = 16, lw - 16, lh - 16
        width, height = float(max_bx - min_b), float(max_by - min_b)
        ncols, nrows = int(width / 35), int(height / 35)
        wcell, hcell = math.ceil(width / ncols), math.ceil(height / nrows)
        for i in range(nrows):
            ini_y = min_b + i * hcell
            if ini_y >= max_by - 3:
                continue
            rows = min(ini_y + hcell + 6, max_by) - ini_y
            ncell = sum(1 for j in range(ncols) if min_b + j * wcell < max_bx - 6)
            while ncell > 0:
                out.append((l, min(ncell, 4), rows, lw))
                ncell -= 4
    return out


def test_geometries_contain_the_shapes():
    s = {k: strips_of(g[0], g[1], g[3]) for k, g in GEOMS.items()}
    assert {n for _, n, _, _ in s["tall"]} == {1, 4} and all(r > 48 for _, _, r, _ in s["tall"])
    assert len(s["tall"]) == 4                                                                       # two cell rows
    assert GEOMS["tall"][0] % 16 != 0 and -(-GEOMS["tall"][0] // 64) * 64 > GEOMS["tall"][0]         # level-0 pitch (a multiple of 64) > width
    assert min(r for _, _, r, _ in s["short7"]) == 7                                                 # < 8 rows, one row of pixels to test
    assert min(r for _, _, r, _ in s["short5"]) == 5 and 5 * (176 // 16) < 64                        # < 64 chunks, no pixel to test
    assert {n for _, n, _, _ in s["pyramid"]} == {1, 2, 3, 4}
    assert any(lw % 16 != 0 for _, _, _, lw in s["pyramid"])
    for k in ("tall", "short7", "short5"):
        assert GEOMS[k][3] == 1                                                                      # single-level extractors
    assert GEOMS["pyramid"][7] % 8 != 0 and GEOMS["retry"][7] % 8 != 0
    assert GEOMS["retry"][4] > GEOMS["retry"][5]                                                     # the retry pass exists


def _check_batch(pkg, oracle, synth, name, seed0=100):
    w, h, nf, nl, ini, mn, kind, frames = GEOMS[name]
    imgs = [synth.gen_image(w, h, seed0 + i, kind) for i in range(frames)]
    ref = oracle.Extractor(nf, 1.2, nl, ini, mn)
    ex = pkg.ORBextractor(nf, 1.2, nl, ini, mn, max_size=(w, h), max_batch=frames)
    try:
        res = ex.extract_batch(imgs, [(0, 0)] * frames) if frames > 1 else [ex(imgs[0], (0, 0))]
        total = 0
        for i, (img, (mono, kps, desc)) in enumerate(zip(imgs, res)):
            n_ref, kps_ref, desc_ref, mono_ref = ref(img, (0, 0))
            assert len(kps) == n_ref and mono == mono_ref, (name, i)
            assert kps.tobytes() == kps_ref.tobytes(), (name, i)                                     # all fields (response included), same order
            assert np.array_equal(desc, desc_ref), (name, i)
            total += n_ref
        # the FAST candidates themselves, in order (the last frame of the batch is the one the oracle holds)
        one = ex(imgs[-1], (0, 0))
        for l in range(nl):
            assert np.array_equal(ex.level_candidates(l), ref.level_candidates(l)), (name, "FAST candidates level %d" % l)
        assert one[1].tobytes() == res[-1][1].tobytes()
        return total
    finally:
        ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMS))
def test_fast_staging_bit_exact(pkg, oracle, synth, name):
    assert _check_batch(pkg, oracle, synth, name) > 0


def test_retry_frames_need_the_retry(oracle, synth):
    """The "retry" frames lose key points without the second pass: the pass is taken."""
    w, h, nf, nl, ini, mn, kind, _ = GEOMS["retry"]
    img = synth.gen_image(w, h, 100, kind)
    assert oracle.Extractor(nf, 1.2, nl, ini, mn)(img, (0, 0))[0] > oracle.Extractor(nf, 1.2, nl, ini, ini)(img, (0, 0))[0]


def _ab_child():
    """In a process on the -DORBX_AB library: a queue of 64 entries per cell on corner-dense frames, so that most cells overflow and are
    redone by k_fast_fix (an overflowing cell must leave its slots and its count alone); the per-strip pitch form of the kernel on every
    group; the kept parent kernel (k_fast4p) as a cross-check of the switch."""
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    pkg = importlib.import_module("orb-slam3_amd")
    synth = importlib.import_module("orb-slam3_amd.synth")
    import orbref
    orbref.lib()
    for env in ({"ORBX_FAST_QCAP": "64"}, {"ORBX_FAST_PITCH0": "1"}, {"ORBX_FAST_PITCH0": "1", "ORBX_FAST_QCAP": "64"}, {"ORBX_FAST_V4P": "1"}):
        os.environ.update(env)
        try:
            for name in ("pyramid", "tall", "short5"):
                _check_batch(pkg, orbref, synth, name, seed0=300)
        finally:
            for k in env:
                del os.environ[k]
    print("ab child ok")


@pytest.mark.gpu
def test_overflowing_cells_and_per_strip_pitch_on_the_ab_library():
    assert os.path.exists(AB_LIB), "build it: make -C orb-slam3_amd/csrc"
    env = dict(os.environ, ORB_LIB=AB_LIB)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "ab-child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ab child ok" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])


if __name__ == "__main__" and sys.argv[1:] == ["ab-child"]:
    _ab_child()
