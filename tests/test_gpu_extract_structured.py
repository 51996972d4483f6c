"""GPU parity on saturated, periodic and tie-heavy images (tests/structured_images.py): the HIP extractor against the CPU oracle, stage
by stage and bit for bit, where the value-noise frames of the rest of the suite never go -- FAST cells over the wave's survivor queue
(k_fast_fix: levels 1-3 of `binary`, level 0 as well of the dense checker, structured_images.DENSE), every 16-bit lane at 0 / 255,
plateaus of equal score, thousands of candidates with one response in the quadtree,
orientation patches with m01 == m10 == 0, all-255 windows next to all-0 windows in the blur and the resize.  Any device-side error word
(slotCap, nodeCap, the iteration guard) makes the call raise OrbError and the test fail.  What these images provoke is asserted on the
oracle alone in tests/test_oracle_structured_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import structured_images as si
from test_gpu_extract import _check
from structured_images import DENSE, MB, MBF, PAIRS, STRUCTURED, case_id as _id, shifted_pair

pytestmark = pytest.mark.gpu


class _Gen:
    """What _check asks of `synth`: kind is (name, parameters) of structured_images.gen."""

    @staticmethod
    def gen_image(w, h, seed, kind):
        return si.gen(kind[0], w, h, seed, **kind[1])


def _same(got, want):
    mono, kps, desc = got
    n_ref, kps_ref, desc_ref, mono_ref = want
    return len(kps) == n_ref and mono == mono_ref and kps.tobytes() == kps_ref.tobytes() and np.array_equal(desc, desc_ref)


@pytest.mark.parametrize("lap", [(0, 1000), (0, 0)], ids=["lap0-1000", "lap0-0"])
@pytest.mark.parametrize("kind,params", STRUCTURED, ids=_id)
def test_every_kind_bit_exact(pkg, oracle, kind, params, lap):
    n = _check(pkg, oracle, _Gen, 752, 480, 1000, 7, lap, (kind, params))
    if not (kind == "halves" and "constant" in params.values()):
        assert n >= 300


SHAPES = [(421, 307, 500, 1.2, 8),        # odd sizes, ragged last cells
          (1241, 376, 1000, 1.2, 8),      # KITTI
          (752, 480, 1000, 1.5, 5),
          (752, 480, 1000, 1.1, 12)]


@pytest.mark.parametrize("w,h,nf,sf,nl", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind,params", [("binary", {}), ("dots", {"pitch": 8}), ("clipped", {"gain": 4.0}), DENSE], ids=_id)
def test_sizes_and_pyramids(pkg, oracle, kind, params, w, h, nf, sf, nl):
    assert _check(pkg, oracle, _Gen, w, h, nf, 13, (0, 1000), (kind, params), scale_factor=sf, nlevels=nl) >= nf // 2


@pytest.mark.parametrize("kind,params", [("binary", {}), ("dots", {"pitch": 8}), DENSE], ids=_id)
def test_5000_features(pkg, oracle, kind, params):
    # more than 512 nodes per level: four fused quadtree iterations, the 1024-thread quadtree
    assert _check(pkg, oracle, _Gen, 752, 480, 5000, 17, (0, 1000), (kind, params)) >= 2500


def test_full_hd_binary_4000(pkg, oracle):
    assert _check(pkg, oracle, _Gen, 1920, 1080, 4000, 19, (0, 0), ("binary", {}), stages=False) >= 3900


def test_full_hd_dense_4000(pkg, oracle):
    # the same size with nearly every level-0 cell over its queue, per level
    assert _check(pkg, oracle, _Gen, 1920, 1080, 4000, 19, (0, 1000), DENSE) >= 3900


@pytest.mark.parametrize("ini,mn", [(20, 7), (40, 2), (7, 7), (254, 7)])
@pytest.mark.parametrize("kind,params", [("binary", {}), DENSE], ids=_id)
def test_saturated_thresholds(pkg, oracle, kind, params, ini, mn):
    # at 254 only 0 <-> 255 steps are corners: the packed threshold and the sign-bit test at their extreme
    assert _check(pkg, oracle, _Gen, 752, 480, 1000, 23, (0, 1000), (kind, params), ini_th=ini, min_th=mn) >= 900


def test_too_small_structured_frame_is_refused_by_both(pkg, oracle):
    img = si.gen("binary", 120, 100, 1)
    assert oracle.Extractor(1000)(img)[0] < 0
    ex = pkg.ORBextractor(1000, max_size=(752, 480), max_batch=1)
    with pytest.raises(pkg.OrbError):
        ex(img)
    ex.close()


BATCH_EXTRA = [("blocks", {"block": 2}), ("blocks", {"block": 6}), ("dots", {"pitch": 11}), ("holes", {"pitch": 7}),
               ("checker", {"period": 5, "contrast": 255}), ("clipped", {"gain": 8.0})]


def test_batch_of_every_kind_side_by_side(pkg, oracle, synth):
    imgs = [si.gen(k, 752, 480, 30 + i, **p) for i, (k, p) in enumerate(STRUCTURED + BATCH_EXTRA)]
    imgs += [synth.gen_image(752, 480, 60 + i) for i in range(3)] + [synth.gen_image(752, 480, 0, "constant")]
    assert len(imgs) >= 24
    laps = [(0, 1000) if i % 2 else (0, 0) for i in range(len(imgs))]
    ex = pkg.ORBextractor(1000, max_size=(752, 480), max_batch=len(imgs))
    res = ex.extract_batch(imgs, laps)
    ref = oracle.Extractor(1000)
    for i, (img, lap) in enumerate(zip(imgs, laps)):
        assert _same(res[i], ref(img, lap)), i
        if i in (0, 3, STRUCTURED.index(DENSE), len(imgs) - 2):     # a binary, a dots, the dense and a textured frame of the batch, stage by stage
            for l in range(8):
                assert np.array_equal(ex.level_image(l, frame=i), ref.level_image(l)), (i, l)
                assert np.array_equal(ex.level_candidates(l, frame=i), ref.level_candidates(l)), (i, l)
                assert np.array_equal(ex.level_selected(l, frame=i), ref.level_keypoints(l)[0]), (i, l)
    ex.close()


def test_batch_of_48_saturated_frames(pkg, oracle):
    # binary and dense-checker frames in turn: most cells of levels 1-3 of every frame, and of level 0 of every other one, on the overflow
    # list (some 19 000 entries for k_fast_fix), k_blur3 in its walking form
    imgs = [si.gen(DENSE[0], 752, 480, 100 + i, **DENSE[1]) if i % 2 else si.gen("binary", 752, 480, 100 + i) for i in range(48)]
    ex = pkg.ORBextractor(1000, max_size=(752, 480), max_batch=len(imgs))
    res = ex.extract_batch(imgs, [(0, 0)] * len(imgs))
    ref = oracle.Extractor(1000)
    for i, img in enumerate(imgs):
        assert _same(res[i], ref(img, (0, 0))), i
    ex.close()


def _upload(pkg, imgs, stride, shift=0):
    h, w = imgs[0].shape
    dev = pkg.DeviceBuffer(len(imgs) * stride * h + 64)
    _refill(dev, imgs, stride, shift)
    arr = (C.c_void_p * len(imgs))(*[dev.ptr + shift + i * stride * h for i in range(len(imgs))])
    return dev, arr


def _refill(dev, imgs, stride, shift=0):
    h, w = imgs[0].shape
    for i, im in enumerate(imgs):
        pad = np.zeros((h, stride), np.uint8); pad[:, :w] = im
        dev.upload(pad, offset=shift + i * stride * h)


def test_graph_replay_resets_the_overflow_list(pkg, oracle, synth):
    """A batch of a binary, a dense-checker, a dots and a textured frame captured into a HIP graph and replayed: whatever resets the
    overflow list and its counter has to be part of the captured work.  The third replay runs on the same buffers with the frames
    rotated, so that the frames with most cells on the list (levels 0-2 of the dense checker, 1-3 of binary) become frames with none:
    a stale list or count would show."""
    w, h, n = 752, 480, 4
    imgs = [si.gen("binary", w, h, 41), si.gen(DENSE[0], w, h, 44, **DENSE[1]), si.gen("dots", w, h, 42, pitch=8), synth.gen_image(w, h, 43)]
    rot = imgs[2:] + imgs[:2]
    stride = 768
    dev, arr = _upload(pkg, imgs, stride)
    L = pkg.lib()
    ex = pkg.ORBextractor(1000, max_size=(w, h), max_batch=n)
    ref = oracle.Extractor(1000)
    want = [ref(im, (0, 0)) for im in imgs]
    ex.enqueue_device(arr, w, h, stride); ex.sync()
    eager = [ex.fetch(i) for i in range(n)]
    for i in range(n):
        assert _same(eager[i], want[i]), i
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    ex.enqueue_device(arr, w, h, stride)
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    for rep, frames in enumerate((imgs, imgs, rot, imgs)):
        _refill(dev, frames, stride)
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        for i in range(n):
            j = (i + 2) % n if frames is rot else i
            got = ex.fetch(i)
            assert _same(got, want[j]), (rep, i)
            assert got[1].tobytes() == eager[j][1].tobytes() and np.array_equal(got[2], eager[j][2]), (rep, i)
    ex.close()


@pytest.mark.parametrize("w,h,stride,shift", [(421, 307, 421, 0), (421, 307, 430, 4), (752, 480, 755, 0), (752, 480, 758, 3)])
def test_device_resident_binary_with_odd_pitch(pkg, oracle, w, h, stride, shift):
    imgs = [si.gen("binary", w, h, 80), si.gen("binary", w, h, 81), si.gen(DENSE[0], w, h, 82, **DENSE[1])]
    dev, arr = _upload(pkg, imgs, stride, shift)
    ex = pkg.ORBextractor(800, max_size=(w, h), max_batch=3)
    ex.enqueue_device(arr, w, h, stride)
    ex.sync()
    ref = oracle.Extractor(800)
    for i in range(3):
        assert _same(ex.fetch(i), ref(imgs[i], (0, 0))), i
    ex.close()


# ---- downstream: what only such images make ----
@pytest.mark.parametrize("kind,d,params", PAIRS, ids=["dots", "binary"])
def test_stereo_matches_on_structured_pairs(pkg, oracle, kind, d, params):
    # a lattice: Hamming ties all along the row band, SAD minima at the window's edge (Frame.cc:1210); binary: every SAD at its extreme
    # (that the pairs give ties and mostly rejections: tests/test_oracle_structured_cpu.py::test_stereo_pairs_provoke_ties_and_rejections)
    l, r = shifted_pair(kind, 752, 480, 51, d, **params)
    exl = pkg.ORBextractor(1200, max_size=(752, 480)); exr = pkg.ORBextractor(1200, max_size=(752, 480))
    _, kl, dl = exl(l, (0, 0)); _, kr, dr = exr(r, (0, 0))
    ol, orr = oracle.Extractor(1200), oracle.Extractor(1200)
    assert _same((len(kl), kl, dl), ol(l, (0, 0))) and _same((len(kr), kr, dr), orr(r, (0, 0)))
    OM = oracle._oracle_matcher_class()()
    m = pkg.ORBmatcher(0.7)
    n_gpu, ur_g, dp_g = m.ComputeStereoMatches(exl, exr, kl, dl, kr, dr, MB, MBF)
    n_ref, ur_r, dp_r = OM.ComputeStereoMatches(ol, orr, kl, dl, kr, dr, MB, MBF)
    assert n_gpu == n_ref and n_ref > 100
    assert ur_g.tobytes() == ur_r.tobytes() and dp_g.tobytes() == dp_r.tobytes()
    exl.close(); exr.close(); m.close()


def test_stereo_batch_on_structured_pairs(pkg, oracle):
    W, H, NF = 752, 480, 1200
    pairs = [shifted_pair(k, W, H, 51, d, **p) for k, d, p in PAIRS]
    P = len(pairs)
    imgs = [p[0] for p in pairs] + [p[1] for p in pairs]                    # frames [0,P) left, [P,2P) right
    stride = 768
    dev, arr = _upload(pkg, imgs, stride)
    L = pkg.lib()
    ex = pkg.ORBextractor(NF, max_size=(W, H), max_batch=2 * P)
    mt = pkg.ORBmatcher(0.6)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    cap = ex.cap
    ex.enqueue_device(arr, W, H, stride, np.zeros(4 * P, np.int32))
    r = ex.result_device()
    ur = pkg.DeviceBuffer(P * cap * 4); dp = pkg.DeviceBuffer(P * cap * 4); sad = pkg.DeviceBuffer(P * cap * 4); kept = pkg.DeviceBuffer(P * 4)
    assert L.orbm_stereo_batch_async(mt.h, ex.h, 0, P, P, r["kps"], r["desc"], r["counts"], cap, MB, MBF, ur.ptr, dp.ptr, sad.ptr, kept.ptr) == 0, L.orbm_last_error()
    ex.sync()
    res = ex.fetch_all()
    ur_h = ur.download(np.float32, P * cap).reshape(P, cap); dp_h = dp.download(np.float32, P * cap).reshape(P, cap)
    kept_h = kept.download(np.int32, P)
    OM = oracle._oracle_matcher_class()()
    for p in range(P):
        ol, orr = oracle.Extractor(NF), oracle.Extractor(NF)
        nl, kl, dl, _ = ol(imgs[p], (0, 0)); nr, kr, dr, _ = orr(imgs[P + p], (0, 0))
        assert res[p][1].tobytes() == kl.tobytes() and res[P + p][1].tobytes() == kr.tobytes(), p
        n_ref, ur_r, dp_r = OM.ComputeStereoMatches(ol, orr, kl, dl, kr, dr, MB, MBF)
        assert kept_h[p] == n_ref and n_ref > 100, (p, kept_h[p], n_ref)
        assert ur_h[p, :nl].tobytes() == ur_r.tobytes() and dp_h[p, :nl].tobytes() == dp_r.tobytes(), p
    ex.close(); mt.close()


def test_knn2_on_identical_descriptor_rows(pkg, oracle):
    # a dot lattice gives hundreds of identical descriptors: among equal distances the lower train index wins
    ref = oracle.Extractor(1000)
    _, _, da, _ = ref(si.gen("dots", 752, 480, 61, pitch=8), (0, 0))
    _, _, db, _ = ref(si.gen("dots", 752, 480, 62, pitch=8), (0, 0))
    assert len(da) - len(np.unique(da, axis=0)) >= 100
    m = pkg.ORBmatcher()
    for q, t in ((da, da), (da, db), (db[::-1], da)):
        idx, dist = m.knn2(q, t)
        ridx, rdist = oracle.knn2(q, t)
        assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist)
    idx, dist = m.knn2(da, da)
    assert np.all(dist[:, 0] == 0) and np.all(idx[:, 0] <= np.arange(len(da))) and np.any(idx[:, 0] < np.arange(len(da)))
    q = np.ascontiguousarray(da); t = np.ascontiguousarray(db)
    P, qs, ts = 2, len(q), max(len(q), len(t))
    qq = np.zeros((P, qs, 32), np.uint8); tt = np.zeros((P, ts, 32), np.uint8)
    qq[0] = q; qq[1] = q; tt[0, :len(q)] = q; tt[1, :len(t)] = t
    nq = np.array([len(q), len(q)], np.int32); nt = np.array([len(q), len(t)], np.int32)
    bi = np.full((P, qs, 2), -7, np.int32); bd = np.full((P, qs, 2), -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert m.L.orbm_knn2_batch(m.h, pkg.HOST, p(qq), qs, p(nq), p(tt), ts, p(nt), P, p(bi), p(bd)) == 0, m.L.orbm_last_error()
    for i, tr in enumerate((q, t)):
        ridx, rdist = oracle.knn2(q, tr)
        assert np.array_equal(bi[i], ridx) and np.array_equal(bd[i], rdist), i
    m.close()
