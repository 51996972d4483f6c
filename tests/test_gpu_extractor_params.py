"""The extractor and the batched matchers beyond the default ORB parameters (scaleFactor 1.2, nLevels 8, iniThFAST 20, minThFAST 7).

orbx_create accepts 1..12 levels, any scale factor above 1 and FAST thresholds 1..255, and the host planner (orbx_plan.h) picks
kernels and table layouts from the geometry those produce: k_resize (the general resize) wherever k_resize2's tap plan is refused,
other FAST launch-group splits, 12-entry scale tables in the matchers, 4 * nIni quadtree nodes on levels whose budget rounds to 0.
Every case is bit-exact against the CPU oracle at the same parameters, stage by stage (tests/test_gpu_extract.py::_check).  The
oracle's pyramid at these scale factors is pinned against a numpy restatement by tests/test_oracle_params_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_extract import _check
from test_gpu_local_points_batch import _Rows, _call, _check_frame, _queries
from test_gpu_stereo_batch import _stereo_bow_triangulation

pytestmark = pytest.mark.gpu

# KITTI stereo (Examples/Stereo/KITTI00-02.yaml): 1241 x 376, nFeatures 2000, Camera.fx 718.856, Camera.bf 386.1448
KITTI_W, KITTI_H, KITTI_NF = 1241, 376, 2000
KITTI_FX, KITTI_BF = 718.856, 386.1448

CASES = [
    # (w, h, nfeatures, seed, lapping, kind, scale_factor, nlevels, ini_th, min_th)
    (1241, 376, 2000, 1, (0, 0), "textured", 1.2, 8, 20, 7),        # KITTI: nIni 3 on some levels, 4 on others; odd widths everywhere
    (1241, 376, 2000, 2, (0, 0), "sparse", 1.2, 8, 12, 7),          # KITTI04-12.yaml's iniThFAST 12 on camera-like density
    (1241, 376, 2000, 3, (0, 1000), "textured", 1.2, 8, 20, 7),     # KITTI with the monocular lapping argument
    (480, 752, 1000, 4, (0, 0), "textured", 1.2, 8, 20, 7),         # portrait: nIni 1 on every level
    (752, 480, 1000, 5, (0, 0), "textured", 1.5, 5, 20, 7),         # levels 2 and 4 on k_resize, 1 and 3 on k_resize2
    (752, 480, 1000, 6, (0, 1000), "textured", 1.6, 4, 20, 7),      # every level on k_resize
    (1920, 1080, 1500, 7, (0, 0), "sparse", 2.0, 4, 20, 7),         # every level on k_resize, exact halving
    (752, 480, 1000, 8, (0, 0), "textured", 1.3, 7, 20, 7),         # other k_resize2 tap patterns
    (752, 480, 1000, 9, (0, 1000), "textured", 1.1, 12, 20, 7),     # 12 levels: the <= 15 % FAST group split, 12-entry tables
    (1920, 1080, 4000, 10, (0, 0), "sparse", 1.2, 12, 20, 7),       # 12 levels at the largest size
    (640, 480, 1000, 11, (0, 0), "textured", 1.2, 1, 20, 7),        # single level: level-0 FAST group only (the `if (first)` branch)
    (640, 480, 1000, 12, (0, 0), "lowcontrast", 1.2, 2, 20, 7),     # two levels: one later FAST group holding level 1 alone
    (752, 480, 1000, 13, (0, 0), "lowcontrast", 1.2, 8, 40, 5),     # the minTh retry in many cells (see test_retry_pass_matters)
    (752, 480, 1000, 14, (0, 0), "lowcontrast", 1.2, 8, 7, 20),     # minTh > iniTh: the retry pass is skipped
    (752, 480, 1000, 15, (0, 0), "textured", 1.2, 8, 20, 20),       # minTh == iniTh: skipped as well
    (752, 480, 1000, 16, (0, 0), "textured", 1.2, 8, 1, 1),         # nearly every pixel passes the quick test: the queue's worst case
    (752, 480, 1000, 17, (0, 1000), "textured", 1.2, 8, 255, 255),  # no corner at all: counts and mono index of an empty result
    (239, 239, 1000, 18, (0, 0), "textured", 1.2, 8, 20, 7),        # the smallest size (1.2, 8) accepts: one-cell top level
    (337, 337, 1000, 19, (0, 0), "textured", 1.5, 5, 20, 7),        # the smallest size (1.5, 5) accepts
]


def _id(c):
    return "%dx%d-nf%d-%s-seed%d-s%g-L%d-th%d_%d" % (c[0], c[1], c[2], c[5], c[3], c[6], c[7], c[8], c[9])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_extract_bit_exact_params(pkg, oracle, synth, case):
    w, h, nf, seed, lap, kind, sf, nl, ini, mn = case
    n = _check(pkg, oracle, synth, w, h, nf, seed, lap, kind, scale_factor=sf, nlevels=nl, ini_th=ini, min_th=mn)
    if ini == 255:
        assert n == 0
    elif kind == "textured":
        assert n >= nf // 2


def test_retry_pass_matters(oracle, synth):
    """The 40/5 case above depends on the per-cell retry: without it (40/40) the oracle finds fewer keypoints."""
    img = synth.gen_image(752, 480, 13, "lowcontrast")
    with_retry = oracle.Extractor(1000, 1.2, 8, 40, 5)(img, (0, 0))
    without = oracle.Extractor(1000, 1.2, 8, 40, 40)(img, (0, 0))
    assert with_retry[0] > without[0] + 100


@pytest.mark.parametrize("nf", [1, 5, 17, 50])
def test_small_budgets(pkg, oracle, synth, nf):
    """Levels whose feature budget N is 0 or below 4 * nIni - 3 still return 4 * nIni keypoints (DistributeOctTree splits the root
    once): the 4 * nIni term of the product's per-level capacity max(N + 3, 4 * nIni) + 1, and a total the capacity must hold."""
    n = _check(pkg, oracle, synth, 752, 480, nf, 20 + nf, (0, 1000), "textured")
    ex = pkg.ORBextractor(nf, max_size=(752, 480), max_batch=1)
    assert nf <= n <= ex.cap
    assert (ex.features_per_level() + 3 < 8).any()                 # nIni is 2 on every level of 752 x 480
    if nf == 1:
        assert n == 64                                            # 8 per level (nIni 2)
    ex.close()


@pytest.mark.parametrize("w,h,nf,nl,per_level0", [(1241, 376, 20, 8, 16), (1241, 376, 4, 1, 16), (2400, 420, 50, 8, 24), (2400, 420, 11, 1, 24)])
def test_small_budgets_on_wide_frames(pkg, oracle, synth, w, h, nf, nl, per_level0):
    """Four and six quadtree roots with a budget below 4 * nIni: every level returns 4 * nIni keypoints, 16 / 24 on level 0."""
    n = _check(pkg, oracle, synth, w, h, nf, 30 + nf, (0, 0), "textured", nlevels=nl)
    ex = pkg.ORBextractor(nf, nlevels=nl, max_size=(w, h), max_batch=1)
    assert n <= ex.cap and (ex.features_per_level() < per_level0 - 3).all()
    mono, kps, _ = ex(synth.gen_image(w, h, 30 + nf, "textured"), (0, 0))
    assert np.count_nonzero(kps["octave"] == 0) == per_level0 and len(kps) >= nl * per_level0       # (the upper levels of 2400 x 420 have 7 and 8 roots)
    ex.close()


@pytest.mark.parametrize("w,h,sf,nl", [(239, 239, 1.2, 8), (337, 337, 1.5, 5)])
def test_one_pixel_below_the_smallest_size(pkg, oracle, synth, w, h, sf, nl):
    """One pixel less in either direction: the oracle returns -3, the product raises OrbError (ORBX_E_TOO_SMALL)."""
    ex = pkg.ORBextractor(100, sf, nl, max_size=(w, h), max_batch=1)
    for ww, hh in ((w - 1, h), (w, h - 1)):
        img = synth.gen_image(ww, hh, 1)
        assert oracle.Extractor(100, sf, nl)(img, (0, 0))[0] == -3
        with pytest.raises(pkg.OrbError, match="code -4"):            # ORBX_E_TOO_SMALL
            ex(img)
    ex.close()


def test_portrait_kitti_is_refused(pkg, oracle, synth):
    """376 x 1241: the quadtree's nIni rounds to 0, where the reference divides by zero.  The oracle returns 0 keypoints, the
    product refuses the geometry (ORBX_E_UNSUPPORTED) -- the documented divergence: at orbx_create when it is
    the maximum size, at the call when a larger maximum was accepted."""
    img = synth.gen_image(376, 1241, 1)
    n, _, _, mono = oracle.Extractor(1000)(img, (0, 0))
    assert n == 0 and mono == 0
    with pytest.raises(pkg.OrbError, match="code -6: .*nIni=0"):
        pkg.ORBextractor(1000, max_size=(376, 1241), max_batch=1)
    ex = pkg.ORBextractor(1000, max_size=(752, 1241), max_batch=1)
    with pytest.raises(pkg.OrbError, match="code -6: .*nIni=0"):
        ex(img)
    ex.close()


@pytest.mark.parametrize("nf,sf,nl,ini,mn", [(2000, 1.2, 8, 12, 7), (1000, 1.1, 12, 20, 7), (1000, 1.5, 5, 20, 7), (1500, 2.0, 4, 20, 7),
                                             (1000, 1.2, 1, 20, 7), (5, 1.3, 7, 40, 5), (4000, 1.2, 12, 20, 7)])
def test_getters_match_oracle_tables_params(pkg, oracle, nf, sf, nl, ini, mn):
    ex = pkg.ORBextractor(nf, sf, nl, ini, mn, max_size=(1920, 1080))
    t = oracle.Extractor(nf, sf, nl, ini, mn).tables()
    assert ex.GetLevels() == nl
    assert ex.GetScaleFactors().tobytes() == t["sf"].tobytes() and ex.GetInverseScaleFactors().tobytes() == t["inv_sf"].tobytes()
    assert ex.GetScaleSigmaSquares().tobytes() == t["sig2"].tobytes()
    assert ex.GetInverseScaleSigmaSquares().tobytes() == t["inv_sig2"].tobytes()
    assert np.array_equal(ex.features_per_level(), t["nfeat"])
    ex.close()


def _check_all(oracle, imgs, res, lap, *params):
    ref = oracle.Extractor(*params)
    for i, img in enumerate(imgs):
        n_ref, kps_ref, desc_ref, mono_ref = ref(img, lap)
        mono, kps, desc = res[i]
        assert len(kps) == n_ref and mono == mono_ref, i
        assert kps.tobytes() == kps_ref.tobytes() and np.array_equal(desc, desc_ref), i


def test_large_batch_twelve_levels(pkg, oracle, synth):
    """48 frames x 12 levels > 512 quadtree workgroups: k_quadtree2<256> and the walking k_blur3 schedule at 1.1 x 12."""
    kinds = ("textured", "sparse", "lowcontrast")
    imgs = [synth.gen_image(752, 480, 5000 + i, kinds[i % 3]) for i in range(48)]
    ex = pkg.ORBextractor(1000, 1.1, 12, 20, 7, max_size=(752, 480), max_batch=len(imgs))
    res = ex.extract_batch(imgs, [(0, 1000)] * len(imgs))
    _check_all(oracle, imgs, res, (0, 1000), 1000, 1.1, 12, 20, 7)
    ex.close()


def test_kitti_from_device_memory_tight_stride(pkg, oracle, synth):
    """KITTI frames from device memory at the tight stride 1241: misaligned rows, so the staging path runs at that width."""
    n, w, h = 3, KITTI_W, KITTI_H
    imgs = [synth.gen_image(w, h, 70 + i, "sparse") for i in range(n)]
    dev = pkg.DeviceBuffer(n * w * h + 64)
    for i, im in enumerate(imgs):
        dev.upload(np.ascontiguousarray(im), offset=i * w * h)
    ptrs = (C.c_void_p * n)(*[dev.ptr + i * w * h for i in range(n)])
    ex = pkg.ORBextractor(KITTI_NF, 1.2, 8, 12, 7, max_size=(w, h), max_batch=n)
    ex.enqueue_device(ptrs, w, h, w, [(0, 0)] * n)
    ex.sync()
    _check_all(oracle, imgs, [ex.fetch(i) for i in range(n)], (0, 0), KITTI_NF, 1.2, 8, 12, 7)
    ex.close()


# ---- batched matchers at non-default level counts and geometry

@pytest.fixture(scope="module", params=[(1.5, 5), (1.1, 12)], ids=["s1.5-L5", "s1.1-L12"])
def pyr_batch(request, pkg, synth):
    """Four 752x480 frames (frame 1 = frame 0, frame 3 = frame 2 shifted by a few pixels) at a non-default (scale, levels), with the
    grids of the whole block built on the device."""
    sf_, nl = request.param
    W, H, NB = 752, 480, 4
    a, b = synth.gen_image(W, H, 300), synth.gen_image(W, H, 301)
    imgs = [a, a, b, np.roll(b, (2, -3), (0, 1))]
    ex = pkg.ORBextractor(1000, sf_, nl, 20, 7, max_size=(W, H), max_batch=NB)
    res = ex.extract_batch(imgs, [(0, 1000)] * NB)
    m = pkg.ORBmatcher(0.9)
    L = pkg.lib()
    r = ex.result_device(); cap = r["cap"]
    inv_w, inv_h = float(np.float32(64) / np.float32(W)), float(np.float32(48) / np.float32(H))
    gs = pkg.DeviceBuffer(NB * 3073 * 4); gi = pkg.DeviceBuffer(NB * cap * 4)
    assert L.orbm_grid_build_batch_async(m.h, r["kps"], r["counts"], NB, cap, 0.0, 0.0, inv_w, inv_h, gs.ptr, gi.ptr) == 0
    m.sync()
    for f in range(NB):
        oct_ = res[f][1]["octave"]
        assert oct_.min() == 0 and oct_.max() == nl - 1, f          # keypoints on both end levels of the pyramid
    yield dict(W=W, H=H, NB=NB, nl=nl, ex=ex, res=res, m=m, L=L, r=r, cap=cap, gs=gs, gi=gi, inv_w=inv_w, inv_h=inv_h,
               sf=ex.GetScaleFactors())
    m.close(); ex.close()


def test_local_points_batch_levels(pkg, oracle, pyr_batch):
    """M3 (orbm_search_by_projection_points_batch_async) with the real level count and scale table: queries predicted on level 0 and
    on the top level reach both ends of the level-1..level window and of the candidate key's octave field."""
    B = pyr_batch
    L, m, res, cap, sf, nl = B["L"], B["m"], B["res"], B["cap"], B["sf"], B["nl"]
    OM = oracle._oracle_matcher_class()()
    rng = np.random.default_rng(17 + nl)
    NF = B["NB"]
    Q = [_queries(rng, res[f][1], res[f][2], 2500, nlev=nl) for f in range(NF)]
    for q in Q:
        lev = q["level"][q["in_view"] != 0]
        assert (lev == 0).any() and (lev == nl - 1).any()
    rows = _Rows(pkg, NF, 2500)
    rows.upload(Q)
    dm = pkg.DeviceBuffer(NF * cap * 4); dn = pkg.DeviceBuffer(NF * 4)
    for th in (1.0, 5.0):
        assert _call(L, m, B["r"], cap, B["gs"], B["gi"], 0, rows, sf, th, 0.8, dm, dn, inv_w=B["inv_w"], inv_h=B["inv_h"], nlev=nl) == 0, \
            L.orbm_last_error()
        m.sync()
        match = dm.download(np.int32, NF * cap).reshape(NF, cap); nm = dn.download(np.int32, NF)
        top = 0
        for f in range(NF):
            kt, dt = res[f][1], res[f][2]
            n_ref = _check_frame(pkg, m, OM, sf, kt, dt, Q[f], match[f], nm[f], th, 0.8, w=B["W"], h=B["H"])[0]
            assert n_ref > 300
            hit = match[f, :len(kt)]
            top += int((Q[f]["level"][hit[hit >= 0]] == nl - 1).sum())
        assert top > 0                                                      # matches of top-level queries


@pytest.mark.parametrize("check_ori", [True, False])
def test_search_by_projection_batch_levels(pkg, oracle, pyr_batch, check_ori):
    """M4 (orbm_search_by_projection_batch_async) with the real level count: queries carry every octave 0..nlevels-1, so the
    octave-1..octave+1 window is clipped at both ends.  Pairs: frame 1 -> 0 (same image), 2 -> 1 (different), 3 -> 2 (shifted)."""
    B = pyr_batch
    L, m, res, cap, sf, nl = B["L"], B["m"], B["res"], B["cap"], B["sf"], B["nl"]
    OM = oracle._oracle_matcher_class()()
    NP = B["NB"] - 1
    dm = pkg.DeviceBuffer(NP * cap * 4); dn = pkg.DeviceBuffer(NP * 4)
    dx, dy = 2.0, -1.0
    rc = L.orbm_search_by_projection_batch_async(m.h, B["r"]["kps"], B["r"]["desc"], B["r"]["counts"], cap, B["gs"].ptr, B["gi"].ptr, 0.0, 0.0,
                                                 B["inv_w"], B["inv_h"], 1, 0, NP, 15.0, sf.ctypes.data_as(C.c_void_p), nl, dx, dy, None, None,
                                                 int(check_ori), dm.ptr, dn.ptr)
    assert rc == 0, L.orbm_last_error()
    m.sync()
    match = dm.download(np.int32, NP * cap).reshape(NP, cap); nm = dn.download(np.int32, NP)
    ends = set()
    for p in range(NP):
        (_, kq, dq), (_, kt, dt) = res[p + 1], res[p]
        nq, nt = len(kq), len(kt)
        args = dict(cur_blocked=np.zeros(nt, np.uint8), scale_factors=sf, valid=np.ones(nq, np.uint8), u=kq["x"] + np.float32(dx),
                    v=kq["y"] + np.float32(dy), invzc=np.zeros(nq, np.float32), octave=kq["octave"], angle=kq["angle"], qdesc=dq,
                    mp_obs=np.ones(nq, np.uint8), th=15.0, check_ori=check_ori)
        n_ref, m_ref = OM.SearchByProjectionFrame(pkg.FrameView(kt, dt, B["W"], B["H"], backend=OM), **args)
        n_host, m_host = m.SearchByProjectionFrame(pkg.FrameView(kt, dt, B["W"], B["H"], backend=m), **args)
        assert n_host == n_ref and np.array_equal(m_host, m_ref)
        assert nm[p] == n_ref, (p, nm[p], n_ref)
        assert np.array_equal(match[p, :nt], m_ref), (p, np.flatnonzero(match[p, :nt] != m_ref)[:10])
        assert np.all(match[p, nt:] == -1)
        ends |= set(kq["octave"][m_ref[m_ref >= 0]].tolist()) & {0, nl - 1}
    assert nm[0] > 300                                                       # the same image
    assert ends == {0, nl - 1}                                               # matched queries on both end octaves


@pytest.mark.parametrize("geom", ["kitti", "s1.5-L5"])
def test_stereo_triangulation_batch_params(pkg, oracle, synth, tmp_path, geom):
    """orbm_stereo_batch_async (the SAD slide reads pyramid levels of these widths) then orbm_triangulation_batch_async with the
    extractor's own level count, against the oracle pair by pair."""
    if geom == "kitti":
        out = _stereo_bow_triangulation(pkg, oracle, synth, tmp_path, W=KITTI_W, H=KITTI_H, NF=KITTI_NF, P=2, mb=KITTI_BF / KITTI_FX,
                                        mbf=KITTI_BF, seed0=520, min_kept=300, min_tri=50)
    else:
        out = _stereo_bow_triangulation(pkg, oracle, synth, tmp_path, NF=1200, P=2, scale_factor=1.5, nlevels=5, seed0=530,
                                        min_kept=300, min_tri=50)
    assert len(out) == 2


def test_grid_build_batch_kitti(pkg, oracle, synth):
    """orbm_grid_build_batch_async at 1241 x 376 (inv_w = 64/1241 in float32) equals Frame::AssignFeaturesToGrid on the host."""
    n, w, h = 3, KITTI_W, KITTI_H
    imgs = [synth.gen_image(w, h, 80 + i, "sparse") for i in range(n)]
    ex = pkg.ORBextractor(KITTI_NF, max_size=(w, h), max_batch=n)
    res = ex.extract_batch(imgs, [(0, 0)] * n)
    m = pkg.ORBmatcher(0.9)
    OM = oracle._oracle_matcher_class()()
    L = pkg.lib()
    r = ex.result_device(); cap = r["cap"]
    inv_w, inv_h = np.float32(64) / np.float32(w), np.float32(48) / np.float32(h)
    gs = pkg.DeviceBuffer(n * 3073 * 4); gi = pkg.DeviceBuffer(n * cap * 4)
    assert L.orbm_grid_build_batch_async(m.h, r["kps"], r["counts"], n, cap, 0.0, 0.0, float(inv_w), float(inv_h), gs.ptr, gi.ptr) == 0
    m.sync()
    g_start = gs.download(np.int32, n * 3073).reshape(n, 3073); g_idx = gi.download(np.int32, n * cap).reshape(n, cap)
    for f in range(n):
        fo = pkg.FrameView(res[f][1], res[f][2], w, h, backend=OM)
        assert fo.inv_w == inv_w and fo.inv_h == inv_h
        assert fo.placed > 1500
        assert np.array_equal(g_start[f], fo.grid_start) and np.array_equal(g_idx[f, :fo.placed], fo.grid_idx[:fo.placed]), f
    m.close(); ex.close()
