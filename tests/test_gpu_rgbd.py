"""RGB-D frames on the device: orbm_stereo_from_rgbd(_batch_async) -- Frame::ComputeStereoFromRGBD with GrabImageRGBD's depth conversion
folded in -- and orbm_unproject_stereo(_batch_async) -- Frame::UnprojectStereo -- against tests/second_reading_rgbd.py, bit for bit
(floats compared as uint32, no tolerance): host form == device form == second reading.  The chain test runs the INTEGRATION recipe
"RGB-D frames on the device" up to the M4 search and compares its match rows with the host search fed by the second reading."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import second_reading as SR
import second_reading_rgbd as R
from test_motion_projection_cpu import project_last_frame_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H, CAP = 97, 61, 300
COUNTS = np.array([5, 0, 1, 63, 64, 65, 257], np.int32)                     # block frames 0..6: the wave and workgroup edges
CALLS = [(1, 6), (3, 1), (3, 4)]                                            # (nframes, first): frame 0 is never in a call
FACTORS = [F(1.0), F(1.0) / F(5000.0), F(0.5), F(1.0 + 5e-6)]
MBF = 40.0
SENT = F(-777.25)
GUARD = 4096                                                                # owned bytes around the images


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _block(pkg, rng):
    """A hand-laid result block of 7 frames: raw keypoints on exact integers, at (w-1+0.99, h-1+0.99), just outside the image on each
    side, inside by truncation ((-0.5, -0.5) reads pixel (0, 0)) and with a NaN coordinate; mvKeysUn is a different array."""
    kps = np.zeros((len(COUNTS), CAP), pkg.KP_DTYPE)
    kps["x"] = rng.uniform(-3, W + 3, kps.shape); kps["y"] = rng.uniform(-3, H + 3, kps.shape)    # slots beyond the count hold garbage too
    special = [(0.0, 0.0), (W - 1.0, H - 1.0), (W - 1 + 0.99, H - 1 + 0.99), (float(W), 5.0), (5.0, float(H)), (-1.0, 3.0), (3.0, -1.0),
               (-0.5, -0.5), (np.nan, 4.0), (4.0, np.nan), (12.0, 7.0), (1e30, 2.0), (np.inf, 2.0)]
    for f, n in enumerate(COUNTS):
        if n == 1:
            kps[f, 0]["x"], kps[f, 0]["y"] = special[2]
        elif n >= len(special):
            inside = rng.random(n) < 0.85
            kps[f, :n]["x"] = np.where(inside, rng.uniform(0, W, n), kps[f, :n]["x"])
            kps[f, :n]["y"] = np.where(inside, rng.uniform(0, H, n), kps[f, :n]["y"])
            at = rng.choice(n, len(special), replace=False)
            at[0] = n - 1                                                   # one special in the row's last slot
            for j, (x, y) in zip(at, special):
                kps[f, j]["x"], kps[f, j]["y"] = x, y
    un = kps.copy()
    un["x"] = (kps["x"] + rng.uniform(-2, 2, kps.shape)).astype(F); un["y"] = (kps["y"] + rng.uniform(-2, 2, kps.shape)).astype(F)
    return kps, un


def _pixels(rng, dtype, shape):
    if dtype == np.uint16:
        a = rng.integers(0, 65536, shape).astype(np.uint16)
        a[rng.random(shape) < 0.15] = 0
        a[rng.random(shape) < 0.05] = 65535
        return a
    a = rng.uniform(0.2, 9.0, shape).astype(F)
    for p, v in ((0.1, 0.0), (0.05, -1.5), (0.04, 1e-40), (0.04, np.nan), (0.04, np.inf), (0.02, -np.inf), (0.02, -0.0)):
        a[rng.random(shape) < p] = v
    return a


class _Images:
    """n images of W x H in rows of `stride` elements, inside one larger owned allocation (GUARD bytes before, between and after), and
    the device table of their pointers."""

    def __init__(self, pkg, rng, dtype, stride, n):
        self.dtype, self.stride, self.n = np.dtype(dtype), stride, n
        self.es = self.dtype.itemsize
        self.img_bytes = H * stride * self.es
        self.pitch = self.img_bytes + GUARD
        self.dev = pkg.DeviceBuffer(GUARD + n * self.pitch)
        self.tab = pkg.DeviceBuffer(8 * n)
        self.fill(rng)
        self.point(list(range(n)))

    def fill(self, rng):
        self.host = [_pixels(rng, self.dtype, (H, self.stride)) for _ in range(self.n)]
        special = 0 if self.dtype == np.uint16 else F(1e-40)
        for im in self.host:                                               # what the special keypoints read
            im[0, 0] = 65535 if self.dtype == np.uint16 else F(2.5); im[H - 1, W - 1] = special; im[7, 12] = 0
        raw = np.full(GUARD + self.n * self.pitch, 0xEE, np.uint8)
        for i, im in enumerate(self.host):
            raw[GUARD + i * self.pitch:GUARD + i * self.pitch + self.img_bytes] = im.view(np.uint8).reshape(-1)
        self.dev.upload(raw)

    def point(self, order):
        """table[f] = image order[f]"""
        self.order = list(order)
        self.tab.upload(np.array([self.dev.ptr + GUARD + i * self.pitch for i in order], np.uint64))

    def view(self, f):
        return self.host[self.order[f]][:, :W]                             # rows of `stride` elements: a strided host view


@pytest.fixture(scope="module")
def S(pkg):
    rng = np.random.default_rng(2026)
    m = pkg.ORBmatcher(0.9)
    kps, un = _block(pkg, rng)
    dk = pkg.DeviceBuffer(kps.nbytes).upload(kps); du = pkg.DeviceBuffer(un.nbytes).upload(un); dc = pkg.DeviceBuffer(COUNTS.nbytes).upload(COUNTS)
    return dict(m=m, L=m.L, kps=kps, un=un, dk=dk, du=du, dc=dc, rng=rng)


def _reading_rows(S, imgs, nframes, first, factor):
    ur = np.full((nframes, CAP), -1, F); dp = np.full((nframes, CAP), -1, F); nv = np.zeros(nframes, np.int32)
    for f in range(nframes):
        n = COUNTS[first + f]
        ur[f, :n], dp[f, :n], nv[f] = R.compute_stereo_from_rgbd(S["kps"][first + f, :n], S["un"][first + f, :n], imgs.view(f), factor, MBF)
    return ur, dp, nv


class _Out:
    """[nframes][CAP] uright / depth and [nframes] nvalid with one sentinel row (entry) before and after."""

    def __init__(self, pkg, nframes):
        self.nf = nframes
        self.ur = pkg.DeviceBuffer((nframes + 2) * CAP * 4); self.dp = pkg.DeviceBuffer((nframes + 2) * CAP * 4); self.nv = pkg.DeviceBuffer((nframes + 2) * 4)
        self.reset()

    def reset(self):
        self.ur.upload(np.full((self.nf + 2) * CAP, SENT, F)); self.dp.upload(np.full((self.nf + 2) * CAP, SENT, F))
        self.nv.upload(np.full(self.nf + 2, -12345, np.int32))

    def ptrs(self):
        return self.ur.ptr + CAP * 4, self.dp.ptr + CAP * 4, self.nv.ptr + 4

    def fetch(self):
        ur = self.ur.download(F, (self.nf + 2) * CAP).reshape(-1, CAP); dp = self.dp.download(F, (self.nf + 2) * CAP).reshape(-1, CAP)
        nv = self.nv.download(np.int32, self.nf + 2)
        assert np.all(ur[[0, -1]] == SENT) and np.all(dp[[0, -1]] == SENT) and nv[0] == nv[-1] == -12345, "a row outside the call was written"
        return ur[1:-1], dp[1:-1], nv[1:-1]


@pytest.mark.parametrize("nframes,first", CALLS)
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_rgbd_device_host_and_reading_agree(pkg, S, dtype, pad, nframes, first):
    m, L = S["m"], S["L"]
    rng = np.random.default_rng(100 + 10 * first + pad + (dtype == np.float32))
    imgs = _Images(pkg, rng, dtype, W + pad, nframes)
    dt = pkg.DEPTH_F32 if dtype == np.float32 else pkg.DEPTH_U16
    out = _Out(pkg, nframes)
    seen_valid = 0
    for factor in FACTORS:
        out.reset()
        pu, pd, pn = out.ptrs()
        rc = L.orbm_stereo_from_rgbd_batch_async(m.h, nframes, first, CAP, S["dk"].ptr, S["du"].ptr, S["dc"].ptr, imgs.tab.ptr, dt, W, H,
                                                 imgs.stride * imgs.es, float(factor), MBF, pu, pd, pn)
        assert rc == 0, L.orbm_last_error()
        m.sync()
        ur, dp, nv = out.fetch()
        eur, edp, env = _reading_rows(S, imgs, nframes, first, factor)
        print("factor %r: nvalid device %s reading %s" % (float(factor), nv.tolist(), env.tolist()))
        assert np.array_equal(nv, env)
        assert np.array_equal(_bits(dp), _bits(edp)), np.argwhere(_bits(dp) != _bits(edp))[:8]
        assert np.array_equal(_bits(ur), _bits(eur)), np.argwhere(_bits(ur) != _bits(eur))[:8]
        for f in range(nframes):
            n = COUNTS[first + f]
            assert np.all(ur[f, n:] == -1) and np.all(dp[f, n:] == -1)                      # slots at or beyond the count
            hn, hur, hdp = m.ComputeStereoFromRGBD(S["kps"][first + f, :n], S["un"][first + f, :n], imgs.view(f), factor, MBF)
            assert hn == env[f] and np.array_equal(_bits(hur), _bits(eur[f, :n])) and np.array_equal(_bits(hdp), _bits(edp[f, :n]))
        seen_valid += int(env.sum())
        if COUNTS[first:first + nframes].max() >= 63:                                       # the specials: outside the image -> -1 / -1
            f = int(np.argmax(COUNTS[first:first + nframes]))
            k = S["kps"][first + f, :COUNTS[first + f]]
            outside = (k["x"] == W) | (k["y"] == H) | (k["x"] == -1) | (k["y"] == -1) | np.isnan(k["x"]) | np.isnan(k["y"]) | (k["x"] > 1e20)
            assert outside.sum() >= 8 and np.all(ur[f, :len(k)][outside] == -1) and np.all(dp[f, :len(k)][outside] == -1)
    assert seen_valid > 0
    if dtype == np.float32:
        assert not R.needs_conversion(True, FACTORS[3]) and R.needs_conversion(True, FACTORS[2])


def test_near_one_factor_is_a_passthrough_only_for_f32(pkg, S):
    """F32 at 1 + 5e-6 must equal F32 at 1 exactly (no multiply); U16 at 1 + 5e-6 must differ from U16 at 1 (the multiply runs)."""
    m = S["m"]
    n = COUNTS[6]
    k, un = S["kps"][6, :n], S["un"][6, :n]
    img32 = np.random.default_rng(5).uniform(1, 3, (H, W)).astype(F)
    a = m.ComputeStereoFromRGBD(k, un, img32, FACTORS[3], MBF); b = m.ComputeStereoFromRGBD(k, un, img32, 1.0, MBF)
    assert a[0] == b[0] > 0 and np.array_equal(_bits(a[2]), _bits(b[2]))
    img16 = np.random.default_rng(6).integers(1, 65536, (H, W)).astype(np.uint16)
    a = m.ComputeStereoFromRGBD(k, un, img16, FACTORS[3], MBF); b = m.ComputeStereoFromRGBD(k, un, img16, 1.0, MBF)
    assert a[0] == b[0] > 0 and not np.array_equal(_bits(a[2]), _bits(b[2]))


def _pose(rng, ang=0.6, trans=2.0):
    a = rng.uniform(-ang, ang, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    Rm = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
          np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    return np.concatenate([Rm, rng.uniform(-trans, trans, 3)[:, None]], 1).astype(F).reshape(12)


@pytest.mark.parametrize("nrows,first", CALLS)
def test_unproject_device_host_and_reading_agree(pkg, S, nrows, first):
    """Random poses, depths with holes (-1, 0, NaN, a negative) and denormal / huge depths (finite results: the bits of a NaN are not pinned); mvKeysUn differs from mvKeys."""
    m, L = S["m"], S["L"]
    rng = np.random.default_rng(300 + first)
    K = np.array([517.3, 516.5, 318.6, 255.3], F)
    depth = rng.uniform(0.3, 12.0, (nrows, CAP)).astype(F)
    for p, v in ((0.15, -1.0), (0.05, 0.0), (0.05, np.nan), (0.03, -2.0), (0.02, 1e-40), (0.02, 3e30)):
        depth[rng.random(depth.shape) < p] = v
    for r in range(nrows):                                                  # the block's NaN / inf / 1e30 coordinates would unproject to NaNs
        u = S["un"][first + r]
        depth[r, ~(np.isfinite(u["x"]) & np.isfinite(u["y"]) & (np.abs(u["x"]) < 1e6))] = -1.0
    twc = np.stack([_pose(rng) for _ in range(nrows)])
    twc[0] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F) if nrows > 1 else twc[0]
    dd = pkg.DeviceBuffer(depth.nbytes).upload(depth); dT = pkg.DeviceBuffer(twc.nbytes).upload(twc)
    dx = pkg.DeviceBuffer((nrows + 2) * CAP * 12).upload(np.full((nrows + 2) * CAP * 3, SENT, F))
    dh = pkg.DeviceBuffer((nrows + 2) * CAP).upload(np.full((nrows + 2) * CAP, 0x5A, np.uint8))
    rc = L.orbm_unproject_stereo_batch_async(m.h, nrows, first, CAP, S["du"].ptr, S["dc"].ptr, dd.ptr, dT.ptr, _vp(K), dx.ptr + CAP * 12, dh.ptr + CAP)
    assert rc == 0, L.orbm_last_error()
    m.sync()
    x = dx.download(F, (nrows + 2) * CAP * 3).reshape(nrows + 2, CAP, 3); has = dh.download(np.uint8, (nrows + 2) * CAP).reshape(nrows + 2, CAP)
    assert np.all(x[[0, -1]] == SENT) and np.all(has[[0, -1]] == 0x5A), "a row outside the call was written"
    x, has = x[1:-1], has[1:-1]
    total = 0
    for r in range(nrows):
        n = COUNTS[first + r]
        ex, eh = R.unproject_stereo(S["un"][first + r, :n], depth[r, :n], twc[r], K)
        assert np.array_equal(has[r, :n], eh) and np.array_equal(_bits(x[r, :n]), _bits(ex)), (r, np.argwhere(_bits(x[r, :n]) != _bits(ex))[:6])
        assert not has[r, n:].any() and not _bits(x[r, n:]).any()                            # slots at or beyond the count: 0 and (0, 0, 0)
        hn, hx, hh = m.UnprojectStereo(S["un"][first + r, :n], depth[r, :n], twc[r], K)
        assert hn == int(eh.sum()) and np.array_equal(hh, eh) and np.array_equal(_bits(hx), _bits(ex))
        total += int(eh.sum())
    assert total > 0


def test_refused_arguments_enqueue_nothing(pkg, S):
    m, L = S["m"], S["L"]
    imgs = _Images(pkg, np.random.default_rng(7), np.uint16, W, 1)
    out = _Out(pkg, 1)
    pu, pd, pn = out.ptrs()
    base = dict(nframes=1, first=6, cap=CAP, kps=S["dk"].ptr, un=S["du"].ptr, counts=S["dc"].ptr, tab=imgs.tab.ptr, dt=pkg.DEPTH_U16, w=W, h=H,
                stride=W * 2, factor=1.0, ur=pu, dp=pd, nv=pn)

    def call(**kw):
        a = dict(base, **kw)
        return L.orbm_stereo_from_rgbd_batch_async(m.h, a["nframes"], a["first"], a["cap"], a["kps"], a["un"], a["counts"], a["tab"], a["dt"], a["w"], a["h"],
                                                   a["stride"], a["factor"], MBF, a["ur"], a["dp"], a["nv"])
    for kw in (dict(kps=None), dict(un=None), dict(counts=None), dict(tab=None), dict(ur=None), dict(dp=None), dict(nv=None),
               dict(nframes=0), dict(cap=0), dict(w=0), dict(h=0), dict(first=-1), dict(stride=W * 2 - 1), dict(stride=W * 2 - 2), dict(stride=W * 2 + 1),
               dict(dt=pkg.DEPTH_F32, stride=W * 4 - 4), dict(dt=2), dict(dt=-1), dict(factor=float("nan")), dict(factor=float("inf"))):
        assert call(**kw) == -2, kw
    assert L.orbm_stereo_from_rgbd_batch_async(None, 1, 6, CAP, base["kps"], base["un"], base["counts"], base["tab"], 0, W, H, W * 2, 1.0, MBF, pu, pd, pn) == -2
    k1 = S["kps"][6, :4]
    host = lambda **kw: L.orbm_stereo_from_rgbd(m.h, 4, _vp(k1), _vp(k1), kw.get("img", _vp(imgs.host[0])), kw.get("dt", 0), W, kw.get("h", H),
                                                kw.get("stride", W * 2), kw.get("factor", 1.0), MBF, _vp(hur), _vp(hdp))
    hur = np.full(4, SENT, F); hdp = np.full(4, SENT, F)
    assert host(img=None) == -2 and host(dt=5) == -2 and host(h=0) == -2 and host(stride=W) == -2 and host(factor=float("-inf")) == -2
    assert np.all(hur == SENT) and np.all(hdp == SENT)
    K = np.array([500, 500, 48, 30], F)
    dx = pkg.DeviceBuffer(3 * CAP * 12).upload(np.full(3 * CAP * 3, SENT, F)); dh = pkg.DeviceBuffer(3 * CAP).upload(np.full(3 * CAP, 0x5A, np.uint8))
    dT = pkg.DeviceBuffer(48).upload(np.zeros(12, F))
    ub = dict(nrows=1, first=6, cap=CAP, un=S["du"].ptr, counts=S["dc"].ptr, depth=pd, twc=dT.ptr, k=_vp(K), x=dx.ptr, has=dh.ptr)

    def ucall(**kw):
        a = dict(ub, **kw)
        return L.orbm_unproject_stereo_batch_async(m.h, a["nrows"], a["first"], a["cap"], a["un"], a["counts"], a["depth"], a["twc"], a["k"], a["x"], a["has"])
    for kw in (dict(un=None), dict(counts=None), dict(depth=None), dict(twc=None), dict(k=None), dict(x=None), dict(has=None), dict(nrows=0), dict(cap=0),
               dict(first=-1)):
        assert ucall(**kw) == -2, kw
    assert ucall(nrows=65536) == -3
    m.sync()
    ur, dp, nv = out.fetch()
    assert np.all(ur == SENT) and np.all(dp == SENT) and nv[0] == -12345
    assert np.all(dx.download(F, 3 * CAP * 3) == SENT) and np.all(dh.download(np.uint8, 3 * CAP) == 0x5A)


# ---------------------------------------------------------------------------------------------------------------------------
# the recipe of INTEGRATION.md "RGB-D frames on the device" on 3 synthetic frames, up to the M4 search, and its graph replay
# ---------------------------------------------------------------------------------------------------------------------------
CW, CH = 239, 239                                                           # the smallest size the (1.2, 8) extractor accepts
CK = np.array([210.0, 208.0, 119.5, 118.5], F)
CDIST = np.array([-0.06, 0.01, 0.0005, -0.0003], F)                         # mvKeysUn != mvKeys
CFACTOR = F(1.0) / F(5000.0)
CMB = 0.08
TH = 7.0


def _plane(frame, seed):
    """A tilted plane with holes, 16-bit at 5000 units per metre.  In frame 1 the right part sits at 40 % of the plane's depth, in frames
    0 and 2 it does not: across both pairs the right coordinate predicted from the last frame's depth (mbf / z, 12 to 35 px here) is off
    by about 20 px there, more than the search radius 7 * scale[octave] up to octave 5."""
    y, x = np.mgrid[0:CH, 0:CW]
    z = 2.0 + 0.004 * x + 0.002 * y
    if frame == 1:
        z = np.where(x > 0.55 * CW, 0.4 * z, z)
    raw = np.round(z * 5000.0).astype(np.uint16)
    raw[(x * 7 + y * 13 + seed) % 11 == 0] = 0
    return raw


@pytest.fixture(scope="module")
def chain(pkg, synth):
    L = pkg.lib()
    base = synth.gen_image(CW + 8, CH + 8, 9100)
    imgs = [np.ascontiguousarray(base[4 - s:4 - s + CH, 4 - 2 * s:4 - 2 * s + CW]) for s in range(3)]   # frame s = the scene shifted by (2s, s) px
    stride = (CW + 63) // 64 * 64
    dimg = pkg.DeviceBuffer(3 * stride * CH)
    for i, im in enumerate(imgs):
        pad = np.zeros((CH, stride), np.uint8); pad[:, :CW] = im
        dimg.upload(pad, offset=i * stride * CH)
    arr = (C.c_void_p * 3)(*[dimg.ptr + i * stride * CH for i in range(3)])
    ex = pkg.ORBextractor(500, max_size=(CW, CH), max_batch=3)
    mt = pkg.ORBmatcher(0.9)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    cap = ex.cap
    ex.enqueue_device(arr, CW, CH, stride)
    ex.sync()
    res = ex.fetch_all()
    counts = np.array([len(r[1]) for r in res], np.int32)
    assert counts.min() > 50
    depth = [_plane(i, 3 * i) for i in range(3)]
    dstride = CW + 3                                                        # odd-padded rows
    ddep = pkg.DeviceBuffer(GUARD + 3 * (dstride * CH * 2 + GUARD))
    pitch = dstride * CH * 2 + GUARD

    def upload_depth(images):
        raw = np.full(GUARD + 3 * pitch, 0xEE, np.uint8)
        for i, im in enumerate(images):
            pad = np.full((CH, dstride), 0xEEEE, np.uint16); pad[:, :CW] = im
            raw[GUARD + i * pitch:GUARD + i * pitch + pad.nbytes] = pad.view(np.uint8).reshape(-1)
        ddep.upload(raw)
    upload_depth(depth)
    dtab = pkg.DeviceBuffer(24).upload(np.array([ddep.ptr + GUARD + i * pitch for i in range(3)], np.uint64))
    bounds = mt.ComputeImageBounds(CW, CH, CK, CDIST)
    inv_w = float(F(64) / (bounds[1] - bounds[0])); inv_h = float(F(48) / (bounds[3] - bounds[2]))
    rng = np.random.default_rng(77)
    # poses: the camera steps to the left and up, so that the scene's points move right and down in the image as the content does
    twc = np.stack([np.array([1, 0, 0, -0.02 * s, 0, 1, 0, -0.01 * s, 0, 0, 1, 0], F) for s in range(3)])
    tcw = twc.copy(); tcw[:, [3, 7, 11]] = -twc[:, [3, 7, 11]]              # identity rotations: Tcw = [I | -Ow]
    return dict(L=L, ex=ex, mt=mt, cap=cap, res=res, counts=counts, arr=arr, stride=stride, depth=depth, dstride=dstride, dtab=dtab, ddep=ddep,
                pitch=pitch, upload_depth=upload_depth, bounds=bounds, inv_w=inv_w, inv_h=inv_h, twc=twc, tcw=tcw, sf=ex.GetScaleFactors(), rng=rng,
                dimg=dimg)


class _ChainBuffers:
    def __init__(self, pkg, cap):
        n3, n2 = 3 * cap, 2 * cap
        self.un = pkg.DeviceBuffer(n3 * 28)
        self.ur = pkg.DeviceBuffer(n3 * 4); self.dp = pkg.DeviceBuffer(n3 * 4); self.nv = pkg.DeviceBuffer(12)
        self.gs = pkg.DeviceBuffer(3 * 3073 * 4); self.gi = pkg.DeviceBuffer(n3 * 4)
        self.x3 = pkg.DeviceBuffer(n2 * 12); self.has = pkg.DeviceBuffer(n2)
        self.valid = pkg.DeviceBuffer(n2); self.u = pkg.DeviceBuffer(n2 * 4); self.v = pkg.DeviceBuffer(n2 * 4); self.iz = pkg.DeviceBuffer(n2 * 4)
        self.dir = pkg.DeviceBuffer(4)
        self.octave = pkg.DeviceBuffer(n2 * 4); self.angle = pkg.DeviceBuffer(n2 * 4); self.obs = pkg.DeviceBuffer(n2)
        self.match = pkg.DeviceBuffer(n2 * 4); self.nm = pkg.DeviceBuffer(8)
        self.twc = pkg.DeviceBuffer(96); self.tcur = pkg.DeviceBuffer(96); self.tlast = pkg.DeviceBuffer(96)


def _enqueue_chain(pkg, Cn, B, with_extract=True):
    """extract, undistort (DEVICE), rgbd, grid, unproject, project_last_frame, M4: pair p = last frame p, current frame p + 1."""
    L, ex, mt, cap = Cn["L"], Cn["ex"], Cn["mt"], Cn["cap"]
    r = ex.result_device()
    if with_extract:
        ex.enqueue_device(Cn["arr"], CW, CH, Cn["stride"])
    assert L.orbm_undistort_keypoints(mt.h, pkg.DEVICE, r["kps"], 3 * cap, _vp(CK), _vp(CDIST), 4, _vp(CK), B.un.ptr) >= 0, L.orbm_last_error()
    assert L.orbm_stereo_from_rgbd_batch_async(mt.h, 3, 0, cap, r["kps"], B.un.ptr, r["counts"], Cn["dtab"].ptr, pkg.DEPTH_U16, CW, CH, Cn["dstride"] * 2,
                                               float(CFACTOR), MBF, B.ur.ptr, B.dp.ptr, B.nv.ptr) == 0, L.orbm_last_error()
    b = Cn["bounds"]
    assert L.orbm_grid_build_batch_async(mt.h, B.un.ptr, r["counts"], 3, cap, float(b[0]), float(b[2]), Cn["inv_w"], Cn["inv_h"], B.gs.ptr, B.gi.ptr) == 0
    assert L.orbm_unproject_stereo_batch_async(mt.h, 2, 0, cap, B.un.ptr, r["counts"], B.dp.ptr, B.twc.ptr, _vp(CK), B.x3.ptr, B.has.ptr) == 0, L.orbm_last_error()
    assert L.orbm_project_last_frame_batch_async(mt.h, 2, B.tcur.ptr, B.tlast.ptr, r["counts"], cap, B.x3.ptr, B.has.ptr, _vp(CK), _vp(b), CMB, 0,
                                                 B.valid.ptr, B.u.ptr, B.v.ptr, B.iz.ptr, B.dir.ptr) == 0, L.orbm_last_error()
    rc = L.orbm_search_by_projection_frame_batch_async(
        mt.h, B.un.ptr, r["desc"], r["counts"], cap, B.gs.ptr, B.gi.ptr, float(b[0]), float(b[2]), Cn["inv_w"], Cn["inv_h"], 1, 2,
        B.ur.ptr + cap * 4, MBF, None, B.dir.ptr, r["counts"], cap, B.valid.ptr, B.u.ptr, B.v.ptr, B.iz.ptr, B.octave.ptr, B.angle.ptr, r["desc"],
        B.obs.ptr, TH, 0, _vp(Cn["sf"]), 8, 1, B.match.ptr, B.nm.ptr, None)
    assert rc == 0, L.orbm_last_error()


def _chain_reference(pkg, Cn, depth_images, order):
    """The same chain from the second readings; returns per pair the host search's row and the precondition's evidence."""
    mt, res, cap, b = Cn["mt"], Cn["res"], Cn["cap"], Cn["bounds"]
    un = [mt.UndistortKeyPoints(res[f][1], CK, CDIST) for f in range(3)]
    rd = [R.compute_stereo_from_rgbd(res[f][1], un[f], depth_images[order[f]], CFACTOR, MBF) for f in range(3)]
    out = []
    for p in range(2):
        x3, has = R.unproject_stereo(un[p], rd[p][1], Cn["twc"][p], CK)
        valid, u, v, iz, d = project_last_frame_np(Cn["tcw"][p + 1][None], Cn["tcw"][p][None], x3[None], has[None], CK, b, CMB, False)
        args = dict(cur_blocked=np.zeros(len(un[p + 1]), np.uint8), scale_factors=Cn["sf"], valid=valid[0], u=u[0], v=v[0], invzc=iz[0],
                    octave=res[p][1]["octave"], angle=res[p][1]["angle"], qdesc=res[p][2], mp_obs=np.ones(len(un[p]), np.uint8), th=TH,
                    forward=int(d[0]) == 1, backward=int(d[0]) == 2, check_ori=True)
        fv = pkg.FrameView(un[p + 1], res[p + 1][2], CW, CH, uright=rd[p + 1][0])
        fv.min_x, fv.min_y, fv.inv_w, fv.inv_h = b[0], b[2], F(Cn["inv_w"]), F(Cn["inv_h"])
        mt.grid_build(fv)
        n_h, m_h = mt.SearchByProjectionFrame(fv, mbf=MBF, **args)
        # the precondition, on the CPU with the second reading alone: the gate rejects a candidate the ungated search accepts
        gf = SR.GridFrame(un[p + 1], res[p + 1][2], b[0], b[2], Cn["inv_w"], Cn["inv_h"], uright=rd[p + 1][0])
        n_g, m_g, t_g = SR.search_by_projection_frame(gf, mbf=MBF, **args)
        gf0 = SR.GridFrame(un[p + 1], res[p + 1][2], b[0], b[2], Cn["inv_w"], Cn["inv_h"])
        n_0, m_0, _ = SR.search_by_projection_frame(gf0, mbf=MBF, **args)
        lost = [(s, int(m_0[s])) for s in np.flatnonzero((m_0 >= 0) & (m_g != m_0))
                if float(rd[p + 1][0][s]) > 0 and abs(F(u[0][m_0[s]]) - F(MBF) * F(iz[0][m_0[s]]) - rd[p + 1][0][s]) > F(TH) * Cn["sf"][res[p][1]["octave"][m_0[s]]]]
        out.append(dict(un=un, rd=rd, x3=x3, has=has, valid=valid[0], u=u[0], v=v[0], iz=iz[0], dir=int(d[0]), n_h=n_h, m_h=m_h, n_g=n_g, m_g=m_g,
                        rejected=t_g["stereo_gate_rejected"], applied=t_g["stereo_gate_applied"], skipped=t_g["stereo_gate_skipped"], lost=lost, n_0=n_0))
    return out


def _upload_rows(Cn, B):
    cap, res = Cn["cap"], Cn["res"]
    octv = np.zeros((2, cap), np.int32); ang = np.zeros((2, cap), F)
    for p in range(2):
        octv[p, :len(res[p][1])] = res[p][1]["octave"]; ang[p, :len(res[p][1])] = res[p][1]["angle"]
    B.octave.upload(octv); B.angle.upload(ang); B.obs.upload(np.ones(2 * cap, np.uint8))
    B.twc.upload(Cn["twc"][:2]); B.tcur.upload(Cn["tcw"][1:3]); B.tlast.upload(Cn["tcw"][:2])


def _check_chain(Cn, B, ref):
    cap, counts = Cn["cap"], Cn["counts"]
    ur = B.ur.download(F, 3 * cap).reshape(3, cap); dp = B.dp.download(F, 3 * cap).reshape(3, cap); nv = B.nv.download(np.int32, 3)
    rd = ref[0]["rd"]
    for f in range(3):
        n = counts[f]
        assert nv[f] == rd[f][2] and np.array_equal(_bits(ur[f, :n]), _bits(rd[f][0])) and np.array_equal(_bits(dp[f, :n]), _bits(rd[f][1]))
        assert np.all(ur[f, n:] == -1) and np.all(dp[f, n:] == -1)
    x3 = B.x3.download(F, 2 * cap * 3).reshape(2, cap, 3); has = B.has.download(np.uint8, 2 * cap).reshape(2, cap)
    match = B.match.download(np.int32, 2 * cap).reshape(2, cap); nm = B.nm.download(np.int32, 2)
    for p in range(2):
        n, n2 = counts[p], counts[p + 1]
        assert np.array_equal(has[p, :n], ref[p]["has"]) and np.array_equal(_bits(x3[p, :n]), _bits(ref[p]["x3"]))
        assert nm[p] == ref[p]["n_h"] == ref[p]["n_g"], (nm[p], ref[p]["n_h"], ref[p]["n_g"])
        assert np.array_equal(match[p, :n2], ref[p]["m_h"]) and np.array_equal(ref[p]["m_h"], ref[p]["m_g"]), np.flatnonzero(match[p, :n2] != ref[p]["m_h"])[:10]
        assert np.all(match[p, n2:] == -1)
    return nv, nm


def test_chain_extract_to_m4(pkg, chain):
    Cn = chain
    B = _ChainBuffers(pkg, Cn["cap"])
    _upload_rows(Cn, B)
    ref = _chain_reference(pkg, Cn, Cn["depth"], [0, 1, 2])
    for p in range(2):                                                      # cannot pass vacuously
        e = ref[p]
        print("pair %d: %d matches gated, %d ungated; gate applied %d, rejected %d, skipped %d; ungated matches the gate takes away: %d"
              % (p, e["n_g"], e["n_0"], e["applied"], e["rejected"], e["skipped"], len(e["lost"])))
        assert e["rejected"] > 0 and e["skipped"] > 0 and len(e["lost"]) >= 1 and e["n_g"] > 20
    _enqueue_chain(pkg, Cn, B)
    Cn["ex"].sync()
    _check_chain(Cn, B, ref)


def test_chain_capture_replay_follows_pixels_and_table(pkg, chain):
    """After one eager run the chain is captured; the depth pixels and the pointer table are then rewritten and the graph replayed:
    the rows follow the new contents, and a second replay gives the same nvalid (nothing accumulates)."""
    Cn = chain
    L, ex = Cn["L"], Cn["ex"]
    B = _ChainBuffers(pkg, Cn["cap"])
    _upload_rows(Cn, B)
    _enqueue_chain(pkg, Cn, B)
    ex.sync()
    eager_nv = B.nv.download(np.int32, 3)
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    _enqueue_chain(pkg, Cn, B)
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    new_depth = [_plane(i, 5 + i) for i in range(3)]                        # other holes
    new_depth[1] = (new_depth[1] // 2).astype(np.uint16)
    Cn["upload_depth"](new_depth)
    order = [2, 1, 0]                                                       # and the table points elsewhere
    Cn["dtab"].upload(np.array([Cn["ddep"].ptr + GUARD + i * Cn["pitch"] for i in order], np.uint64))
    try:
        ref = _chain_reference(pkg, Cn, new_depth, order)
        got = []
        for _ in range(2):
            B.nv.upload(np.full(3, 999, np.int32)); B.ur.upload(np.full(3 * Cn["cap"], SENT, F))
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            ex.sync()
            nv, _ = _check_chain(Cn, B, ref)
            got.append(nv.copy())
        assert np.array_equal(got[0], got[1]) and not np.array_equal(got[0], eager_nv)
    finally:
        Cn["upload_depth"](Cn["depth"])
        Cn["dtab"].upload(np.array([Cn["ddep"].ptr + GUARD + i * Cn["pitch"] for i in range(3)], np.uint64))


def test_cpp_facade_rgbd_helpers(pkg, tmp_path):
    """facade/FrameGeometry.h's ComputeStereoFromRGBD / UnprojectStereoAll on mock vectors against plain C++ in the same file."""
    pkg.build()
    exe = str(tmp_path / "facade_rgbd_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "facade_rgbd_smoke.cpp"),
                           "-L", os.path.join(ROOT, "orb-slam3_amd"), "-lorbslam3_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "orb-slam3_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "need-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "facade_rgbd_smoke ok" in out.stdout, out.stdout + out.stderr
