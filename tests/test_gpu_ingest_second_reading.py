"""k_gray, k_remap, k_clahe_lut / k_clahe_apply and k_undistort held DIRECTLY to tests/second_reading_ingest.py (not via the oracle) on
the cases of tests/ingest_cases.py, through the raw C ABI so that the paths the Python wrappers cannot reach are taken: destination
base offsets 0..3 with strides w, w + 1, w + 3 and the next multiple of 64 (the byte-store fallback as a whole row, not only as the
tail), three separately allocated images per call, device sources at every row alignment, out-of-place CLAHE, a remap destination of
another size than its source.  Every destination lies in an allocation of its own that is prefilled with 0xA5 and compared WHOLE
afterwards: the guard band before the first row, the stride padding of every row and the band after the last row must still hold 0xA5.

Every pointer, offset and stride below stays inside its allocation: a destination buffer is [GUARD][offset][h rows of stride][GUARD]
bytes; a kernel writes at most [dst, dst + (h - 1) * stride + w).  The refused calls (too fine a CLAHE grid, tilt coefficients, a
remap source beyond 32767) return on the host before anything is enqueued (orbx_api.hip / orbm_api.hip: the checks precede
hipSetDevice)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ingest_cases as IC

pytestmark = pytest.mark.gpu

F = np.float32
GUARD, FILL = 64, 0xA5
LAYOUTS = list(itertools.product(range(4), ("w", "w+1", "w+3", "64")))  # destination base offset, stride rule
ORBX_E_UNSUPPORTED, ORBM_E_INVALID = -6, -2


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _stride(w, rule):
    return {"w": w, "w+1": w + 1, "w+3": w + 3, "64": (w + 63) // 64 * 64}[rule]


def _ptrs(values):
    return (C.c_void_p * len(values))(*values)


class Guarded:
    """nimg separate device allocations for destinations of up to w x h pixels under any layout of LAYOUTS."""

    def __init__(self, pkg, w, h, nimg=3):
        self.cap = GUARD + 3 + (w + 64) * h + GUARD
        self.bufs = [pkg.DeviceBuffer(self.cap) for _ in range(nimg)]

    def prepare(self, w, h, layout, rows=None):
        """Fill with 0xA5 (and the images `rows` at the destination itself, for an in-place call) -> (device pointers, stride)."""
        off, rule = layout
        self.w, self.h, self.off, self.stride = w, h, off, _stride(w, rule)
        self.total = GUARD + off + self.stride * h + GUARD
        assert self.total <= self.cap
        for k, b in enumerate(self.bufs):
            b.upload(self._host(None if rows is None else rows[k]))
        return _ptrs([b.ptr + GUARD + off for b in self.bufs]), self.stride

    def _host(self, rows):
        a = np.full(self.total, FILL, np.uint8)
        if rows is not None:
            body = a[GUARD + self.off:GUARD + self.off + self.stride * self.h].reshape(self.h, self.stride)
            body[:, :self.w] = rows
        return a

    def check(self, wants, what):
        for k, (b, want) in enumerate(zip(self.bufs, wants)):
            got = b.download(np.uint8, self.total)
            exp = self._host(want)
            if not np.array_equal(got, exp):
                bad = np.flatnonzero(got != exp)
                body = (bad >= GUARD + self.off) & (bad < GUARD + self.off + self.stride * self.h)
                col = (bad - GUARD - self.off) % self.stride
                inside = body & (col < self.w)
                raise AssertionError("%s, image %d: %d wrong pixels (first at byte %s), %d guard / padding bytes overwritten (first at byte %s)"
                                     % (what, k, int(inside.sum()), bad[inside][:1], int((~inside).sum()), bad[~inside][:1]))


def _device_images(pkg, imgs, stride, base):
    """Three separate device allocations holding the 2-D byte images at `base` bytes from their start, rows `stride` apart; the row
    padding holds 201."""
    h, wb = imgs[0].shape
    bufs = []
    for im in imgs:
        host = np.full(base + stride * h, 201, np.uint8)
        host[base:].reshape(h, stride)[:, :wb] = im
        bufs.append(pkg.DeviceBuffer(host.nbytes).upload(host))
    return bufs, _ptrs([b.ptr + base for b in bufs])


# ---- cvtColor -------------------------------------------------------------------------------------------------------------------
GRAY_SOURCES = [("host", 0, 0)] + [("device", extra, base) for extra in (0, 1, 5) for base in range(4)]


@pytest.mark.parametrize("size", IC.GRAY_SIZES, ids=lambda s: "%dx%d" % s)
def test_gray_against_the_reading(pkg, size):
    """Host sources; ORBX_DEVICE sources with src_stride = w * ch + {0, 1, 5} (3-channel rows start at every alignment) at base offsets
    0..3 (a 4-channel image off the dword path); every destination layout, cycling through the launches."""
    w, h = size
    ex = pkg.ORBextractor(500, max_size=(752, 480), max_batch=1)
    try:
        dst = Guarded(pkg, w, h)
        for idx, ((ch, blue_first, bits), (space, extra, base)) in enumerate(itertools.product(IC.GRAY_VARIANTS, GRAY_SOURCES)):
            imgs = IC.gray_images(w, h, ch)
            wants = [r[0] for r in IC.gray_reading(w, h, ch, blue_first, bits)]
            sstride = w * ch + extra
            if space == "host":
                keep = [np.ascontiguousarray(im) for im in imgs]
                srcs = _ptrs([im.ctypes.data for im in keep])
            else:
                keep, srcs = _device_images(pkg, [im.reshape(h, w * ch) for im in imgs], sstride, base)
            layout = LAYOUTS[idx % len(LAYOUTS)]
            dsts, dstride = dst.prepare(w, h, layout)
            rc = ex.L.orbx_gray_from_color(ex.h, srcs, pkg.DEVICE if space == "device" else pkg.HOST, 3, w, h, sstride, ch, int(blue_first), bits,
                                           dsts, dstride)
            assert rc == 0, ex.L.orbx_last_error()
            ex.sync()
            dst.check(wants, "gray ch=%d blue_first=%d bits=%d src=%s+%d@%d dst=%s" % (ch, blue_first, bits, space, extra, base, layout))
    finally:
        ex.close()


# ---- remap ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IC.REMAP_CASES, ids=lambda c: "%dx%d-%dx%d-%s" % (c[0] + c[1] + (c[2],)))
def test_remap_against_the_reading(pkg, case):
    """A destination of another size than the source, a padded source stride, every destination layout.  The far-outside, non-finite
    entries give 0 and the entries beside them what the reading says."""
    (sw, sh), (dw, dh), _ = case
    mx, my, far = IC.remap_maps(*case)
    wants = [r[0] for r in IC.remap_reading(*case)]
    ex = pkg.ORBextractor(500, max_size=(752, 480), max_batch=1)
    try:
        keep, srcs = _device_images(pkg, IC.remap_sources(sw, sh), sw + 3, 0)
        dmx = pkg.DeviceBuffer(mx.nbytes).upload(mx); dmy = pkg.DeviceBuffer(my.nbytes).upload(my)
        dst = Guarded(pkg, dw, dh)
        for layout in LAYOUTS:
            dsts, dstride = dst.prepare(dw, dh, layout)
            rc = ex.L.orbx_remap_linear(ex.h, srcs, 3, sw, sh, sw + 3, dmx.ptr, dmy.ptr, dw, dh, dsts, dstride)
            assert rc == 0, ex.L.orbx_last_error()
            ex.sync()
            dst.check(wants, "remap dst=%s" % (layout,))
        assert all(not w_[far].any() for w_ in wants)                    # what the comparison above held the kernel to
    finally:
        ex.close()


def test_remap_refuses_a_source_beyond_short_coordinates(pkg):
    ex = pkg.ORBextractor(500, max_size=(752, 480), max_batch=1)
    try:
        dst = Guarded(pkg, 4, 1, nimg=1)
        dsts, dstride = dst.prepare(4, 1, (0, "w"))
        m = pkg.DeviceBuffer(16).upload(np.zeros(4, F))
        src = pkg.DeviceBuffer(64)
        for sw, sh in ((32768, 1), (1, 32768)):                          # refused on the host: nothing is read or written
            rc = ex.L.orbx_remap_linear(ex.h, _ptrs([src.ptr]), 1, sw, sh, sw, m.ptr, m.ptr, 4, 1, dsts, dstride)
            assert rc == ORBX_E_UNSUPPORTED and b"32767" in ex.L.orbx_last_error()
        ex.sync()
        dst.check([np.full((1, 4), FILL, np.uint8)], "refused remap")
    finally:
        ex.close()


# ---- CLAHE ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,tiles", IC.CLAHE_SIZES, ids=lambda v: "%dx%d" % v)
def test_clahe_against_the_reading(pkg, size, tiles):
    """In place, and out of place with src_stride != dst_stride, under every destination layout; the clip limits and image kinds cycle
    through the launches (all twelve (clip, image triplet) pairs occur)."""
    w, h = size
    combos = list(itertools.product(IC.CLAHE_CLIPS, (IC.CLAHE_KINDS[:3], IC.CLAHE_KINDS[3:])))
    ex = pkg.ORBextractor(500, max_size=(752, 480), max_batch=1)
    try:
        dst = Guarded(pkg, w, h)
        for idx, (layout, in_place) in enumerate(itertools.product(LAYOUTS, (True, False))):
            clip, kinds = combos[idx % len(combos)]
            imgs = [IC.clahe_image(w, h, k) for k in kinds]
            wants = [IC.clahe_reading(size, tiles, clip, k)[0] for k in kinds]
            if in_place:
                dsts, dstride = dst.prepare(w, h, layout, rows=imgs)
                keep, srcs, sstride = None, dsts, dstride
            else:
                dsts, dstride = dst.prepare(w, h, layout)
                sstride = w + 5
                keep, srcs = _device_images(pkg, imgs, sstride, 1)
            rc = ex.L.orbx_clahe(ex.h, srcs, 3, w, h, sstride, clip, tiles[0], tiles[1], dsts, dstride)
            assert rc == 0, ex.L.orbx_last_error()
            ex.sync()
            dst.check(wants, "clahe clip=%g %s in_place=%d dst=%s" % (clip, kinds, in_place, layout))
    finally:
        ex.close()


def test_clahe_refuses_too_fine_a_grid(pkg):
    (w, h), tiles = IC.CLAHE_REFUSED
    ex = pkg.ORBextractor(500, max_size=(752, 480), max_batch=1)
    try:
        dst = Guarded(pkg, w, h)
        dsts, dstride = dst.prepare(w, h, (1, "w+1"))
        keep, srcs = _device_images(pkg, [IC.clahe_image(w, h, "random")] * 3, w, 0)
        assert ex.L.orbx_clahe(ex.h, srcs, 3, w, h, w, 3.0, tiles[0], tiles[1], dsts, dstride) == ORBX_E_UNSUPPORTED
        ex.sync()
        dst.check([np.full((h, w), FILL, np.uint8)] * 3, "refused clahe")
    finally:
        ex.close()


# ---- undistortion ---------------------------------------------------------------------------------------------------------------
def _keypoints(pkg, u, v):
    rng = np.random.default_rng(len(u))
    k = np.zeros(len(u), pkg.KP_DTYPE)
    k["x"] = u; k["y"] = v
    k["size"] = rng.uniform(10, 100, len(u)).astype(F); k["angle"] = rng.uniform(0, 360, len(u)).astype(F)
    k["response"] = rng.integers(7, 255, len(u)); k["octave"] = rng.integers(0, 8, len(u)); k["class_id"] = rng.integers(-1, 1000, len(u))
    return k


def _undistort(pkg, m, space, kps, dist, new_k):
    """-> (rc, out): through ORBM_HOST, or ORBM_DEVICE with a guard band of 0xA5 behind the n output records."""
    n = len(kps)
    K = np.array(IC.EUROC_K, F); nk = np.array(new_k, F); d = np.array(dist, F)
    if space == pkg.HOST:
        out = np.full(28 * (n + 2), FILL, np.uint8).view(pkg.KP_DTYPE)
        rc = m.L.orbm_undistort_keypoints(m.h, pkg.HOST, _p(kps), n, _p(K), _p(d), len(d), _p(nk), _p(out))
        assert out[n:].tobytes() == bytes([FILL]) * 56
        return rc, out[:n]
    din = pkg.DeviceBuffer(28 * n).upload(kps)
    dout = pkg.DeviceBuffer(28 * n + GUARD).upload(np.full(28 * n + GUARD, FILL, np.uint8))
    rc = m.L.orbm_undistort_keypoints(m.h, pkg.DEVICE, din.ptr, n, _p(K), _p(d), len(d), _p(nk), dout.ptr)
    m.sync()
    raw = dout.download(np.uint8, 28 * n + GUARD)
    assert np.all(raw[28 * n:] == FILL)
    return rc, raw[:28 * n].view(pkg.KP_DTYPE)


@pytest.mark.parametrize("name,new_k", IC.UNDIST_CASES)
def test_undistort_against_the_reading(pkg, name, new_k):
    """4, 5, 8 and 12 coefficients (the rational and thin-prism terms), the icdist < 0 bail-out, newK != K; n around the workgroup size;
    both spaces; every other keypoint field copied.  Exact: none of the inputs is undecidable."""
    want, undecidable, _ = IC.undistort_reading(name, new_k)
    assert not undecidable.any()
    u, v = IC.undistort_points(name)
    m = pkg.ORBmatcher()
    for n in [c for c in IC.UNDIST_COUNTS if c <= len(want)]:
        kps = _keypoints(pkg, u[:n], v[:n])
        for space in (pkg.HOST, pkg.DEVICE):
            rc, out = _undistort(pkg, m, space, kps, IC.DIST_SETS[name], IC.NEW_K if new_k else IC.EUROC_K)
            assert rc == n, m.L.orbm_last_error()
            got = np.stack([out["x"], out["y"]], axis=1)
            assert got.tobytes() == want[:n].tobytes(), (n, space, np.argwhere(got.view(np.uint32) != want[:n].view(np.uint32))[:8])
            for f in ("size", "angle", "response", "octave", "class_id"):
                assert out[f].tobytes() == kps[f].tobytes(), f


def test_undistort_copies_when_the_first_coefficient_is_zero(pkg):
    u, v = IC.undistort_points("copy")
    m = pkg.ORBmatcher()
    for n in (1, 257):
        kps = _keypoints(pkg, u[:n], v[:n])
        for space in (pkg.HOST, pkg.DEVICE):
            rc, out = _undistort(pkg, m, space, kps, IC.DIST_SETS["copy"], IC.NEW_K)
            assert rc == n and out.tobytes() == kps.tobytes()


@pytest.mark.parametrize("size", IC.BOUNDS_SIZES, ids=lambda s: "%dx%d" % s)
def test_image_bounds_against_the_reading(pkg, size):
    m = pkg.ORBmatcher()
    K = np.array(IC.EUROC_K, F)
    for name in ("euroc4", "five", "rational8", "prism12", "copy"):
        want, undecidable, _ = IC.bounds_reading(name, size)
        assert not undecidable
        d = np.array(IC.DIST_SETS[name], F); b = np.zeros(4, F)
        assert m.L.orbm_image_bounds(m.h, size[0], size[1], _p(K), _p(d), len(d), _p(K), _p(b)) == 0, m.L.orbm_last_error()
        assert b.tobytes() == want.tobytes(), (name, b, want)


def test_tilt_coefficients_are_refused(pkg):
    """dist[12] / dist[13]: there is no inverse tilt in k_undistort, so the call is refused on the host instead of answering with the
    12-term result; 14 coefficients with both of them zero are served."""
    u, v = IC.undistort_points("prism12")
    m = pkg.ORBmatcher()
    kps = _keypoints(pkg, u[:5], v[:5])
    K = np.array(IC.EUROC_K, F); b = np.full(4, 7, F)
    for dist in (IC.TILT, IC.TILT[:13], IC.TILT[:12] + (0.0, 1e-3)):
        for space in (pkg.HOST, pkg.DEVICE):
            rc, out = _undistort(pkg, m, space, kps, dist, IC.EUROC_K)
            assert rc == ORBM_E_INVALID and b"tilt" in m.L.orbm_last_error()
            assert np.all(out.view(np.uint8) == FILL)                    # nothing written
        d = np.array(dist, F)
        assert m.L.orbm_image_bounds(m.h, 752, 480, _p(K), _p(d), len(d), _p(K), _p(b)) == ORBM_E_INVALID and b.tolist() == [7.0] * 4
    rc, out = _undistort(pkg, m, pkg.HOST, kps, IC.TILT[:12] + (0.0, 0.0), IC.EUROC_K)
    want = IC.undistort_reading("prism12")[0][:5]
    assert rc == 5 and np.stack([out["x"], out["y"]], axis=1).tobytes() == want.tobytes()
