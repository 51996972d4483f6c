"""orb-slam3_amd -- MI355X-native ORB front-end (extract + match) for ORB-SLAM3.

Python host mirror of the reference's C++ operator interface, for tests / bench / scripting:
    ORBextractor  <->  ORB_SLAM3::ORBextractor   (include/ORBextractor.h:49-83)
    ORBmatcher    <->  ORB_SLAM3::ORBmatcher     (include/ORBmatcher.h:35-111)  -- flattened-array form
Everything computes through the C ABI of liborbslam3_amd.so (include/orbx.h, include/orbm.h), i.e. the
hand-written gfx950 kernels.  There is NO CPU fallback: a missing library or device raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORB_LIB") or os.path.join(_HERE, "liborbslam3_amd.so")   # ORB_LIB: A/B builds of the same ABI
_LIB = None

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

HOST, DEVICE = 0, 1
DEPTH_U16, DEPTH_F32 = 0, 1                          # include/orbm.h: ORBM_DEPTH_*
DEPTH_SELECT_MAX_CAP = 16384                         # include/orbm.h: ORBM_DEPTH_SELECT_MAX_CAP
BOWVEC_MAX_CAP = 16384                               # include/orbm.h: ORBM_BOWVEC_MAX_CAP
KFDB_MAX_ROWS, KFDB_MAX_QUERIES = 1 << 20, 65535     # include/orbm.h: ORBM_KFDB_MAX_ROWS, ORBM_KFDB_MAX_QUERIES
KFCULL_MAX_CAND, KFCULL_MAX_CAP = 65535, 65535       # include/orbm.h: ORBM_KFCULL_MAX_CAND, ORBM_KFCULL_MAX_CAP
COVIS_MAX_QUERIES, COVIS_MAX_SLOTS, COVIS_MAX_ROWS, COVIS_MAX_VOTES = 65535, 65535, 1 << 20, 1 << 28   # include/orbm.h: ORBM_COVIS_MAX_*
LOCALPTS_MAX_FRAMES, LOCALPTS_MAX_KFS, LOCALPTS_MAX_CAP = 65535, 65535, 65535                          # include/orbm.h: ORBM_LOCALPTS_MAX_*
POSEOPT_MAX_FRAMES, POSEOPT_MAX_CAP, POSEOPT_MAX_LEVELS = 65535, 65535, 32                              # include/orbm.h: ORBM_POSEOPT_MAX_*
TRI_MAX_CAP, TRI_MAX_PAIRS, TRI_MAX_GROUP_PAIRS, TRI_MAX_LEVELS = 65535, 65535, 64, 32                  # include/orbm.h: ORBM_TRI_MAX_*
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30          # ORBmatcher.cc:36-38

EXPORTS = [
    # include/orbx.h
    "orbx_create", "orbx_destroy", "orbx_last_error", "orbx_max_keypoints", "orbx_extract", "orbx_extract_batch",
    "orbx_extract_batch_async", "orbx_sync", "orbx_result_device", "orbx_result_fetch", "orbx_result_fetch_all", "orbx_level_size",
    "orbx_level_image", "orbx_pyramid_fetch", "orbx_pyramid_map", "orbx_scale_tables", "orbx_features_per_level", "orbx_level_candidates",
    "orbx_level_selected", "orbx_last_timings", "orbx_set_stage_timing", "orbx_mean_timings", "orbx_stream_wait_results", "orbx_stream_wait_other", "orbx_guard_results", "orbx_gray_from_color", "orbx_remap_linear", "orbx_clahe", "orbx_algorithmic_bytes", "orbx_blur_in_pass", "orbx_quadtree_threads", "orbx_quadtree_fallbacks", "orbx_blur_form", "orbx_orient_form", "orbx_stream", "orbx_dev_alloc",
    "orbx_dev_free", "orbx_memcpy_h2d", "orbx_memcpy_d2h", "orbx_device_count",
    "orbx_capture_begin", "orbx_capture_end", "orbx_graph_launch", "orbx_result_download_async", "orbx_result_block_layout", "orbx_block_attach", "orbx_block_detach_all", "orbx_download_sync",
    "orbx_host_alloc", "orbx_host_free", "orbx_set_result_block", "orbx_mark", "orbx_mark_elapsed_ms",
    # include/orbm.h
    "orbm_create", "orbm_destroy", "orbm_last_error", "orbm_sync", "orbm_stream", "orbm_set_stream", "orbm_hamming",
    "orbm_three_maxima", "orbm_knn2_batch", "orbm_knn2_batch_async", "orbm_knn2_ratio_batch_async", "orbm_last_timing",
    "orbm_stereo_batch_async", "orbm_bow_nodes_batch_async", "orbm_triangulation_batch_async",
]


class OrbError(RuntimeError):
    pass


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc")] + (["-B"] if force else []))
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise OrbError("liborbslam3_amd.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, ci, i32p = C.c_void_p, C.c_int, C.POINTER(C.c_int32)
        L.orbx_create.argtypes = [C.POINTER(vp), ci, C.c_float, ci, ci, ci, ci, ci, ci, ci]
        L.orbx_destroy.argtypes = [vp]
        L.orbx_last_error.restype = C.c_char_p
        L.orbx_max_keypoints.argtypes = [vp]
        L.orbx_extract.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, i32p]
        L.orbx_extract_batch.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]
        L.orbx_extract_batch_async.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp]
        L.orbx_sync.argtypes = [vp]
        L.orbx_result_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32p]
        L.orbx_result_fetch.argtypes = [vp, ci, vp, vp, ci, i32p]
        L.orbx_result_fetch_all.argtypes = [vp, vp, vp, ci, vp, vp]
        L.orbx_level_size.argtypes = [vp, ci, i32p, i32p]
        L.orbx_level_image.argtypes = [vp, ci, ci, ci, vp, ci]
        L.orbx_scale_tables.argtypes = [vp, vp, vp, vp, vp]
        L.orbx_features_per_level.argtypes = [vp, vp]
        L.orbx_level_candidates.argtypes = [vp, ci, ci, vp, ci]
        L.orbx_level_selected.argtypes = [vp, ci, ci, vp, ci]
        L.orbx_last_timings.argtypes = [vp, vp]
        L.orbx_algorithmic_bytes.restype = C.c_int64
        L.orbx_blur_in_pass.argtypes = [vp]
        L.orbx_quadtree_threads.argtypes = [vp]
        L.orbx_quadtree_fallbacks.argtypes = [vp]
        L.orbx_quadtree_fallbacks.restype = C.c_longlong
        L.orbx_blur_form.argtypes = [vp]
        L.orbx_orient_form.argtypes = [vp]
        L.orbx_algorithmic_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
        L.orbx_mean_timings.argtypes = [vp, vp, i32p]
        L.orbx_stream_wait_results.argtypes = [vp, vp]
        L.orbx_stream_wait_other.argtypes = [vp, vp]
        L.orbx_guard_results.argtypes = [vp, vp]
        L.orbx_set_stage_timing.argtypes = [vp, C.c_int]
        L.orbx_clahe.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, C.c_int]
        L.orbx_remap_linear.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int]
        L.orbx_gray_from_color.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int]
        L.orbx_stream.restype = vp
        L.orbx_stream.argtypes = [vp]
        L.orbx_dev_alloc.restype = vp
        L.orbx_dev_alloc.argtypes = [C.c_size_t]
        L.orbx_dev_free.argtypes = [vp]
        L.orbx_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
        L.orbx_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
        L.orbx_capture_begin.argtypes = [vp, ci]
        L.orbx_capture_end.argtypes = [vp]
        L.orbx_graph_launch.argtypes = [vp, ci]
        L.orbx_result_download_async.argtypes = [vp, vp]
        L.orbx_result_block_layout.argtypes = [vp] + [C.POINTER(C.c_size_t)] * 5
        L.orbx_download_sync.argtypes = [vp]
        L.orbx_block_attach.argtypes = [vp, ci, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.orbx_block_detach_all.argtypes = [vp]
        L.orbx_set_result_block.argtypes = [vp, ci]
        L.orbx_host_alloc.restype = vp
        L.orbx_host_alloc.argtypes = [C.c_size_t]
        L.orbx_host_free.argtypes = [vp]
        L.orbx_mark.argtypes = [vp, ci]
        L.orbx_mark_elapsed_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.orbm_create.argtypes = [C.POINTER(vp), ci]
        L.orbm_destroy.argtypes = [vp]
        L.orbm_last_error.restype = C.c_char_p
        L.orbm_sync.argtypes = [vp]
        L.orbm_stream.restype = vp
        L.orbm_stream.argtypes = [vp]
        L.orbm_set_stream.argtypes = [vp, vp]
        L.orbm_hamming.argtypes = [vp, vp]
        L.orbm_three_maxima.argtypes = [vp, ci, vp]
        L.orbm_knn2_batch.argtypes = [vp, ci, vp, ci, vp, vp, ci, vp, ci, vp, vp]
        L.orbm_knn2_batch_async.argtypes = [vp, vp, ci, vp, vp, ci, vp, ci, ci, vp, vp]
        L.orbm_knn2_ratio_batch_async.argtypes = [vp, vp, ci, vp, vp, ci, vp, ci, C.c_double, vp, vp, vp]
        L.orbm_last_timing.argtypes = [vp, vp]
        L.orbm_stereo_batch_async.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, ci, C.c_float, C.c_float, vp, vp, vp, vp]
        L.orbm_bow_nodes_batch_async.argtypes = [vp, vp, vp, ci, ci, vp]
        L.orbm_triangulation_batch_async.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, ci, ci, ci, vp, vp]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _chk(rc, what):
    if rc < 0:
        L = lib()
        msg = (L.orbx_last_error() or b"").decode() or (L.orbm_last_error() or b"").decode()
        raise OrbError("%s failed with code %d: %s" % (what, rc, msg))
    return rc


class DeviceBuffer:
    """hipMalloc'd bytes owned by Python (keeps tests/bench free of any other HIP binding)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().orbx_dev_alloc(max(1, self.nbytes))
        if not self.ptr:
            raise OrbError("device allocation of %d bytes failed" % nbytes)

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        _chk(lib().orbx_memcpy_h2d(self.ptr + offset, _p(arr), arr.nbytes), "h2d")
        return self

    def download(self, dtype, count, offset=0):
        out = np.empty(count, dtype)
        _chk(lib().orbx_memcpy_d2h(_p(out), self.ptr + offset, out.nbytes), "d2h")
        return out

    def __del__(self):
        try:
            lib().orbx_dev_free(self.ptr)
        except Exception:
            pass


class PinnedBuffer:
    """hipHostMalloc'd bytes with a numpy view (destination of orbx_result_download_async)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().orbx_host_alloc(max(1, self.nbytes))
        if not self.ptr:
            raise OrbError("pinned allocation of %d bytes failed" % nbytes)
        self.bytes = np.ctypeslib.as_array((C.c_uint8 * max(1, self.nbytes)).from_address(self.ptr))

    def view(self, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.bytes[:n].view(dtype).reshape(shape)

    def __del__(self):
        try:
            self.bytes = None
            lib().orbx_host_free(self.ptr)
        except Exception:
            pass


class ORBextractor:
    """ORB_SLAM3::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) on one MI355X.

    __call__(image, lapping) -> (monoIndex, keypoints, descriptors) mirrors operator()
    (src/ORBextractor.cc:1534-1659): keypoints is a structured array with cv::KeyPoint's layout,
    descriptors an (n,32) uint8 array, monoIndex the reference's return value (-1 for an empty image).
    """

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7,
                 device=0, max_size=(752, 480), max_batch=1):
        self.L = lib()
        h = C.c_void_p()
        _chk(self.L.orbx_create(C.byref(h), nfeatures, scale_factor, nlevels, ini_th, min_th, device,
                                int(max_size[0]), int(max_size[1]), int(max_batch)), "orbx_create")
        self.h = h
        self.nfeatures, self.nlevels, self.max_batch = nfeatures, nlevels, max_batch
        self.cap = self.L.orbx_max_keypoints(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.orbx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- getters (include/ORBextractor.h:61-79)
    def GetLevels(self):
        return self.nlevels

    def _tables(self):
        n = self.nlevels
        t = [np.zeros(n, np.float32) for _ in range(4)]
        self.L.orbx_scale_tables(self.h, *[_p(a) for a in t])
        return t

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def GetScaleFactor(self):
        return float(self._tables()[0][1]) if self.nlevels > 1 else 1.0

    def features_per_level(self):
        out = np.zeros(self.nlevels, np.int32)
        self.L.orbx_features_per_level(self.h, _p(out))
        return out

    # ---- operator()
    def __call__(self, image, lapping=(0, 0)):
        if image is None or image.size == 0:
            return -1, None, None
        img = np.ascontiguousarray(image)
        assert img.dtype == np.uint8 and img.ndim == 2, "image must be CV_8UC1"
        h, w = img.shape
        kps = np.zeros(self.cap, KP_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        mono = C.c_int32(0)
        n = _chk(self.L.orbx_extract(self.h, _p(img), w, h, w, int(lapping[0]), int(lapping[1]), _p(kps), _p(desc),
                                     self.cap, C.byref(mono)), "orbx_extract")
        return mono.value, kps[:n].copy(), desc[:n].copy()

    # ---- frame-parallel batch
    def extract_batch(self, images, lapping=None):
        """images: list of equal-size uint8 arrays (host).  Returns list of (mono, kps, desc)."""
        imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        h, w = imgs[0].shape
        ptrs = (C.c_void_p * len(imgs))(*[i.ctypes.data for i in imgs])
        lap = None if lapping is None else np.ascontiguousarray(np.asarray(lapping, np.int32).reshape(-1))
        n_out = np.zeros(len(imgs), np.int32); m_out = np.zeros(len(imgs), np.int32)
        _chk(self.L.orbx_extract_batch(self.h, ptrs, HOST, len(imgs), w, h, w, None if lap is None else _p(lap),
                                       _p(n_out), _p(m_out)), "orbx_extract_batch")
        return self.fetch_all()

    def fetch_all(self):
        """Results of every frame of the last batch with one device-to-host copy per array."""
        B = self.L.orbx_result_fetch_all(self.h, None, None, self.cap, None, None)
        _chk(B, "orbx_result_fetch_all")
        kps = np.zeros((B, self.cap), KP_DTYPE); desc = np.zeros((B, self.cap, 32), np.uint8)
        n = np.zeros(B, np.int32); m = np.zeros(B, np.int32)
        _chk(self.L.orbx_result_fetch_all(self.h, _p(kps), _p(desc), self.cap, _p(n), _p(m)), "orbx_result_fetch_all")
        return [(int(m[i]), kps[i, :n[i]].copy(), desc[i, :n[i]].copy()) for i in range(B)]

    def gray_from_color(self, images, blue_first=False, coef_bits=15):
        """cv::cvtColor(..., COLOR_*2GRAY) of equal-size HxWx{3,4} uint8 host images on the GPU (Tracking.cc:1264-1290).
        Returns (DeviceBuffer, stride): the gray images back to back, usable by enqueue_device / extract."""
        imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        h, w, ch = imgs[0].shape
        stride = (w + 63) // 64 * 64
        buf = DeviceBuffer(stride * h * len(imgs))
        srcs = (C.c_void_p * len(imgs))(*[i.ctypes.data for i in imgs])
        dsts = (C.c_void_p * len(imgs))(*[buf.ptr + k * stride * h for k in range(len(imgs))])
        _chk(self.L.orbx_gray_from_color(self.h, srcs, HOST, len(imgs), w, h, w * ch, ch, 1 if blue_first else 0, int(coef_bits), dsts, stride),
             "orbx_gray_from_color")
        self.sync()                                        # enqueue-only in the C ABI; synced here because callers download the buffer
        return buf, stride

    def clahe(self, images, clip_limit=3.0, tiles=(8, 8)):
        """cv::createCLAHE(clip, Size(tiles))->apply on equal-size uint8 host images, in place on the GPU
        (mono_tum_vi.cc:101-109).  Returns (DeviceBuffer, stride)."""
        imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        h, w = imgs[0].shape
        stride = (w + 63) // 64 * 64
        buf = DeviceBuffer(stride * h * len(imgs))
        pad = np.zeros((h, stride), np.uint8)
        for k, im in enumerate(imgs):
            pad[:, :w] = im
            buf.upload(pad, offset=k * stride * h)
        ptrs = (C.c_void_p * len(imgs))(*[buf.ptr + k * stride * h for k in range(len(imgs))])
        _chk(self.L.orbx_clahe(self.h, ptrs, len(imgs), w, h, stride, float(clip_limit), int(tiles[0]), int(tiles[1]), ptrs, stride), "orbx_clahe")
        self.sync()
        return buf, stride

    def remap_linear(self, images, mapx, mapy):
        """cv::remap(img, M1, M2, INTER_LINEAR) of equal-size uint8 host images on the GPU (stereo_euroc.cc:168-169).
        Returns (DeviceBuffer, stride) with the rectified images back to back."""
        imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        sh, sw = imgs[0].shape
        mx = np.ascontiguousarray(mapx, np.float32); my = np.ascontiguousarray(mapy, np.float32)
        dh, dw = mx.shape
        sstride = (sw + 63) // 64 * 64; dstride = (dw + 63) // 64 * 64
        src = DeviceBuffer(sstride * sh * len(imgs)); dst = DeviceBuffer(dstride * dh * len(imgs))
        pad = np.zeros((sh, sstride), np.uint8)
        for k, im in enumerate(imgs):
            pad[:, :sw] = im
            src.upload(pad, offset=k * sstride * sh)
        dmx = DeviceBuffer(mx.nbytes).upload(mx); dmy = DeviceBuffer(my.nbytes).upload(my)
        sp = (C.c_void_p * len(imgs))(*[src.ptr + k * sstride * sh for k in range(len(imgs))])
        dp = (C.c_void_p * len(imgs))(*[dst.ptr + k * dstride * dh for k in range(len(imgs))])
        _chk(self.L.orbx_remap_linear(self.h, sp, len(imgs), sw, sh, sstride, dmx.ptr, dmy.ptr, dw, dh, dp, dstride), "orbx_remap_linear")
        self.sync()                                        # the source / map buffers above are released when this returns
        return dst, dstride

    def enqueue_device(self, dev_ptrs, w, h, stride, lapping=None):
        """dev_ptrs: ctypes array of device pointers; enqueue only (bench hot loop)."""
        lap = None if lapping is None else np.ascontiguousarray(np.asarray(lapping, np.int32).reshape(-1))
        self._keep = (dev_ptrs, lap)
        _chk(self.L.orbx_extract_batch_async(self.h, dev_ptrs, DEVICE, len(dev_ptrs), w, h, stride,
                                             None if lap is None else _p(lap)), "orbx_extract_batch_async")

    def sync(self):
        _chk(self.L.orbx_sync(self.h), "orbx_sync")

    def fetch(self, i):
        kps = np.zeros(self.cap, KP_DTYPE); desc = np.zeros((self.cap, 32), np.uint8)
        mono = C.c_int32(0)
        n = _chk(self.L.orbx_result_fetch(self.h, i, _p(kps), _p(desc), self.cap, C.byref(mono)), "orbx_result_fetch")
        return mono.value, kps[:n].copy(), desc[:n].copy()

    def result_block_layout(self):
        """(off_kps, off_desc, off_counts, off_monos, bytes) of a result block (include/orbx.h: orbx_result_block_layout)."""
        v = [C.c_size_t() for _ in range(5)]
        _chk(self.L.orbx_result_block_layout(self.h, *[C.byref(x) for x in v]), "result_block_layout")
        return tuple(int(x.value) for x in v)

    def result_device(self):
        k, d, c, m = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        cap = C.c_int32()
        _chk(self.L.orbx_result_device(self.h, C.byref(k), C.byref(d), C.byref(c), C.byref(m), C.byref(cap)), "result_device")
        return dict(kps=k.value, desc=d.value, counts=c.value, monos=m.value, cap=cap.value)

    # ---- stage introspection
    def level_size(self, level):
        w, h = C.c_int32(), C.c_int32()
        _chk(self.L.orbx_level_size(self.h, level, C.byref(w), C.byref(h)), "level_size")
        return w.value, h.value

    def level_image(self, level, frame=0, blurred=False):
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        _chk(self.L.orbx_level_image(self.h, frame, level, int(blurred), _p(out), w), "level_image")
        return out

    def pyramid(self, frame=0):
        """every unblurred level of one frame with one call (orbx_pyramid_fetch)."""
        outs = [np.zeros(self.level_size(l)[::-1], np.uint8) for l in range(self.GetLevels())]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        strides = (C.c_int * len(outs))(*[o.shape[1] for o in outs])
        self.L.orbx_pyramid_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _chk(self.L.orbx_pyramid_fetch(self.h, frame, ptrs, strides), "pyramid_fetch")
        return outs

    def pyramid_views(self, frame=0):
        """zero-copy views of every level in the handle's pinned memory (orbx_pyramid_map); valid until the next call on the handle."""
        n = self.GetLevels()
        ptrs = (C.c_void_p * n)(); pitch = (C.c_int * n)()
        self.L.orbx_pyramid_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _chk(self.L.orbx_pyramid_map(self.h, frame, ptrs, pitch), "pyramid_map")
        out = []
        for l in range(n):
            w, h = self.level_size(l)
            if not ptrs[l]:
                out.append(None); continue
            buf = (C.c_uint8 * (pitch[l] * h)).from_address(ptrs[l])
            out.append(np.frombuffer(buf, np.uint8).reshape(h, pitch[l])[:, :w])
        return out

    def level_candidates(self, level, frame=0):
        n = _chk(self.L.orbx_level_candidates(self.h, frame, level, None, 0), "level_candidates")
        out = np.zeros((max(n, 1), 3), np.int32)
        self.L.orbx_level_candidates(self.h, frame, level, _p(out), n)
        return out[:n]

    def level_selected(self, level, frame=0):
        n = _chk(self.L.orbx_level_selected(self.h, frame, level, None, 0), "level_selected")
        out = np.zeros((max(n, 1), 3), np.int32)
        self.L.orbx_level_selected(self.h, frame, level, _p(out), n)
        return out[:n]

    def timings(self):
        t = np.zeros(8, np.float32)
        _chk(self.L.orbx_last_timings(self.h, _p(t)), "timings")
        return dict(zip(["pyramid", "fast", "quadtree", "slots", "blur", "orient_desc", "total", "pyramid_fast_span"], t.tolist()))

    def mean_timings(self):
        t = np.zeros(8, np.float32); n = C.c_int32()
        _chk(self.L.orbx_mean_timings(self.h, _p(t), C.byref(n)), "mean_timings")
        return dict(zip(["pyramid", "fast", "quadtree", "slots", "blur", "orient_desc", "total", "pyramid_fast_span"], t.tolist())), n.value

    def blur_in_pass(self):
        """True when the blur is scheduled inside the pyramid+FAST pass (include/orbx.h: orbx_blur_in_pass)."""
        return bool(self.L.orbx_blur_in_pass(self.h))

    def quadtree_threads(self):
        """Workgroup size of the last batch's quadtree: 1024 / 256, 0 = the A/B library's k_quadtree (include/orbx.h)."""
        return int(self.L.orbx_quadtree_threads(self.h))

    def quadtree_fallbacks(self):
        """(frame, level) quadtrees that left table mode for passes over their candidates, cumulative since the handle was made; waits
        for the extractor's stream (include/orbx.h: orbx_quadtree_fallbacks)."""
        n = int(self.L.orbx_quadtree_fallbacks(self.h))
        if n < 0:
            raise OrbError("orbx_quadtree_fallbacks: %d %s" % (n, self.L.orbx_last_error().decode()))
        return n

    def blur_form(self):
        """Form of the last batch's blur: 0 one-tile k_blur3, 1 walking k_blur3, 2 = the A/B library's k_blur2, -1 before any batch (include/orbx.h)."""
        return int(self.L.orbx_blur_form(self.h))

    def orient_form(self):
        """Form of the last batch's orientation and descriptor kernel: 0 k_orient_desc2 on tiled blurred levels, 1 k_orient_desc2 on
        row-major ones, 2 = the A/B library's k_orient_desc, -1 before any batch (include/orbx.h)."""
        return int(self.L.orbx_orient_form(self.h))

    def algorithmic_bytes(self):
        f = C.c_int64()
        a = self.L.orbx_algorithmic_bytes(self.h, C.byref(f))
        return int(a), int(f.value)


class ORBmatcher:
    """Flattened-array form of ORB_SLAM3::ORBmatcher (include/ORBmatcher.h:35-111)."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = TH_HIGH, TH_LOW, HISTO_LENGTH

    def __init__(self, nnratio=0.6, check_ori=True, device=0):
        self.L = lib()
        self.nnratio, self.check_ori = float(nnratio), bool(check_ori)
        h = C.c_void_p()
        _chk(self.L.orbm_create(C.byref(h), device), "orbm_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.orbm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
        return lib().orbm_hamming(_p(a), _p(b))

    @staticmethod
    def ComputeThreeMaxima(bin_sizes):
        c = np.ascontiguousarray(bin_sizes, np.int32); out = np.zeros(3, np.int32)
        lib().orbm_three_maxima(_p(c), c.shape[0], _p(out))
        return out

    def knn2(self, q, t):
        """2-NN of every row of q among the rows of t (BFMatcher.knnMatch k=2, Frame.cc:1458)."""
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        nq = np.array([q.shape[0]], np.int32); nt = np.array([t.shape[0]], np.int32)
        idx = np.zeros((max(q.shape[0], 1), 2), np.int32); dist = np.zeros_like(idx)
        if q.shape[0] == 0:
            return idx[:0], dist[:0]
        tt = t if t.shape[0] else np.zeros((1, 32), np.uint8)
        _chk(self.L.orbm_knn2_batch(self.h, HOST, _p(q), q.shape[0], _p(nq), _p(tt), tt.shape[0], _p(nt), 1,
                                    _p(idx), _p(dist)), "orbm_knn2_batch")
        return idx, dist

    def sync(self):
        _chk(self.L.orbm_sync(self.h), "orbm_sync")

    def timing_ms(self):
        t = C.c_float()
        _chk(self.L.orbm_last_timing(self.h, C.byref(t)), "orbm_last_timing")
        return t.value


# ---------------------------------------------------------------------------------------------------------------
# Flattened Frame / KeyFrame views for the searches (include/orbm.h).  FrameView mirrors the members of
# ORB_SLAM3::Frame the matcher reads: mvKeysUn, mDescriptors, mvuRight, mGrid + bounds (include/Frame.h).
# ---------------------------------------------------------------------------------------------------------------
GRID_COLS, GRID_ROWS = 64, 48


class _CFrame(C.Structure):
    _fields_ = [("n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("uright", C.c_void_p),
                ("min_x", C.c_float), ("min_y", C.c_float), ("inv_w", C.c_float), ("inv_h", C.c_float),
                ("grid_start", C.c_void_p), ("grid_idx", C.c_void_p)]


PAIR_GATE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int)      # orbm_pair_gate_fn (include/orbm.h)


def _bind_search(L, prefix):
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    g = lambda n: getattr(L, prefix + n)
    h = [vp] if prefix == "orbm_" else []
    g("grid_build").argtypes = h + [vp, ci, cf, cf, cf, cf, vp, vp]
    g("search_by_projection_frame").argtypes = h + [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, ci, ci, cf, ci, vp]
    g("search_by_projection_points").argtypes = h + [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, cf, vp]
    g("search_for_initialization").argtypes = h + [vp, vp, vp, ci, cf, ci, vp]
    g("search_for_triangulation").argtypes = h + [ci, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp,
                                                  vp, cf, cf, vp, vp, ci, ci, ci, vp]
    g("search_by_bow").argtypes = h + [ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, cf, ci, vp]
    g("search_for_triangulation_legacy").argtypes = g("search_for_triangulation").argtypes
    g("search_for_triangulation_gated").argtypes = h + [ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, PAIR_GATE, vp, ci, vp]
    g("search_by_projection_kf").argtypes = h + [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, cf, ci, ci, vp]
    g("search_by_projection_sim3").argtypes = h + [vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, cf, vp]
    g("search_by_projection_frame_fisheye").argtypes = h + [vp, vp, vp, vp, vp, ci] + [vp] * 9 + [cf, ci, ci, ci, vp, vp]
    g("search_by_projection_points_fisheye").argtypes = h + [vp] * 7 + [ci] + [vp] * 12 + [cf, cf, vp, vp]
    g("search_by_bow_fisheye").argtypes = h + [ci, vp, vp, vp, ci, vp, vp, vp, ci, ci, vp, vp, ci, vp, vp, vp, cf, ci, vp]
    g("search_by_sim3").argtypes = h + [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, cf, vp]
    g("fuse").argtypes = h + [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, cf, ci, vp]
    g("search_by_bow_kf").argtypes = h + [ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, cf, ci, vp]


class FrameView:
    """Plain-array view of a Frame; `backend` is an object exposing grid_build (ORBmatcher here, the oracle in tests)."""

    def __init__(self, kps, desc, width, height, uright=None, backend=None):
        self.kps = np.ascontiguousarray(kps); self.desc = np.ascontiguousarray(desc, np.uint8)
        self.n = len(self.kps)
        self.uright = None if uright is None else np.ascontiguousarray(uright, np.float32)
        # undistortion-free bounds (Frame::ComputeImageBounds with k1 == 0, Frame.cc:1005-1021)
        self.min_x, self.min_y = np.float32(0), np.float32(0)
        self.inv_w = np.float32(GRID_COLS) / (np.float32(width) - self.min_x)
        self.inv_h = np.float32(GRID_ROWS) / (np.float32(height) - self.min_y)
        self.grid_start = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int32)
        self.grid_idx = np.zeros(max(self.n, 1), np.int32)
        if backend is not None:
            backend.grid_build(self)

    def cstruct(self):
        return _CFrame(self.n, self.kps.ctypes.data, self.desc.ctypes.data,
                       None if self.uright is None else self.uright.ctypes.data,
                       float(self.min_x), float(self.min_y), float(self.inv_w), float(self.inv_h),
                       self.grid_start.ctypes.data, self.grid_idx.ctypes.data)


class ResidentFrame:
    """A Frame kept in HBM across searches (include/orbm.h: orbm_frame_create).  `view` is a FrameView (host arrays are
    uploaded once) or a dict of device pointers (kps, desc, n -- e.g. one frame of an extractor's result block, adopted in place)."""

    def __init__(self, matcher, view=None, device=None, width=752, height=480, uright=None):
        L = lib()
        L.orbm_frame_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_void_p)]
        L.orbm_frame_destroy.argtypes = [C.c_void_p]
        L.orbm_frame_size.argtypes = [C.c_void_p]
        rf = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.orbm_search_by_projection_frame_resident.argtypes = rf + [C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
        L.orbm_search_by_projection_points_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_float, C.c_float, C.c_void_p]
        self.L, self.m = L, matcher
        h = C.c_void_p()
        if view is not None:
            self.n = view.n
            self._keep = view
            _chk(L.orbm_frame_create(matcher.h, HOST, view.n, _p(view.kps), _p(view.desc), None if view.uright is None else _p(view.uright),
                                     float(view.min_x), float(view.min_y), float(view.inv_w), float(view.inv_h), C.byref(h)), "orbm_frame_create")
        else:
            self.n = int(device["n"])
            inv_w = np.float32(GRID_COLS) / np.float32(width); inv_h = np.float32(GRID_ROWS) / np.float32(height)
            _chk(L.orbm_frame_create(matcher.h, DEVICE, self.n, device["kps"], device["desc"], uright, 0.0, 0.0, float(inv_w), float(inv_h), C.byref(h)),
                 "orbm_frame_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.orbm_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def feature_vector_csr(node_of_feature):
    """DBoW2::FeatureVector (map<NodeId, vector<unsigned>>) as CSR: nodes ascending, features ascending inside."""
    node_of_feature = np.asarray(node_of_feature, np.int64)
    order = np.argsort(node_of_feature, kind="stable").astype(np.int32)
    nodes, counts = np.unique(node_of_feature, return_counts=True)
    start = np.zeros(len(nodes) + 1, np.int32); start[1:] = np.cumsum(counts)
    return nodes.astype(np.int32), start, order


class _SearchMixin:
    """Search entry points shared by the product matcher and (in tests) the oracle wrapper: same argument lists."""
    _prefix = "orbm_"

    def _call(self, name, *args):
        f = getattr(self.L, self._prefix + name)
        a = ([self.h] if self._prefix == "orbm_" else []) + list(args)
        rc = f(*a)
        if rc < 0 and self._prefix == "orbm_":
            _chk(rc, name)
        return rc

    def grid_build(self, fv):
        fv.placed = self._call("grid_build", _p(fv.kps), fv.n, float(fv.min_x), float(fv.min_y), float(fv.inv_w), float(fv.inv_h),
                                _p(fv.grid_start), _p(fv.grid_idx))
        return fv.placed

    def SearchByProjectionFrame(self, cur, cur_blocked, scale_factors, valid, u, v, invzc, octave, angle, qdesc, mp_obs,
                                th, forward=False, backward=False, mbf=0.0, check_ori=True):
        match = np.full(cur.n, -1, np.int32)
        cs = cur.cstruct()
        arr = [np.ascontiguousarray(a, t) for a, t in ((cur_blocked, np.uint8), (scale_factors, np.float32), (valid, np.uint8),
               (u, np.float32), (v, np.float32), (invzc, np.float32), (octave, np.int32), (angle, np.float32),
               (qdesc, np.uint8), (mp_obs, np.uint8))]
        n = self._call("search_by_projection_frame", C.byref(cs), _p(arr[0]), _p(arr[1]), len(arr[2]), *[_p(a) for a in arr[2:]],
                       float(th), int(forward), int(backward), float(mbf), int(check_ori), _p(match))
        return n, match

    def SearchByProjectionFrameResident(self, cur, cur_blocked, scale_factors, valid, u, v, invzc, octave, angle, qdesc, mp_obs,
                                        th, forward=False, backward=False, mbf=0.0, check_ori=True):
        """M4 against a ResidentFrame: only the queries travel (include/orbm.h: orbm_search_by_projection_frame_resident)."""
        match = np.full(cur.n, -1, np.int32)
        arr = [np.ascontiguousarray(a, t) for a, t in ((cur_blocked, np.uint8), (scale_factors, np.float32), (valid, np.uint8),
               (u, np.float32), (v, np.float32), (invzc, np.float32), (octave, np.int32), (angle, np.float32),
               (qdesc, np.uint8), (mp_obs, np.uint8))]
        n = self._call("search_by_projection_frame_resident", cur.h, _p(arr[0]), _p(arr[1]), len(arr[2]), *[_p(a) for a in arr[2:]],
                       float(th), int(forward), int(backward), float(mbf), int(check_ori), _p(match))
        return n, match

    def SearchByProjectionPointsResident(self, f, blocked, scale_factors, in_view, px, py, pxr, view_cos, level, qdesc, mp_obs, th, nnratio):
        match = np.full(f.n, -1, np.int32)
        arr = [np.ascontiguousarray(a, t) for a, t in ((blocked, np.uint8), (scale_factors, np.float32), (in_view, np.uint8),
               (px, np.float32), (py, np.float32), (pxr, np.float32), (view_cos, np.float32), (level, np.int32),
               (qdesc, np.uint8), (mp_obs, np.uint8))]
        n = self._call("search_by_projection_points_resident", f.h, _p(arr[0]), _p(arr[1]), len(arr[2]), *[_p(a) for a in arr[2:]],
                       float(th), float(nnratio), _p(match))
        return n, match

    def SearchByProjectionPoints(self, f, blocked, scale_factors, in_view, px, py, pxr, view_cos, level, qdesc, mp_obs, th, nnratio):
        match = np.full(f.n, -1, np.int32)
        cs = f.cstruct()
        arr = [np.ascontiguousarray(a, t) for a, t in ((blocked, np.uint8), (scale_factors, np.float32), (in_view, np.uint8),
               (px, np.float32), (py, np.float32), (pxr, np.float32), (view_cos, np.float32), (level, np.int32),
               (qdesc, np.uint8), (mp_obs, np.uint8))]
        n = self._call("search_by_projection_points", C.byref(cs), _p(arr[0]), _p(arr[1]), len(arr[2]), *[_p(a) for a in arr[2:]],
                       float(th), float(nnratio), _p(match))
        return n, match

    def SearchForInitialization(self, f1, f2, prev_matched, window, nnratio, check_ori=True):
        prev = np.ascontiguousarray(prev_matched, np.float32).copy()
        m12 = np.full(f1.n, -1, np.int32)
        c1, c2 = f1.cstruct(), f2.cstruct()
        n = self._call("search_for_initialization", C.byref(c1), C.byref(c2), _p(prev), int(window), float(nnratio), int(check_ori), _p(m12))
        return n, m12, prev

    def SearchByProjectionKF(self, cur, blocked, scale_factors, valid, u, v, level, angle, qdesc, th, orb_dist, check_ori=True):
        match = np.full(cur.n, -1, np.int32)
        cs = cur.cstruct()
        arr = [np.ascontiguousarray(a, t) for a, t in ((blocked, np.uint8), (scale_factors, np.float32), (valid, np.uint8),
               (u, np.float32), (v, np.float32), (level, np.int32), (angle, np.float32), (qdesc, np.uint8))]
        n = self._call("search_by_projection_kf", C.byref(cs), _p(arr[0]), _p(arr[1]), len(arr[2]), *[_p(a) for a in arr[2:]],
                       float(th), int(orb_dist), int(check_ori), _p(match))
        return n, match

    def SearchByProjectionSim3(self, kf, matched_in, scale_factors, valid, u, v, level, qdesc, th, ratio_hamming):
        match = np.full(kf.n, -1, np.int32)
        cs = kf.cstruct()
        arr = [np.ascontiguousarray(a, t) for a, t in ((matched_in, np.uint8), (scale_factors, np.float32), (valid, np.uint8),
               (u, np.float32), (v, np.float32), (level, np.int32), (qdesc, np.uint8))]
        n = self._call("search_by_projection_sim3", C.byref(cs), _p(arr[0]), _p(arr[1]), len(arr[2]), *[_p(a) for a in arr[2:]],
                       int(th), float(ratio_hamming), _p(match))
        return n, match

    def SearchByProjectionFrameFisheye(self, cur_l, cur_r, blocked_l, blocked_r, scale_factors, valid, u, v, ur, vr, octave, angle,
                                       qdesc, mp_obs, th, forward=False, backward=False, check_ori=True):
        ml = np.full(cur_l.n, -1, np.int32); mr = np.full(cur_r.n, -1, np.int32)
        cl, cr = cur_l.cstruct(), cur_r.cstruct()
        arr = [np.ascontiguousarray(a, t) for a, t in ((blocked_l, np.uint8), (blocked_r, np.uint8), (scale_factors, np.float32),
               (valid, np.uint8), (u, np.float32), (v, np.float32), (ur, np.float32), (vr, np.float32), (octave, np.int32),
               (angle, np.float32), (qdesc, np.uint8), (mp_obs, np.uint8))]
        n = self._call("search_by_projection_frame_fisheye", C.byref(cl), C.byref(cr), _p(arr[0]), _p(arr[1]), _p(arr[2]), len(arr[3]),
                       *[_p(a) for a in arr[3:]], float(th), int(forward), int(backward), int(check_ori), _p(ml), _p(mr))
        return n, ml, mr

    def SearchByProjectionPointsFisheye(self, f_l, f_r, blocked_l, blocked_r, l2r, r2l, scale_factors, left, right, qdesc, mp_obs, th, nnratio):
        """left / right: dicts with in_view, px, py, view_cos, level for the two cameras."""
        ml = np.full(f_l.n, -1, np.int32); mr = np.full(f_r.n, -1, np.int32)
        cl, cr = f_l.cstruct(), f_r.cstruct()
        def pack(q):
            return [np.ascontiguousarray(q["in_view"], np.uint8), np.ascontiguousarray(q["px"], np.float32), np.ascontiguousarray(q["py"], np.float32),
                    np.ascontiguousarray(q["view_cos"], np.float32), np.ascontiguousarray(q["level"], np.int32)]
        a = [np.ascontiguousarray(blocked_l, np.uint8), np.ascontiguousarray(blocked_r, np.uint8), np.ascontiguousarray(l2r, np.int32),
             np.ascontiguousarray(r2l, np.int32), np.ascontiguousarray(scale_factors, np.float32)]
        L_, R_ = pack(left), pack(right)
        qd = np.ascontiguousarray(qdesc, np.uint8); ob = np.ascontiguousarray(mp_obs, np.uint8)
        n = self._call("search_by_projection_points_fisheye", C.byref(cl), C.byref(cr), *[_p(x) for x in a], len(L_[0]),
                       *[_p(x) for x in L_], *[_p(x) for x in R_], _p(qd), _p(ob), float(th), float(nnratio), _p(ml), _p(mr))
        return n, ml, mr

    def SearchByBoWFisheye(self, kkf, dkf, kf_good, fvk, kf_, df, nleft, fvf, nnratio, check_ori=True):
        fm = np.full(len(kf_), -1, np.int32)
        kkf = np.ascontiguousarray(kkf); kf_ = np.ascontiguousarray(kf_)
        dkf = np.ascontiguousarray(dkf, np.uint8); df = np.ascontiguousarray(df, np.uint8)
        good = np.ascontiguousarray(kf_good, np.uint8)
        n = self._call("search_by_bow_fisheye", len(kkf), _p(kkf), _p(dkf), _p(good), len(fvk[0]), _p(fvk[0]), _p(fvk[1]), _p(fvk[2]),
                       len(kf_), int(nleft), _p(kf_), _p(df), len(fvf[0]), _p(fvf[0]), _p(fvf[1]), _p(fvf[2]),
                       float(nnratio), int(check_ori), _p(fm))
        return n, fm

    def SearchByBoWFisheyeBatchAsync(self, npairs, nkf_rows, cap_kf, kps_kf, desc_kf, counts_kf, node_kf, weight_kf, good_kf,
                                     nf_rows, cap_f, kps_f, desc_f, counts_f, node_f, weight_f, kf_row, fl_row, fr_row, nnratio, check_ori,
                                     f_match_l, f_match_r, nmatches):
        """SearchByBoWFisheye for a batch, enqueue only: every array argument is a device pointer (include/orbm.h:
        orbm_search_by_bow_fisheye_batch_async).  The product only: the oracle has the single-pair form alone."""
        return _chk(self.L.orbm_search_by_bow_fisheye_batch_async(self.h, npairs, nkf_rows, cap_kf, kps_kf, desc_kf, counts_kf, node_kf, weight_kf, good_kf,
                                                                  nf_rows, cap_f, kps_f, desc_f, counts_f, node_f, weight_f, kf_row, fl_row, fr_row,
                                                                  float(nnratio), int(check_ori), f_match_l, f_match_r, nmatches),
                    "orbm_search_by_bow_fisheye_batch_async")

    def SearchBySim3(self, kf1, kf2, sf1, sf2, q1, q2, th):
        """q1 / q2: dicts with valid, u, v, level, qdesc for the KF1->KF2 and KF2->KF1 projections."""
        m12 = np.full(kf1.n, -1, np.int32)
        c1, c2 = kf1.cstruct(), kf2.cstruct()
        s1 = np.ascontiguousarray(sf1, np.float32); s2 = np.ascontiguousarray(sf2, np.float32)
        def pack(q):
            return [np.ascontiguousarray(q["valid"], np.uint8), np.ascontiguousarray(q["u"], np.float32), np.ascontiguousarray(q["v"], np.float32),
                    np.ascontiguousarray(q["level"], np.int32), np.ascontiguousarray(q["qdesc"], np.uint8)]
        a1, a2 = pack(q1), pack(q2)
        n = self._call("search_by_sim3", C.byref(c1), C.byref(c2), _p(s1), _p(s2), *[_p(a) for a in a1], *[_p(a) for a in a2], float(th), _p(m12))
        return n, m12

    def Fuse(self, kf, scale_factors, inv_sigma2, valid, u, v, ur, level, qdesc, th, chi2_gate=True):
        best = np.full(len(valid), -1, np.int32)
        cs = kf.cstruct()
        arr = [np.ascontiguousarray(a, t) for a, t in ((scale_factors, np.float32), (inv_sigma2, np.float32), (valid, np.uint8),
               (u, np.float32), (v, np.float32), (ur, np.float32), (level, np.int32), (qdesc, np.uint8))]
        n = self._call("fuse", C.byref(cs), _p(arr[0]), _p(arr[1]), len(arr[2]), *[_p(a) for a in arr[2:]],
                       float(th), int(chi2_gate), _p(best))
        return n, best

    def SearchByBoWKF(self, k1, d1, good1, fv1, k2, d2, good2, fv2, nnratio, check_ori=True):
        m12 = np.full(len(k1), -1, np.int32)
        k1 = np.ascontiguousarray(k1); k2 = np.ascontiguousarray(k2)
        d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
        g1 = np.ascontiguousarray(good1, np.uint8); g2 = np.ascontiguousarray(good2, np.uint8)
        n = self._call("search_by_bow_kf", len(k1), _p(k1), _p(d1), _p(g1), len(fv1[0]), _p(fv1[0]), _p(fv1[1]), _p(fv1[2]),
                       len(k2), _p(k2), _p(d2), _p(g2), len(fv2[0]), _p(fv2[0]), _p(fv2[1]), _p(fv2[2]),
                       float(nnratio), int(check_ori), _p(m12))
        return n, m12

    def SearchForTriangulation(self, k1, d1, has_mp1, ur1, fv1, k2, d2, has_mp2, ur2, fv2, F12, ep, sf2, sigma2_2,
                               only_stereo=False, coarse=False, check_ori=False, legacy=False):
        m12 = np.full(len(k1), -1, np.int32)
        k1 = np.ascontiguousarray(k1); k2 = np.ascontiguousarray(k2)
        d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
        h1 = np.ascontiguousarray(has_mp1, np.uint8); h2 = np.ascontiguousarray(has_mp2, np.uint8)
        u1 = None if ur1 is None else np.ascontiguousarray(ur1, np.float32)
        u2 = None if ur2 is None else np.ascontiguousarray(ur2, np.float32)
        F = np.ascontiguousarray(F12, np.float32).reshape(9); sf2 = np.ascontiguousarray(sf2, np.float32)
        sg = np.ascontiguousarray(sigma2_2, np.float32)
        n = self._call("search_for_triangulation_legacy" if legacy else "search_for_triangulation", len(k1), _p(k1), _p(d1), _p(h1), None if u1 is None else _p(u1),
                       len(fv1[0]), _p(fv1[0]), _p(fv1[1]), _p(fv1[2]),
                       len(k2), _p(k2), _p(d2), _p(h2), None if u2 is None else _p(u2),
                       len(fv2[0]), _p(fv2[0]), _p(fv2[1]), _p(fv2[2]),
                       _p(F), float(ep[0]), float(ep[1]), _p(sf2), _p(sg), int(only_stereo), int(coarse), int(check_ori), _p(m12))
        return n, m12

    def SearchForTriangulationGated(self, k1, d1, has_mp1, fv1, k2, d2, has_mp2, fv2, gate, check_ori=False):
        """M10 with a second camera / M12 (ORBmatcher.cc:1388-1629, 1632-1821): `gate(idx1, idx2) -> bool` stands for the
        camera model's epipolarConstrain_ / matchAndtriangulate and is called where the reference calls it."""
        m12 = np.full(len(k1), -1, np.int32)
        k1 = np.ascontiguousarray(k1); k2 = np.ascontiguousarray(k2)
        d1 = np.ascontiguousarray(d1, np.uint8); d2 = np.ascontiguousarray(d2, np.uint8)
        h1 = np.ascontiguousarray(has_mp1, np.uint8); h2 = np.ascontiguousarray(has_mp2, np.uint8)
        cb = PAIR_GATE(lambda user, a, b: int(bool(gate(a, b))))
        n = self._call("search_for_triangulation_gated", len(k1), _p(k1), _p(d1), _p(h1), len(fv1[0]), _p(fv1[0]), _p(fv1[1]), _p(fv1[2]),
                       len(k2), _p(k2), _p(d2), _p(h2), len(fv2[0]), _p(fv2[0]), _p(fv2[1]), _p(fv2[2]), cb, None, int(check_ori), _p(m12))
        return n, m12

    def SearchByBoW(self, kkf, dkf, kf_good, fvk, kf_, df, fvf, nnratio, check_ori=True):
        fm = np.full(len(kf_), -1, np.int32)
        kkf = np.ascontiguousarray(kkf); kf_ = np.ascontiguousarray(kf_)
        dkf = np.ascontiguousarray(dkf, np.uint8); df = np.ascontiguousarray(df, np.uint8)
        good = np.ascontiguousarray(kf_good, np.uint8)
        n = self._call("search_by_bow", len(kkf), _p(kkf), _p(dkf), _p(good), len(fvk[0]), _p(fvk[0]), _p(fvk[1]), _p(fvk[2]),
                       len(kf_), _p(kf_), _p(df), len(fvf[0]), _p(fvf[0]), _p(fvf[1]), _p(fvf[2]),
                       float(nnratio), int(check_ori), _p(fm))
        return n, fm


def _install_search():
    L = lib()
    _bind_search(L, "orbm_")
    L.orbm_window_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 3
    L.orbm_stereo_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    for name in ("grid_build", "SearchByProjectionFrame", "SearchByProjectionPoints", "SearchForInitialization",
                 "SearchForTriangulation", "SearchForTriangulationGated", "SearchByBoW", "SearchByProjectionKF", "SearchByBoWKF", "SearchByProjectionSim3", "Fuse", "SearchBySim3", "SearchByProjectionFrameFisheye",
                 "SearchByProjectionPointsFisheye", "SearchByBoWFisheye", "SearchByBoWFisheyeBatchAsync", "SearchByProjectionFrameResident", "SearchByProjectionPointsResident", "_call"):
        setattr(ORBmatcher, name, getattr(_SearchMixin, name))
    ORBmatcher._prefix = "orbm_"

    def window_candidates(self, f, qx, qy, qr, min_level, max_level, qdesc, cap, q_ur=None, q_er=None):
        nq = len(qx)
        arr = [np.ascontiguousarray(a, t) for a, t in ((qx, np.float32), (qy, np.float32), (qr, np.float32),
               (min_level, np.int32), (max_level, np.int32))]
        ur = None if q_ur is None else np.ascontiguousarray(q_ur, np.float32)
        er = None if q_er is None else np.ascontiguousarray(q_er, np.float32)
        qd = np.ascontiguousarray(qdesc, np.uint8)
        cnt = np.zeros(nq, np.int32); idx = np.zeros((nq, cap), np.int32); dist = np.zeros((nq, cap), np.int32)
        cs = f.cstruct()
        _chk(self.L.orbm_window_candidates(self.h, C.byref(cs), nq, *[_p(a) for a in arr], None if ur is None else _p(ur),
                                           None if er is None else _p(er), _p(qd), cap, _p(cnt), _p(idx), _p(dist)), "window_candidates")
        return cnt, idx, dist

    def stereo_matches(self, ex_left, ex_right, kl, dl, kr, dr, mb, mbf, frame_l=0, frame_r=0):
        kl = np.ascontiguousarray(kl); kr = np.ascontiguousarray(kr)
        dl = np.ascontiguousarray(dl, np.uint8); dr = np.ascontiguousarray(dr, np.uint8)
        ur = np.zeros(max(len(kl), 1), np.float32); dp = np.zeros(max(len(kl), 1), np.float32)
        n = _chk(self.L.orbm_stereo_matches(self.h, ex_left.h, frame_l, ex_right.h, frame_r, len(kl), _p(kl), _p(dl), len(kr), _p(kr), _p(dr),
                                            float(mb), float(mbf), _p(ur), _p(dp)), "stereo_matches")
        return n, ur[:len(kl)], dp[:len(kl)]

    L.orbm_grid_build_batch_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                              C.c_float, C.c_void_p, C.c_void_p]
    L.orbm_track_window_batch_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float,
                                                C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.orbm_search_by_projection_batch_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                        C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float,
                                                        C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                                        C.c_void_p, C.c_void_p]
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.orbm_search_by_projection_points_batch_async.argtypes = [vp, vp, vp, vp, ci, vp, vp, cf, cf, cf, cf, ci, ci,   # block, grid, bounds, frames
                                                               vp, vp, vp, ci,                                  # uright, t_blocked, nq, q_stride
                                                               vp, vp, vp, vp, vp, vp, vp, cf,                  # frustum rows, depth, th_far
                                                               vp, vp, ci, cf, cf, vp, ci, vp, vp]
    L.orbm_search_by_projection_frame_batch_async.argtypes = [vp, vp, vp, vp, ci, vp, vp, cf, cf, cf, cf, ci, ci,   # block, grid, bounds, pairs
                                                              vp, cf, vp, vp, vp, ci,                          # uright, mbf, t_blocked, dir, nq, q_stride
                                                              vp, vp, vp, vp, vp, vp, vp, vp,                  # valid, u, v, invzc, octave, angle, qdesc, mp_obs
                                                              cf, ci, vp, ci, ci, vp, vp, vp]                  # th, retry_below, sf, nlevels, check_ori, outputs
    L.orbm_search_by_projection_frame_fisheye_batch_async.argtypes = [vp, vp, vp, vp, ci, vp, vp, cf, cf, cf, cf, ci, ci, ci,   # pool, grid, bounds, first_l, first_r, pairs
                                                                      vp, vp, vp, vp, ci, vp,                       # blocked_l, blocked_r, dir, nq, q_stride, valid
                                                                      vp, vp, vp, vp, vp, vp, vp, vp,               # u, v, ur, vr, octave, angle, qdesc, mp_obs
                                                                      cf, ci, vp, ci, ci, vp, vp, vp, vp]           # th, retry_below, sf, nlevels, check_ori, outputs
    L.orbm_search_by_projection_points_fisheye_batch_async.argtypes = [vp, vp, vp, vp, ci, vp, vp, cf, cf, cf, cf, ci, ci, ci,   # pool, grid, bounds, first_l, first_r, pairs
                                                                       vp, vp, vp, vp, vp, ci,                       # blocked_l, blocked_r, l2r, r2l, nq, q_stride
                                                                       vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,       # the left, then the right frustum rows
                                                                       vp, cf, vp, vp, ci,                           # depth, th_far, qdesc, mp_obs, q_shared
                                                                       cf, cf, vp, ci, vp, vp, vp]                   # th, nnratio, sf, nlevels, outputs
    L.orbm_project_last_frame_batch_async.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, cf, ci, vp, vp, vp, vp, vp]
    L.orbm_fuse_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp,                 # pairs, KF pool (kps, desc, uright)
                                        vp, vp, cf, cf, cf, cf, vp, vp, vp,         # grid, bounds, kf_row, tcw, ow
                                        vp, ci, vp, vp, vp, vp, vp, vp, ci,         # nq, q_stride, valid, pw, normal, min/max dist, qdesc, q_shared
                                        vp, vp, cf, cf, ci, vp, vp, cf, ci,         # k, bounds, bf, th, chi2_gate, sf, inv_sigma2, log sf, nlevels
                                        vp, vp, vp]                                 # best_idx, nfused, level_out
    L.orbm_search_by_projection_kf_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp,          # pairs, frame pool (kps, desc, counts)
                                                           vp, vp, cf, cf, cf, cf, vp, vp, vp, vp,  # grid, bounds, f_row, f_blocked, tcw, ow
                                                           vp, ci, vp, vp, vp, vp, vp, vp,      # nq, q_stride, valid, pw, min/max dist, angle, qdesc
                                                           vp, vp, cf, ci, vp, cf, ci, ci,      # k, bounds, th, orb_dist, sf, log sf, nlevels, check_ori
                                                           vp, vp]                              # match, nmatches
    L.orbm_bow_transform_batch_async.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp]
    L.orbm_search_by_bow_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp,   # pairs, KF pool
                                                 ci, ci, vp, vp, vp, vp, vp,               # frame pool
                                                 vp, vp, cf, ci, vp, vp]                   # kf_row, f_row, nnratio, check_ori, outputs
    L.orbm_search_by_bow_fisheye_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp,   # pairs, KF pool (stacked rows)
                                                         ci, ci, vp, vp, vp, vp, vp,               # frame pool
                                                         vp, vp, vp, cf, ci, vp, vp, vp]           # kf_row, fl_row, fr_row, nnratio, check_ori, outputs
    L.orbm_search_by_bow_kf_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp,   # pairs, pool 1 (pKF1)
                                                    ci, ci, vp, vp, vp, vp, vp, vp,            # pool 2 (pKF2)
                                                    vp, vp, cf, ci, vp, vp]                    # row1, row2, nnratio, check_ori, outputs
    L.orbm_search_by_projection_sim3_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp,       # pairs, KF pool (kps, desc, counts)
                                                             vp, vp, cf, cf, cf, cf, vp, vp, vp, vp,   # grid, bounds, kf_row, matched_in, tcw, ow
                                                             vp, ci, vp, vp, vp, vp, vp, vp,   # nq, q_stride, valid, pw, normal, min/max dist, qdesc
                                                             vp, vp, ci, cf, ci, vp, cf, ci,   # k, bounds, th, ratio, proj_form, sf, log sf, nlevels
                                                             vp, vp]                           # match, nmatches
    L.orbm_search_for_triangulation_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp,   # pairs, pool 1 (pKF1)
                                                            ci, ci, vp, vp, vp, vp, vp, vp, vp,            # pool 2 (pKF2)
                                                            vp, vp, vp, vp, vp, vp, ci,                    # row1, row2, F12, ep, sf2, sigma2, nlevels
                                                            ci, ci, ci, vp, vp]                            # only_stereo, coarse, check_ori, outputs
    L.orbm_search_for_initialization_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp,                  # pairs, pool 1 (initial frames)
                                                             ci, ci, vp, vp, vp,                          # pool 2 (current frames)
                                                             vp, vp, cf, cf, cf, cf,                      # its grid, bounds
                                                             vp, vp, vp, ci, cf, ci,                      # row1, row2, prev_in, window, nnratio, check_ori
                                                             vp, vp, vp]                                  # matches12, nmatches, prev_out
    L.orbm_stereo_from_rgbd.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ci, cf, cf, vp, vp]   # n, kps, kps_un, image, type, w, h, stride, factor, mbf, outputs
    L.orbm_stereo_from_rgbd_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp,                # nframes, first, cap, kps, kps_un, counts
                                                    vp, ci, ci, ci, ci, cf, cf, vp, vp, vp]    # image table, type, w, h, stride, factor, mbf, outputs
    L.orbm_unproject_stereo.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.orbm_unproject_stereo_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_select_depth_points.argtypes = [vp, ci, vp, vp, vp, cf, ci, vp, vp, vp, vp, vp]     # n, depth, keeps_mp, tracked, th, max_points, outputs
    L.orbm_select_depth_points_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, cf, ci,   # nrows, first, cap, counts, depth, keeps_mp, tracked, th, max
                                                       vp, vp, vp, vp, vp, vp]                   # order, create_new, nvisit, ncreate, nclose_tracked / _untracked
    L.orbm_adopt_new_points_batch_async.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    for name in ("orbm_distinctive_descriptors", "orbm_distinctive_descriptors_batch_async"):
        getattr(L, name).argtypes = [vp, ci, ci, ci, vp, vp,                       # nmp, nkf_rows, cap, desc_kf, counts_kf
                                     ci, vp, vp, vp, vp, vp,                       # nobs, obs_off, obs_row, obs_slot, obs_flags, valid
                                     vp, vp, vp]                                   # mp_desc, best_obs, best_median
    for name in ("orbm_update_normal_and_depth", "orbm_update_normal_and_depth_batch_async"):
        getattr(L, name).argtypes = [vp, ci, ci, ci, vp, vp, vp, vp,               # nmp, nkf_rows, cap, kps_kf, counts_kf, ow_l, ow_r
                                     ci, vp, vp, vp, vp, vp,                       # nobs, obs_off, obs_row, obs_slot, obs_flags, valid
                                     vp, vp, vp, vp, ci,                           # pw, ref_row, ref_slot, scale factors (host), nlevels
                                     vp, vp, vp, vp]                               # normal, min_dist, max_dist, updated
    L.orbm_bow_vector_batch_async.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp]           # word_id, weight, counts, nrows, cap, outputs
    for name in ("orbm_kfdb_query", "orbm_kfdb_query_batch_async"):
        getattr(L, name).argtypes = [vp, ci, vp,                                   # nq, q_row
                                     ci, ci, vp, vp, vp,                           # nq_rows, q_cap, q_word, q_val, q_n
                                     ci, ci, vp, vp, vp,                           # ndb_rows, db_cap, db_word, db_val, db_n
                                     vp, vp,                                       # db_active, exclude
                                     vp, vp, vp, vp, vp, vp, vp, vp]               # common, first_word, score, scored, max / min_common, nsharing, nscored
    for name in ("orbm_keyframe_culling", "orbm_keyframe_culling_batch_async"):
        getattr(L, name).argtypes = [vp, ci, vp, ci, ci,                           # ncand, cand_row, nkf_rows, cap
                                     vp, vp, vp, vp, cf,                           # kps_kf, counts_kf, kf_mp, depth, th_depth
                                     ci, ci, vp, vp, vp, vp,                       # nmp, nobs, obs_off, obs_row, obs_slot, obs_flags
                                     vp, vp, vp, ci, cf,                           # mp_valid, mp_nobs, erased, th_obs, redundant_th
                                     vp, vp, vp, vp, vp]                           # n_mps, n_redundant, cull, slot_state, first_cull
    for name in ("orbm_covisibility_votes", "orbm_covisibility_votes_batch_async"):
        getattr(L, name).argtypes = [vp, ci, ci, vp, vp, vp,                       # nq, q_stride, q_mp, q_n, self_row
                                     ci, ci, vp, vp, ci,                           # nkf_rows, cap, counts_kf, kf_skip, skip_bad
                                     ci, ci, vp, vp, vp, vp, vp,                   # nmp, nobs, obs_off, obs_row, obs_slot, obs_flags, mp_valid
                                     ci, ci,                                       # th, list_cap
                                     vp, vp, vp, vp, vp, vp]                       # votes, n_voted, max_votes, n_over, list_row, list_votes
    for name in ("orbm_local_points", "orbm_local_points_batch_async"):
        getattr(L, name).argtypes = [vp, ci, ci, vp, vp, ci, ci,                   # T, lkf_stride, lkf_row, n_lkf, nkf_rows, cap
                                     vp, vp, ci, vp, ci,                           # counts_kf, kf_mp, nmp, mp_valid, q_stride
                                     vp, vp, vp]                                   # local_mp, n_total, nq
    L.orbm_gather_map_points_batch_async.argtypes = [vp, ci, ci, vp, vp, ci,       # T, q_stride, local_mp, nq, nmp
                                                     vp, vp, vp, vp, vp, vp, vp,   # mp_pw, mp_normal, mp_min_dist, mp_max_dist, mp_desc, mp_nobs, mp_skip
                                                     vp, vp, vp, vp, vp, vp, vp]   # pw, normal, min_dist, max_dist, qdesc, mp_obs, skip
    for name in ("orbm_pose_optimization", "orbm_pose_optimization_batch_async"):
        getattr(L, name).argtypes = [vp, ci, ci, ci, vp, vp,                       # nframes, first, cap, kps_un, counts
                                     vp, vp, ci, vp, vp,                           # uright, q_mp, nmp, mp_pw, tcw_in
                                     vp, cf, vp, ci,                               # k (host), bf, inv_level_sigma2 (host), nlevels
                                     vp, vp, vp, vp]                               # tcw_out, outlier, n_corr, n_good
    L.orbm_discard_outliers_batch_async.argtypes = [vp, ci, ci, vp, vp, vp,        # nframes, cap, counts, q_mp, outlier
                                                    ci, vp, vp, ci, ci,            # nmp, mp_nobs, mp_valid, discard, clear_bad
                                                    vp, vp, vp]                    # mp_seen, n_matches_map, n_discarded
    _tri = [ci, vp, ci,                                                            # ngroups, group_start (host), npairs
            ci, ci, vp, vp, vp, vp, vp, vp, vp,                                    # nrows1, cap1, kps_un1, kps1, counts1, uright1, depth1, tcw1, ow1
            ci, ci, vp, vp, vp, vp, vp, vp, vp,                                    # pool 2
            vp, vp, vp, vp, vp, cf, cf, cf,                                        # row1, row2, matches12, k1, k2 (host), mb1, mbf1, mb2
            vp, vp, vp, vp, ci, cf, cf,                                            # scale factors / level sigma2 of both sides (host), nlevels, ratio_factor, th_far
            vp, vp, vp, vp, vp, vp, vp]                                            # won_pair, won_idx2, x3d, reason, ncreated, order, ntotal
    L.orbm_triangulate_new_points_batch_async.argtypes = [vp] + _tri
    L.orbm_triangulate_new_points.argtypes = [vp, ci] + _tri                       # handle, space
    L.orbm_is_in_frustum_batch_async.argtypes = [vp, ci, vp, vp, vp, ci, vp,                 # nframes, tcw, ow, nq, q_stride, skip
                                                 vp, vp, vp, vp, ci,                         # pw, normal, min_dist, max_dist, q_shared
                                                 vp, vp, cf, cf, cf, ci,                     # k, bounds (host), bf, cos limit, log scale factor, levels
                                                 vp, vp, vp, vp, vp, vp, vp, vp]             # the seven rows, n_in_view
    L.orbm_vocab_load_text.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p]
    L.orbm_vocab_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.orbm_vocab_destroy.argtypes = [C.c_void_p]
    L.orbm_vocab_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
    L.orbm_bow_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.orbm_bow_vectors.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]

    def stereo_from_rgbd(self, kps, kps_un, depth_img, depth_factor, mbf):
        """Frame::ComputeStereoFromRGBD (Frame.cc:1279-1309) on the UNCONVERTED depth image (2-D uint16 or float32, any row stride) and
        mDepthMapFactor (Tracking.cc:1353-1354) -> (number of keypoints with depth, mvuRight, mvDepth)."""
        kps = np.ascontiguousarray(kps, KP_DTYPE); un = kps if kps_un is None else np.ascontiguousarray(kps_un, KP_DTYPE)
        img = np.asarray(depth_img)
        if img.ndim != 2 or img.dtype not in (np.uint16, np.float32) or img.strides[1] != img.itemsize:
            raise OrbError("depth image must be a 2-D uint16 or float32 array with contiguous rows")
        n = len(kps)
        ur = np.zeros(max(n, 1), np.float32); dp = np.zeros(max(n, 1), np.float32)
        rc = _chk(self.L.orbm_stereo_from_rgbd(self.h, n, _p(kps), _p(un), img.ctypes.data, DEPTH_F32 if img.dtype == np.float32 else DEPTH_U16,
                                               img.shape[1], img.shape[0], img.strides[0], float(depth_factor), float(mbf), _p(ur), _p(dp)),
                  "orbm_stereo_from_rgbd")
        return rc, ur[:n], dp[:n]

    def stereo_from_rgbd_batch_async(self, nframes, first, cap, kps, kps_un, counts, depth_imgs, depth_type, w, h, stride_bytes, depth_factor, mbf,
                                     uright, depth, nvalid):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_stereo_from_rgbd_batch_async)."""
        return _chk(self.L.orbm_stereo_from_rgbd_batch_async(self.h, nframes, first, cap, kps, kps_un, counts, depth_imgs, depth_type, w, h, stride_bytes,
                                                             float(depth_factor), float(mbf), uright, depth, nvalid), "orbm_stereo_from_rgbd_batch_async")

    def unproject_stereo(self, kps_un, depth, twc, K):
        """Frame::UnprojectStereo (Frame.cc:1312-1326) for every keypoint: twc = row-major 3x4 [Rwc | Ow], K = (fx, fy, cx, cy) ->
        (number of points, x3Dw [n][3], has_depth [n])."""
        un = np.ascontiguousarray(kps_un, KP_DTYPE); n = len(un)
        d = np.ascontiguousarray(depth, np.float32); T = np.ascontiguousarray(twc, np.float32).reshape(12); K = np.ascontiguousarray(K, np.float32)
        x = np.zeros((max(n, 1), 3), np.float32); hd = np.zeros(max(n, 1), np.uint8)
        rc = _chk(self.L.orbm_unproject_stereo(self.h, n, _p(un), _p(d), _p(T), _p(K), _p(x), _p(hd)), "orbm_unproject_stereo")
        return rc, x[:n], hd[:n]

    def unproject_stereo_batch_async(self, nrows, first, cap, kps_un, counts, depth, twc, K, x3dw, has_depth):
        """Device form, enqueue only: device pointers except K (include/orbm.h: orbm_unproject_stereo_batch_async)."""
        K = np.ascontiguousarray(K, np.float32)
        return _chk(self.L.orbm_unproject_stereo_batch_async(self.h, nrows, first, cap, kps_un, counts, depth, twc, _p(K), x3dw, has_depth),
                    "orbm_unproject_stereo_batch_async")

    def select_depth_points(self, depth, keeps_mp=None, tracked=None, th_depth=float("inf"), max_points=100):
        """The sorted walk of Tracking::UpdateLastFrame / CreateNewKeyFrame (Tracking.cc:3094-3163, :3694-3783) and NeedNewKeyFrame's close
        counts (:3524-3546) over one frame's mvDepth -> (nvisit, order [n], create_new [n], ncreate, nclose_tracked, nclose_untracked).
        keeps_mp = `pMP && pMP->Observations() >= 1`, tracked = `pMP && !mvbOutlier[i]` per slot (None = no slot)."""
        d = np.ascontiguousarray(depth, np.float32); n = len(d)
        k = None if keeps_mp is None else np.ascontiguousarray(keeps_mp, np.uint8); t = None if tracked is None else np.ascontiguousarray(tracked, np.uint8)
        if (k is not None and len(k) != n) or (t is not None and len(t) != n):
            raise OrbError("keeps_mp and tracked hold one flag per depth slot")
        order = np.full(max(n, 1), -1, np.int32); cn = np.zeros(max(n, 1), np.uint8); cnt = np.zeros(3, np.int32)
        rc = _chk(self.L.orbm_select_depth_points(self.h, n, _p(d), None if k is None else _p(k), None if t is None else _p(t), float(th_depth),
                                                  int(max_points), _p(order), _p(cn), cnt.ctypes.data, cnt.ctypes.data + 4, cnt.ctypes.data + 8),
                  "orbm_select_depth_points")
        return rc, order[:n], cn[:n], int(cnt[0]), int(cnt[1]), int(cnt[2])

    def select_depth_points_batch_async(self, nrows, first, cap, counts, depth, keeps_mp, tracked, th_depth, max_points, order, create_new, nvisit,
                                        ncreate, nclose_tracked=None, nclose_untracked=None):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_select_depth_points_batch_async)."""
        return _chk(self.L.orbm_select_depth_points_batch_async(self.h, nrows, first, cap, counts, depth, keeps_mp, tracked, float(th_depth),
                                                                int(max_points), order, create_new, nvisit, ncreate, nclose_tracked, nclose_untracked),
                    "orbm_select_depth_points_batch_async")

    def adopt_new_points_batch_async(self, nrows, first, cap, counts, create_new, x3d_new, desc, outlier, x3dw, has_mp, mp_obs, qdesc):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_adopt_new_points_batch_async)."""
        return _chk(self.L.orbm_adopt_new_points_batch_async(self.h, nrows, first, cap, counts, create_new, x3d_new, desc, outlier, x3dw, has_mp,
                                                             mp_obs, qdesc), "orbm_adopt_new_points_batch_async")

    def _obs_arrays(obs_off, obs_row, obs_slot, obs_flags, valid, nmp):
        off = np.ascontiguousarray(obs_off, np.int32); row = np.ascontiguousarray(obs_row, np.int32); slot = np.ascontiguousarray(obs_slot, np.int32)
        fl = np.ascontiguousarray(obs_flags, np.uint8)
        if len(off) != nmp + 1 or not (len(row) == len(slot) == len(fl)):
            raise OrbError("obs_off must hold nmp + 1 offsets and obs_row / obs_slot / obs_flags one entry each")
        pad = lambda a: a if len(a) else np.zeros(1, a.dtype)               # nobs == 0: the arrays are still required
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        return off, pad(row), pad(slot), pad(fl), v, len(row)

    def distinctive_descriptors(self, desc_kf, counts_kf, obs_off, obs_row, obs_slot, obs_flags, valid=None, mp_desc=None):
        """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:450-538) for nmp = len(obs_off) - 1 MapPoints over a KeyFrame pool desc_kf
        [nkf_rows][cap][32] -> (number with a descriptor, mp_desc [nmp][32], best_obs, best_median).  mp_desc (optional) holds the rows that
        MapPoints without a winner keep."""
        d = np.ascontiguousarray(desc_kf, np.uint8); nrows, cap = d.shape[0], d.shape[1]
        cnt = np.ascontiguousarray(counts_kf, np.int32); nmp = len(obs_off) - 1
        off, row, slot, fl, v, nobs = _obs_arrays(obs_off, obs_row, obs_slot, obs_flags, valid, nmp)
        out = np.zeros((max(nmp, 1), 32), np.uint8) if mp_desc is None else np.array(mp_desc, np.uint8).reshape(-1, 32)
        bo = np.zeros(max(nmp, 1), np.int32); bm = np.zeros(max(nmp, 1), np.int32)
        rc = _chk(self.L.orbm_distinctive_descriptors(self.h, nmp, nrows, cap, _p(d), _p(cnt), nobs, _p(off), _p(row), _p(slot), _p(fl),
                                                      None if v is None else _p(v), _p(out), _p(bo), _p(bm)), "orbm_distinctive_descriptors")
        return rc, out[:nmp], bo[:nmp], bm[:nmp]

    def distinctive_descriptors_batch_async(self, nmp, nkf_rows, cap, desc_kf, counts_kf, nobs, obs_off, obs_row, obs_slot, obs_flags, valid,
                                            mp_desc, best_obs, best_median=None):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_distinctive_descriptors_batch_async)."""
        return _chk(self.L.orbm_distinctive_descriptors_batch_async(self.h, nmp, nkf_rows, cap, desc_kf, counts_kf, nobs, obs_off, obs_row, obs_slot,
                                                                    obs_flags, valid, mp_desc, best_obs, best_median),
                    "orbm_distinctive_descriptors_batch_async")

    def update_normal_and_depth(self, kps_kf, counts_kf, ow_l, ow_r, obs_off, obs_row, obs_slot, obs_flags, valid, pw, ref_row, ref_slot, scale_factors,
                                normal=None, min_dist=None, max_dist=None):
        """MapPoint::UpdateNormalAndDepth (MapPoint.cc:578-652) for nmp MapPoints over a KeyFrame pool kps_kf [nkf_rows][cap] ->
        (number updated, normal [nmp][3], min_dist, max_dist, updated).  normal / min_dist / max_dist (optional) hold the rows that
        MapPoints which are not updated keep."""
        k = np.ascontiguousarray(kps_kf, KP_DTYPE); nrows, cap = k.shape[0], k.shape[1]
        cnt = np.ascontiguousarray(counts_kf, np.int32); nmp = len(obs_off) - 1
        ol = np.ascontiguousarray(ow_l, np.float32).reshape(-1, 3); orr = None if ow_r is None else np.ascontiguousarray(ow_r, np.float32).reshape(-1, 3)
        off, row, slot, fl, v, nobs = _obs_arrays(obs_off, obs_row, obs_slot, obs_flags, valid, nmp)
        P = np.ascontiguousarray(pw, np.float32).reshape(-1, 3); rr = np.ascontiguousarray(ref_row, np.int32); rs = np.ascontiguousarray(ref_slot, np.int32)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        if len(ol) != nrows or (orr is not None and len(orr) != nrows) or not (len(P) == len(rr) == len(rs) == nmp):
            raise OrbError("ow_l / ow_r hold one centre per pool row; pw, ref_row and ref_slot one entry per MapPoint")
        keep = lambda a, shape: np.zeros(shape, np.float32) if a is None else np.array(a, np.float32).reshape(shape)
        nm = keep(normal, (max(nmp, 1), 3)); mn = keep(min_dist, max(nmp, 1)); mx = keep(max_dist, max(nmp, 1)); up = np.zeros(max(nmp, 1), np.uint8)
        rc = _chk(self.L.orbm_update_normal_and_depth(self.h, nmp, nrows, cap, _p(k), _p(cnt), _p(ol), None if orr is None else _p(orr), nobs, _p(off),
                                                      _p(row), _p(slot), _p(fl), None if v is None else _p(v), _p(P), _p(rr), _p(rs), _p(sf), len(sf),
                                                      _p(nm), _p(mn), _p(mx), _p(up)), "orbm_update_normal_and_depth")
        return rc, nm[:nmp], mn[:nmp], mx[:nmp], up[:nmp]

    def update_normal_and_depth_batch_async(self, nmp, nkf_rows, cap, kps_kf, counts_kf, ow_l, ow_r, nobs, obs_off, obs_row, obs_slot, obs_flags, valid,
                                            pw, ref_row, ref_slot, scale_factors, normal, min_dist, max_dist, updated):
        """Device form, enqueue only: device pointers except scale_factors (include/orbm.h: orbm_update_normal_and_depth_batch_async)."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        return _chk(self.L.orbm_update_normal_and_depth_batch_async(self.h, nmp, nkf_rows, cap, kps_kf, counts_kf, ow_l, ow_r, nobs, obs_off, obs_row,
                                                                    obs_slot, obs_flags, valid, pw, ref_row, ref_slot, _p(sf), len(sf),
                                                                    normal, min_dist, max_dist, updated), "orbm_update_normal_and_depth_batch_async")

    def bow_vector_batch_async(self, word_id, weight, counts, nrows, cap, bow_word, bow_val, nbow):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_bow_vector_batch_async)."""
        return _chk(self.L.orbm_bow_vector_batch_async(self.h, word_id, weight, counts, nrows, cap, bow_word, bow_val, nbow),
                    "orbm_bow_vector_batch_async")

    def kfdb_query(self, q_row, q_word, q_val, q_n, db_word, db_val, db_n, db_active=None, exclude=None):
        """The inverted-file walk, the 0.8 rule and the L1 scores of KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates
        (KeyFrameDatabase.cc:869-926, :660-752) for the queries q_row of the pool q_word / q_val [nq_rows][q_cap], q_n against the pool
        db_word / db_val [ndb_rows][db_cap], db_n -> dict of common, first_word, score, scored [nq][ndb_rows] and max_common, min_common,
        nsharing, nscored [nq] (include/orbm.h: orbm_kfdb_query)."""
        qr = np.ascontiguousarray(q_row, np.int32); nq = len(qr)
        qw = np.ascontiguousarray(q_word, np.int32); qv = np.ascontiguousarray(q_val, np.float64); qn = np.ascontiguousarray(q_n, np.int32)
        same = q_word is db_word and q_val is db_val and q_n is db_n
        dw, dv, dn = (qw, qv, qn) if same else (np.ascontiguousarray(db_word, np.int32), np.ascontiguousarray(db_val, np.float64),
                                                np.ascontiguousarray(db_n, np.int32))
        if qw.ndim != 2 or dw.ndim != 2 or qv.shape != qw.shape or dv.shape != dw.shape or len(qn) != len(qw) or len(dn) != len(dw):
            raise OrbError("a pool is word [rows][cap], val [rows][cap] and n [rows]")
        ndb = len(dw)
        act = None if db_active is None else np.ascontiguousarray(db_active, np.uint8)
        exc = None if exclude is None else np.ascontiguousarray(exclude, np.uint8)
        if (act is not None and act.shape != (ndb,)) or (exc is not None and exc.shape != (nq, ndb)):
            raise OrbError("db_active holds one flag per database row and exclude one per (query, row)")
        shape = (max(nq, 1), max(ndb, 1))
        out = {"common": np.zeros(shape, np.int32), "first_word": np.zeros(shape, np.int32), "score": np.zeros(shape, np.float32),
               "scored": np.zeros(shape, np.uint8), "max_common": np.zeros(shape[0], np.int32), "min_common": np.zeros(shape[0], np.int32),
               "nsharing": np.zeros(shape[0], np.int32), "nscored": np.zeros(shape[0], np.int32)}
        _chk(self.L.orbm_kfdb_query(self.h, nq, _p(qr), len(qw), qw.shape[1], _p(qw), _p(qv), _p(qn), ndb, dw.shape[1], _p(dw), _p(dv), _p(dn),
                                    None if act is None else _p(act), None if exc is None else _p(exc),
                                    *[_p(out[k]) for k in ("common", "first_word", "score", "scored", "max_common", "min_common", "nsharing", "nscored")]),
             "orbm_kfdb_query")
        return {k: v[:nq] for k, v in out.items()}

    def kfdb_query_batch_async(self, nq, q_row, nq_rows, q_cap, q_word, q_val, q_n, ndb_rows, db_cap, db_word, db_val, db_n, db_active, exclude,
                               common, first_word, score, scored, max_common, min_common, nsharing, nscored):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_kfdb_query_batch_async)."""
        return _chk(self.L.orbm_kfdb_query_batch_async(self.h, nq, q_row, nq_rows, q_cap, q_word, q_val, q_n, ndb_rows, db_cap, db_word, db_val, db_n,
                                                       db_active, exclude, common, first_word, score, scored, max_common, min_common, nsharing,
                                                       nscored), "orbm_kfdb_query_batch_async")

    def keyframe_culling(self, cand_row, kps_kf, counts_kf, kf_mp, depth, th_depth, obs_off, obs_row, obs_slot, obs_flags, mp_valid, mp_nobs,
                         erased=None, th_obs=3, redundant_th=0.9, slot_state=True):
        """The redundancy counts of LocalMapping::KeyFrameCulling (LocalMapping.cc:1218-1400) for the candidates cand_row of the KeyFrame
        pool kps_kf [nkf_rows][cap] -> dict of n_mps, n_redundant, cull [ncand], slot_state [ncand][cap] (None when not asked for),
        first_cull and ncull.  depth / mp_valid / erased may be None (include/orbm.h: orbm_keyframe_culling)."""
        cr = np.ascontiguousarray(cand_row, np.int32); nc = len(cr)
        k = np.ascontiguousarray(kps_kf, KP_DTYPE); nrows, cap = k.shape[0], k.shape[1]
        cnt = np.ascontiguousarray(counts_kf, np.int32); km = np.ascontiguousarray(kf_mp, np.int32)
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        no = np.ascontiguousarray(mp_nobs, np.int32); nmp = len(no)
        off, row, slot, fl, v, nobs = _obs_arrays(obs_off, obs_row, obs_slot, obs_flags, mp_valid, nmp)
        er = None if erased is None else np.ascontiguousarray(erased, np.uint8)
        if km.shape != (nc, cap) or (dp is not None and dp.shape != (nc, cap)) or len(cnt) != nrows or (er is not None and er.shape != (nrows,)):
            raise OrbError("kf_mp / depth hold one row of cap slots per candidate; counts_kf and erased one entry per pool row")
        out = {"n_mps": np.zeros(max(nc, 1), np.int32), "n_redundant": np.zeros(max(nc, 1), np.int32), "cull": np.zeros(max(nc, 1), np.uint8)}
        ss = np.zeros((max(nc, 1), cap), np.uint8) if slot_state else None
        fc = np.zeros(1, np.int32)
        rc = _chk(self.L.orbm_keyframe_culling(self.h, nc, _p(cr), nrows, cap, _p(k), _p(cnt), _p(km), None if dp is None else _p(dp), float(th_depth),
                                               nmp, nobs, _p(off), _p(row), _p(slot), _p(fl), None if v is None else _p(v), _p(no),
                                               None if er is None else _p(er), int(th_obs), float(redundant_th),
                                               _p(out["n_mps"]), _p(out["n_redundant"]), _p(out["cull"]), None if ss is None else _p(ss), _p(fc)),
                  "orbm_keyframe_culling")
        out = {key: a[:nc] for key, a in out.items()}
        out.update(slot_state=None if ss is None else ss[:nc], first_cull=int(fc[0]), ncull=rc)
        return out

    def keyframe_culling_batch_async(self, ncand, cand_row, nkf_rows, cap, kps_kf, counts_kf, kf_mp, depth, th_depth, nmp, nobs, obs_off, obs_row,
                                     obs_slot, obs_flags, mp_valid, mp_nobs, erased, th_obs, redundant_th, n_mps, n_redundant, cull,
                                     slot_state=None, first_cull=None):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_keyframe_culling_batch_async)."""
        return _chk(self.L.orbm_keyframe_culling_batch_async(self.h, ncand, cand_row, nkf_rows, cap, kps_kf, counts_kf, kf_mp, depth, float(th_depth),
                                                             nmp, nobs, obs_off, obs_row, obs_slot, obs_flags, mp_valid, mp_nobs, erased, int(th_obs),
                                                             float(redundant_th), n_mps, n_redundant, cull, slot_state, first_cull),
                    "orbm_keyframe_culling_batch_async")

    def covisibility_votes(self, q_mp, q_n, self_row, counts_kf, cap, kf_skip, skip_bad, obs_off, obs_row, obs_slot, obs_flags, mp_valid=None, th=15,
                           list_cap=0, list_fill=-1):
        """The covisibility vote of KeyFrame::UpdateConnections step 1 (KeyFrame.cc:474-512, skip_bad 1) or Tracking::UpdateLocalKeyFrames
        (Tracking.cc:3964-4013, skip_bad 0) for the queries q_mp [nq][q_stride] -> dict of votes [nq][nkf_rows], n_voted, max_votes, n_over
        [nq], list_row, list_votes [nq][list_cap] (None with list_cap 0; entries that are not written hold list_fill).  self_row, kf_skip
        and mp_valid may be None (include/orbm.h: orbm_covisibility_votes)."""
        qm = np.ascontiguousarray(q_mp, np.int32); nq, qs = qm.shape
        qn = np.ascontiguousarray(q_n, np.int32); cnt = np.ascontiguousarray(counts_kf, np.int32); nrows = len(cnt)
        sr = None if self_row is None else np.ascontiguousarray(self_row, np.int32)
        ks = None if kf_skip is None else np.ascontiguousarray(kf_skip, np.uint8)
        nmp = len(obs_off) - 1
        off, row, slot, fl, v, nobs = _obs_arrays(obs_off, obs_row, obs_slot, obs_flags, mp_valid, nmp)
        if len(qn) != nq or (sr is not None and len(sr) != nq) or (ks is not None and len(ks) != nrows):
            raise OrbError("q_n and self_row hold one entry per query, kf_skip one per pool row")
        out = {"votes": np.zeros((max(nq, 1), nrows), np.int32), "n_voted": np.zeros(max(nq, 1), np.int32), "max_votes": np.zeros(max(nq, 1), np.int32),
               "n_over": np.zeros(max(nq, 1), np.int32)}
        lr = np.full((max(nq, 1), list_cap), list_fill, np.int32) if list_cap > 0 else None
        lv = np.full((max(nq, 1), list_cap), list_fill, np.int32) if list_cap > 0 else None
        opt = lambda a: None if a is None else _p(a)
        _chk(self.L.orbm_covisibility_votes(self.h, nq, qs, _p(qm), _p(qn), opt(sr), nrows, int(cap), _p(cnt), opt(ks), int(skip_bad), nmp, nobs, _p(off),
                                            _p(row), _p(slot), _p(fl), opt(v), int(th), int(list_cap), _p(out["votes"]), _p(out["n_voted"]),
                                            _p(out["max_votes"]), _p(out["n_over"]), opt(lr), opt(lv)), "orbm_covisibility_votes")
        out = {key: a[:nq] for key, a in out.items()}
        out.update(list_row=None if lr is None else lr[:nq], list_votes=None if lv is None else lv[:nq])
        return out

    def covisibility_votes_batch_async(self, nq, q_stride, q_mp, q_n, self_row, nkf_rows, cap, counts_kf, kf_skip, skip_bad, nmp, nobs, obs_off, obs_row,
                                       obs_slot, obs_flags, mp_valid, th, list_cap, votes, n_voted, max_votes, n_over, list_row=None, list_votes=None):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_covisibility_votes_batch_async)."""
        return _chk(self.L.orbm_covisibility_votes_batch_async(self.h, nq, q_stride, q_mp, q_n, self_row, nkf_rows, cap, counts_kf, kf_skip, int(skip_bad),
                                                               nmp, nobs, obs_off, obs_row, obs_slot, obs_flags, mp_valid, int(th), int(list_cap), votes,
                                                               n_voted, max_votes, n_over, list_row, list_votes),
                    "orbm_covisibility_votes_batch_async")

    def local_points(self, lkf_row, n_lkf, counts_kf, kf_mp, nmp, mp_valid=None, q_stride=None, fill=-1):
        """Tracking::UpdateLocalPoints (Tracking.cc:3917-3948) for T frames: lkf_row [T][lkf_stride] = the local KeyFrames' pool rows in the
        order walked, kf_mp [nkf_rows][cap] -> (local_mp [T][q_stride], n_total [T], nq [T]); slots at and beyond nq hold `fill`
        (include/orbm.h: orbm_local_points)."""
        lk = np.ascontiguousarray(lkf_row, np.int32); T, ls = lk.shape
        nl = np.ascontiguousarray(n_lkf, np.int32); cnt = np.ascontiguousarray(counts_kf, np.int32)
        km = np.ascontiguousarray(kf_mp, np.int32); nrows, cap = km.shape
        v = None if mp_valid is None else np.ascontiguousarray(mp_valid, np.uint8)
        if len(nl) != T or len(cnt) != nrows or (v is not None and len(v) != nmp):
            raise OrbError("n_lkf holds one entry per frame, counts_kf one per pool row, mp_valid one per MapPoint")
        qs = int(q_stride) if q_stride is not None else max(1, min(int(nmp), ls * cap))
        out = np.full((max(T, 1), max(qs, 1)), fill, np.int32); nt = np.zeros(max(T, 1), np.int32); nq = np.zeros(max(T, 1), np.int32)
        _chk(self.L.orbm_local_points(self.h, T, ls, _p(lk), _p(nl), nrows, cap, _p(cnt), _p(km), int(nmp), None if v is None else _p(v), qs, _p(out),
                                      _p(nt), _p(nq)), "orbm_local_points")
        return out[:T], nt[:T], nq[:T]

    def local_points_batch_async(self, T, lkf_stride, lkf_row, n_lkf, nkf_rows, cap, counts_kf, kf_mp, nmp, mp_valid, q_stride, local_mp, n_total, nq):
        """Device form, enqueue only: every array argument is a device pointer (include/orbm.h: orbm_local_points_batch_async)."""
        return _chk(self.L.orbm_local_points_batch_async(self.h, T, lkf_stride, lkf_row, n_lkf, nkf_rows, cap, counts_kf, kf_mp, nmp, mp_valid, q_stride,
                                                         local_mp, n_total, nq), "orbm_local_points_batch_async")

    def gather_map_points_batch_async(self, T, q_stride, local_mp, nq, nmp, mp_pw=None, mp_normal=None, mp_min_dist=None, mp_max_dist=None, mp_desc=None,
                                      mp_nobs=None, mp_skip=None, pw=None, normal=None, min_dist=None, max_dist=None, qdesc=None, mp_obs=None, skip=None):
        """The query rows of SearchLocalPoints gathered from the MapPoint pool by local_mp, enqueue only: every array argument is a device
        pointer, every source / destination pair optional (include/orbm.h: orbm_gather_map_points_batch_async)."""
        return _chk(self.L.orbm_gather_map_points_batch_async(self.h, T, q_stride, local_mp, nq, nmp, mp_pw, mp_normal, mp_min_dist, mp_max_dist, mp_desc,
                                                              mp_nobs, mp_skip, pw, normal, min_dist, max_dist, qdesc, mp_obs, skip),
                    "orbm_gather_map_points_batch_async")

    def pose_optimization(self, kps_un, counts, uright, q_mp, mp_pw, tcw_in, K, bf, inv_level_sigma2, first=0, outlier_fill=255):
        """Optimizer::PoseOptimization(Frame*) (Optimizer.cc:943-1286, !mpCamera2) for the frames first .. first + nframes - 1 of the block
        kps_un [rows][cap] (KP_DTYPE) / counts [rows]: uright [nframes][cap] or None (every edge mono), q_mp [nframes][cap] = mvpMapPoints as
        indices into mp_pw [nmp][3] (outside [0, nmp) = NULL), tcw_in [nframes][3][4] -> dict of tcw [nframes][3][4] float32, outlier
        [nframes][cap] uint8 (slots without a MapPoint hold outlier_fill), n_corr, n_good [nframes] (include/orbm.h:
        orbm_pose_optimization)."""
        kp = np.ascontiguousarray(kps_un, KP_DTYPE); cnt = np.ascontiguousarray(counts, np.int32)
        qm = np.ascontiguousarray(q_mp, np.int32); nf, cap = qm.shape
        ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
        pw = np.ascontiguousarray(mp_pw, np.float32).reshape(-1, 3); nmp = len(pw)
        tin = np.ascontiguousarray(tcw_in, np.float32).reshape(-1, 12)
        k = np.ascontiguousarray(K, np.float32); ils = np.ascontiguousarray(inv_level_sigma2, np.float32)
        if kp.shape != (len(cnt), cap) or len(cnt) < first + nf or len(tin) != nf or (ur is not None and ur.shape != qm.shape) or len(k) != 4:
            raise OrbError("kps_un is [rows][cap] with rows >= first + nframes; uright, q_mp are [nframes][cap]; tcw_in holds one row per frame")
        out = {"tcw": np.zeros((max(nf, 1), 12), np.float32), "outlier": np.full((max(nf, 1), cap), outlier_fill, np.uint8),
               "n_corr": np.zeros(max(nf, 1), np.int32), "n_good": np.zeros(max(nf, 1), np.int32)}
        _chk(self.L.orbm_pose_optimization(self.h, nf, int(first), cap, _p(kp), _p(cnt), None if ur is None else _p(ur), _p(qm), nmp, _p(pw), _p(tin),
                                           _p(k), float(bf), _p(ils), len(ils), _p(out["tcw"]), _p(out["outlier"]), _p(out["n_corr"]),
                                           _p(out["n_good"])), "orbm_pose_optimization")
        out = {key: a[:nf] for key, a in out.items()}
        out["tcw"] = out["tcw"].reshape(-1, 3, 4)
        return out

    def pose_optimization_batch_async(self, nframes, first, cap, kps_un, counts, uright, q_mp, nmp, mp_pw, tcw_in, K, bf, inv_level_sigma2,
                                      tcw_out, outlier, n_corr, n_good):
        """Device form, enqueue only: every array argument is a device pointer except K = (fx, fy, cx, cy) and inv_level_sigma2, which are
        host arrays (include/orbm.h: orbm_pose_optimization_batch_async)."""
        k = np.ascontiguousarray(K, np.float32); ils = np.ascontiguousarray(inv_level_sigma2, np.float32)
        return _chk(self.L.orbm_pose_optimization_batch_async(self.h, nframes, first, cap, kps_un, counts, uright, q_mp, nmp, mp_pw, tcw_in, _p(k),
                                                              float(bf), _p(ils), len(ils), tcw_out, outlier, n_corr, n_good),
                    "orbm_pose_optimization_batch_async")

    def discard_outliers_batch_async(self, nframes, cap, counts, q_mp, outlier, nmp, mp_nobs, mp_valid=None, discard=1, clear_bad=0, mp_seen=None,
                                     n_matches_map=None, n_discarded=None):
        """The outlier discard loops around PoseOptimization and step 1 of SearchLocalPoints, enqueue only: every array argument is a device
        pointer (include/orbm.h: orbm_discard_outliers_batch_async)."""
        return _chk(self.L.orbm_discard_outliers_batch_async(self.h, nframes, cap, counts, q_mp, outlier, nmp, mp_nobs, mp_valid, int(discard),
                                                             int(clear_bad), mp_seen, n_matches_map, n_discarded),
                    "orbm_discard_outliers_batch_async")

    def _tri_tables(k1, k2, sf1, ls1, sf2, ls2):
        t = [np.ascontiguousarray(a, np.float32) for a in (k1, k2, sf1, ls1, sf2, ls2)]
        if len(t[0]) != 6 or len(t[1]) != 6 or not (len(t[2]) == len(t[3]) == len(t[4]) == len(t[5])):
            raise OrbError("k1, k2 are (fx, fy, cx, cy, invfx, invfy); the four level tables hold nlevels entries each")
        return t

    def triangulate_new_points(self, group_start, pool1, pool2, row1, row2, matches12, k1, k2, mb1, mbf1, mb2, sf1, ls1, sf2, ls2, ratio_factor,
                               th_far=0.0, want_reason=True):
        """Step 6 of LocalMapping::CreateNewMapPoints (LocalMapping.cc:609-892) for M10's matches12 [npairs][cap1], host arrays in and out.
        pool = dict(kps_un [rows][cap] KP_DTYPE, counts [rows], tcw [rows][12], ow [rows][3], and optionally kps (mvKeys), uright, depth);
        pool2 may be pool1.  -> dict of won_pair, won_idx2 [ngroups][cap1], x3d [ngroups][cap1][3], reason [npairs][cap1] (or None), ncreated
        [npairs], order [ngroups][cap1], ntotal [ngroups] (include/orbm.h: orbm_triangulate_new_points)."""
        gs = np.ascontiguousarray(group_start, np.int32); ng = len(gs) - 1
        m12 = np.ascontiguousarray(matches12, np.int32); npairs, cap1 = m12.shape
        r1 = np.ascontiguousarray(row1, np.int32); r2 = np.ascontiguousarray(row2, np.int32)
        def flat(pool):
            kp = np.ascontiguousarray(pool["kps_un"], KP_DTYPE); rows, cap = kp.shape
            d = {"rows": rows, "cap": cap, "kps_un": kp, "counts": np.ascontiguousarray(pool["counts"], np.int32),
                 "tcw": np.ascontiguousarray(pool["tcw"], np.float32).reshape(rows, 12), "ow": np.ascontiguousarray(pool["ow"], np.float32).reshape(rows, 3)}
            d["kps"] = None if pool.get("kps") is None else np.ascontiguousarray(pool["kps"], KP_DTYPE)
            for key in ("uright", "depth"):
                d[key] = None if pool.get(key) is None else np.ascontiguousarray(pool[key], np.float32)
                if d[key] is not None and d[key].shape != kp.shape: raise OrbError("%s is [rows][cap]" % key)
            if d["kps"] is not None and d["kps"].shape != kp.shape: raise OrbError("kps is [rows][cap]")
            return d
        a = flat(pool1); b = a if pool2 is pool1 else flat(pool2)
        if a["cap"] != cap1 or len(r1) != npairs or len(r2) != npairs or ng < 0:
            raise OrbError("matches12 is [npairs][cap1]; row1, row2 hold one entry per pair; group_start holds ngroups + 1")
        t = _tri_tables(k1, k2, sf1, ls1, sf2, ls2)
        ngo = max(ng, 1)
        out = {"won_pair": np.full((ngo, cap1), -2, np.int32), "won_idx2": np.full((ngo, cap1), -2, np.int32), "x3d": np.zeros((ngo, cap1, 3), np.float32),
               "reason": np.full((npairs, cap1), 255, np.uint8) if want_reason else None, "ncreated": np.full(max(npairs, 1), -2, np.int32),
               "order": np.full((ngo, cap1), -2, np.int32), "ntotal": np.full(ngo, -2, np.int32)}
        q = lambda x: None if x is None else _p(x)
        pa = lambda d: (d["rows"], d["cap"], _p(d["kps_un"]), q(d["kps"]), _p(d["counts"]), q(d["uright"]), q(d["depth"]), _p(d["tcw"]), _p(d["ow"]))
        _chk(self.L.orbm_triangulate_new_points(self.h, HOST, ng, _p(gs), npairs, *pa(a), *pa(b), _p(r1), _p(r2), _p(m12), _p(t[0]), _p(t[1]),
                                                float(mb1), float(mbf1), float(mb2), _p(t[2]), _p(t[3]), _p(t[4]), _p(t[5]), len(t[2]),
                                                float(ratio_factor), float(th_far), _p(out["won_pair"]), _p(out["won_idx2"]), _p(out["x3d"]),
                                                q(out["reason"]), _p(out["ncreated"]), _p(out["order"]), _p(out["ntotal"])),
             "orbm_triangulate_new_points")
        return out

    def triangulate_new_points_batch_async(self, group_start, npairs, pool1, pool2, row1, row2, matches12, k1, k2, mb1, mbf1, mb2, sf1, ls1, sf2, ls2,
                                           ratio_factor, th_far, won_pair, won_idx2, x3d, reason, ncreated, order, ntotal):
        """Device form, enqueue only: pool = (nrows, cap, kps_un, kps, counts, uright, depth, tcw, ow) of device pointers, every other array
        argument is a device pointer except group_start, k1, k2 and the four level tables, which are host arrays (include/orbm.h:
        orbm_triangulate_new_points_batch_async)."""
        gs = np.ascontiguousarray(group_start, np.int32)
        t = _tri_tables(k1, k2, sf1, ls1, sf2, ls2)
        return _chk(self.L.orbm_triangulate_new_points_batch_async(self.h, len(gs) - 1, _p(gs), npairs, *pool1, *pool2, row1, row2, matches12,
                                                                   _p(t[0]), _p(t[1]), float(mb1), float(mbf1), float(mb2), _p(t[2]), _p(t[3]),
                                                                   _p(t[4]), _p(t[5]), len(t[2]), float(ratio_factor), float(th_far), won_pair,
                                                                   won_idx2, x3d, reason, ncreated, order, ntotal),
                    "orbm_triangulate_new_points_batch_async")

    def is_in_frustum_batch(self, nframes, tcw, ow, nq, q_stride, skip, pw, normal, min_dist, max_dist, q_shared, K, bounds, bf, viewing_cos_limit,
                            log_scale_factor, n_levels, in_view, proj_x, proj_y, proj_xr, depth, level, view_cos, n_in_view=None):
        """Frame::isInFrustum for every frame of a batch in one launch, enqueue only: every array argument is a device pointer except K =
        (fx, fy, cx, cy) and bounds, which are host arrays (include/orbm.h: orbm_is_in_frustum_batch_async)."""
        K = np.ascontiguousarray(K, np.float32); B = np.ascontiguousarray(bounds, np.float32)
        return _chk(self.L.orbm_is_in_frustum_batch_async(self.h, nframes, tcw, ow, nq, q_stride, skip, pw, normal, min_dist, max_dist, int(q_shared),
                                                          _p(K), _p(B), float(bf), float(viewing_cos_limit), float(log_scale_factor), int(n_levels),
                                                          in_view, proj_x, proj_y, proj_xr, depth, level, view_cos, n_in_view),
                    "orbm_is_in_frustum_batch_async")

    ORBmatcher.isInFrustumBatch = is_in_frustum_batch
    ORBmatcher.BowVectorBatchAsync = bow_vector_batch_async
    ORBmatcher.KfdbQuery = kfdb_query
    ORBmatcher.KfdbQueryBatchAsync = kfdb_query_batch_async
    ORBmatcher.KeyframeCulling = keyframe_culling
    ORBmatcher.KeyframeCullingBatchAsync = keyframe_culling_batch_async
    ORBmatcher.CovisibilityVotes = covisibility_votes
    ORBmatcher.CovisibilityVotesBatchAsync = covisibility_votes_batch_async
    ORBmatcher.LocalPoints = local_points
    ORBmatcher.LocalPointsBatchAsync = local_points_batch_async
    ORBmatcher.GatherMapPointsBatchAsync = gather_map_points_batch_async
    ORBmatcher.PoseOptimization = pose_optimization
    ORBmatcher.PoseOptimizationBatchAsync = pose_optimization_batch_async
    ORBmatcher.DiscardOutliersBatchAsync = discard_outliers_batch_async
    ORBmatcher.TriangulateNewPoints = triangulate_new_points
    ORBmatcher.TriangulateNewPointsBatchAsync = triangulate_new_points_batch_async
    ORBmatcher.ComputeDistinctiveDescriptors = distinctive_descriptors
    ORBmatcher.ComputeDistinctiveDescriptorsBatchAsync = distinctive_descriptors_batch_async
    ORBmatcher.UpdateNormalAndDepth = update_normal_and_depth
    ORBmatcher.UpdateNormalAndDepthBatchAsync = update_normal_and_depth_batch_async
    ORBmatcher.window_candidates = window_candidates
    ORBmatcher.ComputeStereoMatches = stereo_matches
    ORBmatcher.ComputeStereoFromRGBD = stereo_from_rgbd
    ORBmatcher.ComputeStereoFromRGBDBatchAsync = stereo_from_rgbd_batch_async
    ORBmatcher.UnprojectStereo = unproject_stereo
    ORBmatcher.UnprojectStereoBatchAsync = unproject_stereo_batch_async
    ORBmatcher.SelectDepthPoints = select_depth_points
    ORBmatcher.SelectDepthPointsBatchAsync = select_depth_points_batch_async
    ORBmatcher.AdoptNewPointsBatchAsync = adopt_new_points_batch_async
    _bind_frame_geometry(L, "orbm_")
    for name, fn in _frame_geometry_methods("orbm_").items():
        setattr(ORBmatcher, name, fn)


def _bind_frame_geometry(L, prefix):
    """argtypes of the undistort / image-bounds / frustum entry points (same argument lists on the product and the oracle,
    except the leading handle + space of the product)."""
    vp, f, i = C.c_void_p, C.c_float, C.c_int
    lead = [vp, i] if prefix == "orbm_" else []
    getattr(L, prefix + "undistort_keypoints").argtypes = lead + [vp, i, vp, vp, i, vp, vp]
    getattr(L, prefix + "image_bounds").argtypes = ([vp] if prefix == "orbm_" else []) + [i, i, vp, vp, i, vp, vp]
    getattr(L, prefix + "is_in_frustum").argtypes = lead + [i, vp, vp, vp, vp, vp, vp, vp, vp, vp, f, f, f, i, vp, vp, vp, vp, vp, vp, vp]


def _frame_geometry_methods(prefix):
    def _lead(self, with_space=True):
        return ([self.h, HOST] if with_space else [self.h]) if prefix == "orbm_" else []

    def UndistortKeyPoints(self, kps, K, dist, newK=None):
        """Frame::UndistortKeyPoints (Frame.cc:924-970).  K / newK = (fx, fy, cx, cy); dist = (k1, k2, p1, p2[, k3])."""
        kps = np.ascontiguousarray(kps, KP_DTYPE); out = np.zeros(max(len(kps), 1), KP_DTYPE)
        K = np.ascontiguousarray(K, np.float32); nk = K if newK is None else np.ascontiguousarray(newK, np.float32)
        d = np.ascontiguousarray(dist, np.float32)
        rc = getattr(self.L, prefix + "undistort_keypoints")(*_lead(self), _p(kps), len(kps), _p(K), _p(d), len(d), _p(nk), _p(out))
        if rc < 0:
            raise OrbError("undistort_keypoints failed with code %d" % rc)
        return out[:len(kps)]

    def ComputeImageBounds(self, cols, rows, K, dist, newK=None):
        """Frame::ComputeImageBounds (Frame.cc:977-1021) -> (minX, maxX, minY, maxY)."""
        K = np.ascontiguousarray(K, np.float32); nk = K if newK is None else np.ascontiguousarray(newK, np.float32)
        d = np.ascontiguousarray(dist, np.float32); b = np.zeros(4, np.float32)
        rc = getattr(self.L, prefix + "image_bounds")(*_lead(self, False), int(cols), int(rows), _p(K), _p(d), len(d), _p(nk), _p(b))
        if rc < 0:
            raise OrbError("image_bounds failed with code %d" % rc)
        return b

    def isInFrustum(self, Pw, normal, min_dist, max_dist, Rcw, tcw, Ow, K, bounds, bf, viewing_cos_limit, log_scale_factor, n_levels):
        """Frame::isInFrustum for n map points (Frame.cc:603-671) -> dict of the MapPoint tracking members."""
        Pw = np.ascontiguousarray(Pw, np.float32).reshape(-1, 3); n = len(Pw)
        nm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        mn = np.ascontiguousarray(min_dist, np.float32); mx = np.ascontiguousarray(max_dist, np.float32)
        R = np.ascontiguousarray(Rcw, np.float32).reshape(9); t = np.ascontiguousarray(tcw, np.float32).reshape(3)
        O = np.ascontiguousarray(Ow, np.float32).reshape(3); K = np.ascontiguousarray(K, np.float32); B = np.ascontiguousarray(bounds, np.float32)
        out = {"in_view": np.zeros(max(n, 1), np.uint8), "proj_x": np.zeros(max(n, 1), np.float32), "proj_y": np.zeros(max(n, 1), np.float32),
               "proj_xr": np.zeros(max(n, 1), np.float32), "depth": np.zeros(max(n, 1), np.float32), "level": np.full(max(n, 1), -1, np.int32),
               "view_cos": np.zeros(max(n, 1), np.float32)}
        rc = getattr(self.L, prefix + "is_in_frustum")(*_lead(self), n, _p(Pw), _p(nm), _p(mn), _p(mx), _p(R), _p(t), _p(O), _p(K), _p(B),
                                                       float(bf), float(viewing_cos_limit), float(log_scale_factor), int(n_levels),
                                                       _p(out["in_view"]), _p(out["proj_x"]), _p(out["proj_y"]), _p(out["proj_xr"]),
                                                       _p(out["depth"]), _p(out["level"]), _p(out["view_cos"]))
        if rc < 0:
            raise OrbError("is_in_frustum failed with code %d" % rc)
        return rc, {k: v[:n] for k, v in out.items()}

    return {"UndistortKeyPoints": UndistortKeyPoints, "ComputeImageBounds": ComputeImageBounds, "isInFrustum": isInFrustum}


EXPORTS += ["orbm_undistort_keypoints", "orbm_image_bounds", "orbm_is_in_frustum", "orbm_is_in_frustum_batch_async"]
EXPORTS += ["orbm_frame_create", "orbm_frame_destroy", "orbm_frame_size", "orbm_search_by_projection_frame_resident", "orbm_search_by_projection_points_resident"]
EXPORTS += ["orbm_grid_build", "orbm_window_candidates", "orbm_search_by_projection_frame", "orbm_search_by_projection_points",
            "orbm_search_for_initialization", "orbm_search_for_triangulation", "orbm_search_by_bow", "orbm_stereo_matches",
            "orbm_search_by_projection_kf", "orbm_search_by_bow_kf", "orbm_search_for_triangulation_legacy", "orbm_search_for_triangulation_gated",
            "orbm_search_by_projection_sim3", "orbm_fuse", "orbm_search_by_sim3",
            "orbm_grid_build_batch_async", "orbm_track_window_batch_async", "orbm_search_by_projection_batch_async",
            "orbm_search_by_projection_points_batch_async", "orbm_search_by_projection_frame_batch_async",
            "orbm_search_by_projection_frame_fisheye_batch_async", "orbm_search_by_projection_points_fisheye_batch_async",
            "orbm_project_last_frame_batch_async", "orbm_bow_transform_batch_async", "orbm_search_by_bow_batch_async", "orbm_search_by_bow_fisheye_batch_async",
            "orbm_fuse_batch_async",
            "orbm_search_by_projection_kf_batch_async", "orbm_search_by_bow_kf_batch_async", "orbm_search_by_projection_sim3_batch_async",
            "orbm_search_for_triangulation_batch_async", "orbm_search_for_initialization_batch_async", "orbm_search_by_projection_frame_fisheye",
            "orbm_search_by_projection_points_fisheye", "orbm_search_by_bow_fisheye",
            "orbm_stereo_from_rgbd", "orbm_stereo_from_rgbd_batch_async", "orbm_unproject_stereo", "orbm_unproject_stereo_batch_async",
            "orbm_select_depth_points", "orbm_select_depth_points_batch_async", "orbm_adopt_new_points_batch_async",
            "orbm_distinctive_descriptors", "orbm_distinctive_descriptors_batch_async",
            "orbm_update_normal_and_depth", "orbm_update_normal_and_depth_batch_async",
            "orbm_bow_vector_batch_async", "orbm_kfdb_query", "orbm_kfdb_query_batch_async",
            "orbm_keyframe_culling", "orbm_keyframe_culling_batch_async",
            "orbm_covisibility_votes", "orbm_covisibility_votes_batch_async", "orbm_local_points", "orbm_local_points_batch_async",
            "orbm_gather_map_points_batch_async",
            "orbm_pose_optimization", "orbm_pose_optimization_batch_async", "orbm_discard_outliers_batch_async",
            "orbm_triangulate_new_points", "orbm_triangulate_new_points_batch_async",
            "orbm_vocab_load_text", "orbm_vocab_create", "orbm_vocab_destroy", "orbm_vocab_info", "orbm_bow_transform", "orbm_bow_vectors"]
_orig_lib = lib
_search_ready = False


def lib():                                         # noqa: F811  (binds the search entry points on first use)
    global _search_ready
    L = _orig_lib()
    if not _search_ready:
        _search_ready = True
        _install_search()
    return L


class ORBVocabulary:
    """DBoW2 ORB vocabulary resident in HBM (include/ORBVocabulary.h typedef; TemplatedVocabulary.h)."""

    def __init__(self, matcher, path):
        self.L = lib(); self.m = matcher
        h = C.c_void_p()
        if isinstance(path, dict):                                  # arrays: k, L, parent, is_leaf, desc, weight (orbm_vocab_create)
            a = path
            arr = [np.ascontiguousarray(a["parent"], np.int32), np.ascontiguousarray(a["is_leaf"], np.uint8),
                   np.ascontiguousarray(a["desc"], np.uint8), np.ascontiguousarray(a["weight"], np.float64)]
            _chk(self.L.orbm_vocab_create(matcher.h, C.byref(h), int(a["k"]), int(a["L"]), len(arr[0]), *[_p(x) for x in arr]), "orbm_vocab_create")
        else:
            _chk(self.L.orbm_vocab_load_text(matcher.h, C.byref(h), path.encode()), "orbm_vocab_load_text")
        self.h = h

    def info(self):
        v = [C.c_int() for _ in range(4)]
        self.L.orbm_vocab_info(self.h, *[C.byref(x) for x in v])
        return dict(zip(["k", "L", "nnodes", "nwords"], [x.value for x in v]))

    def transform(self, desc, levelsup=4):
        """Frame::ComputeBoW: returns (BowVector ids, values), FeatureVector CSR (nodes, start, idx), per-feature arrays."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); n = desc.shape[0]
        w = np.zeros(max(n, 1), np.int32); nd = np.zeros(max(n, 1), np.int32); wt = np.zeros(max(n, 1), np.float64)
        _chk(self.L.orbm_bow_transform(self.m.h, self.h, _p(desc), n, levelsup, _p(w), _p(nd), _p(wt)), "orbm_bow_transform")
        return bow_vectors(self.L.orbm_bow_vectors, n, w[:n], nd[:n], wt[:n]) + (w[:n], nd[:n], wt[:n])

    def __del__(self):
        try:
            self.L.orbm_vocab_destroy(self.h)
        except Exception:
            pass


def bow_vectors(fn, n, w, nd, wt):
    w = np.ascontiguousarray(w, np.int32); nd = np.ascontiguousarray(nd, np.int32); wt = np.ascontiguousarray(wt, np.float64)
    bi = np.zeros(max(n, 1), np.int32); bv = np.zeros(max(n, 1), np.float64); nb = C.c_int()
    fn_ = np.zeros(max(n, 1), np.int32); fs = np.zeros(max(n, 1) + 1, np.int32); fi = np.zeros(max(n, 1), np.int32); nf = C.c_int()
    fn(n, _p(w), _p(nd), _p(wt), _p(bi), _p(bv), C.byref(nb), _p(fn_), _p(fs), _p(fi), C.byref(nf))
    return (bi[:nb.value], bv[:nb.value]), (fn_[:nf.value], fs[:nf.value + 1], fi[:fs[nf.value]])
