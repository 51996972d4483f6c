"""Both device forms of ComputeStereoMatches against the second reading of Frame.cc:1027-1276 (tests/second_reading_stereo.py), byte for
byte and with no oracle in between: orbm_stereo_matches (k_stereo: a wave per keypoint, a full scan, the median cut on the host) and
orbm_stereo_batch_async (k_stereo_rows / k_stereo_batch / k_stereo_cut: four 16-lane keypoints per wave, a row table, a histogram median),
on the rendered pairs and on every constructed pair of tests/stereo_cases.py, and against each other.  The keypoint and descriptor rows
are laid by hand -- host arrays for the first form, a [frames][cap] block on the device for the second; the pyramids are those of ONE
extractor batch of at most 8 frames at 376 x 240, fetched back for the reading and compared with the oracle extractor's once per image."""
import ctypes as C

import numpy as np
import pytest

import second_reading_stereo as srs
import stereo_cases as sc
import structured_images as si
from test_second_reading_stereo_cpu import NF, check_expectations, rendered_pairs

pytestmark = pytest.mark.gpu

F = np.float32
STRIDE = (sc.W + 63) // 64 * 64
SENT_F, SENT_I = F(-777.25), -12345
CASES = sc.constructed_cases()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class _Rig:
    """One extractor (max_batch 8), one matcher on its stream, and the last batch's images, device levels and hand-laid block."""

    def __init__(self, pkg, oracle):
        self.pkg, self.oracle, self.L = pkg, oracle, pkg.lib()
        self.ex = pkg.ORBextractor(NF, max_size=(sc.W, sc.H), max_batch=8)
        self.mt = pkg.ORBmatcher(0.6)
        assert self.L.orbm_set_stream(self.mt.h, self.L.orbx_stream(self.ex.h)) == 0
        self.cap = self.ex.cap
        assert np.array_equal(self.ex.GetScaleFactors(), sc.SF) and np.array_equal(self.ex.GetInverseScaleFactors(), sc.ISF)
        self.dev = pkg.DeviceBuffer(8 * STRIDE * sc.H)
        self.dk = pkg.DeviceBuffer(8 * self.cap * 28); self.dd = pkg.DeviceBuffer(8 * self.cap * 32); self.dc = pkg.DeviceBuffer(8 * 4)
        self.out = [pkg.DeviceBuffer(10 * self.cap * 4) for _ in range(3)]  # uright, depth, sad: a sentinel row before and after
        self.kept = pkg.DeviceBuffer(10 * 4)
        self.level_cache = {}

    def load(self, imgs):
        """Extracts `imgs` as one batch (frame i = imgs[i]) and returns every frame's un-blurred levels as the device holds them; each
        distinct image's levels are compared with the oracle extractor's once."""
        n = len(imgs)
        assert n <= 8
        for i, im in enumerate(imgs):
            pad = np.zeros((sc.H, STRIDE), np.uint8); pad[:, :sc.W] = im
            self.dev.upload(pad, offset=i * STRIDE * sc.H)
        arr = (C.c_void_p * n)(*[self.dev.ptr + i * STRIDE * sc.H for i in range(n)])
        self.ex.enqueue_device(arr, sc.W, sc.H, STRIDE, np.zeros(2 * n, np.int32))
        self.ex.sync()
        levels = []
        for i, im in enumerate(imgs):
            # level 0 of a device-resident input is the caller's own buffer: it is read back from there
            l0 = self.dev.download(np.uint8, STRIDE * sc.H, offset=i * STRIDE * sc.H).reshape(sc.H, STRIDE)[:, :sc.W]
            lv = [l0] + [self.ex.level_image(l, frame=i) for l in range(1, sc.NLEVELS)]
            key = im.tobytes()
            if key not in self.level_cache:
                o = self.oracle.Extractor(NF); o(im, (0, 0))
                self.level_cache[key] = [o.level_image(l) for l in range(sc.NLEVELS)]
            for l in range(sc.NLEVELS):
                assert np.array_equal(lv[l], self.level_cache[key][l]), "pyramid level %d of frame %d differs from the oracle extractor's" % (l, i)
            levels.append(lv)
        return levels

    def lay(self, rows, counts=None, filler=None):
        """The [frames][cap] block: rows[f] = (kps, desc) of frame f; slots at or beyond a row's length hold `filler` (data that would
        match if it were read).  counts defaults to the rows' lengths."""
        n = len(rows)
        kps = np.zeros((n, self.cap), self.pkg.KP_DTYPE); desc = np.zeros((n, self.cap, 32), np.uint8)
        if filler is not None:
            m = min(len(filler[0]), self.cap)
            kps[:, :m] = filler[0][:m]; desc[:, :m] = filler[1][:m]
        for f, (k, d) in enumerate(rows):
            assert len(k) <= self.cap
            kps[f, :len(k)] = k; desc[f, :len(k)] = d
        cnt = np.array([len(k) for k, _ in rows] if counts is None else counts, np.int32)
        self.dk.upload(kps); self.dd.upload(desc); self.dc.upload(cnt)
        return kps, desc, cnt

    def batch(self, first_l, first_r, npairs, mb, mbf, cap=None):
        """One orbm_stereo_batch_async call into sentinel-filled outputs.  Returns (rc, uright, depth, sad [npairs][cap], kept [npairs])."""
        cap_ = self.cap
        for b, v, t in zip(self.out, (SENT_F, SENT_F, SENT_I), (F, F, np.int32)):
            b.upload(np.full(10 * cap_, v, t))
        self.kept.upload(np.full(10, SENT_I, np.int32))
        rc = self.L.orbm_stereo_batch_async(self.mt.h, self.ex.h, first_l, first_r, npairs, self.dk.ptr, self.dd.ptr, self.dc.ptr,
                                            self.cap if cap is None else cap, float(mb), float(mbf), self.out[0].ptr + cap_ * 4,
                                            self.out[1].ptr + cap_ * 4, self.out[2].ptr + cap_ * 4, self.kept.ptr + 4)
        self.mt.sync()
        ur = self.out[0].download(F, 10 * cap_).reshape(10, cap_); dp = self.out[1].download(F, 10 * cap_).reshape(10, cap_)
        sad = self.out[2].download(np.int32, 10 * cap_).reshape(10, cap_); kept = self.kept.download(np.int32, 10)
        p = max(npairs, 0) if rc == 0 else 0
        assert np.all(ur[0] == SENT_F) and np.all(ur[p + 1:] == SENT_F) and np.all(dp[0] == SENT_F) and np.all(dp[p + 1:] == SENT_F) and \
            np.all(sad[0] == SENT_I) and np.all(sad[p + 1:] == SENT_I) and kept[0] == SENT_I and np.all(kept[p + 1:] == SENT_I), \
            "a row outside the call was written"
        return rc, ur[1:p + 1], dp[1:p + 1], sad[1:p + 1], kept[1:p + 1]

    def single(self, frame_l, frame_r, kl, dl, kr, dr, mb, mbf):
        return self.mt.ComputeStereoMatches(self.ex, self.ex, kl, dl, kr, dr, mb, mbf, frame_l=frame_l, frame_r=frame_r)

    def close(self):
        self.ex.close(); self.mt.close()


@pytest.fixture(scope="module")
def rig(pkg, oracle):
    r = _Rig(pkg, oracle)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rendered(synth, oracle):
    return rendered_pairs(synth, oracle)


def _reading(levels_l, levels_r, kl, dl, kr, dr, mb, mbf):
    return srs.compute_stereo_matches(kl, dl, kr, dr, levels_l, levels_r, sc.SF, sc.ISF, mb, mbf)


def _same_as_reading(what, n, got, want):
    """got = (kept, uright [>= n], depth [>= n], sad or None) of a device form, want = the reading's tuple."""
    kept, ur, dp, sad = got
    w_kept, w_ur, w_dp, w_sad, _ = want
    assert kept == w_kept, (what, int(kept), w_kept)
    assert np.array_equal(_bits(ur[:n]), _bits(w_ur)), (what, "uright", np.nonzero(_bits(ur[:n]) != _bits(w_ur))[0][:8])
    assert np.array_equal(_bits(dp[:n]), _bits(w_dp)), (what, "depth", np.nonzero(_bits(dp[:n]) != _bits(w_dp))[0][:8])
    if sad is not None:
        assert np.array_equal(sad[:n], w_sad), (what, "sad", np.nonzero(sad[:n] != w_sad)[0][:8])


def _run_pairs(rig, pairs, mb, mbf):
    """pairs: list of (img_l, img_r, kl, dl, kr, dr), at most 4: one extractor batch (left frames first), both device forms and the
    reading on each.  Returns the reading's tuple per pair."""
    P = len(pairs)
    levels = rig.load([p[0] for p in pairs] + [p[1] for p in pairs])
    rig.lay([(p[2], p[3]) for p in pairs] + [(p[4], p[5]) for p in pairs], filler=(pairs[0][2], pairs[0][3]))
    rc, ur, dp, sad, kept = rig.batch(0, P, P, mb, mbf)
    assert rc == 0, rig.L.orbm_last_error()
    out = []
    for i, (_, _, kl, dl, kr, dr) in enumerate(pairs):
        n = len(kl)
        want = _reading(levels[i], levels[P + i], kl, dl, kr, dr, mb, mbf)
        _same_as_reading("batched form, pair %d" % i, n, (kept[i], ur[i], dp[i], sad[i]), want)
        assert np.all(ur[i, n:] == SENT_F) and np.all(dp[i, n:] == SENT_F) and np.all(sad[i, n:] == SENT_I), "a row at or beyond the count was written"
        k1, ur1, dp1 = rig.single(i, P + i, kl, dl, kr, dr, mb, mbf)
        _same_as_reading("single-pair form, pair %d" % i, n, (k1, ur1, dp1, None), want)
        assert k1 == kept[i] and np.array_equal(_bits(ur1), _bits(ur[i, :n])) and np.array_equal(_bits(dp1), _bits(dp[i, :n])), "the two forms differ"
        out.append(want)
    return out


def test_rendered_pairs_both_forms_equal_second_reading(rig, rendered):
    names = ["synth", "dots", "self"]
    res = _run_pairs(rig, [rendered[n][:6] for n in names], si.MB, si.MBF)
    got = dict(zip(names, res))
    assert got["synth"][0] > 100 and got["synth"][4]["cut"] > 0
    assert got["dots"][4]["distance_tie"] > 0
    assert got["self"][0] == 0 and got["self"][4]["cut"] > 100


GROUPS = [CASES[i:i + 4] for i in range(0, len(CASES), 4)]


@pytest.mark.parametrize("group", GROUPS, ids=["+".join(c.name for c in g) for g in GROUPS])
def test_constructed_cases_both_forms_equal_second_reading(rig, group):
    res = _run_pairs(rig, [(c.img_l, c.img_r) + c.arrays() for c in group], sc.MB, sc.MBF)
    for c, (kept, ur, dp, sad, br) in zip(group, res):
        check_expectations(c, c.arrays()[0], ur, dp, sad, br)               # the case reached its branch on the DEVICE's pyramid too


def test_batched_bookkeeping(rig, rendered):
    """One block of 8 frames, three calls: per-pair counts that differ, an empty left frame, an empty right frame, counts above cap with
    rows filled to cap, first_r < first_l and first_l == first_r (self pairs); rows at or beyond min(count, cap) keep the sentinel."""
    syn, dots = rendered["synth"], rendered["dots"]
    cap = rig.cap
    imgs = [syn[0], dots[0], syn[0], syn[0], syn[1], dots[1], syn[1], syn[1]]
    levels = rig.load(imgs)

    def tiled(k, d):
        rep = -(-cap // len(k))
        return np.tile(k, rep)[:cap], np.tile(d, (rep, 1))[:cap]
    rows = [(syn[2], syn[3]), (dots[2], dots[3]), (syn[2][:0], syn[3][:0]), tiled(syn[2], syn[3]),
            (syn[4][:301], syn[5][:301]), (dots[4], dots[5]), (syn[4], syn[5]), tiled(syn[4], syn[5])]
    counts = [len(k) for k, _ in rows]
    counts[3] = cap + 7; counts[7] = cap + 70000
    rig.lay(rows, counts=counts, filler=(syn[2], syn[3]))
    assert len(set(counts)) >= 6 and counts[2] == 0
    memo = {}
    for first_l, first_r, npairs in ((0, 4, 4), (4, 0, 4), (0, 0, 8), (5, 1, 3)):
        rc, ur, dp, sad, kept = rig.batch(first_l, first_r, npairs, si.MB, si.MBF)
        assert rc == 0, rig.L.orbm_last_error()
        for p in range(npairs):
            fl, fr = first_l + p, first_r + p
            (kl, dl), (kr, dr) = rows[fl], rows[fr]
            n = len(kl)
            if (fl, fr) not in memo:
                memo[(fl, fr)] = _reading(levels[fl], levels[fr], kl, dl, kr, dr, si.MB, si.MBF) if n else (0, np.zeros(0, F), np.zeros(0, F), np.zeros(0, np.int64), {})
            what = "call (%d, %d, %d), pair %d" % (first_l, first_r, npairs, p)
            _same_as_reading(what, n, (kept[p], ur[p], dp[p], sad[p]), memo[(fl, fr)])
            assert np.all(ur[p, n:] == SENT_F) and np.all(dp[p, n:] == SENT_F) and np.all(sad[p, n:] == SENT_I), what
            if len(kr) == 0 and n:
                assert np.all(ur[p, :n] == -1) and np.all(dp[p, :n] == -1) and np.all(sad[p, :n] == -1) and kept[p] == 0
            if n and len(kr) and p < 2:                                      # the single-pair form on the same rows and frames
                k1, ur1, dp1 = rig.single(fl, fr, kl, dl, kr, dr, si.MB, si.MBF)
                assert k1 == kept[p] and np.array_equal(_bits(ur1), _bits(ur[p, :n])) and np.array_equal(_bits(dp1), _bits(dp[p, :n])), what
    assert memo[(0, 4)][0] > 50 and memo[(3, 7)][0] > 50 and memo[(1, 5)][0] > 0


def test_host_side_argument_errors_launch_nothing(rig, rendered):
    syn = rendered["synth"]
    rig.load([syn[0], syn[1]])
    rig.lay([(syn[2], syn[3]), (syn[4], syn[5])] * 4)
    E_INVALID = -2
    for first_l, first_r, npairs, cap in ((0, 1, 1, rig.cap - 1), (0, 1, 1, rig.cap + 1), (8, 0, 1, None), (5, 0, 4, None), (0, 8, 1, None), (0, 6, 3, None)):
        rc, ur, dp, sad, kept = rig.batch(first_l, first_r, npairs, si.MB, si.MBF, cap=cap)     # batch() checks that every output row kept the sentinel
        assert rc == E_INVALID, (first_l, first_r, npairs, cap, rc)
    rc, ur, dp, sad, kept = rig.batch(0, 1, 1, si.MB, si.MBF)
    assert rc == 0 and kept[0] > 50
