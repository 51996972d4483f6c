"""DetectCommonRegionsFromBoW's two searches chained on ONE handle and the SAME extractor result blocks, as INTEGRATION.md lays it out:
M8 (orbm_search_by_bow_kf_batch_async) matches the current KeyFrame rows of pool K against candidate rows of pool F; the host then
picks the points -- the MapPoints M8 matched become vpMatched (matched_in, and spAlreadyFound: not valid), the window's other MapPoints
become the queries --; M6 (orbm_search_by_projection_sim3_batch_async) searches the same rows of pool K through the grid built over that
block.  Both steps are checked against the host entry points and the oracle."""
import types

import numpy as np
import pytest

import test_gpu_bow_kf_batch as T8
import test_gpu_sim3_projection_batch as T6
from test_gpu_bow_batch import NF_IMG, _vocab, pools  # noqa: F401  (fixture + helpers)
from test_gpu_reloc_batch import H, W, _inv

pytestmark = pytest.mark.gpu


class BlockPool:
    """The view of an extractor result block (test_gpu_bow_batch.Pool) that the M6 helpers read: device rows, counts, the block's grid."""

    def __init__(self, pkg, mt, K):
        ptr = lambda v: types.SimpleNamespace(ptr=v)                        # noqa: E731
        self.pkg, self.L, self.m = pkg, pkg.lib(), mt
        self.R, self.cap = K.rows, K.cap
        self.counts = np.array([len(K.kps(r)) for r in range(K.rows)], np.int32)
        self.sf = np.ascontiguousarray(K.ex.GetScaleFactors(), np.float32); self.nlev = len(self.sf)
        self.w, self.h = W, H
        self.inv_w, self.inv_h = _inv(64, W), _inv(48, H)
        self.bounds = np.array([0, W, 0, H], np.float32)
        self.dk, self.dd, self.dc = ptr(K.r["kps"]), ptr(K.r["desc"]), ptr(K.r["counts"])
        self.gs = pkg.DeviceBuffer(self.R * 3073 * 4); self.gi = pkg.DeviceBuffer(self.R * self.cap * 4)
        self._K = K

    def grid(self):
        assert self.L.orbm_grid_build_batch_async(self.m.h, self.dk.ptr, self.dc.ptr, self.R, self.cap, 0.0, 0.0, self.inv_w, self.inv_h,
                                                  self.gs.ptr, self.gi.ptr) == 0, self.L.orbm_last_error()

    def row(self, r):
        return self._K.kps(r), self._K.desc(r)


@pytest.mark.parametrize("form,th,ratio", [(1, 8, 1.5), (0, 5, 1.0)])
def test_bow_then_projection_on_the_same_pools(pkg, oracle, synth, pools, form, th, ratio):
    mt, K, F = pools
    L = pkg.lib()
    OM = oracle._oracle_matcher_class()()
    voc = _vocab(pkg, synth, mt, 10, 6)
    K.transform(voc, 4); F.transform(voc, 4)
    # step 1, M8: current KeyFrames (K rows) against their candidates (F rows: the same scenes, and one unrelated image)
    row1 = [0, 1, 2, 3, 0]; row2 = [0, 1, 2, 3, NF_IMG]
    g1, g2 = np.ones(K.rows * K.cap, np.uint8), np.ones(F.rows * F.cap, np.uint8)
    m12, cnt = T8._run(pkg, mt, K, F, row1, row2, g1, g2, 0.9, 1)
    w, _ = T8._check(oracle, mt, K, F, row1, row2, g1, g2, 0.9, 1, m12, cnt)
    assert w[:4].min() > 100, w
    # step 2, the host picks the points: per pair the KeyFrame slots M8 matched are vpMatched; the candidate window's remaining MapPoints
    # (seen from keypoints M8 left unmatched, a few from matched ones) are the queries, the matched MapPoints among them already found
    pool = BlockPool(pkg, mt, K)
    pool.grid()
    rng = np.random.default_rng(th * 7 + form)
    pairs = []
    for p, r in enumerate(row1):
        n1 = int(pool.counts[r])
        matched = np.zeros(K.cap, np.uint8); matched[:n1] = m12[p, :n1] >= 0
        free = np.flatnonzero(matched[:n1] == 0); taken = np.flatnonzero(matched[:n1])
        src = np.concatenate([rng.choice(free, 500), rng.choice(taken, 60) if len(taken) else free[:0]])
        q = T6.mappoints(rng, pool, r, len(src), src=src)
        q["valid"][500:] = 0                                                # spAlreadyFound: the MapPoints M8 matched
        q.update(row=r, matched=matched)
        pairs.append(q)
    # step 3, M6 on the same handle and the same block rows
    call = T6.Call(pool, pairs, rng=rng)
    got = call.run(th, ratio, form)
    per = T6.check(pkg, OM, pool, call, got, th, ratio, form)[0]
    assert (per > 0).sum() > len(per) / 2 and per.sum() > 100, per          # on the ORACLE's counts
    for p, r in enumerate(row1):                                            # no M6 match lands on a slot M8 filled
        n1 = int(pool.counts[r])
        assert not np.any((got[0][p, :n1] >= 0) & (m12[p, :n1] >= 0)), p
    assert L.orbm_sync(mt.h) == 0
