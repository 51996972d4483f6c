"""SearchByBoW(KeyFrame, Frame) (M7) for a batch of pairs: orbm_bow_transform_batch_async + orbm_search_by_bow_batch_async against a
loop of host orbm_search_by_bow calls over the same pairs.

Two shapes at 752 x 480 / 1000 features with an ORBvoc-sized synthetic vocabulary (synth.gen_vocabulary(10, 6), levelsup 4):
- track: 64 TrackReferenceKeyFrame pairs, frame p (the right image of a stereo pair) against KeyFrame p (its left image), nnratio 0.7;
- reloc: one frame against 32 candidate KeyFrames (f_row all equal), nnratio 0.75.
The batched search is timed eagerly (device events of the handle, orbm_last_timing, and the host clock around enqueue + sync) and as
a captured graph replay (host clock, the capture also holds the frame extraction the graph API requires, timed alone and subtracted);
the host loop is one orbm_search_by_bow per pair fed with host FeatureVectors.  All paths must produce the same rows.  Prints one JSON
line per measurement.

--fuzz N: N random calls (pairs per call, feature counts, nnratio 0.5-1.0, rotation check, good-mask rate, levelsup 1 .. L on a (10, 3)
or (10, 4) vocabulary, stopped words, NULL weights, out-of-range rows) compared pair by pair with the oracle's SearchByBoW; prints
one JSON line with the mismatch count.

--fisheye: the two-camera M7 (F.Nleft != -1) at the C4 shape -- 512 x 512, 1500 features per camera, the same vocabulary, levelsup 4 --
for 1 / 8 / 64 (stacked KeyFrame row, left frame row, right frame row) triples: orbm_search_by_bow_fisheye_batch_async against the loop
of host orbm_search_by_bow_fisheye calls it replaces, and against the one-camera orbm_search_by_bow_batch_async on the left rows
alone.  The three are timed in alternation (host clock around enqueue + sync for the device calls), at least 30 calls each; medians
with quartiles, one JSON line per measurement.  All rows must be equal."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
pkg = importlib.import_module("orb-slam3_amd")
synth = importlib.import_module("orb-slam3_amd.synth")

W, H, REPS = 752, 480, 20


def fv(nodes, keep):
    """FeatureVector CSR as DBoW2 builds it: nodes ascending, indices ascending, only the features with keep set."""
    idx = np.flatnonzero(keep).astype(np.int32)
    order = idx[np.argsort(nodes[idx], kind="stable")]
    un, start = np.unique(nodes[order], return_index=True)
    return un.astype(np.int32), np.append(start, len(order)).astype(np.int32), order.astype(np.int32)


class Pool:
    """Device images -> one extractor result block -> node ids and weights of every slot."""

    def __init__(self, imgs, nfeatures, m, w=W, h=H):
        self.L = pkg.lib()
        self.w, self.h = w, h
        stride = (w + 63) // 64 * 64
        self.stride = stride
        self.dev = pkg.DeviceBuffer(len(imgs) * stride * h)
        for i, im in enumerate(imgs):
            pad = np.zeros((h, stride), np.uint8); pad[:, :w] = im
            self.dev.upload(pad, offset=i * stride * h)
        self.arr = (C.c_void_p * len(imgs))(*[self.dev.ptr + i * stride * h for i in range(len(imgs))])
        self.ex = pkg.ORBextractor(nfeatures, max_size=(w, h), max_batch=len(imgs))
        self.extract()
        self.ex.sync()
        self.r = self.ex.result_device()
        self.rows, self.cap = len(imgs), self.ex.cap
        self.res = self.ex.fetch_all()
        self.node = pkg.DeviceBuffer(4 * self.rows * self.cap); self.weight = pkg.DeviceBuffer(8 * self.rows * self.cap)
        self.m = m

    def extract(self):
        self.ex.enqueue_device(self.arr, self.w, self.h, self.stride, np.zeros(4 * len(self.arr), np.int32))

    def transform(self, voc, levelsup):
        assert self.L.orbm_bow_transform_batch_async(self.m.h, voc.h, self.r["desc"], self.rows * self.cap, levelsup, None, self.node.ptr,
                                                     self.weight.ptr) == 0, self.L.orbm_last_error()

    def host(self):
        self.m.sync()
        n = self.rows * self.cap
        self.h_node = self.node.download(np.int32, n).reshape(self.rows, self.cap)
        self.h_weight = self.weight.download(np.float64, n).reshape(self.rows, self.cap)


def search(L, m, K, F, P, dk, df, dg, nnratio, check_ori, fm, nm, weights=True):
    rc = L.orbm_search_by_bow_batch_async(m.h, P, K.rows, K.cap, K.r["kps"], K.r["desc"], K.r["counts"], K.node.ptr,
                                          K.weight.ptr if weights else None, dg.ptr,
                                          F.rows, F.cap, F.r["kps"], F.r["desc"], F.r["counts"], F.node.ptr, F.weight.ptr if weights else None,
                                          None if dk is None else dk.ptr, None if df is None else df.ptr, float(nnratio), int(check_ori), fm.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()


def ref_inputs(K, F, kr, fr, good, weights=True):
    kk, dkk = K.res[kr][1], K.res[kr][2]; kf_, df_ = F.res[fr][1], F.res[fr][2]
    nk, nf = len(kk), len(kf_)
    g = np.ascontiguousarray(good[kr * K.cap: kr * K.cap + nk])
    keep_k = K.h_weight[kr, :nk] > 0 if weights else np.ones(nk, bool)
    keep_f = F.h_weight[fr, :nf] > 0 if weights else np.ones(nf, bool)
    return kk, dkk, g, fv(K.h_node[kr, :nk], keep_k), kf_, df_, fv(F.h_node[fr, :nf], keep_f)


def bench():
    L = pkg.lib()
    m = pkg.ORBmatcher(0.7)
    voc = pkg.ORBVocabulary(m, synth.gen_vocabulary(10, 6, seed=7))
    NP = 64
    pairs = [synth.gen_stereo_pair(W, H, 700 + i) for i in range(NP)]
    K = Pool([p[0] for p in pairs], 1000, m)
    F = Pool([p[1] for p in pairs], 1000, m)
    assert L.orbm_set_stream(m.h, L.orbx_stream(F.ex.h)) == 0
    for shape, P, kf_row, f_row, nnratio in (("track", NP, None, None, 0.7), ("reloc", 32, list(range(32)), [5] * 32, 0.75)):
        dk = None if kf_row is None else pkg.DeviceBuffer(4 * P).upload(np.asarray(kf_row, np.int32))
        df = None if f_row is None else pkg.DeviceBuffer(4 * P).upload(np.asarray(f_row, np.int32))
        good = np.ones(K.rows * K.cap, np.uint8); dg = pkg.DeviceBuffer(good.nbytes).upload(good)
        fm = pkg.DeviceBuffer(4 * P * F.cap); nm = pkg.DeviceBuffer(4 * P)
        K.transform(voc, 4); F.transform(voc, 4)
        K.host(); F.host()

        def call():
            search(L, m, K, F, P, dk, df, dg, nnratio, 1, fm, nm)

        for _ in range(3):
            call()
        m.sync()
        dev_ms, wall_ms = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            call()
            m.sync()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(m.timing_ms())
        rows = fm.download(np.int32, P * F.cap).reshape(P, F.cap); counts = nm.download(np.int32, P)
        # captured replay: the graph API captures a step that starts with an extraction; that extraction is timed alone and subtracted
        def step(with_search):
            F.extract()
            if with_search:
                K.transform(voc, 4); F.transform(voc, 4)
                call()
        graph_ms = {}
        for ws in (False, True):
            assert L.orbx_capture_begin(F.ex.h, 0) == 0, L.orbx_last_error()
            step(ws)
            assert L.orbx_capture_end(F.ex.h) == 0, L.orbx_last_error()
            for _ in range(3):
                assert L.orbx_graph_launch(F.ex.h, 0) == 0
            F.ex.sync()
            t = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                assert L.orbx_graph_launch(F.ex.h, 0) == 0
                F.ex.sync()
                t.append((time.perf_counter() - t0) * 1e3)
            graph_ms[ws] = float(np.median(t))
        same_graph = np.array_equal(fm.download(np.int32, P * F.cap).reshape(P, F.cap), rows) and np.array_equal(nm.download(np.int32, P), counts)
        print(json.dumps(dict(path="batch", shape=shape, pairs=P, nnratio=nnratio, levelsup=4, search_device_ms_per_call=float(np.median(dev_ms)),
                              search_device_ms_per_pair=float(np.median(dev_ms)) / P, search_wall_ms_per_call=float(np.median(wall_ms)),
                              graph_step_ms=graph_ms[True], graph_extract_only_ms=graph_ms[False],
                              graph_transform_search_ms=graph_ms[True] - graph_ms[False], replay_equals_eager=bool(same_graph),
                              matches=int(counts.sum()))), flush=True)
        kr_ = kf_row or list(range(P)); fr_ = f_row or list(range(P))
        args = [ref_inputs(K, F, kr_[p], fr_[p], good) for p in range(P)]
        out = [m.SearchByBoW(*a, nnratio, True) for a in args]                 # warm-up pass
        same = all(int(counts[p]) == out[p][0] and np.array_equal(rows[p, :len(args[p][4])], out[p][1]) for p in range(P))
        t0 = time.perf_counter()
        for _ in range(3):
            for a in args:
                m.SearchByBoW(*a, nnratio, True)
        per_call = (time.perf_counter() - t0) * 1e3 / (3 * P)
        print(json.dumps(dict(path="host_loop", shape=shape, pairs=P, nnratio=nnratio, wall_ms_per_call=per_call, wall_ms_per_batch=per_call * P,
                              rows_equal_batch=bool(same))), flush=True)
        assert same and same_graph, "batched rows differ from the host rows"
    assert L.orbm_set_stream(m.h, None) == 0
    K.ex.close(); F.ex.close()


def _q(t):
    q = np.percentile(np.asarray(t, np.float64), [25, 50, 75])
    return dict(median=float(q[1]), q25=float(q[0]), q75=float(q[2]), calls=len(t))


def fisheye_bench(reps=30):
    L = pkg.lib()
    m = pkg.ORBmatcher(0.7)
    voc = pkg.ORBVocabulary(m, synth.gen_vocabulary(10, 6, seed=7))
    FW = FH = 512
    NR, NFEAT = 64, 1500                                                    # rigs, features per camera
    rng = np.random.default_rng(12)
    kf_imgs = [synth.gen_stereo_pair(FW, FH, 1300 + i) for i in range(NR)]
    later = lambda im: np.clip(np.roll(im, 3, axis=1).astype(np.float64) + rng.normal(0, 3.0, im.shape), 0, 255).astype(np.uint8)
    # frame pool: one result block, rows 0 .. NR-1 left and NR .. 2 NR-1 right (the rig a little later)
    F = Pool([later(p[0]) for p in kf_imgs] + [later(p[1]) for p in kf_imgs], NFEAT, m, FW, FH)
    F.transform(voc, 4); F.host()
    # KeyFrame pool: a caller-gathered pool of STACKED rows (left features then right) from a block of the KeyFrame images
    G = Pool([p[0] for p in kf_imgs] + [p[1] for p in kf_imgs], NFEAT, m, FW, FH)
    capk = 2 * G.cap
    kps = np.zeros((NR, capk), pkg.KP_DTYPE); desc = np.zeros((NR, capk, 32), np.uint8); cnt = np.zeros(NR, np.int32)
    for r in range(NR):
        (_, kl, dl), (_, kr, dr) = G.res[r], G.res[NR + r]
        n = len(kl) + len(kr); cnt[r] = n
        kps[r, :n] = np.concatenate([kl, kr]); desc[r, :n] = np.concatenate([dl, dr])
    G.ex.close()
    dK = {k: pkg.DeviceBuffer(a.nbytes).upload(a) for k, a in (("kps", kps), ("desc", desc), ("counts", cnt))}
    knode = pkg.DeviceBuffer(4 * NR * capk); kweight = pkg.DeviceBuffer(8 * NR * capk)
    assert L.orbm_bow_transform_batch_async(m.h, voc.h, dK["desc"].ptr, NR * capk, 4, None, knode.ptr, kweight.ptr) == 0, L.orbm_last_error()
    m.sync()
    h_knode = knode.download(np.int32, NR * capk).reshape(NR, capk); h_kweight = kweight.download(np.float64, NR * capk).reshape(NR, capk)
    good = np.ones((NR, capk), np.uint8); dg = pkg.DeviceBuffer(good.nbytes).upload(good)
    for P in (1, 8, 64):
        kf_row = np.arange(P, dtype=np.int32); fl_row = np.arange(P, dtype=np.int32); fr_row = (NR + np.arange(P)).astype(np.int32)
        dk, dl, dr = [pkg.DeviceBuffer(4 * P).upload(a) for a in (kf_row, fl_row, fr_row)]
        ml = pkg.DeviceBuffer(4 * P * F.cap); mr = pkg.DeviceBuffer(4 * P * F.cap); nm = pkg.DeviceBuffer(4 * P)
        m1 = pkg.DeviceBuffer(4 * P * F.cap); n1 = pkg.DeviceBuffer(4 * P)

        def batch():
            rc = L.orbm_search_by_bow_fisheye_batch_async(m.h, P, NR, capk, dK["kps"].ptr, dK["desc"].ptr, dK["counts"].ptr, knode.ptr, kweight.ptr, dg.ptr,
                                                          F.rows, F.cap, F.r["kps"], F.r["desc"], F.r["counts"], F.node.ptr, F.weight.ptr,
                                                          dk.ptr, dl.ptr, dr.ptr, 0.7, 1, ml.ptr, mr.ptr, nm.ptr)
            assert rc == 0, L.orbm_last_error()
            m.sync()
            return m.timing_ms()

        def left_only():
            rc = L.orbm_search_by_bow_batch_async(m.h, P, NR, capk, dK["kps"].ptr, dK["desc"].ptr, dK["counts"].ptr, knode.ptr, kweight.ptr, dg.ptr,
                                                  F.rows, F.cap, F.r["kps"], F.r["desc"], F.r["counts"], F.node.ptr, F.weight.ptr,
                                                  dk.ptr, dl.ptr, 0.7, 1, m1.ptr, n1.ptr)
            assert rc == 0, L.orbm_last_error()
            m.sync()
            return m.timing_ms()

        args = []
        for p in range(P):
            (_, kl, dl_), (_, kr, dr_) = F.res[p], F.res[NR + p]
            nk, nl, nr = int(cnt[p]), len(kl), len(kr)
            node_f = np.concatenate([F.h_node[p, :nl], F.h_node[NR + p, :nr]]); wt_f = np.concatenate([F.h_weight[p, :nl], F.h_weight[NR + p, :nr]])
            args.append((np.ascontiguousarray(kps[p, :nk]), np.ascontiguousarray(desc[p, :nk]), good[p, :nk], fv(h_knode[p, :nk], h_kweight[p, :nk] > 0),
                         np.concatenate([kl, kr]), np.concatenate([dl_, dr_]), nl, fv(node_f, wt_f > 0), 0.7, True))

        def host_loop():
            return [m.SearchByBoWFisheye(*a) for a in args]

        for _ in range(3):                                                  # warm every path at this shape
            batch(); left_only(); out = host_loop()
        rows_l = ml.download(np.int32, P * F.cap).reshape(P, F.cap); rows_r = mr.download(np.int32, P * F.cap).reshape(P, F.cap)
        counts = nm.download(np.int32, P)
        same = all(int(counts[p]) == out[p][0] and np.array_equal(rows_l[p, :args[p][6]], out[p][1][:args[p][6]]) and
                   np.array_equal(rows_r[p, :len(args[p][4]) - args[p][6]], out[p][1][args[p][6]:]) for p in range(P))
        t = dict(batch_wall=[], batch_dev=[], left_wall=[], left_dev=[], host=[])
        for _ in range(reps):                                               # alternate the three paths
            t0 = time.perf_counter(); d = batch(); t["batch_wall"].append((time.perf_counter() - t0) * 1e3); t["batch_dev"].append(d)
            t0 = time.perf_counter(); d = left_only(); t["left_wall"].append((time.perf_counter() - t0) * 1e3); t["left_dev"].append(d)
            t0 = time.perf_counter(); host_loop(); t["host"].append((time.perf_counter() - t0) * 1e3)
        common = dict(shape="c4_fisheye", pairs=P, width=FW, height=FH, features_per_camera=NFEAT, nnratio=0.7, levelsup=4,
                      mean_left=float(np.mean([a[6] for a in args])), mean_right=float(np.mean([len(a[4]) - a[6] for a in args])))
        print(json.dumps(dict(path="fisheye_batch", **common, wall_ms_per_call=_q(t["batch_wall"]), device_ms_per_call=_q(t["batch_dev"]),
                              matches=int(counts.sum()), rows_equal_host=bool(same))), flush=True)
        print(json.dumps(dict(path="one_camera_batch_left_rows", **common, wall_ms_per_call=_q(t["left_wall"]), device_ms_per_call=_q(t["left_dev"]),
                              matches=int(n1.download(np.int32, P).sum()))), flush=True)
        print(json.dumps(dict(path="fisheye_host_loop", **common, wall_ms_per_batch=_q(t["host"]),
                              wall_ms_per_call=float(np.median(t["host"])) / P)), flush=True)
        assert same, "batched rows differ from the host rows"
    F.ex.close()


def fuzz(n, seed):
    import orbref
    orbref.lib()
    OM = orbref._oracle_matcher_class()()
    rng = np.random.default_rng(seed)
    L = pkg.lib()
    m = pkg.ORBmatcher(0.7)
    vocs = {(10, 3): pkg.ORBVocabulary(m, synth.gen_vocabulary(10, 3, seed=3)), (10, 4): pkg.ORBVocabulary(m, synth.gen_vocabulary(10, 4, seed=4))}
    tree = synth.gen_vocabulary(10, 3, seed=5)
    leaves = np.flatnonzero(tree["is_leaf"]); tree["weight"][rng.choice(leaves, len(leaves) // 5, replace=False)] = 0.0
    vocs["stop"] = pkg.ORBVocabulary(m, tree)
    pairs = matches = mismatches = 0
    cases = []
    for c in range(n):
        nk_img, nf_img = int(rng.integers(1, 5)), int(rng.integers(1, 4))
        nfk, nff = int(rng.choice([50, 300, 1000, 2500])), int(rng.choice([50, 300, 1000, 2000]))
        seeds = rng.integers(0, 10 ** 6, max(nk_img, nf_img))
        st = [synth.gen_stereo_pair(W, H, int(s)) for s in seeds]
        K = Pool([st[i][0] for i in range(nk_img)], nfk, m)
        F = Pool([st[i][1] for i in range(nf_img)], nff, m)
        vk = ["(10, 3)", "(10, 4)", "stop"][int(rng.integers(0, 3))]
        voc = vocs[{"(10, 3)": (10, 3), "(10, 4)": (10, 4)}.get(vk, "stop")]
        Lv = 4 if vk == "(10, 4)" else 3
        levelsup = int(rng.integers(1, Lv + 1))
        K.transform(voc, levelsup); F.transform(voc, levelsup); K.host(); F.host()
        P = int(rng.integers(1, 9))
        kf_row = rng.integers(-1, nk_img + 1, P).astype(np.int32); f_row = rng.integers(-1, nf_img + 1, P).astype(np.int32)
        inside = rng.random(P) < 0.8                                           # most pairs in range
        kf_row[inside] = np.minimum(np.maximum(kf_row[inside], 0), nk_img - 1); f_row[inside] = np.minimum(np.maximum(f_row[inside], 0), nf_img - 1)
        grate = float(rng.choice([1.0, 0.5, 0.1]))
        good = (rng.random(K.rows * K.cap) < grate).astype(np.uint8)
        nnratio = float(rng.uniform(0.5, 1.0)); check_ori = int(rng.integers(0, 2)); weights = bool(rng.random() < 0.8)
        dk = pkg.DeviceBuffer(4 * P).upload(kf_row); df = pkg.DeviceBuffer(4 * P).upload(f_row); dg = pkg.DeviceBuffer(good.nbytes).upload(good)
        fm = pkg.DeviceBuffer(4 * P * F.cap); nm = pkg.DeviceBuffer(4 * P)
        search(L, m, K, F, P, dk, df, dg, nnratio, check_ori, fm, nm, weights)
        assert L.orbm_sync(m.h) == 0, L.orbm_last_error()
        rows = fm.download(np.int32, P * F.cap).reshape(P, F.cap); counts = nm.download(np.int32, P)
        bad = 0
        for p in range(P):
            kr, fr = int(kf_row[p]), int(f_row[p])
            if not (0 <= kr < K.rows and 0 <= fr < F.rows):
                ok = counts[p] == 0 and np.all(rows[p] == -1)
            else:
                a = ref_inputs(K, F, kr, fr, good, weights)
                n_ref, row_ref = OM.SearchByBoW(*a, nnratio, bool(check_ori))
                nf = len(a[4])
                ok = counts[p] == n_ref and np.array_equal(rows[p, :nf], row_ref) and np.all(rows[p, nf:] == -1)
                matches += n_ref
            bad += int(not ok); pairs += 1
        mismatches += bad
        cases.append(dict(pairs=P, kf_rows=nk_img, f_rows=nf_img, kf_features=nfk, f_features=nff, vocab=vk, levelsup=levelsup,
                          nnratio=round(nnratio, 3), check_ori=check_ori, good_rate=grate, weights=weights, mismatched_pairs=bad))
        K.ex.close(); F.ex.close()
    print(json.dumps(dict(path="fuzz", seed=seed, calls=n, pairs=pairs, matches=int(matches), mismatches=mismatches, cases=cases)), flush=True)
    return mismatches


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fuzz", type=int, default=0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--fisheye", action="store_true")
    a = ap.parse_args()
    if a.fisheye:
        fisheye_bench()
        sys.exit(0)
    if a.fuzz:
        sys.exit(1 if fuzz(a.fuzz, a.seed) else 0)
    bench()
