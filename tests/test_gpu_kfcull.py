"""orbm_keyframe_culling / orbm_keyframe_culling_batch_async on the GPU: host form == device form == the numpy contract == the sequential
reading of the reference (tests/second_reading_kfcull.py) on every constructed case of tests/kfcull_cases.py, on 20 of the seeded random
maps and on array-level data with entry lists of 0 .. 300 entries; the sequential rule through repeated device calls; the early-exit
path (erased == NULL) against the full path (an all-zero erased row); garbage indices; refused arguments; a captured graph replayed
after its rows were rewritten; orbm_stereo_batch_async's depth rows as the depth gate; the facade loop on mock types."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kfcull_cases as kc
import second_reading_kfcull as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xCD
OUT_KEYS = ("n_mps", "n_redundant", "cull", "slot_state", "first_cull")
ORDER = ("cand_row", "octave", "counts_kf", "kf_mp", "depth", "th_depth", "obs_off", "obs_row", "obs_slot", "obs_flags", "mp_valid", "mp_nobs")


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _kps(pkg, octave):
    k = np.zeros(octave.shape, pkg.KP_DTYPE)
    k["octave"] = octave
    k["x"] = 7.0; k["class_id"] = -1                                         # the fields around the octave are not zero
    return k


@pytest.fixture(scope="module")
def m(pkg):
    return pkg.ORBmatcher(0.9)


class Dev:
    """The arrays of one call on the device, and poisoned outputs."""

    def __init__(self, pkg, cand_row, octave, counts_kf, kf_mp, depth, th_depth, obs_off, obs_row, obs_slot, obs_flags, mp_valid, mp_nobs, erased=None):
        up = lambda a, t: None if a is None else pkg.DeviceBuffer(max(np.asarray(a).nbytes, 4)).upload(np.ascontiguousarray(a, t))
        self.pkg = pkg
        self.ncand, (self.nrows, self.cap), self.nmp, self.nobs = len(cand_row), octave.shape, len(mp_nobs), len(obs_row)
        self.th_depth = float(th_depth)
        self.cand_row, self.kps, self.counts, self.kf_mp = up(cand_row, np.int32), up(_kps(pkg, octave), pkg.KP_DTYPE), up(counts_kf, np.int32), up(kf_mp, np.int32)
        self.depth = up(depth, np.float32)
        self.off, self.row, self.slot, self.flags = up(obs_off, np.int32), up(obs_row, np.int32), up(obs_slot, np.int32), up(obs_flags, np.uint8)
        self.valid, self.mp_nobs, self.erased = up(mp_valid, np.uint8), up(mp_nobs, np.int32), up(erased, np.uint8)
        n = self.ncand
        self.n_mps, self.n_red, self.cull = pkg.DeviceBuffer(n * 4 + 4), pkg.DeviceBuffer(n * 4 + 4), pkg.DeviceBuffer(n + 4)
        self.state, self.first = pkg.DeviceBuffer(n * self.cap + 4), pkg.DeviceBuffer(8)
        self.reset()

    def reset(self):
        for b, nbytes in ((self.n_mps, self.ncand * 4 + 4), (self.n_red, self.ncand * 4 + 4), (self.cull, self.ncand + 4), (self.state, self.ncand * self.cap + 4),
                          (self.first, 8)):
            b.upload(np.full(nbytes, POISON, np.uint8))

    def enqueue(self, m, th_obs=3, th=0.9, **kw):
        p = lambda b: None if b is None else b.ptr
        a = dict(h=m.h, ncand=self.ncand, cand_row=p(self.cand_row), nrows=self.nrows, cap=self.cap, kps=p(self.kps), counts=p(self.counts),
                 kf_mp=p(self.kf_mp), depth=p(self.depth), th_depth=self.th_depth, nmp=self.nmp, nobs=self.nobs, off=p(self.off), row=p(self.row),
                 slot=p(self.slot), flags=p(self.flags), valid=p(self.valid), mp_nobs=p(self.mp_nobs), erased=p(self.erased), th_obs=th_obs, th=th,
                 n_mps=p(self.n_mps), n_red=p(self.n_red), cull=p(self.cull), state=p(self.state), first=p(self.first))
        a.update(kw)
        return m.L.orbm_keyframe_culling_batch_async(a["h"], a["ncand"], a["cand_row"], a["nrows"], a["cap"], a["kps"], a["counts"], a["kf_mp"], a["depth"],
                                                     a["th_depth"], a["nmp"], a["nobs"], a["off"], a["row"], a["slot"], a["flags"], a["valid"], a["mp_nobs"],
                                                     a["erased"], a["th_obs"], a["th"], a["n_mps"], a["n_red"], a["cull"], a["state"], a["first"])

    def fetch(self):
        n = self.ncand
        tail = lambda b, dt, cnt: np.all(b.download(np.uint8, 4, offset=cnt * np.dtype(dt).itemsize) == POISON)
        assert tail(self.n_mps, np.int32, n) and tail(self.n_red, np.int32, n) and tail(self.cull, np.uint8, n) and tail(self.state, np.uint8, n * self.cap)
        return {"n_mps": self.n_mps.download(np.int32, n), "n_redundant": self.n_red.download(np.int32, n), "cull": self.cull.download(np.uint8, n),
                "slot_state": self.state.download(np.uint8, n * self.cap).reshape(n, self.cap), "first_cull": int(self.first.download(np.int32, 1)[0])}

    def untouched(self):
        return all(np.all(b.download(np.uint8, nb) == POISON) for b, nb in ((self.n_mps, self.ncand * 4), (self.n_red, self.ncand * 4), (self.cull, self.ncand),
                                                                           (self.state, self.ncand * self.cap), (self.first, 8)))


def device_call(pkg, m):
    def call(cand_row, octave, counts_kf, kf_mp, depth, th_depth, obs_off, obs_row, obs_slot, obs_flags, mp_valid, mp_nobs, erased=None, th_obs=3,
             redundant_th=0.9):
        pad = lambda a, t: np.zeros(1, t) if len(a) == 0 else a
        d = Dev(pkg, cand_row, octave, counts_kf, kf_mp, depth, th_depth, obs_off, pad(obs_row, np.int32), pad(obs_slot, np.int32), pad(obs_flags, np.uint8),
                mp_valid, mp_nobs, erased)
        d.nobs = len(obs_row)
        assert d.enqueue(m, th_obs, redundant_th) == 0, m.L.orbm_last_error()
        m.sync()
        return d.fetch()
    return call


def host_call(pkg, m):
    def call(cand_row, octave, counts_kf, kf_mp, depth, th_depth, obs_off, obs_row, obs_slot, obs_flags, mp_valid, mp_nobs, erased=None, th_obs=3,
             redundant_th=0.9):
        out = m.KeyframeCulling(cand_row, _kps(pkg, octave), counts_kf, kf_mp, depth, th_depth, obs_off, obs_row, obs_slot, obs_flags, mp_valid, mp_nobs,
                                erased, th_obs, redundant_th)
        assert out["ncull"] == int(out["cull"].sum())
        return out
    return call


def same(a, b):
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])


def args_of(F, erased=None, th=0.9):
    return [F[k] for k in ORDER] + [erased, 3, th]


# ---- maps: the constructed cases and the seeded random maps ----------------------------------------------------------------
def _check_map(pkg, m, covisible, monocular, th, tweak=None, abort=False):
    twin = copy.deepcopy(covisible)
    cands = sr.candidates(twin)
    F = sr.flatten(cands, monocular)
    if tweak:
        tweak(F)
    if len(F["mp_nobs"]) == 0:                                              # a map without MapPoints: the call wants nmp >= 1, hand it one that is not valid
        F.update(mp_nobs=np.zeros(1, np.int32), mp_valid=np.zeros(1, np.uint8), obs_off=np.zeros(2, np.int32))
    dev, host = device_call(pkg, m), host_call(pkg, m)
    want = sr.contract(*args_of(F, None, th))
    same(dev(*args_of(F, None, th)), want)
    same(host(*args_of(F, None, th)), want)
    if tweak:
        return want
    # the full sequential rule through repeated device calls, against the sequential reading on the map itself
    def decide(kf):
        kf.SetBadFlag()
        return kf.isBad()
    rule = sr.sequential_by_contract(F, cands, decide, call=dev, redundant_th=th)
    log = sr.KeyFrameCulling(covisible, monocular, th, abort_ba=lambda: abort)
    assert len(rule) >= len(log) and (abort or len(cands) > 100 or len(rule) == len(log))
    for r, (n_mps, n_red, cull, state) in zip(log, rule):
        assert (r["n_mps"], r["n_redundant"], int(r["cull"])) == (n_mps, n_red, cull)
        assert list(state[:len(r["state"])]) == r["state"] and not state[len(r["state"]):].any()
    return want


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_constructed_cases(pkg, m, name):
    c = kc.case(name)
    want = _check_map(pkg, m, c.covisible, c.monocular, c.th, c.tweak, c.abort)
    if c.con is not None:
        assert list(zip(want["n_mps"].tolist(), want["n_redundant"].tolist(), want["cull"].tolist())) == c.con


def test_twenty_random_maps(pkg, m):
    culls = 0
    for seed in range(20):
        _, cov, monocular, th = kc.random_map(seed)
        culls += int(_check_map(pkg, m, cov, monocular, th)["cull"].sum())
    assert culls >= 10


# ---- array-level data: long lists, odd cap, garbage ------------------------------------------------------------------------
NROWS, CAP, NMP = 12, 97, 400
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 130, 300)


def synthetic(seed, ncand, garbage=False):
    """A pool of 12 rows of 97 slots, counts below cap on some rows, 400 MapPoints whose lists have 0, 1, 3, 4, 5, 63, 64, 65, 130 and 300
    entries (every length at least ten times), left / right pairs, weight-2 entries, every depth class.  garbage: rows, slots, offsets,
    kf_mp and cand_row out of range as well."""
    rng = np.random.RandomState(seed)
    counts = np.where(rng.rand(NROWS) < 0.5, CAP, rng.randint(40, CAP, NROWS)).astype(np.int32)
    counts[0] = CAP + 9                                                      # a count above cap is clamped
    octave = rng.randint(0, 8, (NROWS, CAP)).astype(np.int32)
    lens = np.concatenate([np.repeat(LENGTHS, 10), rng.choice(LENGTHS[:5] + (7, 9, 12, 20), NMP - 10 * len(LENGTHS))])
    rng.shuffle(lens)
    off, row, slot, flags = [0], [], [], []
    for n in lens:
        e = 0
        while e < n:
            r = int(rng.randint(NROWS)); s = int(rng.randint(min(counts[r], CAP)))
            f = int(rng.choice([0, 0, 4, 2, 6]))
            row.append(r); slot.append(s); flags.append(f); e += 1
            if e < n and rng.rand() < 0.25:                                 # the right entry of the same KeyFrame
                row.append(r); slot.append(int(rng.randint(min(counts[r], CAP)))); flags.append((f & 2) | 1); e += 1
        off.append(len(row))
    off, row, slot, flags = np.array(off, np.int32), np.array(row, np.int32), np.array(slot, np.int32), np.array(flags, np.uint8)
    lo = np.where(lens >= 63)[0]
    octave_low = rng.rand(len(row)) < 0.5                                   # half of the entries pass whatever the level
    for e in np.flatnonzero(octave_low):
        octave[row[e], slot[e]] = 0
    mp_nobs = rng.randint(0, 9, NMP).astype(np.int32)
    mp_nobs[lo] = rng.randint(3, 400, len(lo))
    mp_valid = (rng.rand(NMP) < 0.9).astype(np.uint8)
    cand_row = rng.permutation(NROWS)[:ncand].astype(np.int32)
    kf_mp = rng.randint(-1, NMP, (ncand, CAP)).astype(np.int32)
    kf_mp[:, :len(lo)] = rng.permutation(lo)[None, :]                       # every candidate meets every long list
    depth = rng.choice(np.array([1.0, 20.0, 35.0, 36.0, -1.0, -0.0, np.nan, 0.0], np.float32), (ncand, CAP))
    erased = (rng.rand(NROWS) < 0.25).astype(np.uint8)
    if garbage:
        g = rng.rand(len(row))
        row[g < 0.03] = rng.choice([-1, NROWS, 1 << 30, -(1 << 31)], (g < 0.03).sum())
        slot[(g > 0.03) & (g < 0.06)] = rng.choice([-1, CAP, CAP + 9, 1 << 30, -(1 << 31)], ((g > 0.03) & (g < 0.06)).sum())
        off = off.copy()
        off[5] = off[4]; off[9] = -3; off[20] = len(row) + 7; off[31] = off[30] - 2       # malformed pairs around them: empty lists
        kf_mp[rng.rand(ncand, CAP) < 0.05] = NMP; kf_mp[rng.rand(ncand, CAP) < 0.05] = -(1 << 31); kf_mp[0, 0] = (1 << 31) - 1
        if ncand > 2:
            cand_row[1] = NROWS; cand_row[2] = -1
        octave[rng.rand(NROWS, CAP) < 0.02] = (1 << 31) - 1; octave[rng.rand(NROWS, CAP) < 0.02] = -(1 << 31)
        mp_nobs[rng.rand(NMP) < 0.03] = -(1 << 31)
    return dict(cand_row=cand_row, octave=octave, counts_kf=counts, kf_mp=kf_mp, depth=depth, th_depth=np.float32(35.0), obs_off=off, obs_row=row,
                obs_slot=slot, obs_flags=flags, mp_valid=mp_valid, mp_nobs=mp_nobs), erased


@pytest.mark.parametrize("ncand", [1, 7, 12])
@pytest.mark.parametrize("garbage", [False, True], ids=["clean", "garbage"])
def test_lists_of_every_length(pkg, m, ncand, garbage):
    """Host form == device form == contract with and without erased rows; erased == NULL (the early exit) equals an all-zero erased row
    (the full walk) in all outputs.  With garbage indices the defined results come out and the device reports no error."""
    F, erased = synthetic(100 + ncand, ncand, garbage)
    dev, host = device_call(pkg, m), host_call(pkg, m)
    for th in (0.9, 0.5):
        plain = sr.contract(*args_of(F, None, th))
        with_erased = sr.contract(*args_of(F, erased, th))
        early = dev(*args_of(F, None, th))
        same(early, plain)
        same(dev(*args_of(F, np.zeros(NROWS, np.uint8), th)), early)
        same(dev(*args_of(F, erased, th)), with_erased)
        same(host(*args_of(F, erased, th)), with_erased)
    same(host(*args_of(F, None, 0.9)), sr.contract(*args_of(F, None, 0.9)))
    assert (plain["slot_state"] == 2).sum() > 5 * ncand and not np.array_equal(plain["n_redundant"], with_erased["n_redundant"])
    assert m.L.orbm_sync(m.h) == 0
    mono = dict(F, depth=None, mp_valid=None)                                # the NULL forms of depth and mp_valid
    same(dev(*args_of(mono, erased, 0.9)), sr.contract(*args_of(mono, erased, 0.9)))


def test_slot_state_is_optional(pkg, m):
    F, erased = synthetic(5, 7)
    d = Dev(pkg, *[F[k] for k in ORDER], erased)
    assert d.enqueue(m, state=None, first=None) == 0, m.L.orbm_last_error()
    m.sync()
    want = sr.contract(*args_of(F, erased))
    assert np.array_equal(d.n_mps.download(np.int32, 7), want["n_mps"]) and np.array_equal(d.cull.download(np.uint8, 7), want["cull"])
    assert np.all(d.state.download(np.uint8, 7 * CAP) == POISON) and np.all(d.first.download(np.uint8, 8) == POISON)


def test_refused_arguments_enqueue_nothing(pkg, m):
    F, erased = synthetic(6, 7)
    d = Dev(pkg, *[F[k] for k in ORDER], erased)
    for kw in (dict(cand_row=None), dict(kps=None), dict(counts=None), dict(kf_mp=None), dict(off=None), dict(row=None), dict(slot=None), dict(flags=None),
               dict(mp_nobs=None), dict(n_mps=None), dict(n_red=None), dict(cull=None), dict(ncand=0), dict(ncand=-1), dict(nrows=0), dict(cap=0), dict(nmp=0),
               dict(nobs=-1), dict(th_obs=-1), dict(h=None)):
        assert d.enqueue(m, **kw) == -2, kw
    for kw in (dict(ncand=65536), dict(cap=65536), dict(nmp=(1 << 20) + 1), dict(nrows=1 << 16, cap=1 << 15)):
        assert d.enqueue(m, **kw) == -3, kw
    m.sync()
    assert d.untouched()
    n_mps = np.full(7, -7, np.int32)
    rc = m.L.orbm_keyframe_culling(m.h, 7, _vp(F["cand_row"]), NROWS, CAP, None, _vp(F["counts_kf"]), _vp(F["kf_mp"]), None, 35.0, NMP, len(F["obs_row"]),
                                   _vp(F["obs_off"]), _vp(F["obs_row"]), _vp(F["obs_slot"]), _vp(F["obs_flags"]), None, _vp(F["mp_nobs"]), None, 3, 0.9,
                                   _vp(n_mps), _vp(n_mps), _vp(n_mps), None, None)
    assert rc == -2 and np.all(n_mps == -7) and b"kps_kf" in m.L.orbm_last_error()


def test_captured_replay_follows_rewritten_rows(pkg, synth):
    """Captured on its FIRST call behind an extraction (a step graph holds one); erased, kf_mp and cand_row are then rewritten and the graph
    replayed: the outputs follow, and a second replay repeats them (nothing accumulates)."""
    L = pkg.lib()
    cw = ch = 239; stride = 256
    pad = np.zeros((ch, stride), np.uint8); pad[:, :cw] = synth.gen_image(cw, ch, 9100)
    dimg = pkg.DeviceBuffer(pad.nbytes).upload(pad)
    arr = (C.c_void_p * 1)(dimg.ptr)
    ex = pkg.ORBextractor(500, max_size=(cw, ch), max_batch=1)
    ex.enqueue_device(arr, cw, ch, stride); ex.sync()                        # the extractor's own first call is eager
    m2 = pkg.ORBmatcher(0.9)                                                 # a fresh handle: its first KeyFrameCulling call is the captured one
    assert L.orbm_set_stream(m2.h, L.orbx_stream(ex.h)) == 0
    F, erased = synthetic(7, 7)
    d = Dev(pkg, *[F[k] for k in ORDER], erased)
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    ex.enqueue_device(arr, cw, ch, stride)
    assert d.enqueue(m2) == 0, L.orbm_last_error()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    assert d.untouched()                                                    # captured, not run
    rng = np.random.RandomState(3)
    F2 = dict(F, kf_mp=rng.randint(-1, NMP, F["kf_mp"].shape).astype(np.int32), cand_row=F["cand_row"][::-1].copy())
    erased2 = 1 - erased
    for Fi, er in ((F, erased), (F2, erased2)):
        d.kf_mp.upload(Fi["kf_mp"]); d.cand_row.upload(Fi["cand_row"]); d.erased.upload(er)
        want = sr.contract(*args_of(Fi, er))
        for _ in range(2):
            d.reset()
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            ex.sync()
            same(d.fetch(), want)
    assert not np.array_equal(sr.contract(*args_of(F, erased))["n_mps"], want["n_mps"])


def test_stereo_depth_rows_feed_the_gate(pkg, synth):
    """The chain that feeds it: the depth rows orbm_stereo_batch_async leaves on the device are the call's depth, the extractor's result
    block its KeyFrame pool, nothing copied in between."""
    W, H, P = 752, 480, 2
    pairs = [synth.gen_stereo_pair(W, H, 500 + i) for i in range(P)]
    imgs = [p[0] for p in pairs] + [p[1] for p in pairs]
    stride = (W + 63) // 64 * 64
    dev = pkg.DeviceBuffer(2 * P * stride * H)
    for i, im in enumerate(imgs):
        pad = np.zeros((H, stride), np.uint8); pad[:, :W] = im
        dev.upload(pad, offset=i * stride * H)
    arr = (C.c_void_p * (2 * P))(*[dev.ptr + i * stride * H for i in range(2 * P)])
    L = pkg.lib()
    ex = pkg.ORBextractor(800, 1.2, 8, max_size=(W, H), max_batch=2 * P)
    mt = pkg.ORBmatcher(0.6)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    cap = ex.cap
    ex.enqueue_device(arr, W, H, stride, np.zeros(4 * P, np.int32))
    r = ex.result_device()
    ur, dp, sad, kept = pkg.DeviceBuffer(P * cap * 4), pkg.DeviceBuffer(P * cap * 4), pkg.DeviceBuffer(P * cap * 4), pkg.DeviceBuffer(P * 4)
    assert L.orbm_stereo_batch_async(mt.h, ex.h, 0, P, P, r["kps"], r["desc"], r["counts"], cap, 0.11, 47.9, ur.ptr, dp.ptr, sad.ptr, kept.ptr) == 0, L.orbm_last_error()
    ex.sync()
    res = ex.fetch_all()
    counts = np.array([len(res[i][1]) for i in range(2 * P)], np.int32)
    octave = np.zeros((2 * P, cap), np.int32)
    for i in range(2 * P):
        octave[i, :counts[i]] = res[i][1]["octave"]
    depth = dp.download(np.float32, P * cap).reshape(P, cap)
    rng = np.random.RandomState(11)
    nmp = 300
    # MapPoint j sits in slot perm[k][j] of left frame k and is seen by both left frames and three to five right-frame slots
    kf_mp = np.full((P, cap), -1, np.int32)
    off, row, slot = [0], [], []
    for j in range(nmp):
        for k in range(P):
            s = int(rng.randint(counts[k]))
            if kf_mp[k, s] < 0:
                kf_mp[k, s] = j
                row.append(k); slot.append(s)
        for _ in range(int(rng.randint(3, 6))):
            rr = int(rng.randint(P, 2 * P)); row.append(rr); slot.append(int(rng.randint(counts[rr])))
        off.append(len(row))
    F = dict(cand_row=np.arange(P, dtype=np.int32), octave=octave, counts_kf=counts, kf_mp=kf_mp, depth=depth, th_depth=np.float32(35 * 0.11),
             obs_off=np.array(off, np.int32), obs_row=np.array(row, np.int32), obs_slot=np.array(slot, np.int32),
             obs_flags=np.zeros(len(row), np.uint8), mp_valid=None, mp_nobs=np.diff(off).astype(np.int32))
    want = sr.contract(*args_of(F))
    d = Dev(pkg, *[F[k] for k in ORDER])
    assert d.enqueue(mt, kps=r["kps"], counts=r["counts"], depth=dp.ptr) == 0, L.orbm_last_error()
    mt.sync()
    got = d.fetch()
    same(got, want)
    gated = sr.contract(*args_of(dict(F, depth=None)))
    print("chain: n_mps %s of %s without the gate, %s redundant" % (want["n_mps"], gated["n_mps"], want["n_redundant"]))
    assert np.all(want["n_mps"] > 20) and np.all(want["n_mps"] < gated["n_mps"]) and want["n_redundant"].sum() > 10


def test_cpp_facade_keyframe_culling(pkg, tmp_path):
    """facade/KeyFrameCulling.h's loop on mock KeyFrame / MapPoint types against the reference's loop in plain C++ in the same file."""
    pkg.build()
    exe = str(tmp_path / "facade_kfcull_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tests", "facade_kfcull_smoke.cpp"),
                           "-L", os.path.join(ROOT, "orb-slam3_amd"), "-lorbslam3_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "orb-slam3_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "need-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "facade_kfcull_smoke ok" in out.stdout, out.stdout + out.stderr
