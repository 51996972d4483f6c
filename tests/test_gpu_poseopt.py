"""orbm_pose_optimization, orbm_pose_optimization_batch_async and orbm_discard_outliers_batch_async on the GPU: device form == host form
== the g++ build of csrc/orbm_poseopt.h (tests/poseopt_header.cpp), bit for bit, pose included; all three against the second reading by
the header test's rule; two runs and a graph replay give identical bits; a captured {pose optimisation, discard, votes} chain follows
rewritten tcw_in and q_mp; tcw_out may alias tcw_in; garbage indices and octaves; refused arguments; the discard kernel == numpy; the
facade.  Three frames per call with different counts at cap 600, n_corr on every edge of a wave and of the workgroup; one frame at the
largest cap the kernel stages in LDS and one past it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseopt_cases as pc          # noqa: E402
import poseopt_io as io             # noqa: E402
import poseopt_results as res       # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xCD
LDS_CAP = 1536                                                               # csrc: PO_LDS_CAP
E_INVALID, E_CAPACITY = -2, -3

BATCHES = [["ncorr_0", "ncorr_513", "ncorr_3"], ["ncorr_2", "ncorr_255", "ncorr_9"], ["ncorr_10", "ncorr_256", "ncorr_63"],
           ["ncorr_64", "ncorr_257", "ncorr_65"], ["all_mono", "all_stereo", "mixed"], ["readmit", "empty_round1", "behind_camera"],
           ["stereo_invz", "noise_free", "rejected_last_trial"], ["restart_matters", "start_at_optimum", "ncorr_10"]]


@pytest.fixture(scope="module")
def m(pkg):
    return pkg.ORBmatcher(0.9)


@pytest.fixture(scope="module")
def header_exe(tmp_path_factory):
    return io.build_program(tmp_path_factory.mktemp("poseopt_gpu"))


def _up(pkg, a, t=None):
    a = np.ascontiguousarray(a, t)
    return pkg.DeviceBuffer(max(a.nbytes, 4)).upload(a)


class Batch:
    """The flat arrays of one call: block row 0 is a decoy, frame f of the call is block row first + f = 1 + f."""

    def __init__(self, cases, cap, garbage=False):
        self.cases, self.cap, self.nf, self.first = cases, cap, len(cases), 1
        nf = self.nf
        self.kps = np.zeros((nf + 1, cap), pc.KP_DTYPE); self.kps["octave"] = 3; self.kps["x"] = 11.0
        self.counts = np.zeros(nf + 1, np.int32); self.counts[0] = cap
        self.uright = np.full((nf, cap), -1.0, np.float32)
        self.q_mp = np.full((nf, cap), -1, np.int32)
        self.tcw = np.zeros((nf, 12), np.float32)
        pools, base = [], 0
        for f, c in enumerate(cases):
            n = len(c["q_mp"])
            assert n <= cap
            self.kps[1 + f, :n] = c["kps"]; self.counts[1 + f] = n
            if c["uright"] is not None:
                self.uright[f, :n] = c["uright"]
            self.q_mp[f, :n] = np.where(c["q_mp"] >= 0, c["q_mp"] + base, -1)
            if garbage:                                                      # slots past the count hold live-looking rows that must not be read as edges
                self.q_mp[f, n:] = base
                self.kps[1 + f, n:] = self.kps[1 + f, 0]
            self.tcw[f] = c["tcw_in"].reshape(12)
            pools.append(c["mp_pw"]); base += len(c["mp_pw"])
        self.mp_pw = np.concatenate(pools).astype(np.float32)
        self.nmp = len(self.mp_pw)
        if garbage:
            null = self.q_mp < 0
            self.q_mp[null] = np.where(np.arange(null.sum()) % 2 == 0, self.nmp + 5, -7)   # NULL as any index outside [0, nmp)
        self.K, self.bf, self.ils2 = cases[0]["K"], float(cases[0]["bf"]), cases[0]["ils2"]

    def host(self, m):
        return m.PoseOptimization(self.kps, self.counts, self.uright, self.q_mp, self.mp_pw, self.tcw, self.K, self.bf, self.ils2, first=self.first,
                                  outlier_fill=POISON)

    def device(self, pkg, m, alias=False):
        d = DeviceBatch(pkg, self)
        d.enqueue(m, alias=alias); m.sync()
        return d.fetch(alias=alias)

    def flags(self, out, f):
        """outlier row f as the header program prints it: -1 where nothing was written."""
        n = len(self.cases[f]["q_mp"])
        row = out["outlier"][f].astype(np.int16)
        assert np.all(row[n:] == POISON), "a slot at or beyond the count was written"
        return np.where(row[:n] == POISON, -1, row[:n]).astype(np.int8)


class DeviceBatch:
    def __init__(self, pkg, b):
        self.b, self.pkg = b, pkg
        self.kps, self.counts, self.uright, self.q_mp = _up(pkg, b.kps), _up(pkg, b.counts), _up(pkg, b.uright), _up(pkg, b.q_mp)
        self.mp_pw, self.tcw_in = _up(pkg, b.mp_pw), _up(pkg, b.tcw)
        self.tcw_out = _up(pkg, np.full((b.nf, 12), np.nan, np.float32))
        self.outlier = _up(pkg, np.full((b.nf, b.cap), POISON, np.uint8))
        self.n_corr, self.n_good = _up(pkg, np.full(b.nf, -9, np.int32)), _up(pkg, np.full(b.nf, -9, np.int32))

    def enqueue(self, m, alias=False):
        b = self.b
        m.PoseOptimizationBatchAsync(b.nf, b.first, b.cap, self.kps.ptr, self.counts.ptr, self.uright.ptr, self.q_mp.ptr, b.nmp, self.mp_pw.ptr,
                                     self.tcw_in.ptr, b.K, b.bf, b.ils2, self.tcw_in.ptr if alias else self.tcw_out.ptr, self.outlier.ptr,
                                     self.n_corr.ptr, self.n_good.ptr)

    def fetch(self, alias=False):
        b = self.b
        return {"tcw": (self.tcw_in if alias else self.tcw_out).download(np.float32, b.nf * 12).reshape(b.nf, 3, 4),
                "outlier": self.outlier.download(np.uint8, b.nf * b.cap).reshape(b.nf, b.cap),
                "n_corr": self.n_corr.download(np.int32, b.nf), "n_good": self.n_good.download(np.int32, b.nf)}


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("tcw", "outlier", "n_corr", "n_good"))


@pytest.mark.parametrize("names", BATCHES, ids=lambda n: "+".join(n))
def test_device_host_header_and_reading(pkg, m, header_exe, tmp_path, names):
    cases = res.cases()
    b = Batch([cases[n] for n in names], pc.CAP, garbage=True)
    dev, host = b.device(pkg, m), b.host(m)
    assert _same(dev, host), "the device form and the host form differ"
    assert _same(dev, b.device(pkg, m)), "two runs differ"
    path = str(tmp_path / "cases.txt")
    io.write_cases(path, {n: cases[n] for n in names})
    hdr = io.run_program(header_exe, path)
    for f, n in enumerate(names):
        h = hdr[n]
        assert dev["tcw"][f].tobytes() == h["tcw"].tobytes(), "%s: the pose differs from the g++ build of the header by %g" % (
            n, float(np.max(np.abs(dev["tcw"][f].astype(np.float64) - h["tcw"]))))
        assert np.array_equal(b.flags(dev, f), h["outlier"]) and (dev["n_corr"][f], dev["n_good"][f]) == (h["n_corr"], h["n_good"]), n
        res.check_against_reading(n, None, dev["tcw"][f], b.flags(dev, f), int(dev["n_corr"][f]), int(dev["n_good"][f]), "device")


def _big_case(n_slots, n_corr):
    return pc.scene(900 + n_slots, n_slots, n_corr, stereo_share=0.4)


@pytest.mark.parametrize("cap", [LDS_CAP, LDS_CAP + 1])
def test_at_and_past_the_lds_capacity(pkg, m, header_exe, tmp_path, cap):
    """cap 1536 is the last the kernel stages in LDS, 1537 gathers from the rows in every pass: same scene, same bits, and the header's."""
    c = _big_case(LDS_CAP, 1400)
    b = Batch([c], cap)
    dev = b.device(pkg, m)
    assert _same(dev, b.host(m))
    path = str(tmp_path / "big.txt")
    io.write_cases(path, {"big": c})
    h = io.run_program(header_exe, path)["big"]
    assert dev["tcw"][0].tobytes() == h["tcw"].tobytes() and np.array_equal(b.flags(dev, 0), h["outlier"])
    assert (dev["n_corr"][0], dev["n_good"][0]) == (h["n_corr"], h["n_good"]) == (1400, h["n_good"]) and 1000 < h["n_good"] < 1400


def test_uright_null_makes_every_edge_mono(pkg, m):
    cases = res.cases()
    b = Batch([cases["all_mono"], cases["ncorr_65"]], pc.CAP)
    b.uright[:] = -1.0
    with_row = b.host(m)
    b.uright = None
    assert _same(with_row, b.host(m))


def test_alias_replay_and_garbage_octaves(pkg, m):
    cases = res.cases()
    b = Batch([cases["mixed"], cases["ncorr_9"], cases["ncorr_257"]], pc.CAP, garbage=True)
    want = b.device(pkg, m)
    assert _same(want, b.device(pkg, m, alias=True)), "tcw_out aliasing tcw_in changes the result"
    # an octave outside [0, nlevels) makes the slot NULL: not counted, not written
    s = np.nonzero(cases["mixed"]["q_mp"] >= 0)[0][:3]
    b.kps["octave"][1, s[0]] = pc.NLEVELS; b.kps["octave"][1, s[1]] = -1; b.kps["octave"][1, s[2]] = 1 << 30
    got = b.device(pkg, m)
    assert got["n_corr"][0] == want["n_corr"][0] - 3 and np.all(got["outlier"][0, s] == POISON)
    assert got["tcw"][1].tobytes() == want["tcw"][1].tobytes() and got["tcw"][2].tobytes() == want["tcw"][2].tobytes()


def test_refused_arguments_enqueue_nothing(pkg, m):
    L = pkg.lib()
    b = Batch([res.cases()["ncorr_10"]], 64)
    d = DeviceBatch(pkg, b)
    k, ils = np.ascontiguousarray(b.K, np.float32), np.ascontiguousarray(b.ils2, np.float32)
    kp, ip = k.ctypes.data_as(C.c_void_p), ils.ctypes.data_as(C.c_void_p)
    good = [b.nf, b.first, b.cap, d.kps.ptr, d.counts.ptr, d.uright.ptr, d.q_mp.ptr, b.nmp, d.mp_pw.ptr, d.tcw_in.ptr, kp, b.bf, ip, len(ils),
            d.tcw_out.ptr, d.outlier.ptr, d.n_corr.ptr, d.n_good.ptr]

    def call(**kw):
        a = list(good)
        for name, v in kw.items():
            a[POSE.index(name)] = v
        return L.orbm_pose_optimization_batch_async(m.h, *a)

    POSE = ["nframes", "first", "cap", "kps_un", "counts", "uright", "q_mp", "nmp", "mp_pw", "tcw_in", "k_host", "bf", "inv_level_sigma2_host", "nlevels",
            "tcw_out", "outlier", "n_corr", "n_good"]
    for name in ("kps_un", "counts", "q_mp", "mp_pw", "tcw_in", "k_host", "inv_level_sigma2_host", "tcw_out", "outlier", "n_corr", "n_good"):
        assert call(**{name: None}) == E_INVALID and name.encode() in L.orbm_last_error()
    for kw in (dict(nframes=0), dict(cap=0), dict(nmp=0), dict(nlevels=0), dict(first=-1), dict(bf=float("nan"))):
        assert call(**kw) == E_INVALID, kw
    for kw in (dict(nframes=65536), dict(cap=65536), dict(nlevels=33), dict(first=1 << 30, cap=64)):
        assert call(**kw) == E_CAPACITY, kw
    bad = [b.nf, b.cap, d.counts.ptr, d.q_mp.ptr, d.outlier.ptr, b.nmp, d.n_corr.ptr, None, 1, 1, None, None, None]
    for i, want in ((2, E_INVALID), (3, E_INVALID), (4, E_INVALID), (6, E_INVALID)):
        a = list(bad); a[i] = None
        assert L.orbm_discard_outliers_batch_async(m.h, *a) == want
    for i, v, want in ((0, 0, E_INVALID), (1, 0, E_INVALID), (5, 0, E_INVALID), (0, 65536, E_CAPACITY), (1, 65536, E_CAPACITY)):
        a = list(bad); a[i] = v
        assert L.orbm_discard_outliers_batch_async(m.h, *a) == want
    m.sync()
    out = d.fetch()
    assert np.all(out["outlier"] == POISON) and np.all(out["n_corr"] == -9) and np.all(np.isnan(out["tcw"]))


# ---- the discard kernel ----------------------------------------------------------------------------------------------------------
def discard_contract(counts, q_mp, outlier, nmp, mp_nobs, mp_valid, discard, clear_bad):
    q, o = q_mp.copy(), outlier.copy()
    nf, cap = q.shape
    seen = np.zeros((nf, nmp), np.uint8); nmm = np.zeros(nf, np.int32); nd = np.zeros(nf, np.int32)
    for f in range(nf):
        for i in range(min(max(int(counts[f]), 0), cap)):
            j = q_mp[f, i]
            if not 0 <= j < nmp:
                continue
            if discard and outlier[f, i]:
                q[f, i] = -1; o[f, i] = 0; seen[f, j] = 1; nd[f] += 1
                continue
            if not outlier[f, i] and mp_nobs[j] > 0:
                nmm[f] += 1
            if clear_bad and mp_valid is not None and not mp_valid[j]:
                q[f, i] = -1
            else:
                seen[f, j] = 1
    return q, o, seen, nmm, nd


@pytest.mark.parametrize("discard,clear_bad,valid_null", [(1, 0, False), (0, 1, False), (1, 1, False), (0, 0, False), (1, 1, True)])
def test_discard_outliers_equals_numpy(pkg, m, discard, clear_bad, valid_null):
    rs = np.random.RandomState(31 + 2 * discard + clear_bad)
    nf, cap, nmp = 3, 600, 333
    counts = np.array([600, 257, -4], np.int32)
    q_mp = rs.randint(-40, nmp + 40, (nf, cap)).astype(np.int32)
    q_mp[0, 10] = q_mp[0, 11] = q_mp[0, 300] = 17                            # one MapPoint in three slots ...
    outlier = (rs.rand(nf, cap) < 0.3).astype(np.uint8) * rs.choice([1, 7], (nf, cap)).astype(np.uint8)
    outlier[0, 10], outlier[0, 11], outlier[0, 300] = 1, 0, 1               # ... discarded in two of them, kept in one
    mp_nobs = rs.randint(-1, 3, nmp).astype(np.int32)
    mp_valid = None if valid_null else (rs.rand(nmp) < 0.7).astype(np.uint8)
    dq, do, dc, dn = _up(pkg, q_mp), _up(pkg, outlier), _up(pkg, counts), _up(pkg, mp_nobs)
    dv = None if valid_null else _up(pkg, mp_valid)
    ds = _up(pkg, np.full((nf, nmp), POISON, np.uint8)); dm = _up(pkg, np.full(nf, -9, np.int32)); dd = _up(pkg, np.full(nf, -9, np.int32))
    m.DiscardOutliersBatchAsync(nf, cap, dc.ptr, dq.ptr, do.ptr, nmp, dn.ptr, None if dv is None else dv.ptr, discard, clear_bad, ds.ptr, dm.ptr, dd.ptr)
    m.sync()
    q, o, seen, nmm, nd = discard_contract(counts, q_mp, outlier, nmp, mp_nobs, mp_valid, discard, clear_bad)
    assert np.array_equal(dq.download(np.int32, nf * cap).reshape(nf, cap), q)
    assert np.array_equal(do.download(np.uint8, nf * cap).reshape(nf, cap), o)
    assert np.array_equal(ds.download(np.uint8, nf * nmp).reshape(nf, nmp), seen)
    assert np.array_equal(dm.download(np.int32, nf), nmm) and np.array_equal(dd.download(np.int32, nf), nd)
    assert nd[2] == 0 and (nd[0] > 50) == bool(discard)
    # the optional rows may be absent
    dq2, do2 = _up(pkg, q_mp), _up(pkg, outlier)
    m.DiscardOutliersBatchAsync(nf, cap, dc.ptr, dq2.ptr, do2.ptr, nmp, dn.ptr, None if dv is None else dv.ptr, discard, clear_bad, None, None, None)
    m.sync()
    assert np.array_equal(dq2.download(np.int32, nf * cap).reshape(nf, cap), q)


# ---- the chain in a captured graph ------------------------------------------------------------------------------------------------
def test_captured_chain_follows_rewritten_rows(pkg, synth):
    """{pose optimisation, discard, votes} captured once; tcw_in and q_mp are rewritten and the graph replayed: every output equals a
    fresh eager run of the same three calls into other buffers, and the first state again gives the first bits."""
    L = pkg.lib()
    W, H = 320, 240                                                          # a capture is opened on an extractor and holds one extraction
    dimg = pkg.DeviceBuffer(W * H).upload(synth.gen_image(W, H, 7400))
    arr = (C.c_void_p * 1)(dimg.ptr)
    lap = np.array([(0, 500)], np.int32)
    ex = pkg.ORBextractor(500, max_size=(W, H), max_batch=1)
    mt = pkg.ORBmatcher(0.9)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    ex.enqueue_device(arr, W, H, W, lap); ex.sync()
    cases = res.cases()
    names = [["mixed", "ncorr_65", "ncorr_9"], ["all_stereo", "ncorr_257", "ncorr_2"], ["readmit", "ncorr_64", "ncorr_513"]]
    states = [Batch([cases[n] for n in ns], pc.CAP) for ns in names]
    nmp = max(s.nmp for s in states)
    rs = np.random.RandomState(5)
    pool = np.zeros((nmp, 3), np.float32)
    nf, cap = 3, pc.CAP
    # one pool for every state: each state's points sit at its own indices, so q_mp and the pool rows are rewritten together
    nrows = 7
    off = np.concatenate([[0], np.cumsum(rs.randint(0, 6, nmp))]).astype(np.int32)
    orow = rs.randint(0, nrows, off[-1]).astype(np.int32); oslot = rs.randint(0, 100, off[-1]).astype(np.int32); ofl = np.zeros(off[-1], np.uint8)
    kcounts = np.full(nrows, 100, np.int32)
    mp_nobs = rs.randint(0, 3, nmp).astype(np.int32)
    doff, drow, dslot, dfl, dkc, dnobs = (_up(pkg, a) for a in (off, orow, oslot, ofl, kcounts, mp_nobs))
    dkps, dcounts, dur = _up(pkg, states[0].kps), _up(pkg, states[0].counts), _up(pkg, states[0].uright)
    dq_src, dtcw, dpw = _up(pkg, states[0].q_mp), _up(pkg, states[0].tcw), _up(pkg, pool)
    b0 = states[0]

    class Out:
        def __init__(self):
            self.q_mp = _up(pkg, np.zeros((nf, cap), np.int32))
            self.tcw_out, self.outlier = _up(pkg, np.zeros((nf, 12), np.float32)), _up(pkg, np.full((nf, cap), POISON, np.uint8))
            self.cnt = _up(pkg, np.zeros(4 * nf, np.int32))
            self.seen = _up(pkg, np.zeros((nf, nmp), np.uint8))
            self.votes = _up(pkg, np.zeros((nf, nrows), np.int32)); self.vc = _up(pkg, np.zeros(3 * nf, np.int32))

        def enqueue(self):
            # the discard writes the match rows in place and the votes read what it left
            mt.PoseOptimizationBatchAsync(nf, 1, cap, dkps.ptr, dcounts.ptr, dur.ptr, dq_src.ptr, nmp, dpw.ptr, dtcw.ptr, b0.K, b0.bf, b0.ils2,
                                          self.tcw_out.ptr, self.outlier.ptr, self.cnt.ptr, self.cnt.ptr + 4 * nf)
            mt.DiscardOutliersBatchAsync(nf, cap, dcounts.ptr + 4, dq_src.ptr, self.outlier.ptr, nmp, dnobs.ptr, None, 1, 0, self.seen.ptr,
                                         self.cnt.ptr + 8 * nf, self.cnt.ptr + 12 * nf)
            mt.CovisibilityVotesBatchAsync(nf, cap, dq_src.ptr, dcounts.ptr + 4, None, nrows, 100, dkc.ptr, None, 0, nmp, int(off[-1]), doff.ptr, drow.ptr,
                                           dslot.ptr, dfl.ptr, None, 15, 0, self.votes.ptr, self.vc.ptr, self.vc.ptr + 4 * nf, self.vc.ptr + 8 * nf)

        def fetch(self):
            return {"tcw": self.tcw_out.download(np.float32, nf * 12), "outlier": self.outlier.download(np.uint8, nf * cap),
                    "cnt": self.cnt.download(np.int32, 4 * nf), "seen": self.seen.download(np.uint8, nf * nmp),
                    "votes": self.votes.download(np.int32, nf * nrows), "q_mp": dq_src.download(np.int32, nf * cap)}

    def upload(s):
        p = pool.copy(); p[:s.nmp] = s.mp_pw
        dkps.upload(s.kps); dcounts.upload(s.counts); dur.upload(s.uright); dq_src.upload(s.q_mp); dtcw.upload(s.tcw); dpw.upload(p)
        for o in (A, B):                                                     # a slot without a MapPoint keeps the caller's byte: start every run alike
            o.outlier.upload(np.full((nf, cap), POISON, np.uint8))

    A, B = Out(), Out()
    want = []
    for s in states:                                                         # the eager runs, ahead of the capture
        upload(s)
        B.enqueue(); mt.sync()
        want.append(B.fetch())
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    ex.enqueue_device(arr, W, H, W, lap)
    A.enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    for i in (0, 1, 2, 0):
        upload(states[i])
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        got = A.fetch()
        for kk, w in want[i].items():
            assert got[kk].tobytes() == w.tobytes(), (i, kk)
    c0 = want[0]["cnt"]
    assert c0[nf] > 100 and c0[3 * nf] > 10 and want[0]["votes"].sum() > 50 and want[0]["tcw"].tobytes() != want[1]["tcw"].tobytes()
    # the discard took the flagged slots out of the rows the votes then read, and cleared their flags
    gone = (states[0].q_mp >= 0) & (want[0]["q_mp"].reshape(nf, cap) == -1)
    assert np.array_equal(gone.sum(axis=1), c0[3 * nf:]) and np.array_equal(c0[:nf] - c0[nf:2 * nf], c0[3 * nf:])
    assert not np.any(want[0]["outlier"] == 1)
    mt.close()


def test_cpp_facade_pose_optimization(pkg, tmp_path):
    """facade/PoseOptimization.h on mock Frame / MapPoint types: the flattened call gives the bits of the array form."""
    pkg.build()
    exe = str(tmp_path / "facade_poseopt_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "facade_poseopt_smoke.cpp"),
                           "-L", os.path.join(ROOT, "orb-slam3_amd"), "-lorbslam3_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "orb-slam3_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "need-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "facade_poseopt_smoke ok" in out.stdout, out.stdout + out.stderr
