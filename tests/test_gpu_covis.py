"""orbm_covisibility_votes, orbm_local_points, orbm_gather_map_points_batch_async on the GPU: host form == device form == the numpy
contract == the sequential reading of the reference (tests/second_reading_covis.py) on the constructed maps of tests/covis_cases.py, on
seeded random maps and on array-level data whose shapes sit on every boundary of the kernels: entry lists of 0 .. 200 entries, pairs that
straddle a round, rows that alias in the workgroup's LDS table and more rows than it holds, position spaces of one chunk, one chunk plus
one and three chunks; garbage indices; refused arguments; a captured graph {votes, local points, gather, isInFrustum, M3} replayed after
its rows were rewritten; the facade on mock types."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covis_cases as cc
import second_reading_covis as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xCD
PI32 = int(np.frombuffer(bytes([POISON] * 4), np.int32)[0])
TBL, WG_SLOTS, CHUNK = 256, 64, 1024                                        # csrc: COVIS_TBL, COVIS_WG_SLOTS, LP_CHUNK
VOTE_KEYS = ("votes", "n_voted", "max_votes", "n_over", "list_row", "list_votes")


@pytest.fixture(scope="module")
def m(pkg):
    return pkg.ORBmatcher(0.9)


def _up(pkg, a, t=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, t)
    return pkg.DeviceBuffer(max(a.nbytes, 4)).upload(a) if a.nbytes else pkg.DeviceBuffer(4)


def _poisoned(pkg, nbytes):
    return pkg.DeviceBuffer(nbytes + 4).upload(np.full(nbytes + 4, POISON, np.uint8))


def _ptr(b):
    return None if b is None else b.ptr


# ---- votes -----------------------------------------------------------------------------------------------------------------------
class VotesDev:
    def __init__(self, pkg, q_mp, q_n, self_row, counts_kf, cap, kf_skip, skip_bad, obs_off, obs_row, obs_slot, obs_flags, mp_valid, th, list_cap):
        self.pkg = pkg
        q_mp = np.ascontiguousarray(q_mp, np.int32)
        self.nq, self.qs = q_mp.shape
        self.nrows, self.cap, self.nmp, self.nobs = len(counts_kf), int(cap), len(obs_off) - 1, len(obs_row)
        self.skip_bad, self.th, self.list_cap = int(skip_bad), int(th), int(list_cap)
        self.q_mp, self.q_n, self.self_row = _up(pkg, q_mp), _up(pkg, q_n, np.int32), _up(pkg, self_row, np.int32)
        self.counts, self.kf_skip = _up(pkg, counts_kf, np.int32), _up(pkg, kf_skip, np.uint8)
        self.off, self.row, self.slot, self.flags = _up(pkg, obs_off, np.int32), _up(pkg, obs_row, np.int32), _up(pkg, obs_slot, np.int32), _up(pkg, obs_flags, np.uint8)
        self.valid = _up(pkg, mp_valid, np.uint8)
        self.sizes = dict(votes=self.nq * self.nrows * 4, n_voted=self.nq * 4, max_votes=self.nq * 4, n_over=self.nq * 4,
                          list_row=self.nq * self.list_cap * 4, list_votes=self.nq * self.list_cap * 4)
        self.reset()

    def reset(self):
        self.out = {k: _poisoned(self.pkg, n) for k, n in self.sizes.items()}

    def enqueue(self, m, **kw):
        a = dict(h=m.h, nq=self.nq, qs=self.qs, q_mp=_ptr(self.q_mp), q_n=_ptr(self.q_n), self_row=_ptr(self.self_row), nrows=self.nrows, cap=self.cap,
                 counts=_ptr(self.counts), kf_skip=_ptr(self.kf_skip), skip_bad=self.skip_bad, nmp=self.nmp, nobs=self.nobs, off=_ptr(self.off),
                 row=_ptr(self.row), slot=_ptr(self.slot), flags=_ptr(self.flags), valid=_ptr(self.valid), th=self.th, list_cap=self.list_cap,
                 list_row=self.out["list_row"].ptr if self.list_cap else None, list_votes=self.out["list_votes"].ptr if self.list_cap else None,
                 **{k: self.out[k].ptr for k in VOTE_KEYS[:4]})
        a.update(kw)
        return m.L.orbm_covisibility_votes_batch_async(a["h"], a["nq"], a["qs"], a["q_mp"], a["q_n"], a["self_row"], a["nrows"], a["cap"], a["counts"],
                                                       a["kf_skip"], a["skip_bad"], a["nmp"], a["nobs"], a["off"], a["row"], a["slot"], a["flags"], a["valid"],
                                                       a["th"], a["list_cap"], a["votes"], a["n_voted"], a["max_votes"], a["n_over"], a["list_row"],
                                                       a["list_votes"])

    def fetch(self):
        """Downloads; the four bytes behind every output still hold the poison.  List entries that were not written read PI32."""
        got = {}
        for k, n in self.sizes.items():
            assert np.all(self.out[k].download(np.uint8, 4, offset=n) == POISON), k
            got[k] = self.out[k].download(np.int32, n // 4) if n else np.zeros(0, np.int32)
        got["votes"] = got["votes"].reshape(self.nq, self.nrows)
        for k in ("list_row", "list_votes"):
            got[k] = got[k].reshape(self.nq, self.list_cap) if self.list_cap else None
        return got

    def untouched(self):
        return all(np.all(self.out[k].download(np.uint8, n + 4) == POISON) for k, n in self.sizes.items())


def _same_votes(got, want):
    for k in VOTE_KEYS:
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert np.array_equal(got[k], want[k]), (k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:8])


def _three_ways(pkg, m, args):
    """args = the contract's argument list; host form == device form == contract.  Returns the contract's result."""
    want = sr.votes_contract(*args, list_fill=PI32)
    d = VotesDev(pkg, *args)
    assert d.enqueue(m) == 0, m.L.orbm_last_error()
    m.sync()
    _same_votes(d.fetch(), want)
    q_mp, q_n, self_row, counts, cap, kf_skip, skip_bad, off, row, slot, fl, valid, th, list_cap = args
    host = m.CovisibilityVotes(q_mp, q_n, self_row, counts, cap, kf_skip, skip_bad, off, row, slot, fl, valid, th, list_cap, list_fill=PI32)
    _same_votes(host, want)
    return want


@pytest.mark.parametrize("name", sorted(cc.VOTE_CASES))
def test_vote_cases(pkg, m, name):
    kfs, who, want = cc.VOTE_CASES[name]()
    if isinstance(who, sr.Frame):
        F = sr.flatten_votes([who.mvpMapPoints], None, None); seq = sr.LocalKeyFrameVotes(who); skip_bad = 0
    else:
        F = sr.flatten_votes([kfs[who].GetMapPointMatches()], [kfs[who]], kfs[who].map); seq = sr.ConnectionCounts(kfs[who]); skip_bad = 1
    con = _three_ways(pkg, m, sr.vote_args(F, skip_bad, 15, 3))
    assert sr.counter_of(F, con["votes"][0]) == seq and {kfs.index(k): v for k, v in seq.items()} == want


def test_twenty_random_maps(pkg, m):
    """One batch call per map for every KeyFrame of it (a whole LoopClosing loop), and the frame's vote: == the sequential reading."""
    voted = 0
    for seed in range(20):
        kfs, frame, _ = cc.random_map(seed)
        queries = [kf for kf in kfs if not kf.isBad() and kf.map is kfs[0].map]
        if queries:
            F = sr.flatten_votes([kf.GetMapPointMatches() for kf in queries], queries, kfs[0].map)
            con = _three_ways(pkg, m, sr.vote_args(F, 1, 3, 5))
            for q, kf in enumerate(queries):
                seq = sr.ConnectionCounts(kf)
                assert sr.counter_of(F, con["votes"][q]) == seq, (seed, q)
                voted += len(seq)
        Ff = sr.flatten_votes([frame.mvpMapPoints], None, None)
        con = _three_ways(pkg, m, sr.vote_args(Ff, 0, 15, 0))
        assert sr.counter_of(Ff, con["votes"][0]) == sr.LocalKeyFrameVotes(frame), seed
    assert voted > 50


NROWS, NMP, QS = 600, 140, 150                                              # more rows than the LDS table; three workgroups of slots, the last partly dead
LENGTHS = (0, 1, 16, 17, 64, 65, 200)
MP_PAIR16, MP_PAIR64, MP_ALIAS = 0, 1, 2                                    # the first three MapPoints are constructed


def synthetic_votes(seed, nq, cap, garbage=False):
    rng = np.random.RandomState(seed)
    counts = rng.randint(cap // 2, cap + 1, NROWS).astype(np.int32)
    counts[0] = cap + 9                                                     # a count above cap is clamped
    lens = np.concatenate([[20, 70, 2], np.repeat(LENGTHS, 8), rng.choice(LENGTHS[:4] + (5, 9, 12), NMP - 3 - 8 * len(LENGTHS))])
    off, row, slot, flags = [0], [], [], []
    for j, n in enumerate(lens):
        e = 0
        while e < n:
            r = int(rng.randint(NROWS)); f = int(rng.choice([0, 0, 0, 4, 2, 6]))
            row.append(r); slot.append(int(rng.randint(min(counts[r], cap)))); flags.append(f); e += 1
            if e < n and rng.rand() < 0.25:                                 # the right entry of the same KeyFrame
                row.append(r); slot.append(int(rng.randint(min(counts[r], cap)))); flags.append((f & 2) | 1); e += 1
        off.append(len(row))
    row, slot, flags = np.array(row, np.int32), np.array(slot, np.int32), np.array(flags, np.uint8)
    for j, left in ((MP_PAIR16, 15), (MP_PAIR64, 63)):                      # a pair that straddles a round of 16 (the group) and of 64 (the wave)
        a = off[j] + left
        row[a - 1:a + 3] = [590 + j, 5 + j, 5 + j, 592 + j]; slot[a - 1:a + 3] = 0; flags[a - 1:a + 3] = [0, 0, 1, 0]
    a = off[MP_ALIAS]
    row[a:a + 2] = [7, 7 + TBL]; slot[a:a + 2] = 0; flags[a:a + 2] = 0      # two rows that share an entry of the LDS table
    q_mp = rng.randint(-1, NMP, (nq, QS)).astype(np.int32)
    q_mp[:, :3] = [MP_PAIR16, MP_PAIR64, MP_ALIAS]
    q_mp[:, 3:11] = np.flatnonzero(lens == 200)[:8]                         # 1600 entries over 600 rows in the first workgroup: more rows than the table holds
    q_n = rng.randint(QS // 2, QS + 1, nq).astype(np.int32)
    q_n[0] = QS
    if nq >= 3:
        q_n[1], q_n[2] = QS + 40, -3
    self_row = rng.randint(-1, NROWS, nq).astype(np.int32)
    self_row[0] = -1
    kf_skip = (rng.rand(NROWS) < 0.1).astype(np.uint8)
    kf_skip[[5, 6, 7, 7 + TBL]] = 0; kf_skip[590:594] = 0
    mp_valid = (rng.rand(NMP) < 0.9).astype(np.uint8)
    mp_valid[:11] = 1; mp_valid[np.flatnonzero(lens == 200)[:8]] = 1
    off = np.array(off, np.int32)
    if garbage:
        g = rng.rand(len(row))
        row[g < 0.03] = rng.choice([-1, NROWS, 1 << 30, -(1 << 31)], (g < 0.03).sum())
        slot[(g > 0.03) & (g < 0.06)] = rng.choice([-1, cap, cap + 9, 1 << 30, -(1 << 31)], ((g > 0.03) & (g < 0.06)).sum())
        off[25] = off[24]; off[29] = -3; off[40] = len(row) + 7; off[51] = off[50] - 2      # malformed pairs around them: empty lists
        q_mp[rng.rand(nq, QS) < 0.05] = NMP; q_mp[rng.rand(nq, QS) < 0.05] = -(1 << 31); q_mp[0, 11] = (1 << 31) - 1
        self_row[-1] = 1 << 30
    return [q_mp, q_n, self_row, counts, cap, kf_skip, 1, off, row, slot, flags, mp_valid, 15, 40]


@pytest.mark.parametrize("garbage", [False, True], ids=["clean", "garbage"])
@pytest.mark.parametrize("cap", [16, 40])
@pytest.mark.parametrize("nq", [1, 3, 9])
def test_lists_of_every_length(pkg, m, nq, cap, garbage):
    args = synthetic_votes(10 * nq + cap, nq, cap, garbage)
    want = _three_ways(pkg, m, args)
    if not garbage:
        v = want["votes"][0]
        assert v[5] >= 1 and v[6] >= 1 and v[7] >= 1 and v[7 + TBL] >= 1
        assert want["n_voted"][0] > TBL and want["n_voted"][0] > 40          # the list is cut at list_cap
        alone = sr.votes_contract(*(args[:1] + [np.array([1] + [0] * (nq - 1), np.int32)] + [None] + args[3:]))["votes"][0]
        assert alone[5] == 1 and alone[590] == 1 and alone[592] == 1        # slot 0 alone: the pair at entries 15 / 16 votes once
    for variant in (dict(skip_bad=0), dict(list_cap=0), dict(self_row=None, kf_skip=None, mp_valid=None, th=1, list_cap=NROWS)):
        a = list(args)
        for k, v in variant.items():
            a[("q_mp", "q_n", "self_row", "counts_kf", "cap", "kf_skip", "skip_bad", "obs_off", "obs_row", "obs_slot", "obs_flags", "mp_valid", "th",
               "list_cap").index(k)] = v
        _three_ways(pkg, m, a)
    assert m.L.orbm_sync(m.h) == 0


def test_pair_at_the_wave_round_boundary(pkg, m):
    """MapPoint MP_PAIR64 alone: left at entry 63, right at entry 64 of a list of 70, taken by the whole wave: one vote for row 6."""
    args = synthetic_votes(3, 1, 16)
    args[0] = np.full((1, QS), MP_PAIR64, np.int32); args[1] = np.array([1], np.int32); args[2] = None; args[5] = None
    want = _three_ways(pkg, m, args)
    assert want["votes"][0][6] == 1 and want["votes"][0][591] >= 1 and want["votes"][0][593] >= 1


def test_refused_vote_arguments_enqueue_nothing(pkg, m):
    d = VotesDev(pkg, *synthetic_votes(4, 3, 16))
    for kw in (dict(q_mp=None), dict(q_n=None), dict(counts=None), dict(off=None), dict(row=None), dict(slot=None), dict(flags=None), dict(votes=None),
               dict(n_voted=None), dict(max_votes=None), dict(n_over=None), dict(list_row=None), dict(list_votes=None), dict(nq=0), dict(qs=0), dict(nrows=0),
               dict(cap=0), dict(nmp=0), dict(nobs=-1), dict(list_cap=-1), dict(h=None)):
        assert d.enqueue(m, **kw) == -2, kw
    for kw in (dict(nq=65536), dict(qs=65536), dict(nrows=(1 << 20) + 1), dict(nmp=(1 << 20) + 1), dict(nq=1 << 9, nrows=(1 << 19) + 1),
               dict(nrows=1 << 16, cap=1 << 15)):
        assert d.enqueue(m, **kw) == -3, kw
    m.sync()
    assert d.untouched()


# ---- local points ---------------------------------------------------------------------------------------------------------------------
def _local_dev(pkg, m, lkf_row, n_lkf, counts, kf_mp, nmp, valid, qs):
    T, ls = lkf_row.shape
    nrows, cap = kf_mp.shape
    bufs = [_up(pkg, lkf_row, np.int32), _up(pkg, n_lkf, np.int32), _up(pkg, counts, np.int32), _up(pkg, kf_mp, np.int32), _up(pkg, valid, np.uint8)]
    out, nt, nq = _poisoned(pkg, T * qs * 4), _poisoned(pkg, T * 4), _poisoned(pkg, T * 4)
    rc = m.L.orbm_local_points_batch_async(m.h, T, ls, bufs[0].ptr, bufs[1].ptr, nrows, cap, bufs[2].ptr, bufs[3].ptr, nmp, _ptr(bufs[4]), qs, out.ptr, nt.ptr,
                                           nq.ptr)
    assert rc == 0, m.L.orbm_last_error()
    m.sync()
    for b, n in ((out, T * qs * 4), (nt, T * 4), (nq, T * 4)):
        assert np.all(b.download(np.uint8, 4, offset=n) == POISON)
    return out.download(np.int32, T * qs).reshape(T, qs), nt.download(np.int32, T), nq.download(np.int32, T)


def _local_three_ways(pkg, m, lkf_row, n_lkf, counts, kf_mp, nmp, valid, qs):
    want = sr.local_points_contract(lkf_row, n_lkf, counts, kf_mp, nmp, valid, qs, fill=PI32)
    for got in (_local_dev(pkg, m, lkf_row, n_lkf, counts, kf_mp, nmp, valid, qs), m.LocalPoints(lkf_row, n_lkf, counts, kf_mp, nmp, valid, qs, fill=PI32)):
        for g, w, what in zip(got, want, ("local_mp", "n_total", "nq")):
            assert np.array_equal(g, w), (what, g, w)                        # local_mp as an ordered list, the tail untouched
    return want


@pytest.mark.parametrize("ls,cap", [(8, 128), (5, 205), (8, 384)], ids=["one-chunk", "one-chunk-plus-one", "three-chunks"])
@pytest.mark.parametrize("T", [1, 3])
def test_local_points_shapes(pkg, m, T, ls, cap):
    assert ls * cap in (CHUNK, CHUNK + 1, 3 * CHUNK)
    rng = np.random.RandomState(ls * cap + T)
    nrows, nmp = 12, 900
    counts = rng.randint(cap // 2, cap + 1, nrows).astype(np.int32)
    counts[3] = cap + 5; counts[4] = cap
    kf_mp = rng.randint(-1, nmp - 2, (nrows, cap)).astype(np.int32)
    kf_mp[rng.rand(nrows, cap) < 0.02] = nmp + 3                              # out of range: NULL
    n_lkf = np.array([5, 0, 1][:T] if T == 3 else [5], np.int32)
    lkf_row = np.stack([rng.permutation(nrows)[:ls] for _ in range(T)]).astype(np.int32)
    lkf_row[0, :5] = [3, nrows, 3, -1, 4]                                     # a row twice, two rows out of range, the last walked row full
    J, U = nmp - 2, nmp - 1
    kf_mp[3, 2] = J; kf_mp[4, cap - 2] = J                                    # two occurrences in the first and in the last chunk
    kf_mp[4, cap - 1] = U                                                     # a first occurrence in the last position of all
    if ls * cap == CHUNK + 1:
        n_lkf[0] = 5
    valid = (rng.rand(nmp) < 0.9).astype(np.uint8); valid[[J, U]] = 1
    if ls == 5:
        assert (4 * cap + cap - 1) == ls * cap - 1                            # U sits at key 1024: alone in the second chunk
    want = _local_three_ways(pkg, m, lkf_row, n_lkf, counts, kf_mp, nmp, valid, ls * cap)
    n = int(want[1][0])
    assert want[0][0, n - 1] == U and (want[0][0, :n] == J).sum() == 1 and n > 100
    if T == 3:
        assert want[1][1] == 0 and want[1][2] > 0
    for qs in (n, n - 1):                                                     # q_stride == n_total, and one below: the last emission is dropped
        w = _local_three_ways(pkg, m, lkf_row, n_lkf, counts, kf_mp, nmp, valid, qs)
        assert w[2][0] == qs and w[1][0] == n
    _local_three_ways(pkg, m, lkf_row, n_lkf, counts, kf_mp, nmp, None, 64)


@pytest.mark.parametrize("name", sorted(cc.LOCAL_CASES))
def test_local_point_cases(pkg, m, name):
    local, want = cc.LOCAL_CASES[name]()
    F = sr.flatten_local([local, local[::-1]])
    out, nt, nq = _local_three_ways(pkg, m, *[F[k] for k in sr.LOCAL_ORDER], 6)
    assert [F["mps"][j].addr for j in out[0, :nq[0]]] == want == [mp.addr for mp in sr.LocalMapPoints(local, 1)]
    assert [F["mps"][j] for j in out[1, :nq[1]]] == sr.LocalMapPoints(local[::-1], 2)


def test_refused_local_point_arguments_enqueue_nothing(pkg, m):
    T, ls, nrows, cap, nmp, qs = 2, 3, 4, 8, 10, 5
    i32 = lambda n: _up(pkg, np.zeros(n, np.int32))
    a0 = dict(h=m.h, T=T, ls=ls, lkf=i32(T * ls).ptr, n=i32(T).ptr, nrows=nrows, cap=cap, counts=i32(nrows).ptr, kf_mp=i32(nrows * cap).ptr, nmp=nmp, valid=None,
              qs=qs)
    out, nt, nq = _poisoned(pkg, T * qs * 4), _poisoned(pkg, T * 4), _poisoned(pkg, T * 4)
    a0.update(out=out.ptr, nt=nt.ptr, nq=nq.ptr)

    def call(**kw):
        a = dict(a0, **kw)
        return m.L.orbm_local_points_batch_async(a["h"], a["T"], a["ls"], a["lkf"], a["n"], a["nrows"], a["cap"], a["counts"], a["kf_mp"], a["nmp"], a["valid"],
                                                 a["qs"], a["out"], a["nt"], a["nq"])
    for kw in (dict(lkf=None), dict(n=None), dict(counts=None), dict(kf_mp=None), dict(out=None), dict(nt=None), dict(nq=None), dict(T=0), dict(ls=0),
               dict(nrows=0), dict(cap=0), dict(nmp=0), dict(qs=0), dict(h=None)):
        assert call(**kw) == -2, kw
    for kw in (dict(T=65536), dict(ls=65536), dict(cap=65536), dict(ls=65535, cap=65535), dict(T=1 << 9, nmp=(1 << 19) + 1), dict(nmp=(1 << 20) + 1)):
        assert call(**kw) == -3, kw
    d = _poisoned(pkg, 64)
    assert m.L.orbm_gather_map_points_batch_async(m.h, 1, 1, None, nq.ptr, 1, *([None] * 14)) == -2
    assert m.L.orbm_gather_map_points_batch_async(m.h, 1, 1, out.ptr, None, 1, *([None] * 14)) == -2
    assert m.L.orbm_gather_map_points_batch_async(m.h, 0, 1, out.ptr, nq.ptr, 1, *([None] * 14)) == -2
    assert m.L.orbm_gather_map_points_batch_async(m.h, 65536, 1, out.ptr, nq.ptr, 1, *([None] * 14)) == -3
    assert m.L.orbm_gather_map_points_batch_async(m.h, 1, 1, out.ptr, nq.ptr, 1, None, None, None, None, d.ptr + 4, None, None, None, None, None, None,
                                                  d.ptr, None, None) == -2   # a descriptor array that is not 16-byte aligned
    m.sync()
    for b, n in ((out, T * qs * 4 + 4), (nt, T * 4 + 4), (nq, T * 4 + 4), (d, 68)):
        assert np.all(b.download(np.uint8, n) == POISON)
    assert call() == 0, m.L.orbm_last_error()
    m.sync()
    assert np.all(nt.download(np.int32, T) == 0)


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
def _pool(rng, nmp):
    return dict(pw=rng.rand(nmp, 3).astype(np.float32), normal=rng.rand(nmp, 3).astype(np.float32), min_dist=rng.rand(nmp).astype(np.float32),
                max_dist=rng.rand(nmp).astype(np.float32), desc=rng.randint(0, 256, (nmp, 32)).astype(np.uint8), nobs=rng.randint(0, 3, nmp).astype(np.int32))


DST = (("pw", np.float32, 3), ("normal", np.float32, 3), ("min_dist", np.float32, 1), ("max_dist", np.float32, 1), ("qdesc", np.uint8, 32), ("mp_obs", np.uint8, 1),
       ("skip", np.uint8, 1))
SRC = ("pw", "normal", "min_dist", "max_dist", "desc", "nobs")


def test_gather_equals_fancy_indexing(pkg, m):
    rng = np.random.RandomState(5)
    T, qs, nmp = 3, 300, 70
    src = _pool(rng, nmp)
    local_mp = rng.randint(0, nmp, (T, qs)).astype(np.int32)
    local_mp[0, [3, 290]] = [nmp, -1]; local_mp[2, 5] = 1 << 30              # indices only a caller can have written
    nq = np.array([qs + 9, 0, 257], np.int32)
    mp_skip = (rng.rand(T, nmp) < 0.3).astype(np.uint8)
    dsrc = {k: _up(pkg, src[k]) for k in SRC}
    dl, dn, dsk = _up(pkg, local_mp), _up(pkg, nq), _up(pkg, mp_skip)
    for with_skip, drop in ((True, ()), (False, ("normal", "qdesc"))):
        host = {k: np.full((T, qs) + ((w,) if w > 1 else ()), POISON if t is np.uint8 else 0, t) for k, t, w in DST}
        for k, t, w in DST:
            host[k].view(np.uint8)[...] = POISON
        ddst = {k: _up(pkg, host[k]) for k, _, _ in DST}
        dp = lambda k: None if k in drop else ddst[k].ptr
        rc = m.L.orbm_gather_map_points_batch_async(m.h, T, qs, dl.ptr, dn.ptr, nmp, *[dsrc[k].ptr for k in SRC], dsk.ptr if with_skip else None,
                                                    *[dp(k) for k, _, _ in DST])
        assert rc == 0, m.L.orbm_last_error()
        m.sync()
        want = sr.gather_contract(local_mp, nq, src, {k: v.copy() for k, v in host.items()}, mp_skip if with_skip else None)
        for k, t, w in DST:
            got = ddst[k].download(t, host[k].size).reshape(host[k].shape)
            assert got.tobytes() == (host[k] if k in drop else want[k]).tobytes(), k
        assert want["skip"][0, 3] == 1 and np.all(want["pw"][0, 3].view(np.uint8) == POISON) and np.all(want["qdesc"][2, 257:] == POISON)


# ---- the chain in a captured graph ----------------------------------------------------------------------------------------------------
def test_captured_chain_follows_rewritten_rows(pkg, synth):
    """{extraction, grid, votes, local points, gather, isInFrustum, M3} captured once; q_mp, lkf_row and mp_valid are rewritten and the
    graph replayed: every output equals a fresh eager run of the same five calls into other buffers, votes and local points equal the
    contract, and the first state again gives the first result."""
    from test_gpu_local_points_batch import EUROC_K, H, INV_H, INV_W, MBF, NLEV, W, _Rows, _call, _pose
    L = pkg.lib()
    NB = T = 2
    imgs = [synth.gen_image(W, H, 7300 + i) for i in range(NB)]
    stride = (W + 63) // 64 * 64
    dimg = pkg.DeviceBuffer(NB * stride * H)
    for i, im in enumerate(imgs):
        pad = np.zeros((H, stride), np.uint8); pad[:, :W] = im
        dimg.upload(pad, offset=i * stride * H)
    arr = (C.c_void_p * NB)(*[dimg.ptr + i * stride * H for i in range(NB)])
    lap = np.array([(0, 1000)] * NB, np.int32)
    ex = pkg.ORBextractor(1000, max_size=(W, H), max_batch=NB)
    mt = pkg.ORBmatcher(0.9)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(ex.h)) == 0
    ex.enqueue_device(arr, W, H, stride, lap); ex.sync()
    res = ex.fetch_all()
    sf = ex.GetScaleFactors()
    r = ex.result_device(); cap = r["cap"]
    gs = pkg.DeviceBuffer(NB * 3073 * 4); gi = pkg.DeviceBuffer(NB * cap * 4)
    grid = lambda: L.orbm_grid_build_batch_async(mt.h, r["kps"], r["counts"], NB, cap, 0.0, 0.0, INV_W, INV_H, gs.ptr, gi.ptr)
    assert grid() == 0
    # the MapPoint pool: both frames' keypoints back-projected through the identity pose
    rng = np.random.RandomState(17)
    fx, fy, cx, cy = EUROC_K
    k = np.concatenate([res[0][1], res[1][1]]); desc = np.concatenate([res[0][2], res[1][2]])
    nmp = len(k)
    z = rng.uniform(1.0, 10.0, nmp).astype(np.float32)
    Pw = np.stack([(k["x"] - cx) * z / fx, (k["y"] - cy) * z / fy, z], 1).astype(np.float32)
    dist = np.linalg.norm(Pw, axis=1).astype(np.float32)
    mx = (dist * sf[k["octave"]]).astype(np.float32)
    src = dict(pw=Pw, normal=(Pw / dist[:, None]).astype(np.float32), min_dist=(mx / sf[NLEV - 1]).astype(np.float32), max_dist=mx, desc=desc,
               nobs=rng.randint(0, 4, nmp).astype(np.int32))
    dsrc = {kk: _up(pkg, src[kk]) for kk in SRC}
    # the KeyFrame pool of the local map and of the votes
    nrows, kcap, ls, qsv, qs = 9, 300, 4, 200, 700
    counts = rng.randint(200, kcap + 1, nrows).astype(np.int32)
    kf_mp = rng.randint(-1, nmp, (nrows, kcap)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(rng.randint(0, 9, nmp))]).astype(np.int32)
    orow = rng.randint(0, nrows, off[-1]).astype(np.int32); oslot = rng.randint(0, 200, off[-1]).astype(np.int32); ofl = rng.choice([0, 1, 2], off[-1]).astype(np.uint8)
    dcounts, dkf_mp = _up(pkg, counts), _up(pkg, kf_mp)
    doff, drow, dslot, dfl = _up(pkg, off), _up(pkg, orow), _up(pkg, oslot), _up(pkg, ofl)
    q_n, self_row, n_lkf = np.array([qsv, 150], np.int32), np.array([-1, 2], np.int32), np.array([4, 3], np.int32)
    dq_n, dself, dn_lkf = _up(pkg, q_n), _up(pkg, self_row), _up(pkg, n_lkf)
    poses = [_pose(np.random.default_rng(5 + f)) for f in range(T)]
    tcw = _up(pkg, np.stack([np.concatenate([R, t.reshape(3, 1)], 1).reshape(12) for R, t, _ in poses]).astype(np.float32))
    ow = _up(pkg, np.stack([o for _, _, o in poses]).astype(np.float32))
    bounds = np.array([0.0, W, 0.0, H], np.float32)
    lsf = float(np.log(np.float32(1.2)))

    def state(i):
        s = np.random.RandomState(100 + i)
        return dict(q_mp=s.randint(-1, nmp, (T, qsv)).astype(np.int32), lkf_row=s.randint(-1, nrows + 1, (T, ls)).astype(np.int32),
                    valid=(s.rand(nmp) < 0.8).astype(np.uint8), mp_skip=(s.rand(T, nmp) < 0.2).astype(np.uint8))

    states = [state(i) for i in range(3)]
    dq_mp, dlkf, dvalid, dmp_skip = (_up(pkg, states[0][kk]) for kk in ("q_mp", "lkf_row", "valid", "mp_skip"))

    class Out:
        def __init__(self):
            self.votes = {kk: _poisoned(pkg, n) for kk, n in (("votes", T * nrows * 4), ("n_voted", T * 4), ("max_votes", T * 4), ("n_over", T * 4),
                                                              ("list_row", T * 6 * 4), ("list_votes", T * 6 * 4))}
            self.local_mp, self.n_total = _poisoned(pkg, T * qs * 4), _poisoned(pkg, T * 4)
            self.rows = _Rows(pkg, T, qs)                                    # nq, the frustum's seven rows, qdesc, mp_obs
            self.g = {kk: _up(pkg, np.zeros((T, qs, w), t)) for kk, t, w in DST[:4] + DST[6:]}
            self.n_in_view = _poisoned(pkg, T * 4)
            self.match, self.nm = _poisoned(pkg, T * cap * 4), _poisoned(pkg, T * 4)

        def enqueue(self):
            v, R, g = self.votes, self.rows, self.g
            assert L.orbm_covisibility_votes_batch_async(mt.h, T, qsv, dq_mp.ptr, dq_n.ptr, dself.ptr, nrows, kcap, dcounts.ptr, None, 1, nmp, int(off[-1]),
                                                         doff.ptr, drow.ptr, dslot.ptr, dfl.ptr, dvalid.ptr, 15, 6, v["votes"].ptr, v["n_voted"].ptr,
                                                         v["max_votes"].ptr, v["n_over"].ptr, v["list_row"].ptr, v["list_votes"].ptr) == 0, L.orbm_last_error()
            assert L.orbm_local_points_batch_async(mt.h, T, ls, dlkf.ptr, dn_lkf.ptr, nrows, kcap, dcounts.ptr, dkf_mp.ptr, nmp, dvalid.ptr, qs,
                                                   self.local_mp.ptr, self.n_total.ptr, R.nq.ptr) == 0, L.orbm_last_error()
            assert L.orbm_gather_map_points_batch_async(mt.h, T, qs, self.local_mp.ptr, R.nq.ptr, nmp, *[dsrc[kk].ptr for kk in SRC], dmp_skip.ptr,
                                                        g["pw"].ptr, g["normal"].ptr, g["min_dist"].ptr, g["max_dist"].ptr, R.qdesc.ptr, R.mp_obs.ptr,
                                                        g["skip"].ptr) == 0, L.orbm_last_error()
            assert L.orbm_is_in_frustum_batch_async(mt.h, T, tcw.ptr, ow.ptr, R.nq.ptr, qs, g["skip"].ptr, g["pw"].ptr, g["normal"].ptr, g["min_dist"].ptr,
                                                    g["max_dist"].ptr, 0, EUROC_K.ctypes.data_as(C.c_void_p), bounds.ctypes.data_as(C.c_void_p), MBF, 0.5, lsf,
                                                    NLEV, R.in_view.ptr, R.px.ptr, R.py.ptr, R.pxr.ptr, R.depth.ptr, R.level.ptr, R.view_cos.ptr,
                                                    self.n_in_view.ptr) == 0, L.orbm_last_error()
            assert _call(L, mt, r, cap, gs, gi, 0, R, sf, 3.0, 0.8, self.match, self.nm, depth=True, th_far=9.0) == 0, L.orbm_last_error()

        def fetch(self):
            nq = self.rows.nq.download(np.int32, T)
            out = {kk: b.download(np.int32, b.nbytes // 4 - 1) for kk, b in self.votes.items()}
            out.update(n_total=self.n_total.download(np.int32, T), nq=nq, n_in_view=self.n_in_view.download(np.int32, T),
                       match=self.match.download(np.int32, T * cap), nm=self.nm.download(np.int32, T))
            lm = self.local_mp.download(np.int32, T * qs).reshape(T, qs)
            iv = self.rows.in_view.download(np.uint8, T * qs).reshape(T, qs)
            px = self.rows.px.download(np.float32, T * qs).reshape(T, qs)
            qd = self.rows.qdesc.download(np.uint8, T * qs * 32).reshape(T, qs, 32)
            for f in range(T):                                               # the live part of every row; the tails belong to the caller
                out["local_mp%d" % f], out["in_view%d" % f], out["px%d" % f], out["qdesc%d" % f] = lm[f, :nq[f]], iv[f, :nq[f]], px[f, :nq[f]][iv[f, :nq[f]] != 0], qd[f, :nq[f]]
            return out

    def upload(s):
        dq_mp.upload(s["q_mp"]); dlkf.upload(s["lkf_row"]); dvalid.upload(s["valid"]); dmp_skip.upload(s["mp_skip"])

    A, B = Out(), Out()
    want = []
    for s in states:                                                         # the eager runs, ahead of the capture
        upload(s)
        B.enqueue(); mt.sync()
        want.append(B.fetch())
        con = sr.votes_contract(s["q_mp"], q_n, self_row, counts, kcap, None, 1, off, orow, oslot, ofl, s["valid"], 15, 6, list_fill=PI32)
        assert np.array_equal(want[-1]["votes"].reshape(T, nrows), con["votes"]) and np.array_equal(want[-1]["list_row"].reshape(T, 6), con["list_row"])
        lm, nt, nq = sr.local_points_contract(s["lkf_row"], n_lkf, counts, kf_mp, nmp, s["valid"], qs)
        assert np.array_equal(want[-1]["n_total"], nt) and all(np.array_equal(want[-1]["local_mp%d" % f], lm[f, :nq[f]]) for f in range(T))
    assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
    ex.enqueue_device(arr, W, H, stride, lap)
    assert grid() == 0
    A.enqueue()
    assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
    for i in (0, 1, 2, 0):
        upload(states[i])
        assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
        ex.sync()
        got = A.fetch()
        for kk, w in want[i].items():
            assert np.array_equal(got[kk], w), (i, kk)
    assert want[0]["nm"].sum() > 20 and want[0]["n_in_view"].min() > 50 and not np.array_equal(want[0]["match"], want[1]["match"])
    mt.close()


def test_cpp_facade_covisibility(pkg, tmp_path):
    """facade/Covisibility.h on mock KeyFrame / MapPoint / Frame types against the reference's loops in plain C++ in the same file."""
    pkg.build()
    exe = str(tmp_path / "facade_covis_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "facade_covis_smoke.cpp"),
                           "-L", os.path.join(ROOT, "orb-slam3_amd"), "-lorbslam3_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "orb-slam3_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "need-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "facade_covis_smoke ok" in out.stdout, out.stdout + out.stderr
