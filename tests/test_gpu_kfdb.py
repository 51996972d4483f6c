"""The KeyFrameDatabase queries on the device: orbm_bow_vector_batch_async against the second reading of DBoW2's transform tail
(tests/second_reading_frame.py) byte for byte, and orbm_kfdb_query / orbm_kfdb_query_batch_async against the second reading of
KeyFrameDatabase (tests/second_reading_kfdb.py) on the constructed databases of tests/kfdb_cases.py: all eight outputs exactly, score by
bits.  Then refused arguments, a captured graph replayed over a changing pool, facade/KeyFrameDatabase.h on the device, and the chain
extract -> transform -> BowVector -> query -> orbm_search_by_bow_batch_async on the returned candidates."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_cases
import kfdb_cases as kc
import second_reading_frame as srf
from test_gpu_bow_batch import H, W, Pool, _run, _vocab

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_I, SENT_B = -12345, 0x5A
SENT_D = float(np.frombuffer(np.array([0x7FF8DEADBEEF0001], np.uint64).tobytes(), np.float64)[0])     # a NaN with a payload: compared by bytes
OUT8 = ("common", "first_word", "score", "scored", "max_common", "min_common", "nsharing", "nscored")


@pytest.fixture(scope="module")
def M(pkg):
    m = pkg.ORBmatcher(0.9)
    return dict(m=m, L=m.L)


def _up(pkg, a):
    a = np.ascontiguousarray(a)
    return pkg.DeviceBuffer(max(a.nbytes, 8)).upload(a) if a.nbytes else pkg.DeviceBuffer(8)


# ---------------------------------------------------------------------------------------------------------------------------
# part 1: BowVector rows
# ---------------------------------------------------------------------------------------------------------------------------
def _bow_vector(pkg, M, word, weight, counts, cap):
    """Runs the call over rows [nrows][cap] -> (bow_word, bow_val, nbow) with sentinels wherever the call did not write."""
    nrows = len(counts)
    dw, dg, dc = _up(pkg, word.astype(np.int32)), _up(pkg, weight.astype(np.float64)), _up(pkg, np.asarray(counts, np.int32))
    ow = _up(pkg, np.full((nrows, cap), SENT_I, np.int32)); ov = _up(pkg, np.full((nrows, cap), SENT_D, np.float64))
    nb = _up(pkg, np.full(nrows, SENT_I, np.int32))
    assert M["L"].orbm_bow_vector_batch_async(M["m"].h, dw.ptr, dg.ptr, dc.ptr, nrows, cap, ow.ptr, ov.ptr, nb.ptr) == 0, M["L"].orbm_last_error()
    M["m"].sync()
    return ow.download(np.int32, nrows * cap).reshape(nrows, cap), ov.download(np.float64, nrows * cap).reshape(nrows, cap), nb.download(np.int32, nrows)


def _check_bow_rows(got, word, weight, counts, cap):
    gw, gv, gn = got
    sent = np.full(cap, SENT_D, np.float64)
    for r, cnt in enumerate(counts):
        n = min(max(int(cnt), 0), cap)
        ids, vals, _, _ = srf.bow_and_feature_vector(word[r, :n].tolist(), [0] * n, weight[r, :n].tolist())
        k = len(ids)
        assert gn[r] == k, (r, gn[r], k)
        assert np.array_equal(gw[r, :k], ids), r
        assert gv[r, :k].tobytes() == vals.tobytes(), (r, np.flatnonzero(gv[r, :k] != vals)[:4])
        assert np.all(gw[r, k:] == SENT_I) and gv[r, k:].tobytes() == sent[k:].tobytes(), r   # slots past nbow keep the caller's bytes


@pytest.mark.parametrize("cap", kc.BOWVEC_CAPS)
def test_bow_vector_case_rows(pkg, M, cap):
    rows = kc.bow_vector_rows(cap)
    rng = np.random.default_rng(cap + 1)
    n = len(rows) + 2
    word = rng.integers(0, 50, (n, cap)).astype(np.int32); weight = rng.uniform(0.5, 2.0, (n, cap))       # live values beyond every count
    counts = []
    for r, (_, w, g) in enumerate(rows):
        word[r, :len(w)] = w; weight[r, :len(w)] = g
        counts.append(len(w))
    counts += [cap + 9, -3]                                                  # a count above cap is clamped, a negative one is empty
    _check_bow_rows(_bow_vector(pkg, M, word, weight, counts, cap), word, weight, counts, cap)


def test_bow_vector_full_row_at_the_limit(pkg, M):
    cap = pkg.BOWVEC_MAX_CAP
    rng = np.random.default_rng(16384)
    word = rng.integers(0, 5000, (1, cap)).astype(np.int32)
    weight = np.array(kc.MAGNITUDES)[rng.integers(0, 20, (1, cap))]
    weight[0, rng.random(cap) < 0.05] = 0.0
    _check_bow_rows(_bow_vector(pkg, M, word, weight, [cap], cap), word, weight, [cap], cap)


@pytest.mark.parametrize("name", frame_cases.TREE_NAMES)
def test_bow_vector_on_a_real_transform(pkg, M, name):
    """orbm_bow_transform_batch_async feeds the call: ids and values equal the second reading's transform of the same features."""
    L, m = M["L"], M["m"]
    tree = frame_cases.bow_tree(name)
    reading, _ = srf.vocab_from_arrays(tree["k"], tree["L"], tree["parent"], tree["is_leaf"], tree["desc"], tree["weight"])
    feats = frame_cases.bow_features(tree, reading)
    n = len(feats)
    voc = pkg.ORBVocabulary(m, tree)
    dd = _up(pkg, feats); dw = pkg.DeviceBuffer(4 * n); dn = pkg.DeviceBuffer(4 * n); dg = pkg.DeviceBuffer(8 * n)
    assert L.orbm_bow_transform_batch_async(m.h, voc.h, dd.ptr, n, 0, dw.ptr, dn.ptr, dg.ptr) == 0, L.orbm_last_error()
    dc = _up(pkg, np.array([n], np.int32))
    ow = _up(pkg, np.full(n, SENT_I, np.int32)); ov = _up(pkg, np.full(n, SENT_D, np.float64)); nb = _up(pkg, np.full(1, SENT_I, np.int32))
    assert L.orbm_bow_vector_batch_async(m.h, dw.ptr, dg.ptr, dc.ptr, 1, n, ow.ptr, ov.ptr, nb.ptr) == 0, L.orbm_last_error()
    m.sync()
    ids, vals = srf.transform(reading, feats, 0, unwritten_nid=0)[:2]
    k = int(nb.download(np.int32, 1)[0])
    assert k == len(ids) and np.array_equal(ow.download(np.int32, n)[:k], ids)
    assert ov.download(np.float64, n)[:k].tobytes() == vals.tobytes()
    assert (k == 0) == (name == "hand_stopped")


# ---------------------------------------------------------------------------------------------------------------------------
# part 2: the query
# ---------------------------------------------------------------------------------------------------------------------------
class _Pools:
    """The arrays of one call on the device and on the host.  q = (word, val, n) or None for the database pool itself."""

    def __init__(self, pkg, db, q, q_row, active, exclude):
        self.pkg = pkg
        self.dbw, self.dbv, self.dbn = [np.ascontiguousarray(a) for a in db]
        self.alias = q is None
        self.qw, self.qv, self.qn = (self.dbw, self.dbv, self.dbn) if q is None else [np.ascontiguousarray(a) for a in q]
        self.q_row = np.asarray(q_row, np.int32)
        self.active = None if active is None else np.ascontiguousarray(active, np.uint8)
        self.exclude = None if exclude is None else np.ascontiguousarray(exclude, np.uint8)
        self.nq, self.ndb = len(self.q_row), len(self.dbn)
        self.d_db = [_up(pkg, a) for a in (self.dbw, self.dbv, self.dbn)]
        self.d_q = self.d_db if q is None else [_up(pkg, a) for a in (self.qw, self.qv, self.qn)]
        self.d_row = _up(pkg, self.q_row)
        self.d_act = None if self.active is None else _up(pkg, self.active)
        self.d_exc = None if self.exclude is None else _up(pkg, self.exclude)
        n2 = self.nq * self.ndb
        self.sent = dict(common=np.full(n2, SENT_I, np.int32), first_word=np.full(n2, SENT_I, np.int32), score=np.full(n2, -7.5, np.float32),
                         scored=np.full(n2, SENT_B, np.uint8), max_common=np.full(self.nq, SENT_I, np.int32), min_common=np.full(self.nq, SENT_I, np.int32),
                         nsharing=np.full(self.nq, SENT_I, np.int32), nscored=np.full(self.nq, SENT_I, np.int32))
        self.d_out = {k: _up(pkg, v) for k, v in self.sent.items()}

    def args(self, out, **kw):
        a = dict(nq=self.nq, q_row=self.d_row.ptr, nq_rows=len(self.qn), q_cap=self.qw.shape[1], q_word=self.d_q[0].ptr, q_val=self.d_q[1].ptr,
                 q_n=self.d_q[2].ptr, ndb_rows=self.ndb, db_cap=self.dbw.shape[1], db_word=self.d_db[0].ptr, db_val=self.d_db[1].ptr, db_n=self.d_db[2].ptr,
                 db_active=self.d_act.ptr if self.d_act else None, exclude=self.d_exc.ptr if self.d_exc else None)
        a.update(out)
        a.update(kw)
        return [a[k] for k in ("nq", "q_row", "nq_rows", "q_cap", "q_word", "q_val", "q_n", "ndb_rows", "db_cap", "db_word", "db_val", "db_n", "db_active",
                               "exclude") + OUT8]

    def device(self, M, **kw):
        return M["L"].orbm_kfdb_query_batch_async(M["m"].h, *self.args({k: self.d_out[k].ptr for k in OUT8}, **kw))

    def fetch(self):
        return {k: self.d_out[k].download(v.dtype, len(v)) for k, v in self.sent.items()}

    def untouched(self):
        return all(v.tobytes() == self.sent[k].tobytes() for k, v in self.fetch().items())

    def host(self, M, **kw):
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        out = {k: v.copy() for k, v in self.sent.items()}
        a = dict(q_row=vp(self.q_row), q_word=vp(self.qw), q_val=vp(self.qv), q_n=vp(self.qn), db_word=vp(self.dbw), db_val=vp(self.dbv), db_n=vp(self.dbn),
                 db_active=vp(self.active), exclude=vp(self.exclude))
        a.update({k: vp(v) for k, v in out.items()})
        a.update(kw)
        return M["L"].orbm_kfdb_query(M["m"].h, *self.args({}, **a)), out


def _compare(got, want_per_query, ndb, label):
    """got: the eight flat arrays; want_per_query: the second reading's dicts."""
    for q, e in enumerate(want_per_query):
        s = slice(q * ndb, (q + 1) * ndb)
        for k in ("common", "first_word", "scored"):
            assert np.array_equal(got[k][s], e[k]), (label, q, k, np.flatnonzero(got[k][s] != e[k])[:6])
        assert got["score"][s].tobytes() == np.ascontiguousarray(e["score"], np.float32).tobytes(), \
            (label, q, "score", np.flatnonzero(got["score"][s].view(np.uint32) != e["score"].view(np.uint32))[:6])
        for k in ("max_common", "min_common", "nsharing", "nscored"):
            assert got[k][q] == e[k], (label, q, k, got[k][q], e[k])


def _both_forms(pkg, M, pools, want, label):
    assert pools.device(M) == 0, M["L"].orbm_last_error()
    M["m"].sync()
    _compare(pools.fetch(), want, pools.ndb, label + " device")
    rc, out = pools.host(M)
    assert rc == 0, M["L"].orbm_last_error()
    _compare(out, want, pools.ndb, label + " host")


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_query_cases(pkg, M, name):
    """Host form == device form == second reading, the relocalization form (no exclude) and the place-recognition form; db_cap != q_cap."""
    c = kc.case(name)
    db = c.pool(c.max_len() + 3)
    q = c.query_pool(len(c.query[0]) + 1)
    assert db[0].shape[1] != q[0].shape[1]
    _both_forms(pkg, M, _Pools(pkg, db[:3], q, [0], db[3], None), [kc.expected(c, False)], name + " reloc")
    _both_forms(pkg, M, _Pools(pkg, db[:3], q, [0], db[3], np.array([c.exclude], np.uint8)), [kc.expected(c, True)], name + " place")
    if all(c.active):
        _both_forms(pkg, M, _Pools(pkg, db[:3], q, [0], None, None), [kc.expected(c, False)], name + " db_active NULL")


def test_python_mirror(pkg, M):
    """ORBmatcher.KfdbQuery, KfdbQueryBatchAsync and BowVectorBatchAsync reach the same three entry points."""
    c = kc.case("masked_maximum")
    m = M["m"]
    db = c.pool(c.max_len()); q = c.query_pool(c.max_len() + 2)
    exclude = np.array([c.exclude], np.uint8)
    got = m.KfdbQuery([0], q[0], q[1], q[2], db[0], db[1], db[2], db[3], exclude)
    _compare({k: got[k].reshape(-1) for k in OUT8}, [kc.expected(c, True)], len(c.rows), "KfdbQuery")
    same = m.KfdbQuery([1, 3], db[0], db[1], db[2], db[0], db[1], db[2])
    assert same["common"][0, 1] == len(c.rows[1][0]) and same["common"][1, 3] == len(c.rows[3][0]) and same["common"].shape == (2, len(c.rows))
    P = _Pools(pkg, db[:3], q, [0], db[3], exclude)
    assert m.KfdbQueryBatchAsync(*P.args({k: P.d_out[k].ptr for k in OUT8})) == 0
    m.sync()
    _compare(P.fetch(), [kc.expected(c, True)], len(c.rows), "KfdbQueryBatchAsync")
    with pytest.raises(pkg.OrbError):
        m.KfdbQueryBatchAsync(*P.args({k: P.d_out[k].ptr for k in OUT8}, q_cap=65536))
    word = np.array([[7, 3, 7, 9]], np.int32); weight = np.array([[0.5, 0.25, 0.25, 0.0]])
    dw, dg, dc = _up(pkg, word), _up(pkg, weight), _up(pkg, np.array([4], np.int32))
    ow, ov, nb = pkg.DeviceBuffer(16), pkg.DeviceBuffer(32), pkg.DeviceBuffer(4)
    assert m.BowVectorBatchAsync(dw.ptr, dg.ptr, dc.ptr, 1, 4, ow.ptr, ov.ptr, nb.ptr) == 0
    m.sync()
    assert nb.download(np.int32, 1)[0] == 2 and ow.download(np.int32, 2).tolist() == [3, 7] and ov.download(np.float64, 2).tolist() == [0.25, 0.75]


def _with_query(c, ids_vals, exclude):
    import copy
    d = copy.copy(c)
    d.query, d.exclude = ids_vals, list(exclude)
    return d


@pytest.mark.parametrize("nq", [1, 3])
def test_queries_from_the_database_pool(pkg, M, nq):
    """The query pool aliases the database pool: a KeyFrame queries the database it is in (it finds itself, unless it is excluded)."""
    c = kc.case("rows_65")
    q_row = [5, 0, 17][:nq]
    rng = np.random.default_rng(nq)
    exclude = (rng.random((nq, len(c.rows))) < 0.2).astype(np.uint8)
    for q, r in enumerate(q_row):
        exclude[q, r] = q % 2                                                # query 1 excludes itself, the others meet themselves
    db = c.pool(c.max_len())
    want_r = [kc.expected(_with_query(c, c.rows[r], [False] * len(c.rows)), False) for r in q_row]
    want_p = [kc.expected(_with_query(c, c.rows[r], exclude[q]), True) for q, r in enumerate(q_row)]
    assert want_r[0]["common"][5] == len(c.rows[5][0]) and c.active[5]
    _both_forms(pkg, M, _Pools(pkg, db[:3], None, q_row, db[3], None), want_r, "alias reloc")
    _both_forms(pkg, M, _Pools(pkg, db[:3], None, q_row, db[3], exclude), want_p, "alias place")


def test_q_row_out_of_range_writes_the_empty_result(pkg, M):
    c = kc.case("same_first_word")
    db = c.pool(c.max_len()); q = c.query_pool(c.max_len())
    P = _Pools(pkg, db[:3], q, [0, -1, 1, 0], db[3], None)
    assert P.device(M) == 0, M["L"].orbm_last_error()
    M["m"].sync()
    e = kc.expected(c, False)
    n = len(c.rows)
    empty = dict(common=np.zeros(n, np.int32), first_word=np.full(n, -1, np.int32), score=np.zeros(n, np.float32), scored=np.zeros(n, np.uint8),
                 max_common=0, min_common=0, nsharing=0, nscored=0)
    _compare(P.fetch(), [e, empty, empty, e], n, "q_row")
    rc, out = P.host(M)
    assert rc == -2 and all(v.tobytes() == P.sent[k].tobytes() for k, v in out.items())


def test_largest_shape(pkg, M):
    """4096 rows of up to 256 words."""
    c = kc.big_case()
    db = c.pool(256); q = c.query_pool(256)
    e = kc.expected(c, False)
    assert e["nsharing"] > 3000 and e["nscored"] > 50
    _both_forms(pkg, M, _Pools(pkg, db[:3], q, [0], db[3], None), [e], "big")


def test_refused_arguments_leave_the_outputs_untouched(pkg, M):
    L, m = M["L"], M["m"]
    c = kc.case("same_first_word")
    db = c.pool(c.max_len()); q = c.query_pool(c.max_len())
    P = _Pools(pkg, db[:3], q, [0], db[3], np.zeros((1, len(c.rows)), np.uint8))
    required = ("q_row", "q_word", "q_val", "q_n", "db_word", "db_val", "db_n") + OUT8
    for k in required:
        assert P.device(M, **{k: None}) == -2, k
        assert P.host(M, **{k: None})[0] == -2, k
    for k in ("nq", "nq_rows", "q_cap", "ndb_rows", "db_cap"):
        for v in (0, -4):
            assert P.device(M, **{k: v}) == -2 and P.host(M, **{k: v})[0] == -2, (k, v)
    for kw in (dict(q_cap=65536), dict(db_cap=65536), dict(ndb_rows=pkg.KFDB_MAX_ROWS + 1), dict(nq=pkg.KFDB_MAX_QUERIES + 1)):
        assert P.device(M, **kw) == -3 and P.host(M, **kw)[0] == -3, kw
    assert L.orbm_kfdb_query_batch_async(None, *P.args({k: P.d_out[k].ptr for k in OUT8})) == -2
    for bad in (-1, 1, 7):
        P.q_row[0] = bad
        rc, out = P.host(M)
        assert rc == -2 and all(v.tobytes() == P.sent[k].tobytes() for k, v in out.items()), bad
    P.q_row[0] = 0
    # part 1
    w = _up(pkg, np.zeros(8, np.int32)); g = _up(pkg, np.ones(8, np.float64)); cn = _up(pkg, np.array([8], np.int32))
    ow = _up(pkg, np.full(8, SENT_I, np.int32)); ov = _up(pkg, np.full(8, SENT_D, np.float64)); nb = _up(pkg, np.full(1, SENT_I, np.int32))
    full = [w.ptr, g.ptr, cn.ptr, 1, 8, ow.ptr, ov.ptr, nb.ptr]
    for i in (0, 1, 2, 5, 6, 7):
        a = list(full); a[i] = None
        assert L.orbm_bow_vector_batch_async(m.h, *a) == -2, i
    for i in (3, 4):
        for v in (0, -1):
            a = list(full); a[i] = v
            assert L.orbm_bow_vector_batch_async(m.h, *a) == -2, (i, v)
    a = list(full); a[4] = pkg.BOWVEC_MAX_CAP + 1
    assert L.orbm_bow_vector_batch_async(m.h, *a) == -3
    assert L.orbm_bow_vector_batch_async(None, *full) == -2
    m.sync()
    assert P.untouched()
    assert np.all(ow.download(np.int32, 8) == SENT_I) and nb.download(np.int32, 1)[0] == SENT_I
    assert ov.download(np.float64, 8).tobytes() == np.full(8, SENT_D, np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# the facade on the device
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facade_exe(pkg, tmp_path_factory):
    pkg.build()
    exe = str(tmp_path_factory.mktemp("kfdb") / "kfdb_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-DKFDB_WITH_LIBRARY", "-o", exe,
                           os.path.join(ROOT, "tests", "kfdb_facade.cpp"), "-L", os.path.join(ROOT, "orb-slam3_amd"), "-lorbslam3_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "orb-slam3_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _facade(exe, tmp_path, mode, items):
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write(kc.facade_text(items))
    res = subprocess.run([exe, mode, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return kc.parse_facade_output(res.stdout, items)


def test_cpp_facade_on_the_device(facade_exe, tmp_path):
    """facade/KeyFrameDatabase.h end to end on mock types: add, erase, the device query, the selection.  The lists and the members equal
    the second reading's on every constructed case and on 30 random databases, both forms."""
    cases = [kc.case(n) for n in kc.CASE_NAMES] + [kc.random_case(s) for s in range(30)]
    # the program queries the device itself: the three rows of the file are not read
    items = [(c, place, dict(common=[0] * len(c.rows), first_word=[-1] * len(c.rows), score=np.zeros(len(c.rows), np.float32)))
             for c in cases for place in (False, True)]
    for got, (c, place, _) in zip(_facade(facade_exe, tmp_path, "device", items), items):
        kc.check_facade(got, c, place)


# ---------------------------------------------------------------------------------------------------------------------------
# extract -> transform -> BowVector -> query -> SearchByBoW on the candidates; and the same step captured
# ---------------------------------------------------------------------------------------------------------------------------
NKF, NF = 6, 3


@pytest.fixture(scope="module")
def step(pkg, synth):
    pairs = [synth.gen_stereo_pair(W, H, 900 + i) for i in range(NKF)]
    mt = pkg.ORBmatcher(0.75)
    K = Pool(pkg, mt, [p[0] for p in pairs], 600)
    F = Pool(pkg, mt, [pairs[i][1] for i in range(NF)], 500)
    voc = _vocab(pkg, synth, mt, 10, 4)
    K.transform(voc, 4); F.transform(voc, 4)
    for pool in (K, F):
        n = pool.rows * pool.cap
        pool.bw, pool.bv, pool.bn = pkg.DeviceBuffer(4 * n), pkg.DeviceBuffer(8 * n), pkg.DeviceBuffer(4 * pool.rows)
    yield mt, K, F, voc
    K.ex.close(); F.ex.close()


def _bow_rows(pool):
    """The second reading's BowVector of every row of a pool, from the downloaded words and weights."""
    out = []
    for r in range(pool.rows):
        n = len(pool.kps(r))
        ids, vals, _, _ = srf.bow_and_feature_vector(pool.h_word[r, :n].tolist(), [0] * n, pool.h_weight[r, :n].tolist())
        out.append((ids, vals))
    return out


def _enqueue_bow_vectors(L, mt, pool):
    assert L.orbm_bow_vector_batch_async(mt.h, pool.word.ptr, pool.weight.ptr, pool.r["counts"], pool.rows, pool.cap, pool.bw.ptr, pool.bv.ptr,
                                         pool.bn.ptr) == 0, L.orbm_last_error()


def _reading_of(rows_kf, active, query):
    c = kc.Case("chain", 1)
    c.rows, c.active, c.query = list(rows_kf), list(active), query
    return c.finish()


def test_chain_extract_to_search_by_bow(pkg, oracle, step, facade_exe, tmp_path):
    mt, K, F, voc = step
    L = pkg.lib()
    _enqueue_bow_vectors(L, mt, K); _enqueue_bow_vectors(L, mt, F)
    out = {k: pkg.DeviceBuffer(8 * K.rows) for k in OUT8}
    d_row = _up(pkg, np.array([1], np.int32))
    rc = L.orbm_kfdb_query_batch_async(mt.h, 1, d_row.ptr, F.rows, F.cap, F.bw.ptr, F.bv.ptr, F.bn.ptr, K.rows, K.cap, K.bw.ptr, K.bv.ptr, K.bn.ptr, None, None,
                                       *[out[k].ptr for k in OUT8])
    assert rc == 0, L.orbm_last_error()
    mt.sync()
    rows_kf, rows_f = _bow_rows(K), _bow_rows(F)
    for pool, rows in ((K, rows_kf), (F, rows_f)):                           # the BowVector rows the query read
        bn = pool.bn.download(np.int32, pool.rows)
        bw = pool.bw.download(np.int32, pool.rows * pool.cap).reshape(pool.rows, pool.cap)
        bv = pool.bv.download(np.float64, pool.rows * pool.cap).reshape(pool.rows, pool.cap)
        for r, (ids, vals) in enumerate(rows):
            assert bn[r] == len(ids) and np.array_equal(bw[r, :len(ids)], ids) and bv[r, :len(ids)].tobytes() == vals.tobytes(), r
    c = _reading_of(rows_kf, [True] * K.rows, rows_f[1])
    c.map_of, c.covisible = [0] * K.rows, [[] for _ in range(K.rows)]        # one map, no neighbours: every group is its own KeyFrame
    e = kc.expected(c, False)
    dtypes = dict(common=np.int32, first_word=np.int32, score=np.float32, scored=np.uint8)
    got = {k: out[k].download(dtypes.get(k, np.int32), K.rows if k in dtypes else 1) for k in OUT8}
    _compare(got, [e], K.rows, "chain")
    assert e["nsharing"] == K.rows and e["scored"][1] == 1                   # the frame is the right image of KeyFrame 1's pair
    cand = _facade(facade_exe, tmp_path, "select", [(c, False, got)])[0]
    kc.check_facade(cand, c, False)
    kf_row = cand[0]["R"]
    assert int(np.argmax(e["score"])) in kf_row                              # bestAccScore is the best score: its KeyFrame passes the 0.75f cut
    good = np.ones(K.rows * K.cap, np.uint8)
    fm, nm = _run(pkg, mt, K, F, kf_row, [1] * len(kf_row), good, 0.75, 1)   # Tracking::Relocalization's SearchByBoW on the candidates
    from test_gpu_bow_batch import _check
    _check(pkg, oracle, mt, K, F, kf_row, [1] * len(kf_row), good, 0.75, 1, fm, nm)
    print("chain: candidates %s of %d KeyFrames, scores %s, matches %s" % (kf_row, K.rows, e["score"].tolist(), nm.tolist()))
    assert nm.max() > 50


def test_capture_replay_over_a_changing_pool(pkg, step):
    """The step -- extraction of the frames, their transform, their BowVectors, the query -- is captured after one eager run and replayed
    three times; the database pool is rewritten between the replays, first to rows that share far fewer words (a max_common left over
    from the replay before would raise min_common and lose scored rows), then back."""
    mt, K, F, voc = step
    L = pkg.lib()
    _enqueue_bow_vectors(L, mt, K)
    mt.sync()
    n = K.rows * K.cap
    full = (K.bw.download(np.int32, n), K.bv.download(np.float64, n), K.bn.download(np.int32, K.rows))
    rows_kf, rows_f = _bow_rows(K), _bow_rows(F)
    thin_n = np.minimum(full[2], 40).astype(np.int32)                        # every row cut to its first 40 words
    thin_rows = [(ids[:40], vals[:40]) for ids, vals in rows_kf]
    dbn = _up(pkg, full[2])
    out = {k: _up(pkg, np.full(2 * K.rows, SENT_I, np.int32)) for k in OUT8}
    d_row = _up(pkg, np.array([1, 2], np.int32))
    active = np.ones(K.rows, np.uint8); active[0] = 0
    d_act = _up(pkg, active)
    assert L.orbm_set_stream(mt.h, L.orbx_stream(F.ex.h)) == 0

    def enqueue():
        F.ex.enqueue_device(F.arr, W, H, F.stride, np.zeros(4 * F.rows, np.int32))
        assert L.orbm_bow_transform_batch_async(mt.h, voc.h, F.r["desc"], F.rows * F.cap, 4, F.word.ptr, F.node.ptr, F.weight.ptr) == 0
        _enqueue_bow_vectors(L, mt, F)
        assert L.orbm_kfdb_query_batch_async(mt.h, 2, d_row.ptr, F.rows, F.cap, F.bw.ptr, F.bv.ptr, F.bn.ptr, K.rows, K.cap, K.bw.ptr, K.bv.ptr, dbn.ptr,
                                             d_act.ptr, None, *[out[k].ptr for k in OUT8]) == 0, L.orbm_last_error()

    def check(rows, label):
        dtypes = dict(common=np.int32, first_word=np.int32, score=np.float32, scored=np.uint8)
        got = {k: out[k].download(dtypes.get(k, np.int32), 2 * K.rows if k in dtypes else 2) for k in OUT8}
        want = [kc.expected(_reading_of(rows, active, rows_f[q]), False) for q in (1, 2)]
        _compare(got, want, K.rows, label)
        return want

    enqueue()
    F.ex.sync()
    w_full = check(rows_kf, "eager")
    assert L.orbx_capture_begin(F.ex.h, 0) == 0, L.orbx_last_error()
    enqueue()
    assert L.orbx_capture_end(F.ex.h) == 0, L.orbx_last_error()
    for it, (cnt, rows) in enumerate(((thin_n, thin_rows), (full[2], rows_kf), (thin_n, thin_rows))):
        dbn.upload(cnt)
        for k in OUT8:
            out[k].upload(np.full(2 * K.rows, SENT_I, np.int32))
        assert L.orbx_graph_launch(F.ex.h, 0) == 0, L.orbx_last_error()
        F.ex.sync()
        w = check(rows, "replay %d" % it)
        if it != 1:
            assert w[0]["max_common"] < w_full[0]["max_common"] and w[0]["min_common"] < w_full[0]["min_common"]
    assert L.orbm_set_stream(mt.h, None) == 0
