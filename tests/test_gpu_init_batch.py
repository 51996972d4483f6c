"""orbm_search_for_initialization_batch_async (M9 end to end on the device) against the host entry orbm_search_for_initialization, the
CPU oracle and the second reading (tests/second_reading_init.py).  Everything compared is an integer or a copied float: bit-exact.
The frames are laid out as pools whose slots beyond a row's count hold a real level-0 keypoint and its descriptor -- data that would
match if it were read."""
import ctypes as C

import numpy as np
import pytest

import init_cases as ic
import second_reading as sr
import second_reading_init as sri

pytestmark = pytest.mark.gpu
NAME = "orbm_search_for_initialization_batch_async"
SENT = np.float32(-777.25)                                # prev_out entries the call must not write


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def frames(synth, oracle):
    return ic.scene_frames(synth, oracle)


@pytest.fixture(scope="module")
def OM(oracle):
    return oracle._oracle_matcher_class()()


@pytest.fixture(scope="module")
def mt(pkg):
    m = pkg.ORBmatcher(0.9)
    yield m
    m.close()


def own_xy(k):
    return np.stack([k["x"], k["y"]], 1).astype(np.float32)


def oracle_ref(pkg, OM, f1, f2, prev, window, nnratio, ori):
    v1 = pkg.FrameView(f1[0], f1[1], ic.W, ic.H, backend=OM); v2 = pkg.FrameView(f2[0], f2[1], ic.W, ic.H, backend=OM)
    return OM.SearchForInitialization(v1, v2, prev, window, nnratio, ori)


class Pool:
    def __init__(self, pkg, rows, pad):
        cap = max([len(k) for k, _ in rows] + [1]) + pad
        src = next(((k, d) for k, d in rows if len(k) and (k["octave"] == 0).any()), None)
        if src is None:
            filler = (np.zeros(1, ic.KP_DTYPE)[0], np.zeros(32, np.uint8))
        else:
            i = int(np.nonzero(src[0]["octave"] == 0)[0][0])
            filler = (src[0][i], src[1][i])
        self.kps, self.desc, self.counts = ic.make_pool(rows, cap, filler)
        self.rows, self.cap, self.n = rows, cap, len(rows)
        self.dk = pkg.DeviceBuffer(self.kps.nbytes).upload(self.kps); self.dd = pkg.DeviceBuffer(self.desc.nbytes).upload(self.desc)
        self.dc = pkg.DeviceBuffer(4 * self.n).upload(self.counts)
        self.gs = pkg.DeviceBuffer(4 * 3073 * self.n); self.gi = pkg.DeviceBuffer(4 * cap * self.n)

    def build_grid(self, L, mt):
        assert L.orbm_grid_build_batch_async(mt.h, self.dk.ptr, self.dc.ptr, self.n, self.cap, 0.0, 0.0, float(ic.INV_W), float(ic.INV_H),
                                             self.gs.ptr, self.gi.ptr) == 0, L.orbm_last_error()
        return self


def run(pkg, mt, A, B, row1, row2, prevs, window, nnratio, ori, in_place=False, null_rows=False):
    """prevs: per pair an [n1][2] array (or None for a pair without a valid pool-1 row).  Returns rows, counts, prev_out [P][cap1][2]."""
    L = pkg.lib()
    P = len(row1)
    pin = np.empty((P, A.cap, 2), np.float32)
    pin[:] = own_xy(A.kps[0])[A.cap - 1] if A.cap else 0                     # padding: the filler keypoint's own position
    for p, pv in enumerate(prevs):
        if pv is not None:
            pin[p, :len(pv)] = pv
    dpi = pkg.DeviceBuffer(pin.nbytes).upload(pin)
    dpo = dpi if in_place else pkg.DeviceBuffer(pin.nbytes).upload(np.full(pin.shape, SENT, np.float32))
    d1 = pkg.DeviceBuffer(4 * P).upload(np.asarray(row1, np.int32)); d2 = pkg.DeviceBuffer(4 * P).upload(np.asarray(row2, np.int32))
    mm = pkg.DeviceBuffer(4 * P * A.cap).upload(np.full(P * A.cap, -7, np.int32)); nm = pkg.DeviceBuffer(4 * P).upload(np.full(P, -7, np.int32))
    rc = getattr(L, NAME)(mt.h, P, A.n, A.cap, A.dk.ptr, A.dd.ptr, A.dc.ptr, B.n, B.cap, B.dk.ptr, B.dd.ptr, B.dc.ptr, B.gs.ptr, B.gi.ptr,
                          0.0, 0.0, float(ic.INV_W), float(ic.INV_H), None if null_rows else d1.ptr, None if null_rows else d2.ptr, dpi.ptr,
                          int(window), float(nnratio), int(ori), mm.ptr, nm.ptr, dpo.ptr)
    assert rc == 0, L.orbm_last_error()
    mt.sync()
    return (mm.download(np.int32, P * A.cap).reshape(P, A.cap), nm.download(np.int32, P),
            dpo.download(np.float32, P * A.cap * 2).reshape(P, A.cap, 2), pin)


_SECOND = {}


def second_reading_ref(f1, f2, prev, window, nnratio, ori):
    """The second reading of one pair, computed once per distinct input (several tests search the same pairs)."""
    key = (f1[0].tobytes(), f1[1].tobytes(), f2[0].tobytes(), f2[1].tobytes(), np.asarray(prev, np.float32).tobytes(), window, float(nnratio), bool(ori))
    if key not in _SECOND:
        _SECOND[key] = sri.search_for_initialization(sr.GridFrame(f1[0], f1[1], 0.0, 0.0, ic.INV_W, ic.INV_H),
                                                     sr.GridFrame(f2[0], f2[1], 0.0, 0.0, ic.INV_W, ic.INV_H), prev, window, nnratio, bool(ori))
    return _SECOND[key]


def check(pkg, OM, A, B, row1, row2, prevs, window, nnratio, ori, got, in_place=False, mt=None, second=True):
    """Every pair against the oracle; with `mt` also against the host entry orbm_search_for_initialization, with `second` also against
    the second reading (tests/second_reading_init.py)."""
    rows, counts, pout, pin = got
    refs = []
    for p, (r1, r2) in enumerate(zip(row1, row2)):
        ok1, ok2 = 0 <= r1 < A.n, 0 <= r2 < B.n
        n1 = len(A.rows[r1][0]) if ok1 else 0
        if ok1 and ok2 and n1 and len(B.rows[r2][0]):
            n, m, pv = oracle_ref(pkg, OM, A.rows[r1], B.rows[r2], prevs[p], window, nnratio, ori)
            if mt is not None:
                v1 = pkg.FrameView(A.rows[r1][0], A.rows[r1][1], ic.W, ic.H, backend=mt); v2 = pkg.FrameView(B.rows[r2][0], B.rows[r2][1], ic.W, ic.H, backend=mt)
                n_h, m_h, p_h = mt.SearchForInitialization(v1, v2, prevs[p], window, nnratio, bool(ori))
                assert n_h == n and np.array_equal(m_h, m) and np.array_equal(p_h.view(np.uint32), np.asarray(pv, np.float32).view(np.uint32)), p
            if second:
                n_s, m_s, p_s, _ = second_reading_ref(A.rows[r1], B.rows[r2], prevs[p], window, nnratio, ori)
                assert n_s == n and np.array_equal(m_s, m) and np.array_equal(p_s.view(np.uint32), np.asarray(pv, np.float32).view(np.uint32)), p
        else:
            n, m, pv = 0, np.full(n1, -1, np.int32), (prevs[p] if n1 else np.zeros((0, 2), np.float32))
        assert counts[p] == n, (p, int(counts[p]), n)
        assert np.array_equal(rows[p, :n1], m), (p, np.nonzero(rows[p, :n1] != m)[0][:8])
        assert np.all(rows[p, n1:] == -1), p
        assert np.array_equal(pout[p, :n1].view(np.uint32), np.asarray(pv, np.float32).view(np.uint32)), p
        tail = pin[p, n1:] if in_place else np.full((A.cap - n1, 2), SENT, np.float32)
        assert np.array_equal(pout[p, n1:], tail), p                         # entries at or beyond the count are not written
        refs.append((n, m, pv))
    return refs


@pytest.mark.parametrize("ori", [1, 0])
def test_scene_pairs_with_row_indirection(pkg, OM, mt, frames, ori):
    """Nine pairs over two pools: three real pairs, a frame against itself, an empty row on either side, rows out of range on either
    side.  Every real pair is compared with the oracle, the host entry and the second reading (check)."""
    f0, f1, f2 = frames
    empty = (f0[0][:0], f0[1][:0])
    A = Pool(pkg, [f0, f1, empty], 37); B = Pool(pkg, [f1, f2, f0, empty], 53).build_grid(pkg.lib(), mt)
    row1 = [0, 0, 1, 1, 0, 2, 0, 0, -1]; row2 = [0, 1, 1, 2, 2, 0, 3, 7, 0]
    prevs = [own_xy(A.rows[r][0]) if 0 <= r < A.n else None for r in row1]
    got = run(pkg, mt, A, B, row1, row2, prevs, 100, 0.9, ori)
    refs = check(pkg, OM, A, B, row1, row2, prevs, 100, 0.9, ori, got, mt=mt)
    assert refs[0][0] >= 250 and refs[4][0] >= 400                           # the self pair matches nearly every level-0 keypoint
    t = second_reading_ref(f0, f1, prevs[0], 100, 0.9, ori)[3]
    assert t["steal"] >= 1 and t["query_outcome_changed_by_skip"] >= 1     # pair 0 reaches the order-dependent branches


def test_one_pool_passed_twice_null_rows_then_a_smaller_shape(pkg, OM, mt, frames):
    """One pool as both sides with row1 = row2 = NULL (pair p = row p against itself), then the same handle on a smaller shape."""
    f0, f1, f2 = frames
    A = Pool(pkg, [f0, f1, f2], 41).build_grid(pkg.lib(), mt)
    prevs = [own_xy(k) for k, _ in A.rows]
    got = run(pkg, mt, A, A, [0, 1, 2], [0, 1, 2], prevs, 100, 0.9, 1, null_rows=True)
    check(pkg, OM, A, A, [0, 1, 2], [0, 1, 2], prevs, 100, 0.9, 1, got, mt=mt)
    got = run(pkg, mt, A, A, [0, 2], [1, 0], [prevs[0], prevs[2]], 100, 0.9, 1)
    check(pkg, OM, A, A, [0, 2], [1, 0], [prevs[0], prevs[2]], 100, 0.9, 1, got, mt=mt)
    small = [(k[:200], d[:200]) for k, d in (f0, f1)]
    S = Pool(pkg, small, 5).build_grid(pkg.lib(), mt)
    got = run(pkg, mt, S, S, [0], [1], [own_xy(small[0][0])], 100, 0.9, 1)
    check(pkg, OM, S, S, [0], [1], [own_xy(small[0][0])], 100, 0.9, 1, got, mt=mt)


CASES = ic.constructed_pairs()


@pytest.mark.parametrize("nnratio", sorted({p.nnratio for p, _ in CASES.values()}))
def test_constructed_pairs_in_rows_of_a_small_pool(pkg, OM, mt, nnratio):
    names = [n for n in sorted(CASES) if CASES[n][0].nnratio == nnratio]
    arrs = [CASES[n][0].arrays() for n in names]
    A = Pool(pkg, [(a[0], a[1]) for a in arrs], 3); B = Pool(pkg, [(a[2], a[3]) for a in arrs], 7).build_grid(pkg.lib(), mt)
    rows_ = list(range(len(names)))
    prevs = [a[4] for a in arrs]
    got = run(pkg, mt, A, B, rows_, rows_, prevs, ic.WINDOW, nnratio, 1)
    check(pkg, OM, A, B, rows_, rows_, prevs, ic.WINDOW, nnratio, 1, got, mt=mt)
    for p, n in enumerate(names):
        expect = CASES[n][1]
        for q, s in expect["m12"].items():
            assert got[0][p, q] == s, (n, q)
        if "nmatches" in expect:
            assert got[1][p] == expect["nmatches"], n
        if "differs_from_finished_row_cull" in expect:
            a = arrs[p]
            _, _, _, t = sri.search_for_initialization(sr.GridFrame(a[0], a[1], 0.0, 0.0, ic.INV_W, ic.INV_H),
                                                       sr.GridFrame(a[2], a[3], 0.0, 0.0, ic.INV_W, ic.INV_H), a[4], ic.WINDOW, nnratio, True)
            _, m_f = sri.cull_from_finished_row(sr.GridFrame(a[0], a[1], 0.0, 0.0, ic.INV_W, ic.INV_H),
                                                sr.GridFrame(a[2], a[3], 0.0, 0.0, ic.INV_W, ic.INV_H), np.array(t["row_before_cull"]))
            assert not np.array_equal(m_f, got[0][p, :len(m_f)])              # the device did not cull from the finished row


def test_every_level0_slot_in_one_window(pkg, OM, mt):
    """5 000 level-0 slots inside every query's window: more candidates per query than the host entry's table holds (it caps a query's
    list at 4 096 entries, so it is left out here) and more than one chunk of the device's candidate scratch.  Against the oracle."""
    rng = np.random.default_rng(11)
    n2, n1 = 5000, 300
    k2 = np.zeros(n2, ic.KP_DTYPE); k2["x"] = rng.uniform(150, 210, n2); k2["y"] = rng.uniform(90, 150, n2)
    k2["angle"] = rng.uniform(0, 360, n2); k2["size"] = 31
    k2["octave"][rng.random(n2) < 0.1] = 2
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    src = rng.integers(0, n2, n1)
    k1 = k2[src].copy(); k1["x"] += rng.uniform(-3, 3, n1).astype(np.float32); k1["angle"] = (k1["angle"] + rng.choice([0, 0, 0, 40], n1)) % 360
    d1 = d2[src].copy()
    flip = rng.integers(0, 256, (n1, 30))
    for i in range(n1):
        for b in flip[i, :rng.integers(0, 30)]:
            d1[i, b >> 3] ^= np.uint8(1 << (b & 7))
    A = Pool(pkg, [(k1, d1)], 11); B = Pool(pkg, [(k2, d2)], 13).build_grid(pkg.lib(), mt)
    prevs = [own_xy(k1)]
    for ori in (1, 0):
        got = run(pkg, mt, A, B, [0], [0], prevs, 100, 0.9, ori)
        (n, m, _), = check(pkg, OM, A, B, [0], [0], prevs, 100, 0.9, ori, got, second=ori == 1)
        assert n >= 100
    level0 = int((k2["octave"] == 0).sum())
    assert level0 > 4096
    dx = np.abs(k2["x"][None, :] - k1["x"][:, None]); dy = np.abs(k2["y"][None, :] - k1["y"][:, None])
    assert np.all((dx < 100) & (dy < 100))                                   # every slot inside every window


def test_chain_in_place_and_with_two_buffers(pkg, OM, mt, frames):
    """MonocularInitialization's use: prev_out of step k is prev_in of step k + 1.  In place (one buffer, as the reference) and through
    separate buffers, on the device, against the oracle's chain."""
    f0, f1, f2 = frames
    A = Pool(pkg, [f0], 29); B = Pool(pkg, [f1, f2], 31).build_grid(pkg.lib(), mt)
    prev0 = own_xy(f0[0]); n1 = len(prev0)
    _, _, prev1 = oracle_ref(pkg, OM, f0, f1, prev0, 100, 0.9, True)
    n2, m2, prev2 = oracle_ref(pkg, OM, f0, f2, prev1, ic.CHAIN_WINDOW, 0.9, True)
    n2s, m2s, prev2s, _ = second_reading_ref(f0, f2, prev1, ic.CHAIN_WINDOW, 0.9, True)
    assert n2s == n2 and np.array_equal(m2s, m2) and np.array_equal(prev2s, prev2)
    v0 = pkg.FrameView(f0[0], f0[1], ic.W, ic.H, backend=mt); v2 = pkg.FrameView(f2[0], f2[1], ic.W, ic.H, backend=mt)
    n2h, m2h, prev2h = mt.SearchForInitialization(v0, v2, prev1, ic.CHAIN_WINDOW, 0.9, True)
    assert n2h == n2 and np.array_equal(m2h, m2) and np.array_equal(prev2h, prev2)
    for in_place in (True, False):
        g1 = run(pkg, mt, A, B, [0], [0], [prev0], 100, 0.9, 1, in_place=in_place)
        check(pkg, OM, A, B, [0], [0], [prev0], 100, 0.9, 1, g1, in_place=in_place, mt=mt)
        g2 = run(pkg, mt, A, B, [0], [1], [g1[2][0, :n1]], ic.CHAIN_WINDOW, 0.9, 1, in_place=in_place)
        assert g2[1][0] == n2 and np.array_equal(g2[0][0, :n1], m2) and np.array_equal(g2[2][0, :n1], prev2)
    assert n2 > 100 and not np.array_equal(prev1, prev0)


def test_capture_and_three_replays(pkg, OM, mt, frames, synth):
    """After one eager call the same shape is captured behind an extraction (orbx_capture_begin records an extractor's step) and
    replayed three times with separate prev buffers: identical rows, counts and prev_out every time (nothing accumulates), and equal
    to the eager result."""
    L = pkg.lib()
    stride = (ic.W + 63) // 64 * 64
    pad = np.zeros((ic.H, stride), np.uint8); pad[:, :ic.W] = synth.gen_image(ic.W, ic.H, 1)
    dimg = pkg.DeviceBuffer(stride * ic.H).upload(pad)
    arr = (C.c_void_p * 1)(dimg.ptr)
    f0, f1, f2 = frames
    A = Pool(pkg, [f0, f1], 17); B = Pool(pkg, [f1, f2], 6700)         # cap2 > 8192: more than 32 KB of dynamic LDS under capture
    assert B.cap > 8192
    P = 2
    pin = np.zeros((P, A.cap, 2), np.float32); pin[0, :len(f0[0])] = own_xy(f0[0]); pin[1, :len(f1[0])] = own_xy(f1[0])
    dpi = pkg.DeviceBuffer(pin.nbytes).upload(pin); dpo = pkg.DeviceBuffer(pin.nbytes)
    mm = pkg.DeviceBuffer(4 * P * A.cap); nm = pkg.DeviceBuffer(4 * P)
    ex = pkg.ORBextractor(500, max_size=(ic.W, ic.H), max_batch=1)
    m2 = pkg.ORBmatcher(0.9)
    assert L.orbm_set_stream(m2.h, L.orbx_stream(ex.h)) == 0
    try:
        B.build_grid(L, m2)

        def enqueue():
            ex.enqueue_device(arr, ic.W, ic.H, stride, np.zeros(4, np.int32))
            assert getattr(L, NAME)(m2.h, P, A.n, A.cap, A.dk.ptr, A.dd.ptr, A.dc.ptr, B.n, B.cap, B.dk.ptr, B.dd.ptr, B.dc.ptr, B.gs.ptr, B.gi.ptr,
                                    0.0, 0.0, float(ic.INV_W), float(ic.INV_H), None, None, dpi.ptr, 100, 0.9, 1, mm.ptr, nm.ptr, dpo.ptr) == 0, L.orbm_last_error()

        def fetch():
            ex.sync()
            return mm.download(np.int32, P * A.cap).reshape(P, A.cap), nm.download(np.int32, P), dpo.download(np.float32, P * A.cap * 2)
        enqueue()
        eager = fetch()
        for p, (a, b) in enumerate(((f0, f1), (f1, f2))):
            n, m, pv = oracle_ref(pkg, OM, a, b, own_xy(a[0]), 100, 0.9, True)
            assert eager[1][p] == n and np.array_equal(eager[0][p, :len(m)], m)
        assert L.orbx_capture_begin(ex.h, 0) == 0, L.orbx_last_error()
        enqueue()
        assert L.orbx_capture_end(ex.h) == 0, L.orbx_last_error()
        for _ in range(3):
            mm.upload(np.full(P * A.cap, -7, np.int32)); nm.upload(np.full(P, -7, np.int32)); dpo.upload(np.full(P * A.cap * 2, SENT, np.float32))
            assert L.orbx_graph_launch(ex.h, 0) == 0, L.orbx_last_error()
            again = fetch()
            assert np.array_equal(again[0], eager[0]) and np.array_equal(again[1], eager[1])
            for p, k in enumerate((f0[0], f1[0])):
                lo, hi = p * A.cap * 2, p * A.cap * 2 + 2 * len(k)
                assert np.array_equal(again[2][lo:hi], eager[2][lo:hi])
    finally:
        assert L.orbm_set_stream(m2.h, None) == 0
        ex.close(); m2.close()


def test_refusals_enqueue_nothing(pkg):
    m = pkg.ORBmatcher()
    L = m.L
    p = pkg.DeviceBuffer(1 << 16).ptr
    out = pkg.DeviceBuffer(64).upload(np.full(16, 12345, np.int32))
    names = ["kps1", "desc1", "counts1", "kps2", "desc2", "counts2", "gs", "gi", "prev_in", "matches12", "nmatches", "prev_out"]

    def call(npairs=1, n1=1, c1=4, n2=1, c2=4, window=100, **null):
        a = {k: (None if k in null else (out.ptr if k in ("matches12", "nmatches", "prev_out") else p)) for k in names}
        return getattr(L, NAME)(m.h, npairs, n1, c1, a["kps1"], a["desc1"], a["counts1"], n2, c2, a["kps2"], a["desc2"], a["counts2"], a["gs"], a["gi"],
                                0.0, 0.0, 0.17, 0.2, None, None, a["prev_in"], window, 0.9, 1, a["matches12"], a["nmatches"], a["prev_out"])
    for k in names:
        assert call(**{k: 1}) == -2, k
    for kw in (dict(npairs=0), dict(n1=0), dict(n2=0), dict(c1=0), dict(c2=0), dict(window=-1)):
        assert call(**kw) == -2, kw
    assert call(c1=32769) == -3 and b"32768" in L.orbm_last_error()
    assert call(c2=32769) == -3 and call(npairs=65536) == -3
    m.sync()
    assert np.all(out.download(np.int32, 16) == 12345)
    m.close()
