"""The eight batched device searches against tests/second_reading.py directly (not through the oracle): one call each on a moderate
batch of gathered rows -- two extractor frames, an empty row, a constructed row that sits on the thresholds, and a repeated row --
with blocked / matched / good arrays set and the rotation check on where the search has one.  Where a device call projects on its
own (M5, M6, M13) the second reading gets the post-projection arrays the existing tests compute in numpy."""
import numpy as np
import pytest

import second_reading as sr
import test_gpu_fuse_batch as fu
import test_gpu_local_points_batch as lp
import test_gpu_motion_model_batch as mm
import test_gpu_reloc_batch as rl
import test_gpu_sim3_projection_batch as s3
import test_gpu_triangulation_batch as tr
from test_fuse_projection_cpu import fuse_project_np
from test_second_reading_cpu import M10_EP, M10_F12, M10_F12_ROW, M10_ROTATIONS, bow_case, m10_case, threshold_lattice

pytestmark = pytest.mark.gpu

F = np.float32
W, H, CAP = rl.W, rl.H, 1536
INV_W, INV_H = F(64) / F(W), F(48) / F(H)
LATTICE_ROW, EMPTY_ROW = 3, 2


@pytest.fixture(scope="module")
def rows(pkg, oracle, synth):
    """Host rows: extractor frames 0 and 1, an empty row, the threshold lattice, and row 0 again."""
    OM = oracle._oracle_matcher_class()()
    out = []
    for seed in (41, 42):
        _, k, d, _ = oracle.Extractor(1300)(synth.gen_image(W, H, seed), (0, 0))
        assert 1000 <= len(k) <= 1500
        out.append((k, d))
    L = threshold_lattice(oracle)
    L.W, L.H = W, H
    v, _, blocked, Q = L.arrays(pkg, OM, stereo=True)
    out = [out[0], out[1], (out[0][0][:0], out[0][1][:0]), (v.kps, v.desc), out[0]]
    return dict(rows=out, lattice=dict(ur=v.uright, blocked=blocked, Q=Q))


@pytest.fixture(scope="module")
def pool(pkg, rows):
    R = len(rows["rows"])
    kps = np.zeros((R, CAP), pkg.KP_DTYPE); desc = np.zeros((R, CAP, 32), np.uint8)
    for r, (k, d) in enumerate(rows["rows"]):
        for name in ("x", "y", "size", "angle", "response", "octave", "class_id"):
            kps[r, :len(k)][name] = k[name]
        desc[r, :len(k)] = d
    sf = np.cumprod(np.concatenate([[F(1)], np.full(7, F(1.2))]).astype(np.float32)).astype(np.float32)
    return rl.Pool(pkg, kps, desc, [len(k) for k, _ in rows["rows"]], sf)


def _grid(pool, r, ur=None):
    k, d = pool.row(r)
    return sr.GridFrame(k, d, 0.0, 0.0, INV_W, INV_H, None if ur is None else ur[:len(k)])


def _same_row(row, count, want, n, what):
    assert int(count) == int(want[0]), (what, int(count), int(want[0]))
    assert np.array_equal(row[:n], want[1][:n]), (what, np.flatnonzero(row[:n] != want[1][:n])[:8])
    assert np.all(row[n:] == -1), what


def _blocked(rng, R, cap):
    b = np.zeros((R, cap), np.uint8)
    b[1] = rng.random(cap) < 0.35; b[4] = rng.random(cap) < 0.97
    return b


def _uright(rng, pool, rows):
    ur = np.full((pool.R, pool.cap), -1, np.float32)
    for r in range(pool.R):
        k, _ = pool.row(r)
        ur[r, :len(k)] = np.where(rng.random(len(k)) < 0.6, k["x"] - rng.uniform(2, 40, len(k)), -1)
    ur[LATTICE_ROW, :len(rows["lattice"]["ur"])] = rows["lattice"]["ur"]
    return ur


def test_m3_points(pkg, pool, rows):
    rng = np.random.default_rng(3)
    th, nnratio = 1.0, 0.9
    lat = rows["lattice"]; LQ = lat["Q"]
    Q = []
    for r in range(pool.R):
        k, d = pool.row(r)
        if r == LATTICE_ROW:
            Q.append(dict(in_view=LQ["valid"], px=LQ["x"], py=LQ["y"], pxr=LQ["pxr"], view_cos=LQ["view_cos"], level=LQ["level"], qdesc=LQ["desc"],
                          mp_obs=LQ["obs"], depth=np.ones(len(LQ["x"]), np.float32)))
        else:
            src = pool.row(0) if len(k) == 0 else (k, d)
            q = lp._queries(rng, *src, 1200, jitter=1.0)
            q["mp_obs"] = (rng.random(1200) < 0.6).astype(np.uint8)
            Q.append(q)
    blocked = _blocked(rng, pool.R, pool.cap); blocked[LATTICE_ROW, :len(lat["blocked"])] = lat["blocked"]
    ur = _uright(rng, pool, rows)
    R_ = lp._Rows(pkg, pool.R, 1300); R_.upload(Q)
    dm = pkg.DeviceBuffer(pool.R * pool.cap * 4); dn = pkg.DeviceBuffer(pool.R * 4)
    r = dict(kps=pool.dk.ptr, desc=pool.dd.ptr, counts=pool.dc.ptr)
    rc = lp._call(pool.L, pool.m, r, pool.cap, pool.gs, pool.gi, 0, R_, pool.sf, th, nnratio, dm, dn, uright=rl._dev(pkg, ur), blocked=rl._dev(pkg, blocked))
    assert rc == 0, pool.L.orbm_last_error()
    pool.m.sync()
    match = dm.download(np.int32, pool.R * pool.cap).reshape(pool.R, pool.cap); nm = dn.download(np.int32, pool.R)
    total = 0
    for f in range(pool.R):
        n = int(pool.counts[f]); q = Q[f]
        if n == 0:
            assert nm[f] == 0 and np.all(match[f] == -1)
            continue
        want = sr.search_by_projection_points(_grid(pool, f, ur[f]), blocked[f, :n], pool.sf, q["in_view"], q["px"], q["py"], q["pxr"], q["view_cos"],
                                              q["level"], q["qdesc"], q["mp_obs"], th, nnratio)
        _same_row(match[f], nm[f], want, n, "M3 row %d" % f)
        total += want[0]
        if f == LATTICE_ROW:
            for key in ("dist_on_th_high", "dist_on_th_high_plus_1", "ratio_exactly_equal", "ratio_rejected", "ratio_bypassed_by_level",
                        "overwrote_unobserved", "all_candidates_blocked", "exactly_r_away", "stereo_gate_rejected"):
                assert want[2][key] > 0, key
    assert total > 500


def test_m4_frame_with_retry(pkg, pool, rows):
    rng = np.random.default_rng(4)
    th = 7.0
    lat = rows["lattice"]; LQ = lat["Q"]
    Q = []
    for r in range(pool.R):
        k, d = pool.row(r)
        if r == LATTICE_ROW:
            Q.append(dict(valid=LQ["valid"], u=LQ["x"], v=LQ["y"], invzc=LQ["invzc"], octave=LQ["level"], angle=LQ["angle"], qdesc=LQ["desc"], mp_obs=LQ["obs"]))
        else:
            src = pool.row(0) if len(k) == 0 else (k, d)
            q = mm._queries(rng, *src, 1200)
            q["mp_obs"] = (rng.random(1200) < 0.6).astype(np.uint8)
            Q.append(q)
    blocked = _blocked(rng, pool.R, pool.cap); blocked[LATTICE_ROW, :len(lat["blocked"])] = lat["blocked"]
    ur = _uright(rng, pool, rows)
    R_ = mm._Rows(pkg, pool.R, 1300); R_.upload(Q, dirs=[0, 1, 0, 0, 2])
    dm = pkg.DeviceBuffer(pool.R * pool.cap * 4); dn = pkg.DeviceBuffer(pool.R * 4); dr = pkg.DeviceBuffer(8)
    r = dict(kps=pool.dk.ptr, desc=pool.dd.ptr, counts=pool.dc.ptr)
    rc = mm._call(pool.L, pool.m, r, pool.cap, pool.gs, pool.gi, 0, R_, pool.sf, th, dm, dn, uright=rl._dev(pkg, ur), mbf=mm.MBF,
                  blocked=rl._dev(pkg, blocked), retry_below=20, retried=dr, check_ori=True)
    assert rc == 0, pool.L.orbm_last_error()
    pool.m.sync()
    match = dm.download(np.int32, pool.R * pool.cap).reshape(pool.R, pool.cap); nm = dn.download(np.int32, pool.R)
    retried = dr.download(np.uint8, pool.R)
    total = pruned = 0
    for f in range(pool.R):
        n = int(pool.counts[f]); q = Q[f]
        if n == 0:
            assert nm[f] == 0 and np.all(match[f] == -1)
            continue
        want = sr.search_by_projection_frame_with_retry(_grid(pool, f, ur[f]), blocked[f, :n], pool.sf, q["valid"], q["u"], q["v"], q["invzc"], q["octave"],
                                                        q["angle"], q["qdesc"], q["mp_obs"], th, forward=(f == 1), backward=(f == 4), mbf=mm.MBF,
                                                        check_ori=True, retry_below=20)
        _same_row(match[f], nm[f], want, n, "M4 row %d" % f)
        assert bool(retried[f]) == want[3], f
        total += want[0]; pruned += int((want[1] == sr.PRUNED).sum())
    assert total > 500 and pruned > 0 and retried.any() and not retried.all()


def _pairs(rng, pool, make, key):
    """Pairs on rows 0, 1, the empty row, the lattice row's neighbours and row 0 twice more, with blocked fractions 0 / 0.35 / 0.97."""
    pairs = []
    for row, frac in ((0, 0.0), (1, 0.35), (EMPTY_ROW, 0.0), (0, 0.97), (4, 0.35), (0, 0.0)):
        src_row = 0 if pool.counts[row] == 0 else row
        p = make(rng, pool, src_row, 1100)
        p.update(row=row)
        p[key] = (rng.random(pool.cap) < frac).astype(np.uint8)
        pairs.append(p)
    return pairs


def test_m5_kf(pkg, pool):
    rng = np.random.default_rng(5)
    th, orb_dist = 10.0, 100
    pairs = _pairs(rng, pool, rl.keyframe, "blocked")
    call = rl.Call(pool, pairs, rng=rng)
    match, nm = call.run(th, orb_dist, True)
    total = pruned = 0
    for i, p in enumerate(pairs):
        n = int(pool.counts[p["row"]])
        if n == 0:
            assert nm[i] == 0 and np.all(match[i] == -1)
            continue
        ok, u, v, lvl = rl.proj_of(pool, p)
        want = sr.search_by_projection_kf(_grid(pool, p["row"]), p["blocked"][:n], pool.sf, ok, u, v, np.maximum(lvl, 0), p["angle"], p["qdesc"], th, orb_dist, True)
        _same_row(match[i], nm[i], want, n, "M5 pair %d" % i)
        total += want[0]; pruned += int((want[1] == sr.PRUNED).sum())
        if i == 3:
            assert want[2]["all_candidates_blocked"] > 0
    assert total > 300 and pruned > 0


@pytest.mark.parametrize("form", [0, 1])
def test_m6_sim3(pkg, pool, form):
    rng = np.random.default_rng(6 + form)
    th, ratio = 8, 1.5
    pairs = _pairs(rng, pool, s3.mappoints, "matched")
    call = s3.Call(pool, pairs, rng=rng)
    match, nm = call.run(th, ratio, form)
    total = 0
    for i, p in enumerate(pairs):
        n = int(pool.counts[p["row"]])
        if n == 0:
            assert nm[i] == 0 and np.all(match[i] == -1)
            continue
        ok, u, v, lvl = s3.proj_of(pool, p, form)
        want = sr.search_by_projection_sim3(_grid(pool, p["row"]), p["matched"][:n], pool.sf, ok, u, v, np.maximum(lvl, 0), p["qdesc"], th, ratio)
        _same_row(match[i], nm[i], want, n, "M6 pair %d" % i)
        total += want[0]
        if i == 3:
            assert want[2]["all_candidates_blocked"] > 0
    assert total > 300


@pytest.mark.parametrize("chi2", [1, 0])
def test_m13_fuse(pkg, pool, rows, chi2):
    assert np.array_equal(fu.KCAM, rl.KCAM) and fu.NLEV == pool.nlev and (fu.W, fu.H) == (W, H)
    rng = np.random.default_rng(13 + chi2)
    th, NQ = 3.0, 1100
    ur = _uright(rng, pool, rows)
    S = fu.Scenes.gathered(pkg, pool.m, pool.dk.ptr, pool.dd.ptr, pool.R, pool.cap, pool.gs, pool.gi, pool.sf, F(1) / (pool.sf * pool.sf), ur)
    kf_rows = [0, 1, EMPTY_ROW, 4, 0]
    ps = [s3.mappoints(rng, pool, 0 if pool.counts[r] == 0 else r, NQ, maxflip=20) for r in kf_rows]
    st = lambda key: np.stack([p[key] for p in ps])
    tcw, ow, valid = st("tcw"), st("ow"), st("valid")
    c = fu.Call(S, kf_rows, tcw, ow, np.full(len(ps), NQ, np.int32), valid, st("pw"), st("normal"), st("mn"), st("mx"), st("qdesc"), False)
    best, nf, _ = c.run(th, chi2, True)
    ok, u, v, pur, lvl = fuse_project_np(tcw, ow, st("pw"), st("normal"), st("mn"), st("mx"), valid, fu.KCAM, fu.BOUNDS, fu.BF, fu.LOG_SF, fu.NLEV)
    total = 0
    for i, r in enumerate(kf_rows):
        n = int(pool.counts[r])
        if n == 0:
            assert nf[i] == 0 and np.all(best[i] == -1)
            continue
        want = sr.fuse(_grid(pool, r, ur[r]), pool.sf, S.isg, ok[i], u[i], v[i], pur[i], np.maximum(lvl[i], 0), ps[i]["qdesc"], th, bool(chi2))
        assert int(nf[i]) == want[0] and np.array_equal(best[i, :NQ], want[1]) and np.all(best[i, NQ:] == -1), ("M13 pair", i)
        total += want[0]
        if chi2:
            assert want[2]["chi2_stereo"] > 0 and want[2]["chi2_mono"] > 0 and want[2]["chi2_rejected"] > 0
    assert total > 200


# ---- BoW searches: pools laid out by the test, node = low bits of the first descriptor byte or given ---------------------------------
def _bow_pools(pkg, oracle, rows, rng, bits=4):
    """Pool 1: row 0, row 1, empty, the constructed side 1; pool 2: row 0 (a frame against itself), row 1, empty, the constructed side 2."""
    K1, D1, N1, K2, D2, N2 = bow_case(oracle)
    base = rows["rows"]
    k0 = base[0][0].copy()                                   # the frame against itself, its angles spread over five rotation bins
    k0["angle"] = np.mod(k0["angle"] + rng.choice([0.0, 20.0, 80.0, 200.0, 300.0], len(k0), p=[.6, .2, .1, .05, .05]), 360)
    r1 = [base[0], base[1], base[2], (K1, D1)]; r2 = [(k0, base[0][1]), base[1], base[2], (K2, D2)]
    g1 = [(rng.random(len(k)) < 0.8).astype(np.uint8) for k, _ in r1]; g2 = [(rng.random(len(k)) < 0.8).astype(np.uint8) for k, _ in r2]
    g1[3][:] = 1; g2[3][:] = 1
    A = tr.Pool(pkg, r1, CAP, bits, mp=g1); B = tr.Pool(pkg, r2, CAP + 64, bits, mp=g2)
    A.node[3, :len(N1)] = N1; B.node[3, :len(N2)] = N2
    A.upload(); B.upload()
    return A, B


def _bow_run(pkg, mt, name, A, B, row1, row2, nnratio, check_ori, out_cap):
    L = pkg.lib(); P = len(row1)
    d1 = rl._dev(pkg, np.asarray(row1, np.int32)); d2 = rl._dev(pkg, np.asarray(row2, np.int32))
    mm_ = pkg.DeviceBuffer(4 * P * out_cap).upload(np.full(P * out_cap, -7, np.int32)); nm = pkg.DeviceBuffer(4 * P).upload(np.full(P, -7, np.int32))
    a = A.args()[:8]; b = B.args()[:8] if name.endswith("kf_batch_async") else B.args()[:7]
    rc = getattr(L, name)(mt.h, P, *a, *b, d1.ptr, d2.ptr, float(nnratio), int(check_ori), mm_.ptr, nm.ptr)
    assert rc == 0, L.orbm_last_error()
    assert L.orbm_sync(mt.h) == 0
    return mm_.download(np.int32, P * out_cap).reshape(P, out_cap), nm.download(np.int32, P)


PAIRS_1 = [0, 1, 0, 2, 3, 0, 1]          # a frame against itself, an unrelated pair, empty rows, the constructed pair, a repeated row
PAIRS_2 = [0, 0, 1, 1, 3, 2, 1]


def test_m7_bow(pkg, oracle, rows):
    rng = np.random.default_rng(7)
    mt = pkg.ORBmatcher(0.7)
    A, B = _bow_pools(pkg, oracle, rows, rng)
    nnratio = 0.6
    got, nm = _bow_run(pkg, mt, "orbm_search_by_bow_batch_async", A, B, PAIRS_1, PAIRS_2, nnratio, 1, B.cap)
    total = culled = 0
    for p, (r1, r2) in enumerate(zip(PAIRS_1, PAIRS_2)):
        k1, d1, n1, keep1, good1, _ = A.host(r1); k2, d2, n2, keep2, _, _ = B.host(r2)
        if len(k1) == 0 or len(k2) == 0:
            assert nm[p] == 0 and np.all(got[p] == -1)
            continue
        want = sr.search_by_bow(k1, d1, good1, tr.fv(n1, keep1), k2, d2, tr.fv(n2, keep2), nnratio, True)
        _same_row(got[p], nm[p], want, len(k2), "M7 pair %d" % p)
        total += want[0]; culled += want[2]["culled_entries"]
        if r1 == 3:
            for key in ("accepted_on_th_low", "dist_on_th_low_plus_1", "runner_up_equals_best", "ratio_rejected"):
                assert want[2][key] > 0, key
    assert total > 300 and culled > 0


def test_m8_bow_kf(pkg, oracle, rows):
    rng = np.random.default_rng(8)
    mt = pkg.ORBmatcher(0.9)
    A, B = _bow_pools(pkg, oracle, rows, rng)
    nnratio = 0.6
    got, nm = _bow_run(pkg, mt, "orbm_search_by_bow_kf_batch_async", A, B, PAIRS_1, PAIRS_2, nnratio, 1, A.cap)
    total = culled = 0
    for p, (r1, r2) in enumerate(zip(PAIRS_1, PAIRS_2)):
        k1, d1, n1, keep1, good1, _ = A.host(r1); k2, d2, n2, keep2, good2, _ = B.host(r2)
        if len(k1) == 0 or len(k2) == 0:
            assert nm[p] == 0 and np.all(got[p] == -1)
            continue
        want = sr.search_by_bow_kf(k1, d1, good1, tr.fv(n1, keep1), k2, d2, good2, tr.fv(n2, keep2), nnratio, True)
        _same_row(got[p], nm[p], want, len(k1), "M8 pair %d" % p)
        total += want[0]; culled += want[2]["culled_entries"]
        if r1 == 3:
            for key in ("rejected_on_th_low", "dist_on_th_low_plus_1", "runner_up_equals_best", "ratio_rejected", "skipped_claimed_side2"):
                assert want[2][key] > 0, key
    assert total > 300 and culled > 0


def test_m10_triangulation(pkg, oracle, rows, monkeypatch):
    rng = np.random.default_rng(10)
    mt = pkg.ORBmatcher(0.6)
    base = rows["rows"]
    K1, D1, N1, U1, K2, D2, N2, U2 = m10_case(oracle)
    # pool 1's row 0 is frame 0 with its angles turned by M10_ROTATIONS; pool 2's row 0 is frame 0 moved down by 0.75 px
    ka = base[0][0].copy(); ka["angle"] = np.mod(ka["angle"] + rng.choice(M10_ROTATIONS[0], len(ka), p=M10_ROTATIONS[1]), 360)
    kb = base[0][0].copy(); kb["y"] += F(0.75)
    r1 = [(ka, base[0][1]), base[1], base[2], (K1, D1)]; r2 = [(kb, base[0][1]), base[1], base[2], (K2, D2)]
    mp1 = [(rng.random(len(k)) < 0.3).astype(np.uint8) for k, _ in r1]; mp2 = [(rng.random(len(k)) < 0.3).astype(np.uint8) for k, _ in r2]
    u1 = [np.where(rng.random(len(k)) < 0.5, 5.0, -1.0).astype(np.float32) for k, _ in r1]; u2 = [np.where(rng.random(len(k)) < 0.5, 5.0, -1.0).astype(np.float32) for k, _ in r2]
    mp1[3][:] = 0; mp2[3][:] = 0; u1[3] = U1; u2[3] = U2
    A = tr.Pool(pkg, r1, CAP, 3, mp=mp1, ur=u1); B = tr.Pool(pkg, r2, CAP + 64, 3, mp=mp2, ur=u2)
    A.node[3, :len(N1)] = N1; B.node[3, :len(N2)] = N2
    A.upload(); B.upload()
    row1 = [0, 1, 0, 2, 0, 3, 3]; row2 = [0, 0, 1, 1, 0, 3, 3]
    Fs = np.stack([M10_F12] * 6 + [M10_F12_ROW])
    ep = np.array([[W * 0.5, H * 0.5]] * 5 + [M10_EP] * 2, np.float32)
    sf, sig = tr.levels()
    got, nm = tr.run(pkg, mt, A, B, row1, row2, Fs, ep, sf, sig, check_ori=1)
    total = culled = 0
    for p, (a, b) in enumerate(zip(row1, row2)):
        k1, d1, n1, keep1, m1, ur1 = A.host(a); k2, d2, n2, keep2, m2, ur2 = B.host(b)
        if len(k1) == 0 or len(k2) == 0:
            assert nm[p] == 0 and np.all(got[p] == -1)
            continue
        args = (k1, d1, m1, ur1, tr.fv(n1, keep1), k2, d2, m2, ur2, tr.fv(n2, keep2), Fs[p], ep[p], sf, sig, False, False, True)
        want = sr.search_for_triangulation(*args)
        _same_row(got[p], nm[p], want, len(k1), "M10 pair %d" % p)
        total += want[0]; culled += want[2]["culled_entries"]
        t = want[2]
        if p == 0:
            assert t["epipolar_pass"] > 0 and t["epipole_gate_applied"] > 0 and t["epipole_gate_skipped_stereo"] > 0 and t["culled_entries"] > 0
            with monkeypatch.context() as mp:                    # the other searches' factor would cull another set: the row pins 1.0f/30
                mp.setattr(sr, "FACTOR_INV", sr.FACTOR_360)
                other = sr.search_for_triangulation(*args)
            assert other[0] < want[0] and not np.array_equal(other[1], want[1])
        if p == 5:
            for key in ("tie_goes_to_later", "epipolar_pass", "epipolar_fail", "dist_on_th_low", "epipole_gate_rejected", "idx2_shared"):
                assert t[key] > 0, key
        if p == 6:
            assert t["double_product_decides"] > 0 and want[1][9] == int(np.nonzero(N2 == 8)[0][0])
    assert total > 100 and culled > 0
