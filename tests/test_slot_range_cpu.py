"""tests/slot_range_cases.py is what it claims to be, shown from the second reading alone (no GPU): every planted situation is reached,
the accepted matches lie on the upper half of the slot range, the queries left out for the PredictScale caveat are few, the oracle
agrees with the second reading on every case, and the reference side is quick.  tests/test_gpu_slot_range.py compares the device
calls with exactly these rows, so a case that missed its situation would let a kernel fault pass there: the conditions are asserted
here."""
import time

import numpy as np
import pytest

import second_reading as sr
import slot_range_cases as sc

TOP, HALF = sc.CAP_TOP, sc.HALF
SEARCHES = ("m3", "m4", "m3fe", "m4fe", "m5", "m6", "m13")     # m3fe, m4fe: the two-camera forms, each camera's row a unit of its own
OVERWRITING = {"m3": "overwrote_unobserved", "m4": "overwrote_unobserved", "m3fe": "overwrote", "m4fe": "overwrote"}


@pytest.fixture(scope="module")
def cases():
    t0 = time.perf_counter()
    out = {}
    for cap in (sc.CAP_TOP, sc.CAP_HALF):
        sc.pool(cap).csr()
        out["m3", cap] = sc.m3_case(cap); out["m4", cap] = sc.m4_case(cap); out["m5", cap] = sc.m5_case(cap)
        out["m6", cap] = sc.m6_case(cap); out["m13", cap] = sc.m13_case(cap)
        out["m3fe", cap] = sc.m3_fisheye_case(cap); out["m4fe", cap] = sc.m4_fisheye_case(cap); out["m10", cap] = sc.m10_case(cap)
    out["m5", "12 levels"] = sc.m5_case(sc.CAP_TOP, 12)
    sc.tiny_kinds()
    for n in sc.GRID_SIZES:
        sc.grid_want(sc.grid_points(n))
    out["seconds"] = time.perf_counter() - t0
    return out


def _units(case):
    """(row, blocked variant, query dict, want) per frame or pair of a case."""
    if "frames" in case:
        return [(r, v, q, w) for (r, v), q, w in zip(case["frames"], case["Q"], case["want"])]
    hp = case["hp"]
    if "layout" in case:
        first_l, first_r, npairs = case["layout"]
        out = []
        for p, (q, (n, ml, mr, t)) in enumerate(zip(case["Q"], case["want"])):
            out.append((first_l + p, False, dict(planted_at=q["planted_l"]), (n, ml, t)))
            out.append((first_r + p, first_r + p == hp.R - 1, dict(planted_at=q["planted_r"]), (n, mr, t) if hp.n(first_r + p) else None))
        return out
    variants = {id(p): bool(np.any(p.get("blocked", p.get("matched", p.get("unused")))[hp.plants[p["row"]]["blocked"]])) if p["row"] in hp.plants else False
                for p in case["pairs"]}
    return [(p["row"], variants[id(p)], p, w) for p, w in zip(case["pairs"], case["want"])]


def _slot_of(name, want, q):
    """The slot query q ended on: its entry in M13's per-query row, else the slot of the row that names it (-1: none)."""
    if name == "m13":
        return int(want[1][q])
    hit = np.flatnonzero(want[1] == q)
    assert len(hit) <= 1
    return int(hit[0]) if len(hit) else -1


def test_the_reference_side_is_quick(cases):
    assert cases["seconds"] < 30, cases["seconds"]


def test_pool_layout():
    for cap, counts in ((sc.CAP_TOP, [65535, 32769, 32768, 0, 70000, 65535]), (sc.CAP_HALF, [32769, 32768, 0, 32769])):
        hp = sc.pool(cap)
        assert hp.kps.shape == (len(counts), cap) and hp.desc.shape == (len(counts), cap, 32) and list(hp.counts) == counts
        assert np.array_equal(hp.kps[-1], hp.kps[0]) and np.array_equal(hp.desc[-1], hp.desc[0])          # one row repeated
        for r in range(hp.R):                                                                              # past the count: plausible keypoints
            assert np.all(hp.kps[r]["x"] > 0) and np.all(hp.desc[r].reshape(cap, 32).any(1))
        gs, gi, placed = hp.csr()
        assert 0.97 * cap < placed[0] <= cap and gi[0].max() == cap - 1    # (a keypoint that rounds onto column 64 / row 48 is not placed)
    hp = sc.pool(sc.CAP_TOP)
    a, b, _ = hp.plants[0]["tie"]
    _, gi, _ = hp.csr()
    assert gi[0, HALF - 1] == a and gi[0, HALF] == b                       # the tied pair straddles grid position 32768
    last_word = [s for s in hp.plants[0]["blocked"] if s >= (TOP - 1) // 32 * 32]
    assert len(last_word) >= 9 and all(HALF <= s < HALF + 32 for s in hp.plants[0]["word1024"]) and len(hp.plants[0]["word1024"]) == 2
    assert sc.pool(sc.CAP_TOP, 12).nlev == 12 and sc.pool(sc.CAP_TOP, 12).kps["octave"].max() == 11


@pytest.mark.parametrize("name,cap", [(name, cap) for name in SEARCHES for cap in (sc.CAP_TOP, sc.CAP_HALF)] + [("m5", "12 levels")])
def test_planted_situations_are_reached(cases, name, cap):
    case = cases[name, cap]
    hp = case["hp"]
    seen = set()
    for r, variant, q, want in _units(case):
        P = hp.plants.get(r)
        if P is None or want is None:
            continue
        n = P["n"]
        at = q["planted_at"]
        qi = lambda what: sc.planted(P, at, what)
        seen.add((n, variant))
        tops = dict(zip(P["top"], qi("top")))
        blocked = variant and name != "m13"                                 # Fuse has no blocked array
        for s, i in tops.items():                                           # the unique best at n-1, n-2, 32768, 32767 and 0
            if s == n - 1 and blocked:
                assert _slot_of(name, want, i) == P["runner"], (name, r, "blocked best: the runner-up")
                assert name == "m13" or want[1][s] == -1
            else:
                assert _slot_of(name, want, i) == s, (name, r, s)
        c = qi("cluster")[0]                                                # more than TK_K candidates; blocked: the eight listed ones are all blocked
        assert len(P["cluster"]) > sc.TK_K
        assert _slot_of(name, want, c) == (P["cluster"][sc.TK_K] if blocked else P["cluster"][0]), (name, r, "cluster")
        for s, i in zip(P["word1024"], qi("word1024")):                     # blocked bits in bitmap word 1024
            assert HALF <= s < HALF + 32
            assert _slot_of(name, want, i) == (-1 if blocked else s), (name, r, s)
        if blocked:                                                         # ... and in the last word
            assert all(want[1][s] == -1 for s in P["blocked"])
        if n == TOP:                                                        # two queries on one slot >= 32768: the search's own rule
            g8, fa, fb = qi("shared8"), qi("shared64a")[0], qi("shared64b")[0]
            assert g8[0] // 8 == g8[1] // 8 and fa // 64 != fb // 64 and min(P["shared"]) >= HALF
            if name == "m13":                                               # no claims: both fuse into it
                assert [_slot_of(name, want, i) for i in g8 + [fa, fb]] == [P["shared"][0]] * 2 + [P["shared"][1]] * 2
            elif name in OVERWRITING:                                       # the first MapPoint of the pair has no observations: overwritten
                assert want[1][P["shared"][0]] == g8[1] and want[1][P["shared"][1]] == fa and want[2][OVERWRITING[name]] > 0
            else:                                                           # every claim holds: first come
                assert want[1][P["shared"][0]] == g8[0] and want[1][P["shared"][1]] == fa
        if P["tie"]:                                                        # equal distances either side of grid position 32768: the first visited
            a, b, _ = P["tie"]
            assert _slot_of(name, want, qi("tie")[0]) == a, (name, r, "tie")
    # every planted row was met plain and in its blocked variant (M13 has no blocked array: its second unit on the row repeats the plain one)
    assert seen >= {TOP: {(TOP, False), (TOP, True), (sc.CAP_HALF, False)}, sc.CAP_HALF: {(sc.CAP_HALF, False), (sc.CAP_HALF, True)},
                    "12 levels": {(TOP, False), (TOP, True)}}[cap]


@pytest.mark.parametrize("name", SEARCHES)
def test_matches_lie_on_the_upper_half(cases, name):
    case = cases[name, sc.CAP_TOP]
    high = total = 0
    on = set()
    for r, _, q, want in _units(case):
        if want is None:
            continue
        slots = want[1][want[1] >= 0] if name == "m13" else np.flatnonzero(want[1] >= 0)
        high += int((slots >= HALF).sum()); total += len(slots)
        on |= set(int(s) for s in slots if s in (TOP - 1, HALF))
    assert total > 3000 and high >= 0.25 * total, (name, high, total)
    assert on == {TOP - 1, HALF}, (name, on)
    if name in ("m4", "m4fe", "m5"):                                              # matches on slots >= 32768 in a culled rotation bin are cleared
        culled = sum(int((w[1][HALF:] == sr.PRUNED).sum()) for _, _, _, w in _units(case) if w is not None)
        assert culled > 0


@pytest.mark.parametrize("cap", [sc.CAP_TOP, sc.CAP_HALF])
def test_m10_case(cases, cap):
    c = cases["m10", cap]
    n, (count, m12, t) = c["n"], c["want"]
    assert n == cap and all(m12[s] == s for s in c["own"]) and {n - 1, HALF, HALF - 1} <= set(c["own"])
    q, lo, hi = c["tie"]                                                    # equal distance at slots 3 and n-1: the last listed wins
    assert m12[q] == hi == n - 1 and lo == 3 and t["tie_goes_to_later"] > 0 and t["idx2_shared"] > 0
    assert np.array_equal(sr.descriptor_distances(c["d1"][q], c["d2"][[lo, hi]]), [6, 6])
    for s in c["taken"]:                                                    # the partner carries a MapPoint: another feature or none
        assert c["mp2"][s] and not c["mp1"][s] and m12[s] != s
    assert c["taken"][0] >= (n - 1) // 32 * 32 - 32 and (cap != TOP or HALF <= c["taken"][1] < HALF + 32)
    active = np.flatnonzero(c["mp1"] == 0)
    assert len(active) < 0.1 * n and (active >= n // 2).mean() > 0.8      # most slots carry a MapPoint; the active ones are few and high
    nodes = np.unique(c["node"])
    assert len(np.unique(nodes & 255)) < len(nodes)                         # node ids that share their low byte
    assert count > 1000 and t["culled_entries"] > 0 and t["epipolar_fail"] > 0
    if cap == TOP:
        hit = m12[m12 >= 0]
        assert (hit >= HALF).mean() >= 0.25 and (np.flatnonzero(m12 >= 0) >= HALF).mean() >= 0.25


def test_few_queries_are_left_out(cases):
    for name in ("m5", "m6", "m13"):
        for cap in (sc.CAP_TOP, sc.CAP_HALF):
            pairs = cases[name, cap]["pairs"]
            assert sum(p["excluded"] for p in pairs) <= 0.01 * sum(len(p["valid"]) for p in pairs), (name, cap)
    hp, kinds = sc.tiny_kinds()
    assert sum(p["excluded"] for p in kinds) <= 1


def test_grid_keypoint_sets():
    for n in (8193, 65535):
        s, i, t = sc.grid_want(sc.grid_points(n))
        assert t["half_way_cell"] > 0 and t["rounded_onto_edge"] > 0 and t["not_placed"] > t["rounded_onto_edge"] and len(i) == n - t["not_placed"]
        k = sc.grid_points(n)
        assert (k["x"] < -15).any() and (k["y"] < -12).any()               # negative cells
    s, i, _ = sc.grid_want(sc.grid_points(65535, crowded=True))
    s2, i2, _ = sc.grid_want(sc.grid_points(65535, crowded="several"))       # cells of exactly 64, 65, 100 and 700, all on the upper half
    for (cx, cy), count in sc.LONG_CELLS:
        cell = cx * 48 + cy
        assert s2[cell + 1] - s2[cell] == count and i2[s2[cell]:s2[cell + 1]].min() >= HALF - 1
    assert int((np.diff(s2) > 64).sum()) == 3 and sorted(c for _, c in sc.LONG_CELLS)[:2] == [64, 65]
    c = int(np.argmax(np.diff(s)))                                          # one cell of 2048 high slots, the rest sparse
    assert np.diff(s).max() >= 2048 and np.sort(np.diff(s))[-2] < 64 and int((i[s[c]:s[c + 1]] > HALF).sum()) >= 2048


# ---- the oracle agrees with the second reading on these cases ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def OM(oracle):
    return oracle._oracle_matcher_class()()


def _same(got, want, what):
    assert int(got[0]) == int(want[0]) and np.array_equal(np.asarray(got[1]), want[1]), what


@pytest.mark.parametrize("cap", [sc.CAP_TOP, sc.CAP_HALF])
def test_oracle_agrees(pkg, OM, cases, cap):
    hp = sc.pool(cap)
    views = {}

    def view(r):
        if r not in views:
            k, d = hp.row(r)
            views[r] = pkg.FrameView(np.ascontiguousarray(k).view(pkg.KP_DTYPE), d, sc.W, sc.H, backend=OM)
            s, i = hp.grid(r).csr()
            assert np.array_equal(views[r].grid_start, s) and np.array_equal(views[r].grid_idx[:len(i)], i)
        return views[r]

    z = np.zeros(sc.NQ, np.float32)
    for (r, _), q, b, want in zip(cases["m3", cap]["frames"], cases["m3", cap]["Q"], cases["m3", cap]["blocked"], cases["m3", cap]["want"]):
        if want is not None:
            _same(OM.SearchByProjectionPoints(view(r), blocked=b[:hp.n(r)], scale_factors=hp.sf, in_view=q["valid"], px=q["u"], py=q["v"], pxr=z,
                                              view_cos=q["view_cos"], level=q["level"], qdesc=q["desc"], mp_obs=q["mp_obs"], th=sc.M3_TH,
                                              nnratio=sc.M3_NNRATIO), want, ("M3", r))
    for (r, _), q, b, want in zip(cases["m4", cap]["frames"], cases["m4", cap]["Q"], cases["m4", cap]["blocked"], cases["m4", cap]["want"]):
        if want is not None:
            _same(OM.SearchByProjectionFrame(view(r), cur_blocked=b[:hp.n(r)], scale_factors=hp.sf, valid=q["valid"], u=q["u"], v=q["v"],
                                             invzc=q["invzc"], octave=q["level"], angle=q["angle"], qdesc=q["desc"], mp_obs=q["mp_obs"], th=sc.M4_TH,
                                             check_ori=True), want, ("M4", r))
    for p, want in zip(cases["m5", cap]["pairs"], cases["m5", cap]["want"]):
        if want is not None:
            ok, u, v, lvl = sc.proj_m5(hp, p)
            _same(OM.SearchByProjectionKF(view(p["row"]), blocked=p["blocked"][:hp.n(p["row"])], scale_factors=hp.sf, valid=ok, u=u, v=v,
                                          level=np.maximum(lvl, 0), angle=p["angle"], qdesc=p["qdesc"], th=sc.M5_TH, orb_dist=sc.M5_ORB_DIST,
                                          check_ori=True), want, ("M5", p["row"]))
    for p, want in zip(cases["m6", cap]["pairs"], cases["m6", cap]["want"]):
        if want is not None:
            ok, u, v, lvl = sc.proj_m6(hp, p, 0)
            _same(OM.SearchByProjectionSim3(view(p["row"]), matched_in=p["matched"][:hp.n(p["row"])], scale_factors=hp.sf, valid=ok, u=u, v=v,
                                            level=np.maximum(lvl, 0), qdesc=p["qdesc"], th=sc.M6_TH, ratio_hamming=sc.M6_RATIO), want, ("M6", p["row"]))
    for p, want in zip(cases["m13", cap]["pairs"], cases["m13", cap]["want"]):
        if want is not None:
            ok, u, v, ur, lvl = sc.proj_m13(hp, p)
            _same(OM.Fuse(view(p["row"]), scale_factors=hp.sf, inv_sigma2=cases["m13", cap]["isg"], valid=ok, u=u, v=v, ur=ur, level=np.maximum(lvl, 0),
                          qdesc=p["qdesc"], th=sc.M13_TH, chi2_gate=True), want, ("M13", p["row"]))


@pytest.mark.parametrize("cap", [sc.CAP_TOP, sc.CAP_HALF])
def test_oracle_agrees_m10_and_two_camera_forms(pkg, OM, cases, cap):
    from test_triangulation_batch_rule_cpu import ref_pair
    c = cases["m10", cap]
    keep = np.ones(c["n"], bool)
    k1, k2 = (np.ascontiguousarray(k).view(pkg.KP_DTYPE) for k in (c["k1"], c["k2"]))
    _same(ref_pair(OM, k1, c["d1"], c["node"], keep, c["mp1"], None, k2, c["d2"], c["node"], keep, c["mp2"], None, sc.M10_F12, sc.M10_EP, c["sf"],
                   c["sigma2"], False, False, True), c["want"], "M10")
    hp = sc.pool(cap)
    view = lambda r: pkg.FrameView(np.ascontiguousarray(hp.row(r)[0]).view(pkg.KP_DTYPE), hp.row(r)[1], sc.W, sc.H, backend=OM)
    for name in ("m4fe", "m3fe"):
        case = cases[name, cap]
        first_l, first_r, npairs = case["layout"]
        for p in range(npairs):
            q, want = case["Q"][p], case["want"][p]
            nl, nr = hp.n(first_l + p), hp.n(first_r + p)
            if nl == 0 or nr == 0:                                          # (the host form of the oracle takes two non-empty cameras)
                continue
            fl, fr = view(first_l + p), view(first_r + p)
            bl, br = case["blocked_l"][p][:nl], case["blocked_r"][p][:nr]
            if name == "m4fe":
                got = OM.SearchByProjectionFrameFisheye(fl, fr, blocked_l=bl, blocked_r=br, scale_factors=hp.sf, valid=q["valid"], u=q["u"], v=q["v"],
                                                        ur=q["ur"], vr=q["vr"], octave=q["octave"], angle=q["angle"], qdesc=q["qdesc"], mp_obs=q["mp_obs"],
                                                        th=sc.M4_TH, check_ori=True)
            else:
                left = dict(in_view=q["in_view"], px=q["px"], py=q["py"], view_cos=q["view_cos"], level=q["level"])
                right = dict(in_view=q["in_view_r"], px=q["pxr"], py=q["pyr"], view_cos=q["view_cos_r"], level=q["level_r"])
                got = OM.SearchByProjectionPointsFisheye(fl, fr, blocked_l=bl, blocked_r=br, l2r=np.full(nl, -1, np.int32), r2l=np.full(nr, -1, np.int32),
                                                         scale_factors=hp.sf, left=left, right=right, qdesc=q["qdesc"], mp_obs=q["mp_obs"], th=sc.M3_TH,
                                                         nnratio=sc.M3_NNRATIO)
            assert int(got[0]) == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (name, p)
