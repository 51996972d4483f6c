"""The extractor's host planner (orb-slam3_amd/csrc/orbx_plan.h) on the CPU: tests/plan_dump.cpp, compiled with g++ against the header
the library compiles, plans every configuration below and prints what this module asserts.  Host-only: no GPU, no HIP.

What is held to what:
  * the constructor tables to the oracle's (bit for bit) and to the second reading's features_per_level; level sizes to the oracle's;
  * the FAST cells to structured_images.fast_cells, the queue capacities to structured_images.fast_queue_caps (which pins those
    restatements to the code), the strips, launch groups and k_fast4 tables to the field limits the kernels' comments leave to the host;
  * k_resize2's task records to the tap table they were made from, to an exactly-once cover of every destination row and dword, to
    test_gpu_resize_tasks.classes_of, and rz_launch's multiply-high division to the integer quotient for every wave of the largest batch;
  * k_blur3's two task lists to an exactly-once cover of every (column group, tile), its weights to sums of 256;
  * the quadtree's capacities to max(N + 3, 4 * nIni), its form to the restatement in tests/test_gpu_extract_second_reading.py;
  * refused sizes to the code and text the library has always given.
Both the product form and the -DORBX_AB form of the header run, the latter also with the planner's A/B knobs set, and a second build
under AddressSanitizer and UBSan runs the whole list as a plain child process."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import second_reading_extract as sr
import structured_images as si
import test_gpu_resize_tasks as rt
from test_gpu_extract_second_reading import _max_n             # the restated rule: wide from 512 nodes on, or while frames * levels <= 512
from test_oracle_params_cpu import _level_sizes, _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan_dump.cpp")
KNOBS = dict(blurTiled=1, fastV3=0, noFixedPitch=0, qcapForce=0, qtWideForce=-1, fastWgs=7, fastLdsPad=0, rzNoPack=0)
LDS = 160 * 1024
F3_WAVES = 4                                                    # F3_NT / 64


def cfg(w, h, nf=1000, sf=1.2, nl=8, mb=1, name=None, **knobs):
    assert set(knobs) <= set(KNOBS)
    return dict(w=w, h=h, nf=nf, sf=sf, nl=nl, mb=mb, name=name, knobs=dict(KNOBS, **knobs))


def _smallest(sf, nl):
    """Smallest accepted width and height as tests/test_oracle_params_cpu.py::test_too_small_boundary predicts them."""
    inv_sf = _tables(10, sf, nl)["inv_sf"]
    ok = lambda w, h: all(sw - 32 >= 35 and sh - 32 >= 35 for sw, sh in _level_sizes(w, h, inv_sf))
    return next(w for w in range(30, 4000) if ok(w, 600)), next(h for h in range(30, 4000) if ok(800, h))


WMIN, HMIN = _smallest(1.2, 8)
FIXED = [cfg(752, 480, mb=1), cfg(752, 480, mb=512),
         cfg(421, 307), cfg(1241, 376), cfg(1920, 1080, nf=4000), cfg(1920, 1080, nf=4000, mb=64), cfg(320, 240, nf=300, nl=4),
         cfg(752, 480, sf=1.5, nl=5), cfg(752, 480, sf=1.1, nl=12)]
FIXED += [cfg(w, h, nf=200, sf=s, nl=nl, mb=n, name=k) for k, (w, h, nl, s, n) in rt.GEOMS.items()]
EDGES = [cfg(WMIN, HMIN), cfg(WMIN - 1, HMIN), cfg(WMIN, HMIN - 1),
         cfg(4200, 600, nl=1),                                   # a level beyond 4095 px
         cfg(2000, 150, nl=1)]                                   # inner area 1968 x 118: 17 quadtree roots


def _sweep():
    rng = np.random.default_rng(20240917)
    out = []
    for _ in range(300):
        sf = float(np.float32(1.0 + rng.uniform(0.02, 0.7)))
        nl = int(rng.integers(1, 13))
        grow = float(sf) ** (nl - 1)                            # (top level from about one cell up; frames up to 1800 x 1200)
        w = min(int(rng.integers(67, 330) * grow), 1800); h = min(int(rng.integers(67, 220) * grow), 1200)
        out.append(cfg(w, h, nf=int(rng.integers(50, 5001)), sf=sf, nl=nl, mb=int(rng.choice([1, 2, 7, 64, 512]))))
    return out


SWEEP = _sweep()
AB_KNOBS = [cfg(752, 480, mb=512, rzNoPack=1), cfg(312, 96, nf=200, nl=3, mb=65, name="pack64", rzNoPack=1), cfg(752, 480, fastV3=1),
            cfg(752, 480, noFixedPitch=1), cfg(1241, 376, noFixedPitch=1), cfg(752, 480, blurTiled=0), cfg(752, 480, fastWgs=8),
            cfg(752, 480, qcapForce=100), cfg(1920, 1080, nf=4000, qcapForce=64), cfg(752, 480, qtWideForce=0), cfg(752, 480, mb=512, qtWideForce=1),
            cfg(752, 480, fastLdsPad=4096)]
PRODUCT = FIXED + EDGES + SWEEP


def _line(c):
    k = c["knobs"]
    return "%d %d %d %.9g %d 20 7 %d  %d %d %d %d %d %d %d %d" % (c["w"], c["h"], c["nf"], c["sf"], c["nl"], c["mb"], k["blurTiled"], k["fastV3"],
                                                                 k["noFixedPitch"], k["qcapForce"], k["qtWideForce"], k["fastWgs"], k["fastLdsPad"], k["rzNoPack"])


def _build(out, *flags):
    return subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *flags, "-o", out, SRC], capture_output=True, text=True)


def _run(exe, configs):
    r = subprocess.run([exe], input="\n".join(_line(c) for c in configs) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(configs)
    return lines


BUILDS = {"product": ((), PRODUCT), "ab": (("-DORBX_AB",), PRODUCT + AB_KNOBS)}     # name -> (flags, configurations)


def _build_and_run(directory, *flags):
    """{build: printed lines, or the compiler's complaint}; the two builds side by side."""
    def one(name):
        exe = os.path.join(str(directory), "plan_dump_" + name)
        r = _build(exe, *flags, *BUILDS[name][0])
        return _run(exe, BUILDS[name][1]) if r.returncode == 0 else r.stderr
    with ThreadPoolExecutor(2) as pool:
        return dict(zip(BUILDS, pool.map(one, BUILDS)))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{build: [(configuration, printed line)]}: every list planned once."""
    out = _build_and_run(tmp_path_factory.mktemp("plan_dump"))
    for name, lines in out.items():
        assert isinstance(lines, list), lines
    return {name: list(zip(BUILDS[name][1], lines)) for name, lines in out.items()}


# ---- what a configuration must be refused with (the library's codes and texts), from the restated level sizes
def expected_refusal(c):
    for l, (lw, lh) in enumerate(sr.level_sizes(c["w"], c["h"], c["sf"], c["nl"])):
        if lw > 4095 or lh > 4095:
            return -6, "level %d is %dx%d: packed candidates hold 12-bit coordinates" % (l, lw, lh)
        if (lw - 32) // 35 < 1 or (lh - 32) // 35 < 1:
            return -4, "level %d (%dx%d) is smaller than one FAST cell" % (l, lw, lh)
        n_ini = sr.c_round(np.float32(lw - 32) / np.float32(lh - 32))
        if n_ini < 1 or n_ini > 16:
            return -6, "aspect ratio of level %d unsupported (nIni=%d; the reference divides by zero for nIni=0)" % (l, n_ini)
    # the quadtree's workgroup must hold a level's lists in LDS: k_quadtree2's, then the A/B kernel's (quadtree)
    sizes = sr.level_sizes(c["w"], c["h"], c["sf"], c["nl"])
    max_n = _max_n((c["w"], c["h"], c["nf"], c["nl"], c["sf"]))
    if 2 * max_n + 64 > 65000:
        return -6, "nfeatures per level %d too large for 16-bit node ids" % max_n
    pow2 = lambda n: 1 << (n - 1).bit_length()
    max_ini = max(sr.c_round(np.float32(lw - 32) / np.float32(lh - 32)) for lw, lh in sizes)
    max_cells = max(len(si.fast_cells(lw, lh)[0]) for lw, lh in sizes)
    hist, path = (340, 256) if max_n >= 512 and max_ini <= 4 else (84, 64)
    cap = max_n + 8
    for lds in (pow2(cap) * 8 + cap * 68 + (max_cells + 1) * 4 + 64 + max_ini * (hist * 4 + path * 2) + cap * 4 + 8,
                pow2(max_n + 8) * 8 + (2 * max_n + 64) * 56 + 64):
        if lds > LDS - 512:
            return -6, "quadtree for %d features/level needs %d B of LDS (> 160 KiB)" % (max_n, lds)
    return 0, ""


_level_size_cache = {}


def oracle_level_sizes(oracle, c):
    key = (c["w"], c["h"], c["sf"], c["nl"])
    if key not in _level_size_cache:
        ref = oracle.Extractor(50, c["sf"], c["nl"], 20, 7)
        assert ref(np.zeros((c["h"], c["w"]), np.uint8), (0, 0))[0] == 0
        _level_size_cache[key] = [ref.level_size(l) for l in range(c["nl"])]
    return _level_size_cache[key]


LV = ("w", "h", "pitch", "off", "boff", "btpr", "rzx", "rzy", "cellBase", "nCells", "slotBase", "slotCap", "N", "nIni", "qtW", "qtH", "hX", "selBase",
      "selCap", "sf", "patch")
G = ("nlevels", "w0", "h0", "iniTh", "minTh", "lowTh", "totalCells", "totalSlots", "totalSel", "kpCap", "nodeCap", "sortCap", "pyrFrameBytes",
     "blrFrameBytes", "blurTiled")
RZ = ("stream", "nFull", "nPack", "pack", "r", "nsrcMin", "nsrcMax", "x4max", "coverBad", "ytBad", "fieldBad", "mulhiBad", "nWaves", "taskOff", "ntasks",
      "streamP", "taskOffP", "ntasksP")


def check(oracle, c, d, ab):
    """Every assertion on one planned configuration (d: the decoded line)."""
    tag = (c["w"], c["h"], c["nf"], c["sf"], c["nl"], c["mb"], c["knobs"])
    L, k = c["nl"], c["knobs"]
    # tables: the oracle's, bit for bit
    t = oracle.Extractor(c["nf"], c["sf"], L, 20, 7).tables()
    for name, ref in (("sf", "sf"), ("invsf", "inv_sf"), ("sig2", "sig2"), ("invsig2", "inv_sig2")):
        assert np.array_equal(np.array(d["tab"][name], np.uint32), t[ref].view(np.uint32)), (tag, name)
    assert d["tab"]["nfeat"] == t["nfeat"].tolist() == sr.features_per_level(c["nf"], c["sf"], L), tag
    assert d["tab"]["umax"] == t["umax"].tolist(), tag
    odw = np.array(d["tab"]["odW"], np.uint32).reshape(17, 8)
    for va in range(17):                                        # byte b of dword j: u + 16 inside the disc row, 0 outside; row 16 all zero
        row = odw[va].view(np.uint8).astype(int)
        u = np.arange(32) - 15
        assert np.array_equal(row, np.where((np.abs(u) <= t["umax"][va]) & (u <= 15), u + 16, 0) if va < 16 else np.zeros(32, int)), (tag, va)
    want_rc, want_err = expected_refusal(c)
    assert (d["rc"], d["err"]) == (want_rc, want_err), tag
    if d["rc"]:
        return
    g = dict(zip(G, d["g"]))
    lv = [dict(zip(LV, v)) for v in d["lv"]]
    assert len(lv) == L == g["nlevels"] and (g["w0"], g["h0"], g["iniTh"], g["minTh"], g["lowTh"]) == (c["w"], c["h"], 20, 7, 7)
    sizes = oracle_level_sizes(oracle, c)
    assert [(D["w"], D["h"]) for D in lv] == sizes == sr.level_sizes(c["w"], c["h"], c["sf"], L), tag
    assert g["blurTiled"] == k["blurTiled"]
    off = boff = 0
    for l, D in enumerate(lv):                                  # slabs: levels in order, 64-byte pitches, 256-byte aligned starts
        assert D["pitch"] % 64 == 0 and 0 <= D["pitch"] - D["w"] < 64 and D["off"] == off and D["boff"] == (boff if k["blurTiled"] else off), (tag, l)
        off += -(-D["pitch"] * D["h"] // 256) * 256
        assert D["btpr"] == D["pitch"] // 16 + 1
        boff += -(-D["btpr"] * ((D["h"] + 7) // 8) * 128 // 256) * 256
        assert D["N"] == int(t["nfeat"][l]) and D["sf"] == int(t["sf"][l:l + 1].view(np.uint32)[0])
    assert g["pyrFrameBytes"] == off and g["blrFrameBytes"] == (boff if k["blurTiled"] else off), tag
    # cells: structured_images.fast_cells, cell by cell; evaluated windows tile the level's inner area
    cells = np.array(d["cells"], np.int64).reshape(-1, 10)
    assert len(cells) == g["totalCells"] == sum(D["nCells"] for D in lv)
    slot = 0
    for l, D in enumerate(lv):
        want, (wc, hc) = si.fast_cells(D["w"], D["h"])
        assert D["cellBase"] == sum(x["nCells"] for x in lv[:l]) and D["nCells"] == len(want) and D["slotBase"] == slot, (tag, l)
        assert D["slotCap"] == ((wc + 1) // 2) * ((hc + 1) // 2)
        got = cells[D["cellBase"]:D["cellBase"] + D["nCells"]]
        exp = np.array([[l, x0, y0, cw, ch, j * wc, i * hc, 0, slot + n * D["slotCap"], D["cellBase"] + n] for n, (x0, y0, cw, ch, i, j) in enumerate(want)], np.int64)
        assert np.array_equal(got, exp), (tag, l)
        slot += len(want) * D["slotCap"]
    assert g["totalSlots"] == slot and d["cell_cover_bad"] == [0] * L, tag
    # strips: a partition of the cells in order, each inside one cell row
    strips = np.array(d["strips"], np.int64).reshape(-1, 9)
    nxt = 0
    for s_level, ncell, x0, y0, sw, sh, xal, lp, cell0 in strips.tolist():
        assert cell0 == nxt and 1 <= ncell <= F3_WAVES, tag
        mine = cells[cell0:cell0 + ncell]
        assert (mine[:, 0] == s_level).all() and (mine[:, 2] == y0).all() and (mine[:, 4] == sh).all() and mine[0, 1] == x0, tag
        assert sw == mine[-1, 1] + mine[-1, 3] - x0
        assert lp % 16 == 0 and lp <= 512 and xal % 16 == 0 and x0 - xal >= 4 and mine[-1, 1] + mine[-1, 3] - 3 - xal + 8 <= lp, tag
        nxt += ncell
    assert nxt == len(cells)
    assert d["stripTile"] == (strips[:, 7] * strips[:, 5]).tolist()
    # FAST groups: a partition of the strips; queue capacities as structured_images.fast_queue_caps restates them
    groups = np.array(d["f3g"], np.int64).reshape(-1, 8)
    nxt, caps = 0, [None] * L
    for strip0, nstrips, tile, qcap, last_level, pitch, lds, v4 in groups.tolist():
        assert strip0 == nxt and nstrips > 0, tag
        mine = strips[strip0:strip0 + nstrips]
        assert qcap % 64 == 0 and qcap >= 64 and lds <= LDS - 256 and lds == 2 * tile + F3_WAVES * qcap * 2 + k["fastLdsPad"], tag
        assert last_level == mine[-1, 0] and tile % 16 == 0 and pitch in (0, 176, 208) and v4 == (0 if k["fastV3"] else 1)
        assert tile >= (pitch * mine[:, 5].max() if pitch else max(d["stripTile"][strip0:strip0 + nstrips])) and (pitch == 0 or mine[:, 7].max() <= pitch)
        for l in set(mine[:, 0].tolist()):
            assert caps[l] is None
            caps[l] = qcap
        nxt += nstrips
    assert nxt == len(strips) and d["fastLds"] == groups[:, 6].max()
    if k["fastWgs"] == 7 and not k["qcapForce"] and not k["noFixedPitch"]:
        assert caps == si.fast_queue_caps(sizes), tag
    if k["qcapForce"]:
        assert max(caps) <= -(-k["qcapForce"] // 64) * 64
    # k_fast4's tables
    assert d["f4_cell_bad"] == 0 and d["f4_cells"] == (0 if k["fastV3"] else len(cells)) and d["f4_items"] >= 64, tag
    for pb, vw, vh, a, nit, npix, dup, outside, offq_bad in np.array(d["f4_shapes"], np.int64).reshape(-1, 9).tolist():
        ncol = (a + vw + 7) // 8
        assert npix == vw * vh and dup == 0 and outside == 0 and offq_bad == 0 and nit * 64 >= vh * ncol, (tag, pb, vw, vh, a)
        assert ncol <= 16 and vh <= 127 and a + vw - 1 < 128 and (vh - 1) * pb + 8 * (ncol - 1) <= 65535, (tag, pb, vw, vh, a)
    # resize
    classes = {x[0]: x for x in rt.classes_of(oracle, c["name"])} if c["name"] else {}
    for l, v in enumerate(d["rz"], 1):
        R = dict(zip(RZ, v))
        if c["name"]:
            assert R["stream"] == (0 if c["name"] == "scale17" else 1), (tag, l)
        if c["sf"] <= 1.2 and c["w"] >= 40:
            assert R["stream"] == 1, (tag, l)
        if not R["stream"]:
            assert R["ntasks"] == R["nFull"] == R["nPack"] == 0 and R["pack"] == 1
            continue
        ndw = (lv[l]["w"] + 3) // 4
        rows = -(-lv[l]["h"] // 8)
        assert R["coverBad"] == R["ytBad"] == R["fieldBad"] == R["mulhiBad"] == 0, (tag, l, R)
        assert 2 <= R["nsrcMin"] <= R["nsrcMax"] <= 12 and R["x4max"] <= 6 and R["pack"] * R["r"] <= 64, (tag, l, R)
        assert R["nFull"] == rows * (ndw // 64) and R["nPack"] == (rows if ndw % 64 else 0) and R["r"] == ndw % 64 and R["ntasks"] == R["nFull"] + R["nPack"]
        slabs_fit = g["pyrFrameBytes"] * 64 <= 1 << 32
        assert R["pack"] == (64 // R["r"] if R["r"] and slabs_fit and not k["rzNoPack"] else 1), (tag, l, R)
        assert R["nWaves"] == R["nFull"] * c["mb"] + R["nPack"] * -(-c["mb"] // R["pack"])
        assert R["taskOff"] == sum(x[14] for x in d["rz"][:l - 1])
        if classes and not k["rzNoPack"]:
            _, cw, ch, cdw, cr, cpack = classes[l]
            assert (lv[l]["w"], lv[l]["h"], ndw, R["r"]) == (cw, ch, cdw, cr) and (R["pack"] if cr else 0) == cpack, (tag, l)
        if ab:
            assert R["streamP"] == 1 and R["ntasksP"] == rows * -(-ndw // 64)
    # k_blur3 / k_blur2
    walk, one, walk_bad, one_bad, range_bad, sum_bad, ntiles2 = d["blur"]
    assert walk_bad == one_bad == range_bad == sum_bad == 0, tag
    assert one == sum(-(-D["w"] // 128) * -(-D["h"] // 26) for D in lv) and walk == sum(-(-D["w"] // 128) * -(-(-(-D["h"] // 26)) // 8) for D in lv)
    assert ntiles2 > 0
    # quadtree
    q = dict(zip(("qtLds", "qt2Lds", "qtFuseD", "maxIni", "qt2Cap", "qt2Sort", "maxCells", "qtWide", "l0pitch", "algBytes", "fusedBytes"), d["qt"]))
    for l, D in enumerate(lv):
        assert D["nIni"] == sr.c_round(np.float32(D["w"] - 32) / np.float32(D["h"] - 32)) and (D["qtW"], D["qtH"]) == (D["w"] - 32, D["h"] - 32)
        assert q["qt2Cap"] >= max(D["N"] + 3, 4 * D["nIni"]) and D["selCap"] == max(D["N"] + 3, 4 * D["nIni"]) + 1, (tag, l)
        assert D["selBase"] == sum(x["selCap"] for x in lv[:l])
    assert q["qt2Sort"] >= q["qt2Cap"] and q["qt2Sort"] & (q["qt2Sort"] - 1) == 0 and q["qtLds"] <= LDS - 512 and q["qt2Lds"] <= LDS - 512, tag
    assert sum(D["selCap"] for D in lv) == g["kpCap"] == g["totalSel"]
    assert q["maxIni"] == max(D["nIni"] for D in lv) and q["maxCells"] == max(D["nCells"] for D in lv) and q["l0pitch"] == -(-c["w"] // 64) * 64
    assert q["qtFuseD"] == (4 if q["qt2Cap"] - 8 >= 512 and q["maxIni"] <= 4 else 3)
    max_n = _max_n((c["w"], c["h"], c["nf"], L, c["sf"]))
    assert q["qt2Cap"] == max_n + 8 and g["nodeCap"] == 2 * max_n + 64, tag
    wide1, wide_mb, wide_many, walk1, walk_mb, walk_f1, walk_f0 = d["launch"]
    if k["qtWideForce"] < 0:
        assert q["qtWide"] == (max_n >= 512) and wide1 == 1 and wide_many == q["qtWide"] and wide_mb == (1 if q["qtWide"] or c["mb"] * L <= 512 else 0), tag
    else:
        assert q["qtWide"] == wide1 == wide_mb == wide_many == k["qtWideForce"], tag
    assert walk1 == (walk >= 2048) and walk_mb == (c["mb"] * walk >= 2048) and walk_f1 == 1 and walk_f0 == 0
    assert q["fusedBytes"] == sum(D["w"] * D["h"] for D in lv[:-1]) + sum(D["w"] * D["h"] for D in lv[1:])
    assert q["algBytes"] == q["fusedBytes"] + sum(D["w"] * D["h"] for D in lv)


@pytest.mark.parametrize("build", ["product", "ab"])
def test_every_plan(oracle, runs, build):
    accepted = 0
    for c, line in runs[build]:
        d = json.loads(line)
        check(oracle, c, d, build == "ab")
        accepted += d["rc"] == 0
    assert accepted >= len(FIXED) + 1 + 150                     # the sweep is mostly accepted sizes


def test_lists_hold_what_they_are_for(runs):
    rc = [json.loads(line)["rc"] for _, line in runs["product"]]
    assert rc[:len(FIXED)] == [0] * len(FIXED)
    assert rc[len(FIXED):len(FIXED) + len(EDGES)] == [0, -4, -4, -6, -6] and (WMIN, HMIN) == (239, 239)
    sweep = [json.loads(line) for _, line in runs["product"][len(FIXED) + len(EDGES):]]
    assert {d["rc"] for d in sweep} >= {0, -4}
    streams = [v[0] for d in sweep if d["rc"] == 0 for v in d["rz"]]
    assert 0 in streams and 1 in streams                       # both resize kernels
    assert {d["qt"][7] for d in sweep if d["rc"] == 0} == {0, 1} and {d["qt"][2] for d in sweep if d["rc"] == 0} == {3, 4}
    assert {g for d in sweep if d["rc"] == 0 for g in d["f3g"][5::8]} >= {176, 208}


def test_ab_header_plans_as_the_product_header(runs):
    """-DORBX_AB adds k_resize2p's task list and the knobs; with the knobs at rest every plan is the product's."""
    for (c, a), (_, b) in zip(runs["product"], runs["ab"]):
        a, b = json.loads(a), json.loads(b)
        assert a.get("hash") == b.get("hash") and a["rc"] == b["rc"] and a["err"] == b["err"], c
    base = {(c["w"], c["h"], c["nf"], c["mb"]): json.loads(line) for c, line in runs["ab"][:len(FIXED)] if c["name"] is None and c["sf"] == 1.2 and c["nl"] == 8}
    for c, line in runs["ab"][len(PRODUCT):]:                   # every knob changes the plan it is meant to change
        d = json.loads(line)
        assert d["rc"] == 0
        ref = base.get((c["w"], c["h"], c["nf"], c["mb"]))
        if ref is not None and c["knobs"]["qtWideForce"] < 0:
            assert d["hash"] != ref["hash"], c


def test_sanitized_build_plans_the_same(runs, tmp_path):
    """The same program under AddressSanitizer and UBSan, as a plain child process: every table index of the planner and of the walks
    in plan_dump.cpp is checked, and the printed lines equal the plain build's."""
    out = _build_and_run(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for name, lines in out.items():
        if not isinstance(lines, list):
            pytest.skip("no sanitizer runtime to link against: " + lines[-300:])
        assert lines == [line for _, line in runs[name]], name
