"""The inputs of tests/test_gpu_mappoint.py: a KeyFrame pool of 12 rows of 96 slots and one call of about 200 MapPoints whose
observation lists interleave every size at which the kernel changes its path (numpy only; shared by the GPU tests and the facade
smoke's expectations).  Nothing here depends on the product."""
import numpy as np

F = np.float32
NROWS, CAP, NLEV = 12, 96, 8
COUNTS = np.array([96, 96, 0, 50, 96, 96, 96, 96, 96, 96, 96, 96], np.int32)   # an empty row and a partly filled one
STACKED = (4, 5, 6, 7)                                                          # two-camera rows: 48 left slots, then 48 right slots
CROW = 11                                                                       # the row of constructed descriptors
NS = [0, -1, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 300]   # -1: 0 after skipping
RIGHT, BAD_KF = 1, 2
SCALE = (F(1.2) ** np.arange(NLEV)).astype(F)


def flip(base, bits):
    d = np.array(base, np.uint8).copy()
    for b in bits:
        d[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return d


def pool(seed=5):
    rng = np.random.default_rng(seed)
    kp_dtype = np.dtype([("x", F), ("y", F), ("size", F), ("angle", F), ("response", F), ("octave", np.int32), ("class_id", np.int32)])
    desc = rng.integers(0, 256, (NROWS, CAP, 32)).astype(np.uint8)
    base = desc[CROW, 0].copy()
    # the constructed row: exact distances to the base, duplicates, complements
    for s in range(1, 40):
        desc[CROW, s] = flip(base, rng.choice(256, s, replace=False))       # distance s to the base
    desc[CROW, 40] = base; desc[CROW, 41] = base                            # duplicates of the base
    desc[CROW, 42] = ~base; desc[CROW, 43] = ~base                          # complements: distance 256
    desc[CROW, 44] = flip(base, range(0, 10)); desc[CROW, 45] = flip(base, range(10, 40))
    q = flip(base, range(100, 220))                                         # a second cluster, 120 bits away
    desc[CROW, 50] = q; desc[CROW, 51] = flip(q, [8, 9]); desc[CROW, 52] = flip(q, [8, 9, 10, 11])
    desc[CROW, 53] = flip(base, [0, 1]); desc[CROW, 54] = flip(base, [0, 1, 2, 3])
    kps = np.zeros((NROWS, CAP), kp_dtype)
    kps["octave"] = rng.integers(0, NLEV, (NROWS, CAP))
    kps["octave"][0, 90:96] = [NLEV, NLEV + 1, -1, 100, -5, NLEV]           # octaves outside the scale table
    kps["x"] = rng.uniform(0, 640, (NROWS, CAP)); kps["y"] = rng.uniform(0, 480, (NROWS, CAP))
    ow_l = rng.uniform(-2, 2, (NROWS, 3)).astype(F); ow_r = (ow_l + rng.uniform(-0.3, 0.3, (NROWS, 3))).astype(F)
    return dict(desc=desc, kps=kps, counts=COUNTS.copy(), ow_l=ow_l, ow_r=ow_r, base=base)


def _live_slots():
    return [(r, s) for r in range(NROWS) for s in range(COUNTS[r])]


def _junk_entry(rng):
    """An entry both functions skip: a row outside the pool, a slot outside the row's count."""
    kind = rng.integers(0, 7)
    return [(-1, 3), (NROWS, 0), (1 << 20, 5), (0, -1), (3, int(COUNTS[3])), (2, 0), (1, 1 << 30)][kind]


def mappoints(P, seed=9, cycles=10):
    """-> dict of the call's arrays.  MapPoint i of cycle c has NS[i] live descriptors; every third MapPoint also carries skipped
    entries and bad-KeyFrame entries between its live ones, so that the positions reported count them and lists of at most 64 live
    entries cross 64 entries in all."""
    rng = np.random.default_rng(seed)
    live = _live_slots()
    few_rows = [(r, s) for r in (0, 1, 4, 5) for s in range(COUNTS[r])]     # N = 300 comes from many slots of few rows
    off, row, slot, flags, ns = [5], [], [], [], []
    for _ in range(5):                                                      # obs_off[0] > 0: entries before the first list
        r, s = live[rng.integers(len(live))]
        row.append(r); slot.append(s); flags.append(0)
    special = []                                                            # (first entry, kind) of the constructed MapPoints
    for c in range(cycles):
        for i, n in enumerate(NS):
            if n == 300 and c not in (0, 5):
                n = 5
            if n == 129 and c not in (0, 3, 6):
                n = 6
            ent = []
            if n == -1:                                                     # 0 after skipping: bad KeyFrames (the normal counts them) or junk only
                for k in range(4):
                    if c % 2:
                        ent.append(_junk_entry(rng) + (0,))
                    else:
                        r, s = live[rng.integers(len(live))]
                        ent.append((r, s, BAD_KF))
                n = 0
            else:
                src = few_rows if n > 200 else live
                for k in rng.choice(len(src), n, replace=False):
                    r, s = src[k]
                    ent.append((r, s, RIGHT if (r in STACKED and s >= 48) else 0))
                if (c * len(NS) + i) % 3 == 0 and n > 0:
                    for _ in range(rng.integers(1, 6)):
                        at = rng.integers(0, len(ent) + 1)
                        if rng.random() < 0.5:
                            ent.insert(at, _junk_entry(rng) + (int(rng.integers(0, 2)),))
                        else:
                            r, s = live[rng.integers(len(live))]
                            ent.insert(at, (r, s, BAD_KF | (RIGHT if (r in STACKED and s >= 48) else 0)))
            for r, s, f in ent:
                row.append(r); slot.append(s); flags.append(f)
            off.append(len(row)); ns.append(n)
    # the constructed MapPoints, over the constructed row
    for kind, slots in (("complement", [0, 42, 43]), ("equal", [0, 40, 41]), ("clusters", [50, 0, 51, 53, 52, 54]), ("lower_median", [45, 44, 0]),
                        ("complement_pair", [42, 0])):
        special.append((len(off) - 1, kind))
        for s in slots:
            row.append(CROW); slot.append(s); flags.append(0)
        off.append(len(row)); ns.append(len(slots))
    off = np.array(off, np.int32)
    nmp = len(off) - 1
    # a decreasing pair: MapPoint `dec` ends before it starts, and its successor's list starts inside earlier entries
    dec = 7
    off[dec + 1] = off[dec] - 3
    row, slot, flags = np.array(row, np.int32), np.array(slot, np.int32), np.array(flags, np.uint8)
    valid = np.ones(nmp, np.uint8); valid[[11, 37, 58, 120]] = 0
    pw = rng.uniform(-5, 5, (nmp, 3)).astype(F)
    # the reference slot: the first entry of the list that is inside the pool (what the caller's :627-638 rule names when the reference
    # KeyFrame is the first one observed); then the gated cases
    ref_row = np.full(nmp, -1, np.int32); ref_slot = np.full(nmp, -1, np.int32)
    for mp in range(nmp):
        for e in range(off[mp], max(off[mp + 1], off[mp])):
            if 0 <= row[e] < NROWS and 0 <= slot[e] < COUNTS[row[e]]:
                ref_row[mp], ref_slot[mp] = row[e], slot[e]
                break
    gated = {}
    with_ref = [mp for mp in range(nmp) if ref_row[mp] >= 0 and valid[mp]]
    for k, (rr, rs) in enumerate([(0, 90), (0, 92), (0, 93), (NROWS, 0), (-1, 0), (3, 50), (2, 0), (1, -1), (0, 95)]):
        mp = with_ref[3 + 9 * k]
        ref_row[mp], ref_slot[mp] = rr, rs
        gated[mp] = (rr, rs)
    return dict(nmp=nmp, off=off, row=row, slot=slot, flags=flags, valid=valid, pw=pw, ref_row=ref_row, ref_slot=ref_slot, ns=np.array(ns),
                special=dict((k, i) for i, k in special), dec=dec, gated=gated)
