"""A second reading of the three covisibility walks, written from the reference alone on plain Python objects, plus a numpy statement of
the call contracts of orbm_covisibility_votes, orbm_local_points and orbm_gather_map_points_batch_async (include/orbm.h) and the flatten
of facade/Covisibility.h.  Nothing here imports the package.

  ConnectionCounts      KeyFrame::UpdateConnections step 1, KeyFrame.cc:474-512: the KFcounter map
  LocalKeyFrameVotes    Tracking::UpdateLocalKeyFrames, Tracking.cc:3964-4013: the keyframeCounter map, bad MapPoints set to NULL (:3986)
  LocalMapPoints        Tracking::UpdateLocalPoints, Tracking.cc:3917-3948: mvpLocalMapPoints in the reference's order
The objects are those of tests/second_reading_kfcull.py (KeyFrame, MapPoint with AddObservation's left / right tuple).  "Pointer order" is
the explicit attribute `addr`: a std::map<KeyFrame*, ...> is walked in ascending addr."""
import numpy as np

from second_reading_kfcull import KeyFrame, Map, MapPoint, link  # noqa: F401  (re-exported: the cases build on them)

MP_MAX_OBS = 65535


class Frame:
    def __init__(self, mnId, mps):
        self.mnId = mnId
        self.mvpMapPoints = list(mps)
        self.N = len(self.mvpMapPoints)


def by_addr(counter):
    """A std::map<KeyFrame*, int> as a list of (KeyFrame, count) in pointer order."""
    return sorted(counter.items(), key=lambda kv: kv[0].addr)


def ConnectionCounts(kf):                                                   # KeyFrame.cc:474-512
    counter = {}
    for mp in list(kf.mvpMapPoints):
        if mp is None:
            continue
        if mp.isBad():
            continue
        for kfi, _ in mp.GetObservations():
            if kfi.mnId == kf.mnId or kfi.isBad() or kfi.map is not kf.map:
                continue
            counter[kfi] = counter.get(kfi, 0) + 1
    return counter


def connection_summary(counter, th=15):
    """:520-560: pKFmax = the first maximum in pointer order (strict >), vPairs = the (weight, KeyFrame) pairs at or above th."""
    nmax, kfmax, pairs = 0, None, []
    for kf, n in by_addr(counter):
        if n > nmax:
            nmax, kfmax = n, kf
        if n >= th:
            pairs.append((n, kf))
    return nmax, kfmax, pairs


def LocalKeyFrameVotes(frame):                                              # Tracking.cc:3964-4013 (both branches run the same loop)
    counter = {}
    for i in range(frame.N):
        mp = frame.mvpMapPoints[i]
        if mp is not None:
            if not mp.isBad():
                for kfi, _ in mp.GetObservations():
                    counter[kfi] = counter.get(kfi, 0) + 1
            else:
                frame.mvpMapPoints[i] = None
    return counter


def LocalMapPoints(local_kfs, frame_id):                                    # Tracking.cc:3917-3948
    out = []
    for kf in reversed(local_kfs):
        for mp in kf.GetMapPointMatches():
            if mp is None:
                continue
            if getattr(mp, "mnTrackReferenceForFrame", None) == frame_id:
                continue
            if not mp.isBad():
                out.append(mp)
                mp.mnTrackReferenceForFrame = frame_id
    return out


# ---- the call contracts in numpy -------------------------------------------------------------------------------------------
def _live(e, counts_kf, cap, obs_row, obs_slot):
    r, s = int(obs_row[e]), int(obs_slot[e])
    return 0 <= r < len(counts_kf) and 0 <= s < min(int(counts_kf[r]), cap)


def _range(j, obs_off, nobs, mp_valid):
    if mp_valid is not None and not mp_valid[j]:
        return 0, 0
    a, b = int(obs_off[j]), int(obs_off[j + 1])
    if a < 0 or b > nobs or b <= a or b - a > MP_MAX_OBS:
        return 0, 0
    return a, b


def votes_contract(q_mp, q_n, self_row, counts_kf, cap, kf_skip, skip_bad, obs_off, obs_row, obs_slot, obs_flags, mp_valid=None, th=15, list_cap=0,
                   list_fill=-1):
    """orbm_covisibility_votes.  Entries that the call does not write hold list_fill."""
    q_mp = np.asarray(q_mp); nq, qs = q_mp.shape
    nrows, nmp, nobs = len(counts_kf), len(obs_off) - 1, len(obs_row)
    votes = np.zeros((nq, nrows), np.int32)

    def voter(e, self_r):                                                   # the row entry e may vote for, or -1
        if not _live(e, counts_kf, cap, obs_row, obs_slot):
            return -1
        r = int(obs_row[e])
        if r == self_r or (kf_skip is not None and kf_skip[r]) or (skip_bad and (int(obs_flags[e]) & 2)):
            return -1
        return r

    for q in range(nq):
        self_r = -1 if self_row is None else int(self_row[q])
        for i in range(min(max(int(q_n[q]), 0), qs)):
            j = int(q_mp[q, i])
            if not 0 <= j < nmp:
                continue
            a, b = _range(j, obs_off, nobs, mp_valid)
            for e in range(a, b):
                r = voter(e, self_r)
                if r < 0:
                    continue
                if (int(obs_flags[e]) & 1) and e > a and int(obs_row[e - 1]) == r and not (int(obs_flags[e - 1]) & 1) and voter(e - 1, self_r) == r:
                    continue                                                # the KeyFrame voted at the left entry
                votes[q, r] += 1
    out = {"votes": votes, "n_voted": (votes > 0).sum(1).astype(np.int32), "max_votes": votes.max(1).astype(np.int32),
           "n_over": ((votes >= th) & (votes > 0)).sum(1).astype(np.int32), "list_row": None, "list_votes": None}
    if list_cap > 0:
        lr = np.full((nq, list_cap), list_fill, np.int32); lv = np.full((nq, list_cap), list_fill, np.int32)
        for q in range(nq):
            rows = np.flatnonzero(votes[q] > 0)[:list_cap]
            lr[q, :len(rows)] = rows; lv[q, :len(rows)] = votes[q, rows]
        out.update(list_row=lr, list_votes=lv)
    return out


def local_points_contract(lkf_row, n_lkf, counts_kf, kf_mp, nmp, mp_valid=None, q_stride=None, fill=-1):
    """orbm_local_points -> (local_mp [T][q_stride] with `fill` at and beyond nq, n_total, nq)."""
    lkf_row = np.asarray(lkf_row); T, ls = lkf_row.shape
    kf_mp = np.asarray(kf_mp); nrows, cap = kf_mp.shape
    qs = q_stride if q_stride is not None else max(1, min(nmp, ls * cap))
    out = np.full((T, qs), fill, np.int32); nt = np.zeros(T, np.int32)
    for f in range(T):
        seen, n = set(), 0
        for k in range(min(max(int(n_lkf[f]), 0), ls)):
            r = int(lkf_row[f, k])
            if not 0 <= r < nrows:
                continue
            for i in range(min(int(counts_kf[r]), cap)):
                j = int(kf_mp[r, i])
                if not 0 <= j < nmp or (mp_valid is not None and not mp_valid[j]) or j in seen:
                    continue
                seen.add(j)
                if n < qs:
                    out[f, n] = j
                n += 1
        nt[f] = n
    return out, nt, np.minimum(nt, qs).astype(np.int32)


def gather_contract(local_mp, nq, src, dst, mp_skip=None):
    """orbm_gather_map_points_batch_async: src = dict of pool rows (pw, normal, min_dist, max_dist, desc, nobs), dst = dict of the
    caller's destination arrays (pw, normal, min_dist, max_dist, qdesc, mp_obs, skip), changed in place and returned."""
    T, qs = local_mp.shape
    nmp = len(src["nobs"])
    for f in range(T):
        n = min(max(int(nq[f]), 0), qs)
        idx = local_mp[f, :n]
        ok = (idx >= 0) & (idx < nmp)
        e, j = np.flatnonzero(ok), idx[ok]
        dst["skip"][f, np.flatnonzero(~ok)] = 1
        dst["skip"][f, e] = 0 if mp_skip is None else (mp_skip[f, j] != 0)
        for d, s in (("pw", "pw"), ("normal", "normal"), ("min_dist", "min_dist"), ("max_dist", "max_dist"), ("qdesc", "desc")):
            dst[d][f, e] = src[s][j]
        dst["mp_obs"][f, e] = src["nobs"][j] > 0
    return dst


# ---- the flatten of facade/Covisibility.h ------------------------------------------------------------------------------------
def flatten_votes(queries, self_kfs=None, this_map=None):
    """queries = per query the slot list (MapPoint or None); self_kfs = per query the query KeyFrame, or None for Frames.  Pool rows: the
    query KeyFrames in order, then every other observing KeyFrame in the order it is met; the MapPoint list: the order in which the
    queries' slots meet them.  Entries per MapPoint in pointer order, left before right; flags bit 0 right, bit 1 the KeyFrame isBad(),
    bit 2 the entry weighs 2 (ignored by the vote).  A bad MapPoint has an empty list.  kf_skip = the KeyFrame lies in another map than
    this_map (None: no row is skipped)."""
    rows, row_of, mps, mp_of = [], {}, [], {}

    def row_for(kf):
        if kf not in row_of:
            row_of[kf] = len(rows)
            rows.append(kf)
        return row_of[kf]

    for kf in (self_kfs or []):
        if kf is not None:
            row_for(kf)
    off, orow, oslot, oflags, valid = [0], [], [], [], []
    q_rows = []
    for slots in queries:
        r = []
        for mp in slots:
            if mp is None:
                r.append(-1)
                continue
            if mp not in mp_of:
                mp_of[mp] = len(mps)
                mps.append(mp)
                valid.append(0 if mp.isBad() else 1)
                if not mp.isBad():
                    for kfi, (left, right) in mp.GetObservations():
                        ri = row_for(kfi)
                        b = 2 if kfi.isBad() else 0
                        if left != -1:
                            w2 = 4 if (not kfi.mpCamera2 and kfi.mvuRight[left] >= 0) else 0
                            orow.append(ri); oslot.append(left); oflags.append(b | w2)
                        if right != -1:
                            orow.append(ri); oslot.append(right); oflags.append(b | 1)
                off.append(len(orow))
            r.append(mp_of[mp])
        q_rows.append(r)
    qs = max([1] + [len(r) for r in q_rows])
    q_mp = np.full((len(q_rows), qs), -1, np.int32)
    for q, r in enumerate(q_rows):
        q_mp[q, :len(r)] = r
    if not mps:                                                             # the call wants nmp >= 1: one MapPoint that is not valid
        off, valid = [0, 0], [0]
    if not rows:
        rows_n, counts = 1, np.zeros(1, np.int32)
    else:
        rows_n, counts = len(rows), np.array([kf.N for kf in rows], np.int32)
    return {"q_mp": q_mp, "q_n": np.array([len(r) for r in q_rows], np.int32),
            "self_row": None if self_kfs is None else np.array([-1 if kf is None else row_of[kf] for kf in self_kfs], np.int32),
            "counts_kf": counts, "cap": max([1] + [kf.N for kf in rows]),
            "kf_skip": None if this_map is None else np.array([0 if kf.map is this_map else 1 for kf in rows] + [0] * (rows_n - len(rows)), np.uint8),
            "obs_off": np.array(off, np.int32), "obs_row": np.array(orow, np.int32), "obs_slot": np.array(oslot, np.int32),
            "obs_flags": np.array(oflags, np.uint8), "mp_valid": np.array(valid, np.uint8), "rows": rows, "mps": mps}


VOTE_ORDER = ("q_mp", "q_n", "self_row", "counts_kf", "cap", "kf_skip")
OBS_ORDER = ("obs_off", "obs_row", "obs_slot", "obs_flags", "mp_valid")


def vote_args(F, skip_bad, th=15, list_cap=0):
    return [F[k] for k in VOTE_ORDER] + [skip_bad] + [F[k] for k in OBS_ORDER] + [th, list_cap]


def counter_of(F, votes_row):
    """The dense vote row of one query as the reference's map."""
    return {F["rows"][r]: int(v) for r, v in enumerate(votes_row[:len(F["rows"])]) if v > 0}


def flatten_local(frames_local_kfs):
    """frames_local_kfs = per frame mvpLocalKeyFrames (the reference's order).  Pool rows: the KeyFrames in the order the reverse walks
    meet them; MapPoints in the order the rows' slots meet them; lkf_row = each list reversed."""
    rows, row_of, mps, mp_of = [], {}, [], {}
    for kfs in frames_local_kfs:
        for kf in reversed(kfs):
            if kf not in row_of:
                row_of[kf] = len(rows)
                rows.append(kf)
    cap = max([1] + [kf.N for kf in rows])
    kf_mp = np.full((max(len(rows), 1), cap), -1, np.int32)
    for r, kf in enumerate(rows):
        for i, mp in enumerate(kf.GetMapPointMatches()):
            if mp is None:
                continue
            if mp not in mp_of:
                mp_of[mp] = len(mps)
                mps.append(mp)
            kf_mp[r, i] = mp_of[mp]
    ls = max([1] + [len(k) for k in frames_local_kfs])
    lkf_row = np.full((len(frames_local_kfs), ls), -1, np.int32)
    for f, kfs in enumerate(frames_local_kfs):
        lkf_row[f, :len(kfs)] = [row_of[kf] for kf in reversed(kfs)]
    return {"lkf_row": lkf_row, "n_lkf": np.array([len(k) for k in frames_local_kfs], np.int32),
            "counts_kf": np.array([kf.N for kf in rows] or [0], np.int32), "kf_mp": kf_mp, "nmp": max(len(mps), 1),
            "mp_valid": np.array([0 if mp.isBad() else 1 for mp in mps] or [0], np.uint8), "rows": rows, "mps": mps}


LOCAL_ORDER = ("lkf_row", "n_lkf", "counts_kf", "kf_mp", "nmp", "mp_valid")
