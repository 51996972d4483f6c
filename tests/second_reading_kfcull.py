"""A second reading of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:1218-1400) and of the map surgery it triggers, written from
the reference alone on plain Python objects, plus a numpy statement of the call contract of orbm_keyframe_culling (include/orbm.h) and
the flatten of facade/KeyFrameCulling.h.  Nothing here imports the package.

  MapPoint.AddObservation / EraseObservation   MapPoint.cc:191-216, :220-257 (the weights, the <= 2 rule)
  MapPoint.SetBadFlag                          MapPoint.cc:280-305 (EraseMapPointMatch in every observer)
  KeyFrame.SetBadFlag                          KeyFrame.cc:746-887 without the spanning tree (mbNotErase, the initial KeyFrame)
  KeyFrameCulling                              LocalMapping.cc:1266-1399: skips, depth gate, Observations() > thObs, the level count,
                                               the float32 compare of :1349, the count rule of :1395
The reference walks mObservations in pointer order; here every object carries `addr`, its creation number, and maps are walked in
ascending addr: the order a std::map<KeyFrame*, ...> has when the KeyFrames sit in one array.

Deviation shared with the library: for a two-camera candidate the reference reads mvKeysRight[i].octave with the stacked index i
(:1303-1305), past the end or the wrong feature; this reading takes slot i of the stacked row, mvKeysRight[i - NLeft]."""
import numpy as np

MP_MAX_OBS = 65535


class Map:
    def __init__(self, init_id=0):
        self.init_id = init_id

    def GetInitKFid(self):
        return self.init_id


class KeyFrame:
    def __init__(self, addr, mnId, octaves, pmap, NLeft=-1, camera2=False, uRight=None, depth=None, thDepth=35.0, notErase=False):
        self.addr, self.mnId, self.map = addr, mnId, pmap
        self.NLeft = NLeft                                                  # -1, or the number of left keypoints of a stacked row
        self.octaves = list(octaves)                                        # mvKeysUn (NLeft == -1) or mvKeys then mvKeysRight
        self.N = len(self.octaves)
        self.mpCamera2 = camera2
        self.mvuRight = list(uRight) if uRight is not None else [-1.0] * self.N
        self.mvDepth = list(depth) if depth is not None else [-1.0] * self.N
        self.mThDepth = thDepth
        self.mvpMapPoints = [None] * self.N
        self.mbNotErase, self.mbToBeErased, self.mbBad = notErase, False, False

    def isBad(self):
        return self.mbBad

    def GetMapPointMatches(self):
        return list(self.mvpMapPoints)

    def EraseMapPointMatch(self, idx):
        self.mvpMapPoints[idx] = None

    def SetBadFlag(self):                                                   # KeyFrame.cc:746-887
        if self.mnId == self.map.GetInitKFid():
            return
        if self.mbNotErase:
            self.mbToBeErased = True
            return
        for mp in self.mvpMapPoints:                                        # :773-780
            if mp is not None:
                mp.EraseObservation(self)
        self.mbBad = True                                                   # :881


class MapPoint:
    def __init__(self, addr):
        self.addr = addr
        self.mObservations = {}                                             # KeyFrame -> (leftIndex, rightIndex)
        self.nObs = 0
        self.mbBad = False

    def isBad(self):
        return self.mbBad

    def Observations(self):
        return self.nObs

    def GetObservations(self):
        return [(kf, self.mObservations[kf]) for kf in sorted(self.mObservations, key=lambda k: k.addr)]

    def AddObservation(self, kf, idx):                                      # MapPoint.cc:191-216
        left, right = self.mObservations.get(kf, (-1, -1))
        if kf.NLeft != -1 and idx >= kf.NLeft:
            right = idx
        else:
            left = idx
        self.mObservations[kf] = (left, right)
        if not kf.mpCamera2 and kf.mvuRight[idx] >= 0:
            self.nObs += 2
        else:
            self.nObs += 1

    def EraseObservation(self, kf):                                         # MapPoint.cc:220-257
        bad = False
        if kf in self.mObservations:
            left, right = self.mObservations[kf]
            if left != -1:
                if not kf.mpCamera2 and kf.mvuRight[left] >= 0:
                    self.nObs -= 2
                else:
                    self.nObs -= 1
            if right != -1:
                self.nObs -= 1
            del self.mObservations[kf]
            if self.nObs <= 2:
                bad = True
        if bad:
            self.SetBadFlag()

    def SetBadFlag(self):                                                   # MapPoint.cc:280-305
        self.mbBad = True
        obs = self.GetObservations()
        self.mObservations = {}
        for kf, (left, right) in obs:
            if left != -1:
                kf.EraseMapPointMatch(left)
            if right != -1:
                kf.EraseMapPointMatch(right)


def link(kf, idx, mp):
    """kf->AddMapPoint(mp, idx); mp->AddObservation(kf, idx): the pair every call site of the reference makes."""
    kf.mvpMapPoints[idx] = mp
    mp.AddObservation(kf, idx)


def candidate_level(kf, i):
    """:1303-1305 with the deviation of the module docstring: slot i of the stacked row."""
    return kf.octaves[i]


def observer_level(kf, left, right):                                        # :1316-1328
    level = -1
    if kf.NLeft == -1:
        return kf.octaves[left]
    if left != -1:
        level = kf.octaves[left]
    if right != -1:
        rl = kf.octaves[right]                                              # mvKeysRight[rightIndex - NLeft] = slot rightIndex of the stacked row
        level = rl if (level == -1 or level > rl) else level
    return level


def count_candidate(kf, monocular, th_obs=3):
    """The body of the loop for one candidate, :1275-1347 -> (nMPs, nRedundantObservations, per-slot state 0 / 1 / 2)."""
    vp = kf.GetMapPointMatches()
    n_mps = n_red = 0
    state = [0] * len(vp)
    for i, mp in enumerate(vp):
        if mp is None or mp.isBad():
            continue
        if not monocular:
            if kf.mvDepth[i] > kf.mThDepth or kf.mvDepth[i] < 0:
                continue
        n_mps += 1
        state[i] = 1
        if mp.Observations() > th_obs:
            level = candidate_level(kf, i)
            n = 0
            for kfi, (left, right) in mp.GetObservations():
                if kfi is kf:
                    continue
                if observer_level(kfi, left, right) <= level + 1:
                    n += 1
                    if n > th_obs:
                        break
            if n > th_obs:
                n_red += 1
                state[i] = 2
    return n_mps, n_red, state


def voted_out(n_red, n_mps, redundant_th):
    """:1349: int > float * int, all of it in float."""
    return bool(np.float32(n_red) > np.float32(redundant_th) * np.float32(n_mps))


def KeyFrameCulling(covisible, monocular, redundant_th=0.9, abort_ba=lambda: False, on_redundant=None, th_obs=3):
    """:1266-1399.  covisible = GetVectorCovisibleKeyFrames(); on_redundant(kf) is :1350-1392 and returns False where the reference
    `continue`s (:1356, :1359), the default is the non-inertial branch.  Returns one record per KeyFrame that was counted."""
    log = []
    count = 0
    for kf in covisible:
        count += 1
        if kf.mnId == kf.map.GetInitKFid() or kf.isBad():
            continue
        n_mps, n_red, state = count_candidate(kf, monocular, th_obs)
        cull = voted_out(n_red, n_mps, redundant_th)
        rec = {"kf": kf, "n_mps": n_mps, "n_redundant": n_red, "cull": cull, "state": state, "erased": False}
        log.append(rec)
        if cull:
            if on_redundant is None:
                kf.SetBadFlag()
                through = True
            else:
                through = on_redundant(kf)
            rec["erased"] = kf.isBad()
            if not through:
                continue
        if (count > 20 and abort_ba()) or count > 100:
            break
    return log


# ---- the flatten of facade/KeyFrameCulling.h -------------------------------------------------------------------------------
def candidates(covisible):
    """The KeyFrames of the first chunk the facade hands to the library: the skips of :1272, up to and including the first KeyFrame
    whose count is above 100."""
    out, count = [], 0
    for kf in covisible:
        count += 1
        if kf.mnId == kf.map.GetInitKFid() or kf.isBad():
            continue
        out.append(kf)
        if count > 100:
            break
    return out


def flatten(cands, monocular):
    """Pool rows: the candidates in order, then every other observing KeyFrame in the order it is met; the MapPoint list: the order in
    which the candidates' slots meet them.  Entries per MapPoint in map order, left before right; flags bit 0 right, bit 1 the KeyFrame
    isBad(), bit 2 the entry weighs 2.  A bad MapPoint has an empty list."""
    rows, row_of, mps, mp_of = [], {}, [], {}

    def row_for(kf):
        if kf not in row_of:
            row_of[kf] = len(rows)
            rows.append(kf)
        return row_of[kf]

    for kf in cands:
        row_for(kf)
    cand_row = [row_of[kf] for kf in cands]
    off, orow, oslot, oflags, valid, nobs = [0], [], [], [], [], []
    kf_mp_rows = []
    for kf in cands:
        r = []
        for mp in kf.GetMapPointMatches():
            if mp is None:
                r.append(-1)
                continue
            if mp not in mp_of:
                mp_of[mp] = len(mps)
                mps.append(mp)
                valid.append(0 if mp.isBad() else 1)
                nobs.append(mp.Observations())
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
        kf_mp_rows.append(r)
    cap = max([1] + [kf.N for kf in rows])
    octave = np.full((len(rows), cap), -1, np.int32)
    counts = np.zeros(len(rows), np.int32)
    for i, kf in enumerate(rows):
        counts[i] = kf.N
        octave[i, :kf.N] = kf.octaves
    kf_mp = np.full((len(cands), cap), -1, np.int32)
    depth = None if monocular else np.full((len(cands), cap), -1.0, np.float32)
    for k, kf in enumerate(cands):
        kf_mp[k, :kf.N] = kf_mp_rows[k]
        if depth is not None:
            depth[k, :kf.N] = np.array(kf.mvDepth, np.float32)
    return {"rows": rows, "mps": mps, "cand_row": np.array(cand_row, np.int32), "octave": octave, "counts_kf": counts, "kf_mp": kf_mp,
            "depth": depth, "th_depth": np.float32(cands[0].mThDepth) if cands else np.float32(0),
            "obs_off": np.array(off, np.int32), "obs_row": np.array(orow, np.int32), "obs_slot": np.array(oslot, np.int32),
            "obs_flags": np.array(oflags, np.uint8), "mp_valid": np.array(valid, np.uint8), "mp_nobs": np.array(nobs, np.int32), "cap": cap}


# ---- the call contract of include/orbm.h -----------------------------------------------------------------------------------
def _entries(j, counts_kf, cap, obs_off, obs_row, obs_slot, nobs):
    """The live entries of MapPoint j after the skip rules -> list of (position in the CSR, row)."""
    a, b = int(obs_off[j]), int(obs_off[j + 1])
    if a < 0 or b > nobs or b <= a or b - a > MP_MAX_OBS:
        return []
    out = []
    for e in range(a, b):
        r, s = int(obs_row[e]), int(obs_slot[e])
        if r < 0 or r >= len(counts_kf) or s < 0 or s >= min(int(counts_kf[r]), cap):
            out.append((e, None))
        else:
            out.append((e, r))
    return out


def contract(cand_row, octave, counts_kf, kf_mp, depth, th_depth, obs_off, obs_row, obs_slot, obs_flags, mp_valid, mp_nobs, erased=None,
             th_obs=3, redundant_th=0.9):
    """orbm_keyframe_culling on numpy arrays; octave [nkf_rows][cap] stands for kps_kf[..].octave."""
    octave = np.asarray(octave)
    nrows, cap = octave.shape
    ncand, nmp, nobs = len(cand_row), len(mp_nobs), len(obs_row)
    n_mps = np.zeros(ncand, np.int32); n_red = np.zeros(ncand, np.int32); cull = np.zeros(ncand, np.uint8)
    state = np.zeros((ncand, cap), np.uint8)
    gone = (lambda r: False) if erased is None else (lambda r: bool(erased[r]))
    th_depth = np.float32(th_depth)
    for k in range(ncand):
        r = int(cand_row[k])
        if r < 0 or r >= nrows or gone(r):
            continue
        for i in range(min(int(counts_kf[r]), cap)):
            j = int(kf_mp[k][i])
            if j < 0 or j >= nmp or (mp_valid is not None and not mp_valid[j]):
                continue
            ents = _entries(j, counts_kf, cap, obs_off, obs_row, obs_slot, nobs)
            lost = [e for e, row in ents if row is not None and gone(row)]
            eff = int(mp_nobs[j]) - sum(2 if obs_flags[e] & 4 else 1 for e in lost)
            if lost and eff <= 2:
                continue
            if depth is not None:
                d = np.float32(depth[k][i])
                if d > th_depth or d < 0:
                    continue
            n_mps[k] += 1
            state[k, i] = 1
            if eff > th_obs:
                L = int(octave[r, i])
                n = 0
                passes = {}
                for pos, (e, row) in enumerate(ents):
                    if row is None or gone(row) or row == r:
                        continue
                    ok = int(octave[row, int(obs_slot[e])]) <= L + 1
                    passes[pos] = ok
                    if not ok:
                        continue
                    if obs_flags[e] & 1 and pos > 0:
                        pe, prow = ents[pos - 1]
                        if prow == row and not (obs_flags[pe] & 1) and passes.get(pos - 1, False):
                            continue                                          # one KeyFrame with its left entry, already counted there
                    n += 1
                if n > th_obs:
                    n_red[k] += 1
                    state[k, i] = 2
        cull[k] = 1 if np.float32(n_red[k]) > np.float32(redundant_th) * np.float32(n_mps[k]) else 0
    hit = np.flatnonzero(cull)
    return {"n_mps": n_mps, "n_redundant": n_red, "cull": cull, "slot_state": state, "first_cull": int(hit[0]) if len(hit) else -1}


def sequential_by_contract(F, cands, decide, call=contract, th_obs=3, redundant_th=0.9):
    """The sequential rule of include/orbm.h on the arrays F of flatten(): call, trust candidates 0 .. first_cull, let decide(kf) do
    :1350-1392 (it returns whether the KeyFrame isBad() afterwards), set erased[row] and call again for the rest.  Returns one record
    per candidate in order: (n_mps, n_redundant, cull, slot_state row)."""
    erased = np.zeros(len(F["rows"]), np.uint8)
    out, start = [], 0
    while start < len(cands):
        res = call(F["cand_row"][start:], F["octave"], F["counts_kf"], F["kf_mp"][start:], None if F["depth"] is None else F["depth"][start:],
                   F["th_depth"], F["obs_off"], F["obs_row"], F["obs_slot"], F["obs_flags"], F["mp_valid"], F["mp_nobs"],
                   erased if erased.any() else None, th_obs, redundant_th)
        fc = res["first_cull"]
        last = len(cands) - start - 1 if fc < 0 else fc
        for k in range(last + 1):
            out.append((int(res["n_mps"][k]), int(res["n_redundant"][k]), int(res["cull"][k]), res["slot_state"][k].copy()))
        if fc < 0:
            break
        if decide(cands[start + fc]):
            erased[F["cand_row"][start + fc]] = 1
        start += fc + 1
    return out
