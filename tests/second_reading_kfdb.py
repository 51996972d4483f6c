"""A second, independent reading of KeyFrameDatabase's candidate queries, in plain Python on plain objects.

Written from the reference alone -- src/KeyFrameDatabase.cc (add :40-47, erase :50-70, clearMap :79-103, DetectNBestCandidates :660-866,
DetectRelocalizationCandidates :869-981) and Thirdparty/DBoW2/DBoW2/ScoringObject.cpp (L1Scoring::score :23-68) -- it imports no product
code and no oracle.  One reference function is one function here and cites the lines it restates; each counts the branches it took in a
collections.Counter, so that a test can assert that a situation was reached.

A BowVector is a std::map<WordId, double>: here two parallel sequences (ascending word ids, values), which is what iterating the map
gives.  DBoW2 arithmetic is double and Python floats are IEEE doubles; `float si = mpVoc->score(..)` narrows once, np.float32(..) here.
accScore += score, `accScore > bestAccScore` and `0.75f * bestAccScore` are float operations: one np.float32 operation each.

Where the reference does not return, the reading says so: DetectNBestCandidates' selection loop `continue`s on a bad KeyFrame without
advancing (:815-816) and spins forever; detect_n_best_candidates raises BadKeyFrameSpin there.
"""
import bisect
import math
from collections import Counter, defaultdict

import numpy as np

F = np.float32


class BadKeyFrameSpin(RuntimeError):
    """KeyFrameDatabase.cc:815-816: `if(pKFi->isBad()) continue;` inside a while loop whose increments lie below it."""


class Map:
    def __init__(self, bad=False):
        self.bad = bad

    def IsBad(self):
        return self.bad


class KeyFrame:
    """The members the two functions read and write (include/KeyFrame.h), on a plain object."""
    _next = 0

    def __init__(self, ids, vals, kf_map, bad=False):
        self.mnId = KeyFrame._next; KeyFrame._next += 1
        self.bow_ids, self.bow_vals = [int(i) for i in ids], [float(v) for v in vals]    # mBowVec in iteration order
        self.map, self.bad = kf_map, bad
        self.covisible = []                                                  # mvpOrderedConnectedKeyFrames, best first
        self.connected = set()                                               # GetConnectedKeyFrames
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = -1, 0, F(0)
        self.mnPlaceRecognitionQuery, self.mnPlaceRecognitionWords, self.mPlaceRecognitionScore = -1, 0, F(0)

    def GetMap(self):
        return self.map

    def isBad(self):
        return self.bad

    def GetBestCovisibilityKeyFrames(self, n):                               # KeyFrame.cc: the first min(n, size) of the ordered vector
        return self.covisible[:n]


class Frame:
    def __init__(self, ids, vals, frame_id):
        self.mnId = frame_id
        self.bow_ids, self.bow_vals = [int(i) for i in ids], [float(v) for v in vals]


def l1_score(ids1, vals1, ids2, vals2, t=None):
    """L1Scoring::score, ScoringObject.cpp:23-68, with its lower_bound walk.  Returns the double."""
    t = Counter() if t is None else t
    i1, i2, n1, n2 = 0, 0, len(ids1), len(ids2)                              # :29-30
    score = 0.0                                                              # :32
    while i1 != n1 and i2 != n2:                                             # :34
        vi, wi = vals1[i1], vals2[i2]                                        # :36-37
        if ids1[i1] == ids2[i2]:                                             # :39
            score += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)      # :41
            i1 += 1; i2 += 1                                                 # :44-45
            t["l1_equal"] += 1
        elif ids1[i1] < ids2[i2]:                                            # :47
            i1 = bisect.bisect_left(ids1, ids2[i2])                          # :50, v1.lower_bound
            t["l1_advance_v1"] += 1
        else:
            i2 = bisect.bisect_left(ids2, ids1[i1])                          # :56
            t["l1_advance_v2"] += 1
    score = -score / 2.0                                                     # :65
    return score


class KeyFrameDatabase:
    def __init__(self, nwords):
        self.nwords = nwords
        self.inverted = defaultdict(list)                                    # mvInvertedFile, :76: one (empty) list per word, made when first named
        self.t = Counter()

    def add(self, kf):                                                       # :40-47
        for w in kf.bow_ids:
            self.inverted[w].append(kf)

    def erase(self, kf):                                                     # :50-70
        for w in kf.bow_ids:
            l = self.inverted[w]
            for pos, other in enumerate(l):
                if other is kf:                                              # :63
                    del l[pos]
                    break

    def clear_map(self, kf_map):                                             # :79-103
        for l in self.inverted.values():
            l[:] = [kf for kf in l if kf.GetMap() is not kf_map]

    # -------------------------------------------------------------------------------------------------------------------
    def detect_relocalization_candidates(self, frame, p_map):
        """:869-981.  Returns the candidate list; self.last holds lKFsSharingWords, maxCommonWords, minCommonWords and lScoreAndMatch."""
        t = self.t
        sharing = []                                                         # :871
        for w in frame.bow_ids:                                              # :877
            for kfi in self.inverted[w]:                                     # :881
                if kfi.mnRelocQuery != frame.mnId:                           # :884
                    kfi.mnRelocWords = 0
                    kfi.mnRelocQuery = frame.mnId
                    sharing.append(kfi)                                      # :888
                kfi.mnRelocWords += 1                                        # :890
        self.last = dict(sharing=sharing, max_common=0, min_common=0, scores=[])
        if not sharing:                                                      # :894
            t["no_sharing"] += 1
            return []
        max_common = 0                                                       # :898
        for kfi in sharing:
            if kfi.mnRelocWords > max_common:                                # :901
                max_common = kfi.mnRelocWords
        min_common = int(F(max_common) * F(0.8))                             # :905, int * float -> float, then truncation
        t[("max_common", max_common)] += 1
        scores = []                                                          # :907
        for kfi in sharing:                                                  # :912
            if kfi.mnRelocWords > min_common:                                # :916, strict
                si = F(l1_score(frame.bow_ids, frame.bow_vals, kfi.bow_ids, kfi.bow_vals, t))    # :919
                kfi.mRelocScore = si                                         # :920
                scores.append((si, kfi))
                t["scored"] += 1
            else:
                t["at_or_below_min_common" if kfi.mnRelocWords == min_common else "below_min_common"] += 1
        self.last.update(max_common=max_common, min_common=min_common, scores=scores)
        if not scores:                                                       # :925
            return []
        acc = []                                                             # :928
        best_acc = F(0)
        for si, kfi in scores:                                               # :932
            best_score = si                                                  # :937
            acc_score = best_score
            best_kf = kfi
            for kf2 in kfi.GetBestCovisibilityKeyFrames(10):                 # :935, :940
                if kf2.mnRelocQuery != frame.mnId:                           # :943
                    t["neighbour_not_sharing"] += 1
                    continue
                if not any(k is kf2 for _, k in scores):
                    t["neighbour_stale_score"] += 1                          # shares words, was not scored: its old mRelocScore counts
                acc_score = F(acc_score + kf2.mRelocScore)                   # :946
                if kf2.mRelocScore > best_score:                             # :947
                    best_kf = kf2
                    best_score = kf2.mRelocScore
                    t["neighbour_is_best"] += 1
            acc.append((acc_score, best_kf))                                 # :954
            if acc_score > best_acc:                                         # :955
                best_acc = acc_score
        min_retain = F(F(0.75) * best_acc)                                   # :960
        added, out = set(), []
        for si, kfi in acc:                                                  # :964
            if si > min_retain:                                              # :967
                if kfi.GetMap() is not p_map:                                # :970
                    t["other_map"] += 1
                    continue
                if id(kfi) not in added:                                     # :972
                    out.append(kfi)
                    added.add(id(kfi))
                else:
                    t["duplicate"] += 1
            else:
                t["cut_by_075"] += 1
        return out

    # -------------------------------------------------------------------------------------------------------------------
    def detect_n_best_candidates(self, kf, n_candidates):
        """:660-866.  Returns (vpLoopCand, vpMergeCand)."""
        t = self.t
        sharing = []                                                         # :663
        connected = kf.connected                                             # :672
        for w in kf.bow_ids:                                                 # :675
            for kfi in self.inverted[w]:                                     # :679
                if kfi.mnPlaceRecognitionQuery != kf.mnId:                   # :687
                    kfi.mnPlaceRecognitionWords = 0                          # :690
                    if kfi not in connected:                                 # :692
                        kfi.mnPlaceRecognitionQuery = kf.mnId
                        sharing.append(kfi)                                  # :697
                    else:
                        t["excluded_connected"] += 1
                kfi.mnPlaceRecognitionWords += 1                             # :701
        self.last = dict(sharing=sharing, max_common=0, min_common=0, scores=[])
        loop, merge = [], []
        if not sharing:                                                      # :712
            t["no_sharing"] += 1
            return loop, merge
        max_common = 0                                                       # :717
        for kfi in sharing:
            if kfi.mnPlaceRecognitionWords > max_common:
                max_common = kfi.mnPlaceRecognitionWords
        min_common = int(F(max_common) * F(0.8))                             # :724
        t[("max_common", max_common)] += 1
        scores = []
        for kfi in sharing:                                                  # :735
            if kfi.mnPlaceRecognitionWords > min_common:                     # :739
                si = F(l1_score(kf.bow_ids, kf.bow_vals, kfi.bow_ids, kfi.bow_vals, t))      # :743
                kfi.mPlaceRecognitionScore = si
                scores.append((si, kfi))
                t["scored"] += 1
            else:
                t["at_or_below_min_common" if kfi.mnPlaceRecognitionWords == min_common else "below_min_common"] += 1
        self.last.update(max_common=max_common, min_common=min_common, scores=scores)
        if not scores:                                                       # :751
            return loop, merge
        acc = []
        best_acc = F(0)
        for si, kfi in scores:                                               # :760
            best_score = si
            acc_score = best_score
            best_kf = kfi
            for kf2 in kfi.GetBestCovisibilityKeyFrames(10):                 # :765, :773
                if kf2.mnPlaceRecognitionQuery != kf.mnId:                   # :777
                    t["neighbour_not_sharing"] += 1
                    continue
                if not any(k is kf2 for _, k in scores):
                    t["neighbour_stale_score"] += 1
                acc_score = F(acc_score + kf2.mPlaceRecognitionScore)        # :780
                if kf2.mPlaceRecognitionScore > best_score:                  # :782
                    best_kf = kf2
                    best_score = kf2.mPlaceRecognitionScore
                    t["neighbour_is_best"] += 1
            acc.append((acc_score, best_kf))                                 # :790
            if acc_score > best_acc:
                best_acc = acc_score
        acc = stable_sort_comp_first(acc)                                    # :798, list::sort(compFirst) is stable
        added = set()
        i = 0
        while i < len(acc) and (len(loop) < n_candidates or len(merge) < n_candidates):       # :810
            kfi = acc[i][1]
            if kfi.isBad():                                                  # :815-816
                raise BadKeyFrameSpin("DetectNBestCandidates never advances past a bad KeyFrame")
            if id(kfi) not in added:                                         # :819
                if kf.GetMap() is kfi.GetMap() and len(loop) < n_candidates:             # :822
                    loop.append(kfi)
                elif kf.GetMap() is not kfi.GetMap() and len(merge) < n_candidates and not kfi.GetMap().IsBad():      # :828
                    merge.append(kfi)
                else:
                    t["not_taken"] += 1
                added.add(id(kfi))                                           # :834
            else:
                t["duplicate"] += 1
            i += 1
        return loop, merge


def stable_sort_comp_first(pairs):
    """std::list::sort(compFirst), compFirst(a, b) = a.first > b.first (KeyFrameDatabase.h): a stable merge sort, descending by score.
    An insertion sort that moves an element left only past strictly smaller firsts is the same permutation."""
    out = []
    for p in pairs:
        pos = len(out)
        while pos > 0 and p[0] > out[pos - 1][0]:
            pos -= 1
        out.insert(pos, p)
    return out


# -----------------------------------------------------------------------------------------------------------------------
# what the device query reports, derived from the objects above only (no arrays, no sorting by key)
# -----------------------------------------------------------------------------------------------------------------------
def query_rows(db, rows, query, exclude=None, place=False):
    """Runs the walk for `query` (a Frame, or a KeyFrame with place=True) over the database db whose add order is `rows`, and reports it in
    the eight outputs of the device query: per row common / first_word / score / scored, and max_common, min_common, nsharing, nscored.
    The sharing list's order is returned as row indices in `order`."""
    if place:
        saved = query.connected
        query.connected = set() if exclude is None else {rows[r] for r in range(len(rows)) if exclude[r]}
        try:
            db.detect_n_best_candidates(query, 0)
        finally:
            query.connected = saved
    else:
        db.detect_relocalization_candidates(query, None)
    last = db.last
    index = {id(kf): r for r, kf in enumerate(rows)}
    n = len(rows)
    common, first, score, scored = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    for kf in last["sharing"]:
        r = index[id(kf)]
        common[r] = kf.mnPlaceRecognitionWords if place else kf.mnRelocWords
        for w in query.bow_ids:                                              # the word at which the walk pushed it: the first it shares
            if any(k is kf for k in db.inverted[w]):
                first[r] = w
                break
    for si, kf in last["scores"]:
        r = index[id(kf)]
        score[r] = si; scored[r] = 1
    return dict(common=common, first_word=first, score=score, scored=scored, max_common=last["max_common"], min_common=last["min_common"],
                nsharing=len(last["sharing"]), nscored=len(last["scores"]), order=[index[id(kf)] for kf in last["sharing"]])
