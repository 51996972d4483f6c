"""A second, independent reading of the two Frame-side producers that feed the matcher searches, in plain Python / numpy / mpmath:
Frame::ComputeBoW (DBoW2's TemplatedVocabulary::transform) and Frame::isInFrustum + MapPoint::PredictScale.

Written from the reference alone -- Thirdparty/DBoW2/DBoW2/{TemplatedVocabulary.h, BowVector.cpp, FeatureVector.cpp, FORB.cpp}, Frame.cc,
MapPoint.cc, CameraModels/Pinhole.cpp -- it imports no product code and no oracle.  One reference function is one function here and cites
the lines it restates; each returns a collections.Counter of the branches it took, as tests/second_reading.py does.

FORB::distance (FORB.cpp:81-101) is the loop of ORBmatcher::DescriptorDistance (ORBmatcher.cc:2911-2931) line for line -- eight 32-bit
words, v = a ^ b, the same three SWAR lines with the same masks, `>> 24`, summed into an int -- so second_reading.descriptor_distance is
reused for it.

DBoW2 arithmetic is double and Python floats are IEEE doubles: with the reference's summation order kept, BowVector values are bit-exact.

isInFrustum arithmetic follows the C++ operand types: every float operation is one np.float32 operation (no contraction).  The cv::Matx
expressions are restated from the rule DESIGN.md section 2 and include/orbm.h state, because OpenCV's headers are not part of the
reference tree and are not available to this file's author: Matx * Matx accumulates `s += a(i, k) * b(k, j)` in float from s = 0 in k
order, Matx + Matx is one float add per element, Matx::dot accumulates in float from 0, cv::norm(Matx) accumulates the squares in a
double that starts at 0, takes the double sqrt, and the assignment to `const float` narrows it.

Where the reference is undefined, the reading says so instead of guessing:
  * transform(feature, ..., &nid, levelsup) leaves *nid unwritten when a leaf ends the descent above nid_level (:1251 never fires):
    transform_one returns nid = None and counts `nid_unwritten`; transform() files such a feature under the `unwritten_nid` its caller
    hands in (include/orbm.h documents 0).
  * loadFromTextFile's `while(!f.eof())` (:1378) goes round once more on the empty string after a final newline and builds a node from
    values it never read: vocab_from_text counts `trailing_empty_line` and ends there, as the project's loaders do.
  * PredictScale converts ceil(log(ratio) / logScaleFactor) to int (:733); for ratio <= 0, a non-finite ratio or logScaleFactor == 0
    the operand is not finite and the conversion is undefined: predict_scale returns level None and counts `level_undefined`.
"""
import math
from collections import Counter

import mpmath
import numpy as np

from second_reading import F, descriptor_distance

MP_DIGITS = 60                                   # PredictScale's quotient is evaluated to this many decimal digits

# PredictScale's ambiguity band.  The reference computes ceil(logf(ratio) / logScaleFactor) in float, the product
# ceil((float)log((double)ratio) / logScaleFactor).  Against the exact q = log(ratio) / logScaleFactor (ratio and logScaleFactor the
# float32 values both sides hold), either side carries
#     the logarithm: at most 1 ulp of its result (glibc documents logf within 1 ulp; a double log narrowed to float is within 0.5 ulp
#                    and a little), and 1 ulp(x) <= 2**-23 |x|                                          -> relative 2 * 2**-24
#     the division:  correctly rounded, half an ulp                                                      -> relative 1 * 2**-24
# so the computed quotient is q (1 + e) with |e| <= 3 * 2**-24 = 1.5 * 2**-23 to first order, and its ceil can differ from ceil(q) only
# if an integer m lies within 1.5 * 2**-23 |q| of q.  Twice that, rounded up to a whole factor, is 4 * 2**-23; max(|q|, 1) keeps the
# band from collapsing around m = 0, where it is wider than the error needs.
AMBIGUITY_FACTOR = 4
AMBIGUITY_UNIT = 2.0 ** -23

FRUSTUM_BRANCHES = ("PcZ_negative", "u_below_minX", "u_above_maxX", "v_below_minY", "v_above_maxY", "dist_below_min", "dist_above_max",
                    "viewCos_below_limit", "in_view")
# further counters mark an edge that was hit exactly or a case worth proving: u_on_minX, u_on_maxX, v_on_minY, v_on_maxY, dist_on_min,
# dist_on_max, viewCos_on_limit, PcZ_zero, PcZ_subnormal, projection_non_finite, proj_kept_after_reject, ambiguous_level,
# ratio_one_exact, clamped_low, clamped_high, level_undefined


# ---------------------------------------------------------------------------------------------------------------------------
# DBoW2
# ---------------------------------------------------------------------------------------------------------------------------
class Node:
    """TemplatedVocabulary::Node (TemplatedVocabulary.h:297-329)."""
    __slots__ = ("id", "parent", "children", "descriptor", "weight", "word_id")

    def __init__(self, nid):
        self.id, self.parent, self.children, self.descriptor, self.weight, self.word_id = nid, 0, [], None, 0.0, 0

    def is_leaf(self):                                                       # :328, `children.empty()`
        return not self.children


class Vocabulary:
    def __init__(self, k, L, scoring, weighting):
        self.k, self.L, self.scoring, self.weighting = k, L, scoring, weighting
        self.nodes = [Node(0)]                                               # :1376-1377
        self.words = []                                                      # node ids, in word-id order

    def info(self):
        return dict(k=self.k, L=self.L, nnodes=len(self.nodes), nwords=len(self.words))


def _add_node(voc, pid, n_is_leaf, descriptor, weight, t):
    """One pass of the loop at :1385-1419."""
    nid = len(voc.nodes)                                                     # :1385
    nd = Node(nid); voc.nodes.append(nd)                                     # :1386-1387
    nd.parent = pid                                                          # :1391
    voc.nodes[pid].children.append(nid)                                      # :1392, children in file order
    nd.descriptor = np.array(descriptor, np.uint8).reshape(32)               # :1404
    nd.weight = float(weight)                                                # :1406
    if n_is_leaf > 0:                                                        # :1408
        nd.word_id = len(voc.words)                                          # :1410-1413, word ids in leaf order
        voc.words.append(nid)
        t["word"] += 1
    else:
        t["inner_node"] += 1


def vocab_from_text(path):
    """TemplatedVocabulary::loadFromTextFile, TemplatedVocabulary.h:1338-1424.  Returns (Vocabulary, branches); a header outside :1359's
    ranges raises ValueError, where the reference returns false."""
    t = Counter()
    with open(path) as f:
        lines = f.read().split("\n")                                         # getline's view of the file: the text between newlines
    k, L, n1, n2 = (int(x) for x in lines[0].split()[:4])                    # :1350-1357
    if k < 0 or k > 20 or L < 1 or L > 10 or n1 < 0 or n1 > 5 or n2 < 0 or n2 > 3:      # :1359
        raise ValueError("Vocabulary loading failure: This is not a correct text file!")
    voc = Vocabulary(k, L, n1, n2)                                           # :1365-1366
    for i, s in enumerate(lines[1:]):                                        # :1378
        if s == "":
            if i == len(lines) - 2:
                t["trailing_empty_line"] += 1                                # see the module docstring
                break
            raise ValueError("empty line inside the vocabulary")
        tok = s.split()
        _add_node(voc, int(tok[0]), int(tok[1]), [int(x) for x in tok[2:34]], float(tok[34]), t)
    return voc, t


def vocab_from_arrays(k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
    """What loadFromTextFile builds from a file whose line i - 1 is `parent[i] is_leaf[i] desc[i] weight[i]` (node 0 is the root)."""
    t = Counter()
    voc = Vocabulary(k, L, scoring, weighting)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    for nid in range(1, len(parent)):
        assert 0 <= int(parent[nid]) < nid
        _add_node(voc, int(parent[nid]), int(is_leaf[nid]), desc[nid], float(weight[nid]), t)
    return voc, t


def transform_one(voc, feature, levelsup, t=None):
    """TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup), :1217-1259.  Returns (word_id, weight, nid, branches);
    nid is None where the reference leaves *nid unwritten."""
    t = Counter() if t is None else t
    nid = None
    nid_level = voc.L - levelsup                                             # :1226
    if nid_level <= 0:                                                       # :1227
        nid = 0
        t["nid_root"] += 1
    final_id = 0                                                             # :1229
    current_level = 0                                                        # :1230
    while True:                                                              # :1232
        current_level += 1                                                   # :1234
        nodes = voc.nodes[final_id].children                                 # :1235
        t[("children", len(nodes))] += 1
        final_id = nodes[0]                                                  # :1236
        best_d = descriptor_distance(feature, voc.nodes[final_id].descriptor)            # :1238
        best_pos, ties = 0, []
        for pos in range(1, len(nodes)):                                     # :1240
            d = descriptor_distance(feature, voc.nodes[nodes[pos]].descriptor)           # :1243
            if d < best_d:                                                   # :1244, strict: the earlier child keeps a tie
                best_d = d; final_id = nodes[pos]; best_pos, ties = pos, []
            elif d == best_d:
                ties.append(pos)
        t[("winner", best_pos)] += 1
        t[("best_d", best_d)] += 1
        for pos in ties:
            t[("tie", best_pos, pos)] += 1
        if current_level == nid_level:                                       # :1251
            nid = final_id
            t["nid_written"] += 1
        if voc.nodes[final_id].is_leaf():                                    # :1254
            break
    t[("leaf_depth", current_level)] += 1
    if nid is None:
        t["nid_unwritten"] += 1
    return voc.nodes[final_id].word_id, voc.nodes[final_id].weight, nid, t   # :1257-1258


def bow_and_feature_vector(word_ids, nids, weights, t=None):
    """The loop body and the tail of transform(features, v, fv, levelsup) for weighting TF_IDF, scoring L1_NORM: :1157-1161, :1193.
    Returns (bow ids, bow values, [(node id, [features])], branches)."""
    t = Counter() if t is None else t
    v, fv = {}, {}
    for i_feature, (wid, nid, w) in enumerate(zip(word_ids, nids, weights)):
        w = float(w)
        if w > 0:                                                            # :1157, not stopped
            if wid in v:                                                     # BowVector::addWeight, BowVector.cpp:34-46
                v[wid] = v[wid] + w                                          # :40, in feature order
                t["addWeight_accumulate"] += 1
            else:
                v[wid] = w                                                   # :44
                t["addWeight_insert"] += 1
            fv.setdefault(int(nid), []).append(i_feature)                    # FeatureVector::addFeature, FeatureVector.cpp:31-45
        else:
            t["stopped_zero" if w == 0 else ("stopped_negative" if w < 0 else "stopped_nan")] += 1
    ids = sorted(v)                                                          # std::map: ascending word id
    norm = 0.0                                                               # BowVector::normalize(L1), BowVector.cpp:62-84
    for wid in ids:
        norm += math.fabs(v[wid])                                            # :70, in ascending word id
    if norm > 0.0:                                                           # :79
        vals = [v[wid] / norm for wid in ids]                                # :82
        t["normalized"] += 1
    else:
        vals = [v[wid] for wid in ids]
        t["norm_zero_no_division"] += 1
    return np.array(ids, np.int32), np.array(vals, np.float64), [(nid, fv[nid]) for nid in sorted(fv)], t


def transform(voc, features, levelsup, unwritten_nid=None):
    """TemplatedVocabulary::transform(features, v, fv, levelsup), :1126-1194, for the header `0 0` (weighting TF_IDF: the branch at
    :1145; scoring L1_NORM: mustNormalize gives true and L1, so :1164-1170 is skipped and :1193 normalises).
    Returns (bow ids, bow values, feature vector, word ids, node ids (None = unwritten), weights, branches)."""
    assert voc.scoring == 0 and voc.weighting == 0, "only the header `0 0` is restated"
    t = Counter()
    features = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
    words, nids, weights = [], [], []
    for fit in features:                                                     # :1148
        wid, w, nid, _ = transform_one(voc, fit, levelsup, t)                # :1155
        words.append(wid); nids.append(nid); weights.append(w)
    filed = []
    for nid, w in zip(nids, weights):
        if nid is None:
            if w > 0:
                assert unwritten_nid is not None, "an unwritten node id reaches the FeatureVector: the reference reads an uninitialised value"
                t["nid_unwritten_filed"] += 1
            filed.append(unwritten_nid if unwritten_nid is not None else -1)
        else:
            filed.append(nid)
    ids, vals, fv, _ = bow_and_feature_vector(words, filed, weights, t)
    return ids, vals, fv, np.array(words, np.int32), nids, np.array(weights, np.float64), t


# ---------------------------------------------------------------------------------------------------------------------------
# MapPoint::PredictScale(const float&, Frame*), MapPoint.cc:725-740
# ---------------------------------------------------------------------------------------------------------------------------
def scale_quotient(ratio, log_scale_factor):
    """q = log(ratio) / logScaleFactor from the two float32 values, to MP_DIGITS digits; None where it is not finite."""
    r, l = float(F(ratio)), float(F(log_scale_factor))
    if not (math.isfinite(r) and r > 0.0 and math.isfinite(l) and l != 0.0):
        return None
    with mpmath.workdps(MP_DIGITS):
        return mpmath.log(mpmath.mpf(r)) / mpmath.mpf(l)


def predict_scale(max_distance, current_dist, log_scale_factor, n_scale_levels, t=None):
    """Returns (level, ambiguous, q, branches).  level = clamp(ceil(q), 0, nlevels - 1) from the exact q; `ambiguous` says that a
    float evaluation of :733 may legitimately land on the other side of the integer next to q (see AMBIGUITY_FACTOR)."""
    t = Counter() if t is None else t
    with np.errstate(all="ignore"):
        ratio = F(F(max_distance) / F(current_dist))                         # :730
    q = scale_quotient(ratio, log_scale_factor)
    if q is None:
        t["level_undefined"] += 1
        return None, False, None, t
    with mpmath.workdps(MP_DIGITS):
        n_scale = int(mpmath.ceil(q))                                        # :733
        m = int(mpmath.nint(q))
        near = abs(q - m) <= AMBIGUITY_FACTOR * AMBIGUITY_UNIT * max(abs(q), 1)
    ambiguous = bool(near) and 0 <= m <= n_scale_levels - 2                  # at any other m both sides clamp to the same level
    if float(ratio) == 1.0:
        # log(1) is +0 exactly in every libm (C Annex F) and 0 / logScaleFactor is 0: q == 0 is computed without error on both sides.
        # It is the only exact integer: log of any other float is irrational, logScaleFactor is rational.
        ambiguous = False
        t["ratio_one_exact"] += 1
    if ambiguous:
        t["ambiguous_level"] += 1
    if n_scale < 0:                                                          # :734
        n_scale = 0
        t["clamped_low"] += 1
    elif n_scale >= n_scale_levels:                                          # :736
        n_scale = n_scale_levels - 1
        t["clamped_high"] += 1
    return n_scale, ambiguous, q, t


# ---------------------------------------------------------------------------------------------------------------------------
# Frame::isInFrustum, Frame.cc:603-699 (Nleft == -1), with Pinhole::project (Pinhole.cpp:33-47)
# ---------------------------------------------------------------------------------------------------------------------------
def _matx33_times_31_plus_31(R, P, tr):
    """mRcwx * Px + mtcwx (:621): the Matx rule of the module docstring."""
    out = []
    for i in range(3):
        s = F(0)
        for k in range(3):
            s = F(s + F(F(R[3 * i + k]) * F(P[k])))
        out.append(F(s + F(tr[i])))
    return out


def _cv_norm31(v):
    """cv::norm(Matx31f) assigned to a float (:622, :653)."""
    s = 0.0
    for k in range(3):
        s += float(v[k]) * float(v[k])                                       # double products of floats are exact; the sum rounds
    return F(math.sqrt(s))


def is_in_frustum(pw, normal, min_dist, max_dist, rcw, tcw, ow, k, bounds, bf, viewing_cos_limit, log_scale_factor, n_scale_levels,
                  init=None):
    """Frame::isInFrustum for every map point in turn.  pw / normal [n][3], min_dist / max_dist = mfMinDistance / mfMaxDistance,
    rcw[9] row-major, tcw[3], ow[3], k = (fx, fy, cx, cy) = mvParameters, bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY).
    Returns (out, ambiguous, branches).  out mirrors the MapPoint members: in_view (mbTrackInView), proj_x / proj_y (-1 unless the
    bounds test passed; they stay set when a later gate rejects), and proj_xr, depth, level, view_cos, which are written only where in
    view and elsewhere keep what `init` holds (default 0, level -1).  ambiguous[i] marks a level that must not be compared."""
    pw = np.ascontiguousarray(pw, F).reshape(-1, 3); normal = np.ascontiguousarray(normal, F).reshape(-1, 3)
    n = len(pw)
    rcw = np.ascontiguousarray(rcw, F).reshape(9); tcw = np.ascontiguousarray(tcw, F).reshape(3); ow = np.ascontiguousarray(ow, F).reshape(3)
    fx, fy, cx, cy = (F(x) for x in k)
    min_x, max_x, min_y, max_y = (F(x) for x in bounds)
    bf, cos_limit = F(bf), F(viewing_cos_limit)
    t = Counter()
    out = {"in_view": np.zeros(n, np.uint8), "proj_x": np.zeros(n, F), "proj_y": np.zeros(n, F), "proj_xr": np.zeros(n, F),
           "depth": np.zeros(n, F), "level": np.full(n, -1, np.int32), "view_cos": np.zeros(n, F)}
    for key, a in (init or {}).items():
        out[key][:] = np.asarray(a)[:n]
    ambiguous = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            out["in_view"][i] = 0                                            # :609
            out["proj_x"][i] = F(-1)                                         # :610
            out["proj_y"][i] = F(-1)                                         # :611
            px = pw[i]                                                       # :615
            pc = _matx33_times_31_plus_31(rcw, px, tcw)                      # :621
            pc_dist = _cv_norm31(pc)                                         # :622
            pc_z = pc[2]                                                     # :625
            invz = F(F(1.0) / pc_z)                                          # :626
            if pc_z < F(0.0):                                                # :628
                t["PcZ_negative"] += 1
                if abs(float(pc_z)) < 2.0 ** -126: t["PcZ_subnormal"] += 1
                continue
            if pc_z == F(0.0): t["PcZ_zero"] += 1
            elif float(pc_z) < 2.0 ** -126: t["PcZ_subnormal"] += 1
            u = F(F(F(fx * pc[0]) / pc_z) + cx)                              # :631, Pinhole.cpp:35
            v = F(F(F(fy * pc[1]) / pc_z) + cy)                              # Pinhole.cpp:36
            if not (np.isfinite(u) and np.isfinite(v)): t["projection_non_finite"] += 1
            if u < min_x or u > max_x:                                       # :635, closed on both sides; false for NaN
                t["u_below_minX" if u < min_x else "u_above_maxX"] += 1
                continue
            if v < min_y or v > max_y:                                       # :637
                t["v_below_minY" if v < min_y else "v_above_maxY"] += 1
                continue
            if u == min_x: t["u_on_minX"] += 1
            if u == max_x: t["u_on_maxX"] += 1
            if v == min_y: t["v_on_minY"] += 1
            if v == max_y: t["v_on_maxY"] += 1
            out["proj_x"][i] = u                                             # :641
            out["proj_y"][i] = v                                             # :642
            max_distance = F(F(1.2) * F(max_dist[i]))                        # :647, MapPoint.cc:680
            min_distance = F(F(0.8) * F(min_dist[i]))                        # :648, MapPoint.cc:671
            po = [F(px[c] - ow[c]) for c in range(3)]                        # :651
            dist = _cv_norm31(po)                                            # :653
            if dist < min_distance or dist > max_distance:                   # :656
                t["dist_below_min" if dist < min_distance else "dist_above_max"] += 1
                t["proj_kept_after_reject"] += 1
                continue
            if dist == min_distance: t["dist_on_min"] += 1
            if dist == max_distance: t["dist_on_max"] += 1
            pn = normal[i]                                                   # :663
            dot = F(0)
            for c in range(3):
                dot = F(dot + F(po[c] * pn[c]))                              # Matx::dot
            view_cos = F(dot / dist)                                         # :667
            if view_cos < cos_limit:                                         # :670
                t["viewCos_below_limit"] += 1
                t["proj_kept_after_reject"] += 1
                continue
            if view_cos == cos_limit: t["viewCos_on_limit"] += 1
            level, amb, _, _ = predict_scale(max_dist[i], dist, log_scale_factor, n_scale_levels, t)    # :675
            ambiguous[i] = amb or level is None
            out["in_view"][i] = 1                                            # :681
            out["proj_xr"][i] = F(u - F(bf * invz))                          # :685
            out["depth"][i] = pc_dist                                        # :687
            out["level"][i] = -1 if level is None else level                 # :692
            out["view_cos"][i] = view_cos                                    # :694
            t["in_view"] += 1
    return out, ambiguous, t
