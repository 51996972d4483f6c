"""The device forms of Frame::ComputeBoW and Frame::isInFrustum against the second reading of the reference
(tests/second_reading_frame.py), bit for bit and with no oracle in between, on the case sets of tests/frame_cases.py.

BoW: orbm_bow_transform + orbm_bow_vectors (pkg.ORBVocabulary), orbm_bow_transform_batch_async and orbm_bow_nodes_batch_async -- all
k_bow_transform2 -- on trees with 17, 20 and 31 children per node (the second chunk of 16 lanes, the first-minimum rule across the chunk
seam, the 5-bit child index), nodes of 16 and of 1 child, leaves at depths 1, 2 and 3 side by side, descriptor counts that leave the last
wave and workgroup partly dead, every levelsup from 0 to beyond L, stopped words, and sums whose order is visible in the doubles.
Frustum: orbm_is_in_frustum in ORBM_HOST and ORBM_DEVICE -- k_frustum -- on points constructed ON each closed gate edge and one ulp beyond
it, PcZ around zero, and PredictScale ratios just outside the band in which a float logarithm may legitimately land on either side."""
import ctypes as C

import numpy as np
import pytest

import frame_cases as fc
import second_reading_frame as srf
from test_second_reading_frame_cpu import bow_arrays, bow_reading, check_frustum_expectations, compare_frustum, fv_csr, nodes_as_documented

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID = -2
SENT_I, SENT_D, SENT_F = -12345, -777.25, F(-777.25)


@pytest.fixture(scope="module")
def m(pkg):
    return pkg.ORBmatcher(0.7)


def _guarded(pkg, n, dtype, value):
    """A device array of n + 2 entries filled with a sentinel; the call gets the address of entry 1."""
    b = pkg.DeviceBuffer((n + 2) * np.dtype(dtype).itemsize)
    b.upload(np.full(n + 2, value, dtype))
    return b


def _inner(b, n, dtype, value, what):
    a = b.download(dtype, n + 2)
    assert a[0] == value and a[-1] == value, what + ": an entry outside the call was written"
    return a[1:-1]


def _three_forms(pkg, m, voc, rows, lu):
    """(word, node, weight) of `rows` from the host form, checked equal to both batched device forms; and the host form's vectors."""
    L, n = m.L, len(rows)
    bow, fv, w, nd, wt = voc.transform(rows, lu)
    dd = pkg.DeviceBuffer(rows.nbytes).upload(rows)
    dw, dn, dwt, dn2 = _guarded(pkg, n, np.int32, SENT_I), _guarded(pkg, n, np.int32, SENT_I), _guarded(pkg, n, np.float64, SENT_D), _guarded(pkg, n, np.int32, SENT_I)
    assert L.orbm_bow_transform_batch_async(m.h, voc.h, dd.ptr, n, lu, dw.ptr + 4, dn.ptr + 4, dwt.ptr + 8) == 0, L.orbm_last_error()
    assert L.orbm_bow_nodes_batch_async(m.h, voc.h, dd.ptr, n, lu, dn2.ptr + 4) == 0, L.orbm_last_error()
    m.sync()
    what = "levelsup %d, %d rows" % (lu, n)
    bw, bn, bwt, bn2 = _inner(dw, n, np.int32, SENT_I, what), _inner(dn, n, np.int32, SENT_I, what), _inner(dwt, n, np.float64, SENT_D, what), _inner(dn2, n, np.int32, SENT_I, what)
    assert np.array_equal(bw, w) and np.array_equal(bn, nd) and bwt.tobytes() == wt.tobytes(), what + ": orbm_bow_transform_batch_async differs from orbm_bow_transform"
    assert np.array_equal(bn2, nd), what + ": orbm_bow_nodes_batch_async differs from orbm_bow_transform"
    return bow, fv, w, nd, wt


def _same_as_reading(what, got, w, nids, wt):
    """got = _three_forms(...) on a prefix; w / nids / wt = the reading's rows of the same prefix."""
    (bi, bv), (fn, fs, fi), gw, gnd, gwt = got
    want_nd = nodes_as_documented(nids)
    assert np.array_equal(gw, w), (what, "word", np.nonzero(gw != w)[0][:8])
    assert np.array_equal(gnd, want_nd), (what, "node", np.nonzero(gnd != want_nd)[0][:8], gnd[gnd != want_nd][:8], want_nd[gnd != want_nd][:8])
    assert gwt.tobytes() == wt.tobytes(), (what, "weight")
    ids, vals, fv, t = srf.bow_and_feature_vector(w, want_nd, wt)
    assert np.array_equal(bi, ids) and bv.tobytes() == vals.tobytes(), (what, "BowVector")
    rn, rs, ri = fv_csr(fv)
    assert np.array_equal(fn, rn) and np.array_equal(fs, rs) and np.array_equal(fi, ri), (what, "FeatureVector")
    return t


@pytest.mark.parametrize("name", fc.TREE_NAMES)
def test_bow_three_device_forms_equal_second_reading(pkg, m, name):
    tree = fc.bow_tree(name)
    voc_r, rows, by_lu = bow_reading(name)
    voc = pkg.ORBVocabulary(m, tree)
    assert voc.info() == voc_r.info()
    unwritten = 0
    for lu, (ids, vals, fv, w, nids, wt, t) in by_lu.items():
        for n in fc.COUNTS + (len(rows),):
            if n > len(rows):
                continue
            seen = _same_as_reading("%s, levelsup %d, %d rows" % (tree["name"], lu, n), _three_forms(pkg, m, voc, rows[:n], lu), w[:n], nids[:n], wt[:n])
            if tree["name"] == "hand_stopped":
                assert seen["norm_zero_no_division"] == 1 and seen["addWeight_insert"] == 0       # every word stopped: empty vectors, no division
        unwritten += t["nid_unwritten"]
    if tree["name"] == "hand":                                               # a leaf above nid_level: the documented node 0 (checked above, row by row)
        assert unwritten > 0
    assert len(rows) > 67 or tree["name"] == "identical"


def test_bow_text_file_builds_the_same_device_tree(pkg, m, tmp_path):
    """orbm_vocab_load_text on k = 20, L = 3 (the header's largest k): the same words, nodes and weights as orbm_vocab_create's tree."""
    tree = fc.bow_tree("k20_L3")
    assert (tree["k"], tree["L"]) == (20, 3)
    voc_r, rows, by_lu = bow_reading("k20_L3")
    path = str(tmp_path / "voc.txt")
    open(path, "w").write(fc.tree_text(tree))
    assert srf.vocab_from_text(path)[0].info() == voc_r.info()
    voc = pkg.ORBVocabulary(m, path)
    assert voc.info() == voc_r.info()
    ids, vals, fv, w, nids, wt, t = by_lu[1]
    _same_as_reading("text file", _three_forms(pkg, m, voc, rows, 1), w, nids, wt)


def test_bow_node_of_32_children_is_refused(pkg, m):
    tree = fc.too_many_children_tree()
    arr = [np.ascontiguousarray(tree[k]) for k in ("parent", "is_leaf", "desc", "weight")]
    h = C.c_void_p()
    rc = m.L.orbm_vocab_create(m.h, C.byref(h), tree["k"], tree["L"], len(arr[0]), *[a.ctypes.data_as(C.c_void_p) for a in arr])
    assert rc == E_INVALID and not h.value and b"children" in m.L.orbm_last_error()
    with pytest.raises(pkg.OrbError):
        pkg.ORBVocabulary(m, tree)
    tree31 = {k: (v[:-1] if isinstance(v, np.ndarray) else v) for k, v in tree.items()}       # one child fewer loads
    assert pkg.ORBVocabulary(m, tree31).info()["nwords"] == 31


def test_bow_vectors_keep_the_order_of_both_sums(pkg):
    """40 features of one word with weights over 30 decades, between words that make the norm's order visible (the doubles of any other
    order differ: tests/test_second_reading_frame_cpu.py shows it on the same arrays)."""
    w, nd, wt = bow_arrays()
    (bi, bv), (fn, fs, fi) = pkg.bow_vectors(pkg.lib().orbm_bow_vectors, len(w), w, nd, wt)
    ids, vals, fv, t = srf.bow_and_feature_vector(w, nd, wt)
    rn, rs, ri = fv_csr(fv)
    assert np.array_equal(bi, ids) and bv.tobytes() == vals.tobytes()
    assert np.array_equal(fn, rn) and np.array_equal(fs, rs) and np.array_equal(fi, ri)


# ---------------------------------------------------------------------------------------------------------------------------
# isInFrustum
# ---------------------------------------------------------------------------------------------------------------------------
_KEYS = (("in_view", np.uint8, 200), ("proj_x", F, SENT_F), ("proj_y", F, SENT_F), ("proj_xr", F, SENT_F), ("depth", F, SENT_F),
         ("level", np.int32, SENT_I), ("view_cos", F, SENT_F))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _device_form(pkg, m, case, n):
    """orbm_is_in_frustum(ORBM_DEVICE) into sentinel-filled rows: every field of every point, and the entries on either side."""
    pw, nm, mn, mx, rcw, tcw, ow, k, bounds, bf, cos_limit, lsf, nlevels = case.args(n)
    ins = [pkg.DeviceBuffer(max(a.nbytes, 4)).upload(np.ascontiguousarray(a, F)) for a in (pw, nm, mn, mx)]
    outs = [_guarded(pkg, n, dt, v) for _, dt, v in _KEYS]
    host = [np.ascontiguousarray(a, F) for a in (rcw, tcw, ow, k, bounds)]
    rc = m.L.orbm_is_in_frustum(m.h, pkg.DEVICE, n, *[b.ptr for b in ins], *[_vp(a) for a in host], float(bf), float(cos_limit), float(lsf), int(nlevels),
                                *[b.ptr + np.dtype(dt).itemsize for b, (_, dt, _) in zip(outs, _KEYS)])
    assert rc == 0, m.L.orbm_last_error()
    m.sync()
    return {key: _inner(b, n, dt, v, case.name + " " + key) for b, (key, dt, v) in zip(outs, _KEYS)}


def _both_forms(pkg, m, case, n=None):
    """Both spaces against the reading; returns the reading's (out, ambiguous, branches) and the device outputs."""
    n = len(case.scene["pw"]) if n is None else n
    out, amb, t = case.reading(n)
    cnt, got = m.isInFrustum(*case.args(n))                                  # ORBM_HOST: the wrapper hands in zeros and level -1, the reading's defaults
    differ = compare_frustum(case.name + " (host space)", got, out, amb)
    assert cnt == t["in_view"]
    init = {key: np.full(n, v, dt) for key, dt, v in _KEYS}
    out_d, amb_d, _ = case.reading(n, init=init)                             # fields the reference does not write keep the sentinel
    dev = _device_form(pkg, m, case, n)
    assert compare_frustum(case.name + " (device space)", dev, out_d, amb_d) == differ
    assert np.array_equal(dev["level"][amb], got["level"][amb])
    return out, amb, t, got


@pytest.mark.parametrize("name", fc.FRUSTUM_NAMES)
def test_constructed_frustum_case_both_spaces_equal_second_reading(pkg, m, name):
    case = fc.frustum_case(name)
    out, amb, t, got = _both_forms(pkg, m, case)
    check_frustum_expectations(case, got, amb, t)                            # the DEVICE's outputs show the constructed outcome
    check_frustum_expectations(case, out, amb, t)


@pytest.mark.parametrize("n", fc.POINT_COUNTS + (fc.BIG,))
def test_random_scene_both_spaces_equal_second_reading(pkg, m, n):
    case = fc.FrustumCase("random %d" % n, fc.random_scene(n, 100 + n))
    out, amb, t, got = _both_forms(pkg, m, case)
    if n == fc.BIG:
        assert amb.sum() <= 0.001 * n and all(t[b] > 0 for b in srf.FRUSTUM_BRANCHES)
        # sanity bound, independent of the product rule: accepted projections within the expression's rounding margin of the exact value
        u, v, mu, mv = fc.exact_projection(case)
        s = (got["in_view"] == 1) & np.isfinite(mu)
        assert s.sum() > 0.2 * n
        assert np.all(np.abs(got["proj_x"][s].astype(np.float64) - u[s]) <= mu[s]) and np.all(np.abs(got["proj_y"][s].astype(np.float64) - v[s]) <= mv[s])
        assert np.median(mu[s] / np.spacing(np.abs(got["proj_x"][s])).astype(np.float64)) < 8
