"""k_quadtree2 (path histograms in every iteration) against its previous body, k_quadtree2p (ORBX_QT_V2P: candidate passes behind the
fused iterations), on the A/B library: byte for byte on the hand-laid frames of tests/quadtree_table_cases.py and on three seeded
synthetic frames.  ORBX_QT_HISTD caps the table depth at the fused depth, so that on the synthetic frames nearly every level leaves
table mode: the same bytes again.  The counter moves by exactly what the watched second reading (quadtree_table_cases.
levels_that_fall_back) says for each table depth, and not at all under the previous body."""
import numpy as np
import pytest

import extract_cases as ec
import quadtree_table_cases as qc
import second_reading_extract as sr
from test_quadtree_table_cases_cpu import levels_of

pytestmark = pytest.mark.gpu

GROUPS = {}
for _c in qc.all_cases():
    GROUPS.setdefault(ec.key(_c), []).append(_c)


def run(pkg, monkeypatch, env, make, frames, laps):
    """Single calls and one batch of the frames on a handle created under `env`: (results, fallbacks)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ex = make(len(frames))
    for k in env:
        monkeypatch.delenv(k)
    try:
        out = [ex(f, l) for f, l in zip(frames, laps)] + list(ex.extract_batch(frames, laps))
        return out, ex.quadtree_fallbacks()
    finally:
        ex.close()


def falls(c, depth=None):
    """Levels of the frame that leave table mode (at the planned depth, or at `depth`), by the watched second reading."""
    rd = sr.extract(levels_of(c), c["nf"], c["sf"], c["ini"], c["mn"], c["lap"])
    return len(qc.levels_that_fall_back(c, rd, depth))


def same(a, b):
    return all(x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and np.array_equal(x[2], y[2]) for x, y in zip(a, b)) and len(a) == len(b)


def test_previous_body_equals_the_new_one_on_the_cases(pkg, monkeypatch):
    for k, group in GROUPS.items():
        w, h, nf, nl, sf, ini, mn = k
        make = lambda n: pkg.ORBextractor(nf, sf, nl, ini, mn, max_size=(w, h), max_batch=n)
        frames, laps = [c["img"] for c in group], [c["lap"] for c in group]
        new, moved = run(pkg, monkeypatch, {}, make, frames, laps)
        old, none = run(pkg, monkeypatch, {"ORBX_QT_V2P": "1"}, make, frames, laps)
        assert same(new, old), k
        assert none == 0 and moved == 2 * sum(falls(c) for c in group), k        # (single + batch; the previous body has no table mode to leave)


@pytest.mark.parametrize("kind", ["textured", "sparse", "lowcontrast"])
def test_previous_body_equals_the_new_one_on_synthetic_frames(pkg, synth, monkeypatch, kind):
    frames = [synth.gen_image(752, 480, 4100 + i, kind) for i in range(2)]
    laps = [(0, 1000), (100, 400)]
    make = lambda n: pkg.ORBextractor(1000, max_size=(752, 480), max_batch=n)
    new, moved = run(pkg, monkeypatch, {}, make, frames, laps)
    old, none = run(pkg, monkeypatch, {"ORBX_QT_V2P": "1"}, make, frames, laps)
    capped, forced = run(pkg, monkeypatch, {"ORBX_QT_HISTD": "3"}, make, frames, laps)
    assert same(new, old) and same(new, capped), kind
    cs = [dict(img=f, nf=1000, nl=8, sf=1.2, ini=20, mn=7, lap=l) for f, l in zip(frames, laps)]
    at4, at3 = sum(falls(dict(c, D=4)) for c in cs), sum(falls(c, 3) for c in cs)
    assert none == 0 and moved == 2 * at4 and forced == 2 * at3, (kind, moved, forced, at4, at3)
    if kind == "textured":
        assert at3 > at4                                                         # dense levels are still splitting at depth 3
