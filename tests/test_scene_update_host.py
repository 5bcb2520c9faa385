"""The numpy model of ptmi_update_triangles (tests/scene_update_ref.py) against the library's own host builders: no GPU.

A refit recomputes boxes over a fixed topology. On unmoved triangles it must therefore give back what the builders made, and on moved
ones what a fresh host build of (moved triangles, refitted nodes) derives from the triangle set alone: pad, safe_origin, the root box
and the leaf boxes. Boxes are compared by value (which of -0 / +0 a tie returns is open), references and triangle words by bits."""
import dataclasses

import numpy as np
import pytest

import scene_update_ref as ref
from ptmi import scenes

NAMES = ["cornell", "cornell_spheres", "feature_box", "deep_chain", "soup80", "soup81", "soup82", "soup83"]
_made = {}


def scene(name):
    if name not in _made:
        _made[name] = scenes.random_soup(int(name[4:])) if name.startswith("soup") else scenes.make(name)
    return _made[name]


def same_image_words(got, want, what):
    """boxes by value, the reference words and the spare words by bits"""
    assert got.shape == want.shape, what
    assert np.array_equal(got[:, :12], want[:, :12]), f"{what}: {(got[:, :12] != want[:, :12]).any(axis=1).sum()} nodes differ in a box"
    assert np.array_equal(got.view(np.uint32)[:, 12:], want.view(np.uint32)[:, 12:]), f"{what}: references"


@pytest.mark.parametrize("name", NAMES)
def test_refit_of_unmoved_triangles_gives_the_built_nodes(name):
    s = scene(name)
    assert ref.refit_nodes(s.nodes, s.tris).tobytes() == s.nodes.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_refit_of_unmoved_triangles_gives_the_built_own_image(name):
    from ptmi import native
    s = scene(name)
    info, wn, qn, tp, lb = native.build_image(s, leaves=2)
    assert info.leaves_used == 2
    m = ref.refit_image(info, wn, qn, tp, lb, s.tris, s.nodes)
    same_image_words(m.wn, wn, name)
    assert np.array_equal(m.tp.view(np.uint32), tp.view(np.uint32))
    assert np.array_equal(m.lb, lb)
    assert (qn is None) == (m.qn is None)
    if qn is not None:
        assert np.array_equal(m.qn, qn), f"{(m.qn != qn).any(axis=1).sum()} quantised nodes differ"
        assert np.array_equal(m.q_origin, np.array(info.q_origin, np.float32)) and np.array_equal(m.q_scale, np.array(info.q_scale, np.float32))
    assert (m.pad, m.safe_origin) == (info.pad, info.safe_origin)
    assert np.array_equal(m.root_min, np.array(info.root_min, np.float32)) and np.array_equal(m.root_max, np.array(info.root_max, np.float32))
    assert m.cost == ref.image_cost(info, wn)


@pytest.mark.parametrize("opts", [dict(leaves=1), dict(leaves=2, keep_reference_tree=1)], ids=["leaves1", "kept"])
@pytest.mark.parametrize("name", NAMES)
def test_refit_of_unmoved_triangles_gives_the_built_exact_image(name, opts):
    from ptmi import native
    s = scene(name)
    info, wn, qn, tp, lb = native.build_image(s, **opts)
    assert info.leaves_used == 1 and lb is None
    m = ref.refit_image(info, wn, qn, tp, lb, s.tris, s.nodes)
    same_image_words(m.wn, wn, name)
    assert np.array_equal(m.tp, tp)
    assert m.qn is None                                                     # the quantised nodes of leaves = 1 are not refitted
    assert np.array_equal(m.root_min, np.array(info.root_min, np.float32)) and np.array_equal(m.root_max, np.array(info.root_max, np.float32))


def boxes_hold_what_is_below(info, m, tris):
    """every stored child box contains the boxes of an inner child, or the vertices (and v0 + e1, v0 + e2) of a leaf child's triangles"""
    wn, u = m.wn, m.wn.view(np.uint32)
    own = info.leaves_used == 2
    for side in range(2):
        lo, hi, r = wn[:, 6 * side:6 * side + 3], wn[:, 6 * side + 3:6 * side + 6], u[:, 12 + side]
        leaf = (r & ref.REF_LEAF) != 0
        ch = r[~leaf].astype(np.int64)
        for cs in range(2):
            assert (wn[ch, 6 * cs:6 * cs + 3] >= lo[~leaf]).all() and (wn[ch, 6 * cs + 3:6 * cs + 6] <= hi[~leaf]).all()
        first, cnt = ref._ref_parts(r[leaf])
        for k in range(int(cnt.max())):
            sel = cnt > k
            at = first[sel] + k
            t = tris[m.tp.view(np.uint32)[at, 3]] if own else tris[at]
            pts = [t["v0"], t["v1"], t["v2"]]
            if own:
                pts += [m.tp[at, 0:3] + m.tp[at, 4:7], m.tp[at, 0:3] + m.tp[at, 8:11]]
            for p in pts:
                assert (p >= lo[leaf][sel]).all() and (p <= hi[leaf][sel]).all()


@pytest.mark.parametrize("kind", ref.DEFORMATIONS)
@pytest.mark.parametrize("name", NAMES)
def test_refit_of_moved_triangles_agrees_with_a_fresh_host_build(name, kind):
    from ptmi import native
    s = scene(name)
    info, wn, qn, tp, lb = native.build_image(s, leaves=2)
    moved = ref.deformed(s.tris, kind)
    m = ref.refit_image(info, wn, qn, tp, lb, moved, s.nodes)
    fresh = dataclasses.replace(s, tris=moved, nodes=ref.refit_nodes(s.nodes, moved))
    finfo, fwn, fqn, ftp, flb = native.build_image(fresh, leaves=2)         # accepted: the refitted nodes are nested and finite
    assert finfo.leaves_used == 2
    assert (m.pad, m.safe_origin) == (finfo.pad, finfo.safe_origin)
    assert np.array_equal(m.root_min, np.array(finfo.root_min, np.float32)) and np.array_equal(m.root_max, np.array(finfo.root_max, np.float32))
    assert np.array_equal(m.lb, flb)
    boxes_hold_what_is_below(info, m, moved)
    if kind == "squash":
        assert m.n_slivers > 0 and ref.slivers(moved).sum() > ref.slivers(s.tris).sum()
    # ... and the exact image over the reference's leaves
    info1, wn1, qn1, tp1, _ = native.build_image(s, leaves=1)
    m1 = ref.refit_image(info1, wn1, qn1, tp1, None, moved, s.nodes)
    boxes_hold_what_is_below(info1, m1, moved)
    f1 = native.build_image(fresh, leaves=1)[0]
    assert np.array_equal(m1.root_min, np.array(f1.root_min, np.float32)) and np.array_equal(m1.root_max, np.array(f1.root_max, np.float32))
