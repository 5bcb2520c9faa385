"""A morph and a skin on one context (include/ptmi.h ptmi_set_morph "Interactions"; csrc/scene_morph.hip morph_relink): they compose in
glTF's order. For a triangle both list, ptmi_pose_morph writes to the skin's rest row and ptmi_pose_skin carries it to the live record;
a triangle only the morph lists goes to its live record at once.

cornell with three disjoint triangle sets: morph only, skin only, both. The model is the two models in a row: the morphed records
(tests/morph_ref.py) are the rest pose the skin's model (tests/skin_ref.py) blends from. A equals B = update_triangles(0, that) with no
tolerance.

Every case fails without the feature: the binding has no set_morph."""
import numpy as np
import pytest

import morph_ref as mref
import skin_ref as sref
import transform_ref as tref
from test_gpu_scene_update import ctx_a, ctx_b, scene  # noqa: F401 (fixtures)
from test_gpu_skin import pose
from test_gpu_skin import records as joint_records
from test_gpu_transform import same_state

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
N_TARGETS, N_JOINTS = 5, 3


def sets(s, only_morph=True):
    """(the morph's list, its rows and records, the skin's list and corners, the triangles in both)"""
    n = len(s.tris)
    rng = np.random.default_rng(91)
    which = rng.integers(0, 4, n)                                        # 0: neither, 1: morph only, 2: skin only, 3: both
    if not only_morph:
        which[which == 1] = 3
    m_list = np.flatnonzero((which == 1) | (which == 3)).astype(np.uint32)
    s_list = np.flatnonzero((which == 2) | (which == 3)).astype(np.uint32)
    both = np.flatnonzero(which == 3)
    assert len(both) > 8 and (which == 2).sum() > 8 and ((which == 1).sum() > 8) == only_morph
    row_start, deltas = mref.table(rng, len(m_list), N_TARGETS, (2, 0, 1, 3))
    corners = sref.random_corners(rng, len(s_list), N_JOINTS, 3)
    return m_list, row_start, deltas, s_list, corners, both


def model(tris, m_rest, m_list, row_start, deltas, w, s_list, corners, joints):
    """(the records after pose_morph + pose_skin, the morphed records the skin blends from)"""
    m = mref.morphed(tris, m_rest, m_list, row_start, deltas, w)
    return sref.skinned(m, tref.rest_of(m), s_list, corners, joints), m


def prepare(ctx_a, ctx_b, s):
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
        c.upload_scene(s)


@pytest.mark.parametrize("order", ["morph first", "skin first"])
def test_morph_then_skin_equals_the_two_models_in_a_row(ctx_a, ctx_b, order):
    s = scene("cornell")
    m_list, row_start, deltas, s_list, corners, both = sets(s)
    w = mref.weights_for(np.random.default_rng(92), N_TARGETS, 4)
    joints = pose(N_JOINTS, 93)
    rest = tref.rest_of(s.tris)
    want, m = model(s.tris, rest, m_list, row_start, deltas, w, s_list, corners, joints)
    assert not np.array_equal(want[both], sref.skinned(s.tris, rest, s_list, corners, joints)[both])      # the morph shows through the skin
    prepare(ctx_a, ctx_b, s)
    if order == "morph first":
        ctx_a.set_morph(m_list, row_start, deltas, N_TARGETS)
        assert ctx_a.morph_status().n_in_skin == 0
        ctx_a.set_skin(s_list, corners, N_JOINTS)
    else:
        ctx_a.set_skin(s_list, corners, N_JOINTS)
        ctx_a.set_morph(m_list, row_start, deltas, N_TARGETS)
    st = ctx_a.morph_status()
    assert (st.n_morphed, st.n_in_skin, st.skin_stale) == (len(m_list), len(both), 0)
    ctx_a.pose_morph(w)
    st = ctx_a.morph_status()
    assert (st.poses, st.skin_stale, st.first_bad) == (1, 1, NONE) and ctx_a.scene_update_status().updates == 1
    half = m.copy()
    half[both] = s.tris[both]                                            # the live records of the shared triangles wait for the skin
    assert ctx_a.read_triangles().tobytes() == half.tobytes()
    ctx_a.pose_skin(joint_records(joints))
    assert ctx_a.morph_status().skin_stale == 0 and ctx_a.scene_update_status().updates == 2
    assert ctx_a.read_triangles().tobytes() == want.tobytes()
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, order)
    # a second frame: both absolute, from the same rest poses
    w2 = mref.weights_for(np.random.default_rng(94), N_TARGETS, None)
    j2 = pose(N_JOINTS, 95)
    ctx_a.pose_morph(w2)
    ctx_a.pose_skin(joint_records(j2))
    m2 = mref.morphed(want, rest, m_list, row_start, deltas, w2)
    want2 = sref.skinned(m2, tref.rest_of(mref.morphed(s.tris, rest, m_list, row_start, deltas, w2)), s_list, corners, j2)
    assert ctx_a.read_triangles().tobytes() == want2.tobytes()
    ctx_b.update_triangles(0, want2)
    same_state(ctx_a, ctx_b, f"{order}: the second frame")
    # without the skin the morph writes to the live records again
    ctx_a.set_skin(None)
    st = ctx_a.morph_status()
    assert (st.present, st.n_in_skin, st.skin_stale) == (1, 0, 0)
    ctx_a.pose_morph(w)
    want3 = mref.morphed(want2, rest, m_list, row_start, deltas, w)
    assert ctx_a.read_triangles().tobytes() == want3.tobytes() and ctx_a.morph_status().skin_stale == 0
    ctx_b.update_triangles(0, want3)
    same_state(ctx_a, ctx_b, f"{order}: after the skin's removal")


def test_a_morph_inside_the_skin_runs_no_refit(ctx_a, ctx_b):
    s = scene("cornell")
    m_list, row_start, deltas, s_list, corners, both = sets(s, only_morph=False)
    assert np.isin(m_list, s_list).all() and len(m_list) < len(s_list)
    w = mref.weights_for(np.random.default_rng(96), N_TARGETS, None)
    joints = pose(N_JOINTS, 97)
    prepare(ctx_a, ctx_b, s)
    ctx_a.set_skin(s_list, corners, N_JOINTS)
    ctx_a.set_morph(m_list, row_start, deltas, N_TARGETS)
    assert ctx_a.morph_status().n_in_skin == len(m_list)
    ctx_a.pose_skin(joint_records(joints))
    live, upd = ctx_a.read_triangles(), bytes(ctx_a.scene_update_status())
    ctx_a.pose_morph(w)
    st = ctx_a.morph_status()
    assert (st.poses, st.skin_stale, st.active_targets) == (1, 1, N_TARGETS) and st.pose_ms > 0.0
    assert ctx_a.read_triangles().tobytes() == live.tobytes() and bytes(ctx_a.scene_update_status()) == upd     # no live record, no refit
    ctx_a.pose_skin(joint_records(joints))
    assert ctx_a.morph_status().skin_stale == 0 and ctx_a.scene_update_status().updates == 2
    want, _ = model(s.tris, tref.rest_of(s.tris), m_list, row_start, deltas, w, s_list, corners, joints)
    assert ctx_a.read_triangles().tobytes() == want.tobytes() != live.tobytes()
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, "a morph inside the skin")
