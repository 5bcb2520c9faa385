"""ptmi_set_skin / ptmi_pose_skin (include/ptmi.h; csrc/scene_skin.hip): linear-blend skinning on the device.

The rule of tests/test_gpu_scene_update.py and tests/test_gpu_transform.py applies: context A uploads scene S, sets a skin and poses
it; context B uploads S and calls update_triangles(0, the model's records) (tests/skin_ref.py: the header's arithmetic in float32
numpy). Then A equals B with no tolerance anywhere: the live records over all 128 bytes, the image, (t, triangle, u, v) and the shadow
predicate on 100 000 rays, a small render, and cost_now. On one upload mode per case B's render also equals the oracle's render of the
edited scene.

The scenes are the smallest that cover: a list of 5 (no multiple of 8: a wave with three idle octets), a list of 1, a scattered third
(332) and half (6 246: no multiple of 8 or of 64, many blocks, the last one ending in a partial wave), four non-zero weights per
corner, the device builder above 4 096 triangles, and 600 joints, which take the instantiation that reads the joint records from
global memory (above 512), every one of them referenced. Lists of more than one round of the grid, the joint counts 512 and 513, the
magnitude classes of the normals and the weights as given are in tests/test_gpu_edit_edges.py.

Every case fails without the feature: the binding has no set_skin."""
import numpy as np
import pytest

import scene_update_ref as uref
import skin_ref as ref
import transform_ref as tref
from ptmi import layout
from test_gpu_parity import assert_same_floats
from test_gpu_scene_update import UPLOADS, camera_for, ctx_a, ctx_b, rays_for, render, same_trace, scene, trace  # noqa: F401 (fixtures)
from test_gpu_transform import big_cornell, err, fresh_scene, same_state

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_UNSUPPORTED = -1, -4, -5
NONE = 0xFFFFFFFF


def pose(n_joints, seed):
    """a seeded pose: per joint a small rotation, a scale near 1 and a small shift, as (m, nm) without negative zeros"""
    rng = np.random.default_rng(seed)
    return [ref.joint(tref.affine(tref.rot_y(rng.uniform(-0.3, 0.3)), scale=1.0 + rng.uniform(-0.1, 0.1, 3), shift=rng.uniform(-0.03, 0.03, 3)))
            for _ in range(n_joints)]


def records(joints):
    from ptmi import native
    return native.joint_ops(joints)


def skin_for(s, listing, n_joints, influences=2, cover=False):
    """(the ascending list, the corner records) of a case"""
    n = len(s.tris)
    rng = np.random.default_rng(31)
    if listing == "all":
        listed = np.arange(n)
    elif listing == "one":
        listed = np.array([n // 2])
    elif listing == "third":
        listed = np.sort(rng.choice(n, n // 3, replace=False))
    elif listing == "half":
        listed = np.sort(rng.choice(n, n // 2, replace=False))
    else:
        raise KeyError(listing)
    return listed.astype(np.uint32), ref.random_corners(rng, len(listed), n_joints, influences, cover)


# (scene, listing, joints, non-zero weights per corner, the upload modes (indices into UPLOADS), the mode whose renders are compared)
ALL = (0, 1, 2, 3, 4)
CASES = [("tiny5", "all", 2, 2, ALL, 0), ("tiny4", "one", 2, 2, ALL, 2), ("cornell", "third", 3, 3, ALL, 4),
         ("soup80", "all", 7, 4, ALL, 1), ("grid80", "half", 3, 2, (1, 3), 1), ("grid80", "half", 600, 2, (1, 3), 3)]


def test_listed_counts_cover_partial_octets_and_waves():
    counts = [len(skin_for(scene(name), listing, nj)[0]) for name, listing, nj, _, _, _ in CASES]
    assert any(c % 8 for c in counts) and any(c % 64 for c in counts) and any(c > 64 and c % 64 for c in counts), counts
    assert 5 in counts and 1 in counts


@pytest.mark.parametrize("name,listing,n_joints,influences,modes,render_mode", CASES)
def test_posed_context_equals_an_updated_one(ctx_a, ctx_b, oracle, name, listing, n_joints, influences, modes, render_mode):
    from ptmi import native
    s = scene(name)
    listed, corners = skin_for(s, listing, n_joints, influences, cover=n_joints > 512)
    assert (np.count_nonzero(corners["weight"], axis=1) == influences).all()
    assert len(np.unique(corners["joint"])) == n_joints or n_joints <= 512          # the global-memory case references every joint
    joints = pose(n_joints, 32)
    moved = ref.skinned(s.tris, tref.rest_of(s.tris), listed, corners, joints)
    assert not np.array_equal(moved[listed], s.tris[listed])
    fresh = fresh_scene(s, moved)
    o, d, dist = rays_for(fresh)
    cam, frames = camera_for(name)
    assert render_mode in modes
    for mode in modes:
        leaves, builder, keep = UPLOADS[mode]
        what = f"{name} {listing} {n_joints} joints leaves {leaves} builder {builder} keep {keep}"
        for c in (ctx_a, ctx_b):
            c.set_options(leaves=leaves, tree_builder=builder, keep_reference_tree=keep, traversal=native.TRAVERSAL_AUTO, cull=1)
        ctx_a.upload_scene(s)
        assert ctx_a.skin_status().present == 0
        ctx_a.set_skin(listed, corners, n_joints)
        st = ctx_a.skin_status()
        assert (st.present, st.n_joints, st.n_skinned, st.poses, st.first_bad) == (1, n_joints, len(listed), 0, NONE), what
        ctx_a.pose_skin(records(joints))
        st = ctx_a.skin_status()
        assert (st.present, st.n_joints, st.n_skinned, st.poses, st.first_bad) == (1, n_joints, len(listed), 1, NONE), what
        assert st.pose_ms > 0.0 and ctx_a.scene_update_status().updates == 1
        ctx_b.upload_scene(s)
        ctx_b.update_triangles(0, moved)
        same_state(ctx_a, ctx_b, what)
        assert ctx_a.read_triangles().tobytes() == moved.tobytes(), f"{what}: live records against the model"
        same_trace(trace(ctx_a, o, d, dist), trace(ctx_b, o, d, dist), f"{what}: posed against updated")
        if mode == render_mode:
            got_a, st_a = render(ctx_a, cam, frames)
            got_b, st_b = render(ctx_b, cam, frames)
            assert st_a == st_b, what
            assert_same_floats(got_a, got_b, f"{what}: radiance, posed against updated")
            ref_img, ost = oracle.render(fresh, cam, frames, max_bounces=8, do_mis=1)
            assert st_b == (ost.segments, ost.shadow_rays, ost.paths), what
            assert_same_floats(got_b, ref_img, f"{what}: radiance, updated against the oracle")


def test_one_hot_skinning_equals_transform_groups(ctx_a, ctx_b):
    """weights (1, 0, 0, 0) with joint = group: the same bytes as the groups feature on another context"""
    s = scene("cornell")
    groups = np.random.default_rng(33).integers(0, 5, len(s.tris)).astype(np.uint32)
    joints = pose(5, 34)
    listed = np.arange(len(s.tris), dtype=np.uint32)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
        c.upload_scene(s)
    ctx_a.set_skin(listed, ref.one_hot(groups), 5)
    ctx_a.pose_skin(records(joints))
    ctx_b.set_triangle_groups(groups)
    ctx_b.transform_groups([(g, m, nm) for g, (m, nm) in enumerate(joints)])
    same_state(ctx_a, ctx_b, "one-hot skin against groups")
    assert not np.array_equal(ctx_a.read_triangles(), s.tris)
    ctx_b.set_triangle_groups(None)


def test_poses_are_absolute_from_the_rest_pose(ctx_a):
    s = scene("cornell")
    listed, corners = skin_for(s, "third", 3, 3)
    rest = tref.rest_of(s.tris)
    p1, p2 = pose(3, 35), pose(3, 36)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_skin(listed, corners, 3)
    ctx_a.pose_skin(records(p1))
    first = ctx_a.read_triangles()
    assert first.tobytes() == ref.skinned(s.tris, rest, listed, corners, p1).tobytes()
    ctx_a.pose_skin(records(p2))                                         # P2 from the rest pose, not on top of P1
    second = ctx_a.read_triangles()
    assert second.tobytes() == ref.skinned(s.tris, rest, listed, corners, p2).tobytes() and second.tobytes() != first.tobytes()
    ctx_a.pose_skin(records(p2))                                         # the same pose again: the same bytes
    assert ctx_a.read_triangles().tobytes() == second.tobytes()
    assert ctx_a.skin_status().poses == 3 and ctx_a.scene_update_status().updates == 3


def test_update_triangles_rebases_the_rest_pose(ctx_a, ctx_b):
    s = scene("soup80")
    listed, corners = skin_for(s, "half", 4, 3)
    lo, hi = 37, 251
    inside = (listed >= lo) & (listed < hi)
    assert inside.any() and (listed < lo).any() and (listed >= hi).any()  # the range cuts through the list
    edit = uref.deformed(s.tris, "wobble")[lo:hi]
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_skin(listed, corners, 4)
    ctx_a.pose_skin(records(pose(4, 37)))
    ctx_a.update_triangles(lo, edit)                                      # these records are the rest pose of the listed among [lo, hi)
    live = ctx_a.read_triangles()
    assert live[lo:hi].tobytes() == edit.tobytes()
    rebased = s.tris.copy()
    rebased[lo:hi] = edit                                                 # listed triangles outside the range keep the old rest pose
    p2 = pose(4, 38)
    ctx_a.pose_skin(records(p2))
    want = ref.skinned(live, tref.rest_of(rebased), listed, corners, p2)
    assert ctx_a.read_triangles().tobytes() == want.tobytes()
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, "re-based")


@pytest.mark.parametrize("which,scale", [("vertices", (1e38, 1e38, 1e38)), ("edges", (2e38, 1.0, 1.0))])
def test_a_refused_pose_changes_nothing(ctx_a, ctx_b, which, scale):
    """vertices: blended weights on a cornell with coordinates up to 8; a joint scaled by 1e38 takes the vertices it weighs enough out
    of float32 (weight times coordinate above 3.4), which are some of the listed ones and not the first of the list. edges: one-hot weights on cornell itself (|x| <= 1, so 2e38 x is finite): every vertex stays finite and the edge
    arithmetic a + (b - a) of own leaves overflows on the triangles that span x = -1 .. 1."""
    from ptmi import native
    if which == "vertices":
        s = big_cornell()
        n_joints = 3
        listed, corners = skin_for(s, "third", n_joints, 2)
    else:
        s = scene("cornell")
        groups = s.tris["material_index"].astype(np.uint32)
        n_joints = int(groups.max()) + 1
        listed, corners = np.arange(len(s.tris), dtype=np.uint32), ref.one_hot(groups)
    rest = tref.rest_of(s.tris)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_skin(listed, corners, n_joints)
    good = pose(n_joints, 39)
    ctx_a.pose_skin(records(good))
    tris, image, upd, sk = ctx_a.read_triangles(), ctx_a.read_image(), ctx_a.scene_update_status(), ctx_a.skin_status()
    refused = 0
    for g in range(n_joints):
        joints = list(good)
        joints[g] = ref.joint(tref.affine(scale=scale), np.eye(3))
        want = ref.first_bad(tris, rest, listed, corners, joints, own=True)
        if want == NONE:
            continue
        out = ref.skinned(tris, rest, listed, corners, joints)
        vertices_finite = all(np.isfinite(out[f]).all() for f in ("v0", "v1", "v2"))
        assert vertices_finite == (which == "edges")
        refused += 1
        with pytest.raises(native.PtmiError) as e:
            ctx_a.pose_skin(records(joints))
        assert e.value.code == E_INVALID
        now = ctx_a.skin_status()
        assert now.first_bad == want and (now.poses, now.pose_ms) == (sk.poses, sk.pose_ms)
        assert ctx_a.read_triangles().tobytes() == tris.tobytes()
        again = ctx_a.read_image()
        assert bytes(again[0]) == bytes(image[0]) and all(x is None or x.tobytes() == y.tobytes() for x, y in zip(image[1:], again[1:]))
        assert bytes(ctx_a.scene_update_status()) == bytes(upd)
    assert refused
    # the next valid call gives the usual bits
    p2 = pose(n_joints, 40)
    ctx_a.pose_skin(records(p2))
    assert ctx_a.skin_status().first_bad == NONE
    want = ref.skinned(tris, rest, listed, corners, p2)
    assert ctx_a.read_triangles().tobytes() == want.tobytes()
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, "after a refusal")


def test_reference_leaves_do_not_check_edges(ctx_a):
    """leaves = 1: ptmi_update_triangles asks for finite vertices only, and so does the check pass"""
    s = scene("cornell")
    listed = np.arange(len(s.tris), dtype=np.uint32)
    corners = ref.one_hot(np.zeros(len(s.tris), np.uint32))
    joints = [ref.joint(tref.affine(scale=(2e38, 1.0, 1.0)), np.eye(3))]
    rest = tref.rest_of(s.tris)
    assert ref.first_bad(s.tris, rest, listed, corners, joints, own=True) != NONE
    assert ref.first_bad(s.tris, rest, listed, corners, joints, own=False) == NONE
    ctx_a.set_options(leaves=1, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_skin(listed, corners, 1)
    ctx_a.pose_skin(records(joints))
    assert ctx_a.read_triangles().tobytes() == ref.skinned(s.tris, rest, listed, corners, joints).tobytes()


def test_errors_and_clearing(ctx_a):
    import dataclasses

    from ptmi import native
    s = scene("cornell")
    n = len(s.tris)
    listed, corners = skin_for(s, "third", 3, 3)
    good = records(pose(3, 41))
    with native.Context(0) as empty:                                     # no scene
        assert err(empty.set_skin, listed, corners, 3) == E_INVALID
        assert err(empty.pose_skin, good) == E_STATE
        assert empty.skin_status().as_dict() == dict(present=0, n_joints=0, n_skinned=0, poses=0, first_bad=0, pose_ms=0.0)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    assert err(ctx_a.pose_skin, good) == E_STATE                         # no skin
    ctx_a.set_skin(listed, corners, 3)

    def refused_set(tri=listed, cor=corners, nj=3, code=E_INVALID):
        assert err(ctx_a.set_skin, tri, cor, nj) == code
        st = ctx_a.skin_status()                                         # a failed call keeps the previous skin
        assert (st.present, st.n_joints, st.n_skinned) == (1, 3, len(listed))

    bad = listed.copy()
    bad[-1] = n
    refused_set(tri=bad)                                                 # an index >= n_triangles
    bad = listed.copy()
    bad[4] = bad[3]
    refused_set(tri=bad)                                                 # not strictly ascending: equal
    bad = listed.copy()
    bad[[3, 4]] = bad[[4, 3]]
    refused_set(tri=bad)                                                 # ... descending
    refused_set(cor=None)                                                # corners NULL
    bad = corners.copy()
    bad["joint"][7, 3] = 3
    bad["weight"][7, 3] = 0.0
    refused_set(cor=bad)                                                 # joint >= n_joints in a slot of weight zero
    for value in (np.nan, np.inf, -np.inf):
        bad = corners.copy()
        bad["weight"][-1, 1] = value
        refused_set(cor=bad)                                             # a weight that is not finite
    refused_set(nj=0)
    refused_set(cor=ref.random_corners(np.random.default_rng(1), len(listed), 2), nj=65537, code=E_UNSUPPORTED)
    ctx_a.set_skin(listed, ref.random_corners(np.random.default_rng(1), len(listed), 65536), 65536)
    assert ctx_a.skin_status().n_joints == 65536
    ctx_a.set_skin(listed, corners, 3)
    # pose_skin's host-side errors: the context is unchanged
    before = ctx_a.read_triangles().tobytes()
    assert err(ctx_a.pose_skin, good[:2]) == E_INVALID                   # not the skin's joint count
    assert err(ctx_a.pose_skin, records(pose(4, 41))) == E_INVALID
    assert err(ctx_a.pose_skin, None, n_joints=3) == E_INVALID           # NULL joints
    for field, value in (("reserved0", 1), ("reserved1", 7), ("group", 0), ("group", 3)):
        bad = good.copy()
        bad[field][1] = value
        assert err(ctx_a.pose_skin, bad) == E_INVALID, field
    assert err(ctx_a.pose_skin, good[::-1].copy()) == E_INVALID          # a shuffled pose
    for field, at, value in (("m", 3, np.nan), ("m", 11, np.inf), ("nm", 0, -np.inf)):
        bad = good.copy()
        bad[field][0, at] = value
        assert err(ctx_a.pose_skin, bad) == E_INVALID, field
    assert ctx_a.read_triangles().tobytes() == before == s.tris.tobytes() and ctx_a.skin_status().poses == 0
    assert ctx_a.scene_update_status().updates == 0
    ctx_a.pose_skin(good)
    assert ctx_a.skin_status().poses == 1
    ctx_a.set_skin(listed, corners, 3)                                   # set again: the rest pose is the live one, the count restarts
    assert ctx_a.skin_status().poses == 0
    live = ref.skinned(s.tris, tref.rest_of(s.tris), listed, corners, good)
    ctx_a.pose_skin(good)                                                # the pose of the posed records
    assert ctx_a.read_triangles().tobytes() == ref.skinned(live, tref.rest_of(live), listed, corners, good).tobytes()
    # materials and lights leave the skin alone
    ctx_a.update_materials(0, s.mats[:1])
    assert ctx_a.skin_status().present == 1
    # a tree that is not nested: where update_triangles is unsupported, so is this
    loose = s.nodes.copy()
    inner = int(np.flatnonzero(loose["triangle_count"] == 0)[1])
    loose["aabb_min"][inner] += np.float32(0.01)
    ctx_a.upload_scene(dataclasses.replace(s, nodes=loose))
    assert ctx_a.skin_status().present == 0                              # an upload removes the skin
    assert err(ctx_a.pose_skin, good) == E_STATE
    ctx_a.set_skin(listed, corners, 3)
    assert err(ctx_a.pose_skin, good) == E_UNSUPPORTED
    ctx_a.set_skin(None)
    assert ctx_a.skin_status().as_dict() == dict(present=0, n_joints=0, n_skinned=0, poses=0, first_bad=0, pose_ms=0.0)
    assert err(ctx_a.pose_skin, good) == E_STATE
    ctx_a.set_skin(listed, corners, 3)
    ctx_a.set_skin(listed[:0], corners[:0], 3)                           # n_skinned = 0 removes it too
    assert ctx_a.skin_status().present == 0


@pytest.mark.parametrize("name,builder", [("grid80", 2), ("cornell", 1)])
def test_rebuild_after_a_pose(ctx_a, ctx_b, name, builder):
    s = scene(name)
    listed, corners = skin_for(s, "half", 3, 2)
    p1, p2 = pose(3, 42), pose(3, 43)
    rest = tref.rest_of(s.tris)
    moved = ref.skinned(s.tris, rest, listed, corners, p1)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=builder, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_skin(listed, corners, 3)
    ctx_a.pose_skin(records(p1))
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, moved)
    assert ctx_a.rebuild_tree(builder).builder_used == ctx_b.rebuild_tree(builder).builder_used
    a, b = ctx_a.read_image(), ctx_b.read_image()
    assert bytes(a[0]) == bytes(b[0]) and all((x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()) for x, y in zip(a[1:], b[1:]))
    assert ctx_a.skin_status().present == 1                              # a rebuild leaves the skin alone
    ctx_a.pose_skin(records(p2))
    ctx_b.update_triangles(0, ref.skinned(moved, rest, listed, corners, p2))
    same_state(ctx_a, ctx_b, f"{name}: posed after a rebuild")


def test_motion_follows_a_pose(ctx_a, ctx_b):
    s = scene("cornell")
    listed, corners = skin_for(s, "third", 3, 3)
    joints = [ref.joint(tref.affine(tref.rot_y(0.1 * k), shift=(0.03, 0.0, 0.02 * k))) for k in range(3)]
    moved = ref.skinned(s.tris, tref.rest_of(s.tris), listed, corners, joints)
    lo, hi = int(listed.min()), int(listed.max())
    assert lo > 0 or hi < len(s.tris) - 1
    cam = layout.make_camera(96, 64, aperture=0.0)
    got = []
    try:
        for c in (ctx_a, ctx_b):
            c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
            c.upload_scene(s)
            c.resize(96, 64)
            c.set_aovs("normal", "id")
            c.set_moments(True)
            c.set_motion(True)
            c.dispatch(cam, 4)
            if c is ctx_a:
                c.set_skin(listed, corners, 3)
                c.pose_skin(records(joints))
            else:
                c.update_triangles(lo, moved[lo:hi + 1])
            ms = c.motion_status()
            assert (ms.dirty_first, ms.dirty_count) == (lo, hi - lo + 1)
            c.reproject(cam, cam)
            got.append((c.read_motion(), c.read_output(), c.read_moments(), c.read_aov("normal"), c.read_aov("id"), c.motion_status().moved))
    finally:
        for c in (ctx_a, ctx_b):
            c.set_motion(False)
            c.set_aovs()
            c.set_moments(False)
    for x, y, what in zip(got[0][:5], got[1][:5], ("motion", "output", "moments", "normal", "id")):
        assert x.tobytes() == y.tobytes(), what
    assert got[0][5] == got[1][5]


@pytest.mark.parametrize("n", [2, 3])
def test_pose_on_every_shard_assembles_the_single_device_frame(ctx_a, n):
    from ptmi import native
    s = scene("cornell")
    listed, corners = skin_for(s, "third", 3, 3)
    joints = records(pose(3, 44))
    W, H, frames = 80, 50, 3
    cam = layout.make_camera(W, H)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_skin(listed, corners, 3)
    ctx_a.pose_skin(joints)
    single, _ = render(ctx_a, cam, frames)
    with native.MultiContext([0] * n, loopback=True) as m:
        m.upload_scene(s)
        m.resize(W, H)
        m.set_options(max_bounces=8, do_mis=1)
        assert err(m.pose_skin, joints) == E_STATE
        m.set_skin(listed, corners, 3)
        m.pose_skin(joints)
        st = m.skin_status()
        assert (st.present, st.n_joints, st.n_skinned, st.poses) == (1, 3, len(listed), 1)
        assert m.scene_update_status().cost_now == ctx_a.scene_update_status().cost_now
        for i in range(n):
            assert m.read_triangles(i).tobytes() == ctx_a.read_triangles().tobytes()
        m.dispatch(cam, frames)
        assert_same_floats(m.read_output(), single, f"{n} posed shards against one posed device")
        bad = joints.copy()
        bad["group"][1] = 2
        assert err(m.pose_skin, bad) == E_INVALID
        bad = listed.copy()
        bad[0] = len(s.tris)
        assert err(m.set_skin, bad, corners, 3) == E_INVALID
        assert m.skin_status().poses == 1
