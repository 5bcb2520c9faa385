"""ptmi_set_triangle_groups / ptmi_transform_groups (include/ptmi.h; csrc/scene_transform.hip): objects moved by matrix on the device.

The rule of tests/test_gpu_scene_update.py applies: context A uploads scene S, sets groups and calls transform_groups(ops); context B
uploads S and calls update_triangles(0, the model's records) (tests/transform_ref.py: the header's arithmetic in float32 numpy).
Then A equals B with no tolerance anywhere: the live records over all 128 bytes (this pins normals, uvs and padding), the image
by that file's comparison rules, (t, triangle, u, v) and the shadow predicate on 100 000 rays of its rays_for with seed 71, a small
render with equal segment, shadow-ray and path counts, and cost_now. On one upload mode per case B's render also equals the oracle's
render of the edited scene - pinned already by the scene-update suite; here it ties the chain together.

The scenes are the smallest that cover: a triangle count that is no multiple of 8 or of 64 (996, 304, 402, 4, 5, 12 492), a group of
one triangle, one group that is everything, members that straddle wave boundaries (a seeded random assignment scatters them), an empty
group, the device builder above 4 096 triangles, and more ops than one launch holds in LDS (600 over a 600-group table on grid80).
Scenes of more than one round of the grid, the op counts 512, 513 and 1 025 and the magnitude classes of the normals are in
tests/test_gpu_edit_edges.py.

Every case fails without the feature: the binding has no set_triangle_groups."""
import dataclasses

import numpy as np
import pytest

import scene_update_ref as uref
import transform_ref as ref
from ptmi import layout
from test_gpu_parity import assert_same_floats
from test_gpu_scene_update import UPLOADS, camera_for, ctx_a, ctx_b, rays_for, render, same_trace, scene, trace  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_UNSUPPORTED = -1, -4, -5
NONE = 0xFFFFFFFF

ROTATE = ref.affine(ref.rot_y(0.4), shift=(0.05, 0.02, -0.03))
SCALE = ref.affine(scale=(3, 0.5, 1))
MIRROR = ref.affine(scale=(-1, 1, 1), shift=(0.1, 0, 0))


def grouping(s, kind):
    n = len(s.tris)
    if kind == "material":
        return s.tris["material_index"].astype(np.uint32)
    if kind == "random5":
        return np.random.default_rng(11).integers(0, 5, n).astype(np.uint32)
    if kind == "empty":                                            # five ids, id 2 without a member
        g = np.random.default_rng(12).integers(0, 4, n).astype(np.uint32)
        return np.where(g >= 2, g + 1, g).astype(np.uint32)
    if kind == "all":
        return np.zeros(n, np.uint32)
    if kind == "single":
        g = np.zeros(n, np.uint32)
        g[n // 2] = 1
        return g
    if kind == "random600":
        return np.random.default_rng(13).integers(0, 600, n).astype(np.uint32)
    raise KeyError(kind)


def ops_for(groups, kind):
    ids = np.unique(groups)
    ga = int(groups[len(groups) // 2])
    gb = int(ids[ids != ga][0]) if len(ids) > 1 else ga
    if kind == "rotate":
        return [ref.op(ga, ROTATE)]
    if kind == "scale":
        return [ref.op(ga, SCALE)]
    if kind == "mirror":
        return [ref.op(ga, MIRROR)]
    if kind == "two":
        return [ref.op(gb, SCALE), ref.op(ga, ROTATE)]
    if kind == "with_empty":                                       # group 2 has no member (grouping "empty")
        return [ref.op(2, SCALE), ref.op(ga, ROTATE)]
    if kind == "all600":
        rng = np.random.default_rng(14)
        return [ref.op(g, ref.affine(ref.rot_y(rng.uniform(-0.3, 0.3)), shift=rng.uniform(-0.02, 0.02, 3))) for g in rng.permutation(600)]
    raise KeyError(kind)


def records(ops):
    from ptmi import native
    return native.group_ops(ops)


def fresh_scene(s, moved):
    return dataclasses.replace(s, tris=moved, nodes=uref.refit_nodes(s.nodes, moved))


def same_images(a, b, what):
    """tests/test_gpu_scene_update.py same_image's rules between two contexts: references, triangle words and quantised nodes by
    bits, boxes and header floats by value"""
    (ia, wa, qa, ta, la), (ib, wb, qb, tb, lb) = a, b
    assert wa.shape == wb.shape and np.array_equal(wa[:, :12], wb[:, :12]), f"{what}: node boxes"
    assert np.array_equal(wa.view(np.uint32)[:, 12:], wb.view(np.uint32)[:, 12:]), f"{what}: references"
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), f"{what}: triangle words"
    assert (la is None) == (lb is None) and (la is None or np.array_equal(la, lb)), f"{what}: leaf boxes"
    assert (qa is None) == (qb is None) and (qa is None or np.array_equal(qa, qb)), f"{what}: quantised nodes"
    for f in ("leaves_used", "n_wnodes", "n_tris", "root_ref", "depth", "n_leaves", "max_leaf_tris", "quantised", "pad", "safe_origin"):
        assert getattr(ia, f) == getattr(ib, f), f"{what}: header {f}"
    for f in ("root_min", "root_max", "q_origin", "q_scale"):
        assert np.array_equal(np.array(getattr(ia, f), np.float32), np.array(getattr(ib, f), np.float32)), f"{what}: header {f}"


def same_state(ctx_a, ctx_b, what):
    assert ctx_a.read_triangles().tobytes() == ctx_b.read_triangles().tobytes(), f"{what}: live records"
    same_images(ctx_a.read_image(), ctx_b.read_image(), what)
    sa, sb = ctx_a.scene_update_status(), ctx_b.scene_update_status()
    assert sa.cost_now == sb.cost_now and sa.quantised_kept == sb.quantised_kept, what


# (scene, grouping, ops, the upload mode whose renders are compared: an index into UPLOADS)
CASES = [("cornell", "material", "rotate", 0), ("cornell", "random5", "two", 2), ("cornell", "random5", "scale", 4),
         ("feature_box", "material", "mirror", 0), ("feature_box", "empty", "with_empty", 2),
         ("soup80", "random5", "scale", 0), ("soup80", "material", "two", 2),
         ("tiny4", "single", "rotate", 0), ("tiny4", "all", "mirror", 0), ("tiny5", "all", "scale", 0), ("tiny5", "single", "mirror", 2),
         ("grid80", "material", "rotate", 1), ("grid80", "random5", "mirror", 3), ("grid80", "random600", "all600", 1)]


@pytest.mark.parametrize("name,group_kind,op_kind,render_mode", CASES)
def test_transformed_context_equals_an_updated_one(ctx_a, ctx_b, oracle, name, group_kind, op_kind, render_mode):
    from ptmi import native
    s = scene(name)
    groups = grouping(s, group_kind)
    ops = ops_for(groups, op_kind)
    moved = ref.transformed(s.tris, ref.rest_of(s.tris), groups, ops)
    members = int(np.isin(groups, [g for g, _, _ in ops]).sum())
    assert members > 0 and not np.array_equal(moved, s.tris)
    fresh = fresh_scene(s, moved)
    o, d, dist = rays_for(fresh)
    cam, frames = camera_for(name)
    for mode, (leaves, builder, keep) in enumerate(UPLOADS):
        what = f"{name} {group_kind} {op_kind} leaves {leaves} builder {builder} keep {keep}"
        for c in (ctx_a, ctx_b):
            c.set_options(leaves=leaves, tree_builder=builder, keep_reference_tree=keep, traversal=native.TRAVERSAL_AUTO, cull=1)
        ctx_a.upload_scene(s)
        assert ctx_a.transform_status().present == 0
        ctx_a.set_triangle_groups(groups)
        ctx_a.transform_groups(records(ops))
        st = ctx_a.transform_status()
        assert (st.present, st.n_groups, st.transforms, st.last_moved, st.first_bad) == (1, int(groups.max()) + 1, 1, members, NONE), what
        assert st.transform_ms > 0.0 and ctx_a.scene_update_status().updates == 1
        ctx_b.upload_scene(s)
        ctx_b.update_triangles(0, moved)
        same_state(ctx_a, ctx_b, what)
        assert ctx_a.read_triangles().tobytes() == moved.tobytes(), f"{what}: live records against the model"
        same_trace(trace(ctx_a, o, d, dist), trace(ctx_b, o, d, dist), f"{what}: transformed against updated")
        if mode == render_mode:
            got_a, st_a = render(ctx_a, cam, frames)
            got_b, st_b = render(ctx_b, cam, frames)
            assert st_a == st_b, what
            assert_same_floats(got_a, got_b, f"{what}: radiance, transformed against updated")
            ref_img, ost = oracle.render(fresh, cam, frames, max_bounces=8, do_mis=1)
            assert st_b == (ost.segments, ost.shadow_rays, ost.paths), what
            assert_same_floats(got_b, ref_img, f"{what}: radiance, updated against the oracle")


def test_transforms_are_absolute_from_the_rest_pose(ctx_a):
    s = scene("cornell")
    groups = grouping(s, "random5")
    rest = ref.rest_of(s.tris)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_triangle_groups(groups)
    ctx_a.transform_groups(records([ref.op(1, ROTATE), ref.op(3, SCALE)]))
    first = ctx_a.read_triangles()
    assert first.tobytes() == ref.transformed(s.tris, rest, groups, [ref.op(1, ROTATE), ref.op(3, SCALE)]).tobytes()
    ctx_a.transform_groups(records([ref.op(1, MIRROR)]))                 # M2 from the rest pose, not on top of M1; group 3 keeps M1's bytes
    second = ctx_a.read_triangles()
    want = ref.transformed(first, rest, groups, [ref.op(1, MIRROR)])
    assert second.tobytes() == want.tobytes()
    assert second[groups == 1].tobytes() == ref.transformed(s.tris, rest, groups, [ref.op(1, MIRROR)])[groups == 1].tobytes()
    assert second[groups == 3].tobytes() == first[groups == 3].tobytes()
    st = ctx_a.transform_status()
    assert st.transforms == 2 and st.last_moved == int((groups == 1).sum()) and ctx_a.scene_update_status().updates == 2
    # no ops: what update_triangles(0, 0 records) does
    ctx_a.transform_groups(records([]))
    assert ctx_a.read_triangles().tobytes() == second.tobytes()
    assert ctx_a.transform_status().transforms == 3 and ctx_a.transform_status().last_moved == 0 and ctx_a.scene_update_status().updates == 3
    # ops on nothing: one op, and the group it names has no member (group 2 of the grouping "empty")
    s = scene("feature_box")
    groups = grouping(s, "empty")
    assert not (groups == 2).any()
    ctx_a.upload_scene(s)
    ctx_a.set_triangle_groups(groups)
    before, t0, u0 = ctx_a.read_triangles(), ctx_a.transform_status().transforms, ctx_a.scene_update_status().updates
    ctx_a.transform_groups(records([ref.op(2, SCALE)]))
    st = ctx_a.transform_status()
    assert ctx_a.read_triangles().tobytes() == before.tobytes() == s.tris.tobytes()
    assert (st.transforms, st.last_moved, st.first_bad) == (t0 + 1, 0, NONE) and ctx_a.scene_update_status().updates == u0 + 1
    ga = int(groups[len(groups) // 2])
    ctx_a.transform_groups(records([ref.op(ga, ROTATE)]))                # a real group after it still equals the model
    assert ctx_a.read_triangles().tobytes() == ref.transformed(s.tris, ref.rest_of(s.tris), groups, [ref.op(ga, ROTATE)]).tobytes()
    st = ctx_a.transform_status()
    assert (st.transforms, st.last_moved, st.first_bad) == (t0 + 2, int((groups == ga).sum()), NONE)


def test_update_triangles_rebases_the_rest_pose(ctx_a, ctx_b):
    s = scene("soup80")
    groups = grouping(s, "random5")
    lo, hi = 37, 251
    edit = uref.deformed(s.tris, "wobble")[lo:hi]
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_triangle_groups(groups)
    ctx_a.transform_groups(records([ref.op(2, ROTATE)]))
    ctx_a.update_triangles(lo, edit)                                      # these records are the rest pose of [lo, hi) from now on
    live = ctx_a.read_triangles()
    assert live[lo:hi].tobytes() == edit.tobytes()
    rebased = s.tris.copy()
    rebased[lo:hi] = edit
    ctx_a.transform_groups(records([ref.op(2, SCALE), ref.op(4, MIRROR)]))
    want = ref.transformed(live, ref.rest_of(rebased), groups, [ref.op(2, SCALE), ref.op(4, MIRROR)])
    assert ctx_a.read_triangles().tobytes() == want.tobytes()
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, "re-based")


def big_cornell():
    """cornell four times as large (coordinates up to 8), so that a scale of 1e38 leaves float32"""
    if "cornell_x4" not in _big:
        s = scene("cornell")
        tris = s.tris.copy()
        for f in ("v0", "v1", "v2"):
            tris[f] *= np.float32(4.0)
        _big["cornell_x4"] = fresh_scene(s, tris)
    return _big["cornell_x4"]


_big = {}


@pytest.mark.parametrize("which,scale", [("vertices", (1e38, 1e38, 1e38)), ("edges", (2e38, 1.0, 1.0))])
def test_a_refused_transform_changes_nothing(ctx_a, ctx_b, which, scale):
    """vertices: a scale of 1e38 on a cornell with coordinates up to 8 takes vertices out of float32. edges: on cornell itself
    (|x| <= 1, so 2e38 x is finite) a scale of 2e38 along x leaves every vertex finite and overflows the edge arithmetic a + (b - a)
    of own leaves on the triangles that span x = -1 .. 1. These are argument checks: the pass that finds them reads the rest pose and
    writes one word."""
    from ptmi import native
    s = big_cornell() if which == "vertices" else scene("cornell")
    groups = grouping(s, "material")
    rest = ref.rest_of(s.tris)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_triangle_groups(groups)
    ctx_a.transform_groups(records([ref.op(1, ROTATE)]))
    tris, image, upd, tf = ctx_a.read_triangles(), ctx_a.read_image(), ctx_a.scene_update_status(), ctx_a.transform_status()
    refused = None
    for g in np.unique(groups):
        ops = [ref.op(int(g), ref.affine(scale=scale), np.eye(3))]
        want = ref.first_bad(tris, rest, groups, ops, own=True)
        if want == NONE:
            continue
        out = ref.transformed(tris, rest, groups, ops)
        vertices_finite = all(np.isfinite(out[f]).all() for f in ("v0", "v1", "v2"))
        assert vertices_finite == (which == "edges")                # edges: finite results, an overflow in a + (b - a) alone
        refused = ops
        with pytest.raises(native.PtmiError) as e:
            ctx_a.transform_groups(records(ops))
        assert e.value.code == E_INVALID
        now = ctx_a.transform_status()
        assert now.first_bad == want and (now.transforms, now.last_moved, now.transform_ms) == (tf.transforms, tf.last_moved, tf.transform_ms)
        assert ctx_a.read_triangles().tobytes() == tris.tobytes()
        again = ctx_a.read_image()
        assert bytes(again[0]) == bytes(image[0]) and all(x is None or x.tobytes() == y.tobytes() for x, y in zip(image[1:], again[1:]))
        assert bytes(ctx_a.scene_update_status()) == bytes(upd)
    assert refused is not None
    # two groups in one call, one of them fine: still nothing
    with pytest.raises(native.PtmiError):
        ctx_a.transform_groups(records([ref.op(1, SCALE)] + refused if refused[0][0] != 1 else [ref.op(0, SCALE)] + refused))
    assert ctx_a.read_triangles().tobytes() == tris.tobytes()
    # the next valid call gives the usual bits
    ctx_a.transform_groups(records([ref.op(2, MIRROR)]))
    assert ctx_a.transform_status().first_bad == NONE
    want = ref.transformed(tris, rest, groups, [ref.op(2, MIRROR)])
    assert ctx_a.read_triangles().tobytes() == want.tobytes()
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, "after a refusal")


def test_reference_leaves_do_not_check_edges(ctx_a):
    """leaves = 1: ptmi_update_triangles asks for finite vertices only, and so does the check pass"""
    s = scene("cornell")
    groups = grouping(s, "all")
    ops = [ref.op(0, ref.affine(scale=(2e38, 1.0, 1.0)), np.eye(3))]
    assert ref.first_bad(s.tris, ref.rest_of(s.tris), groups, ops, own=True) != NONE
    assert ref.first_bad(s.tris, ref.rest_of(s.tris), groups, ops, own=False) == NONE
    ctx_a.set_options(leaves=1, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_triangle_groups(groups)
    ctx_a.transform_groups(records(ops))
    assert ctx_a.read_triangles().tobytes() == ref.transformed(s.tris, ref.rest_of(s.tris), groups, ops).tobytes()


def err(call, *args, **kw):
    from ptmi import native
    with pytest.raises(native.PtmiError) as e:
        call(*args, **kw)
    return e.value.code


def test_errors_and_clearing(ctx_a):
    from ptmi import native
    s = scene("cornell")
    groups = grouping(s, "random5")
    n = len(s.tris)
    with native.Context(0) as empty:                                     # no scene
        assert err(empty.set_triangle_groups, groups) == E_INVALID
        assert err(empty.transform_groups, records([ref.op(0, ROTATE)])) == E_STATE
        assert err(empty.read_triangles, 0, 1) == E_INVALID
        assert empty.transform_status().as_dict() == dict(present=0, n_groups=0, transforms=0, last_moved=0, first_bad=0, transform_ms=0.0)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    assert err(ctx_a.transform_groups, records([ref.op(0, ROTATE)])) == E_STATE           # no table
    assert err(ctx_a.set_triangle_groups, groups[:-1]) == E_INVALID
    assert err(ctx_a.set_triangle_groups, groups, n_triangles=n + 1) == E_INVALID
    far = groups.copy()
    far[5] = 65536
    assert err(ctx_a.set_triangle_groups, far) == E_UNSUPPORTED
    far[5] = 65535
    ctx_a.set_triangle_groups(far)
    assert ctx_a.transform_status().n_groups == 65536
    assert err(ctx_a.set_triangle_groups, groups[:-1]) == E_INVALID      # a failed call keeps the previous table
    assert ctx_a.transform_status().n_groups == 65536
    ctx_a.set_triangle_groups(groups)
    assert ctx_a.transform_status().n_groups == 5
    good = records([ref.op(0, ROTATE), ref.op(1, SCALE)])
    for field, value in (("reserved0", 1), ("reserved1", 7), ("group", 5)):
        bad = good.copy()
        bad[field][1] = value
        assert err(ctx_a.transform_groups, bad) == E_INVALID, field
    bad = good.copy()
    bad["group"][1] = 0                                                   # named twice
    assert err(ctx_a.transform_groups, bad) == E_INVALID
    for field, at, value in (("m", 3, np.nan), ("m", 11, np.inf), ("nm", 0, -np.inf)):
        bad = good.copy()
        bad[field][0, at] = value
        assert err(ctx_a.transform_groups, bad) == E_INVALID, field
    assert err(ctx_a.transform_groups, None, n_ops=2) == E_INVALID       # NULL ops with a count
    assert err(ctx_a.read_triangles, n - 1, 2) == E_INVALID and err(ctx_a.read_triangles, n + 1, 0) == E_INVALID
    assert len(ctx_a.read_triangles(n, 0)) == 0
    assert ctx_a.read_triangles().tobytes() == s.tris.tobytes() and ctx_a.transform_status().transforms == 0
    ctx_a.transform_groups(good)
    assert ctx_a.transform_status().transforms == 1 and ctx_a.transform_status().last_moved == int(np.isin(groups, (0, 1)).sum())
    ctx_a.set_triangle_groups(groups)                                    # set again: the rest pose is the live one, the count restarts
    assert ctx_a.transform_status().transforms == 0
    live = ref.transformed(s.tris, ref.rest_of(s.tris), groups, [ref.op(0, ROTATE), ref.op(1, SCALE)])
    ctx_a.transform_groups(records([ref.op(0, ROTATE)]))                 # ROTATE of the rotated pose
    assert ctx_a.read_triangles().tobytes() == ref.transformed(live, ref.rest_of(live), groups, [ref.op(0, ROTATE)]).tobytes()
    # a tree that is not nested: where update_triangles is unsupported, so is this
    loose = s.nodes.copy()
    inner = int(np.flatnonzero(loose["triangle_count"] == 0)[1])
    loose["aabb_min"][inner] += np.float32(0.01)
    ctx_a.upload_scene(dataclasses.replace(s, nodes=loose))
    assert ctx_a.transform_status().present == 0                          # an upload removes the table
    assert err(ctx_a.transform_groups, good) == E_STATE
    ctx_a.set_triangle_groups(groups)
    assert err(ctx_a.transform_groups, good) == E_UNSUPPORTED
    ctx_a.set_triangle_groups(None)
    assert ctx_a.transform_status().present == 0 and err(ctx_a.transform_groups, good) == E_STATE


@pytest.mark.parametrize("name,builder", [("grid80", 2), ("cornell", 1)])
def test_rebuild_after_a_transform(ctx_a, ctx_b, name, builder):
    s = scene(name)
    groups = grouping(s, "random5")
    ops = [ref.op(1, ROTATE), ref.op(4, SCALE)]
    moved = ref.transformed(s.tris, ref.rest_of(s.tris), groups, ops)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=builder, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_triangle_groups(groups)
    ctx_a.transform_groups(records(ops))
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, moved)
    assert ctx_a.rebuild_tree(builder).builder_used == ctx_b.rebuild_tree(builder).builder_used
    a, b = ctx_a.read_image(), ctx_b.read_image()
    assert bytes(a[0]) == bytes(b[0]) and all((x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()) for x, y in zip(a[1:], b[1:]))
    assert ctx_a.transform_status().present == 1                         # a rebuild leaves the table alone
    ctx_a.transform_groups(records([ref.op(1, MIRROR)]))
    ctx_b.update_triangles(0, ref.transformed(moved, ref.rest_of(s.tris), groups, [ref.op(1, MIRROR)]))
    same_state(ctx_a, ctx_b, f"{name}: transformed after a rebuild")


def test_motion_follows_a_transform(ctx_a, ctx_b):
    s = scene("cornell")
    groups = grouping(s, "material")
    g = int(groups[len(groups) // 2])
    ops = [ref.op(g, ref.affine(ref.rot_y(0.1), shift=(0.03, 0.0, 0.02)))]
    moved = ref.transformed(s.tris, ref.rest_of(s.tris), groups, ops)
    member = np.flatnonzero(groups == g)
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
                c.set_triangle_groups(groups)
                c.transform_groups(records(ops))
                ms = c.motion_status()
                assert (ms.dirty_first, ms.dirty_count) == (int(member.min()), int(member.max() - member.min() + 1))
            else:
                c.update_triangles(0, moved)
                assert c.motion_status().dirty_count == len(s.tris)
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
def test_transform_on_every_shard_assembles_the_single_device_frame(ctx_a, n):
    from ptmi import native
    s = scene("cornell")
    groups = grouping(s, "random5")
    ops = records([ref.op(0, ROTATE), ref.op(3, MIRROR)])
    W, H, frames = 80, 50, 3
    cam = layout.make_camera(W, H)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_triangle_groups(groups)
    ctx_a.transform_groups(ops)
    single, _ = render(ctx_a, cam, frames)
    with native.MultiContext([0] * n, loopback=True) as m:
        m.upload_scene(s)
        m.resize(W, H)
        m.set_options(max_bounces=8, do_mis=1)
        assert err(m.transform_groups, ops) == E_STATE
        m.set_triangle_groups(groups)
        m.transform_groups(ops)
        st = m.transform_status()
        assert (st.present, st.n_groups, st.transforms) == (1, 5, 1) and st.last_moved == ctx_a.transform_status().last_moved
        assert m.scene_update_status().cost_now == ctx_a.scene_update_status().cost_now
        for i in range(n):
            assert m.read_triangles(i).tobytes() == ctx_a.read_triangles().tobytes()
        m.dispatch(cam, frames)
        assert_same_floats(m.read_output(), single, f"{n} transformed shards against one transformed device")
        bad = ops.copy()
        bad["group"][1] = 9
        assert err(m.transform_groups, bad) == E_INVALID
        assert err(m.set_triangle_groups, groups[:-1]) == E_INVALID
        assert m.transform_status().transforms == 1
