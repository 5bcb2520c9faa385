"""ptmi_set_morph / ptmi_pose_morph (include/ptmi.h; csrc/scene_morph.hip): morph targets on the device.

The rule of tests/test_gpu_skin.py applies: context A uploads scene S, sets a morph and poses it; context B uploads S and calls
update_triangles(0, the model's records) (tests/morph_ref.py: the header's arithmetic in float32 numpy). Then A equals B with no
tolerance anywhere: the live records over all 128 bytes, the image, (t, triangle, u, v) and the shadow predicate on 100 000 rays, a
small render, and cost_now. On one upload mode per case B's render also equals the oracle's render of the edited scene.

The scenes are the smallest that cover: lists of 1 and 5, a scattered third of cornell (332) with rows of 0 .. 3 records mixed, all of
soup80 with 40 targets of which 3 are non-zero (rows of which no record is applied among them), half of grid80 (6 246: no multiple of
8 or of 64, the device builder), one target, and 8 192 targets (the whole 32 KB of LDS) every one of which some record names. Lists of
more than one round of the grid are in tests/test_gpu_morph_rounds.py, the skin beside the morph in tests/test_gpu_morph_skin.py, and
the value edges (normal magnitudes, weights as given, the edge of the vertex check), rows of 8 192 records, refusals with a skin in
place, the groups beside the morph, the re-base ranges and motion with a mixed list in tests/test_gpu_morph_edges.py.

Every case fails without the feature: the binding has no set_morph."""
import numpy as np
import pytest

import morph_ref as ref
import scene_update_ref as uref
import transform_ref as tref
from ptmi import layout
from test_gpu_parity import assert_same_floats
from test_gpu_scene_update import UPLOADS, camera_for, ctx_a, ctx_b, rays_for, render, same_trace, scene, trace  # noqa: F401 (fixtures)
from test_gpu_transform import err, fresh_scene, same_state

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_UNSUPPORTED = -1, -4, -5
NONE = 0xFFFFFFFF


def listing_of(s, listing, seed=81):
    n = len(s.tris)
    rng = np.random.default_rng(seed)
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
    return listed.astype(np.uint32)


def morph_for(s, listing, n_targets, lengths, cover=False):
    """(the ascending list, the row bounds, the records) of a case"""
    listed = listing_of(s, listing)
    row_start, deltas = ref.table(np.random.default_rng(82), len(listed), n_targets, lengths, cover)
    return listed, row_start, deltas


def counts(ctx):
    st = ctx.morph_status()
    return st.present, st.n_targets, st.n_morphed, st.n_records, st.n_in_skin, st.poses, st.first_bad, st.skin_stale


# (scene, listing, targets, row lengths (cycled), non-zero weights (None: all), every target named, upload modes, the rendered mode)
ALL = (0, 1, 2, 3, 4)
CASES = [("tiny5", "all", 3, (1, 2, 0, 3, 1), None, False, ALL, 0), ("tiny4", "one", 1, (1,), None, False, ALL, 2),
         ("cornell", "third", 4, (0, 1, 2, 3), None, False, ALL, 4), ("soup80", "all", 40, (3, 5, 8), 3, False, ALL, 1),
         ("grid80", "half", 6, (2, 0, 1), 4, False, (1, 3), 1), ("cornell", "third", 8192, (25,), None, True, (0, 2), 0)]


def test_listed_counts_cover_partial_octets_and_waves():
    made = [morph_for(scene(name), listing, nt, lengths, cover) for name, listing, nt, lengths, _, cover, _, _ in CASES]
    n = [len(m[0]) for m in made]
    assert any(c % 8 for c in n) and any(c % 64 for c in n) and any(c > 64 and c % 64 for c in n), n
    assert 5 in n and 1 in n and 6246 in n
    assert any((np.diff(m[1].astype(np.int64)) == 0).any() for m in made)                # empty rows
    assert sorted({int(x) for x in np.diff(made[2][1].astype(np.int64))}) == [0, 1, 2, 3]
    assert len(np.unique(made[5][2]["target"])) == 8192 == ref.MAX_TARGETS               # every LDS word is referenced
    assert {nt for _, _, nt, *_ in CASES} >= {1, 40, 8192}


@pytest.mark.parametrize("name,listing,n_targets,lengths,active,cover,modes,render_mode", CASES)
def test_posed_context_equals_an_updated_one(ctx_a, ctx_b, oracle, name, listing, n_targets, lengths, active, cover, modes, render_mode):
    from ptmi import native
    s = scene(name)
    listed, row_start, deltas = morph_for(s, listing, n_targets, lengths, cover)
    w = ref.weights_for(np.random.default_rng(83), n_targets, active)
    k = ref.applied_counts(row_start, deltas, w)
    assert k.max() > 0 and (active is None or (k == 0).any())
    moved = ref.morphed(s.tris, tref.rest_of(s.tris), listed, row_start, deltas, w)
    assert not np.array_equal(moved[listed], s.tris[listed])
    fresh = fresh_scene(s, moved)
    o, d, dist = rays_for(fresh)
    cam, frames = camera_for(name)
    assert render_mode in modes
    n_active = int(np.count_nonzero(w))
    for mode in modes:
        leaves, builder, keep = UPLOADS[mode]
        what = f"{name} {listing} {n_targets} targets leaves {leaves} builder {builder} keep {keep}"
        for c in (ctx_a, ctx_b):
            c.set_options(leaves=leaves, tree_builder=builder, keep_reference_tree=keep, traversal=native.TRAVERSAL_AUTO, cull=1)
        ctx_a.upload_scene(s)
        assert ctx_a.morph_status().present == 0
        ctx_a.set_morph(listed, row_start, deltas, n_targets)
        assert counts(ctx_a) == (1, n_targets, len(listed), len(deltas), 0, 0, NONE, 0), what
        ctx_a.pose_morph(w)
        assert counts(ctx_a) == (1, n_targets, len(listed), len(deltas), 0, 1, NONE, 0), what
        st = ctx_a.morph_status()
        assert st.pose_ms > 0.0 and st.active_targets == n_active and ctx_a.scene_update_status().updates == 1
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


def test_8193_targets_are_unsupported(ctx_a):
    s = scene("cornell")
    listed, row_start, deltas = morph_for(s, "third", 4, (1,))
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    assert err(ctx_a.set_morph, listed, row_start, deltas, 8193) == E_UNSUPPORTED
    assert ctx_a.morph_status().present == 0
    ctx_a.set_morph(listed, row_start, deltas, 8192)
    assert ctx_a.morph_status().n_targets == 8192


def test_a_zero_pose_restores_the_upload_and_poses_are_absolute(ctx_a, ctx_b):
    s = scene("cornell")
    tris = s.tris.copy()
    listed, row_start, deltas = morph_for(s, "third", 5, (0, 1, 2, 3))
    tris["v1"][listed[::3], 2] = -0.0                                    # rest components that -0 + 0 * d would turn into +0
    tris["n2"][listed[1]] = (0.0, 2.0, 0.0)                              # a rest normal that is not unit: not renormalised when untouched
    s = fresh_scene(s, tris)
    rest = tref.rest_of(s.tris)
    rng = np.random.default_rng(84)
    w1, w2 = ref.weights_for(rng, 5, None), ref.weights_for(rng, 5, 2)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
        c.upload_scene(s)
    ctx_a.set_morph(listed, row_start, deltas, 5)
    ctx_a.pose_morph(w1)
    first = ctx_a.read_triangles()
    assert first.tobytes() == ref.morphed(s.tris, rest, listed, row_start, deltas, w1).tobytes() != s.tris.tobytes()
    ctx_a.pose_morph(w2)                                                 # w2 from the rest pose, not on top of w1
    second = ctx_a.read_triangles()
    assert second.tobytes() == ref.morphed(s.tris, rest, listed, row_start, deltas, w2).tobytes() != first.tobytes()
    ctx_a.pose_morph(w2)
    assert ctx_a.read_triangles().tobytes() == second.tobytes()
    ctx_a.pose_morph(np.array([0.0, -0.0, 0.0, -0.0, -0.0], np.float32))  # all zero, either sign: the untouched upload, bit for bit
    assert ctx_a.read_triangles().tobytes() == s.tris.tobytes()
    st = ctx_a.morph_status()
    assert (st.poses, st.active_targets) == (4, 0) and ctx_a.scene_update_status().updates == 4
    ctx_b.update_triangles(0, s.tris)
    same_state(ctx_a, ctx_b, "an all-zero pose")


def test_update_triangles_rebases_the_rest_pose(ctx_a, ctx_b):
    s = scene("soup80")
    listed, row_start, deltas = morph_for(s, "half", 4, (1, 0, 3))
    lo, hi = 37, 251
    inside = (listed >= lo) & (listed < hi)
    assert inside.any() and (listed < lo).any() and (listed >= hi).any()  # the range cuts through the list
    edit = uref.deformed(s.tris, "wobble")[lo:hi]
    rng = np.random.default_rng(85)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_morph(listed, row_start, deltas, 4)
    ctx_a.pose_morph(ref.weights_for(rng, 4, None))
    ctx_a.update_triangles(lo, edit)                                      # these records are the rest pose of the listed among [lo, hi)
    live = ctx_a.read_triangles()
    assert live[lo:hi].tobytes() == edit.tobytes()
    rebased = s.tris.copy()
    rebased[lo:hi] = edit                                                 # listed triangles outside the range keep the old rest pose
    w2 = ref.weights_for(rng, 4, None)
    ctx_a.pose_morph(w2)
    want = ref.morphed(live, tref.rest_of(rebased), listed, row_start, deltas, w2)
    assert ctx_a.read_triangles().tobytes() == want.tobytes()
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, "re-based")


def refusing(s, which):
    """a table on a third of cornell with one record more, on a target of its own (4), in the row of entry 7: vertices: a delta of 3e38
    that weight 2 takes out of float32; edges: v0.x - 3e38 and v1.x + 3e38 under weight 0.75 stay finite and their difference does not"""
    listed, row_start, deltas = morph_for(s, "third", 4, (0, 1, 2, 3))
    at = int(row_start[8])                                                # behind the last record of entry 7 (targets < 4 come first)
    extra = np.zeros(1, layout.MORPH_DELTA)
    extra["target"] = 4
    if which == "vertices":
        extra["dv2"][0, 1] = 3e38
        weight = 2.0
    else:
        extra["dv0"][0, 0], extra["dv1"][0, 0] = -3e38, 3e38
        weight = 0.75
    deltas = np.concatenate([deltas[:at], extra, deltas[at:]])
    row_start = row_start.copy()
    row_start[8:] += 1
    return listed, row_start, deltas, np.float32(weight)


@pytest.mark.parametrize("which", ["vertices", "edges"])
def test_a_refused_pose_changes_nothing(ctx_a, ctx_b, which):
    from ptmi import native
    s = scene("cornell")
    listed, row_start, deltas, weight = refusing(s, which)
    rest = tref.rest_of(s.tris)
    rng = np.random.default_rng(86)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_morph(listed, row_start, deltas, 5)
    good = ref.weights_for(rng, 5, None)
    good[4] = 0.0
    ctx_a.pose_morph(good)
    tris, image, upd, ms = ctx_a.read_triangles(), ctx_a.read_image(), ctx_a.scene_update_status(), ctx_a.morph_status()
    bad = good.copy()
    bad[4] = weight
    want = ref.first_bad(tris, rest, listed, row_start, deltas, bad, own=True)
    assert want == int(listed[7]) and ref.first_bad(tris, rest, listed, row_start, deltas, good, own=True) == NONE
    out = ref.morphed(tris, rest, listed, row_start, deltas, bad)
    assert all(np.isfinite(out[f]).all() for f in ref.VERTS) == (which == "edges")
    with pytest.raises(native.PtmiError) as e:
        ctx_a.pose_morph(bad)
    assert e.value.code == E_INVALID
    now = ctx_a.morph_status()
    assert now.first_bad == want and (now.poses, now.pose_ms, now.active_targets) == (ms.poses, ms.pose_ms, ms.active_targets)
    assert ctx_a.read_triangles().tobytes() == tris.tobytes()
    again = ctx_a.read_image()
    assert bytes(again[0]) == bytes(image[0]) and all(x is None or x.tobytes() == y.tobytes() for x, y in zip(image[1:], again[1:]))
    assert bytes(ctx_a.scene_update_status()) == bytes(upd)
    w2 = ref.weights_for(rng, 5, None)                                    # the next valid call gives the usual bits
    w2[4] = 0.0
    ctx_a.pose_morph(w2)
    assert ctx_a.morph_status().first_bad == NONE
    want = ref.morphed(tris, rest, listed, row_start, deltas, w2)
    assert ctx_a.read_triangles().tobytes() == want.tobytes()
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, "after a refusal")


def test_reference_leaves_do_not_check_edges(ctx_a):
    """leaves = 1: ptmi_update_triangles asks for finite vertices only, and so does the check pass"""
    s = scene("cornell")
    listed, row_start, deltas, weight = refusing(s, "edges")
    rest = tref.rest_of(s.tris)
    w = np.array([0.5, 0.0, -0.25, 0.0, weight], np.float32)
    assert ref.first_bad(s.tris, rest, listed, row_start, deltas, w, own=True) != NONE
    assert ref.first_bad(s.tris, rest, listed, row_start, deltas, w, own=False) == NONE
    ctx_a.set_options(leaves=1, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_morph(listed, row_start, deltas, 5)
    ctx_a.pose_morph(w)
    assert ctx_a.read_triangles().tobytes() == ref.morphed(s.tris, rest, listed, row_start, deltas, w).tobytes()


def test_errors_and_clearing(ctx_a):
    import dataclasses

    from ptmi import native
    s = scene("cornell")
    n = len(s.tris)
    listed, row_start, deltas = morph_for(s, "third", 4, (0, 1, 2, 3))
    good = ref.weights_for(np.random.default_rng(87), 4, None)
    nothing = dict(present=0, n_targets=0, n_morphed=0, n_records=0, n_in_skin=0, poses=0, active_targets=0, first_bad=0, skin_stale=0,
                   pose_ms=0.0)
    with native.Context(0) as empty:                                     # no scene
        assert err(empty.set_morph, listed, row_start, deltas, 4) == E_INVALID
        assert err(empty.pose_morph, good) == E_STATE
        assert empty.morph_status().as_dict() == nothing
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    assert err(ctx_a.pose_morph, good) == E_STATE                        # no morph
    ctx_a.set_morph(listed, row_start, deltas, 4)

    def refused_set(tri=listed, rows=row_start, rec=deltas, nt=4, code=E_INVALID):
        assert err(ctx_a.set_morph, tri, rows, rec, nt) == code
        st = ctx_a.morph_status()                                        # a failed call keeps the previous morph
        assert (st.present, st.n_targets, st.n_morphed, st.n_records) == (1, 4, len(listed), len(deltas))

    bad = listed.copy()
    bad[-1] = n
    refused_set(tri=bad)                                                 # an index >= n_triangles
    bad = listed.copy()
    bad[4] = bad[3]
    refused_set(tri=bad)                                                 # not strictly ascending: equal
    bad = listed.copy()
    bad[[3, 4]] = bad[[4, 3]]
    refused_set(tri=bad)                                                 # ... descending
    refused_set(rec=None)                                                # deltas NULL where records exist
    assert err(ctx_a.set_morph, listed, None, deltas, 4) == E_INVALID    # row_start NULL beside records
    bad = row_start.copy()
    bad[0] = 1
    refused_set(rows=bad)                                                # the rows do not start at 0
    bad = row_start.copy()
    bad[5] = bad[6] + 1
    refused_set(rows=bad)                                                # ... decrease
    two = int(np.flatnonzero(np.diff(row_start.astype(np.int64)) >= 2)[0])
    r = int(row_start[two])
    bad = deltas.copy()
    bad["target"][r] = 4
    refused_set(rec=bad)                                                 # target >= n_targets
    bad = deltas.copy()
    bad["target"][r + 1] = bad["target"][r]
    refused_set(rec=bad)                                                 # a row that names a target twice
    bad = deltas.copy()
    bad["target"][[r, r + 1]] = bad["target"][[r + 1, r]]
    refused_set(rec=bad)                                                 # ... descends
    for field in ("reserved0", "reserved1", "reserved2", "reserved3", "reserved4"):
        bad = deltas.copy()
        bad[field][-1] = 1
        refused_set(rec=bad)                                             # a non-zero reserved word
    for field, value in (("dv0", np.nan), ("dv2", np.inf), ("dn1", -np.inf)):
        bad = deltas.copy()
        bad[field][3, 1] = value
        refused_set(rec=bad)                                             # a delta that is not finite
    refused_set(nt=0)
    refused_set(nt=8193, code=E_UNSUPPORTED)
    # pose_morph's host-side errors: the context is unchanged
    assert err(ctx_a.pose_morph, good[:3]) == E_INVALID                  # not the morph's target count
    assert err(ctx_a.pose_morph, np.zeros(5, np.float32)) == E_INVALID
    assert err(ctx_a.pose_morph, None, n_targets=4) == E_INVALID         # NULL weights
    for value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[2] = value
        assert err(ctx_a.pose_morph, bad) == E_INVALID                   # a weight that is not finite
    assert ctx_a.read_triangles().tobytes() == s.tris.tobytes() and ctx_a.morph_status().poses == 0
    assert ctx_a.scene_update_status().updates == 0
    ctx_a.pose_morph(good)
    assert ctx_a.morph_status().poses == 1
    ctx_a.set_morph(listed, row_start, deltas, 4)                        # set again: the rest pose is the live one, the count restarts
    assert ctx_a.morph_status().poses == 0
    live = ref.morphed(s.tris, tref.rest_of(s.tris), listed, row_start, deltas, good)
    ctx_a.pose_morph(good)                                               # the pose of the posed records
    assert ctx_a.read_triangles().tobytes() == ref.morphed(live, tref.rest_of(live), listed, row_start, deltas, good).tobytes()
    ctx_a.set_morph(listed, None, None, 4)                               # every row empty: a pose restores the rest pose
    assert ctx_a.morph_status().n_records == 0
    before = ctx_a.read_triangles().tobytes()
    ctx_a.pose_morph(good)
    assert ctx_a.read_triangles().tobytes() == before
    ctx_a.set_morph(listed, row_start, deltas, 4)
    # materials and lights leave the morph alone
    ctx_a.update_materials(0, s.mats[:1])
    assert ctx_a.morph_status().present == 1
    # a tree that is not nested: where update_triangles is unsupported, so is this
    loose = s.nodes.copy()
    inner = int(np.flatnonzero(loose["triangle_count"] == 0)[1])
    loose["aabb_min"][inner] += np.float32(0.01)
    ctx_a.upload_scene(dataclasses.replace(s, nodes=loose))
    assert ctx_a.morph_status().present == 0                             # an upload removes the morph
    assert err(ctx_a.pose_morph, good) == E_STATE
    ctx_a.set_morph(listed, row_start, deltas, 4)
    assert err(ctx_a.pose_morph, good) == E_UNSUPPORTED
    ctx_a.set_morph(None)
    assert ctx_a.morph_status().as_dict() == nothing
    assert err(ctx_a.pose_morph, good) == E_STATE
    ctx_a.set_morph(listed, row_start, deltas, 4)
    ctx_a.set_morph(listed[:0], row_start[:1], deltas[:0], 4)            # n_morphed = 0 removes it too
    assert ctx_a.morph_status().present == 0


@pytest.mark.parametrize("name,builder", [("grid80", 2), ("cornell", 1)])
def test_rebuild_after_a_pose(ctx_a, ctx_b, name, builder):
    s = scene(name)
    listed, row_start, deltas = morph_for(s, "half", 3, (2, 0, 1))
    rng = np.random.default_rng(88)
    w1, w2 = ref.weights_for(rng, 3, None), ref.weights_for(rng, 3, 2)
    rest = tref.rest_of(s.tris)
    moved = ref.morphed(s.tris, rest, listed, row_start, deltas, w1)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=builder, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_morph(listed, row_start, deltas, 3)
    ctx_a.pose_morph(w1)
    ctx_b.upload_scene(s)
    ctx_b.update_triangles(0, moved)
    assert ctx_a.rebuild_tree(builder).builder_used == ctx_b.rebuild_tree(builder).builder_used
    a, b = ctx_a.read_image(), ctx_b.read_image()
    assert bytes(a[0]) == bytes(b[0]) and all((x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()) for x, y in zip(a[1:], b[1:]))
    assert ctx_a.morph_status().present == 1                             # a rebuild leaves the morph alone
    ctx_a.pose_morph(w2)
    ctx_b.update_triangles(0, ref.morphed(moved, rest, listed, row_start, deltas, w2))
    same_state(ctx_a, ctx_b, f"{name}: posed after a rebuild")


def test_motion_follows_a_pose(ctx_a, ctx_b):
    s = scene("cornell")
    listed, row_start, deltas = morph_for(s, "third", 3, (1, 2, 0))
    w = np.array([0.8, -0.5, 0.6], np.float32)
    moved = ref.morphed(s.tris, tref.rest_of(s.tris), listed, row_start, deltas, w)
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
                c.set_morph(listed, row_start, deltas, 3)
                c.pose_morph(w)
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
    listed, row_start, deltas = morph_for(s, "third", 4, (0, 1, 2, 3))
    w = ref.weights_for(np.random.default_rng(89), 4, 3)
    W, H, frames = 80, 50, 3
    cam = layout.make_camera(W, H)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.set_morph(listed, row_start, deltas, 4)
    ctx_a.pose_morph(w)
    single, _ = render(ctx_a, cam, frames)
    with native.MultiContext([0] * n, loopback=True) as m:
        m.upload_scene(s)
        m.resize(W, H)
        m.set_options(max_bounces=8, do_mis=1)
        assert err(m.pose_morph, w) == E_STATE
        m.set_morph(listed, row_start, deltas, 4)
        m.pose_morph(w)
        st = m.morph_status()
        assert (st.present, st.n_targets, st.n_morphed, st.n_records, st.poses, st.active_targets) == (1, 4, len(listed), len(deltas), 1, 3)
        assert m.scene_update_status().cost_now == ctx_a.scene_update_status().cost_now
        for i in range(n):
            assert m.read_triangles(i).tobytes() == ctx_a.read_triangles().tobytes()
        m.dispatch(cam, frames)
        assert_same_floats(m.read_output(), single, f"{n} posed shards against one posed device")
        bad = w.copy()
        bad[1] = np.nan
        assert err(m.pose_morph, bad) == E_INVALID
        bad = listed.copy()
        bad[0] = len(s.tris)
        assert err(m.set_morph, bad, row_start, deltas, 4) == E_INVALID
        assert m.morph_status().poses == 1
