"""ptmi_reproject with motion on (include/ptmi.h ptmi_set_motion) on the GPU against tests/reproject_motion_ref.py, bit for bit. As in
tests/test_gpu_reproject.py the model is fed the device's own centre rays, their hits with (u, v) (ptmi_debug_intersect on the EDITED
scene), tan(fov / 2) as the kernels compute it and the previous positions the device holds (ptmi_debug_motion_prev, read before the
call), so what is compared is step 4 with the moved rule, the motion plane and the commit. The edit of every case moves one box of the
scene (the triangles of material 5) and is sent as ONE range from the box's first to its last triangle: the scenes are in tree order,
so that range also rewrites triangles of other parts with the bits they had, and those must take the static rule.

Every case fails without the feature: the binding has no set_motion."""
import dataclasses

import numpy as np
import pytest

import adaptive_ref
import reproject_motion_ref as motion_ref
import scene_update_ref as sur
from ptmi import layout, native
from test_gpu_reproject import ALL, BASE, FRAMES, H, MISS, MOVES, W, at, bits, err, same_planes

pytestmark = pytest.mark.gpu

f32 = np.float32
E_INVALID, E_STATE = -1, -4
SIDEWAYS = MOVES["sideways"]
BOX_MATERIAL = 5                                      # the short box of cornell and of feature_box
TURN = 0.5                                            # radians about +Y, then the scene's shift: to where the camera still sees the box
SHIFT = {"cornell": (-0.4, 0.0, 0.3), "feature_box": (0.1, 0.4, 0.1)}     # (feature_box: up, clear of the sphere in front of it)


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the planes and options it sets never reach the session's shared context"""
    c = native.Context(0)
    yield c
    c.close()


def verts(tris):
    return np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1).astype(f32)


def box_edit(sc):
    """(the scene's triangles with the box moved, first, end): the range [first, end) spans the box's triangles"""
    sel = sc.tris["material_index"] == BOX_MATERIAL
    idx = np.flatnonzero(sel)
    assert 0 < len(idx) < len(sc.tris)
    moved = sur.move_part(sc.tris, sel, sur.rot_y(TURN), SHIFT[sc.name])
    return moved, int(idx.min()), int(idx.max()) + 1


def setup(ctx, sc, aovs=ALL, motion=True, **opt):
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=0,
             overlap=2, perf_mode=0, leaves=0, timing=0)
    o.update(opt)
    ctx.set_motion(False)
    ctx.set_aovs()
    ctx.set_moments(False)
    ctx.set_options(**o)
    ctx.upload_scene(sc)
    ctx.resize(W, H)
    ctx.set_aovs(*aovs)
    ctx.set_moments(True)
    ctx.set_motion(motion)
    ctx.reset_stats()


def read_planes(ctx):
    on = ctx.aovs()
    return dict(output=ctx.read_output(), moments=ctx.read_moments(), normal=ctx.read_aov("normal"),
                albedo=ctx.read_aov("albedo") if "albedo" in on else None, id=ctx.read_aov("id") if "id" in on else None,
                motion=ctx.read_motion() if ctx.motion() else None)


def rendered(ctx, sc, aovs=ALL, motion=True, **opt):
    setup(ctx, sc, aovs=aovs, motion=motion, **opt)
    ctx.dispatch(at(BASE, 0), FRAMES)
    return read_planes(ctx)


def model(ctx, sc, tris_now, snap, cam_from, cam_to, rows=None, **params):
    """tests/reproject_motion_ref.py on the device's own centre rays, hits, tan, previous positions and dirty range"""
    o, d = ctx.debug_center_rays(cam_to)
    t, tri, u, v = ctx.debug_intersect(o, d)
    assert ((tri == MISS) == (t < 0)).all()
    th = ctx.debug_math(11, np.array([f32(cam_from["fov"]) * f32(0.5)], f32))[0]
    st = ctx.motion_status()
    prev = ctx.debug_motion_prev(0, len(sc.tris))
    planes, status = motion_ref.reproject(snap, cam_from, o, d, t, tri, u, v, sc.tris["material_index"], th, prev, verts(tris_now),
                                          (st.dirty_first, st.dirty_count), rows=rows, **params)
    moved = motion_ref.moved_mask(tri, prev, verts(tris_now), (st.dirty_first, st.dirty_count)).reshape(H, W)
    return planes, status, moved


def check_against_model(ctx, sc, tris_now, cam_from, cam_to, snap, rows=None, **params):
    want, want_st, moved = model(ctx, sc, tris_now, snap, cam_from, cam_to, rows=rows, **params)
    ctx.reproject(cam_from, cam_to, **params)
    got = read_planes(ctx)
    ms = ctx.motion_status().as_dict()
    got_st = dict(ctx.reproject_status().as_dict(), moved=ms["moved"], moved_carried=ms["moved_carried"])
    print("status", got_st, "model", want_st)
    same_planes(got, want)
    assert got_st == want_st
    return want, want_st, moved


def status(ctx):
    return ctx.motion_status().as_dict()


@pytest.mark.parametrize("name", ["cornell", "feature_box"])
def test_no_edit_no_difference(ctx, scene_factory, name):
    sc = scene_factory(name)
    rendered(ctx, sc, motion=False)
    assert ctx.motion_device_ptr() is None
    ctx.reproject(BASE, SIDEWAYS)
    off, off_st = read_planes(ctx), ctx.reproject_status().as_dict()
    snap = rendered(ctx, sc, motion=True)
    assert ctx.motion_device_ptr() and not snap["motion"].any()
    want, st, moved = check_against_model(ctx, sc, sc.tris, BASE, SIDEWAYS, snap)
    on = read_planes(ctx)
    same_planes({k: on[k] for k in off if k != "motion"}, {k: off[k] for k in off if k != "motion"})
    assert ctx.reproject_status().as_dict() == off_st
    assert st["moved"] == 0 and not moved.any() and st["carried"] > 0 and st["disoccluded"] > 0 and st["missed"] > 0
    m = on["motion"]
    assert np.array_equal(m[..., 3] == 0, on["moments"][..., 2] > 0) and np.array_equal(m[..., 3] == 2, on["id"][..., 0] == MISS)
    assert status(ctx) == dict(on=1, epochs=1, dirty_first=0, dirty_count=0, moved=0, moved_carried=0)


@pytest.mark.parametrize("move", ["unmoved", "sideways"])
@pytest.mark.parametrize("name", ["cornell", "feature_box"])
def test_a_moved_part_matches_the_model(ctx, scene_factory, name, move):
    sc = scene_factory(name)
    to = BASE if move == "unmoved" else SIDEWAYS
    moved_tris, first, end = box_edit(sc)
    snap = rendered(ctx, sc)
    ctx.update_triangles(first, moved_tris[first:end])
    assert status(ctx) == dict(on=1, epochs=0, dirty_first=first, dirty_count=end - first, moved=0, moved_carried=0)
    want, st, moved = check_against_model(ctx, sc, moved_tris, BASE, to, snap)
    # the comparison shows something: moved pixels that are carried, moved pixels that are disoccluded, all three outcomes
    w = want["motion"][..., 3]
    assert st["moved"] == int(moved.sum()) and st["moved_carried"] == int((moved & (w == 0)).sum()) > 0
    assert (moved & (w == 1)).any(), "no moved pixel is disoccluded"
    assert st["carried"] > 0 and st["disoccluded"] > 0 and st["missed"] > 0, st
    assert (want["id"][..., 1][moved] == BOX_MATERIAL).all()          # the range's other triangles were rewritten unchanged: static
    px = np.hypot(want["motion"][..., 0], want["motion"][..., 1])[moved]
    print(f"{name} {move}: {st['moved']} moved pixels, {st['moved_carried']} carried, median motion {np.median(px):.2f} px")
    assert np.median(px) >= 2.0
    # the same state without motion: the static rule carries strictly fewer of those pixels, so the rule did the work, not the id test
    rendered(ctx, sc, motion=False)
    ctx.update_triangles(first, moved_tris[first:end])
    ctx.reproject(BASE, to)
    static_carried = int((ctx.read_moments()[..., 2] > 0)[moved].sum())
    print("carried of the moved pixels without motion:", static_carried)
    assert static_carried < st["moved_carried"]


def test_dirty_range_semantics(ctx, scene_factory):
    sc = scene_factory("cornell")
    n = len(sc.tris)
    moved_tris, first, end = box_edit(sc)
    uploaded = verts(sc.tris)
    snap = rendered(ctx, sc)
    assert np.array_equal(bits(ctx.debug_motion_prev(0, n)), bits(uploaded))
    # two updates of different ranges: the previous positions stay the upload's, the dirty range is the union
    wob = sur.wobble(sc.tris, 0.02)
    lo = end + 10                                                     # a second range, apart from the box's
    assert lo + 7 <= n
    ctx.update_triangles(lo, wob[lo:lo + 7])
    assert status(ctx)["dirty_first"] == lo and status(ctx)["dirty_count"] == 7
    ctx.update_triangles(first, moved_tris[first:end])
    now = moved_tris.copy()
    now[lo:lo + 7] = wob[lo:lo + 7]
    st = status(ctx)
    assert (st["dirty_first"], st["dirty_count"], st["epochs"]) == (first, lo + 7 - first, 0)
    assert np.array_equal(bits(ctx.debug_motion_prev(0, n)), bits(uploaded))
    unchanged = (bits(verts(now)) == bits(uploaded)).all(axis=(1, 2))
    assert unchanged[first:lo + 7].any() and not unchanged[first:lo + 7].all()    # the range holds triangles rewritten unchanged, and moved ones
    want, mst, moved = check_against_model(ctx, sc, now, BASE, SIDEWAYS, snap)
    assert mst["moved"] > 0 and not unchanged[want["id"][..., 0][moved]].any()
    in_range_static = (want["id"][..., 0] >= first) & (want["id"][..., 0] < lo + 7) & ~moved
    assert in_range_static.any()                                      # pixels on a rewritten-unchanged triangle of the range: static rule
    # the reproject committed
    st = status(ctx)
    assert (st["dirty_first"], st["dirty_count"], st["epochs"]) == (0, 0, 1)
    assert np.array_equal(bits(ctx.debug_motion_prev(0, n)), bits(verts(now)))
    # ptmi_motion_commit after a further update does the same without a reproject, and touches no plane
    before = read_planes(ctx)
    ctx.update_triangles(first, sc.tris[first:end])
    assert np.array_equal(bits(ctx.debug_motion_prev(0, n)), bits(verts(now)))
    now[first:end] = sc.tris[first:end]
    ctx.motion_commit()
    st = status(ctx)
    assert (st["dirty_first"], st["dirty_count"], st["epochs"]) == (0, 0, 2)
    assert np.array_equal(bits(ctx.debug_motion_prev(0, n)), bits(verts(now)))
    same_planes(read_planes(ctx), before)
    ctx.motion_commit()                                               # nothing dirty: an epoch all the same
    assert status(ctx)["epochs"] == 3
    # an upload resets to the new scene
    ctx.update_triangles(lo, wob[lo:lo + 7])
    other = dataclasses.replace(sc, tris=moved_tris, nodes=sur.refit_nodes(sc.nodes, moved_tris))
    ctx.upload_scene(other)
    st = status(ctx)
    assert (st["on"], st["dirty_first"], st["dirty_count"], st["epochs"]) == (1, 0, 0, 0)
    assert np.array_equal(bits(ctx.debug_motion_prev(0, n)), bits(verts(moved_tris)))
    assert np.array_equal(bits(ctx.debug_motion_prev(n - 1, 1)), bits(verts(moved_tris)[n - 1:]))
    assert ctx.debug_motion_prev(n, 0).shape == (0, 3, 3)


def test_lifetime_of_the_buffers(scene_factory):
    sc = scene_factory("cornell")
    with native.Context(0) as c:
        assert not c.motion() and c.motion_device_ptr() is None
        c.set_motion(True)                                            # before an upload and a resize: the buffers appear with them
        assert c.motion() and c.motion_device_ptr() is None
        assert err(c.debug_motion_prev, 0, 1) == E_STATE and err(c.read_motion) == E_STATE
        c.upload_scene(sc)
        assert np.array_equal(bits(c.debug_motion_prev(0, len(sc.tris))), bits(verts(sc.tris)))
        c.resize(W, H)
        c.set_aovs(*ALL)
        c.set_moments(True)
        assert c.motion_device_ptr() and not c.read_motion().any()
        c.dispatch(at(BASE, 0), 2)
        c.reproject(BASE, SIDEWAYS)
        assert c.read_motion().any()
        c.resize(W, H)                                                # re-made zero-filled, like an AOV plane
        assert not c.read_motion().any()
        c.set_motion(True)                                            # again: previous := current, epochs 0
        assert status(c) == dict(on=1, epochs=0, dirty_first=0, dirty_count=0, moved=0, moved_carried=0)
        c.set_motion(False)
        assert not c.motion() and c.motion_device_ptr() is None and status(c)["on"] == 0


VARIANTS = {
    "leaves_1": (dict(leaves=1), dict(), ALL, dict()),
    "band": (dict(), dict(tile_y0=5, tile_y1=29), ALL, dict()),
    "strips": (dict(), dict(tile_parts=2, tile_part=1, tile_strip=3), ALL, dict()),
    "only_normal": (dict(), dict(), ("normal",), dict()),
    "max_history_4": (dict(), dict(), ALL, dict(max_history=4)),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variants_match_the_model(ctx, scene_factory, variant):
    opt, tile, aovs, params = VARIANTS[variant]
    sc = scene_factory("cornell")
    moved_tris, first, end = box_edit(sc)
    rendered(ctx, sc, aovs=aovs, **opt)                       # every row holds samples, the rows of other contexts too
    ctx.reproject(BASE, BASE)                                 # ... and a motion plane that is not zeros
    if tile:
        ctx.set_options(**tile)
    snap = read_planes(ctx)
    assert snap["motion"][..., 2].any()
    rows = adaptive_ref.band_rows(H, tile.get("tile_y0", 0), tile.get("tile_y1", 0), tile.get("tile_parts", 1), tile.get("tile_part", 0),
                                  tile.get("tile_strip", 1))
    ctx.update_triangles(first, moved_tris[first:end])
    want, st, moved = check_against_model(ctx, sc, moved_tris, BASE, SIDEWAYS, snap, rows=rows, **params)
    assert st["carried"] > 0 and st["disoccluded"] > 0 and st["missed"] > 0 and st["moved_carried"] > 0, st
    assert st["carried"] + st["disoccluded"] + st["missed"] == int(rows.sum()) * W
    if tile:                                                  # rows outside the context's: untouched, byte for byte
        assert snap["output"][~rows].any() and snap["motion"][~rows].any()
        for k in snap:
            assert np.array_equal(bits(want[k][~rows]), bits(snap[k][~rows])), k
    if "max_history" in params:
        assert want["moments"][..., 2].max() == params["max_history"]


def test_the_next_round_continues_every_pixel_from_its_count(ctx, oracle, scene_factory):
    sc = scene_factory("cornell")
    moved_tris, first, end = box_edit(sc)
    snap = rendered(ctx, sc)
    ctx.update_triangles(first, moved_tris[first:end])
    max_history = 6                                          # below FRAMES: the cap is in play
    want, st, moved = check_against_model(ctx, sc, moved_tris, BASE, SIDEWAYS, snap, max_history=max_history)
    assert st["moved_carried"] > 0
    counts = want["moments"][..., 2]
    assert set(np.unique(counts).tolist()) == {0.0, float(max_history)}
    p = dict(threshold=1e-9, min_frames=max_history + 4, step=4, neighbourhood=0)
    edited = dataclasses.replace(sc, tris=moved_tris, nodes=sur.refit_nodes(sc.nodes, moved_tris))
    state = adaptive_ref.State(H, W, want["output"], want["moments"])
    adaptive_ref.run_planes(oracle, edited, SIDEWAYS, p, 1, state=state, restart=False)
    assert state.active == [W * H]
    ctx.dispatch_adaptive(at(SIDEWAYS, 1), 1, **p)
    got = read_planes(ctx)
    assert np.array_equal(got["moments"][..., 2], counts + 4)
    assert np.array_equal(bits(got["output"]), bits(state.image)) and np.array_equal(bits(got["moments"]), bits(state.moments))
    assert np.array_equal(bits(got["motion"]), bits(want["motion"]))      # a dispatch leaves the motion plane alone


def test_errors_write_nothing(ctx, scene_factory):
    sc = scene_factory("cornell")
    n = len(sc.tris)
    moved_tris, first, end = box_edit(sc)
    before = rendered(ctx, sc, motion=False)
    st0 = status(ctx)
    for call, args in ((ctx.read_motion, ()), (ctx.motion_commit, ()), (ctx.debug_motion_prev, (0, 1))):
        assert err(call, *args) == E_STATE                            # while off
        same_planes(read_planes(ctx), before)
        assert status(ctx) == st0 and st0["on"] == 0
    assert err(ctx.set_motion, 2) == E_INVALID
    assert not ctx.motion()
    ctx.set_motion(True)
    ctx.update_triangles(first, moved_tris[first:end])
    before, prev0, st0 = read_planes(ctx), ctx.debug_motion_prev(0, n), status(ctx)
    assert st0["dirty_count"] == end - first

    def unchanged():
        same_planes(read_planes(ctx), before)
        assert np.array_equal(bits(ctx.debug_motion_prev(0, n)), bits(prev0)) and status(ctx) == st0

    assert err(ctx.set_motion, 2) == E_INVALID
    unchanged()
    assert ctx.motion()
    for bad in (W * H * 4 - 1, W * H * 4 + 4, 0):
        assert err(ctx.read_motion, bad) == E_INVALID
        unchanged()
    for a, b in ((0, n + 1), (n, 1), (n - 1, 2), (0xFFFFFFFF, 2)):
        assert err(ctx.debug_motion_prev, a, b) == E_INVALID
        unchanged()
    other = layout.make_camera(W + 1, H)
    assert err(ctx.reproject, BASE, other) == E_INVALID               # a failed reproject writes nothing and commits nothing
    unchanged()
    assert err(ctx.reproject, BASE, SIDEWAYS, reserved=(0, 0, 0, 0, 1)) == E_INVALID
    unchanged()
