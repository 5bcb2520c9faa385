"""ptmi_reproject on the GPU (include/ptmi.h) against tests/reproject_ref.py, bit for bit: the model is fed the device's own centre
rays (ptmi_debug_center_rays), their closest hits (ptmi_debug_intersect) and tan(fov / 2) as the kernels compute it (ptmi_debug_math
op 11), so what is compared is step 4 of the pass and the snapshot in front of it. Two further tests keep a wrong count or a stale
plane from hiding behind the model: with everything disoccluded the next adaptive round must leave exactly a fresh render, and after
a real move it must fold the frames count .. count + 3 of every pixel onto the reprojected values."""
import numpy as np
import pytest

import adaptive_ref
import reproject_ref
from ptmi import layout, native

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, FRAMES = 70, 37, 8                    # a width that is no multiple of the 64-pixel row segment of a wave
E_INVALID, E_STATE = -1, -4
ALL = ("albedo", "normal", "id")
MISS = reproject_ref.MISS


def yawed(deg):
    a = np.radians(deg)
    return dict(forward=(-np.sin(a), 0.0, -np.cos(a)), right=(np.cos(a), 0.0, -np.sin(a)))


BASE = layout.make_camera(W, H)
MOVES = {"sideways": layout.make_camera(W, H, position=(0.3, 1.0, 2.8)), "yaw": layout.make_camera(W, H, **yawed(10.0)),
         "dolly": layout.make_camera(W, H, position=(0.0, 1.0, 2.2))}


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the planes and options it sets never reach the session's shared context"""
    c = native.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def at(cam, frame):
    c = cam.copy()
    c["frame_index"] = frame
    return c


def err(fn, *a, **kw):
    with pytest.raises(native.PtmiError) as e:
        fn(*a, **kw)
    return e.value.code


def setup(ctx, sc, aovs=ALL, moments=True, size=(W, H), **opt):
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=0,
             overlap=2, perf_mode=0, leaves=0, timing=0)
    o.update(opt)
    if ctx.width:
        ctx.bind_output_device(0, 0)
    ctx.set_aovs()
    ctx.set_moments(False)
    ctx.set_options(**o)
    ctx.upload_scene(sc)
    ctx.resize(*size)
    ctx.set_aovs(*aovs)
    ctx.set_moments(moments)
    ctx.reset_stats()


def read_planes(ctx):
    on = ctx.aovs()
    return dict(output=ctx.read_output(), moments=ctx.read_moments() if ctx.moments() else None,
                normal=ctx.read_aov("normal") if "normal" in on else None, albedo=ctx.read_aov("albedo") if "albedo" in on else None, id=ctx.read_aov("id") if "id" in on else None)


def same_planes(got, want):
    """bit for bit, two NaNs of any payload counting as equal"""
    for k, w in want.items():
        g = got[k]
        if w is None or g is None:
            assert w is None and g is None, k
            continue
        if w.dtype == np.uint32:
            assert np.array_equal(g, w), k
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), k
        assert np.array_equal(bits(g)[~nan], bits(w)[~nan]), (k, int((bits(g) != bits(w)).sum()))


def model(ctx, sc, snap, cam_from, cam_to, rows=None, **params):
    """tests/reproject_ref.py on the device's own centre rays, hits and tan"""
    o, d = ctx.debug_center_rays(cam_to)
    t, tri, _, _ = ctx.debug_intersect(o, d)
    assert ((tri == MISS) == (t < 0)).all()
    th = ctx.debug_math(11, np.array([f32(cam_from["fov"]) * f32(0.5)], f32))[0]
    return reproject_ref.reproject(snap, cam_from, o, d, t, tri, sc.tris["material_index"], th, rows=rows, **params)


def rendered(ctx, sc, cam=BASE, aovs=ALL, frames=FRAMES, **opt):
    """FRAMES frames of `cam` in a context set up afresh; returns the planes they leave"""
    setup(ctx, sc, aovs=aovs, **opt)
    ctx.dispatch(at(cam, 0), frames)
    return read_planes(ctx)


def check_against_model(ctx, sc, cam_from, cam_to, snap, rows=None, **params):
    want, want_st = model(ctx, sc, snap, cam_from, cam_to, rows=rows, **params)
    ctx.reproject(cam_from, cam_to, **params)
    got, got_st = read_planes(ctx), ctx.reproject_status().as_dict()
    print("status", got_st, "model", want_st)
    same_planes(got, want)
    assert got_st == want_st
    return want, want_st


@pytest.mark.parametrize("move", sorted(MOVES))
@pytest.mark.parametrize("name", ["cornell", "feature_box"])
def test_matches_the_model(ctx, scene_factory, name, move):
    sc = scene_factory(name)
    snap = rendered(ctx, sc)
    assert (snap["moments"][..., 2] == FRAMES).all()
    want, st = check_against_model(ctx, sc, BASE, MOVES[move], snap)
    # all three outcomes occur, or the comparison shows nothing
    assert st["carried"] > 0 and st["disoccluded"] > 0 and st["missed"] > 0, st
    assert st["carried"] + st["disoccluded"] + st["missed"] == W * H
    assert st["samples"] == st["carried"] * FRAMES                       # every tap had FRAMES samples, below the cap of 32


VARIANTS = {
    "match_ids_never": (dict(), ALL, dict(match_ids=1)),
    "match_ids_always": (dict(), ALL, dict(match_ids=2)),
    "albedo_off": (dict(), ("normal", "id"), dict()),
    "id_off": (dict(), ("albedo", "normal"), dict()),
    "only_normal": (dict(), ("normal",), dict()),
    "max_history_4": (dict(), ALL, dict(max_history=4)),
    "tight_depth": (dict(), ALL, dict(depth_tolerance=1e-3)),
    "band": (dict(tile_y0=5, tile_y1=29), ALL, dict()),
    "strips": (dict(tile_parts=2, tile_part=1, tile_strip=3), ALL, dict()),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variants_match_the_model(ctx, scene_factory, variant):
    tile, aovs, params = VARIANTS[variant]
    sc = scene_factory("cornell")
    rendered(ctx, sc, aovs=aovs)                             # every row holds samples, the rows of other contexts too
    if tile:
        ctx.set_options(**tile)
    snap = read_planes(ctx)
    rows = adaptive_ref.band_rows(H, tile.get("tile_y0", 0), tile.get("tile_y1", 0), tile.get("tile_parts", 1), tile.get("tile_part", 0),
                                  tile.get("tile_strip", 1))
    want, st = check_against_model(ctx, sc, BASE, MOVES["sideways"], snap, rows=rows, **params)
    assert st["carried"] > 0 and st["disoccluded"] > 0 and st["missed"] > 0, st
    assert st["carried"] + st["disoccluded"] + st["missed"] == int(rows.sum()) * W
    if tile:                                                 # rows outside the context's: untouched, byte for byte (the model keeps them)
        assert snap["output"][~rows].any()
        for k in snap:
            assert np.array_equal(bits(want[k][~rows]), bits(snap[k][~rows])), k
    if "max_history" in params:
        assert want["moments"][..., 2].max() == params["max_history"]


def test_center_rays(ctx, scene_factory):
    setup(ctx, scene_factory("cornell"))
    for cam in (BASE, MOVES["yaw"], layout.make_camera(W, H, position=(0.3, 1.0, 2.8), aperture=0.3)):     # the aperture is ignored
        o, d = ctx.debug_center_rays(cam)
        o64, d64 = reproject_ref.center_rays64(cam)
        assert np.array_equal(bits(o), bits(np.broadcast_to(cam["position"], o.shape)))
        worst = np.abs(d.astype(np.float64) - d64).max()
        print("centre ray directions: worst component error", worst)
        assert worst <= 2e-6
    assert err(ctx.debug_center_rays, layout.make_camera(W + 1, H)) == E_INVALID


def away(cam):
    c = cam.copy()
    c["forward"] = -c["forward"]
    return c


def test_everything_disoccluded_then_a_round_equals_a_fresh_render(ctx, scene_factory):
    sc = scene_factory("cornell")
    to = MOVES["sideways"]
    fresh = rendered(ctx, sc, cam=to, frames=4)
    rendered(ctx, sc)
    ran = ctx.stats()
    ctx.set_options(traversal=native.TRAVERSAL_GLOBAL_EXACT)        # the centre rays are traced by another variant than the dispatch ran
    ctx.reproject(away(BASE), to)
    ctx.set_options(traversal=native.TRAVERSAL_AUTO)
    after = ctx.stats()                                              # ... and the statistics still name the dispatch's
    assert (after.extend_variant, after.shadow_variant) == (ran.extend_variant, ran.shadow_variant) and ran.extend_variant // 10 not in (1, 9)
    st = ctx.reproject_status().as_dict()
    assert st["carried"] == 0 and st["samples"] == 0 and st["disoccluded"] > 0 and st["missed"] > 0
    assert st["disoccluded"] + st["missed"] == W * H
    got = read_planes(ctx)
    for k in ("output", "moments", "normal", "albedo"):
        assert not got[k].any(), k
    ctx.dispatch_adaptive(at(to, 1), 1, threshold=0.5, min_frames=4, step=4)
    same_planes(read_planes(ctx), fresh)


def test_a_round_after_a_move_continues_every_pixel_from_its_count(ctx, oracle, scene_factory):
    sc = scene_factory("cornell")
    to = MOVES["sideways"]
    snap = rendered(ctx, sc)
    max_history = 6                                          # below FRAMES: the cap is in play
    want, st = check_against_model(ctx, sc, BASE, to, snap, max_history=max_history)
    counts = want["moments"][..., 2]
    assert set(np.unique(counts).tolist()) == {0.0, float(max_history)}
    p = dict(threshold=1e-9, min_frames=max_history + 4, step=4, neighbourhood=0)
    state = adaptive_ref.State(H, W, want["output"], want["moments"])
    adaptive_ref.run_planes(oracle, sc, to, p, 1, state=state, restart=False)
    assert state.active == [W * H]
    ctx.dispatch_adaptive(at(to, 1), 1, **p)
    got = read_planes(ctx)
    assert np.array_equal(got["moments"][..., 2], counts + 4)
    # every pixel, the missed ones (count 0: frames 0 .. 3 overwrite) included
    assert np.array_equal(bits(got["output"]), bits(state.image)) and np.array_equal(bits(got["moments"]), bits(state.moments))


def test_errors_write_nothing(ctx, scene_factory):
    sc = scene_factory("cornell")
    to = MOVES["sideways"]
    fresh = native.Context(0)
    try:
        assert err(fresh.reproject, BASE, to) == E_STATE                             # no scene
        fresh.upload_scene(sc)
        assert err(fresh.reproject, BASE, to) == E_STATE                             # no output buffer
        assert fresh.reproject_status().as_dict() == dict(carried=0, disoccluded=0, missed=0, samples=0)
    finally:
        fresh.close()

    def unchanged(before):
        same_planes(read_planes(ctx), before)

    before = rendered(ctx, sc, aovs=("albedo", "id"))
    assert err(ctx.reproject, BASE, to) == E_STATE                                   # the NORMAL plane is off
    unchanged(before)
    before = rendered(ctx, sc, moments=False)
    assert err(ctx.reproject, BASE, to) == E_STATE                                   # the moments plane is off
    unchanged(before)
    before = rendered(ctx, sc, aovs=("albedo", "normal"))
    assert err(ctx.reproject, BASE, to, match_ids=2) == E_STATE                      # match_ids = 2 without the ID plane
    unchanged(before)
    before = rendered(ctx, sc)
    L = ctx.L
    cam_p = BASE.ctypes.data_as(native.ctypes.c_void_p)
    assert L.ptmi_reproject(ctx.h, None, cam_p, None) == E_INVALID                   # from NULL
    assert L.ptmi_reproject(ctx.h, cam_p, None, None) == E_INVALID                   # to NULL
    other = layout.make_camera(W + 1, H)
    taller = layout.make_camera(W, H + 1)
    for a, b, kw in ((other, to, {}), (BASE, other, {}), (taller, to, {}), (BASE, taller, {}),
                     (BASE, to, dict(depth_tolerance=-0.01)), (BASE, to, dict(depth_tolerance=float("nan"))),
                     (BASE, to, dict(depth_tolerance=float("inf"))), (BASE, to, dict(max_history=(1 << 24) + 1)),
                     (BASE, to, dict(match_ids=3)), (BASE, to, dict(reserved=(1, 0, 0, 0, 0))), (BASE, to, dict(reserved=(0, 0, 0, 0, 7)))):
        assert err(ctx.reproject, a, b, **kw) == E_INVALID, kw
        unchanged(before)
    assert L.ptmi_reproject(ctx.h, cam_p, to.ctypes.data_as(native.ctypes.c_void_p), None) == 0      # params NULL: the defaults
    want, _ = model(ctx, sc, before, BASE, to)
    same_planes(read_planes(ctx), want)
    ctx.reproject(BASE, to, max_history=1 << 24)                                     # the largest cap is accepted


def test_caller_bound_output(ctx, scene_factory):
    import torch
    sc = scene_factory("cornell")
    to = MOVES["sideways"]
    snap = rendered(ctx, sc)
    ctx.reproject(BASE, to)
    unbound = read_planes(ctx)
    setup(ctx, sc)
    frame = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    own = ctx.output_device_ptr()
    ctx.bind_output_device(frame.data_ptr(), frame.numel() * 4)
    ctx.dispatch(at(BASE, 0), FRAMES)
    ctx.synchronize()
    assert np.array_equal(bits(frame.cpu().numpy().reshape(H, W, 4)), bits(snap["output"]))
    ctx.reproject(BASE, to)
    ctx.synchronize()
    same_planes(read_planes(ctx), unbound)
    assert np.array_equal(bits(frame.cpu().numpy().reshape(H, W, 4)), bits(unbound["output"]))
    ctx.bind_output_device(0, 0)
    assert ctx.output_device_ptr() == own
    assert not ctx.read_output().any()                                               # the context's own buffer was never written
