"""Camera projections on the GPU (include/ptmi.h ptmi_set_projections) against tests/projection_ref.py and the CPU
oracle, bit for bit. The oracle renders the pinhole only, which is all it needs to: the model's ray (org0, raw) of a pixel is that
pixel of the oracle camera with position = org0, forward = raw, fov = 0 (tests/test_projection_host.py), so whole renders are pinned
per sample through Oracle.trace_paths with one camera per pixel.

  1. off means off: the goldens keep their bits with garbage in the two words and the switch off, and with the switch on, kind 0 and
     a NaN ymag, through ptmi_dispatch and an adaptive round of every pixel
  2. ptmi_debug_raygen and ptmi_debug_center_rays against the model: origin, direction, RNG state
  3. renders per sample, cornell and feature_box, the output after every one-frame dispatch; depth and ids of frame 0; one
     orthographic case under an environment map (oracle) and under a blend table (the device's own pinhole kernels, pixel by pixel)
  4. the dispatch paths agree: n frames = n dispatches = an adaptive round of every pixel = two and three loopback contexts
  5. reprojection from an orthographic camera against the model, with motion, onto itself; an equirectangular camera is refused
  6. a bad camera is PTMI_E_INVALID from every entry that takes one, and nothing is written

Every case fails without the feature: the binding has no set_projections."""
import numpy as np
import pytest

import adaptive_ref
import env_ref
import projection_ref as pr
import reproject_ref
from ptmi import layout, native, scenes
from test_golden import HERE, load, same
from test_gpu_parity import assert_same_floats, bits
from test_projection_host import APERTURES, FRAMES, SIZES, all_pixels, rotated_basis

pytestmark = pytest.mark.gpu

f32 = np.float32
E_INVALID = -1
MISS = 0xFFFFFFFF
PROJECTIONS = ("orthographic", "equirect")
GARBAGE = 0xDEADBEEF
RW, RH, RFRAMES, RBOUNCES = 16, 12, 3, 4            # the per-sample renders
DW, DH = 70, 33                                     # the dispatch paths: neither a multiple of 64
PW, PH = 65, 33                                     # reprojection


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the switch, planes and options it sets never reach the session's shared context"""
    with native.Context(0) as c:
        yield c
        c.set_projections(False)


def at(cam, frame):
    cam = cam.copy()
    cam["frame_index"] = frame
    return cam


def err(fn, *a, **kw):
    with pytest.raises(native.PtmiError) as e:
        fn(*a, **kw)
    return e.value.code


def setup(c, sc, W, H, aovs=(), moments=False, projections=True, **opt):
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=0, cull=1,
             traversal=0, overlap=2, perf_mode=0, leaves=0, timing=0)
    o.update(opt)
    c.set_options(**o)
    if isinstance(c, native.Context):
        c.set_motion(False)
    c.upload_scene(sc)
    c.upload_environment(None)
    c.set_medium(None)
    c.set_aovs(*aovs)
    c.set_moments(moments)
    c.resize(W, H)
    c.set_projections(projections)
    c.reset_stats()


def view(W, H, projection, aperture=0.05, ymag=1.15, position=None, **kw):
    """a camera turned about all three axes (no component of forward, or of any equirectangular direction, is a zero) that looks
    into the box from its open side (orthographic) or stands inside it (equirect)"""
    if position is None:
        position = (0.11, 1.03, 2.6) if projection != "equirect" else (0.11, 1.03, 0.35)
    basis = rotated_basis(0.17, -0.11, 0.07)
    basis.update(kw)
    return layout.make_camera(W, H, position=position, aperture=aperture, focus_distance=2.75, projection=projection, ymag=ymag, **basis)


def pixels(W, H):
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    return xs, ys


# ---- 1. off means off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["off_garbage", "on_kind0_nan"])
@pytest.mark.parametrize("name", ["cornell_64x48_4spp_mis", "cornell_64x64_4spp_b4_nomis"])
def test_goldens_keep_their_bits(ctx, name, how):
    z, sc, cam = load(HERE + "/golden/" + name + ".npz")
    W, H, frames = int(cam["width"]), int(cam["height"]), int(z["frames"])
    cam = cam.copy()
    if how == "off_garbage":
        cam["_p3"] = (GARBAGE, GARBAGE)
    else:
        cam["_p3"] = (0, 0x7FC00000)
    setup(ctx, sc, W, H, moments=True, projections=how != "off_garbage", max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
    assert ctx.projections() == (how != "off_garbage")
    ctx.dispatch(at(cam, 0), frames)
    out, st = ctx.read_output(), ctx.stats()
    assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"])
    assert same(out, z["image"])
    # one adaptive round in which every pixel is below min_frames and receives `frames` frames
    ctx.write_output(np.zeros((H, W, 4), f32))
    ctx.dispatch_adaptive(at(cam, 0), 1, threshold=1e-3, min_frames=frames, max_frames=frames, step=frames)
    assert ctx.adaptive_status().active == W * H
    assert same(ctx.read_output(), z["image"])
    # the centre rays and the listed raygen too: the pinhole's, whatever the words say
    clean = cam.copy()
    clean["_p3"] = 0
    ctx.set_projections(False)
    want_c, want_r = ctx.debug_center_rays(clean), ctx.debug_raygen(clean, *all_pixels(7, 5))
    ctx.set_projections(how != "off_garbage")
    for got, want in zip(ctx.debug_center_rays(cam) + ctx.debug_raygen(cam, *all_pixels(7, 5)), want_c + want_r):
        assert same(got, want)


def test_the_switch(ctx):
    assert err(ctx.set_projections, 2) == E_INVALID
    ctx.set_projections(True)
    assert ctx.projections() is True
    assert err(ctx.set_projections, 7) == E_INVALID and ctx.projections() is True
    ctx.set_projections(False)
    assert ctx.projections() is False


# ---- 2. rays -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aperture", APERTURES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("projection", PROJECTIONS)
def test_rays_match_the_model(ctx, oracle, projection, size, aperture):
    W, H = size
    cam = view(W, H, projection, aperture)
    ctx.resize(W, H)
    ctx.set_projections(True)
    xs, ys, fr = all_pixels(W, H, FRAMES)                    # every pixel: the first and last column and row are among them
    m = pr.rays(oracle, cam, xs, ys, fr)
    o, d, rng = ctx.debug_raygen(cam, xs, ys, fr)
    assert_same_floats(o, m["o"], "origins")
    assert_same_floats(d, m["d"], "directions")
    assert np.array_equal(rng, m["rng"])
    px, py = pixels(W, H)
    mc = pr.rays(oracle, cam, px, py)
    oc, dc = ctx.debug_center_rays(cam)
    assert_same_floats(oc, mc["o"], "centre origins")
    assert_same_floats(dc, mc["d"], "centre directions")
    if projection == "equirect":                            # the corner pixels are half a pixel from lon = +-pi, lat = +-pi / 2
        up, fw = np.asarray(cam["up"], np.float64), np.asarray(cam["forward"], np.float64)
        lat = np.degrees(np.arcsin(np.clip(dc @ up, -1, 1)))
        assert abs(lat[0] + 90 * (1 - 1 / H)) < 1e-3 and abs(lat[-1] - 90 * (1 - 1 / H)) < 1e-3
        assert (dc[[0, W - 1]] @ fw < 0).all()               # the first and last column look backwards
    else:
        assert (bits(dc) == bits(dc[0])[None, :]).all() and not (bits(oc) == bits(oc[0])[None, :]).all(axis=1)[1:].any()


# ---- 3. renders, per sample ----------------------------------------------------------------------------------------------------------
def per_pixel_cameras(oracle, cam, frame):
    xs, ys = pixels(int(cam["width"]), int(cam["height"]))
    m = pr.rays(oracle, cam, xs, ys, np.full(len(xs), frame, np.uint32))
    return xs, ys, m, pr.fov0_cameras(cam, m["org0"], m["raw"])


def oracle_radiance(oracle, sc, cam, frame, extras=None):
    """per pixel, the radiance of the oracle's path (x, y, frame) under the pixel's own fov = 0 camera; (n, 3), and the paths whose
    sky lookups came within the band of a texel border (with extras)"""
    xs, ys, m, cams = per_pixel_cameras(oracle, cam, frame)
    rad, aside = np.zeros((len(xs), 3), f32), np.zeros(len(xs), bool)
    for i in range(len(xs)):
        a = (sc, cams[i:i + 1], xs[i:i + 1], ys[i:i + 1], [frame])
        if extras is None:
            rad[i] = oracle.trace_paths(*a, max_bounces=RBOUNCES, do_mis=1, threads=1)[0][0]
        else:
            r, _, border = oracle.trace_paths_ext(*a, extras, max_bounces=RBOUNCES, do_mis=1, threads=1)
            rad[i], aside[i] = r[0], border[0] < env_ref.BORDER_BAND
    return rad, aside, m


@pytest.mark.parametrize("projection", PROJECTIONS)
@pytest.mark.parametrize("name", ["cornell", "feature_box"])
def test_renders_per_sample(ctx, oracle, scene_factory, name, projection):
    sc = scene_factory(name)
    cam = view(RW, RH, projection)
    setup(ctx, sc, RW, RH, aovs=("normal", "id"), moments=True, max_bounces=RBOUNCES)
    rgb, mom = np.zeros((RW * RH, 3), f32), np.zeros((RW * RH, 4), f32)
    for f in range(RFRAMES):
        rad, _, m = oracle_radiance(oracle, sc, cam, f)
        rgb, mom = adaptive_ref.fold_listed(rgb, mom, rad, np.full(RW * RH, f, np.uint32))
        ctx.dispatch(at(cam, f), 1)
        out = ctx.read_output().reshape(-1, 4)
        assert_same_floats(out[:, :3], rgb, "%s %s, after frame %d" % (name, projection, f))
        assert not out[:, 3].any()
        assert_same_floats(ctx.read_moments().reshape(-1, 4), mom, "moments after frame %d" % f)
        if f == 0:                                          # depth and ids: the first hit of the model's frame-0 ray
            t, tri, _, _, _ = oracle.intersect(sc, m["o"], m["d"])
            nrm, ids = ctx.read_aov("normal").reshape(-1, 4), ctx.read_aov("id").reshape(-1, 2)
            hit = tri != MISS
            assert hit.mean() > 0.5
            assert np.array_equal(ids[:, 0], tri)
            assert np.array_equal(ids[hit, 1], sc.tris["material_index"][tri[hit]]) and (ids[~hit, 1] == MISS).all()
            assert_same_floats(nrm[:, 3], np.where(hit, t, f32(0)), "depth")
    assert np.isfinite(rgb).all() and rgb.max() > 0.05       # a picture, not a black frame


def test_orthographic_render_under_an_environment_map(ctx, oracle, scene_factory):
    sc = scene_factory("cornell")
    cam = view(RW, RH, "orthographic", ymag=1.6)             # wider than the box: rays pass beside it into the sky
    texels = scenes.sky(16, 8, "disc")
    c, prob, alias, wsum = native.env_table(texels)
    extras = oracle.extras(dict(texels=texels, c=c, prob=prob, alias=alias, sampled=int(wsum > 0), intensity=1.0))
    setup(ctx, sc, RW, RH, max_bounces=RBOUNCES)
    try:
        ctx.upload_environment(texels)
        rgb, mom, aside = np.zeros((RW * RH, 3), f32), np.zeros((RW * RH, 4), f32), np.zeros(RW * RH, bool)
        for f in range(RFRAMES):
            rad, a, _ = oracle_radiance(oracle, sc, cam, f, extras)
            aside |= a
            rgb, mom = adaptive_ref.fold_listed(rgb, mom, rad, np.full(RW * RH, f, np.uint32))
            ctx.dispatch(at(cam, f), 1)
        out = ctx.read_output().reshape(-1, 4)
    finally:
        ctx.upload_environment(None)
    print("paths set aside for a sky lookup within the border band: %d of %d pixels" % (aside.sum(), aside.size))
    assert aside.mean() < 0.25
    assert_same_floats(out[~aside, :3], rgb[~aside], "orthographic under a sky")


def test_orthographic_render_under_a_blend_table(ctx, scene_factory):
    """the oracle has no alpha blending: the reference is the device's own pinhole path, one dispatch per pixel with that pixel's
    fov = 0 camera and the switch off, under the same table (the hash is the ray's own, and the rays are the same)"""
    from oracle_lib import Oracle
    oracle = Oracle()
    sc = scene_factory("cornell")
    W, H, frames = 8, 6, 2
    cam = view(W, H, "orthographic")
    table = np.full(len(sc.mats), 0.5, f32)
    setup(ctx, sc, W, H, max_bounces=RBOUNCES)
    try:
        ctx.set_alpha_blend(table, seed=3)
        for f in range(frames):
            ctx.dispatch(at(cam, f), 1)
        got = ctx.read_output().reshape(-1, 4)
        assert ctx.alpha_blend_status().as_dict()["path_passes"] > 0
        ctx.set_projections(False)
        want = np.zeros((W * H, 4), f32)
        for f in range(frames):
            xs, ys, m, cams = per_pixel_cameras(oracle, cam, f)
            ctx.write_output(want.reshape(H, W, 4))
            frame_f = want.copy()
            for i in range(W * H):
                ctx.write_output(want.reshape(H, W, 4))
                ctx.dispatch(at(cams[i:i + 1], f), 1)
                frame_f[i] = ctx.read_output().reshape(-1, 4)[i]
            want = frame_f
    finally:
        ctx.set_alpha_blend(None)
    assert_same_floats(got, want, "orthographic under a blend table")


# ---- 4. the dispatch paths agree -----------------------------------------------------------------------------------------------------
def test_dispatch_paths_agree(ctx, scene_factory):
    sc = scene_factory("cornell")
    cam = view(DW, DH, "orthographic", ymag=1.3)
    n = 4
    setup(ctx, sc, DW, DH, moments=True, max_bounces=RBOUNCES)
    ctx.dispatch(at(cam, 0), n)
    whole = ctx.read_output()
    assert whole[..., :3].max() > 0.05
    ctx.write_output(np.zeros_like(whole))
    for f in range(n):
        ctx.dispatch(at(cam, f), 1)
    assert same(ctx.read_output(), whole)
    ctx.write_output(np.zeros_like(whole))
    ctx.dispatch_adaptive(at(cam, 0), 1, threshold=1e-3, min_frames=n, max_frames=n, step=n)
    assert ctx.adaptive_status().active == DW * DH
    assert same(ctx.read_output(), whole)
    # the perspective kernels give another picture from the same record: the words are what selects
    ctx.set_projections(False)
    ctx.write_output(np.zeros_like(whole))
    ctx.dispatch(at(cam, 0), n)
    assert not same(ctx.read_output(), whole)
    for devices in (2, 3):
        with native.MultiContext([0] * devices, loopback=True) as m:
            setup(m, sc, DW, DH, moments=True, max_bounces=RBOUNCES)
            assert m.projections() is True
            m.dispatch(at(cam, 0), n)
            assert same(m.read_output(), whole), devices
            m.write_output(np.zeros_like(whole))
            m.dispatch_adaptive_rounds(at(cam, 0), 1, threshold=1e-3, min_frames=n, max_frames=n, step=n, neighbourhood=1)
            assert same(m.read_output(), whole), devices
            bad = view(DW, DH, 3)
            before = m.stats().dispatches
            assert err(m.dispatch, bad, 1) == E_INVALID
            assert err(m.dispatch_adaptive_rounds, bad, 1, threshold=1e-3) == E_INVALID
            assert m.stats().dispatches == before and same(m.read_output(), whole)
            assert err(m.set_projections, 2) == E_INVALID
            m.set_projections(False)
            assert m.projections() is False


# ---- 5. reprojection -----------------------------------------------------------------------------------------------------------------
ALL = ("albedo", "normal", "id")


def read_planes(c, motion=False):
    p = dict(output=c.read_output(), moments=c.read_moments(), normal=c.read_aov("normal"), albedo=c.read_aov("albedo"), id=c.read_aov("id"))
    if motion:
        p["motion"] = c.read_motion()
    return p


def same_planes(got, want):
    for k, w in want.items():
        if w.dtype == np.uint32:
            assert np.array_equal(got[k], w), k
        else:
            assert_same_floats(got[k], w, k)


def model_reproject(c, sc, snap, cam_from, cam_to, **kw):
    """the model of the `from` camera's projection on the device's own centre rays of `to`, their hits and (pinhole) tan"""
    o, d = c.debug_center_rays(cam_to)
    t, tri, u, v = c.debug_intersect(o, d)
    if pr.projection_of(cam_from)[0] == pr.ORTHOGRAPHIC:
        if "prev" in kw:
            kw.update(u=u, v=v)
        return pr.reproject_ortho(snap, cam_from, o, d, t, tri, sc.tris["material_index"], **kw)
    th = c.debug_math(11, np.array([f32(cam_from["fov"]) * f32(0.5)], f32))[0]
    return reproject_ref.reproject(snap, cam_from, o, d, t, tri, sc.tris["material_index"], th)


ORTHO_A = dict(projection="orthographic", ymag=1.15)
ORTHO_B = dict(projection="orthographic", ymag=1.0, position=(0.21, 1.08, 2.6))     # a small pan and a change of ymag
PAIRS = {"ortho_to_ortho": (ORTHO_A, ORTHO_B), "perspective_to_ortho": (dict(projection="perspective"), ORTHO_A),
         "ortho_to_perspective": (ORTHO_A, dict(projection="perspective", position=(0.2, 1.0, 2.7)))}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_reprojection_matches_the_model(ctx, scene_factory, pair):
    sc = scene_factory("cornell")
    cam_from, cam_to = (view(PW, PH, aperture=0.0, **kw) for kw in PAIRS[pair])
    setup(ctx, sc, PW, PH, aovs=ALL, moments=True)
    ctx.dispatch(at(cam_from, 0), 6)
    snap = read_planes(ctx)
    want, want_st = model_reproject(ctx, sc, snap, cam_from, cam_to)
    ctx.reproject(cam_from, cam_to)
    got, got_st = read_planes(ctx), ctx.reproject_status().as_dict()
    print(pair, got_st)
    same_planes(got, want)
    assert got_st == want_st
    # both outcomes of a hit occur, or the comparison shows nothing
    assert got_st["carried"] > 100 and got_st["disoccluded"] > 0 and got_st["carried"] + got_st["disoccluded"] + got_st["missed"] == PW * PH


def test_reprojection_onto_the_same_orthographic_camera(ctx, scene_factory):
    """a view of the back wall alone, at a slant: every pixel's jittered samples lie on the one surface, within 0.1 % of the centre
    ray's depth (checked with the oracle when the view was chosen), so no tap can fail the depth or the material test"""
    sc = scene_factory("cornell")
    cam = view(PW, PH, aperture=0.0, projection="orthographic", ymag=0.2, position=(0.3, 1.5, 1.0))
    setup(ctx, sc, PW, PH, aovs=ALL, moments=True)
    ctx.set_motion(True)
    try:
        ctx.dispatch(at(cam, 0), 6)
        snap = read_planes(ctx)
        hits = int((snap["id"][..., 0] != MISS).sum())
        cur = np.stack([sc.tris[k] for k in ("v0", "v1", "v2")], axis=1)
        want, want_st = model_reproject(ctx, sc, snap, cam, cam, prev=cur, cur=cur, dirty=(0, 0))
        ctx.reproject(cam, cam)
        got, st = read_planes(ctx, motion=True), ctx.reproject_status().as_dict()
        same_planes(got, want)
        assert st["carried"] == hits == PW * PH and st["disoccluded"] == 0, st
        carried = got["motion"][..., 3] == 0
        # within the model's bits of zero: fx - x of a point projected back where it came from, a few float32 roundings of a pixel index
        assert np.abs(got["motion"][carried][:, :2]).max() < 1e-3
    finally:
        ctx.set_motion(False)


def test_the_motion_planes_depth_is_zf(ctx, scene_factory):
    sc = scene_factory("cornell")
    cam_from, cam_to = view(PW, PH, aperture=0.0, **ORTHO_A), view(PW, PH, aperture=0.0, **ORTHO_B)
    setup(ctx, sc, PW, PH, aovs=ALL, moments=True)
    ctx.set_motion(True)
    try:
        ctx.dispatch(at(cam_from, 0), 6)
        snap = read_planes(ctx)
        seen = snap["id"][..., 0].ravel()
        count = 38                                           # 38 triangles moved, around the one most pixels see
        first = int(np.clip(int(np.bincount(seen[seen != MISS]).argmax()) - count // 2, 0, len(sc.tris) - count))
        prev = np.stack([sc.tris[k] for k in ("v0", "v1", "v2")], axis=1).copy()
        moved = sc.tris[first:first + count].copy()
        for k in ("v0", "v1", "v2"):
            moved[k] += np.asarray((0.05, 0.02, -0.03), f32)
        ctx.update_triangles(first, moved)
        cur = prev.copy()
        cur[first:first + count] = np.stack([moved[k] for k in ("v0", "v1", "v2")], axis=1)
        want, want_st = model_reproject(ctx, sc, snap, cam_from, cam_to, prev=prev, cur=cur, dirty=(first, count))
        ctx.reproject(cam_from, cam_to)
        got = read_planes(ctx, motion=True)
        st = dict(ctx.reproject_status().as_dict(), **{k: v for k, v in ctx.motion_status().as_dict().items() if k in ("moved", "moved_carried")})
        print(st)
        same_planes(got, want)
        assert st == want_st and st["moved"] > 0
        # z is zf: the distance along forward of the projected point from the camera plane, not its distance from the position
        o, d = ctx.debug_center_rays(cam_to)
        t, tri, _, _ = ctx.debug_intersect(o, d)
        static = (tri != MISS) & ~((tri >= first) & (tri < first + count))
        P = o + t[:, None] * d
        v = P - np.asarray(cam_from["position"], f32)[None, :]
        zf = (v[:, 0] * cam_from["forward"][0] + v[:, 1] * cam_from["forward"][1] + v[:, 2] * cam_from["forward"][2]).astype(f32)
        z = got["motion"].reshape(-1, 4)[:, 2]
        proj = static & (zf > 0)
        assert proj.sum() > 100
        assert_same_floats(z[proj], zf[proj], "motion.z")
    finally:
        ctx.set_motion(False)
        ctx.upload_scene(sc)


@pytest.mark.parametrize("side", ["from", "to"])
def test_reprojection_refuses_an_equirectangular_camera(ctx, scene_factory, side):
    sc = scene_factory("cornell")
    ortho, pano = view(PW, PH, aperture=0.0, **ORTHO_A), view(PW, PH, "equirect", aperture=0.0)
    setup(ctx, sc, PW, PH, aovs=ALL, moments=True)
    ctx.dispatch(at(ortho, 0), 2)
    before = read_planes(ctx)
    assert err(ctx.reproject, *((pano, ortho) if side == "from" else (ortho, pano))) == E_INVALID
    same_planes(read_planes(ctx), before)


# ---- 6. validation -------------------------------------------------------------------------------------------------------------------
BAD = {"kind_3": (3, 1.0), "ymag_zero": (1, 0.0), "ymag_negative": (1, -1.0), "ymag_infinite": (1, np.inf), "ymag_nan": (1, np.nan),
       "kind_garbage": (GARBAGE, 1.0)}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_a_bad_camera_is_refused_everywhere(ctx, scene_factory, bad):
    sc = scene_factory("cornell")
    good = view(PW, PH, aperture=0.0, **ORTHO_A)
    cam = layout.set_projection(good.copy(), *BAD[bad])
    setup(ctx, sc, PW, PH, aovs=ALL, moments=True)
    ctx.dispatch(at(good, 0), 2)
    before, st = read_planes(ctx), ctx.stats()
    ad, rp = ctx.adaptive_status().as_dict(), ctx.reproject_status().as_dict()
    xs, ys, fr = all_pixels(7, 5)
    assert err(ctx.dispatch, at(cam, 2), 1) == E_INVALID
    assert err(ctx.dispatch_adaptive, at(cam, 2), 1, threshold=1e-3) == E_INVALID
    assert err(ctx.reproject, cam, good) == E_INVALID and err(ctx.reproject, good, cam) == E_INVALID
    assert err(ctx.debug_raygen, cam, xs, ys, fr) == E_INVALID
    assert err(ctx.debug_center_rays, cam) == E_INVALID
    same_planes(read_planes(ctx), before)
    after = ctx.stats()
    assert (after.frames, after.paths, after.dispatches, after.segments) == (st.frames, st.paths, st.dispatches, st.segments)
    assert ctx.adaptive_status().as_dict() == ad
    assert ctx.reproject_status().as_dict() == rp
    # the same record is fine while the switch is off: the words are padding again
    ctx.set_projections(False)
    ctx.dispatch(at(cam, 2), 1)
    ctx.set_projections(True)
