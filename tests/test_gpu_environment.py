"""Environment lighting on the GPU (include/ptmi.h ptmi_upload_environment): nothing moves without a map, the lookup and
the sampling routine against the float64 model of tests/env_ref.py, the camera seeing the sky, next-event estimation against plain
BSDF sampling (two estimators of one integral), the light-selection probability, and every path through the dispatch."""
import functools

import numpy as np
import pytest

import env_ref
from ptmi import layout, native, scenes
from test_golden import load, same, HERE

pytestmark = pytest.mark.gpu

LUM = np.array((0.2126, 0.7152, 0.0722))
FW, FH = 64, 48


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the session's stays without an environment"""
    with native.Context(0) as c:
        yield c


def unique_map(W, H, seed=3):
    """every texel its own positive rgb (so that a lookup's radiance names its texel), float32"""
    rng = np.random.default_rng(seed)
    t = np.ones((H, W, 4), np.float32)
    t[..., :3] = rng.random((H, W, 3), np.float32) * 2.0 + 0.01
    return t


@functools.lru_cache(maxsize=None)
def cornell():
    return scenes.make("cornell")


def empty_scene():
    full = cornell()
    return scenes.Scene("empty", np.zeros(0, layout.TRIANGLE), full.mats, np.zeros(0, layout.BVH_NODE), np.zeros(0, layout.LIGHT), None)


def open_box():
    """feature_box-like geometry under the open sky: floor, back wall and one side wall of the Cornell shell, a glass and a metal box,
    a glossy and a diffuse sphere; no ceiling, nothing emissive, no light record"""
    S = scenes
    mats = [S._material(S._WHITE), S._material(S._RED), S._material(S._GREEN), S._material(S._WHITE),
            S._material((0.9, 1.0, 0.95), roughness=0.08, transmission=1.0, ior=1.45),
            S._material((0.9, 0.7, 0.3), metallic=1.0, roughness=0.25),
            S._material((0.6, 0.6, 0.9), metallic=0.4, roughness=0.35), S._material((0.7, 0.7, 0.7))]
    room = S._cornell_shell(0, 1, 2, 3)                       # floor, ceiling, back, +x, -x, light
    parts = [room[0], room[2], room[3],
             S._box((-0.45, 0.3, -0.1), (0.5, 0.6, 0.5), 4), S._box((0.5, 0.2, -0.2), (0.5, 0.4, 0.5), 5),
             S._uv_sphere((0.1, 0.3, 0.5), 0.3, 6, segments=12, rings=8), S._uv_sphere((-0.5, 0.85, -0.1), 0.22, 7, segments=10, rings=6)]
    sc = S._finish("open_box", parts, mats)
    assert len(sc.lights) == 0
    return sc


def setup(c, sc, W, H, moments=False, aovs=(), **opt):
    c.upload_scene(sc)
    c.set_aovs(*aovs)
    c.set_moments(moments)
    c.resize(W, H)
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, frames_per_batch=0, cull=1, traversal=0, overlap=2)
    o.update(opt)
    c.set_options(**o)


def at(cam, frame):
    cam = cam.copy()
    cam["frame_index"] = frame
    return cam


# ---- 1. nothing moves without it ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_64x48_4spp_mis", "cornell_64x64_4spp_b4_nomis"])
@pytest.mark.parametrize("how", ["uploaded_then_removed", "all_black_in_place"])
def test_goldens_keep_their_bits(ctx, name, how):
    z, sc, cam = load(HERE + "/golden/" + name + ".npz")
    setup(ctx, sc, int(cam["width"]), int(cam["height"]), max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
    if how == "uploaded_then_removed":
        ctx.upload_environment(scenes.sky(16, 8, "disc"))
        assert ctx.environment_status().sampled == 1
        ctx.upload_environment(None)
        assert ctx.environment_status().as_dict() == {"width": 0, "height": 0, "sampled": 0, "weight_sum": 0.0}
    else:                                                   # the ENV kernels with nothing to sample and nothing to add
        black = np.zeros((8, 16, 4), np.float32)
        ctx.upload_environment(black)
        st = ctx.environment_status()
        assert (st.width, st.height, st.sampled, st.weight_sum) == (16, 8, 0, 0.0)
    try:
        ctx.reset_stats()
        ctx.dispatch(cam, int(z["frames"]))
        out, st = ctx.read_output(), ctx.stats()
    finally:
        ctx.upload_environment(None)
    assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"])
    assert same(out, z["image"])


def test_errors_leave_the_environment_in_place(ctx):
    setup(ctx, empty_scene(), 8, 8)
    with pytest.raises(native.PtmiError) as e:
        ctx.set_environment(intensity=2.0)
    assert e.value.code == -4                               # none in place
    t = unique_map(16, 8)
    ctx.upload_environment(t, intensity=0.5)
    bad = t.copy()
    bad[3, 3, 0] = np.nan
    for call in (lambda: ctx.upload_environment(bad), lambda: ctx.upload_environment(t, intensity=-1.0),
                 lambda: ctx.upload_environment(t, rotation=np.inf), lambda: ctx.upload_environment(t, sample=2),
                 lambda: ctx.upload_environment(t, reserved=(0, 0, 1, 0, 0)), lambda: ctx.set_environment(intensity=np.nan)):
        with pytest.raises(native.PtmiError) as e:
            call()
        assert e.value.code == -1
    st = ctx.environment_status()
    assert (st.width, st.height, st.sampled) == (16, 8, 1)
    d = env_ref.texel_centres(16, 8)
    assert np.array_equal(ctx.debug_env_lookup(d)[:, :3], t.reshape(-1, 4)[:, :3] * np.float32(0.5))
    ctx.set_environment(intensity=0.5, sample=1)
    assert ctx.environment_status().sampled == 0
    with pytest.raises(native.PtmiError):
        ctx.debug_env_sample(np.zeros((1, 4), np.float32))
    ctx.upload_environment(None)


# ---- 2. lookup --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(16, 8), (64, 32)])
@pytest.mark.parametrize("rotation", [0.0, 1.0, -2.5])
def test_lookup_at_every_texel_centre(ctx, W, H, rotation):
    t = unique_map(W, H)
    ctx.upload_environment(t, intensity=0.75, rotation=rotation)
    d = env_ref.texel_centres(W, H, rotation)
    got = ctx.debug_env_lookup(d)
    ctx.upload_environment(None)
    idx, le, pdf, _, _ = env_ref.lookup(t, d, 0.75, rotation)
    assert np.array_equal(idx, np.arange(W * H))              # the model finds every centre in its own texel
    assert same(got[:, :3], le)                               # texel x intensity, one float32 multiply
    rel = np.abs(got[:, 3].astype(np.float64) - pdf) / pdf
    print("lookup %dx%d rot %g: worst relative pdf error %.3g (pole rows %.3g)" % (W, H, rotation, rel.max(), rel.reshape(H, W)[[0, -1]].max()))
    assert rel.max() <= 1e-5


# ---- 3. sampling -------------------------------------------------------------------------------------------------------------
def uniforms(n, seed):
    r = np.random.default_rng(seed).random((n, 4), np.float32)
    hi = np.float32(1.0 - 2.0 ** -24)
    corners = np.array([[a, b, c, d] for a in (0, hi) for b in (0, hi) for c in (0, hi) for d in (0, hi)], np.float32)
    return np.concatenate([r, corners])


@pytest.mark.parametrize("W,H,rotation", [(16, 8, 0.0), (64, 32, 1.0), (64, 32, -2.5)])
def test_sampling_routine_against_the_model(ctx, W, H, rotation):
    t = scenes.sky(W, H, "disc") * np.float32(0.25) + unique_map(W, H) * np.float32(0.01)
    t[H // 2, :, :3] = 0.0                                    # a row that must never be picked
    r = uniforms(4096, 11)
    ctx.upload_environment(t, rotation=rotation)
    d, out, tex = ctx.debug_env_sample(r)
    _, prob, alias, _ = native.env_table(t)
    mt, md, mpdf = env_ref.sample(t, prob, alias, r, rotation)
    assert np.array_equal(tex, mt)
    assert not np.isin(tex, np.arange(W) + (H // 2) * W).any()
    err = np.abs(d.astype(np.float64) - md).max()
    print("sample %dx%d rot %g: worst direction error %.3g" % (W, H, rotation, err))
    assert err <= 2e-6
    assert same(out[:, :3], t.reshape(-1, 4)[tex, :3])        # the texel's radiance (intensity 1)
    # density: c_t / max(sin theta, eps). The kernel's sin theta is within 1e-6 of the model's (v and v pi each round once in
    # float32, 2e-7 at theta near pi; the polynomial and its pi add as much), the division and c_t round once more
    sin_t = np.sin((tex // W + r[:, 3].astype(np.float64)) / H * np.pi)
    ok = sin_t > 1e-3
    assert np.all(np.abs(out[ok, 3] - mpdf[ok]) <= (1e-6 + 1e-6 / sin_t[ok]) * mpdf[ok])
    # the direction sampled at the texel's centre looks up the same texel and the same density
    rc = r.copy()
    rc[:, 2:] = 0.5
    dc, outc, texc = ctx.debug_env_sample(rc)
    back = ctx.debug_env_lookup(dc)
    ctx.upload_environment(None)
    assert np.array_equal(texc, tex)
    assert same(back[:, :3], outc[:, :3]) and same(back[:, :3], t.reshape(-1, 4)[tex, :3])
    assert np.all(np.abs(back[:, 3].astype(np.float64) - outc[:, 3]) <= 1e-5 * outc[:, 3])


def test_share_of_samples_in_the_bright_texel(ctx):
    W, H = 16, 8
    t = np.ones((H, W, 4), np.float32)
    t[..., :3] = 0.01
    t[H // 3, (2 * W) // 3, :3] = (9.0, 8.0, 7.0)
    bright = (H // 3) * W + (2 * W) // 3
    P = env_ref.weights(t)[1].reshape(-1)[bright]
    n = 1 << 18
    r = np.random.default_rng(2024).random((n, 4), np.float32)
    ctx.upload_environment(t)
    tex = ctx.debug_env_sample(r)[2]
    ctx.upload_environment(None)
    share = float((tex == bright).mean())
    print("bright texel: P %.6f, share %.6f, standard error %.2g" % (P, share, np.sqrt(P * (1 - P) / n)))
    assert 0.05 < P < 0.95
    assert abs(share - P) <= 4.0 * np.sqrt(P * (1.0 - P) / n)


# ---- 4. the camera sees the sky --------------------------------------------------------------------------------------------------
def test_camera_sees_the_sky(ctx):
    t = scenes.sky(64, 32, "disc")
    # the map's disc stands at azimuth 40 + 40.1 (the rotation), 35 degrees up: a camera that looks that way, a little lower, has
    # the disc, the horizon and a stretch of the gradient in view
    f = np.array((0.15, 0.45, 0.85)) / np.linalg.norm((0.15, 0.45, 0.85))
    right = np.cross(f, (0.0, 1.0, 0.0)) / np.linalg.norm(np.cross(f, (0.0, 1.0, 0.0)))
    cam = layout.make_camera(FW, FH, position=(0.0, 1.0, 2.8), forward=tuple(f), right=tuple(right), up=tuple(np.cross(right, f)),
                             aperture=0.0)
    setup(ctx, empty_scene(), FW, FH, aovs=("albedo", "normal", "id"))
    ctx.upload_environment(t, intensity=0.5, rotation=0.7)
    ctx.dispatch(cam, 1)
    got = ctx.read_output()
    ids, alb = ctx.read_aov("id"), ctx.read_aov("albedo")
    ys, xs = np.divmod(np.arange(FW * FH), FW)
    _, d, _ = ctx.debug_raygen(cam, xs, ys, np.zeros(FW * FH))
    _, le, _, uW, vH = env_ref.lookup(t, d, 0.5, 0.7)
    near = (np.abs(uW - np.round(uW)) < env_ref.BORDER_BAND) | (np.abs(vH - np.round(vH)) < env_ref.BORDER_BAND)
    assert near.mean() <= 0.01
    want = np.minimum(le, np.float32(2.5))                    # the fold's clamp of a sample (pt.wgsl:752): the disc is brighter
    assert same(got.reshape(-1, 4)[~near, :3], want[~near])
    assert (le.max(axis=1) > 2.5).any() and len(np.unique(le, axis=0)) > 8     # the disc and several rows of the gradient are in view
    assert np.all(ids == 0xFFFFFFFF) and not alb.any()       # the first-hit planes of a miss stay as they are
    # a constant map over 16 frames: the fold of equal values only rounds
    ctx.set_aovs()
    ctx.upload_environment(scenes.sky(16, 8, "constant"))
    ctx.dispatch(cam, 16)
    got = ctx.read_output()[..., :3]
    ctx.upload_environment(None)
    want = np.float32((0.3, 0.2, 0.1))
    assert np.all(np.abs(got - want) <= 2 * np.spacing(want))


# ---- 5. / 6. two estimators of one integral -----------------------------------------------------------------------------------------
BW = 64
BOX_CAM = dict(position=(0.0, 1.0, 2.8), forward=(0.0, 0.0, -1.0))


def box_sky():
    t = scenes.sky(64, 32, "disc")
    t[..., :3] *= np.float32(0.4) / t[..., :3].max()
    return t


def clamp_never_engaged(c, cam):
    worst = 0.0
    for f in range(8):
        c.write_output(np.zeros((BW, BW, 4), np.float32))
        c.dispatch(at(cam, f), 1)
        worst = max(worst, (f + 1) * float(c.read_output()[..., :3].max()))
    return worst


def render_with_moments(c, cam, frames=256):
    c.write_output(np.zeros((BW, BW, 4), np.float32))
    c.dispatch(at(cam, 0), frames)
    return c.read_output(), c.read_moments()


def assert_same_mean(a, b, frames, what):
    """a, b: (output, moments). Tile and image means of the luminance within 4 combined standard errors."""
    def stats(om):
        mom = om[1].astype(np.float64)
        assert np.all(mom[..., 2] == frames)
        return mom[..., 0], np.maximum(mom[..., 1] - mom[..., 0] ** 2, 0.0) / frames       # per pixel: mean, variance of the mean
    (ma, va), (mb, vb) = stats(a), stats(b)
    tiles = lambda x: x.reshape(BW // 16, 16, BW // 16, 16).sum(axis=(1, 3))
    diff, se = np.abs(tiles(ma) - tiles(mb)) / 256, np.sqrt(tiles(va) + tiles(vb)) / 256
    print(what, "tile means |diff| / se:", np.round(diff / se, 2).tolist())
    assert np.all(se > 0) and np.all(diff <= 4.0 * se), what
    d_img, se_img = abs(ma.mean() - mb.mean()), np.sqrt(va.sum() + vb.sum()) / ma.size
    print(what, "image means %.6f %.6f, |diff| / se %.2f" % (ma.mean(), mb.mean(), d_img / se_img))
    assert d_img <= 4.0 * se_img, what


@pytest.fixture(scope="module")
def box_renders(ctx):
    """the open box under the sky with do_mis = 0 (the bounce loop plus the lookup) and do_mis = 1 (the sky also sampled), rendered once"""
    sc, cam, t = open_box(), layout.make_camera(BW, BW, **BOX_CAM), box_sky()
    out = {"scene": sc, "cam": cam, "sky": t}
    setup(ctx, sc, BW, BW, moments=True, max_bounces=6, do_mis=0)
    ctx.upload_environment(t)
    out["clamp0"] = clamp_never_engaged(ctx, cam)
    out["mis0"] = render_with_moments(ctx, cam)
    ctx.set_options(do_mis=1)
    out["clamp1"] = clamp_never_engaged(ctx, cam)
    out["mis1"] = render_with_moments(ctx, cam)
    out["nee_rays"] = ctx.stats().shadow_rays
    ctx.set_environment(sample=1)
    out["lookup_only"] = render_with_moments(ctx, cam)
    ctx.upload_environment(None)
    ctx.set_moments(False)
    return out


def test_mis_agrees_with_bsdf_sampling(box_renders):
    b = box_renders
    print("largest sample of frames 0..7: do_mis 0 %.4f, do_mis 1 %.4f" % (b["clamp0"], b["clamp1"]))
    assert b["clamp0"] < 2.5 and b["clamp1"] < 2.5            # the 2.5 clamp never engaged: the two means are of the same integrand
    assert b["nee_rays"] > 0 and not same(b["mis0"][0], b["mis1"][0])      # next-event estimation did run
    assert_same_mean(b["mis1"], b["mis0"], 256, "do_mis 1 against do_mis 0:")


def test_lookup_only_runs_no_next_event_estimation(box_renders):
    b = box_renders
    assert same(b["lookup_only"][0], b["mis0"][0]) and same(b["lookup_only"][1], b["mis0"][1])


def test_selection_probability_with_a_second_light(ctx, box_renders):
    """one point light of intensity 0 beside the sky: every sky sample now carries 1 / 2"""
    b = box_renders
    sc = b["scene"]
    lights = np.zeros(1, layout.LIGHT)
    lights[0]["position"], lights[0]["light_type"], lights[0]["color"], lights[0]["intensity"] = (0.0, 1.5, 0.5), layout.LIGHT_POINT, (1, 1, 1), 0.0
    sc2 = scenes.Scene("open_box_dark_light", sc.tris, sc.mats, sc.nodes, lights, None)
    setup(ctx, sc2, BW, BW, moments=True, max_bounces=6, do_mis=1)
    ctx.upload_environment(b["sky"])
    worst = clamp_never_engaged(ctx, b["cam"])
    got = render_with_moments(ctx, b["cam"])
    ctx.upload_environment(None)
    ctx.set_moments(False)
    assert worst < 2.5
    assert_same_mean(got, b["mis0"], 256, "sky + dark point light against do_mis 0:")


# ---- 7. every path through the dispatch ----------------------------------------------------------------------------------------------
def cornell_under_sky(c, frames=5, aovs=(), moments=False, sample=0, **opt):
    setup(c, cornell(), FW, FH, aovs=aovs, moments=moments, **opt)
    c.upload_environment(scenes.sky(64, 32, "disc"), intensity=0.05, rotation=0.7, sample=sample)
    c.dispatch(layout.make_camera(FW, FH), frames)
    out = c.read_output()
    c.upload_environment(None)
    return out


@pytest.mark.parametrize("sample", [0, 1])
def test_dispatch_paths_agree(ctx, sample):
    base = cornell_under_sky(ctx, sample=sample, overlap=1, frames_per_batch=1)
    assert base[..., :3].max() > 0
    assert same(base, cornell_under_sky(ctx, sample=sample, overlap=0, frames_per_batch=1))
    assert same(base, cornell_under_sky(ctx, sample=sample, overlap=1, frames_per_batch=3))
    assert same(base, cornell_under_sky(ctx, sample=sample, overlap=0, frames_per_batch=3, aovs=("albedo", "normal", "id")))
    assert same(base, cornell_under_sky(ctx, sample=sample, overlap=1, frames_per_batch=0, aovs=("normal",)))
    ctx.set_aovs()


def test_adaptive_with_every_pixel_active_equals_plain_dispatch(ctx):
    cam = layout.make_camera(FW, FH)
    setup(ctx, cornell(), FW, FH, moments=True)
    ctx.upload_environment(scenes.sky(64, 32, "disc"), intensity=0.05, rotation=0.7)
    ctx.dispatch(at(cam, 0), 8)
    want = ctx.read_output(), ctx.read_moments()
    ctx.dispatch_adaptive(at(cam, 0), 2, threshold=1e-9, neighbourhood=0, min_frames=8, max_frames=64, step=4)
    got = ctx.read_output(), ctx.read_moments()
    ctx.upload_environment(None)
    ctx.set_moments(False)
    assert same(got[0], want[0]) and same(got[1], want[1])


def test_two_loopback_contexts_equal_one(ctx):
    want = cornell_under_sky(ctx, frames=3)
    with native.MultiContext([0, 0], loopback=True) as m:
        m.upload_scene(cornell())
        m.resize(FW, FH)
        m.set_options(max_bounces=8, do_mis=1)
        m.upload_environment(scenes.sky(64, 32, "disc"), intensity=0.05, rotation=0.7)
        m.dispatch(layout.make_camera(FW, FH), 3)
        got = m.read_output()
        with pytest.raises(native.PtmiError):
            m.upload_environment(np.full((8, 16, 4), -1.0, np.float32))
        m.set_environment(intensity=0.05, rotation=0.7, sample=1)
    assert same(got, want)


def test_one_bounce_shows_the_sky_only_where_the_camera_ray_misses(ctx):
    """The sky itself is seen by the rays that miss. Looked up only (sample = 1), a pixel whose camera ray hits keeps the bits it has
    without a map; sampled, such a pixel also receives the sky through its next-event sample, and the misses read the same texels."""
    t, cam = scenes.sky(64, 32, "disc"), layout.make_camera(FW, FH)
    sc = cornell()
    setup(ctx, sc, FW, FH, max_bounces=1)
    ctx.dispatch(cam, 1)
    dark = ctx.read_output()
    ctx.upload_environment(t, intensity=0.05, rotation=0.7, sample=1)
    ctx.dispatch(cam, 1)
    lit = ctx.read_output()
    ctx.set_environment(intensity=0.05, rotation=0.7, sample=0)
    ctx.dispatch(cam, 1)
    sampled = ctx.read_output()
    ctx.upload_environment(None)
    ys, xs = np.divmod(np.arange(FW * FH), FW)
    o, d, _ = ctx.debug_raygen(cam, xs, ys, np.zeros(FW * FH))
    miss = ctx.debug_intersect(o, d)[1] == 0xFFFFFFFF
    assert 0 < miss.sum() < miss.size
    lit, dark, sampled = lit.reshape(-1, 4), dark.reshape(-1, 4), sampled.reshape(-1, 4)
    assert same(lit[~miss], dark[~miss]) and not dark[miss, :3].any()
    assert same(sampled[miss], lit[miss]) and not same(sampled[~miss], dark[~miss])
    _, le, _, uW, vH = env_ref.lookup(t, d, 0.05, 0.7)
    near = (np.abs(uW - np.round(uW)) < env_ref.BORDER_BAND) | (np.abs(vH - np.round(vH)) < env_ref.BORDER_BAND)
    keep = miss & ~near
    assert same(lit[keep, :3], np.minimum(le[keep], np.float32(2.5)))
