"""The participating medium on the GPU (include/ptmi.h ptmi_set_medium): the two probes against the float64 model of
tests/medium_ref.py, nothing moving without a medium, errors, Beer-Lambert attenuation, the white furnace with and without next-event
estimation, two estimators of one integral, single scattering of a point light against a quadrature, every path through the dispatch,
and the perf-mode build."""
import functools

import numpy as np
import pytest

import medium_ref
from ptmi import layout, native, scenes
from test_golden import load, same, HERE
from test_gpu_environment import (BOX_CAM, BW, assert_same_mean, at, box_sky, clamp_never_engaged, empty_scene, open_box,
                                  render_with_moments, setup)

pytestmark = pytest.mark.gpu

LUM = np.float32((0.2126, 0.7152, 0.0722)).astype(np.float64)
FW, FH = 64, 48
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the session's stays without a medium"""
    with native.Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def cornell():
    return scenes.make("cornell")


def scene_box(sc):
    v = np.concatenate([sc.tris[k][:, :3] for k in ("v0", "v1", "v2")]).astype(np.float64)
    return tuple(np.float32(v.min(axis=0))), tuple(np.float32(v.max(axis=0)))


# ---- 1. the probes against the model ----------------------------------------------------------------------------------------------
from medium_ref import (BOXES, TOL_DIR, TOL_GEOM, TOL_PDF, deviation, probe_inputs, step_deviations, tr_inputs)  # noqa: E402


@pytest.mark.parametrize("g", [0.0, 0.6, -0.8])
@pytest.mark.parametrize("box_index", [0, 1])
def test_probes_against_the_model(ctx, box_index, g):
    setup(ctx, empty_scene(), 8, 8)
    with pytest.raises(native.PtmiError) as e:
        ctx.debug_medium_step(np.zeros((1, 3)), np.float32([[0, 0, 1]]), [INF], np.zeros((1, 3)))
    assert e.value.code == -4                                               # none in place
    with pytest.raises(native.PtmiError) as e:
        ctx.debug_medium_tr(np.zeros((1, 3)), np.float32([[0, 0, 1]]), [1.0])
    assert e.value.code == -4
    m = medium_ref.Medium(1.3, 0.8, g, *BOXES[box_index])
    o, d, t_hit, r = probe_inputs(box_index)
    ctx.set_medium(**m.kwargs())
    try:
        sc, x, direc, out = ctx.debug_medium_step(o, d, t_hit, r)
        o2, wi, dist = tr_inputs(box_index)
        tr = ctx.debug_medium_tr(o2, wi, dist)
    finally:
        ctx.set_medium(None)
    m64 = medium_ref.step(m, o, d, t_hit, r)
    got = dict(scattered=sc, x=x, dir=direc, a=out[:, 0], b=out[:, 1], s=out[:, 2], pdf=out[:, 3])
    geom, dev_dir, pdf, aside = step_deviations(got, m64)
    dev_tr = deviation(tr, medium_ref.transmittance(m, o2, wi, dist))
    print("box %d g %g: a, b, s, x %.3g, Tr %.3g (limit %.3g); direction %.3g (limit %.3g); density %.3g (limit %.3g); %.2f %% of decisions set aside"
          % (box_index, g, geom, dev_tr, TOL_GEOM, dev_dir, TOL_DIR, pdf, TOL_PDF, 100 * aside))
    assert aside <= 0.01
    assert not out[~(m64["b"] > m64["a"]), 2].any() and not x[~sc].any() and not direc[~sc].any() and not out[~sc, 3].any()
    assert geom <= TOL_GEOM and dev_tr <= TOL_GEOM and dev_dir <= TOL_DIR and pdf <= TOL_PDF


# ---- 2. nothing moves without it ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_64x48_4spp_mis", "cornell_64x64_4spp_b4_nomis", "random_soup3_48x48_3spp"])
@pytest.mark.parametrize("how", ["set_then_removed", "flat_box_in_place"])
def test_goldens_keep_their_bits(ctx, name, how):
    """(the soup's degenerate triangles make rays whose origin and direction are NaN: no box gives such a ray an interval)"""
    z, sc, cam = load(HERE + "/golden/" + name + ".npz")
    setup(ctx, sc, int(cam["width"]), int(cam["height"]), max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
    if how == "set_then_removed":
        ctx.set_medium(sigma_t=0.7, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
        assert ctx.get_medium() is not None
        ctx.set_medium(None)
        assert ctx.get_medium() is None
    else:                                                   # the MED kernels with no segment that has an interval
        ctx.set_medium(sigma_t=50.0, albedo=0.9, g=0.3, box=((-5.0, 0.3712, -5.0), (5.0, 0.3712, 5.0)))
        assert ctx.get_medium().as_dict()["box"][0][1] == ctx.get_medium().as_dict()["box"][1][1]
    try:
        ctx.reset_stats()
        ctx.dispatch(cam, int(z["frames"]))
        out, st = ctx.read_output(), ctx.stats()
    finally:
        ctx.set_medium(None)
    assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"])
    assert same(out, z["image"])


def test_errors_keep_the_medium(ctx):
    sc = cornell()
    setup(ctx, sc, FW, FH)
    box = scene_box(sc)
    good = dict(sigma_t=0.6, albedo=(0.9, 0.8, 0.7), g=0.4, box=box)
    ctx.set_medium(**good)
    cam = layout.make_camera(FW, FH)
    ctx.dispatch(cam, 2)
    before, was = ctx.read_output(), ctx.get_medium().as_dict()
    lo, hi = box
    bad = [dict(sigma_t=0.0), dict(sigma_t=-1.0), dict(sigma_t=np.inf), dict(sigma_t=np.nan), dict(albedo=(0.5, 1.5, 0.5)),
           dict(albedo=(-0.1, 0.5, 0.5)), dict(albedo=(0.5, 0.5, np.nan)), dict(g=0.995), dict(g=-1.0), dict(g=np.nan),
           dict(box=((lo[0], hi[1] + 1.0, lo[2]), hi)), dict(box=(lo, (np.inf, hi[1], hi[2]))), dict(box=((np.nan, lo[1], lo[2]), hi)),
           dict(reserved=(0, 0, 0, 0, 1))]
    for kw in bad:
        with pytest.raises(native.PtmiError) as e:
            ctx.set_medium(**dict(good, **kw))
        assert e.value.code == -1, kw
    try:
        assert ctx.get_medium().as_dict() == was
        assert was["sigma_t"] == float(np.float32(0.6)) and was["box"] == (tuple(map(float, lo)), tuple(map(float, hi)))
        ctx.dispatch(cam, 2)
        assert same(ctx.read_output(), before)
    finally:
        ctx.set_medium(None)
    ctx.dispatch(cam, 2)
    assert not same(ctx.read_output(), before)              # and the medium did shape that render


# ---- 3. Beer-Lambert ----------------------------------------------------------------------------------------------------------------------
def uniform_sky(radiance=0.5):
    t = np.ones((8, 16, 4), np.float32)
    t[..., :3] = radiance
    return t


def tile_stats(mom, frames, tile=16):
    """the moments plane as (per-pixel mean luminance, variance of that mean), and a function summing square tiles"""
    mom = mom.astype(np.float64)
    assert np.all(mom[..., 2] == frames)
    H, W = mom.shape[:2]
    return mom[..., 0], np.maximum(mom[..., 1] - mom[..., 0] ** 2, 0.0) / frames, lambda x: x.reshape(H // tile, tile, W // tile, tile).sum(axis=(1, 3))


def assert_means(mean, var, tiles, want, what):
    """tile and image means of `mean` within 4 standard errors of those of `want` (per pixel)"""
    per = mean.size // tiles(mean).size
    diff, se = np.abs(tiles(mean) - tiles(want)) / per, np.sqrt(tiles(var)) / per
    print(what, "tile means |diff| / se:", np.round(diff / se, 2).tolist())
    assert np.all(se > 0) and np.all(diff <= 4.0 * se), what
    d_img, se_img = abs(mean.mean() - want.mean()), np.sqrt(var.sum()) / mean.size
    print(what, "image means %.6f %.6f, |diff| / se %.2f" % (mean.mean(), want.mean(), d_img / se_img))
    assert d_img <= 4.0 * se_img, what


@pytest.mark.parametrize("depth", [0.5, 2.0])
def test_beer_lambert(ctx, depth):
    """an absorbing slab (albedo 0) between the camera and a uniform sky: every sample is 0.5 with the probability exp(-sigma_t l) of
    its own ray, l the length that ray spends in the slab"""
    W = H = 32
    frames, thickness = 64, 0.8
    m = medium_ref.Medium(depth / thickness, 0.0, 0.0, (-50.0, -50.0, 0.5), (50.0, 50.0, 0.5 + thickness))
    cam = layout.make_camera(W, H)
    setup(ctx, empty_scene(), W, H, moments=True, max_bounces=2)
    ctx.upload_environment(uniform_sky(0.5), sample=1)
    ctx.set_medium(**m.kwargs())
    try:
        ctx.write_output(np.zeros((H, W, 4), np.float32))
        ctx.dispatch(at(cam, 0), frames)
        mom = ctx.read_moments()
        f, ys, xs = np.meshgrid(np.arange(frames), np.arange(H), np.arange(W), indexing="ij")
        o, d, _ = ctx.debug_raygen(cam, xs.ravel(), ys.ravel(), f.ravel())
    finally:
        ctx.set_medium(None)
        ctx.upload_environment(None)
        ctx.set_moments(False)
    _, _, a, b = medium_ref.interval(m, o, d, np.full(len(o), INF))
    assert np.all(b > a)                                    # the slab covers the view
    length = b - a
    want = (0.5 * LUM.sum() * np.exp(-m.sigma_t * length)).reshape(frames, H, W).mean(axis=0)
    mean, var, tiles = tile_stats(mom, frames)
    print("optical depth %.2f: path lengths %.3f .. %.3f" % (depth, length.min(), length.max()))
    assert_means(mean, var, tiles, want, "Beer-Lambert, depth %g:" % depth)


# ---- 4. the white furnace -----------------------------------------------------------------------------------------------------------------
def furnace_medium(cam):
    p = np.asarray(cam["position"], np.float64)
    return medium_ref.Medium(1.0, 1.0, 0.6, tuple(p - 0.5), tuple(p + 0.5))          # optical half-width 0.5 around the camera


def test_furnace_without_next_event_estimation_is_exact(ctx):
    """albedo 1 inside a uniform sky: the throughput stays 1, roulette (rng > 1) never fires, and whatever the path does it ends in a
    miss that adds the sky's radiance; a path of 64 scatters at this thickness has negligible probability"""
    cam = layout.make_camera(BW, BW)
    setup(ctx, empty_scene(), BW, BW, do_mis=0, max_bounces=64)
    ctx.upload_environment(uniform_sky(0.5), sample=1)
    ctx.set_medium(**furnace_medium(cam).kwargs())
    try:
        ctx.reset_stats()
        ctx.dispatch(at(cam, 0), 1)
        out, st = ctx.read_output(), ctx.stats()
    finally:
        ctx.set_medium(None)
        ctx.upload_environment(None)
    assert st.segments > 1.2 * BW * BW                      # paths did scatter
    assert np.all(out[..., :3] == np.float32(0.5))


def test_furnace_with_mis(ctx):
    """the same with the sky sampled: next-event samples from scatter points and the weighted misses add up to the sky's radiance only
    if the phase value next-event estimation uses is the density the directions are drawn from"""
    frames = 256
    cam = layout.make_camera(BW, BW)
    setup(ctx, empty_scene(), BW, BW, moments=True, do_mis=1, max_bounces=64)
    ctx.upload_environment(uniform_sky(0.5))
    ctx.set_medium(**furnace_medium(cam).kwargs())
    try:
        assert ctx.environment_status().sampled == 1
        worst = clamp_never_engaged(ctx, cam)
        ctx.reset_stats()
        _, mom = render_with_moments(ctx, cam, frames)
        rays = ctx.stats().shadow_rays
    finally:
        ctx.set_medium(None)
        ctx.upload_environment(None)
        ctx.set_moments(False)
    print("largest sample of frames 0..7: %.4f" % worst)
    assert worst < 2.5 and rays > 0
    mean, var, tiles = tile_stats(mom, frames)
    assert_means(mean, var, tiles, np.full(mean.shape, 0.5 * LUM.sum()), "furnace with MIS:")


# ---- 5. two estimators of one integral -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fog_box_renders(ctx):
    """the environment suite's open box under its disc sky, in a fog of optical thickness about 1 across the scene, albedo 0.8: with
    do_mis = 0, do_mis = 1, and do_mis = 1 through the perf-mode build; rendered once"""
    sc, cam, t = open_box(), layout.make_camera(BW, BW, **BOX_CAM), box_sky()
    lo, hi = scene_box(sc)
    fog = dict(sigma_t=float(1.0 / (np.asarray(hi, np.float64) - lo).max()), albedo=0.8, g=0.3, box=(lo, hi))
    out = {}
    setup(ctx, sc, BW, BW, moments=True, max_bounces=6, do_mis=0)
    ctx.upload_environment(t)
    ctx.set_medium(**fog)
    try:
        out["clamp0"] = clamp_never_engaged(ctx, cam)
        out["mis0"] = render_with_moments(ctx, cam)
        ctx.set_options(do_mis=1)
        out["clamp1"] = clamp_never_engaged(ctx, cam)
        ctx.reset_stats()
        out["mis1"] = render_with_moments(ctx, cam)
        out["stats1"] = ctx.stats()
        ctx.set_options(perf_mode=1)
        ctx.reset_stats()
        out["fast"] = render_with_moments(ctx, cam)
        out["stats_fast"] = ctx.stats()
        ctx.set_medium(None)
        ctx.set_options(perf_mode=0)
        out["clear"] = render_with_moments(ctx, cam)
    finally:
        ctx.set_options(perf_mode=0)
        ctx.set_medium(None)
        ctx.upload_environment(None)
        ctx.set_moments(False)
    return out


def test_mis_agrees_with_phase_and_bsdf_sampling(fog_box_renders):
    """covers Tr on surface samples, samples from scatter points, and W"""
    b = fog_box_renders
    print("largest sample of frames 0..7: do_mis 0 %.4f, do_mis 1 %.4f" % (b["clamp0"], b["clamp1"]))
    assert b["clamp0"] < 2.5 and b["clamp1"] < 2.5
    assert b["stats1"].shadow_rays > 0 and not same(b["mis0"][0], b["mis1"][0]) and not same(b["mis1"][0], b["clear"][0])
    assert_same_mean(b["mis1"], b["mis0"], 256, "fog, do_mis 1 against do_mis 0:")


def test_perf_mode_agrees_statistically(fog_box_renders):
    """the criterion of test_gpu_perf_mode.py: the same RNG streams, every 16x16 tile within 3 standard errors of the contract
    build's Monte-Carlo mean, image means within 5e-3, counters within 1e-3"""
    b = fog_box_renders
    st0, st1 = b["stats1"], b["stats_fast"]
    assert st1.paths == st0.paths and abs(st1.segments / st0.segments - 1) < 1e-3 and abs(st1.shadow_rays / st0.shadow_rays - 1) < 1e-3
    exact, fast = b["mis1"], b["fast"]
    assert np.isfinite(fast[0][..., :3]).all()
    mean, var, tiles = tile_stats(exact[1], 256)
    fmean = fast[1].astype(np.float64)[..., 0]
    ratio = (np.abs(tiles(fmean) - tiles(mean)) / 256) / (np.sqrt(tiles(var)) / 256 + 1e-7)
    rel = fast[0][..., :3].mean() / exact[0][..., :3].mean() - 1.0
    print("perf mode in fog: worst tile %.2f standard errors, image mean %+.2e" % (ratio.max(), rel))
    assert ratio.max() <= 3.0 and abs(rel) <= 5e-3


# ---- 6. single scattering of a point light ---------------------------------------------------------------------------------------------------
def test_single_scattering_of_a_point_light(ctx):
    """max_bounces = 1 in an empty scene: the only light a pixel receives is the next-event sample of the camera ray's scatter point.
    Its expectation along the pixel's centre ray is the integral over the distance t from the box's entry of
    sigma_t exp(-sigma_t t) (the free flight's density) albedo Tr(x -> light) p I / dist^2 w_mis / pdf_light, with the reference's
    point-light pdf (1 / n_lights) 10000 and w_mis the power heuristic of that against p; a float64 midpoint rule of 4 096 steps."""
    W = H = 32
    frames = 256
    light_pos, intensity = np.array((0.3, 3.2, -0.2)), 6.0e4
    lights = np.zeros(1, layout.LIGHT)
    lights[0]["position"], lights[0]["light_type"], lights[0]["color"], lights[0]["intensity"] = tuple(light_pos), layout.LIGHT_POINT, (1, 1, 1), intensity
    e = empty_scene()
    sc = scenes.Scene("empty_with_point_light", e.tris, e.mats, e.nodes, lights, None)
    m = medium_ref.Medium(0.9, (0.9, 0.7, 0.5), 0.0, (-1.5, 0.0, -1.2), (1.5, 2.0, 1.0))
    cam = layout.make_camera(W, H, aperture=0.0)
    setup(ctx, sc, W, H, moments=True, max_bounces=1, do_mis=1)
    ctx.set_medium(**m.kwargs())
    try:
        worst = 0.0
        for f in range(4):
            ctx.write_output(np.zeros((H, W, 4), np.float32))
            ctx.dispatch(at(cam, f), 1)
            worst = max(worst, (f + 1) * float(ctx.read_output()[..., :3].max()))
        ctx.write_output(np.zeros((H, W, 4), np.float32))
        ctx.reset_stats()
        ctx.dispatch(at(cam, 0), frames)
        mom, st = ctx.read_moments(), ctx.stats()
        o, d = ctx.debug_center_rays(cam)
    finally:
        ctx.set_medium(None)
        ctx.set_moments(False)
    assert worst < 2.5 and st.shadow_rays > 0               # the fold's clamp did not engage
    _, _, a, b = medium_ref.interval(m, o, d, np.full(len(o), INF))
    inside = b > a
    steps = 4096
    want = np.zeros(len(o))
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    p = 1.0 / (4.0 * np.pi)
    pdf_l = 10000.0
    w_mis = pdf_l ** 2 / (pdf_l ** 2 + p ** 2)
    for k in np.flatnonzero(inside):
        t = a[k] + (np.arange(steps) + 0.5) * (b[k] - a[k]) / steps
        x = o64[k] + t[:, None] * d64[k]
        to_l = light_pos - x
        dist = np.linalg.norm(to_l, axis=1)
        assert dist.min() > 1.0 and dist.max() < 100.0
        tr = medium_ref.transmittance(m, x.astype(np.float32), (to_l / dist[:, None]).astype(np.float32), dist.astype(np.float32))
        f = m.sigma_t * np.exp(-m.sigma_t * (t - a[k])) * tr * p * intensity / dist ** 2 * w_mis / pdf_l
        want[k] = f.sum() * (b[k] - a[k]) / steps * float((m.albedo * LUM).sum())
    mean, var, tiles = tile_stats(mom, frames)
    assert 0.3 < inside.mean() and want.max() > 0.05
    assert_means(mean, var, tiles, want.reshape(H, W), "single scattering:")


# ---- 7. every path through the dispatch ------------------------------------------------------------------------------------------------------
def cornell_in_fog(c, frames=5, aovs=(), moments=False, fog=True, **opt):
    sc = cornell()
    setup(c, sc, FW, FH, aovs=aovs, moments=moments, **opt)
    if fog:
        c.set_medium(sigma_t=0.5, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
    try:
        c.dispatch(layout.make_camera(FW, FH), frames)
        out = c.read_output()
        planes = {a: c.read_aov(a) for a in aovs}
    finally:
        c.set_medium(None)
    return out, planes


def test_dispatch_paths_agree(ctx):
    base, _ = cornell_in_fog(ctx, overlap=1, frames_per_batch=1)
    clear, _ = cornell_in_fog(ctx, overlap=1, frames_per_batch=1, fog=False)
    assert base[..., :3].max() > 0 and not same(base, clear)
    assert same(base, cornell_in_fog(ctx, overlap=0, frames_per_batch=1)[0])
    assert same(base, cornell_in_fog(ctx, overlap=1, frames_per_batch=3)[0])
    assert same(base, cornell_in_fog(ctx, overlap=0, frames_per_batch=0)[0])
    all_planes = ("albedo", "normal", "id")
    with_planes, planes = cornell_in_fog(ctx, overlap=0, frames_per_batch=3, aovs=all_planes)
    assert same(base, with_planes)
    assert same(base, cornell_in_fog(ctx, overlap=1, frames_per_batch=0, aovs=("normal",))[0])
    # the planes record the camera ray's surface hit whether or not the path scattered in front of it
    _, clear_planes = cornell_in_fog(ctx, overlap=0, frames_per_batch=3, aovs=all_planes, fog=False)
    for a in all_planes:
        assert same(planes[a], clear_planes[a]), a
    ctx.set_aovs()


def test_adaptive_with_every_pixel_active_equals_plain_dispatch(ctx):
    sc, cam = cornell(), layout.make_camera(FW, FH)
    setup(ctx, sc, FW, FH, moments=True)
    ctx.set_medium(sigma_t=0.5, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
    try:
        ctx.dispatch(at(cam, 0), 8)
        want = ctx.read_output(), ctx.read_moments()
        ctx.dispatch_adaptive(at(cam, 0), 2, threshold=1e-9, neighbourhood=0, min_frames=8, max_frames=64, step=4)
        got = ctx.read_output(), ctx.read_moments()
    finally:
        ctx.set_medium(None)
        ctx.set_moments(False)
    assert same(got[0], want[0]) and same(got[1], want[1])


def test_two_loopback_contexts_equal_one(ctx):
    sc = cornell()
    want, _ = cornell_in_fog(ctx, frames=3)
    with native.MultiContext([0, 0], loopback=True) as m:
        m.upload_scene(sc)
        m.resize(FW, FH)
        m.set_options(max_bounces=8, do_mis=1)
        m.set_medium(sigma_t=0.5, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
        m.dispatch(layout.make_camera(FW, FH), 3)
        got = m.read_output()
        with pytest.raises(native.PtmiError) as e:
            m.set_medium(sigma_t=-1.0, box=scene_box(sc))
        assert e.value.code == -1
        m.set_medium(None)
    assert same(got, want)
