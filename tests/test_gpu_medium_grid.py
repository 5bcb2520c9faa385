"""The medium's density grid on the GPU (include/ptmi.h ptmi_upload_medium_density): the lookup and both trackers
against the models of tests/medium_grid_ref.py, a constant grid against the homogeneous medium in distribution, Beer-Lambert through a
slab whose far half is empty, the white furnace under a grid that varies, single scattering of a point light through two cells against
a quadrature, every path through the dispatch, nothing moving once the grid is gone, errors and the life cycle."""
import numpy as np
import pytest

import medium_grid_ref as R
import medium_ref
from ptmi import layout, native, scenes
from test_golden import load, same, HERE
from test_gpu_environment import (BOX_CAM, BW, assert_same_mean, at, box_sky, clamp_never_engaged, empty_scene, open_box,
                                  render_with_moments, setup)
from test_gpu_medium import FH, FW, INF, LUM, assert_means, cornell, furnace_medium, scene_box, tile_stats, uniform_sky

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the session's stays without a medium"""
    with native.Context(0) as c:
        yield c


# ---- 1. the probes against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("dims", R.GRID_DIMS)
def test_probes_against_the_model(ctx, dims, filt):
    setup(ctx, empty_scene(), 8, 8)
    m, g = R.probe_medium(), R.probe_grid(dims)
    ctx.set_medium(**m.kwargs())
    try:
        with pytest.raises(native.PtmiError) as e:
            ctx.debug_medium_density(np.zeros((1, 3)))
        assert e.value.code == -4                                           # no grid in place
        with pytest.raises(native.PtmiError) as e:
            ctx.debug_medium_track(np.zeros((1, 3)), np.float32([[0, 0, 1]]), [INF], [1], 0)
        assert e.value.code == -4
        ctx.upload_medium_density(g, filter=filt)
        p = R.lookup_points()
        rho = ctx.debug_medium_density(p)
        got = {mode: ctx.debug_medium_track(*R.probe_rays(mode), mode) for mode in (0, 1)}
    finally:
        ctx.set_medium(None)
    # the lookup: within four times the float32 model's deviation from the float64 model's (nearest: the same cell but on the points
    # where the two precisions find different ones), and, its arithmetic being under the contract, the float32 model's cell exactly
    r64, r32 = R.lookup(m, g, filt, p.astype(np.float64), np.float64), R.lookup(m, g, filt, p, np.float32)
    if filt == 0:
        agree = r64 == r32
        assert (~agree).mean() <= R.ASIDE_CAP
        assert np.array_equal(rho[agree], r64[agree].astype(np.float32)) and np.array_equal(rho, r32)
    else:
        tol = R.tolerance(R.deviation(r32, r64))
        dev = R.deviation(rho, r64)
        print("grid %s trilinear lookup: deviation %.3g (limit %.3g); %d of %d values are the float32 model's bits"
              % (dims, dev, tol, (rho.view(np.uint32) == r32.view(np.uint32)).sum(), len(p)))
        assert dev <= tol
    for mode in (0, 1):
        m64, m32, aside = R.models(dims, filt, mode)
        sc, t, v, steps, after = got[mode]
        keep = ~aside
        tol_t, tol_v = R.tolerance(R.deviation(m32["t"][keep], m64["t"][keep])), R.tolerance(R.deviation(m32["value"][keep], m64["value"][keep]))
        off = (steps != m64["steps"]) | (after != m64["rng"]) | (sc != m64["scattered"])
        dev_t, dev_v = R.deviation(t[keep & ~off], m64["t"][keep & ~off]), R.deviation(v[keep & ~off], m64["value"][keep & ~off])
        print("grid %s filter %d mode %d: %.3f %% set aside, %d other rays differ in steps, RNG state or outcome; t %.3g (limit %.3g), value %.3g (limit %.3g)"
              % (dims, filt, mode, 100 * aside.mean(), (off & keep).sum(), dev_t, tol_t, dev_v, tol_v))
        assert aside.mean() <= R.ASIDE_CAP
        assert np.array_equal(steps[keep], m64["steps"][keep]) and np.array_equal(after[keep], m64["rng"][keep])
        assert np.array_equal(sc[keep], m64["scattered"][keep])
        assert dev_t <= tol_t and dev_v <= tol_v
        assert steps.max() < R.TRACK_CAP // 100


# ---- 2. a constant grid is the homogeneous medium, in distribution ---------------------------------------------------------------------------
def image_means_within(a, b, frames, k, what):
    """the image means of the luminance of two (output, moments) pairs within k combined standard errors"""
    def stats(om):
        mom = om[1].astype(np.float64)
        return mom[..., 0], np.maximum(mom[..., 1] - mom[..., 0] ** 2, 0.0) / frames
    (ma, va), (mb, vb) = stats(a), stats(b)
    d, se = abs(ma.mean() - mb.mean()), np.sqrt(va.sum() + vb.sum()) / ma.size
    print(what, "image means |diff| / se %.2f" % (d / se))
    assert d <= k * se, what


def tile_means_within(a, b, frames, k, what, tile=16):
    """the mean luminance of every tile x tile block of two (output, moments) pairs within k combined standard errors"""
    (ma, va, tiles), (mb, vb, _) = tile_stats(a[1], frames, tile), tile_stats(b[1], frames, tile)
    diff, se = np.abs(tiles(ma) - tiles(mb)), np.sqrt(tiles(va) + tiles(vb))
    print(what, "tile means |diff| / se, held to %g:" % k, np.round(diff / se, 2).tolist())
    assert np.all(se > 0) and np.all(diff <= k * se), what


@pytest.fixture(scope="module")
def constant_grid_renders(ctx):
    """the fogged open box of test_gpu_medium.py's fog_box_renders, with do_mis 0 and 1: homogeneous, under constant grids that describe
    the same medium, without a medium, and under a grid of zeros; rendered once"""
    sc, cam, t = open_box(), layout.make_camera(BW, BW, **BOX_CAM), box_sky()
    lo, hi = scene_box(sc)
    sigma = float(1.0 / (np.asarray(hi, np.float64) - lo).max())
    fog = dict(sigma_t=sigma, albedo=0.8, g=0.3, box=(lo, hi))
    out = {}
    setup(ctx, sc, BW, BW, moments=True, max_bounces=6, do_mis=0)
    ctx.upload_environment(t)
    try:
        for mis in (0, 1):
            ctx.set_options(do_mis=mis)
            ctx.set_medium(None)
            out["clear", mis] = render_with_moments(ctx, cam)
            ctx.set_medium(**fog)
            out["homogeneous", mis] = render_with_moments(ctx, cam)
            ctx.upload_medium_density(np.ones((1, 1, 1), np.float32))
            out["clamp", mis] = clamp_never_engaged(ctx, cam)
            out["ones_1", mis] = render_with_moments(ctx, cam)
            ctx.upload_medium_density(np.ones((2, 5, 3), np.float32), filter=1)
            out["ones_352", mis] = render_with_moments(ctx, cam)
            ctx.upload_medium_density(np.zeros((2, 5, 3), np.float32))
            out["zeros", mis] = render_with_moments(ctx, cam)
            ctx.set_medium(**dict(fog, sigma_t=2.0 * sigma))                # keeps the grid
            ctx.upload_medium_density(np.full((2, 5, 3), 0.5, np.float32), filter=1)
            assert ctx.medium_grid_status().as_dict() == dict(dims=(3, 5, 2), filter=1, rho_min=0.5, rho_max=0.5, rho_mean=0.5)
            out["half", mis] = render_with_moments(ctx, cam)
    finally:
        ctx.set_medium(None)
        ctx.upload_environment(None)
        ctx.set_moments(False)
    return out


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("which,against", [("ones_1", "homogeneous"), ("ones_352", "homogeneous"), ("half", "homogeneous"), ("zeros", "clear")])
def test_constant_grid_equals_the_homogeneous_medium(constant_grid_renders, which, against, mis):
    """per 16 x 16 tile within 3 combined standard errors (assert_same_mean as it stands holds 4), and the image means within 3"""
    b = constant_grid_renders
    assert b["clamp", mis] < 2.5
    assert not same(b["homogeneous", mis][0], b["clear", mis][0])
    if which != "zeros":
        assert not same(b[which, mis][0], b[against, mis][0])               # another estimator: other draws, other bits
    what = "%s against %s, do_mis %d:" % (which, against, mis)
    assert_same_mean(b[which, mis], b[against, mis], 256, what)
    tile_means_within(b[which, mis], b[against, mis], 256, 3.0, what)
    image_means_within(b[which, mis], b[against, mis], 256, 3.0, what)


# ---- 3. Beer-Lambert through a split slab -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [0.5, 2.0])
def test_beer_lambert_through_a_split_slab(ctx, depth):
    """test_beer_lambert's absorbing slab between the camera and a uniform sky, its density (1, 0) along the view axis: every ray spends
    half of its length in each half, so a sample is 0.5 with probability exp(-sigma_t l / 2)"""
    W = H = 32
    frames, thickness = 64, 0.8
    # (the slab is 10 wide where test_beer_lambert's is 100: a grid's box has the optical-depth limit to meet, and the view fits)
    m = medium_ref.Medium(depth / thickness, 0.0, 0.0, (-5.0, -5.0, 0.5), (5.0, 5.0, 0.5 + thickness))
    cam = layout.make_camera(W, H)
    setup(ctx, empty_scene(), W, H, moments=True, max_bounces=2)
    ctx.upload_environment(uniform_sky(0.5), sample=1)
    ctx.set_medium(**m.kwargs())
    ctx.upload_medium_density(np.float32([1.0, 0.0]).reshape(2, 1, 1))
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
    assert np.all(b > a)
    assert np.allclose((b - a) * np.abs(d[:, 2].astype(np.float64)), thickness, rtol=1e-5)     # in through one z face, out through the other
    want = (0.5 * LUM.sum() * np.exp(-m.sigma_t * (b - a) / 2.0)).reshape(frames, H, W).mean(axis=0)
    mean, var, tiles = tile_stats(mom, frames)
    assert_means(mean, var, tiles, want, "Beer-Lambert through half a slab, depth %g:" % depth)
    full = (0.5 * LUM.sum() * np.exp(-m.sigma_t * (b - a))).reshape(frames, H, W).mean(axis=0)
    assert abs(mean.mean() - full.mean()) > 8.0 * np.sqrt(var.sum()) / mean.size       # and the whole slab is told apart


# ---- 4. the white furnace under a grid that varies ----------------------------------------------------------------------------------------
def furnace_grid():
    g = R.probe_grid((3, 5, 2)).copy()
    assert g.min() == 0.0 and g.max() == 1.0 and 0.2 < g.mean() < 0.8
    return g


def test_furnace_without_next_event_estimation_is_exact(ctx):
    """albedo 1 inside a uniform sky: whatever the density does, the throughput stays 1 and every path ends in a miss that adds the sky's
    radiance"""
    cam = layout.make_camera(BW, BW)
    setup(ctx, empty_scene(), BW, BW, do_mis=0, max_bounces=64)
    ctx.upload_environment(uniform_sky(0.5), sample=1)
    fm = furnace_medium(cam)
    ctx.set_medium(**dict(fm.kwargs(), sigma_t=3.0))
    ctx.upload_medium_density(furnace_grid(), filter=1)
    try:
        ctx.reset_stats()
        ctx.dispatch(at(cam, 0), 1)
        out, st = ctx.read_output(), ctx.stats()
    finally:
        ctx.set_medium(None)
        ctx.upload_environment(None)
    assert st.segments > 1.2 * BW * BW                      # paths did scatter
    assert np.all(out[..., :3] == np.float32(0.5))


@pytest.mark.parametrize("filt", [0, 1])
def test_furnace_with_mis(ctx, filt):
    """the same with the sky sampled: the next-event samples, weighted by ratio tracking, and the weighted misses add up to the sky's
    radiance only if ratio tracking estimates the transmittance of the medium delta tracking walks"""
    frames = 256
    cam = layout.make_camera(BW, BW)
    setup(ctx, empty_scene(), BW, BW, moments=True, do_mis=1, max_bounces=64)
    ctx.upload_environment(uniform_sky(0.5))
    ctx.set_medium(**dict(furnace_medium(cam).kwargs(), sigma_t=3.0))
    ctx.upload_medium_density(furnace_grid(), filter=filt)
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
    assert_means(mean, var, tiles, np.full(mean.shape, 0.5 * LUM.sum()), "furnace under a grid with MIS, filter %d:" % filt)


# ---- 5. single scattering of a point light through two cells ---------------------------------------------------------------------------------
def optical_depth(m, rho2, p, w, t0, t1):
    """the integral of sigma_t rho over p + t w, t in [t0, t1] (inside the box), for the 2 x 1 x 1 nearest grid rho2: piecewise constant
    on either side of the plane x = the box's middle; float64"""
    mid = 0.5 * (float(m.box_min[0]) + float(m.box_max[0]))
    x0 = p[:, 0] + t0 * w[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = np.where(w[:, 0] != 0, (mid - p[:, 0]) / w[:, 0], np.inf)
    tc = np.clip(np.where(np.isnan(tc), np.inf, tc), t0, t1)                # where the plane is crossed, within the stretch
    low_first = (x0 < mid) | ((x0 == mid) & (w[:, 0] < 0))
    first, second = np.where(low_first, rho2[0], rho2[1]), np.where(low_first, rho2[1], rho2[0])
    crossed = (tc > t0) & (tc < t1)
    tc = np.where(crossed, tc, t1)
    return m.sigma_t * (first * (tc - t0) + second * (t1 - tc))


def test_single_scattering_of_a_point_light_through_two_cells(ctx):
    """test_single_scattering_of_a_point_light with the density (1, 0.25) on the two halves of the box along x. The expectation along a
    pixel's centre ray is the integral over t of sigma_t rho(x) exp(-tau(a .. t)) albedo exp(-tau(x -> light)) p I / dist^2 w_mis /
    pdf_light, tau the piecewise-linear optical depth; a float64 midpoint rule of 4 096 steps."""
    W = H = 32
    frames = 256
    rho2 = np.float64([1.0, 0.25])
    light_pos, intensity = np.array((0.3, 3.2, -0.2)), 6.0e4
    lights = np.zeros(1, layout.LIGHT)
    lights[0]["position"], lights[0]["light_type"], lights[0]["color"], lights[0]["intensity"] = tuple(light_pos), layout.LIGHT_POINT, (1, 1, 1), intensity
    e = empty_scene()
    sc = scenes.Scene("empty_with_point_light", e.tris, e.mats, e.nodes, lights, None)
    m = medium_ref.Medium(1.8, (0.9, 0.7, 0.5), 0.0, (-1.5, 0.0, -1.2), (1.5, 2.0, 1.0))
    cam = layout.make_camera(W, H, aperture=0.0)
    setup(ctx, sc, W, H, moments=True, max_bounces=1, do_mis=1)
    ctx.set_medium(**m.kwargs())
    ctx.upload_medium_density(rho2.astype(np.float32).reshape(1, 1, 2))
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
    mid = 0.5 * (float(m.box_min[0]) + float(m.box_max[0]))
    low = crossing = 0
    for k in np.flatnonzero(inside):
        t = a[k] + (np.arange(steps) + 0.5) * (b[k] - a[k]) / steps
        x = o64[k] + t[:, None] * d64[k]
        to_l = light_pos - x
        dist = np.linalg.norm(to_l, axis=1)
        assert dist.min() > 1.0 and dist.max() < 100.0
        wi = to_l / dist[:, None]
        _, far, _, _ = medium_ref.interval(m, x.astype(np.float32), wi.astype(np.float32), np.full(steps, INF))
        tau_light = optical_depth(m, rho2, x, wi, np.zeros(steps), np.minimum(far, dist))      # x is inside: the leg starts at 0
        tau_cam = optical_depth(m, rho2, np.tile(o64[k], (steps, 1)), np.tile(d64[k], (steps, 1)), np.full(steps, a[k]), t)
        rho = np.where(x[:, 0] < mid, rho2[0], rho2[1])
        low += rho[0] == rho2[0]                                                # a view ray keeps to its side of the plane x = middle ...
        crossing += bool(np.any((x[:, 0] < mid) != (light_pos[0] < mid)))      # ... and on one side its legs to the light cross it
        f = m.sigma_t * rho * np.exp(-tau_cam) * np.exp(-tau_light) * p * intensity / dist ** 2 * w_mis / pdf_l
        want[k] = f.sum() * (b[k] - a[k]) / steps * float((m.albedo * LUM).sum())
    mean, var, tiles = tile_stats(mom, frames)
    assert 0.3 < inside.mean() and want.max() > 0.05
    assert 0.3 * inside.sum() < low < 0.7 * inside.sum() and crossing > 0.3 * inside.sum()       # both cells are seen, both legs matter
    assert_means(mean, var, tiles, want.reshape(H, W), "single scattering through two cells:")


# ---- 6. every path through the dispatch ------------------------------------------------------------------------------------------------------
def cornell_in_smoke(c, frames=5, aovs=(), moments=False, fog=True, **opt):
    sc = cornell()
    setup(c, sc, FW, FH, aovs=aovs, moments=moments, **opt)
    if fog:
        c.set_medium(sigma_t=1.5, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
        c.upload_medium_density(R.probe_grid((3, 5, 2)), filter=1)
    try:
        c.dispatch(layout.make_camera(FW, FH), frames)
        out = c.read_output()
        planes = {a: c.read_aov(a) for a in aovs}
    finally:
        c.set_medium(None)
    return out, planes


def test_dispatch_paths_agree(ctx):
    base, _ = cornell_in_smoke(ctx, overlap=1, frames_per_batch=1)
    clear, _ = cornell_in_smoke(ctx, overlap=1, frames_per_batch=1, fog=False)
    assert base[..., :3].max() > 0 and not same(base, clear)
    assert same(base, cornell_in_smoke(ctx, overlap=0, frames_per_batch=1)[0])
    assert same(base, cornell_in_smoke(ctx, overlap=1, frames_per_batch=3)[0])
    assert same(base, cornell_in_smoke(ctx, overlap=0, frames_per_batch=0)[0])
    all_planes = ("albedo", "normal", "id")
    with_planes, planes = cornell_in_smoke(ctx, overlap=0, frames_per_batch=3, aovs=all_planes)
    assert same(base, with_planes)
    assert same(base, cornell_in_smoke(ctx, overlap=1, frames_per_batch=0, aovs=("normal",))[0])
    # the first-hit planes are those without a medium, bit for bit
    _, clear_planes = cornell_in_smoke(ctx, overlap=0, frames_per_batch=3, aovs=all_planes, fog=False)
    for a in all_planes:
        assert same(planes[a], clear_planes[a]), a
    ctx.set_aovs()


def test_adaptive_with_every_pixel_active_equals_plain_dispatch(ctx):
    sc, cam = cornell(), layout.make_camera(FW, FH)
    setup(ctx, sc, FW, FH, moments=True)
    ctx.set_medium(sigma_t=1.5, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
    ctx.upload_medium_density(R.probe_grid((3, 5, 2)), filter=1)
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
    want, _ = cornell_in_smoke(ctx, frames=3)
    g = R.probe_grid((3, 5, 2))
    with native.MultiContext([0, 0], loopback=True) as m:
        m.upload_scene(sc)
        m.resize(FW, FH)
        m.set_options(max_bounces=8, do_mis=1)
        with pytest.raises(native.PtmiError) as e:
            m.upload_medium_density(g)
        assert e.value.code == -4                                           # no medium in place
        m.set_medium(sigma_t=1.5, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
        m.upload_medium_density(g, filter=1)
        m.dispatch(layout.make_camera(FW, FH), 3)
        got = m.read_output()
        bad = g.copy()
        bad[1, 2, 1] = 1.5
        with pytest.raises(native.PtmiError) as e:
            m.upload_medium_density(bad, filter=1)
        assert e.value.code == -1
        with pytest.raises(native.PtmiError) as e:                          # the optical-depth limit, checked before any device changes
            m.set_medium(sigma_t=1e4, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
        assert e.value.code == -5
        for i in range(2):
            h = m.L.ptmi_multi_context(m.h, i)
            st = native.MediumGridStatus()
            assert m.L.ptmi_medium_grid_status(h, native.ctypes.byref(st)) == 0 and st.as_dict()["dims"] == (3, 5, 2) and st.filter == 1
        m.dispatch(layout.make_camera(FW, FH), 3)
        again = m.read_output()
        m.upload_medium_density(None)
        m.set_medium(None)
    assert same(got, want) and same(again, want)


# ---- 7. nothing else moved -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_64x48_4spp_mis", "cornell_64x64_4spp_b4_nomis", "random_soup3_48x48_3spp"])
@pytest.mark.parametrize("how", ["grid_removed_then_medium", "medium_removed_with_its_grid"])
def test_goldens_keep_their_bits(ctx, name, how):
    z, sc, cam = load(HERE + "/golden/" + name + ".npz")
    setup(ctx, sc, int(cam["width"]), int(cam["height"]), max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
    ctx.set_medium(sigma_t=0.7, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
    ctx.upload_medium_density(R.probe_grid((3, 5, 2)), filter=1)
    assert ctx.medium_grid_status().as_dict()["dims"] == (3, 5, 2)
    if how == "grid_removed_then_medium":
        ctx.upload_medium_density(None)
        assert ctx.medium_grid_status().as_dict()["dims"] == (0, 0, 0) and ctx.get_medium() is not None
    ctx.set_medium(None)
    assert ctx.medium_grid_status().as_dict()["dims"] == (0, 0, 0) and ctx.get_medium() is None
    ctx.reset_stats()
    ctx.dispatch(cam, int(z["frames"]))
    out, st = ctx.read_output(), ctx.stats()
    assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"])
    assert same(out, z["image"])


def test_homogeneous_fog_keeps_its_bits_around_a_grid(ctx):
    sc, cam = cornell(), layout.make_camera(FW, FH)
    setup(ctx, sc, FW, FH)
    ctx.set_medium(sigma_t=0.5, albedo=(0.9, 0.8, 0.7), g=0.3, box=scene_box(sc))
    try:
        ctx.dispatch(cam, 4)
        before = ctx.read_output()
        ctx.upload_medium_density(R.probe_grid((16, 16, 16)))
        ctx.dispatch(cam, 4)
        gridded = ctx.read_output()
        ctx.upload_medium_density(None)
        ctx.dispatch(cam, 4)
        after = ctx.read_output()
    finally:
        ctx.set_medium(None)
    assert same(before, after) and not same(before, gridded)


# ---- 8. errors and the life cycle ------------------------------------------------------------------------------------------------------------
def test_errors_keep_the_grid_and_the_medium(ctx):
    sc = cornell()
    setup(ctx, sc, FW, FH)
    box = scene_box(sc)
    diag = float(np.linalg.norm(np.asarray(box[1], np.float64) - box[0]))
    g = R.probe_grid((3, 5, 2))
    with pytest.raises(native.PtmiError) as e:
        ctx.upload_medium_density(g)
    assert e.value.code == -4                                               # needs a medium
    ctx.upload_medium_density(None)                                         # nothing to remove: fine
    good = dict(sigma_t=1.5, albedo=(0.9, 0.8, 0.7), g=0.4, box=box)
    cam = layout.make_camera(FW, FH)
    try:
        # the optical-depth limit on upload: just above it is refused, and the medium stays homogeneous
        ctx.set_medium(**dict(good, sigma_t=256.5 / diag))
        with pytest.raises(native.PtmiError) as e:
            ctx.upload_medium_density(g)
        assert e.value.code == -5 and ctx.medium_grid_status().as_dict()["dims"] == (0, 0, 0)
        ctx.set_medium(**dict(good, sigma_t=255.5 / diag))
        ctx.upload_medium_density(g)                                        # just below it is accepted
        ctx.set_medium(**good)
        ctx.upload_medium_density(g, filter=1)
        was_grid, was = ctx.medium_grid_status().as_dict(), ctx.get_medium().as_dict()
        assert dict(was_grid, rho_mean=0) == dict(dims=(3, 5, 2), filter=1, rho_min=0.0, rho_max=1.0, rho_mean=0)
        assert abs(was_grid["rho_mean"] - float(g.astype(np.float64).mean())) < 1e-12
        ctx.dispatch(cam, 2)
        before = ctx.read_output()
        for v in (1.0000001, -1e-6, np.nan, np.inf, -np.inf):
            bad = g.copy()
            bad[1, 3, 2] = v
            with pytest.raises(native.PtmiError) as e:
                ctx.upload_medium_density(bad)
            assert e.value.code == -1, v
        for kw in (dict(filter=2), dict(reserved=(0, 0, 0, 0, 0, 0, 1)), dict(reserved=(1, 0, 0, 0, 0, 0, 0)), dict(dims=(1025, 1, 1)),
                   dict(dims=(1, 1025, 1)), dict(dims=(1, 1, 1025))):
            with pytest.raises(native.PtmiError) as e:
                ctx.upload_medium_density(g, **kw)
            assert e.value.code == -1, kw
        # ... and on a later ptmi_set_medium, which leaves the medium and the grid as they were; a bad field does too
        with pytest.raises(native.PtmiError) as e:
            ctx.set_medium(**dict(good, sigma_t=256.5 / diag))
        assert e.value.code == -5
        with pytest.raises(native.PtmiError) as e:
            ctx.set_medium(**dict(good, g=2.0))
        assert e.value.code == -1
        assert ctx.medium_grid_status().as_dict() == was_grid and ctx.get_medium().as_dict() == was
        ctx.dispatch(cam, 2)
        assert same(ctx.read_output(), before)
        # a zero dimension removes the grid like a NULL pointer
        ctx.upload_medium_density(g, dims=(3, 0, 2))
        assert ctx.medium_grid_status().as_dict()["dims"] == (0, 0, 0) and ctx.get_medium().as_dict() == was
        ctx.dispatch(cam, 2)
        assert not same(ctx.read_output(), before)          # and the grid did shape that render
        # a medium past the limit is fine once the grid is gone
        ctx.set_medium(**dict(good, sigma_t=256.5 / diag))
    finally:
        ctx.set_medium(None)
