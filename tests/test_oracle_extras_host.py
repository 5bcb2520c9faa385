"""The oracle's extras without a GPU (oracle/pt_oracle.h pto_extras): the environment map and the participating medium inside the
oracle's trace(), held against what does not depend on any kernel before tests/test_gpu_shade_extras.py holds the kernels to them:
  * absent, they change nothing render() and render_census() return; in place but inert (an all-black map, a flat box) they
    reproduce the stored fixtures bit for bit — what DESIGN.md §10 and §11 say of the kernels;
  * their functions against the float64 models of tests/medium_ref.py and tests/env_ref.py, within the tolerances the device
    probes are held to;
  * physics: the white furnace without next-event estimation is exactly the sky's radiance; an absorbing slab follows Beer-Lambert;
  * the fog / sky gauntlet (tests/gauntlet_scenes.py gauntlet_fog, FOG_STATES) reaches every new census event in every bounce class;
  * what the device's 1 - 2 ulp logf / expf / atan2f / acosf may change in those renders (ulp_nudge): the tolerance and the
    set-aside shares the GPU test uses, measured here and held to the constants in tests/medium_ref.py."""
import numpy as np
import pytest

import env_ref
import gauntlet_scenes as G
import medium_ref
import oracle_lib
import test_env_host
from ptmi import layout, native, scenes
from test_golden import FILES, load, same
from test_gpu_environment import empty_scene, uniforms, unique_map
from test_gpu_medium import furnace_medium, uniform_sky
from test_shade_census_host import MIN_COUNT, classes, extras_events

LUM = np.float32((0.2126, 0.7152, 0.0722)).astype(np.float64)
STATS = ("paths", "segments", "shadow_rays", "nodes_visited", "tris_tested", "closest_hits", "max_stack")
GOLDEN_IDS = [f.split("/")[-1][:-4] for f in FILES]


@pytest.fixture(scope="module")
def fog_scene():
    return G.gauntlet_fog()


def env_of(texels, **kw):
    c, prob, alias, wsum = native.env_table(texels)
    return dict(dict(texels=texels, c=c, prob=prob, alias=alias, sampled=int(wsum > 0)), **kw)


# ---- 1. absent, and in place but inert ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_IDS + list(G.SCENES) + ["gauntlet_fog"])
def test_absent_extras_change_nothing(oracle, name):
    if name in GOLDEN_IDS:
        z, sc, cam = load(FILES[GOLDEN_IDS.index(name)])
        frames, mb, mis = int(z["frames"]), int(z["bounces"]), int(z["mis"])
    else:
        sc, cam, frames, mb, mis = (G.gauntlet_fog() if name == "gauntlet_fog" else G.SCENES[name]()), G.camera(), 3, 8, 1
    ref, rst, rcen = oracle.render_census(sc, cam, frames, max_bounces=mb, do_mis=mis)
    plain, pst = oracle.render(sc, cam, frames, max_bounces=mb, do_mis=mis)
    assert same(plain, ref)
    for extras in (None, oracle.extras()):                  # no struct, and a struct with neither part
        out, st, border = oracle.render_ext(sc, cam, frames, extras, max_bounces=mb, do_mis=mis)
        cout, cst, cborder, cen = oracle.render_census_ext(sc, cam, frames, extras, max_bounces=mb, do_mis=mis)
        assert same(out, ref) and same(cout, ref)
        assert np.all(np.isinf(border)) and np.all(np.isinf(cborder))
        for k in STATS:
            assert getattr(st, k) == getattr(rst, k) == getattr(cst, k) == getattr(pst, k), k
        assert list(cen) == list(rcen)
        for ev in cen:
            assert np.array_equal(cen[ev], rcen[ev]), ev
    xs, ys, fr = np.arange(40) % int(cam["width"]), np.arange(40) % int(cam["height"]), np.arange(40) % frames
    rad, seg = oracle.trace_paths(sc, cam, xs, ys, fr, max_bounces=mb, do_mis=mis)
    rad2, seg2, _ = oracle.trace_paths_ext(sc, cam, xs, ys, fr, None, max_bounces=mb, do_mis=mis)
    assert np.array_equal(rad.view(np.uint32), rad2.view(np.uint32)) and np.array_equal(seg, seg2)
    one, log = oracle.trace_path(sc, cam, 5, 7, 1, max_bounces=mb, do_mis=mis)
    one2, log2 = oracle.trace_path_ext(sc, cam, 5, 7, 1, oracle.extras(), max_bounces=mb, do_mis=mis)
    assert np.array_equal(one.view(np.uint32), one2.view(np.uint32)) and np.array_equal(log.view(np.uint32), log2.view(np.uint32))


@pytest.mark.parametrize("how", ["all_black_map", "flat_box", "both"])
@pytest.mark.parametrize("name", GOLDEN_IDS)
def test_inert_features_keep_the_goldens(oracle, name, how):
    """the ENV / MED branches of trace() with nothing to add, nothing to sample and no segment with an interval"""
    z, sc, cam = load(FILES[GOLDEN_IDS.index(name)])
    black = np.zeros((8, 16, 4), np.float32)
    black[..., 3] = 1.0
    env = env_of(black, intensity=1.0) if how != "flat_box" else None
    assert env is None or env["sampled"] == 0               # what the library decides for a map whose weights sum to zero
    fog = dict(sigma_t=50.0, albedo=0.9, g=0.3, box=((-5.0, 0.3712, -5.0), (5.0, 0.3712, 5.0))) if how != "all_black_map" else None
    out, st, _, cen = oracle.render_census_ext(sc, cam, int(z["frames"]), oracle.extras(env, fog), max_bounces=int(z["bounces"]),
                                               do_mis=int(z["mis"]))
    assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"])
    assert same(out, z["image"])
    if fog:
        assert cen["med_no_interval"].sum() == st.segments and not cen["med_interval_no_scatter"].any()
    if env:                                                 # a black sky adds nothing but the NaN of a throughput that is not finite, as no sky does
        plain = oracle.render_census(sc, cam, int(z["frames"]), max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))[2]
        assert not cen["miss_sky_weighted"].any() and not cen["nee_env"].any() and not cen["env_weight_at_surface"].any()
        assert np.array_equal(cen["miss_sky_unweighted"], plain["miss_nonfinite"]) and np.array_equal(cen["miss_sky_zero"], plain["miss_finite"])


# ---- 2. the extras' functions against the float64 models -------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0.0, 0.6, -0.8])
@pytest.mark.parametrize("box_index", [0, 1])
def test_medium_functions_against_the_model(oracle, box_index, g):
    """the inputs, the criterion and the limits of test_gpu_medium.py::test_probes_against_the_model"""
    m = medium_ref.Medium(1.3, 0.8, g, *medium_ref.BOXES[box_index])
    ex = oracle.extras(medium=m.kwargs())
    o, d, t_hit, r = medium_ref.probe_inputs(box_index)
    step = oracle.ext_probe(ex, oracle_lib.PROBE_MED_STEP, np.column_stack([o, d, t_hit, r[:, 0]]))
    ph = oracle.ext_probe(ex, oracle_lib.PROBE_MED_PHASE, np.column_stack([d, r[:, 1], r[:, 2]]))
    sc = step[:, 3] != 0
    got = dict(scattered=sc, a=step[:, 0], b=step[:, 1], s=step[:, 2], x=step[:, 4:7],
               dir=np.where(sc[:, None], ph[:, :3], 0.0), pdf=np.where(sc, ph[:, 4], 0.0))
    m64 = medium_ref.step(m, o, d, t_hit, r)
    geom, dev_dir, pdf, aside = medium_ref.step_deviations(got, m64)
    o2, wi, dist = medium_ref.tr_inputs(box_index)
    tr = oracle.ext_probe(ex, oracle_lib.PROBE_MED_TR, np.column_stack([o2, wi, dist]))[:, 0]
    dev_tr = medium_ref.deviation(tr, medium_ref.transmittance(m, o2, wi, dist))
    print("box %d g %g: a, b, s, x %.3g, Tr %.3g (limit %.3g); direction %.3g (limit %.3g); density %.3g (limit %.3g); %.2f %% set aside"
          % (box_index, g, geom, dev_tr, medium_ref.TOL_GEOM, dev_dir, medium_ref.TOL_DIR, pdf, medium_ref.TOL_PDF, 100 * aside))
    assert aside <= 0.01
    assert not step[~(m64["b"] > m64["a"]), 2].any() and not step[~sc, 4:7].any()
    assert geom <= medium_ref.TOL_GEOM and dev_tr <= medium_ref.TOL_GEOM and dev_dir <= medium_ref.TOL_DIR and pdf <= medium_ref.TOL_PDF
    # the sampled cosine is the one the direction makes with the ray, and the phase value is the model's at that cosine
    both = sc & m64["scattered"]
    ct64 = medium_ref.sample_cos(g, r[:, 1])
    assert np.abs(ph[both, 3] - ct64[both]).max() <= medium_ref.TOL_DIR


@pytest.mark.parametrize("W,H,content", [c for c in test_env_host.CASES if c[:2] != (1, 1)])
@pytest.mark.parametrize("rotation", [0.0, 1.0, -2.5])
def test_environment_functions_against_the_model(oracle, W, H, content, rotation):
    """test_env_host.py's maps; the criteria of test_gpu_environment.py's lookup and sampling tests"""
    t = test_env_host.make_map(W, H, content) * np.float32(0.25) + unique_map(W, H) * np.float32(0.01)
    if content == "one_black_row":
        t[H // 2, :, :3] = 0.0
    env = env_of(t, intensity=0.75, rotation=rotation)
    ex = oracle.extras(env)
    # sampling
    r = uniforms(4096, 11)
    got = oracle.ext_probe(ex, oracle_lib.PROBE_ENV_SAMPLE, r)
    tex = got[:, 7].view(np.uint32)
    mt, md, mpdf = env_ref.sample(t, env["prob"], env["alias"], r, rotation)
    assert np.array_equal(tex, mt)
    if content == "one_black_row":
        assert not np.isin(tex, np.arange(W) + (H // 2) * W).any()
    err = np.abs(got[:, :3].astype(np.float64) - md).max()
    assert err <= 2e-6
    assert same(got[:, 3:6], t.reshape(-1, 4)[tex, :3] * np.float32(0.75))
    sin_t = np.sin((tex // W + r[:, 3].astype(np.float64)) / H * np.pi)
    ok = sin_t > 1e-3
    assert np.all(np.abs(got[ok, 6] - mpdf[ok]) <= (1e-6 + 1e-6 / sin_t[ok]) * mpdf[ok])
    # lookup: every texel's centre, and the sampled directions (which lie in the texel they were sampled from unless near its border)
    d = env_ref.texel_centres(W, H, rotation)
    look = oracle.ext_probe(ex, oracle_lib.PROBE_ENV_LOOKUP, d)
    idx, le, pdf, uW, vH = env_ref.lookup(t, d, 0.75, rotation)
    assert np.array_equal(idx, np.arange(W * H)) and np.array_equal(look[:, 4].view(np.uint32), idx)
    assert same(look[:, :3], le)
    lit = pdf > 0
    assert np.all(look[~lit, 3] == 0) and (np.abs(look[lit, 3] - pdf[lit]) / pdf[lit]).max() <= 1e-5
    assert np.abs(look[:, 5] - 0.5).max() <= 1e-3             # a centre is half a texel from its borders
    back = oracle.ext_probe(ex, oracle_lib.PROBE_ENV_LOOKUP, got[:, :3])
    _, _, _, uW, vH = env_ref.lookup(t, got[:, :3], 0.75, rotation)
    model_border = np.minimum(np.abs(uW - np.round(uW)), np.abs(vH - np.round(vH)))
    inner = model_border >= env_ref.BORDER_BAND
    assert inner.mean() > 0.9 and np.array_equal(back[inner, 4].view(np.uint32), tex[inner])
    # the distance the oracle reports is the model's, within the float32 roundings of u W (atan2f, the rotation, / 2 pi + 0.5, the
    # product: a few steps of a float32 of magnitude up to W, W 2^-23 each; 4 of them is a third of the band for W = 64)
    assert np.abs(back[:, 5] - model_border).max() <= 4 * W * 2.0 ** -23 < env_ref.BORDER_BAND / 3
    print("%dx%d %s rot %g: direction error %.3g, %.2f %% of the sampled directions within the band" % (W, H, content, rotation, err, 100 * (1 - inner.mean())))


# ---- 3. physics, on the oracle alone ----------------------------------------------------------------------------------------------
def test_furnace_without_next_event_estimation_is_exact(oracle):
    """albedo 1 inside a uniform sky: the throughput stays 1, roulette (rng > 1) never fires, every path ends in a miss that adds 0.5"""
    BW = 64
    cam = layout.make_camera(BW, BW)
    ex = oracle.extras(env_of(uniform_sky(0.5), intensity=1.0), furnace_medium(cam).kwargs())
    out, st, _, cen = oracle.render_census_ext(empty_scene(), cam, 1, ex, max_bounces=64, do_mis=0)
    assert st.segments > 1.2 * BW * BW                      # paths did scatter
    assert np.all(out[..., :3] == np.float32(0.5))
    assert not cen["med_roulette_kill"].any() and cen["med_roulette_survival"].any() and not cen["miss_sky_weighted"].any()


@pytest.mark.parametrize("depth", [0.5, 2.0])
def test_beer_lambert(oracle, depth):
    """test_gpu_medium.py::test_beer_lambert on the oracle: an absorbing slab between the camera and a uniform sky; every sample is 0.5
    with the probability exp(-sigma_t l) of its own ray. Tile and image means within 4 standard errors, from the samples' own variance."""
    W = H = 32
    frames, thickness, tile = 64, 0.8, 16
    m = medium_ref.Medium(depth / thickness, 0.0, 0.0, (-50.0, -50.0, 0.5), (50.0, 50.0, 0.5 + thickness))
    cam = layout.make_camera(W, H)
    ex = oracle.extras(env_of(uniform_sky(0.5), intensity=1.0), m.kwargs())
    f, ys, xs = np.meshgrid(np.arange(frames), np.arange(H), np.arange(W), indexing="ij")
    rad, seg, _ = oracle.trace_paths_ext(empty_scene(), cam, xs.ravel(), ys.ravel(), f.ravel(), ex, max_bounces=2)
    o, d, _ = oracle.raygen(cam, xs.ravel(), ys.ravel(), f.ravel())
    _, _, a, b = medium_ref.interval(m, o, d, np.full(len(o), np.inf, np.float32))
    assert np.all(b > a) and np.all(seg == 1)               # the slab covers the view; a scatter ends the path (albedo 0)
    lum = (rad.astype(np.float64) @ LUM).reshape(frames, H, W)
    assert set(np.unique(rad)) == {np.float32(0.0), np.float32(0.5)}
    want = (0.5 * LUM.sum() * np.exp(-m.sigma_t * (b - a))).reshape(frames, H, W).mean(axis=0)
    mean, var = lum.mean(axis=0), lum.var(axis=0) / frames
    tiles = lambda x: x.reshape(H // tile, tile, W // tile, tile).sum(axis=(1, 3))
    diff, se = np.abs(tiles(mean) - tiles(want)), np.sqrt(tiles(var))
    print("optical depth %g: tile means |diff| / se" % depth, np.round(diff / se, 2).tolist())
    assert np.all(se > 0) and np.all(diff <= 4.0 * se)
    d_img, se_img = abs(mean.mean() - want.mean()), np.sqrt(var.sum()) / mean.size
    print("image means %.6f %.6f, |diff| / se %.2f" % (mean.mean(), want.mean(), d_img / se_img))
    assert d_img <= 4.0 * se_img


# ---- 4. the census of the fog / sky gauntlet -------------------------------------------------------------------------------------
# Cells that cannot occur, each with its reason (classes as in test_shade_census_host.py: A bounce 0, B 1 .. rb, C rb + 1, D later)
EXEMPT = {
    ("med_roulette_kill", "A"): "roulette is played from bounce rb on",
    ("med_roulette_survival", "A"): "roulette is played from bounce rb on",
    ("miss_sky_weighted", "A"): "the camera ray carries no weight",
}


def new_events(oracle):
    return extras_events(oracle.census_events())


@pytest.fixture(scope="module")
def fog_census(oracle, fog_scene):
    """{(state, max_bounces, tile): (image, stats, border, census)} of every reference render the GPU test uses, and of the fog whose albedo is 0"""
    return {(state, mb, tile): G.render_fog(oracle, fog_scene, state, native.env_table, mb, tile)
            for state in G.FOG_STATES for mb, tile in G.fog_oracle_renders()}


def test_fog_gauntlet_reaches_every_new_branch_in_every_bounce_class(oracle, fog_scene, fog_census):
    assert len(fog_scene.tris) <= 400 and G.FOG_FRAMES <= G.FRAMES
    kinds = set(fog_scene.lights["light_type"].tolist())
    assert kinds == {layout.LIGHT_EMISSIVE, layout.LIGHT_DIRECTIONAL, layout.LIGHT_POINT}
    events = new_events(oracle)
    assert len(events) == 23 and {e for e, _ in EXEMPT} <= set(events)
    total = {n: np.zeros(64, np.int64) for n in oracle.census_events()}
    for (state, mb, tile), (_, st, _, cen) in fog_census.items():
        fig = G.gpu_figures_ext(cen, mb)
        assert fig["shadow_rays"] == st.shadow_rays and sum(fig["segments_by_bounce"]) == st.segments, (state, mb, tile)
        for n in total:
            total[n] += cen[n].astype(np.int64)
    rb = G.repack_bounce()
    assert not total["med_roulette_kill"][:rb].any() and not total["med_roulette_survival"][:rb].any() and total["miss_sky_weighted"][0] == 0
    short = []
    for n in events:
        for cls, count in classes(total[n]).items():
            if (n, cls) in EXEMPT:
                assert count == 0, f"{n} in class {cls} is listed as impossible but happened {count} times"
            elif count < MIN_COUNT:
                short.append((n, cls, count))
    assert not short, f"cells reached fewer than {MIN_COUNT} times: {short}"
    # and the surface's own next-event events still happen beside the new ones, in every class
    for n in ("nee_directional", "nee_point", "nee_emissive", "would_leave_record", "contribution_zero", "sample_pdf_not_positive"):
        assert min(classes(total[n]).values()) >= MIN_COUNT, n


def test_fog_gauntlet_geometry(fog_scene):
    """what the scene is built to hold: the fog box covers a part of the room, one camera stands outside it and one inside, a
    transmissive object lies inside it, one albedo channel is 0 and one state's albedo is all 0, the map is 16 x 8 and not uniform"""
    lo, hi = (np.asarray(b) for b in G.FOG_BOX)
    inside = lambda p: bool(np.all(np.asarray(p) > lo) and np.all(np.asarray(p) < hi))
    assert not inside(G.CAMERA["position"]) and inside(G.FOG_CAMERA_INSIDE["position"])
    assert hi[0] < 1 and hi[1] < 2 and hi[2] < 1 and lo[0] > -1
    glass = fog_scene.mats["transmission"][fog_scene.tris["material_index"]] > 0
    assert glass.any() and all(inside(v) for v in fog_scene.tris["v0"][glass][:, :3])
    alb = [s["fog"]["albedo"] for s in G.FOG_STATES.values() if s["fog"]]
    assert any(0.0 in a and max(a) > 0 for a in alb) and any(max(a) == 0 for a in alb)
    assert {G.FOG_STATES[s]["camera"]["position"] for s in G.FOG_GPU_STATES if G.FOG_STATES[s]["fog"]} == {G.CAMERA["position"], G.FOG_CAMERA_INSIDE["position"]}
    t = G.fog_sky()
    assert t.shape == (8, 16, 4) and len(np.unique(t[..., :3].reshape(-1, 3), axis=0)) > 64 and (t[..., :3].max(axis=-1) == 0).sum() > 8
    assert {s["sky"] for s in G.FOG_STATES.values()} == {None, "lookup", "sampled"}


# ---- 5. what the GPU may differ by: set-aside shares and the tolerance, measured on the oracle ---------------------------------
@pytest.mark.parametrize("state", ["sky_lookup", "sky_sampled"])
def test_sky_alone_sets_aside_at_most_one_percent(fog_census, state):
    """ENV alone: bit equality but on the pixels one of whose paths looked the sky up within BORDER_BAND of a texel border"""
    for mb, tile in G.fog_oracle_renders():
        out, _, border, cen = fog_census[state, mb, tile]
        rows = G.rendered_rows(tile)
        share = float((border[rows] < env_ref.BORDER_BAND).mean())
        looked = int(np.isfinite(border[rows]).sum())
        print("%s b%d%s: %.3f %% of pixels set aside; %d of %d looked the sky up" % (state, mb, "-rows" if tile else "", 100 * share, looked, border[rows].size))
        assert share <= 0.01 and np.isfinite(out).all()
        assert looked > (0.2 * border[rows].size if mb == 8 else MIN_COUNT)     # the cap is not met by looking nothing up


def test_fog_tolerance_is_four_times_what_two_ulp_change(oracle, fog_scene):
    """MED alone and ENV + MED: each reference render again with every result of logf / expf / atan2f / acosf moved by -2 .. 2 float32
    steps (the device library's documented 1 - 2 ulp). A pixel is a flip where a path of some variant took another branch — known
    exactly, from the oracle's hash of a path's decisions, not guessed from the size of the deviation: a flip late in a dim path moves
    its pixel by 1e-4 or less, one at the first bounce by the order of a sample, and the sizes in between all occur (printed). What is
    left is rounding. Holds medium_ref.MEASURED_SHADE to the largest deviation of the pixels that are no flips, that deviation to
    at least two decades below FLIP_FROM, and the share of pixels set aside to 1 %."""
    worst, edges = 0.0, np.array([0.0, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, np.inf])
    kept, flipped = np.zeros(len(edges) - 1, np.int64), np.zeros(len(edges) - 1, np.int64)
    for state in ("fog", "fog_sky_sampled"):
        for mb, tile in G.fog_oracle_renders():
            s = G.nudge_study(oracle, fog_scene, state, native.env_table, mb, tile)
            rows = G.rendered_rows(tile)
            dev, flips = s["dev"][rows], s["flips"][rows]
            aside = flips
            kept += np.histogram(dev[~flips], edges)[0]
            flipped += np.histogram(dev[flips], edges)[0]
            print("%s b%d%s: drift %.3g, %d pixels flipped (largest deviation %.3g), %.3f %% set aside"
                  % (state, mb, "-rows" if tile else "", s["drift"], flips.sum(), dev[flips].max() if flips.any() else 0.0, 100 * aside.mean()))
            assert aside.mean() <= 0.01
            assert 100.0 * s["drift"] <= G.FLIP_FROM        # the gap: rounding stays two decades below a flip of a sample's order
            worst = max(worst, s["drift"])
    print("deviation of a pixel, all renders:  " + "  ".join("[%g, %g)" % (a, b) for a, b in zip(edges[:-1], edges[1:])))
    print("   pixels whose paths kept their branches: " + "  ".join(str(n) for n in kept))
    print("   pixels with a flipped path:             " + "  ".join(str(n) for n in flipped))
    print("largest rounding deviation %.3g; medium_ref.MEASURED_SHADE %.3g, TOL_SHADE %.3g" % (worst, medium_ref.MEASURED_SHADE, medium_ref.TOL_SHADE))
    assert flipped.sum() > 0 and not kept[np.searchsorted(edges, 100.0 * worst):].any()
    # the constant is the measurement rounded up; libm's logf / expf may differ by an ulp between C libraries (as in test_medium_host.py)
    assert 0.5 * medium_ref.MEASURED_SHADE <= worst <= 1.25 * medium_ref.MEASURED_SHADE
    assert medium_ref.TOL_SHADE == 4.0 * medium_ref.MEASURED_SHADE
