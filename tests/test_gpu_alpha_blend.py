"""Alpha blending on the device (include/ptmi.h ptmi_set_alpha_blend; csrc/alpha.hip): the two probes are the numpy
model (tests/alpha_blend_ref.py) bit for bit, the ends alpha = 0 and alpha = 1 are results the library already gave, the counters
and the accumulated albedo hold the fraction alpha, both tables work together, the layer limits do what they say, refusals keep the
table, and three loopback devices give one device's bits. scenes.cornell_fence at 64 x 48 or smaller throughout."""
import numpy as np
import pytest

import alpha_blend_ref as B
import alpha_ref as A
from ptmi import layout, native, scenes
from test_gpu_alpha import ALL, at, err, fence_rays, prepare, same, same_render
from test_gpu_alpha import render as cutout_render

pytestmark = pytest.mark.gpu

W, H = 64, 48
EVERY = np.ones((1, 8, 8), bool)
NO_COUNTS = dict(path_tests=0, path_passes=0, shadow_tests=0, shadow_passes=0)


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: its tables, planes and options never reach the session's shared context"""
    with native.Context(0) as c:
        yield c


def render(c, cam, frames):
    r = cutout_render(c, cam, frames)
    r["blend"] = c.alpha_blend_status().as_dict()
    return r


def cycle(n_fences):
    """alpha [fence, row, column] cycling through 0, 0.25, 0.5, 0.75, 1 (all exact in f16)"""
    f, j, i = np.mgrid[0:n_fences, 0:scenes.FENCE_CELLS, 0:scenes.FENCE_CELLS]
    return (((f + 2 * j + i) % 5) * 0.25).astype(np.float32)


def camera_rays(c, cam, frames):
    """the rays ray generation gives every pixel of `cam` in frames 0 .. frames - 1"""
    ys, xs, fs = np.mgrid[0:int(cam["height"]), 0:int(cam["width"]), 0:frames]
    o, d, _ = c.debug_raygen(at(cam, 0), xs.ravel(), ys.ravel(), fs.ravel())
    return o, d


def binomial_ok(passes, tests, a, sigmas):
    return abs(passes - tests * (1.0 - a)) <= sigmas * np.sqrt(tests * a * (1.0 - a))


# ---- 1. the probes are the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [1, 2])
def test_probes_are_the_model(ctx, leaves):
    zs = (0.4, 0.3, 0.2)
    sc = scenes.cornell_fence(cycle(3), z=zs)
    prepare(ctx, sc, W, H, leaves=leaves)
    co, cd = camera_rays(ctx, layout.make_camera(W, H), 3)                  # 9 216 camera rays
    ro, rd = fence_rays(10784, 21, zs)
    o, d = np.concatenate([co, ro]), np.concatenate([cd, rd])
    assert len(o) == 20000
    assert err(ctx.debug_alpha_intersect, o, d) == -4                       # no table of either kind
    rng = np.random.default_rng(22)
    raw_t = ctx.debug_intersect(o, d)[0]
    dist = rng.uniform(0.3, 6.0, len(o)).astype(np.float32)
    dist[::4] = -1.0
    on_hit = (np.arange(len(o)) % 4 == 1) & (raw_t > 0)
    dist[on_hit] = raw_t[on_hit]
    results = {}
    for factor in (1.0, 0.5):
        table = B.blend_table(sc, factor)
        for seed in (0, 7):
            ctx.set_alpha_blend(table, seed=seed)
            ctx.reset_stats()
            counts, scounts = {}, {}
            want = B.resolve(ctx.debug_intersect, sc, table, o, d, seed=seed, counts=counts)
            got = ctx.debug_alpha_intersect(o, d)
            what = "factor %g seed %d leaves %d" % (factor, seed, leaves)
            assert np.array_equal(got[1], want[1]), "triangles, %s: %d differ" % (what, (got[1] != want[1]).sum())
            assert np.array_equal(got[2], want[2]), "layers, " + what
            assert same(got[0], want[0]), "t, " + what
            want_occ = B.occluded(ctx.debug_intersect, sc, table, o, d, dist, seed=seed, counts=scounts)
            got_occ = ctx.debug_alpha_occluded(o, d, dist)
            assert np.array_equal(got_occ[0], want_occ[0]) and np.array_equal(got_occ[1], want_occ[1]), "occluded, " + what
            st = ctx.alpha_blend_status().as_dict()
            assert (st["path_tests"], st["path_passes"]) == (counts["tests"], counts["passes"]), what
            assert (st["shadow_tests"], st["shadow_passes"]) == (scounts["tests"], scounts["passes"]), what
            assert (st["present"], st["n_blend"], st["seed"], st["max_layers"]) == (1, 3, seed, 4)
            assert {0, 1, 2, 3} <= set(want[2].tolist()) and 0 < want_occ[0].sum() < len(o)
            assert not want_occ[0][on_hit].any()
            assert same(ctx.debug_intersect(o, d)[0], raw_t)                # the raw probes stay raw
            results[factor, seed] = want[1]
    assert not np.array_equal(results[1.0, 0], results[1.0, 7]) and not np.array_equal(results[1.0, 0], results[0.5, 0])
    ctx.set_alpha_blend(None)


# ---- 2. the ends are old results ----------------------------------------------------------------------------------------------------
def test_the_ends_are_old_results(ctx):
    frames = 4
    cam = layout.make_camera(W, H)

    def one(alpha, drop=None, blend=None, cutoff=None):
        sc = scenes.cornell_fence(alpha, drop=drop)
        prepare(ctx, sc, W, H, aovs=ALL, moments=True, do_mis=1)
        if blend is not None:
            ctx.set_alpha_blend(np.where(np.arange(len(sc.mats)) == sc.info["fence_materials"][0], blend, -1.0))
        if cutoff is not None:
            ctx.set_alpha_cutoff(A.fence_scene(alpha)[1])
        return sc, render(ctx, cam, frames)
    zero, one_ = np.zeros((1, 8, 8), np.float32), np.ones((1, 8, 8), np.float32)
    with_fence, gone = one(zero, blend=1.0)
    assert gone["blend"]["path_tests"] == gone["blend"]["path_passes"] > 0
    assert gone["blend"]["shadow_tests"] == gone["blend"]["shadow_passes"] > 0
    assert gone["alpha"]["path_passes"] == gone["blend"]["path_passes"] and gone["alpha"]["path_exhausted"] == 0
    _, cut = one(zero, cutoff=True)
    same_render(gone, cut, "alpha 0 under factor 1 against the cutoff table at 0.5")
    assert cut["blend"] == dict(present=0, n_materials=0, n_blend=0, max_layers=0, seed=0, **NO_COUNTS)
    without, dropped = one(None, drop=EVERY)
    # (each scene numbers its triangles in its own tree's order: the ID plane names the same triangle under either numbering)
    ids, want_ids = gone.pop("id"), dropped.pop("id")
    same_render(gone, dropped, "alpha 0 under factor 1 against the scene without the fence")
    assert np.array_equal(ids[..., 1], want_ids[..., 1]) and (ids[..., 0] != 0xFFFFFFFF).all()
    for k in ("v0", "v1", "v2", "n0", "uv0"):
        assert np.array_equal(with_fence.tris[ids[..., 0]][k], without.tris[want_ids[..., 0]][k]), k
    sc, plain = one(one_)
    _, there = one(one_, blend=1.0)
    assert there["blend"]["path_tests"] > 0 and there["blend"]["path_passes"] == 0 and there["blend"]["shadow_passes"] == 0
    same_render(there, plain, "alpha 1 under factor 1 against no table")
    assert not same(plain["output"], dropped["output"])
    # a table of -1 is inert: the bits of no table, and alpha_active() stays false (it governs the schedule, and the probes ask it)
    ctx.set_alpha_blend(np.full(len(sc.mats), -1.0, np.float32), seed=5, max_layers=7)
    inert = render(ctx, cam, frames)
    same_render(inert, plain, "a table of -1 against no table")
    assert inert["blend"] == dict(present=1, n_materials=len(sc.mats), n_blend=0, max_layers=7, seed=5, **NO_COUNTS)
    assert err(ctx.debug_alpha_intersect, np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)) == -4
    # under an active cutoff table a blend table of -1 changes nothing either (the BLEND = false kernels: no test is counted)
    ctx.set_alpha_blend(None)
    cutoff = A.fence_scene(one_)[1]
    ctx.set_alpha_cutoff(cutoff)
    only_cut = render(ctx, cam, frames)
    ctx.set_alpha_blend(np.full(len(sc.mats), -1.0, np.float32))
    both = render(ctx, cam, frames)
    same_render(both, only_cut, "a cutoff table with and without a blend table of -1")
    assert both["blend"]["path_tests"] == 0 and both["alpha"] == only_cut["alpha"]
    ctx.set_alpha_cutoff(None)
    ctx.set_alpha_blend(None)
    ctx.set_aovs()
    ctx.set_moments(False)


# ---- 3. fractions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0.25, 0.5])
def test_fractions(ctx, a):
    """The counters of a 16-frame render are binomial in the tests: |passes - tests (1 - a)| <= 4 sqrt(tests a (1 - a)), for path and
    shadow rays. The seed is chosen beforehand, by the model alone, on the camera rays the device generates for those frames: the
    first one for which the model's own count stays within 3 standard errors."""
    frames = 16
    sc = scenes.cornell_fence(np.full((1, 8, 8), a, np.float32))
    assert np.all(sc.atlas[..., 3].astype(np.float32) == np.float32(a))     # exact in f16
    cam = layout.make_camera(W, H)
    prepare(ctx, sc, W, H, do_mis=1)
    table = B.blend_table(sc, 1.0)
    o, d = camera_rays(ctx, cam, frames)
    seed = None
    for s in range(8):
        counts = {}
        B.resolve(ctx.debug_intersect, sc, table, o, d, seed=s, counts=counts)
        print("model, a = %g seed %d: %d of %d pass" % (a, s, counts["passes"], counts["tests"]))
        assert counts["tests"] > 10000
        if binomial_ok(counts["passes"], counts["tests"], a, 3.0):
            seed = s
            break
    assert seed is not None
    ctx.set_alpha_blend(table, seed=seed)
    r = render(ctx, cam, frames)
    st = r["blend"]
    print("a = %g seed %d: %s" % (a, seed, st))
    assert st["path_tests"] >= counts["tests"] and st["shadow_tests"] > 1000
    assert binomial_ok(st["path_passes"], st["path_tests"], a, 4.0), st
    assert binomial_ok(st["shadow_passes"], st["shadow_tests"], a, 4.0), st
    assert r["alpha"]["path_exhausted"] == 0 and r["alpha"]["shadow_exhausted"] == 0
    assert r["alpha"]["path_passes"] == st["path_passes"] and r["alpha"]["shadow_passes"] == st["shadow_passes"]
    ctx.set_alpha_blend(None)


# ---- 4. frames decorrelate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0.25, 0.5])
def test_frames_decorrelate(ctx, a):
    """64 frames into the ALBEDO plane. Where every sample of a pixel meets the fence and, without the fence, a wall of one albedo,
    the plane holds fence * k / 64 + wall * (64 - k) / 64 with k the frames in which the fence was there: strictly between the two in
    every such pixel, and the k sum to a binomial count."""
    frames = 64
    cam = layout.make_camera(W, H, aperture=0.0)

    def albedo(alpha, drop=None, blend=False):
        sc = scenes.cornell_fence(alpha, drop=drop, furniture=False)
        prepare(ctx, sc, W, H, aovs=("albedo",), max_bounces=1, do_mis=0)
        if blend:
            ctx.set_alpha_blend(B.blend_table(sc, 1.0), seed=1)
        ctx.dispatch(at(cam, 0), frames)
        return ctx.read_aov("albedo")[..., :3].astype(np.float64)
    fence = albedo(np.ones((1, 8, 8), np.float32))
    wall = albedo(None, drop=EVERY)
    mixed = albedo(np.full((1, 8, 8), a, np.float32), blend=True)
    fence_colour = np.float64(np.float16((0.75, 0.6, 0.3)))
    wall_colour = wall[H // 2, W // 2]
    interior = (np.abs(fence - fence_colour).max(axis=2) < 1e-5) & (np.abs(wall - wall_colour).max(axis=2) < 1e-5)
    ch = np.abs(fence_colour - wall_colour) > 0.1                           # the channels in which the two albedos differ
    print("interior pixels %d, fence %s, wall %s" % (interior.sum(), fence_colour, wall_colour))
    assert interior.sum() > W * H // 8 and ch.any()
    lo, hi = np.minimum(fence_colour, wall_colour)[ch], np.maximum(fence_colour, wall_colour)[ch]
    m = mixed[interior][:, ch]
    assert np.all((m > lo + 1e-4) & (m < hi - 1e-4)), "a pixel holds the fence's or the wall's albedo alone"
    k = (m - wall_colour[ch]) / (fence_colour - wall_colour)[ch] * frames   # per channel: the frames with the fence there
    assert np.abs(k - np.round(k)).max() < 1e-2 and np.abs(k - k[:, :1]).max() < 1e-2
    n = interior.sum() * frames
    got = np.round(k[:, 0]).sum() / n
    se = np.sqrt(a * (1.0 - a) / n)
    print("a = %g: the fence is there in %.5f of %d samples (se %.5f)" % (a, got, n, se))
    assert abs(got - a) <= 4.0 * se
    ctx.set_alpha_blend(None)
    ctx.set_aovs()


# ---- 5. both tables ------------------------------------------------------------------------------------------------------------------
def test_both_tables(ctx):
    """fence 0 is MASK at 0.5 and blended as well, fence 1 is blended alone: the cutoff rule is asked first, and its holes are no tests"""
    zs = (0.4, 0.3)
    sc = scenes.cornell_fence(cycle(2), z=zs)
    prepare(ctx, sc, W, H)
    cutoff = np.zeros(len(sc.mats), np.float32)
    cutoff[sc.info["fence_materials"][0]] = 0.5
    table = B.blend_table(sc, 1.0)
    o, d = fence_rays(8192, 31, zs)
    dist = np.random.default_rng(32).uniform(0.3, 6.0, len(o)).astype(np.float32)
    dist[::3] = -1.0
    ctx.set_alpha_cutoff(cutoff, max_layers=3)
    ctx.set_alpha_blend(table, seed=3, max_layers=2)
    ctx.reset_stats()
    counts, scounts = {}, {}
    want = B.resolve(ctx.debug_intersect, sc, table, o, d, 3, seed=3, cutoff=cutoff, counts=counts)
    got = ctx.debug_alpha_intersect(o, d)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and same(got[0], want[0])
    want_occ = B.occluded(ctx.debug_intersect, sc, table, o, d, dist, 3, seed=3, cutoff=cutoff, counts=scounts)
    got_occ = ctx.debug_alpha_occluded(o, d, dist)
    assert np.array_equal(got_occ[0], want_occ[0]) and np.array_equal(got_occ[1], want_occ[1])
    st, ast = ctx.alpha_blend_status().as_dict(), ctx.alpha_status().as_dict()
    assert (st["path_tests"], st["path_passes"]) == (counts["tests"], counts["passes"])
    assert (st["shadow_tests"], st["shadow_passes"]) == (scounts["tests"], scounts["passes"])
    # every hole passed is counted by ptmi_alpha_status; the MASK holes among them are no tests
    passed = int(np.minimum(want[2], 3).sum())
    assert ast["path_passes"] == passed > st["path_passes"] > 0
    # the blend table alone tests the cells the cutoff rule took, and so tests more
    ctx.set_alpha_cutoff(None)
    ctx.reset_stats()
    alone = {}
    want = B.resolve(ctx.debug_intersect, sc, table, o, d, 2, seed=3, counts=alone)
    got = ctx.debug_alpha_intersect(o, d)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and same(got[0], want[0])
    assert ctx.alpha_blend_status().path_tests == alone["tests"] > counts["tests"]
    ctx.set_alpha_blend(None)


# ---- 6. layers -----------------------------------------------------------------------------------------------------------------------
def test_layers(ctx):
    zs = (0.4, 0.3, 0.2)
    sc = scenes.cornell_fence(np.zeros((3, 8, 8), np.float32), z=zs, furniture=False)
    prepare(ctx, sc, W, H)
    table = B.blend_table(sc, 1.0)
    third = sc.info["fence_materials"][2]
    n = 2048
    rng = np.random.default_rng(41)
    o = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(0.5, 1.5, n), np.full(n, 2.0)], 1).astype(np.float32)
    d = np.tile(np.float32([0.0, 0.0, -1.0]), (n, 1))
    ctx.set_alpha_blend(table, max_layers=2)
    ctx.reset_stats()
    t, tri, layers = ctx.debug_alpha_intersect(o, d)
    assert np.all(layers == 3) and np.all(sc.tris[tri]["material_index"] == third)       # still on the third fence: it stands as opaque
    assert np.allclose(t, 1.8, atol=1e-5)
    ast, st = ctx.alpha_status().as_dict(), ctx.alpha_blend_status().as_dict()
    assert (ast["path_passes"], ast["path_exhausted"]) == (2 * n, n) and (st["path_tests"], st["path_passes"]) == (3 * n, 3 * n)
    assert (ast["present"], ast["max_layers"], st["max_layers"]) == (0, 0, 2)
    ctx.reset_stats()
    occ, slayers = ctx.debug_alpha_occluded(o, d, np.full(n, 1.9, np.float32))            # a light between the third fence and the wall
    assert np.all(occ == 1) and np.all(slayers == 3)
    ast = ctx.alpha_status().as_dict()
    assert (ast["shadow_passes"], ast["shadow_exhausted"]) == (2 * n, n)
    # the loops run to the larger of the two limits: a cutoff table, even one that cuts nothing, with max_layers = 3
    ctx.set_alpha_cutoff(np.zeros(len(sc.mats), np.float32), max_layers=3)
    assert ctx.alpha_status().max_layers == 3 and ctx.alpha_blend_status().max_layers == 2
    t, tri, layers = ctx.debug_alpha_intersect(o, d)
    assert np.all(layers == 3) and not np.isin(sc.tris[tri]["material_index"], sc.info["fence_materials"]).any() and np.all(t > 2.5)
    occ, slayers = ctx.debug_alpha_occluded(o, d, np.full(n, 1.9, np.float32))
    assert np.all(occ == 0) and np.all(slayers == 3)
    ctx.set_alpha_cutoff(None)
    assert np.all(ctx.debug_alpha_intersect(o, d)[2] == 3) and np.allclose(ctx.debug_alpha_intersect(o, d)[0], 1.8, atol=1e-5)
    # ... and a render under the limit of 2 is not the render under the default
    cam = layout.make_camera(W, H)
    short = render(ctx, cam, 2)
    assert short["alpha"]["path_exhausted"] > 0 and short["alpha"]["shadow_exhausted"] > 0
    ctx.set_alpha_blend(table)
    full = render(ctx, cam, 2)
    assert full["alpha"]["path_exhausted"] == 0 and full["blend"]["max_layers"] == 4 and not same(full["output"], short["output"])
    ctx.set_alpha_blend(None)


# ---- 7. errors and the life cycle -------------------------------------------------------------------------------------------------------
def test_errors_keep_the_table_and_the_life_cycle(ctx):
    frames = 2
    fresh = native.Context(0)
    try:
        assert err(fresh.set_alpha_blend, np.zeros(3, np.float32)) == -1                   # no scene
        assert err(fresh.set_alpha_blend, None) == -1
        assert fresh.alpha_blend_status().as_dict() == dict(present=0, n_materials=0, n_blend=0, max_layers=0, seed=0, **NO_COUNTS)
    finally:
        fresh.close()
    sc = scenes.cornell_fence(cycle(2), z=(0.4, 0.3))
    cam = layout.make_camera(W, H)
    prepare(ctx, sc, W, H)
    opaque = render(ctx, cam, frames)
    ctx.set_alpha_blend(None)                                               # nothing to remove: fine
    table = B.blend_table(sc, 0.5)
    ctx.set_alpha_blend(table, max_layers=3, seed=9)
    was = ctx.alpha_blend_status().as_dict()
    assert was == dict(present=1, n_materials=len(sc.mats), n_blend=2, max_layers=3, seed=9, **NO_COUNTS)
    base = render(ctx, cam, frames)
    assert not same(base["output"], opaque["output"]) and base["blend"]["path_passes"] > 0
    for bad in (1.5, np.nan, np.inf, -np.inf, np.nextafter(np.float32(1), np.float32(2))):
        t = table.copy()
        t[0] = bad
        assert err(ctx.set_alpha_blend, t) == -1, bad
    assert err(ctx.set_alpha_blend, table[:-1]) == -1 and err(ctx.set_alpha_blend, np.append(table, 0)) == -1
    assert err(ctx.set_alpha_blend, table, max_layers=33) == -1
    for r in ((1, 0), (0, 1)):
        assert err(ctx.set_alpha_blend, table, reserved=r) == -1
    assert err(ctx.set_alpha_blend, None, reserved=(0, 1)) == -1            # a removal checks its params too
    after = render(ctx, cam, frames)
    assert after["blend"] == base["blend"] and after["blend"]["seed"] == 9
    same_render(after, base, "after the refused calls")
    # ptmi_upload_atlas and ptmi_update_materials leave the table alone
    a = sc.atlas
    ctx._ck(ctx._c.upload_atlas(ctx.h, native._p(a), a.shape[1], a.shape[0], native.ATLAS_RGBA16F))
    mats = sc.mats.copy()
    mats["base_color"][0] = (0.2, 0.3, 0.9)
    ctx.update_materials(0, mats)
    st = ctx.alpha_blend_status().as_dict()
    assert (st["present"], st["n_blend"], st["max_layers"], st["seed"]) == (1, 2, 3, 9)
    # any negative entry means "not blended", -0.0 is a factor of 0, max_layers 32 is accepted, a zero-length table removes it
    t = table.copy()
    t[0], t[1] = -7.0, -0.0
    ctx.set_alpha_blend(t, max_layers=32)
    st = ctx.alpha_blend_status().as_dict()
    assert (st["n_blend"], st["max_layers"], st["seed"]) == (3, 32, 0)
    ctx.set_alpha_blend(table, n_materials=0)
    assert ctx.alpha_blend_status().present == 0
    # a cutoff table set or removed leaves the blend table alone, and an upload removes both
    ctx.set_alpha_blend(table, seed=9, max_layers=3)
    ctx.set_alpha_cutoff(np.zeros(len(sc.mats), np.float32))
    ctx.set_alpha_cutoff(None)
    ctx.reset_stats()
    assert ctx.alpha_blend_status().as_dict() == was
    ctx.upload_scene(sc)
    ctx.reset_stats()
    assert ctx.alpha_blend_status().as_dict() == dict(present=0, n_materials=0, n_blend=0, max_layers=0, seed=0, **NO_COUNTS)
    same_render(render(ctx, cam, frames), opaque, "after the upload")


# ---- 8. multi-device -----------------------------------------------------------------------------------------------------------------
def test_three_loopback_devices_give_one_devices_bits(ctx):
    w, h, frames = 50, 37, 4
    sc = scenes.cornell_fence(cycle(2), z=(0.4, 0.3))
    cam = layout.make_camera(w, h)
    table = B.blend_table(sc, 1.0)
    prepare(ctx, sc, w, h)
    ctx.set_alpha_blend(table, seed=4)
    base = render(ctx, cam, frames)
    assert base["blend"]["path_passes"] > 0 and base["blend"]["shadow_passes"] > 0
    with native.MultiContext([0, 0, 0], loopback=True) as m:
        m.upload_scene(sc)
        m.resize(w, h)
        m.set_options(max_bounces=8, do_mis=1)
        assert err(m.set_alpha_blend, table[:-1]) == -1 and err(m.set_alpha_blend, table, max_layers=33) == -1
        bad = table.copy()
        bad[-1] = 2.0
        assert err(m.set_alpha_blend, bad) == -1 and m.alpha_blend_status().present == 0
        m.set_alpha_blend(table, seed=4)
        m.reset_stats()
        m.dispatch(at(cam, 0), frames)
        got = m.read_output()
        st, ast = m.alpha_blend_status().as_dict(), m.alpha_status().as_dict()
        for i in range(3):
            one = native.AlphaBlendStatus()
            assert m.L.ptmi_alpha_blend_status(m.L.ptmi_multi_context(m.h, i), native.ctypes.byref(one)) == 0
            assert (one.present, one.n_blend, one.seed) == (1, 2, 4) and 0 < one.path_tests < st["path_tests"]
    assert same(got, base["output"])
    assert st == base["blend"] and ast == base["alpha"]                     # the devices' counters add up to the one device's
    ctx.set_alpha_blend(None)
