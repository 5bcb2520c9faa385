"""Alpha cutouts on the device (include/ptmi.h ptmi_set_alpha_cutoff; csrc/alpha.hip): an inactive or never-passed table
changes no bit, the two probes are the numpy model (tests/alpha_ref.py) run on the raw probes, a hole renders as an absent triangle, the
layer limit and the step far from the origin do what they say, every route through the dispatch gives one result, reprojection sees the
surface behind a hole, and errors leave the table as it was."""
import functools

import numpy as np
import pytest

import alpha_ref as A
from ptmi import layout, native, scenes
from test_gpu_medium_grid import tile_means_within

pytestmark = pytest.mark.gpu

ALL = ("albedo", "normal", "id")
MEMORY_VARIANTS = (1, 8, 9)                 # PT_VARIANT_GLOBAL, _OWN_QGLOBAL, _OWN_GLOBAL: ptmi_stats.extend_variant // 10


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the table, planes and options it sets never reach the session's shared context"""
    with native.Context(0) as c:
        yield c


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def at(cam, frame):
    cam = cam.copy()
    cam["frame_index"] = frame
    return cam


def err(fn, *a, **kw):
    with pytest.raises(native.PtmiError) as e:
        fn(*a, **kw)
    return e.value.code


def prepare(c, sc, W, H, aovs=(), moments=False, **opt):
    """options first (leaves takes effect at the upload), then the scene: the upload removes any table"""
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=0, cull=1,
             traversal=0, overlap=2, perf_mode=0, leaves=0, timing=0)
    o.update(opt)
    c.set_options(**o)
    c.upload_scene(sc)
    c.upload_environment(None)
    c.set_medium(None)
    c.set_aovs(*aovs)
    c.set_moments(moments)
    c.resize(W, H)


def render(c, cam, frames):
    """`frames` frames from frame 0: the output, whatever planes are on, and the statistics of just this render"""
    c.reset_stats()
    c.write_output(np.zeros((c.height, c.width, 4), np.float32))
    c.dispatch(at(cam, 0), frames)
    r = dict(output=c.read_output())
    if c.moments():
        r["moments"] = c.read_moments()
    for a in c.aovs():
        r[a] = c.read_aov(a)
    st, ast = c.stats(), c.alpha_status()
    r["counts"] = (int(st.segments), int(st.shadow_rays))
    r["variant"] = int(st.extend_variant)
    r["alpha"] = ast.as_dict()
    return r


def same_render(got, want, what):
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            assert same(got[k], w), (what, k)
    assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "grid96":
        return scenes.grid_1m(n=96)                     # the 1 M-triangle scene's construction at 18 050 triangles
    return scenes.make(name)


# ---- 1. inert, bit for bit ---------------------------------------------------------------------------------------------------------
def inert_case(c, sc, cam, frames, what):
    plain = render(c, cam, frames)
    assert plain["output"][..., :3].max() > 0 and plain["alpha"]["present"] == 0
    n = len(sc.mats)
    c.set_alpha_cutoff(np.zeros(n, np.float32))
    zeros = render(c, cam, frames)
    assert zeros["alpha"] == dict(present=1, n_materials=n, n_cutout=0, max_layers=4, path_passes=0, path_exhausted=0,
                                  shadow_passes=0, shadow_exhausted=0)
    same_render(zeros, plain, what + ", a table of zeros")
    c.set_alpha_cutoff(np.full(n, 0.5, np.float32))
    half = render(c, cam, frames)
    assert half["alpha"] == dict(zeros["alpha"], n_cutout=n)
    same_render(half, plain, what + ", cutoff 0.5 everywhere over alpha 1")
    c.set_alpha_cutoff(None)
    assert c.alpha_status().present == 0
    return plain


@pytest.mark.parametrize("leaves", [1, 2])
@pytest.mark.parametrize("name", ["cornell_spheres", "grid96"])
def test_inert_bit_for_bit(ctx, name, leaves):
    """no pass ever happens, so the closest-hit shadow stage and the order of its additions to L must give the any-hit kernel's bits"""
    sc = scene(name)
    assert sc.atlas is None or np.all(sc.atlas[..., 3] == 1)
    W, H, frames = 64, 48, 4
    cam = layout.make_camera(W, H)
    prepare(ctx, sc, W, H, aovs=ALL, moments=True, leaves=leaves)
    for mis in (0, 1):
        for overlap in (0, 2):
            ctx.set_options(do_mis=mis, overlap=overlap)
            plain = inert_case(ctx, sc, cam, frames, "%s leaves %d do_mis %d overlap %d" % (name, leaves, mis, overlap))
            assert ctx.options().overlap == overlap                         # the stored option is left alone
            if name == "grid96":
                assert plain["variant"] // 10 in MEMORY_VARIANTS, plain["variant"]
    if name == "cornell_spheres":                                           # ... and under a sampled sky plus fog
        ctx.set_options(do_mis=1, overlap=2)
        ctx.upload_environment(scenes.sky(16, 8, "disc"), sample=1)
        v = np.concatenate([sc.tris[k][:, :3] for k in ("v0", "v1", "v2")])
        ctx.set_medium(sigma_t=0.5, albedo=(0.9, 0.8, 0.7), g=0.3, box=(tuple(v.min(axis=0)), tuple(v.max(axis=0))))
        try:
            inert_case(ctx, sc, cam, frames, "cornell_spheres under a sampled sky, in fog")
        finally:
            ctx.upload_environment(None)
            ctx.set_medium(None)
    ctx.set_aovs()
    ctx.set_moments(False)


# ---- 2. the probes against the model -----------------------------------------------------------------------------------------------
def fence_rays(n, seed, zs, offset=(0.0, 0.0, 0.0)):
    """origins on both sides of the fences, aimed at points of the fence planes' cross-section and a little beyond its rim"""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(0.1, 1.9, n), rng.uniform(1.2, 3.0, n)], 1)
    back = rng.random(n) < 0.25
    o[back, 2] = rng.uniform(-0.9, min(zs) - 0.05, back.sum())
    target = np.stack([rng.uniform(-1.1, 1.1, n), rng.uniform(-0.1, 2.1, n), rng.choice(zs, n)], 1)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (o + np.asarray(offset)).astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("leaves,offset", [(1, 0.0), (2, 0.0), (2, 200.0)])
def test_probes_are_the_model(ctx, leaves, offset):
    """... also 200 units from the origin, where the step is 2^-18 of the coordinates and a scratch origin rounds by 15 PT_EPS"""
    zs = (0.4, 0.3)
    sc, cutoff = A.fence_scene(A.checker(2), z=zs, offset=(offset,) * 3)
    prepare(ctx, sc, 8, 8, leaves=leaves)
    o, d = fence_rays(4096, 11, zs, offset=(offset,) * 3)
    assert err(ctx.debug_alpha_intersect, o, d) == -4 and err(ctx.debug_alpha_occluded, o, d, np.ones(len(o))) == -4   # no table
    rng = np.random.default_rng(12)
    raw_t = ctx.debug_intersect(o, d)[0]
    dist = rng.uniform(0.3, 6.0, len(o)).astype(np.float32)
    dist[::4] = -1.0                                                        # directional
    on_hit = (np.arange(len(o)) % 4 == 1) & (raw_t > 0)
    dist[on_hit] = raw_t[on_hit]                                            # the t < dist - 2e-6 edge at the first surface
    seen = {}
    for max_layers in (0, 1, 2):
        ctx.set_alpha_cutoff(cutoff, max_layers=max_layers)
        L = max_layers or A.DEFAULT_LAYERS
        assert ctx.alpha_status().max_layers == L
        want = A.resolve(ctx.debug_intersect, sc, cutoff, o, d, L)
        got = ctx.debug_alpha_intersect(o, d)
        assert np.array_equal(got[1], want[1]), "triangles, max_layers %d: %d differ" % (L, (got[1] != want[1]).sum())
        assert np.array_equal(got[2], want[2]), "layers, max_layers %d" % L
        assert same(got[0], want[0]), "t, max_layers %d: %d differ" % (L, (got[0].view(np.uint32) != want[0].view(np.uint32)).sum())
        seen[L] = want[2]
        want_occ = A.occluded(ctx.debug_intersect, sc, cutoff, o, d, dist, L)
        got_occ = ctx.debug_alpha_occluded(o, d, dist)
        assert np.array_equal(got_occ[0], want_occ[0]) and np.array_equal(got_occ[1], want_occ[1]), "occluded, max_layers %d" % L
        # behind the holes of a closed room something is always there: a directional light is occluded whatever it passes
        assert want_occ[0][dist < 0].all() and want_occ[1][dist < 0].max() >= 1
        assert 0 < want_occ[0][dist > 0].sum() < (dist > 0).sum() and want_occ[1][dist > 0].max() >= 1
        assert not want_occ[0][on_hit].any()                                # a light on the first surface is not occluded by it
        # the raw probes stay raw
        assert same(ctx.debug_intersect(o, d)[0], raw_t)
    assert {0, 1, 2} <= set(seen[4].tolist())                               # no hole, one fence, both
    exhausted = seen[1] == 2                                                # still on the second fence's hole after one layer
    assert exhausted.any() and np.all(seen[4][exhausted] == 2) and np.array_equal(seen[2], seen[4])
    ctx.set_alpha_cutoff(None)


# ---- 3. a hole is an absent triangle -----------------------------------------------------------------------------------------------
FW, FH, FRAMES = 96, 64, 16
HOLES = (np.add.outer(np.arange(8), np.arange(8)) % 3 != 1)[None]          # two cells of every three, in diagonal stripes


def holes_vs_dropped(c, holes, zs=(0.4,), offset=(0.0, 0.0, 0.0), max_layers=0, fog=False, **opt):
    """(the fences with alpha 0 on `holes` under the cutoff table, a fresh upload of the scene without those cells' triangles)"""
    cam = layout.make_camera(FW, FH, position=tuple(np.float32((0.0, 1.0, 2.8)) + np.float32(offset)))
    out = []
    for cut in (True, False):
        sc, cutoff = A.fence_scene(1.0 - holes if cut else None, z=zs, offset=offset, drop=None if cut else holes)
        prepare(c, sc, FW, FH, moments=True, **opt)
        if fog:
            v = np.concatenate([sc.tris[k][:, :3] for k in ("v0", "v1", "v2")])
            c.set_medium(sigma_t=0.3, albedo=(0.9, 0.8, 0.7), g=0.3, box=(tuple(v.min(axis=0)), tuple(v.max(axis=0))))
        if cut:
            c.set_alpha_cutoff(cutoff, max_layers=max_layers)
        try:
            out.append(render(c, cam, FRAMES))
        finally:
            c.set_medium(None)
    return out


def pair(r):
    return r["output"], r["moments"]


@pytest.mark.parametrize("mis,fog", [(0, False), (1, False), (1, True), (0, True)])
def test_a_hole_is_an_absent_triangle(ctx, mis, fog):
    cut, dropped = holes_vs_dropped(ctx, HOLES, do_mis=mis, fog=fog)
    assert cut["alpha"]["path_passes"] > 0 and (cut["alpha"]["shadow_passes"] > 0) == (mis == 1)
    assert cut["alpha"]["path_exhausted"] == 0 and cut["alpha"]["shadow_exhausted"] == 0
    assert dropped["alpha"]["present"] == 0
    tile_means_within(pair(cut), pair(dropped), FRAMES, 3.0, "holes against dropped triangles, do_mis %d fog %d:" % (mis, fog))


def test_light_through_the_holes_reaches_the_floor(ctx):
    """the floor on the camera's side of the fence sees the lights only through it: brighter than behind an opaque fence, darker than
    without one, by more than 3 combined standard errors each way"""
    checker = A.checker(1)[0] < 0.5
    cam = layout.make_camera(FW, FH)
    sc, cutoff = A.fence_scene(1.0 - checker[None])
    prepare(ctx, sc, FW, FH, moments=True)
    opaque = render(ctx, cam, FRAMES)
    ctx.set_alpha_cutoff(cutoff)
    holes = render(ctx, cam, FRAMES)
    assert holes["alpha"]["shadow_passes"] > 0
    bare, _ = A.fence_scene(drop=np.ones((1, 8, 8), bool))
    prepare(ctx, bare, FW, FH, moments=True)
    none = render(ctx, cam, FRAMES)
    o, d = ctx.debug_center_rays(cam)
    t = ctx.debug_intersect(o, d)[0]
    p = o + t[:, None] * d
    floor = ((t > 0) & (np.abs(p[:, 1]) < 1e-3) & (p[:, 2] > 0.45) & (p[:, 2] < 0.95) & (np.abs(p[:, 0]) < 0.95)).reshape(FH, FW)
    assert floor.sum() > 100

    def stats(r):
        m = r["moments"].astype(np.float64)
        assert np.all(m[..., 2] == FRAMES)
        return m[..., 0][floor].mean(), (np.maximum(m[..., 1] - m[..., 0] ** 2, 0.0) / FRAMES)[floor].sum() / floor.sum() ** 2
    (mo, vo), (mh, vh), (mn, vn) = stats(opaque), stats(holes), stats(none)
    print("floor in front of the fence: opaque %.5f, holes %.5f, none %.5f; se %.5f %.5f" % (mo, mh, mn, np.sqrt(vo + vh), np.sqrt(vh + vn)))
    assert mh - mo > 3.0 * np.sqrt(vo + vh) and mn - mh > 3.0 * np.sqrt(vh + vn)


# ---- 4. layers ---------------------------------------------------------------------------------------------------------------------
def test_layers(ctx):
    everything = np.ones((2, 8, 8), bool)
    cut1, free = holes_vs_dropped(ctx, everything, zs=(0.4, 0.3), max_layers=1)
    assert cut1["alpha"]["max_layers"] == 1 and cut1["alpha"]["path_exhausted"] > 0
    assert not same(cut1["output"], free["output"])
    cut, free = holes_vs_dropped(ctx, everything, zs=(0.4, 0.3))
    assert cut["alpha"]["max_layers"] == 4 and cut["alpha"]["path_exhausted"] == 0 and cut["alpha"]["shadow_exhausted"] == 0
    assert cut["alpha"]["path_passes"] > 0 and cut["alpha"]["shadow_passes"] > 0
    tile_means_within(pair(cut), pair(free), FRAMES, 3.0, "two all-hole fences against none:")


# ---- 5. far from the origin --------------------------------------------------------------------------------------------------------
def test_far_from_the_origin(ctx):
    """at 200 units one ulp of a coordinate is 15 PT_EPS: a step of PT_EPS would leave the ray on the triangle it is passing"""
    cut, dropped = holes_vs_dropped(ctx, HOLES, offset=(200.0, 200.0, 200.0))
    assert cut["alpha"]["path_passes"] > 0 and cut["alpha"]["shadow_passes"] > 0
    assert cut["alpha"]["path_exhausted"] == 0 and cut["alpha"]["shadow_exhausted"] == 0
    tile_means_within(pair(cut), pair(dropped), FRAMES, 3.0, "holes against dropped triangles at (200, 200, 200):")


# ---- 6. one result through every route ---------------------------------------------------------------------------------------------
def checker_fence():
    return A.fence_scene(A.checker(2), z=(0.4, 0.3))


def test_one_result_through_every_route(ctx):
    W, H, frames = 64, 48, 4
    sc, cutoff = checker_fence()
    cam = layout.make_camera(W, H)
    prepare(ctx, sc, W, H, moments=True)
    ctx.set_alpha_cutoff(cutoff)
    base = render(ctx, cam, frames)
    assert base["alpha"]["path_passes"] > 0 and base["alpha"]["shadow_passes"] > 0
    for k in range(2):                                                      # the list order varies from run to run; no result does
        again = render(ctx, cam, frames)
        same_render(again, base, "dispatch %d" % (k + 2))
        assert again["alpha"] == base["alpha"]
    for fpb in (1, frames):
        ctx.set_options(frames_per_batch=fpb)
        same_render(render(ctx, cam, frames), base, "frames_per_batch %d" % fpb)
    ctx.set_options(frames_per_batch=0)
    ctx.set_aovs(*ALL)
    same_render(render(ctx, cam, frames), base, "planes on")
    ctx.set_aovs()
    # one adaptive round in which every pixel is active against plain frames of the same count
    ctx.dispatch(at(cam, 0), 8)
    want = ctx.read_output(), ctx.read_moments()
    ctx.dispatch_adaptive(at(cam, 0), 1, threshold=1e-9, neighbourhood=0, min_frames=8, max_frames=64, step=8)
    assert same(ctx.read_output(), want[0]) and same(ctx.read_moments(), want[1])
    ctx.set_moments(False)
    # two loopback contexts against one device
    with native.MultiContext([0, 0], loopback=True) as m:
        m.upload_scene(sc)
        m.resize(W, H)
        m.set_options(max_bounces=8, do_mis=1)
        assert err(m.set_alpha_cutoff, cutoff[:-1]) == -1 and err(m.set_alpha_cutoff, cutoff, max_layers=33) == -1
        assert m.alpha_status().present == 0
        m.set_alpha_cutoff(cutoff)
        m.reset_stats()
        m.dispatch(at(cam, 0), frames)
        got = m.read_output()
        st = m.alpha_status().as_dict()
        for i in range(2):
            one = native.AlphaStatus()
            assert m.L.ptmi_alpha_status(m.L.ptmi_multi_context(m.h, i), native.ctypes.byref(one)) == 0 and one.present == 1 and one.n_cutout == 2
    assert same(got, base["output"])
    assert st == base["alpha"]                                              # the devices' counters add up to the one device's
    ctx.set_alpha_cutoff(None)


# ---- 7. reprojection ---------------------------------------------------------------------------------------------------------------
def test_reprojection_sees_the_surface_behind_a_hole(ctx):
    """from == to: every pixel finds its own history, also where the centre ray passes a hole. A pixel's samples are jittered over
    its footprint, so a pixel that straddles a hole's rim would hold a mean depth of both surfaces and fail any depth test that tells
    them apart. The view is therefore laid out so that no pixel straddles one: a pinhole camera on the fence's axis, one unit in front
    of it, whose field of view and aspect put every cell edge on a pixel boundary, in the box without its furniture (whose silhouettes
    are depth steps of their own). A cell is 12 x 8 pixels, not square: the diagonal its two triangles share then passes through no
    pixel centre (it would through eight of an 8 x 8 cell's, and a centre ray exactly on a shared edge can slip between the triangles).
    The fence is 1 away, what shows through it up to 2.4."""
    W, H = 96, 48
    cell_h = 2.0015 / 8
    half_h = 3 * cell_h                                                     # six rows of cells fill the 48 rows of pixels at distance 1
    sc, cutoff = A.fence_scene(A.checker(1), furniture=False)
    cam = layout.make_camera(W, H, position=(0.0, 4 * cell_h, 1.4), fov=2.0 * np.arctan(half_h), aspect=1.0 / half_h, aperture=0.0)
    prepare(ctx, sc, W, H, aovs=("normal",), moments=True)
    ctx.set_alpha_cutoff(cutoff)
    ctx.dispatch(at(cam, 0), 4)
    assert np.isfinite(ctx.read_output()).all()
    depth = ctx.read_aov("normal")[..., 3]
    assert (depth < 1.3).sum() > W * H // 4 and (depth > 1.5).sum() > W * H // 4      # the fence's cells, and what its holes show
    ctx.reproject(cam, cam, depth_tolerance=0.2, match_ids=1)
    st = ctx.reproject_status().as_dict()
    print("with the table:", st)
    assert st["disoccluded"] == 0 and st["missed"] == 0 and st["carried"] == W * H
    # without the resolve loop the centre rays stop at the fence, and the pixels that show what is behind it are disoccluded
    ctx.set_alpha_cutoff(None)
    ctx.reproject(cam, cam, depth_tolerance=0.2, match_ids=1)
    raw = ctx.reproject_status().as_dict()
    print("without it:", raw)
    assert raw["disoccluded"] > W * H // 4
    ctx.set_aovs()
    ctx.set_moments(False)


# ---- 8. lifetime and refusals ------------------------------------------------------------------------------------------------------
def test_errors_keep_the_table_and_the_life_cycle(ctx):
    W, H, frames = 64, 48, 2
    fresh = native.Context(0)
    try:
        assert err(fresh.set_alpha_cutoff, np.zeros(3, np.float32)) == -1                  # no scene
        assert err(fresh.set_alpha_cutoff, None) == -1
        assert fresh.alpha_status().as_dict() == dict(present=0, n_materials=0, n_cutout=0, max_layers=0, path_passes=0,
                                                      path_exhausted=0, shadow_passes=0, shadow_exhausted=0)
    finally:
        fresh.close()
    sc, cutoff = checker_fence()
    cam = layout.make_camera(W, H)
    prepare(ctx, sc, W, H)
    opaque = render(ctx, cam, frames)
    ctx.set_alpha_cutoff(None)                                              # nothing to remove: fine
    ctx.set_alpha_cutoff(cutoff, max_layers=3)
    was = ctx.alpha_status().as_dict()
    assert (was["present"], was["n_materials"], was["n_cutout"], was["max_layers"]) == (1, len(sc.mats), 2, 3)
    base = render(ctx, cam, frames)
    assert not same(base["output"], opaque["output"])
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        t = cutoff.copy()
        t[0] = bad
        assert err(ctx.set_alpha_cutoff, t) == -1, bad
    assert err(ctx.set_alpha_cutoff, cutoff[:-1]) == -1 and err(ctx.set_alpha_cutoff, np.append(cutoff, 0)) == -1
    assert err(ctx.set_alpha_cutoff, cutoff, max_layers=33) == -1
    for r in ((1, 0, 0), (0, 0, 1)):
        assert err(ctx.set_alpha_cutoff, cutoff, reserved=r) == -1
    assert err(ctx.set_alpha_cutoff, None, reserved=(0, 1, 0)) == -1        # a removal checks its params too
    after = render(ctx, cam, frames)
    assert dict(after["alpha"]) == dict(base["alpha"]) and after["alpha"]["max_layers"] == 3
    same_render(after, base, "after the refused calls")
    # ptmi_upload_atlas and ptmi_update_materials leave the table alone, and renders still use it
    a = sc.atlas
    ctx._ck(ctx._c.upload_atlas(ctx.h, native._p(a), a.shape[1], a.shape[0], native.ATLAS_RGBA16F))
    assert ctx.alpha_status().present == 1
    mats = sc.mats.copy()
    mats["base_color"][0] = (0.2, 0.3, 0.9)
    ctx.update_materials(0, mats)
    st = ctx.alpha_status().as_dict()
    assert (st["present"], st["n_cutout"], st["max_layers"]) == (1, 2, 3)
    edited = render(ctx, cam, frames)
    assert edited["alpha"]["path_passes"] > 0 and edited["alpha"]["shadow_passes"] > 0 and not same(edited["output"], base["output"])
    # max_layers 32 is accepted, a zero-length table removes it, and an upload removes it
    ctx.set_alpha_cutoff(cutoff, max_layers=32)
    assert ctx.alpha_status().max_layers == 32
    ctx.set_alpha_cutoff(cutoff, n_materials=0)
    assert ctx.alpha_status().present == 0
    ctx.set_alpha_cutoff(cutoff)
    assert ctx.alpha_status().present == 1
    ctx.upload_scene(sc)
    assert ctx.alpha_status().as_dict()["present"] == 0 and ctx.alpha_status().n_cutout == 0
    same_render(render(ctx, cam, frames), opaque, "after the upload")
