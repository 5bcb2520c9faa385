"""Lightmap baking on the GPU (include/ptmi.h ptmi_upload_bake_surface, ptmi_dispatch_bake, ptmi_bake_dilate) against
tests/bake_ref.py and the CPU oracle, bit for bit. The oracle renders from a pinhole only, which is all it needs to: the model's bake
ray (org, raw) of a texel is that texel's pixel of the oracle camera with position = org, forward = raw, fov = 0, aperture = 0
(tests/test_bake_host.py), so whole bakes are pinned per sample through Oracle.trace_paths with one camera per texel.

  1. off means off: the goldens keep their bits with a surface uploaded, and again after a bake has run on the context
  2. ptmi_debug_bake_rays against the model: origin, direction, RNG state; zeros for an uncovered texel
  3. bakes per sample, cornell and feature_box, texels on the scenes' own surfaces: the output and the moments after every one-frame
     bake; uncovered texels keep what was there
  4. the dispatch paths agree: n frames = n bakes, frames_per_batch 1 = 0, for 0, 1, 63, 64, 65 and all texels covered
  5. a bake under a sky, half the texels above the box
  6. the gutter fill against the model
  7. every refusal leaves the status and the next bake's bits alone

Every case fails without the feature: the binding has no such calls."""
import numpy as np
import pytest

import adaptive_ref
import bake_ref
import env_ref
import projection_ref as pr
from ptmi import layout, native, scenes
from test_bake_host import ray_surface, texel_grid
from test_golden import HERE, load, same
from test_gpu_parity import assert_same_floats

pytestmark = pytest.mark.gpu

f32 = np.float32
E_INVALID = -1
MISS = 0xFFFFFFFF
RW, RH, RFRAMES, RBOUNCES = 16, 12, 3, 4            # the per-sample bakes
DW, DH = 70, 33                                     # the dispatch paths: neither a multiple of 64


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the surface, planes and options it sets never reach the session's shared context"""
    with native.Context(0) as c:
        yield c


def err(fn, *a, **kw):
    with pytest.raises(native.PtmiError) as e:
        fn(*a, **kw)
    return e.value.code


def setup(c, sc, W, H, aovs=(), moments=False, **opt):
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=0, cull=1,
             traversal=0, overlap=2, perf_mode=0, leaves=0, timing=0)
    o.update(opt)
    c.set_options(**o)
    c.set_motion(False)
    c.set_projections(False)
    c.upload_scene(sc)
    c.upload_environment(None)
    c.set_medium(None)
    c.set_aovs(*aovs)
    c.set_moments(moments)
    c.resize(W, H)
    c.upload_bake_surface(None)
    c.reset_stats()


def scene_surface(sc, W, H, covered=None):
    """(H, W) texel records on the scene's own triangles: texel i lies inside triangle (37 i + 5) mod n, at barycentrics that move
    with i, and carries the triangle's interpolated normal. covered: (H, W) bool (None: every texel)."""
    t = sc.tris
    i = np.arange(W * H)
    k = (37 * i + 5) % len(t)
    b0, b1 = 0.2 + 0.05 * (i % 5), 0.15 + 0.04 * (i % 7)
    b2 = 1.0 - b0 - b1
    rec = np.zeros(W * H, layout.BAKE_TEXEL)
    for field, (a, b, c) in (("position", ("v0", "v1", "v2")), ("normal", ("n0", "n1", "n2"))):
        rec[field] = b0[:, None] * t[a][k].astype(np.float64) + b1[:, None] * t[b][k] + b2[:, None] * t[c][k]
    rec["covered"] = 1 if covered is None else np.asarray(covered).ravel()
    return rec.reshape(H, W)


def holes(W, H):
    """the coverage of the per-sample bakes: texels with (7 x + 3 y) % 4 == 0 are uncovered, so no wave is all covered or all empty"""
    ys, xs = np.divmod(np.arange(W * H), W)
    return ((7 * xs + 3 * ys) % 4 != 0).reshape(H, W)


def sentinel(W, H):
    s = np.empty((H, W, 4), f32)
    s[...] = np.arange(W * H * 4, dtype=f32).reshape(H, W, 4) * f32(0.5) - f32(7)
    return s


def oracle_radiance(oracle, sc, tex, frame, extras=None, bias=bake_ref.DEFAULT_BIAS):
    """per covered texel (ascending), the radiance of the oracle's path (x, y, frame) under the texel's own fov = 0 camera; (n, 3), its
    segment counts, the paths whose sky lookups came within the band of a texel border (with extras), and the model's rays"""
    H, W = tex.shape
    lst = bake_ref.covered_list(tex)
    ys, xs = np.divmod(lst, np.uint32(W))
    m = bake_ref.rays(oracle, tex, xs, ys, np.full(len(lst), frame, np.uint32), bias)
    cams = pr.fov0_cameras(layout.make_camera(W, H, aperture=0.0), m["org"], m["raw"])
    rad, seg, aside = np.zeros((len(lst), 3), f32), np.zeros(len(lst), np.uint32), np.zeros(len(lst), bool)
    for i in range(len(lst)):
        a = (sc, cams[i:i + 1], xs[i:i + 1], ys[i:i + 1], [frame])
        if extras is None:
            r, s = oracle.trace_paths(*a, max_bounces=RBOUNCES, do_mis=1, threads=1)
        else:
            r, s, border = oracle.trace_paths_ext(*a, extras, max_bounces=RBOUNCES, do_mis=1, threads=1)
            aside[i] = border[0] < env_ref.BORDER_BAND
        rad[i], seg[i] = r[0], s[0]
    return rad, seg, aside, m


# ---- 1. off means off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_64x48_4spp_mis", "cornell_64x64_4spp_b4_nomis"])
def test_goldens_keep_their_bits(ctx, name):
    z, sc, cam = load(HERE + "/golden/" + name + ".npz")
    W, H, frames = int(cam["width"]), int(cam["height"]), int(z["frames"])
    setup(ctx, sc, W, H, max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
    ctx.upload_bake_surface(scene_surface(sc, W, H, holes(W, H)))
    assert ctx.bake_status().as_dict() == dict(present=1, width=W, height=H, covered=int(holes(W, H).sum()))
    for after_a_bake in (False, True):
        if after_a_bake:
            ctx.dispatch_bake(2)
            assert not same(ctx.read_output(), z["image"])
            ctx.reset_stats()
        cam["frame_index"] = 0
        ctx.dispatch(cam, frames)
        out, st = ctx.read_output(), ctx.stats()
        assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"]), after_a_bake
        assert same(out, z["image"]), after_a_bake


# ---- 2. rays -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [0.0, None, 0.25], ids=["bias0", "default", "bias0.25"])
@pytest.mark.parametrize("size", [(7, 5), (70, 33)], ids=lambda s: "%dx%d" % s)
def test_rays_match_the_model(ctx, oracle, size, bias):
    W, H = size
    tex = ray_surface(W, H)
    ctx.resize(W, H)
    ctx.upload_bake_surface(tex)
    xs, ys, fr = texel_grid(W, H, (0, 1, 1000))
    m = bake_ref.rays(oracle, tex, xs, ys, fr, bake_ref.DEFAULT_BIAS if bias is None else bias)
    o, d, rng = ctx.debug_bake_rays(xs, ys, fr, bias=bias)
    assert_same_floats(o, m["org"], "origins")
    assert_same_floats(d, m["d"], "directions")
    assert np.array_equal(rng, m["rng"])
    empty = ~m["covered"]
    assert empty.sum() == 3 * ((W * H) // 9) and not o[empty].any() and not d[empty].any() and not rng[empty].any()
    assert np.isfinite(o[~empty]).all() and np.abs((d[~empty].astype(np.float64) ** 2).sum(axis=1) - 1).max() < 1e-6
    # both branches of constructTBN were taken among the covered texels
    nx = np.abs(pr.normalize3(tex[ys.astype(int), xs.astype(int)]["normal"][~empty])[:, 0])
    assert (nx > 0.9).any() and (nx <= 0.9).any()
    assert err(ctx.debug_bake_rays, [W], [0], [0]) == E_INVALID and err(ctx.debug_bake_rays, [0], [H], [0]) == E_INVALID


# ---- 3. bakes, per sample ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "feature_box"])
def test_bakes_per_sample(ctx, oracle, scene_factory, name):
    sc = scene_factory(name)
    tex = scene_surface(sc, RW, RH, holes(RW, RH))
    lst = bake_ref.covered_list(tex).astype(np.int64)
    assert 0 < len(lst) < RW * RH
    setup(ctx, sc, RW, RH, moments=True, max_bounces=RBOUNCES)
    # something in every entry of both planes: a camera's frames in the moments plane, a sentinel in the output buffer
    ctx.dispatch(layout.make_camera(RW, RH), 2)
    mom0 = ctx.read_moments().reshape(-1, 4)
    assert (mom0[:, 2] == 2).all()
    keep = sentinel(RW, RH)
    ctx.write_output(keep)
    ctx.upload_bake_surface(tex)
    rgb, mom = np.zeros((len(lst), 3), f32), np.zeros((len(lst), 4), f32)
    for f in range(RFRAMES):
        rad, _, _, _ = oracle_radiance(oracle, sc, tex, f)
        rgb, mom = adaptive_ref.fold_listed(rgb, mom, rad, np.full(len(lst), f, np.uint32))
        ctx.dispatch_bake(1, first_frame=f)
        out, gm = ctx.read_output().reshape(-1, 4), ctx.read_moments().reshape(-1, 4)
        assert_same_floats(out[lst, :3], rgb, "%s, after frame %d" % (name, f))
        assert not out[lst, 3].any()
        assert_same_floats(gm[lst], mom, "moments after frame %d" % f)
        rest = np.setdiff1d(np.arange(RW * RH), lst)
        assert same(out[rest], keep.reshape(-1, 4)[rest]) and same(gm[rest], mom0[rest])
    assert np.isfinite(rgb).all() and rgb.max() > 0.05           # a lightmap, not a black frame
    st = ctx.stats()
    assert st.paths == 2 * RW * RH + RFRAMES * len(lst) and st.dispatches == 1 + RFRAMES


# ---- 4. the dispatch paths agree -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, DW * DH])
def test_dispatch_paths_agree(ctx, scene_factory, count):
    sc = scene_factory("cornell")
    cov = np.zeros(DW * DH, bool)
    cov[(np.arange(count) * 97) % (DW * DH)] = True              # 97 and 2310 share no factor: `count` different texels, scattered
    assert cov.sum() == count
    tex = scene_surface(sc, DW, DH, cov.reshape(DH, DW))
    n = 3
    setup(ctx, sc, DW, DH, moments=True, max_bounces=RBOUNCES)
    ctx.upload_bake_surface(tex)
    assert ctx.bake_status().covered == count
    keep = sentinel(DW, DH)

    def bake(calls, **opt):
        ctx.set_options(**opt)
        ctx.write_output(keep)
        for f0, k in calls:
            ctx.dispatch_bake(k, first_frame=f0)
        return ctx.read_output(), ctx.read_moments()

    whole, whole_m = bake([(0, n)], frames_per_batch=0)
    assert same(whole.reshape(-1, 4)[~cov], keep.reshape(-1, 4)[~cov])
    if count:
        assert not same(whole.reshape(-1, 4)[cov], keep.reshape(-1, 4)[cov]) and (whole_m.reshape(-1, 4)[cov, 2] == n).all()
    if count == DW * DH:
        assert whole[..., :3].max() > 0.05
    for calls, opt in (([(f, 1) for f in range(n)], dict(frames_per_batch=0)), ([(0, n)], dict(frames_per_batch=1)),
                       ([(0, 1), (1, n - 1)], dict(frames_per_batch=2))):
        got, got_m = bake(calls, **opt)
        assert same(got, whole) and same(got_m, whole_m), (calls, opt)
    ctx.set_options(frames_per_batch=0)
    before = ctx.stats().dispatches
    ctx.dispatch_bake(0)                                        # no frames: nothing happens
    assert same(ctx.read_output(), whole) and ctx.stats().dispatches == before


# ---- 5. under a sky ------------------------------------------------------------------------------------------------------------------
def test_bake_under_a_sky(ctx, oracle, scene_factory):
    sc = scene_factory("cornell")
    tex = scene_surface(sc, RW, RH)
    above = np.zeros((RH, RW), bool)
    above[1::2] = True                                          # every other row: just above the outer side of the ceiling, normal up
    ys, xs = np.nonzero(above)
    tex["position"][above] = np.stack([-0.8 + 0.1 * xs, np.full(len(xs), scenes._ROOM_Y + 0.01), -0.8 + 0.13 * ys], axis=1)
    tex["normal"][above] = (0.0, 1.0, 0.0)
    texels = scenes.sky(16, 8, "disc")
    c, prob, alias, wsum = native.env_table(texels)
    extras = oracle.extras(dict(texels=texels, c=c, prob=prob, alias=alias, sampled=int(wsum > 0), intensity=1.0))
    lst = bake_ref.covered_list(tex).astype(np.int64)
    assert len(lst) == RW * RH
    # the oracle's side first: what the bake must give, how many paths leave into the sky at once, how many are set aside
    rgb, mom, aside = np.zeros((len(lst), 3), f32), np.zeros((len(lst), 4), f32), np.zeros(len(lst), bool)
    for f in range(RFRAMES):
        rad, seg, a, m = oracle_radiance(oracle, sc, tex, f, extras)
        aside |= a
        rgb, mom = adaptive_ref.fold_listed(rgb, mom, rad, np.full(len(lst), f, np.uint32))
        if f == 0:
            _, tri, _, _, _ = oracle.intersect(sc, m["org"], m["d"])
            sky_first = (tri == MISS) & (seg == 1)
            assert ((tri == MISS) <= (seg == 1)).all()
            print("frame 0: %d of %d paths end in the sky on their first segment" % (sky_first.sum(), len(lst)))
            assert sky_first.sum() * 3 >= len(lst) and sky_first[above.ravel()[lst]].all()
    print("paths set aside for a sky lookup within the border band: %d of %d texels" % (aside.sum(), aside.size))
    assert aside.mean() < 0.25
    setup(ctx, sc, RW, RH, max_bounces=RBOUNCES)
    try:
        ctx.upload_environment(texels)
        ctx.upload_bake_surface(tex)
        for f in range(RFRAMES):
            ctx.dispatch_bake(1, first_frame=f)
        out = ctx.read_output().reshape(-1, 4)
    finally:
        ctx.upload_environment(None)
    assert_same_floats(out[~aside, :3], rgb[~aside], "a bake under a sky")
    assert out[above.ravel(), :3].max() > 0.05 and out[~above.ravel(), :3].max() > 0.05


# ---- 6. the gutter fill --------------------------------------------------------------------------------------------------------------
def coverage(kind, W, H):
    cov = np.zeros((H, W), bool)
    if kind == "corner":
        cov[H - 1, W - 1] = True
    elif kind == "checker":
        ys, xs = np.divmod(np.arange(W * H), W)
        cov = ((xs // 2 + ys // 3) % 3 == 0).reshape(H, W)      # blocks with gaps two and three texels wide
    elif kind == "full":
        cov[:] = True
    return cov


@pytest.mark.parametrize("kind", ["corner", "checker", "empty", "full"])
@pytest.mark.parametrize("size", [(1, 1), (7, 5), (70, 33)], ids=lambda s: "%dx%d" % s)
def test_dilate_matches_the_model(ctx, size, kind):
    W, H = size
    cov = coverage(kind, W, H)
    tex = np.zeros((H, W), layout.BAKE_TEXEL)
    tex["normal"], tex["covered"] = (0.0, 0.0, 1.0), cov
    ctx.resize(W, H)
    ctx.upload_bake_surface(tex)
    assert ctx.bake_status().covered == cov.sum()
    rs = np.random.RandomState(W * 131 + H)
    out = rs.uniform(-4, 4, (H, W, 4)).astype(f32)
    out[..., 3] = 5.0                                           # the state is not what the output buffer holds in w
    ctx.write_output(out)
    for passes in (0, 1, 3, 40):
        got = ctx.bake_dilate(passes)
        want = bake_ref.dilate(out, cov, passes)
        assert_same_floats(got, want, "%s %dx%d, %d passes" % (kind, W, H, passes))
    if kind in ("corner", "checker") and size == (7, 5):
        assert (want[..., 3] != 0).all() and (want[..., 3] == 2).any()   # 40 passes, more than the diameter: everything is filled
    assert same(ctx.read_output(), out)
    assert err(ctx.bake_dilate, 1, n_floats=W * H * 4 + 1) == E_INVALID and err(ctx.bake_dilate, 1, n_floats=0) == E_INVALID


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def bad_texels(tex, what):
    t = tex.copy()
    i = tuple(np.argwhere(t["covered"] != 0)[5])
    if what == "position_nan":
        t["position"][i] = (0.0, np.nan, 0.0)
    elif what == "position_inf":
        t["position"][i] = (np.inf, 0.0, 0.0)
    elif what == "normal_nan":
        t["normal"][i] = (np.nan, 1.0, 0.0)
    elif what == "normal_zero":
        t["normal"][i] = (0.0, -0.0, 0.0)
    elif what == "normal_underflows":
        t["normal"][i] = (1e-30, 0.0, 0.0)                       # its squared length is zero in float32
    return t


UPLOADS = ("position_nan", "position_inf", "normal_nan", "normal_zero", "normal_underflows", "wrong_width", "wrong_height")
BAKES = ("bias_negative", "bias_nan", "bias_inf", "reserved", "aov_on", "tile_rows", "tile_rows_end", "tile_parts")


@pytest.mark.parametrize("case", UPLOADS + BAKES + ("dilate_size", "no_surface"))
def test_a_refusal_changes_nothing(ctx, scene_factory, case):
    sc = scene_factory("cornell")
    W, H = 16, 12
    tex = scene_surface(sc, W, H, holes(W, H))
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_bake_surface(tex)
    keep = sentinel(W, H)

    def bake():
        ctx.write_output(keep)
        ctx.dispatch_bake(2)
        return ctx.read_output(), ctx.read_moments()

    want, want_m = bake()
    status, st = ctx.bake_status().as_dict(), ctx.stats()
    if case in UPLOADS:
        if case == "wrong_width":
            assert err(ctx.upload_bake_surface, tex, width=W + 1) == E_INVALID
        elif case == "wrong_height":
            assert err(ctx.upload_bake_surface, tex.reshape(W, H)) == E_INVALID
        else:
            assert err(ctx.upload_bake_surface, bad_texels(tex, case)) == E_INVALID
            uncovered = bad_texels(tex, case)                   # the same values in an uncovered texel are nobody's business ...
            uncovered["covered"][tuple(np.argwhere(tex["covered"] != 0)[5])] = 0
            ctx.upload_bake_surface(uncovered)
            assert ctx.bake_status().covered == status["covered"] - 1
            ctx.upload_bake_surface(tex)                        # ... and the surface is put back for what follows
    elif case == "dilate_size":
        assert err(ctx.bake_dilate, 1, n_floats=W * H * 4 - 4) == E_INVALID
    elif case == "no_surface":
        ctx.upload_bake_surface(None)
        assert ctx.bake_status().as_dict() == dict(present=0, width=0, height=0, covered=0)
        assert err(ctx.dispatch_bake, 1) == E_INVALID and err(ctx.bake_dilate, 1) == E_INVALID
        assert err(ctx.debug_bake_rays, [0], [0], [0]) == E_INVALID
        assert same(ctx.read_output(), want) and same(ctx.read_moments(), want_m)
        ctx.upload_bake_surface(tex)
        ctx.resize(W + 1, H)                                    # another size: the surface goes
        assert ctx.bake_status().present == 0
        ctx.resize(W, H)
        ctx.upload_bake_surface(tex)
        ctx.resize(W, H)                                        # the same size: it stays
    else:
        undo = lambda: None
        kw = {}
        if case == "aov_on":
            ctx.set_aovs("normal")
            undo = ctx.set_aovs
        elif case.startswith("tile"):
            ctx.set_options(**{"tile_rows": dict(tile_y0=1), "tile_rows_end": dict(tile_y1=H - 1), "tile_parts": dict(tile_parts=2, tile_strip=4)}[case])
            undo = lambda: ctx.set_options(tile_y0=0, tile_y1=0, tile_parts=0, tile_strip=0)
        else:
            kw = dict(bias_negative=dict(bias=-1e-6), bias_nan=dict(bias=np.nan), bias_inf=dict(bias=np.inf), reserved=dict(reserved=(0, 1)))[case]
        assert err(ctx.dispatch_bake, 1, first_frame=2, **kw) == E_INVALID
        if kw:
            assert err(ctx.debug_bake_rays, [1], [0], [0], **kw) == E_INVALID
        undo()
    if case != "no_surface":
        assert same(ctx.read_output(), want) and same(ctx.read_moments(), want_m)
    assert ctx.bake_status().as_dict() == status
    after = ctx.stats()
    assert (after.frames, after.paths, after.dispatches, after.segments) == (st.frames, st.paths, st.dispatches, st.segments)
    got, got_m = bake()
    assert same(got, want) and same(got_m, want_m)
