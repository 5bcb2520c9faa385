"""Light probes on the GPU (include/ptmi.h ptmi_upload_probes, ptmi_dispatch_probes, ptmi_probe_sh, ptmi_probe_irradiance; DESIGN.md
§23) against tests/probe_ref.py and the CPU oracle, bit for bit. The oracle renders from a pinhole only, which is all it needs to: the
model's probe ray (org, raw) of a texel is that texel's pixel of the oracle camera with position = org, forward = raw, fov = 0,
aperture = 0 (tests/test_probe_host.py), so whole probe dispatches are pinned per sample through Oracle.trace_paths with one camera per
texel.

  1. ptmi_debug_probe_rays against the model: origin, direction, RNG state; zeros for a disabled probe's tile
  2. probe dispatches per sample, cornell and feature_box: the output and the moments after every one-frame dispatch
  3. one case under a sky
  4. the counts: 48, 64, 80 and 256 listed texels and none; unlisted texels keep a sentinel; statistics; first_frame
  5. ptmi_probe_sh and ptmi_probe_irradiance against the model on written outputs: N = 4, 8, 16, 64, disabled probes interleaved,
     signed zeros, denormals and 2.5 among the values
  6. off means off: the goldens keep their bits with probes uploaded and removed; a bake keeps its bits after a probe dispatch
  7. every refusal leaves the output, the statistics and the probes alone

Every case fails without the feature: the binding has no such calls."""
import numpy as np
import pytest

import adaptive_ref
import env_ref
import probe_ref
import projection_ref as pr
from ptmi import layout, native, scenes
from test_golden import HERE, load, same
from test_gpu_parity import assert_same_floats
from test_probe_host import atlas_probes, texel_grid

pytestmark = pytest.mark.gpu

f32 = np.float32
E_INVALID = -1
RFRAMES, RBOUNCES = 3, 4                            # the per-sample dispatches


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the probes, planes and options it sets never reach the session's shared context"""
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
    c.upload_probes(None)
    c.reset_stats()


def interior_probes(sc, W, H, N, disabled=()):
    """one probe per tile at points inside the scene's bounds, none on a lattice plane of the scene"""
    v = np.concatenate([sc.tris[k] for k in ("v0", "v1", "v2")]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rec = atlas_probes(W, H, N, disabled)
    i = np.arange(len(rec))
    frac = np.stack([0.37 + 0.29 * (i % 2), 0.58 - 0.21 * (i % 3) / 2, 0.44 + 0.17 * ((i // 2) % 2)], axis=1)
    rec["position"] = lo + (hi - lo) * frac
    return rec


def sentinel(W, H):
    s = np.empty((H, W, 4), f32)
    s[...] = np.arange(W * H * 4, dtype=f32).reshape(H, W, 4) * f32(0.5) - f32(7)
    return s


def oracle_radiance(oracle, sc, rec, N, W, H, frame, extras=None):
    """per listed texel (ascending), the radiance of the oracle's path (x, y, frame) under the texel's own fov = 0 camera: (n, 3), the
    paths whose sky lookups came within the band of a texel border (with extras), and the list"""
    lst = probe_ref.texel_list(rec, N, W, H)
    ys, xs = np.divmod(lst, np.uint32(W))
    m = probe_ref.rays(oracle, rec, N, W, xs, ys, np.full(len(lst), frame, np.uint32))
    assert m["enabled"].all() and (m["raw"] != 0).all()
    cams = pr.fov0_cameras(layout.make_camera(W, H, aperture=0.0), m["org"], m["raw"])
    rad, aside = np.zeros((len(lst), 3), f32), np.zeros(len(lst), bool)
    for i in range(len(lst)):
        a = (sc, cams[i:i + 1], xs[i:i + 1], ys[i:i + 1], [frame])
        if extras is None:
            r, _ = oracle.trace_paths(*a, max_bounces=RBOUNCES, do_mis=1, threads=1)
        else:
            r, _, border = oracle.trace_paths_ext(*a, extras, max_bounces=RBOUNCES, do_mis=1, threads=1)
            aside[i] = border[0] < env_ref.BORDER_BAND
        rad[i] = r[0]
    return rad, aside, lst.astype(np.int64)


# ---- 1. rays -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 4, 4), (16, 8, 8), (64, 64, 64)], ids=lambda s: "%dx%d_N%d" % s)
def test_rays_match_the_model(ctx, oracle, shape):
    W, H, N = shape
    rec = atlas_probes(W, H, N, disabled=(1,) if W > N else ())
    ctx.resize(W, H)
    ctx.upload_probes(rec, N)
    xs, ys, fr = texel_grid(W, H, (0, 1, 7))
    m = probe_ref.rays(oracle, rec, N, W, xs, ys, fr)
    o, d, rng = ctx.debug_probe_rays(xs, ys, fr)
    assert_same_floats(o, m["org"], "origins")
    assert_same_floats(d, m["d"], "directions")
    assert np.array_equal(rng, m["rng"])
    off = ~m["enabled"]
    assert off.sum() == (3 * N * N if W > N else 0) and not o[off].any() and not d[off].any() and not rng[off].any()
    assert np.abs((d[~off].astype(np.float64) ** 2).sum(axis=1) - 1).max() < 1e-6 and (d[~off, 2] < 0).any() and (d[~off, 2] > 0).any()
    assert err(ctx.debug_probe_rays, [W], [0], [0]) == E_INVALID and err(ctx.debug_probe_rays, [0], [H], [0]) == E_INVALID
    if W == N:                                                    # a single tile: the same atlas again with its only probe off
        rec["enabled"] = 0
        ctx.upload_probes(rec, N)
        o, d, rng = ctx.debug_probe_rays(xs[:N * N], ys[:N * N], fr[:N * N])
        assert not o.any() and not d.any() and not rng.any()


def test_rays_of_tiles_past_the_last_probe_are_zeros(ctx, oracle):
    W, H, N = 16, 8, 4                                            # eight tiles, five probes
    rec = atlas_probes(W, H, N)[:5]
    ctx.resize(W, H)
    ctx.upload_probes(rec, N)
    xs, ys, fr = texel_grid(W, H, (2,))
    m = probe_ref.rays(oracle, rec, N, W, xs, ys, fr)
    o, d, rng = ctx.debug_probe_rays(xs, ys, fr)
    assert_same_floats(o, m["org"], "origins")
    assert_same_floats(d, m["d"], "directions")
    assert np.array_equal(rng, m["rng"]) and (~m["enabled"]).sum() == 3 * N * N
    assert ctx.probe_status().as_dict() == dict(present=1, tile=N, count=5, enabled=5, texels=5 * N * N)


# ---- 2. dispatches, per sample -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 8, 8), (8, 8, 4)], ids=lambda s: "%dx%d_N%d" % s)
@pytest.mark.parametrize("name", ["cornell", "feature_box"])
def test_probes_per_sample(ctx, oracle, scene_factory, name, shape):
    W, H, N = shape
    sc = scene_factory(name)
    rec = interior_probes(sc, W, H, N, disabled=(1,) if N == 4 else ())      # 8x8, N = 4: four tiles, three probes on
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.dispatch(layout.make_camera(W, H), 2)                     # something in every entry of both planes
    mom0 = ctx.read_moments().reshape(-1, 4)
    keep = sentinel(W, H)
    ctx.write_output(keep)
    ctx.upload_probes(rec, N)
    rgb = mom = None
    for f in range(RFRAMES):
        rad, _, lst = oracle_radiance(oracle, sc, rec, N, W, H, f)
        if f == 0:
            rgb, mom = np.zeros((len(lst), 3), f32), np.zeros((len(lst), 4), f32)
        rgb, mom = adaptive_ref.fold_listed(rgb, mom, rad, np.full(len(lst), f, np.uint32))
        ctx.dispatch_probes(1, first_frame=f)
        out, gm = ctx.read_output().reshape(-1, 4), ctx.read_moments().reshape(-1, 4)
        assert_same_floats(out[lst, :3], rgb, "%s, after frame %d" % (name, f))
        assert not out[lst, 3].any()
        assert_same_floats(gm[lst], mom, "moments after frame %d" % f)
        rest = np.setdiff1d(np.arange(W * H), lst)
        assert same(out[rest], keep.reshape(-1, 4)[rest]) and same(gm[rest], mom0[rest])
    assert len(lst) == int((rec["enabled"] != 0).sum()) * N * N
    assert np.isfinite(rgb).all() and rgb.max() > 0.05            # light arrives
    st = ctx.stats()
    assert st.paths == 2 * W * H + RFRAMES * len(lst) and st.dispatches == 1 + RFRAMES


# ---- 3. under a sky ------------------------------------------------------------------------------------------------------------------
def test_probes_under_a_sky(ctx, oracle, scene_factory):
    W, H, N = 16, 8, 8
    sc = scene_factory("cornell")
    rec = interior_probes(sc, W, H, N)
    rec["position"][1] = (0.13, scenes._ROOM_Y + 0.31, -0.07)     # the second probe stands above the box: its upper half sees the sky
    texels = scenes.sky(16, 8, "disc")
    c, prob, alias, wsum = native.env_table(texels)
    extras = oracle.extras(dict(texels=texels, c=c, prob=prob, alias=alias, sampled=int(wsum > 0), intensity=1.0))
    rgb = mom = aside = None
    for f in range(RFRAMES):
        rad, a, lst = oracle_radiance(oracle, sc, rec, N, W, H, f, extras)
        if f == 0:
            rgb, mom, aside = np.zeros((len(lst), 3), f32), np.zeros((len(lst), 4), f32), np.zeros(len(lst), bool)
        aside |= a
        rgb, mom = adaptive_ref.fold_listed(rgb, mom, rad, np.full(len(lst), f, np.uint32))
    print("paths set aside for a sky lookup within the border band: %d of %d texels" % (aside.sum(), aside.size))
    assert aside.mean() < 0.25
    setup(ctx, sc, W, H, max_bounces=RBOUNCES)
    try:
        ctx.upload_environment(texels)
        ctx.upload_probes(rec, N)
        for f in range(RFRAMES):
            ctx.dispatch_probes(1, first_frame=f)
        out = ctx.read_output().reshape(-1, 4)[lst]
    finally:
        ctx.upload_environment(None)
    assert_same_floats(out[~aside, :3], rgb[~aside], "probes under a sky")
    second = (lst % W) >= N
    assert out[second, :3].max() > 0.05 and out[~second, :3].max() > 0.05


# ---- 4. the counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enabled", [0, 3, 4, 5, 16])
def test_dispatch_counts(ctx, scene_factory, enabled):
    W, H, N = 32, 8, 4                                            # sixteen tiles in two rows
    sc = scene_factory("cornell")
    on = np.zeros(16, bool)
    on[(np.arange(enabled) * 5) % 16] = True                      # 5 and 16 share no factor: `enabled` different tiles, both rows
    rec = interior_probes(sc, W, H, N, disabled=np.flatnonzero(~on))
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_probes(rec, N)
    listed = enabled * N * N
    assert ctx.probe_status().as_dict() == dict(present=1, tile=N, count=16, enabled=enabled, texels=listed)
    lst = probe_ref.texel_list(rec, N, W, H)
    assert len(lst) == listed
    mask = np.zeros(W * H, bool)
    mask[lst] = True
    keep = sentinel(W, H)

    def run(calls, **opt):
        ctx.set_options(**opt)
        ctx.write_output(keep)
        for f0, k in calls:
            ctx.dispatch_probes(k, first_frame=f0)
        return ctx.read_output(), ctx.read_moments()

    ctx.reset_stats()
    whole, whole_m = run([(0, 4)], frames_per_batch=0)
    st = ctx.stats()
    assert (st.paths, st.frames, st.dispatches) == ((listed * 4, 4, 1) if enabled else (0, 0, 0))
    assert same(whole.reshape(-1, 4)[~mask], keep.reshape(-1, 4)[~mask])
    if enabled:
        assert not same(whole.reshape(-1, 4)[mask], keep.reshape(-1, 4)[mask]) and (whole_m.reshape(-1, 4)[mask, 2] == 4).all()
        assert not whole.reshape(-1, 4)[mask, 3].any()
    for calls, opt in (([(0, 2), (2, 2)], dict(frames_per_batch=0)), ([(0, 4)], dict(frames_per_batch=1)),
                       ([(f, 1) for f in range(4)], dict(frames_per_batch=3))):
        got, got_m = run(calls, **opt)
        assert same(got, whole) and same(got_m, whole_m), (calls, opt)
    ctx.set_options(frames_per_batch=0)
    before = ctx.stats().dispatches
    ctx.dispatch_probes(0)                                        # no frames: nothing happens
    assert same(ctx.read_output(), whole) and ctx.stats().dispatches == before


# ---- 5. the two reductions -----------------------------------------------------------------------------------------------------------
# (W, H, N, probes, disabled): N = 4 leaves 48 lanes idle and fills four workgroups of the SH kernel; N = 8 is exactly one round of a
# wave; N = 16 with its last tile unused; N = 64 alone. Neither kernel strides: a probe has a wave or a workgroup of its own.
ATLASES = [(32, 8, 4, 16, (1, 2, 7, 12)), (32, 16, 8, 8, (0, 5)), (48, 32, 16, 5, (3,)), (64, 64, 64, 1, ())]
SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-42, 1.4e-45, 2.5, -2.5, 1.17549435e-38], f32)


def written_atlas(W, H, N, n, disabled):
    rs = np.random.RandomState(W * 131 + N)
    out = rs.uniform(-4, 4, (H, W, 4)).astype(f32)
    flat = out.reshape(-1)
    at = rs.choice(flat.size, flat.size // 6, replace=False)
    flat[at] = SPECIALS[rs.randint(0, len(SPECIALS), len(at))]
    rec = atlas_probes(W, H, N, disabled)[:n]
    assert np.isfinite(out).all()
    return out, rec


@pytest.mark.parametrize("atlas", ATLASES, ids=lambda a: "N%d" % a[2])
def test_sh_matches_the_model(ctx, atlas):
    W, H, N, n, disabled = atlas
    out, rec = written_atlas(W, H, N, n, disabled)
    ctx.resize(W, H)
    ctx.upload_probes(rec, N)
    ctx.write_output(out)
    got = ctx.probe_sh()
    want = probe_ref.sh(out, rec, N)
    assert got.shape == (n, 9, 3)
    assert_same_floats(got, want, "SH9, N = %d" % N)
    assert not got[list(disabled)].any() and all(got[i].any() for i in range(n) if i not in disabled)
    assert same(ctx.read_output(), out)
    # a constant radiance of 1: c_00 = 2 sqrt(pi) within the rule's error, everything else near zero
    ctx.write_output(np.ones((H, W, 4), f32))
    const = ctx.probe_sh()[[i for i in range(n) if i not in disabled]]
    tol = {4: 1.5, 8: 0.09, 16: 0.021, 64: 0.0013}[N]
    assert np.abs(const[:, 0] - 2 * np.sqrt(np.pi)).max() < tol and np.abs(const[:, 1:]).max() < tol


@pytest.mark.parametrize("atlas", ATLASES, ids=lambda a: "N%d" % a[2])
def test_irradiance_matches_the_model(ctx, atlas):
    W, H, N, n, disabled = atlas
    out, rec = written_atlas(W, H, N, n, disabled)
    ctx.resize(W, H)
    ctx.upload_probes(rec, N)
    ctx.write_output(out)
    for m in sorted({2, min(N, 16), 16} & {k for k in (2, 4, 8, 16) if k <= N}):
        got = ctx.probe_irradiance(m)
        want = probe_ref.irradiance(out, rec, N, m)
        assert got.shape == (n, m, m, 4)
        assert_same_floats(got, want, "irradiance, N = %d, m = %d" % (N, m))
        assert not got[list(disabled)].any() and (np.delete(got, list(disabled), axis=0)[..., 3] == 1).all()
    assert same(ctx.read_output(), out)


def test_reductions_read_a_bound_output_in_place(ctx):
    """an output buffer the caller owns (ptmi_bind_output_device; here a second context's): the same bits as from the context's own,
    which holds other values meanwhile"""
    W, H, N, n, disabled = ATLASES[1]
    out, rec = written_atlas(W, H, N, n, disabled)
    ctx.resize(W, H)
    ctx.upload_probes(rec, N)
    ctx.write_output(sentinel(W, H))
    with native.Context(0) as owner:
        owner.resize(W, H)
        owner.write_output(out)
        ctx.bind_output_device(owner.output_device_ptr(), W * H * 16)
        try:
            sh, irr = ctx.probe_sh(), ctx.probe_irradiance(8)
        finally:
            ctx.bind_output_device(0, 0)
    assert_same_floats(sh, probe_ref.sh(out, rec, N), "SH9 of a bound buffer")
    assert_same_floats(irr, probe_ref.irradiance(out, rec, N, 8), "irradiance of a bound buffer")
    assert same(ctx.read_output(), sentinel(W, H))


# ---- 6. off means off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_64x48_4spp_mis", "cornell_64x64_4spp_b4_nomis"])
def test_goldens_keep_their_bits(ctx, name):
    z, sc, cam = load(HERE + "/golden/" + name + ".npz")
    W, H, frames = int(cam["width"]), int(cam["height"]), int(z["frames"])
    setup(ctx, sc, W, H, max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
    N = 16
    rec = interior_probes(sc, W, H, N, disabled=(2,))
    for state in ("uploaded", "dispatched", "removed"):
        if state == "uploaded":
            ctx.upload_probes(rec, N)
        elif state == "dispatched":
            ctx.dispatch_probes(2)
            assert not same(ctx.read_output(), z["image"])
            ctx.reset_stats()
        else:
            ctx.upload_probes(None)
            assert ctx.probe_status().as_dict() == dict(present=0, tile=0, count=0, enabled=0, texels=0)
        cam["frame_index"] = 0
        ctx.dispatch(cam, frames)
        out, st = ctx.read_output(), ctx.stats()
        assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"]), state
        assert same(out, z["image"]), state
        ctx.reset_stats()


def test_a_bake_keeps_its_bits_after_a_probe_dispatch(ctx, scene_factory):
    from test_gpu_bake import holes, scene_surface
    W, H, N = 16, 16, 8
    sc = scene_factory("cornell")
    tex = scene_surface(sc, W, H, holes(W, H))
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_bake_surface(tex)
    keep = sentinel(W, H)

    def bake():
        ctx.write_output(keep)
        ctx.dispatch_bake(2)
        return ctx.read_output(), ctx.read_moments(), ctx.bake_status().as_dict()

    want = bake()
    ctx.upload_probes(interior_probes(sc, W, H, N, disabled=(3,)), N)      # probes and a surface are independent state
    ctx.dispatch_probes(2)
    assert ctx.bake_status().as_dict() == want[2] and ctx.probe_status().enabled == 3
    got = bake()
    cov = holes(W, H)                                             # (the probes folded their own moments into the texels between)
    assert same(got[0], want[0]) and same(got[1][cov], want[1][cov]) and got[2] == want[2]
    ctx.upload_bake_surface(None)
    assert ctx.probe_status().enabled == 3                                  # ... in both directions
    ctx.upload_probes(None)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
UPLOADS = ("tile_2", "tile_3", "tile_12", "tile_128", "width", "height", "count_0", "count_7", "position_nan", "position_inf")
DISPATCHES = ("reserved_0", "reserved_1", "reserved_2", "aov_on", "tile_rows", "tile_rows_end", "tile_parts")
REDUCTIONS = ("sh_size", "sh_size_0", "irr_m1", "irr_m3", "irr_m32", "irr_m_above_tile", "irr_size", "rays_outside")


@pytest.mark.parametrize("case", UPLOADS + DISPATCHES + REDUCTIONS + ("no_probes",))
def test_a_refusal_changes_nothing(ctx, scene_factory, case):
    sc = scene_factory("cornell")
    W, H, N = (16, 24, 8) if case == "height" else (24, 16, 8)    # 3 x 2 or 2 x 3 tiles: room for six probes
    rec = interior_probes(sc, W, H, N, disabled=(4,))
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_probes(rec, N)
    keep = sentinel(W, H)

    def run():
        ctx.write_output(keep)
        ctx.dispatch_probes(2)
        return ctx.read_output(), ctx.read_moments()

    want, want_m = run()
    status, st = ctx.probe_status().as_dict(), ctx.stats()
    assert status == dict(present=1, tile=N, count=6, enabled=5, texels=5 * N * N)
    if case in UPLOADS:
        bad = rec.copy()
        if case.startswith("tile_"):
            assert err(ctx.upload_probes, rec[:1], int(case[5:])) == E_INVALID
        elif case in ("width", "height"):
            assert err(ctx.upload_probes, rec[:1], 16) == E_INVALID   # 24 is not a multiple of 16; the other side is
        elif case == "count_0":
            assert err(ctx.upload_probes, rec, N, count=0) == E_INVALID
        elif case == "count_7":
            assert err(ctx.upload_probes, np.concatenate([rec, rec[:1]]), N) == E_INVALID
        else:
            bad["position"][2] = (0.0, np.nan, 0.0) if case == "position_nan" else (np.inf, 0.0, 0.0)
            assert err(ctx.upload_probes, bad, N) == E_INVALID
            bad["enabled"][2] = 0                                 # the same values in a disabled probe are nobody's business ...
            ctx.upload_probes(bad, N)
            assert ctx.probe_status().enabled == 4
            ctx.upload_probes(rec, N)                             # ... and the probes are put back for what follows
    elif case in DISPATCHES:
        undo = lambda: None
        kw = {}
        if case == "aov_on":
            ctx.set_aovs("normal")
            undo = ctx.set_aovs
        elif case.startswith("tile"):
            ctx.set_options(**{"tile_rows": dict(tile_y0=1), "tile_rows_end": dict(tile_y1=H - 1), "tile_parts": dict(tile_parts=2, tile_strip=4)}[case])
            undo = lambda: ctx.set_options(tile_y0=0, tile_y1=0, tile_parts=0, tile_strip=0)
        else:
            r = [0, 0, 0]
            r[int(case[-1])] = 1
            kw = dict(reserved=tuple(r))
        assert err(ctx.dispatch_probes, 1, first_frame=2, **kw) == E_INVALID
        if kw:
            assert err(ctx.debug_probe_rays, [1], [0], [0], **kw) == E_INVALID
        undo()
    elif case == "sh_size":
        assert err(ctx.probe_sh, n_floats=6 * 27 + 1) == E_INVALID and err(ctx.probe_sh, n_floats=5 * 27) == E_INVALID
    elif case == "sh_size_0":
        assert err(ctx.probe_sh, n_floats=0) == E_INVALID
    elif case.startswith("irr_m"):
        m = dict(irr_m1=1, irr_m3=3, irr_m32=32, irr_m_above_tile=16)[case]
        assert err(ctx.probe_irradiance, m, n_floats=6 * m * m * 4) == E_INVALID
    elif case == "irr_size":
        assert err(ctx.probe_irradiance, 4, n_floats=6 * 16 * 4 - 4) == E_INVALID and err(ctx.probe_irradiance, 4, n_floats=0) == E_INVALID
    elif case == "rays_outside":
        assert err(ctx.debug_probe_rays, [W], [0], [0]) == E_INVALID and err(ctx.debug_probe_rays, [0], [H], [0]) == E_INVALID
    elif case == "no_probes":
        ctx.upload_probes(None)
        assert ctx.probe_status().as_dict() == dict(present=0, tile=0, count=0, enabled=0, texels=0)
        assert err(ctx.dispatch_probes, 1) == E_INVALID and err(ctx.debug_probe_rays, [0], [0], [0]) == E_INVALID
        assert err(ctx.probe_sh, n_floats=0) == E_INVALID and err(ctx.probe_irradiance, 2, n_floats=0) == E_INVALID
        assert same(ctx.read_output(), want) and same(ctx.read_moments(), want_m)
        ctx.upload_probes(rec, N)
        ctx.resize(W + N, H)                                      # another size: the probes go
        assert ctx.probe_status().present == 0
        ctx.resize(W, H)
        ctx.upload_probes(rec, N)
        ctx.resize(W, H)                                          # the same size: they stay
    if case != "no_probes":
        assert same(ctx.read_output(), want) and same(ctx.read_moments(), want_m)
    assert ctx.probe_status().as_dict() == status
    after = ctx.stats()
    assert (after.frames, after.paths, after.dispatches, after.segments) == (st.frames, st.paths, st.dispatches, st.segments)
    got, got_m = run()
    assert same(got, want) and same(got_m, want_m)
