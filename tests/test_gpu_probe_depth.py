"""Probe visibility on the GPU (include/ptmi.h ptmi_set_probe_depth, ptmi_probe_visibility) against
tests/probe_depth_ref.py and the CPU oracle, bit for bit. The depth plane folds the first hit of every probe path, and the first ray of
a probe path is the model's (tests/probe_ref.py rays, pinned by tests/test_gpu_probes.py), so a probe dispatch is pinned per sample by
Oracle.intersect on those rays.

  1. per sample, cornell and feature_box: the plane after every one-frame dispatch; radiance, moments and statistics as with the switch off
  2. frames: three in one call equal three calls; first_frame = 5 continues a written plane; unlisted texels keep a sentinel
  3. batching: 48, 64, 80 and 256 listed texels, one frame per batch and automatic sizing
  4. a cutout fence: the plane of the scene with the cut triangles removed
  5. fog: the plane keeps its bits under a homogeneous medium
  6. ptmi_probe_visibility against the model on written planes: N = 4, 8, 16, 64, every m and s, value edges, the border
  7. off means off: the goldens, a bake, a probe dispatch after the switch went off again; first-hit planes still refuse a probe dispatch
  8. every refusal leaves the plane, the output, the statistics and the probes alone

Every case fails without the feature: the binding has no such calls."""
import numpy as np
import pytest

import probe_depth_ref as pdr
import probe_ref
from ptmi import native, probes as host_probes
from test_golden import HERE, load, same
from test_gpu_parity import assert_same_floats
from test_gpu_probes import ATLASES, RBOUNCES, RFRAMES, err, interior_probes, sentinel, setup as probe_setup
from test_probe_host import atlas_probes

pytestmark = pytest.mark.gpu

f32 = np.float32
E_INVALID, E_STATE = -1, -4
MAXD = f32(1.0)             # of the first hits of the per-sample probes about half lie beyond it (checked below, on the CPU, per frame)


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the switch, probes and options it sets never reach the session's shared context"""
    with native.Context(0) as c:
        yield c
        c.set_probe_depth(None)


def setup(c, sc, W, H, **kw):
    c.set_probe_depth(None)
    probe_setup(c, sc, W, H, **kw)


def depth_sentinel(W, H):
    return sentinel(W, H) * f32(0.25) + f32(3)


def counts(st):
    return (st.paths, st.frames, st.dispatches, st.segments, st.shadow_rays, st.shadow_traced)


# ---- 1. per sample -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 8, 8), (8, 8, 4)], ids=lambda s: "%dx%d_N%d" % s)
@pytest.mark.parametrize("name", ["cornell", "feature_box"])
def test_plane_per_sample(ctx, oracle, scene_factory, name, shape):
    W, H, N = shape
    sc = scene_factory(name)
    rec = interior_probes(sc, W, H, N, disabled=(1,))             # two tiles, one probe on; four tiles, three on
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_probes(rec, N)
    keep = sentinel(W, H)

    def run(check=None):
        ctx.write_output(keep)
        ctx.reset_stats()
        res = []
        for f in range(RFRAMES):
            ctx.dispatch_probes(1, first_frame=f)
            res.append((ctx.read_output(), ctx.read_moments()))
            if check:
                check(f)
        return res, counts(ctx.stats())

    off, st_off = run()
    ctx.set_probe_depth(MAXD)
    assert ctx.get_probe_depth() == MAXD and not ctx.read_probe_depth().any()      # made zeroed
    model = [depth_sentinel(W, H)]
    ctx.write_probe_depth(model[0])
    seen = dict(miss=0, clamped=0, kept=0)

    def check(f):
        model[0], t, tri, lst = pdr.fold_rays(oracle, sc, rec, N, model[0], MAXD, f)
        hit = tri != pdr.MISS
        assert (~hit).any() and (hit & (t > MAXD)).any() and (hit & (t < MAXD)).any(), "frame %d: misses, clamped and unclamped hits" % f
        seen["miss"] += int((~hit).sum()); seen["clamped"] += int((hit & (t > MAXD)).sum()); seen["kept"] += int((hit & (t < MAXD)).sum())
        got = ctx.read_probe_depth()
        assert_same_floats(got, model[0], "%s, the depth plane after frame %d" % (name, f))      # every texel, the unlisted ones too

    on, st_on = run(check)
    print("first hits over %d frames: %s" % (RFRAMES, seen))
    for f in range(RFRAMES):
        assert same(on[f][0], off[f][0]) and same(on[f][1], off[f][1]), "frame %d: radiance and moments with the switch on" % f
    assert st_on == st_off
    lst = probe_ref.texel_list(rec, N, W, H)
    got = ctx.read_probe_depth().reshape(-1, 4)[lst]
    assert (got[:, 0] > 0).all() and (got[:, 0] <= MAXD * f32(1.000001)).all() and (got[:, 2] >= 0).all() and (got[:, 2] <= 1).all() and not got[:, 3].any()
    assert (got[:, 2] < 1).any() and (got[:, 2] == 1).any()


# ---- 2. frames -----------------------------------------------------------------------------------------------------------------------
def test_frames_in_one_call_equal_calls_and_a_plane_continues(ctx, oracle, scene_factory):
    W, H, N = 16, 8, 4                                            # eight tiles, six probes, one of them off
    sc = scene_factory("cornell")
    rec = interior_probes(sc, W, H, N, disabled=(2,))[:6]
    setup(ctx, sc, W, H, max_bounces=RBOUNCES)
    ctx.upload_probes(rec, N)
    ctx.set_probe_depth(MAXD)
    keep = depth_sentinel(W, H)
    lst = probe_ref.texel_list(rec, N, W, H).astype(np.int64)
    assert len(lst) == 5 * N * N
    rest = np.setdiff1d(np.arange(W * H), lst)

    def run(calls):
        ctx.write_probe_depth(keep)
        for f0, k in calls:
            ctx.dispatch_probes(k, first_frame=f0)
        return ctx.read_probe_depth()

    whole = run([(0, 3)])
    assert same(whole.reshape(-1, 4)[rest], keep.reshape(-1, 4)[rest])
    assert not same(whole.reshape(-1, 4)[lst], keep.reshape(-1, 4)[lst])
    for calls in ([(0, 1), (1, 1), (2, 1)], [(0, 2), (2, 1)]):
        assert same(run(calls), whole), calls
    model = keep
    for f in range(3):
        model = pdr.fold_rays(oracle, sc, rec, N, model, MAXD, f)[0]
    assert_same_floats(whole, model, "three frames")
    # a plane restored from elsewhere goes on from frame 5
    rs = np.random.RandomState(3)
    cached = rs.uniform(0.1, 1.0, (H, W, 4)).astype(f32)
    ctx.write_probe_depth(cached)
    ctx.dispatch_probes(2, first_frame=5)
    want = pdr.fold_rays(oracle, sc, rec, N, pdr.fold_rays(oracle, sc, rec, N, cached, MAXD, 5)[0], MAXD, 6)[0]
    got = ctx.read_probe_depth()
    assert_same_floats(got, want, "frames 5 and 6 onto a written plane")
    assert same(got.reshape(-1, 4)[rest], cached.reshape(-1, 4)[rest]) and not same(got, cached)


# ---- 3. batching ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enabled", [3, 4, 5, 16])
def test_batch_sizes_give_one_plane(ctx, scene_factory, enabled):
    W, H, N = 32, 8, 4                                            # sixteen tiles in two rows: 48, 64, 80 and 256 listed texels
    sc = scene_factory("cornell")
    on = np.zeros(16, bool)
    on[(np.arange(enabled) * 5) % 16] = True
    rec = interior_probes(sc, W, H, N, disabled=np.flatnonzero(~on))
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_probes(rec, N)
    ctx.set_probe_depth(MAXD)
    assert ctx.probe_status().texels == enabled * N * N
    keep = depth_sentinel(W, H)

    def run(calls, **opt):
        ctx.set_options(**opt)
        ctx.write_probe_depth(keep)
        ctx.write_output(sentinel(W, H))
        for f0, k in calls:
            ctx.dispatch_probes(k, first_frame=f0)
        return ctx.read_probe_depth(), ctx.read_output(), ctx.read_moments(), ctx.stats().frames_per_batch_used

    whole = run([(0, 4)], frames_per_batch=0)
    assert whole[3] == 4
    one = run([(0, 4)], frames_per_batch=1)
    assert one[3] == 1
    for got in (one, run([(0, 4)], frames_per_batch=3), run([(f, 1) for f in range(4)], frames_per_batch=0)):
        assert same(got[0], whole[0]) and same(got[1], whole[1]) and same(got[2], whole[2])
    ctx.set_options(frames_per_batch=0)


# ---- 4. alpha ------------------------------------------------------------------------------------------------------------------------
def test_depth_is_that_of_the_first_present_surface(ctx):
    """a fence with holes between the probe and the back of the room: under the cutoff table the plane is the plane of the scene whose
    hole triangles are gone"""
    from test_gpu_alpha import prepare
    from test_gpu_alpha_per_sample import scene_set
    cut, cutoff, n_fences, ghost, hole = scene_set("stripes")     # one fence at z = 0.4
    W = H = N = 8
    rec = atlas_probes(W, H, N)
    rec["position"][0] = (0.13, 0.93, 0.81)                       # in front of the fence, inside the room
    far = f32(1.5)

    def run(table, edit=None):
        ctx.set_probe_depth(None)
        prepare(ctx, cut, W, H, max_bounces=RBOUNCES)
        ctx.upload_bake_surface(None)
        if edit is not None:
            ctx.update_triangles(0, edit)
        ctx.set_alpha_cutoff(table)
        ctx.upload_probes(rec, N)
        ctx.set_probe_depth(far)
        ctx.reset_stats()
        ctx.dispatch_probes(2)
        return ctx.read_probe_depth(), ctx.alpha_status().path_passes

    try:
        under_table, passes = run(cutoff)
        removed, none = run(None, ghost.tris)
        solid, _ = run(None)
    finally:
        ctx.set_alpha_cutoff(None)
        ctx.set_probe_depth(None)
    assert hole.any() and passes > 0 and none == 0
    assert_same_floats(under_table, removed, "the plane under the table against the plane without the hole triangles")
    deeper = under_table[..., 0] > solid[..., 0]
    assert deeper.any() and (under_table[..., 0] >= solid[..., 0]).all()          # a hole only ever lets a ray go further


# ---- 5. fog --------------------------------------------------------------------------------------------------------------------------
def test_fog_does_not_shorten_the_depth(ctx, scene_factory):
    W, H, N = 16, 8, 8
    sc = scene_factory("cornell")
    rec = interior_probes(sc, W, H, N)
    setup(ctx, sc, W, H, max_bounces=RBOUNCES)
    ctx.upload_probes(rec, N)
    ctx.set_probe_depth(MAXD)

    def run():
        ctx.write_output(np.zeros((H, W, 4), f32))
        ctx.dispatch_probes(3)
        return ctx.read_probe_depth(), ctx.read_output()

    clear, clear_rgb = run()
    try:
        ctx.set_medium(2.5, albedo=0.8, g=0.3, box=((-2.0, -1.0, -2.0), (2.0, 3.0, 2.0)))
        fog, fog_rgb = run()
    finally:
        ctx.set_medium(None)
    assert not same(fog_rgb, clear_rgb)                           # the fog is there
    assert_same_floats(fog, clear, "the depth plane under a homogeneous medium")
    assert clear[..., 0].max() > f32(0.99) * MAXD and clear[..., 0].min() < f32(0.9) * MAXD


# ---- 6. the reduction ----------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-42, 1.4e-45, 1.17549435e-38, float(MAXD), float(MAXD) * float(MAXD), 1.0], f32)


def written_plane(W, H, N, n, disabled, scale=1.0):
    rs = np.random.RandomState(W * 137 + N)
    plane = (rs.uniform(0, 4, (H, W, 4)) * scale).astype(f32)
    flat = plane.reshape(-1)
    at = rs.choice(flat.size, flat.size // 6, replace=False)
    flat[at] = SPECIALS[rs.randint(0, len(SPECIALS), len(at))]
    return plane, atlas_probes(W, H, N, disabled)[:n]


def sizes_of(N):
    return sorted({2, 4, 16, N} & {k for k in (2, 4, 8, 16) if k <= N})


@pytest.mark.parametrize("atlas", ATLASES, ids=lambda a: "N%d" % a[2])
def test_visibility_matches_the_model(ctx, atlas):
    W, H, N, n, disabled = atlas                                  # N = 4: 16 probes; 8: 8; 16: 5 (no multiple of four); 64: 1
    plane, rec = written_plane(W, H, N, n, disabled)
    ctx.set_probe_depth(None)
    ctx.resize(W, H)
    ctx.upload_probes(rec, N)
    ctx.set_probe_depth(MAXD)
    ctx.write_probe_depth(plane)
    out = sentinel(W, H)
    ctx.write_output(out)
    on = [i for i in range(n) if i not in disabled]
    for m in sizes_of(N):
        for s in (0, 1, 6):
            got = ctx.probe_visibility(m, s)
            want = pdr.visibility(plane, rec, N, m, s)
            assert got.shape == (n, m, m, 4)
            assert_same_floats(got, want, "visibility, N = %d, m = %d, s = %d" % (N, m, s))
            assert not got[list(disabled)].any() and (got[on][..., 3] == 1).all() and np.isfinite(got).all()
        bordered = ctx.probe_visibility(m, 6, border=True)
        assert bordered.shape == (n, m + 2, m + 2, 4)
        assert same(bordered, host_probes.add_border(ctx.probe_visibility(m, 6), m)), "the border, m = %d" % m
        assert not bordered[list(disabled)].any()
    assert same(ctx.read_probe_depth(), plane) and same(ctx.read_output(), out)


@pytest.mark.parametrize("atlas", [ATLASES[1], ATLASES[3]], ids=lambda a: "N%d" % a[2])
def test_visibility_of_a_plane_whose_products_are_denormal(ctx, atlas):
    """values below 2e-38 under the sharpest lobe: every product wgt * D is a denormal or zero, the three sums stay denormal, and the
    quotient by the normal weight sum comes back to the values' size"""
    W, H, N, n, disabled = atlas
    plane, rec = written_plane(W, H, N, n, disabled, scale=5e-39)
    plane = np.minimum(plane, f32(2e-38))                         # (the specials too)
    wgt = pdr.weights(N, min(N, 16), 6)
    with np.errstate(all="ignore"):
        prod = wgt * f32(2e-38)
    assert (prod < f32(1.17549435e-38)).all() and (prod > 0).any()   # the plane's largest value under the largest weight
    ctx.set_probe_depth(None)
    ctx.resize(W, H)
    ctx.upload_probes(rec, N)
    ctx.set_probe_depth(MAXD)
    ctx.write_probe_depth(plane)
    for m in (2, min(N, 16)):
        got = ctx.probe_visibility(m, 6)
        assert_same_floats(got, pdr.visibility(plane, rec, N, m, 6), "denormal products, N = %d, m = %d" % (N, m))
        assert np.isfinite(got).all()


# ---- 7. off means off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_64x48_4spp_mis", "cornell_64x64_4spp_b4_nomis"])
def test_goldens_keep_their_bits(ctx, name):
    z, sc, cam = load(HERE + "/golden/" + name + ".npz")
    W, H, frames = int(cam["width"]), int(cam["height"]), int(z["frames"])
    setup(ctx, sc, W, H, max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
    for state in ("on", "dispatched", "off"):
        if state == "on":
            ctx.set_probe_depth(MAXD)
        elif state == "dispatched":
            ctx.upload_probes(interior_probes(sc, W, H, 16, disabled=(2,)), 16)
            ctx.dispatch_probes(2)
            assert ctx.read_probe_depth().any()
            ctx.reset_stats()
        else:
            ctx.set_probe_depth(None)
        depth = ctx.read_probe_depth() if state != "off" else None
        cam["frame_index"] = 0
        ctx.dispatch(cam, frames)
        out, st = ctx.read_output(), ctx.stats()
        assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"]), state
        assert same(out, z["image"]), state
        if depth is not None:
            assert same(ctx.read_probe_depth(), depth)            # a camera's dispatch folds nothing into it
        ctx.reset_stats()
    ctx.upload_probes(None)


def test_a_bake_keeps_its_bits(ctx, scene_factory):
    from test_gpu_bake import holes, scene_surface
    W, H = 16, 16
    sc = scene_factory("cornell")
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_bake_surface(scene_surface(sc, W, H, holes(W, H)))
    keep = sentinel(W, H)

    def bake():
        ctx.write_output(keep)
        ctx.reset_stats()
        ctx.dispatch_bake(2)
        return ctx.read_output(), ctx.read_moments(), counts(ctx.stats())

    want = bake()
    ctx.set_probe_depth(MAXD)
    plane = depth_sentinel(W, H)
    ctx.write_probe_depth(plane)
    got = bake()
    assert same(got[0], want[0]) and same(got[1], want[1]) and got[2] == want[2]
    assert same(ctx.read_probe_depth(), plane)
    ctx.upload_bake_surface(None)


def test_a_probe_dispatch_after_the_switch_went_off(ctx, scene_factory):
    W, H, N = 16, 8, 4
    sc = scene_factory("cornell")
    rec = interior_probes(sc, W, H, N, disabled=(3,))
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_probes(rec, N)
    keep = sentinel(W, H)

    def run(**opt):
        ctx.set_options(**opt)
        ctx.write_output(keep)
        ctx.reset_stats()
        ctx.dispatch_probes(4)
        return ctx.read_output(), ctx.read_moments(), counts(ctx.stats())

    want = run(frames_per_batch=0)
    ctx.set_probe_depth(MAXD)
    on = run(frames_per_batch=0)
    ctx.set_aovs("normal")                                        # first-hit planes refuse a probe dispatch, whatever the switch says
    assert err(ctx.dispatch_probes, 1) == E_INVALID
    ctx.set_aovs()
    ctx.set_probe_depth(None)
    assert ctx.get_probe_depth() is None and not ctx.probe_depth_device_ptr()
    for got in (on, run(frames_per_batch=0), run(frames_per_batch=1)):
        assert same(got[0], want[0]) and same(got[1], want[1]) and got[2] == want[2]
    ctx.set_options(frames_per_batch=0)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
SETS = ("max_nan", "max_inf", "max_zero", "max_negative", "reserved_0", "reserved_1", "reserved_2")
PLANES = ("read_size", "write_size", "write_size_0")
REDUCTIONS = ("m1", "m3", "m32", "m_above_tile", "s7", "border2", "reserved", "size", "size_0", "size_of_the_other_border")
OFF = ("off", "no_probes", "resized")


@pytest.mark.parametrize("case", SETS + PLANES + REDUCTIONS + OFF)
def test_a_refusal_changes_nothing(ctx, scene_factory, case):
    sc = scene_factory("cornell")
    W, H, N = 24, 16, 8                                           # 3 x 2 tiles, six probes
    rec = interior_probes(sc, W, H, N, disabled=(4,))
    setup(ctx, sc, W, H, moments=True, max_bounces=RBOUNCES)
    ctx.upload_probes(rec, N)
    ctx.set_probe_depth(MAXD)
    keep = sentinel(W, H)

    def run():
        ctx.write_output(keep)
        ctx.write_probe_depth(depth_sentinel(W, H))
        ctx.dispatch_probes(2)
        return ctx.read_output(), ctx.read_moments(), ctx.read_probe_depth()

    want = run()
    vis = ctx.probe_visibility(4, 6, border=True)
    status, st = ctx.probe_status().as_dict(), counts(ctx.stats())
    if case in SETS:
        if case.startswith("max_"):
            bad = dict(max_nan=np.nan, max_inf=np.inf, max_zero=0.0, max_negative=-1.0)[case]
            assert err(ctx.set_probe_depth, bad) == E_INVALID
        else:
            r = [0, 0, 0]
            r[int(case[-1])] = 1
            assert err(ctx.set_probe_depth, 2.0, reserved=tuple(r)) == E_INVALID
    elif case == "read_size":
        assert err(ctx.read_probe_depth, n_floats=W * H * 4 - 4) == E_INVALID and err(ctx.read_probe_depth, n_floats=0) == E_INVALID
    elif case.startswith("write_size"):
        n = 0 if case.endswith("_0") else W * H * 4 + 4
        assert err(ctx.write_probe_depth, np.zeros((H + 1, W, 4), f32), n_floats=n) == E_INVALID
    elif case in REDUCTIONS:
        kw = dict(m1=dict(m=1), m3=dict(m=3), m32=dict(m=32), m_above_tile=dict(m=16), s7=dict(m=4, sharpness_log2=7),
                  border2=dict(m=4, border=2), reserved=dict(m=4, reserved=1), size=dict(m=4, n_floats=6 * 16 * 4 - 4),
                  size_0=dict(m=4, n_floats=0), size_of_the_other_border=dict(m=4, border=1, n_floats=6 * 16 * 4))[case]
        assert err(ctx.probe_visibility, **kw) == E_INVALID
    elif case == "off":
        ctx.set_probe_depth(None)
        assert err(ctx.read_probe_depth) == E_STATE and err(ctx.write_probe_depth, want[2]) == E_STATE
        assert err(ctx.probe_visibility, 4) == E_STATE and not ctx.probe_depth_device_ptr()
        ctx.set_probe_depth(MAXD)
        assert not ctx.read_probe_depth().any()                   # off and on again: a fresh plane
        ctx.write_probe_depth(want[2])
    elif case == "no_probes":
        ctx.upload_probes(None)
        assert err(ctx.probe_visibility, 4, n_floats=0) == E_INVALID
        ctx.upload_probes(rec, N)
    elif case == "resized":
        ctx.resize(W, H)                                          # as the moments plane: a resize gives a fresh plane, the switch stays
        assert ctx.get_probe_depth() == MAXD and not ctx.read_probe_depth().any() and ctx.probe_status().present == 1
        ctx.write_probe_depth(want[2])
        ctx.write_output(want[0])
    assert ctx.get_probe_depth() == MAXD and ctx.probe_depth_device_ptr()
    assert same(ctx.read_probe_depth(), want[2]) and same(ctx.read_output(), want[0])
    if case != "resized":
        assert same(ctx.read_moments(), want[1])
    assert ctx.probe_status().as_dict() == status and counts(ctx.stats()) == st
    assert same(ctx.probe_visibility(4, 6, border=True), vis)
    got = run()
    assert all(same(g, w) for g, w in zip(got, want))
