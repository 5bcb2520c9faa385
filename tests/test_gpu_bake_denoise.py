"""The lightmap filter on the GPU (include/ptmi.h ptmi_bake_denoise, ptmi_bake_denoised_device_ptr, ptmi_write_moments; DESIGN.md
§26) against tests/bake_denoise_ref.py, within the camera filter's bound for the same two transcendental functions
(tests/test_gpu_denoise.py close_to_ref), and bit for bit wherever the arithmetic is exact.

  1. matches the model on real bakes: a 70 x 37 surface built by hand, iterations 1, 5 and 7, chosen and default parameters
  2. uncovered texels are never read
  3. no bleed between charts that touch in the atlas
  4. a NaN and a firefly stay where they are
  5. the gutter fill composes with the filter
  6. quality and back-off: the host test's scene, sizes, frame counts and bars
  7. nothing else moves: the inputs, ptmi_bake_dilate, a bake and a camera golden keep their bits
  8. life cycle and refusals
  9. ptmi_write_moments: round trip, and a bake resumed in another context

Every case fails without the feature: the binding has no such calls."""
import ctypes

import numpy as np
import pytest

import bake_denoise_ref as bdr
import bake_ref
from ptmi import layout, native, scenes
from test_bake_denoise_host import (BACKOFF, K, QFRAMES, QH, QTRUTH, QW, bits, chart, holes, quality_measures, quality_surface,
                                    two_chart_planes, two_charts, within_chart_constants)
from test_golden import HERE, load, same
from test_gpu_bake import err, sentinel, setup
from test_gpu_denoise import close_to_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
E_INVALID, E_STATE = -1, -4
MW, MH = 70, 37                                     # partial workgroups in x and y, two workgroups across


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the surface, planes and options it sets never reach the session's shared context"""
    with native.Context(0) as c:
        yield c


def hand_surface():
    """MW x MH records on the Cornell box's shell: the floor from the map's corner (0, 0), the back wall three texels of gutter to
    its right with holes()-style gaps, the +x wall above them, and one texel of the -x wall on its own"""
    X, Y, Z = scenes._ROOM_X, scenes._ROOM_Y, scenes._ROOM_Z
    tex = np.zeros((MH, MW), layout.BAKE_TEXEL)
    chart(tex, 0, 0, 30, 20, (-X, 0, -Z), (2 * X / 30, 0, 0), (0, 0, 2 * Z / 20), (0, 1, 0))
    chart(tex, 33, 2, 35, 18, (-X, 0, -Z), (2 * X / 35, 0, 0), (0, Y / 18, 0), (0, 0, 2))
    gaps = ~holes(MW, MH)
    gaps[:, :33] = False
    gaps[20:] = False
    tex["covered"][gaps] = 0
    chart(tex, 4, 24, 50, 12, (X, 0, -Z), (0, 0, 2 * Z / 50), (0, Y / 12, 0), (-0.5, 0, 0))
    chart(tex, 67, 30, 1, 1, (-X, 0.7, 0.1), (0, 0, 0.05), (0, 0.05, 0), (1, 0, 0))
    return tex


def baked(ctx, sc, tex, frames=(3, 3)):
    """the context after a bake of `tex` with the moments plane on, in calls of `frames` frames: (output, moments) read back"""
    H, W = tex.shape
    setup(ctx, sc, W, H, moments=True)
    ctx.upload_bake_surface(tex)
    first = 0
    for n in frames:
        ctx.dispatch_bake(n, first_frame=first)
        first += n
    return ctx.read_output(), ctx.read_moments()


def synthetic(ctx, tex, rad, mom):
    H, W = tex.shape
    ctx.set_aovs()
    ctx.set_moments(True)
    ctx.resize(W, H)
    ctx.upload_bake_surface(tex)
    ctx.write_output(rad)
    ctx.write_moments(mom)


def device_plane(ptr, H, W):
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros((H, W, 4), f32)
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0              # device to host
    return out


# ---- 1. the model --------------------------------------------------------------------------------------------------------------------
PARAMS = (dict(), dict(phi_color=1.5, phi_normal=8.0, phi_position=2.5))


@pytest.mark.parametrize("name", ["cornell", "cornell_spheres"])
def test_matches_the_model(ctx, scene_factory, name):
    tex = hand_surface()
    cov = tex["covered"] != 0
    assert cov[0, 0] and cov[25, 10] and not cov[:20, 30:33].any() and 0 < cov[2:20, 33:68].sum() < 18 * 35
    assert cov[30, 67] and cov[29:32, 66:69].sum() == 1
    rad, mom = baked(ctx, scene_factory(name), tex)
    assert (mom[cov][:, 2] == 6).all() and rad[cov][:, :3].max() > 0.05 and np.isfinite(rad[cov]).all()
    for it in (1, 5, 7):
        for kw in PARAMS:
            got = ctx.bake_denoise(iterations=it, **kw)
            want = bdr.denoise(tex, rad, mom, iterations=it, **kw)
            close_to_ref(got[..., :3], want[..., :3])
            assert np.array_equal(bits(got[..., 3]), bits(want[..., 3])), (it, kw)
            assert (got[cov][:, 3] == 1).all() and not got[~cov].any()
    # the filter did something, and the isolated texel kept its value
    assert np.abs(got[cov][:, :3] - rad[cov][:, :3]).max() > 1e-3
    assert np.array_equal(bits(got[30, 67, :3]), bits(rad[30, 67, :3]))
    # iterations = 0 is the default, 5
    assert np.array_equal(bits(ctx.bake_denoise()), bits(ctx.bake_denoise(iterations=5)))


# ---- 2. uncovered texels -------------------------------------------------------------------------------------------------------------
def test_uncovered_texels_are_never_read(ctx, scene_factory):
    tex = hand_surface()
    cov = tex["covered"] != 0
    rad, mom = baked(ctx, scene_factory("cornell"), tex)
    rad[~cov], mom[~cov] = 0, 0
    ctx.write_output(rad)
    ctx.write_moments(mom)
    want = ctx.bake_denoise(dilate=2)
    assert np.isfinite(want).all() and (want[..., 3] == 2).any()
    for junk in (np.nan, 1e30):
        r, m = rad.copy(), mom.copy()
        r[~cov], m[~cov] = junk, junk
        ctx.write_output(r)
        ctx.write_moments(m)
        assert np.array_equal(bits(ctx.bake_denoise(dilate=2)), bits(want)), junk


# ---- 3. no bleed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_no_bleed_between_charts_that_touch_in_the_atlas(ctx, case):
    tex, right = two_charts(case)
    rad, mom = two_chart_planes(right)
    synthetic(ctx, tex, rad, mom)
    out = ctx.bake_denoise(iterations=3)
    within_chart_constants(out, tex, right)
    close_to_ref(out, bdr.denoise(tex, rad, mom, iterations=3))


# ---- 4. a firefly and a NaN ----------------------------------------------------------------------------------------------------------
def test_a_nan_and_a_firefly_stay_where_they_are(ctx, scene_factory):
    tex = hand_surface()
    rad, mom = baked(ctx, scene_factory("cornell"), tex)
    rad[5, 7, :3], rad[12, 41, :3] = np.nan, 1e30
    assert tex["covered"][5, 7] and tex["covered"][12, 41]
    ctx.write_output(rad)
    out = ctx.bake_denoise()
    bad = ~np.isfinite(out[..., :3]).all(axis=-1)
    assert bad.sum() == 1 and bad[5, 7] and out[12, 41, 0] > 1e29
    close_to_ref(out, bdr.denoise(tex, rad, mom))


# ---- 5. the gutter fill --------------------------------------------------------------------------------------------------------------
def test_dilate_composes(ctx, scene_factory):
    tex = hand_surface()
    cov = tex["covered"] != 0
    baked(ctx, scene_factory("cornell"), tex)
    plain = ctx.bake_denoise(iterations=2)
    for k in (1, 4, 100):
        got = ctx.bake_denoise(iterations=2, dilate=k)
        want = bake_ref.dilate(plain, cov, k)
        assert np.array_equal(bits(got), bits(want)), k
    assert (got[..., 3] != 0).all() and (got[..., 3] == 2).sum() == (~cov).sum()


# ---- 6. quality and back-off ---------------------------------------------------------------------------------------------------------
def test_cleans_a_cornell_bake_and_backs_off(ctx, scene_factory):
    tex = quality_surface()
    assert tex.shape == (QH, QW)
    sc = scene_factory("cornell")
    raw4, _ = baked(ctx, sc, tex, (QFRAMES,))
    den4 = ctx.bake_denoise()
    raw1024, _ = baked(ctx, sc, tex, (QTRUTH,))
    den1024 = ctx.bake_denoise()
    assert np.isfinite(den4).all() and np.isfinite(den1024).all()
    k, backoff = quality_measures(tex, raw4, den4, raw1024, den1024)
    print("K = mse(raw) / mse(filtered) = %.3f, back-off ratio = %.4f" % (k, backoff))
    assert k > K and backoff < BACKOFF, (k, backoff)


# ---- 7. nothing else moves -----------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(ctx, scene_factory):
    z, sc, cam = load(HERE + "/golden/cornell_64x48_4spp_mis.npz")
    W, H, frames = int(cam["width"]), int(cam["height"]), int(z["frames"])
    tex = np.zeros((H, W), layout.BAKE_TEXEL)
    chart(tex, 0, 0, W, H, (-0.9, 0, -0.9), (1.8 / W, 0, 0), (0, 0, 1.8 / H), (0, 1, 0))       # on the floor
    tex["covered"] = holes(W, H)

    def bake():
        setup(ctx, sc, W, H, moments=True, max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
        ctx.upload_bake_surface(tex)
        ctx.write_output(sentinel(W, H))
        ctx.dispatch_bake(3)
        return ctx.read_output(), ctx.read_moments(), ctx.bake_dilate(3)

    out0, mom0, dil0 = bake()
    ctx.bake_denoise(dilate=2)
    ctx.bake_denoise(iterations=1, dst=False)
    assert same(ctx.read_output(), out0) and same(ctx.read_moments(), mom0) and same(ctx.bake_dilate(3), dil0)
    out1, mom1, dil1 = bake()                                   # the same bake, in the context that has denoised
    assert same(out1, out0) and same(mom1, mom0) and same(dil1, dil0)
    ctx.bake_denoise()
    ctx.set_moments(False)
    ctx.reset_stats()
    cam["frame_index"] = 0
    ctx.dispatch(cam, frames)                                   # a camera golden, the surface still in place
    st = ctx.stats()
    assert st.segments == int(z["segments"]) and st.shadow_rays == int(z["shadow_rays"])
    assert same(ctx.read_output(), z["image"])


# ---- 8. life cycle and refusals ------------------------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(scene_factory):
    L = native.load()
    with native.Context(0) as c:
        assert c.bake_denoised_device_ptr() is None
        assert err(c.bake_denoise) == E_STATE                   # no output buffer
        assert err(c.write_moments, np.zeros(4, f32)) == E_STATE
        W, H = 24, 16
        tex, right = two_charts("a", W, H)
        rad, mom = two_chart_planes(right)
        c.resize(W, H)
        assert err(c.bake_denoise) == E_INVALID                 # no surface
        c.upload_bake_surface(tex)
        assert err(c.bake_denoise) == E_STATE                   # the moments plane is off
        assert err(c.write_moments, mom) == E_STATE
        c.set_moments(True)
        c.write_output(rad)
        c.write_moments(mom)
        for kw in (dict(phi_color=-1.0), dict(phi_normal=float("nan")), dict(phi_position=float("inf")), dict(iterations=11),
                   dict(reserved=(0, 0, 1)), dict(n_floats=W * H * 4 - 4), dict(n_floats=W * H * 4 + 1)):
            assert err(c.bake_denoise, **kw) == E_INVALID, kw
        assert err(c.write_moments, mom, n_floats=W * H * 4 - 1) == E_INVALID
        assert L.ptmi_write_moments(c.h, None, W * H * 4) == E_INVALID
        assert c.bake_denoised_device_ptr() is None             # nothing was made by a refused call
        assert same(c.read_moments(), mom) and same(c.read_output(), rad)
        # queued, then read through the device pointer
        assert c.bake_denoise(dilate=1, dst=False) is None
        c.synchronize()
        p = c.bake_denoised_device_ptr()
        assert p
        on_device = device_plane(p, H, W)
        copied = c.bake_denoise(dilate=1)
        assert c.bake_denoised_device_ptr() == p and same(on_device, copied) and same(device_plane(p, H, W), copied)
        # a refused call leaves the plane as it is
        assert err(c.bake_denoise, iterations=11) == E_INVALID and err(c.bake_denoise, phi_color=-2.0) == E_INVALID
        c.set_moments(False)
        assert err(c.bake_denoise) == E_STATE
        assert same(device_plane(p, H, W), copied)
        c.set_moments(True)
        c.write_moments(mom)
        # without a surface
        c.upload_bake_surface(None)
        assert err(c.bake_denoise) == E_INVALID
        assert same(device_plane(p, H, W), copied)
        # a resize forgets the plane
        c.upload_bake_surface(tex)
        c.resize(W, H)
        assert c.bake_denoised_device_ptr() is None
        c.write_output(rad)
        c.write_moments(mom)
        assert same(c.bake_denoise(dilate=1), copied) and c.bake_denoised_device_ptr()
        c.resize(W + 1, H)                                      # another size: the surface goes too
        assert c.bake_denoised_device_ptr() is None and err(c.bake_denoise) == E_INVALID


# ---- 9. ptmi_write_moments -----------------------------------------------------------------------------------------------------------
def test_write_moments_round_trips_and_resumes_a_bake(ctx, scene_factory):
    sc = scene_factory("cornell")
    tex = hand_surface()
    whole, whole_m = baked(ctx, sc, tex, (4,))
    half, half_m = baked(ctx, sc, tex, (2,))
    rs = np.random.RandomState(11)
    junk = rs.uniform(-3, 3, whole_m.shape).astype(f32)
    junk[0, 0] = (np.nan, np.inf, -0.0, 1e-42)
    ctx.write_moments(junk)
    assert np.array_equal(bits(ctx.read_moments()), bits(junk))
    with native.Context(0) as c:
        setup(c, sc, MW, MH, moments=True)
        c.upload_bake_surface(tex)
        c.write_output(half)
        c.write_moments(half_m)
        c.dispatch_bake(2, first_frame=2)
        assert same(c.read_output(), whole) and same(c.read_moments(), whole_m)
