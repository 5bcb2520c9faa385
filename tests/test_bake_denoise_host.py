"""The lightmap filter (include/ptmi.h ptmi_bake_denoise, ptmi_write_moments) without a GPU: the numpy model of
tests/bake_denoise_ref.py on hand-made surfaces and on oracle bakes of the Cornell box, and the ABI surface of the feature.

The helpers here (surfaces, the no-bleed cases, the quality surface and its measures) are what tests/test_gpu_bake_denoise.py runs on
the device too."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref
import bake_denoise_ref as bdr
import bake_ref
import projection_ref as pr
from oracle_lib import PtoOptions, _ptr
from ptmi import layout, native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = ("ptmi_bake_denoise", "ptmi_bake_denoised_device_ptr", "ptmi_write_moments")

# The model's filtered 4-frame bake of QW x QH texels on the Cornell box's floor and walls (quality_surface, default parameters) has
# 1 / K_MEASURED of the raw bake's MSE against the 1024-frame bake, and at 1024 frames the filter changes a covered texel by
# BACKOFF_MEASURED of what it changes at 4 frames (mean absolute change of rgb; both measured with this module's oracle_bake,
# test_model_cleans_a_cornell_bake_and_backs_off prints them). The bars are half the one and twice the other: half the reference's own
# margin. tests/test_gpu_bake_denoise.py uses the same bars.
K_MEASURED = 19.245
BACKOFF_MEASURED = 0.1013
K = K_MEASURED / 2
BACKOFF = BACKOFF_MEASURED * 2
QW = QH = 64
QFRAMES, QTRUTH = 4, 1024
QBOUNCES = 8


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- surfaces --------------------------------------------------------------------------------------------------------------------
def chart(tex, x0, y0, w, h, origin, du, dv, normal):
    """covers texels [x0, x0 + w) x [y0, y0 + h) of tex with the plane origin + (i + 0.5) du + (j + 0.5) dv"""
    i, j = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    pos = np.asarray(origin, np.float64) + i[..., None] * np.asarray(du, np.float64) + j[..., None] * np.asarray(dv, np.float64)
    tex["position"][y0:y0 + h, x0:x0 + w] = pos
    tex["normal"][y0:y0 + h, x0:x0 + w] = normal
    tex["covered"][y0:y0 + h, x0:x0 + w] = 1


def flat_surface(W, H, covered=None, spacing=0.01):
    """one plane z = 0 under the whole map, `spacing` between texels; covered: (H, W) bool (None: every texel)"""
    tex = np.zeros((H, W), layout.BAKE_TEXEL)
    chart(tex, 0, 0, W, H, (0, 0, 0), (spacing, 0, 0), (0, spacing, 0), (0, 0, 1))
    if covered is not None:
        tex["covered"] = covered
    return tex


def two_charts(case, W=24, H=16, spacing=0.01):
    """two charts that touch in the atlas at column W / 2, with no gutter: (a) the same plane and normal, the right chart 1.0 further
    along x; (b) parallel planes 0.5 apart. Returns the records and the mask of the right chart."""
    tex = np.zeros((H, W), layout.BAKE_TEXEL)
    h = W // 2
    chart(tex, 0, 0, h, H, (0, 0, 0), (spacing, 0, 0), (0, spacing, 0), (0, 0, 1))
    origin = dict(a=(h * spacing + 1.0, 0, 0), b=(h * spacing, 0, 0.5))[case]
    chart(tex, h, 0, W - h, H, origin, (spacing, 0, 0), (0, spacing, 0), (0, 0, 1))
    right = np.zeros((H, W), bool)
    right[:, h:] = True
    return tex, right


def two_chart_planes(right):
    """radiance 1 on the left chart and 5 on the right, variance of the mean 1 everywhere"""
    rad = np.zeros(right.shape + (4,), f32)
    rad[..., :3] = np.where(right, f32(5), f32(1))[..., None]
    return rad, moments_of(rad, 1.0)


def moments_of(rad, variance, frames=1):
    """a moments plane that gives every texel the luminance of rad as its mean and `variance` as the variance of its mean"""
    from denoise_ref import lum
    mom = np.zeros(rad.shape, f32)
    l = lum(rad[..., 0], rad[..., 1], rad[..., 2])
    mom[..., 0], mom[..., 1], mom[..., 2] = l, l * l + f32(variance) * f32(frames), frames
    return mom


def within_chart_constants(out, tex, right, tol=1e-5):
    cov = tex["covered"] != 0
    for mask, c in ((cov & ~right, 1.0), (cov & right, 5.0)):
        dev = np.abs(out[mask][:, :3].astype(np.float64) - c).max() / c
        assert dev <= tol, (c, dev)


def quality_surface():
    """QW x QH records on the Cornell box's floor, back wall and side walls: four charts of 28 x 28 texels, 4 texels of gutter between
    them and 2 to the border"""
    X, Y, Z = scenes._ROOM_X, scenes._ROOM_Y, scenes._ROOM_Z
    n = 28
    tex = np.zeros((QH, QW), layout.BAKE_TEXEL)
    chart(tex, 2, 2, n, n, (-X, 0, -Z), (2 * X / n, 0, 0), (0, 0, 2 * Z / n), (0, 1, 0))            # floor
    chart(tex, 34, 2, n, n, (-X, 0, -Z), (2 * X / n, 0, 0), (0, Y / n, 0), (0, 0, 1))                 # back wall
    chart(tex, 2, 34, n, n, (X, 0, -Z), (0, 0, 2 * Z / n), (0, Y / n, 0), (-1, 0, 0))                 # +x wall
    chart(tex, 34, 34, n, n, (-X, 0, -Z), (0, 0, 2 * Z / n), (0, Y / n, 0), (1, 0, 0))                # -x wall
    return tex


def quality_measures(tex, raw4, den4, raw1024, den1024):
    """K = mse(raw 4 frames) / mse(filtered 4 frames) against the 1024-frame bake, and the mean change the filter makes at 1024 frames
    over the mean change it makes at 4 frames; over the covered texels"""
    cov = tex["covered"] != 0
    gt = raw1024[cov][:, :3].astype(np.float64)

    def mse(a):
        return float(np.mean((a[cov][:, :3].astype(np.float64) - gt) ** 2))

    def change(a, b):
        return float(np.mean(np.abs(a[cov][:, :3].astype(np.float64) - b[cov][:, :3])))

    return mse(raw4) / mse(den4), change(den1024, raw1024) / change(den4, raw4)


def oracle_bake(oracle, sc, tex, n_frames, keep=()):
    """the output buffer and the moments plane a bake of frames 0 .. n_frames - 1 leaves, by the oracle: per covered texel and frame
    the model's bake ray (bake_ref.rays) as the fov = 0 pinhole of tests/test_bake_host.py, its path by pto_trace_paths, folded with
    the listed fold (adaptive_ref.fold_listed). keep: frame counts whose planes are wanted; {count: (output, moments)}"""
    H, W = tex.shape
    lst = bake_ref.covered_list(tex)
    ys, xs = np.divmod(lst, np.uint32(W))
    n = len(lst)
    scs = oracle.scene_struct(sc)
    opt = PtoOptions(QBOUNCES, 1, 0, 0, 1)
    fn = oracle.L.pto_trace_paths
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 6
    base = layout.make_camera(W, H, aperture=0.0)
    rgb, mom = np.zeros((n, 3), f32), np.zeros((n, 4), f32)
    got = {}
    for f in range(n_frames):
        fr = np.full(n, f, np.uint32)
        m = bake_ref.rays(oracle, tex, xs, ys, fr)
        cams = pr.fov0_cameras(base, m["org"], m["raw"])
        rad, seg = np.zeros((n, 3), f32), np.zeros(n, np.uint32)
        addr = [a.ctypes.data for a in (cams, xs, ys, fr, rad, seg)]
        step = [a.strides[0] for a in (cams, xs, ys, fr, rad, seg)]
        s_ref, o_ref = ctypes.byref(scs), ctypes.byref(opt)
        for i in range(n):                                      # one camera per sample, so one call per sample
            fn(s_ref, addr[0] + i * step[0], 1, addr[1] + i * step[1], addr[2] + i * step[2], addr[3] + i * step[3], o_ref,
               addr[4] + i * step[4], addr[5] + i * step[5])
        rgb, mom = adaptive_ref.fold_listed(rgb, mom, rad, fr)
        if f + 1 in keep:
            out, mo = np.zeros((H * W, 4), f32), np.zeros((H * W, 4), f32)
            out[lst, :3], mo[lst] = rgb, mom
            got[f + 1] = (out.reshape(H, W, 4), mo.reshape(H, W, 4))
    return got


# ---- the model -------------------------------------------------------------------------------------------------------------------
def holes(W, H):
    """texels with (7 x + 3 y) % 4 == 0 are uncovered, so no wave is all covered or all empty (tests/test_gpu_bake.py's rule)"""
    ys, xs = np.divmod(np.arange(W * H), W)
    return ((7 * xs + 3 * ys) % 4 != 0).reshape(H, W)


@pytest.mark.parametrize("variance", [0.0, 1e-3, 7.0])
def test_a_constant_map_comes_back_unchanged(variance):
    W, H = 37, 21
    tex = flat_surface(W, H, holes(W, H))
    cov = tex["covered"] != 0
    rad = np.zeros((H, W, 4), f32)
    # powers of two: every w c is w with another exponent, so sum w c = c sum w and the quotient is c, bit for bit
    rad[..., :3] = (0.5, 2.0, 0.125)
    out = bdr.denoise(tex, rad, moments_of(rad, variance, 4))
    assert np.array_equal(bits(out[cov][:, :3]), bits(rad[cov][:, :3]))
    assert (out[cov][:, 3] == 1).all() and not out[~cov].any()
    # any other constant: per pass 25 products, 24 + 24 additions of positive terms and one division, each within 2^-24 relative
    rad[..., :3] = (0.3, 1.7, 2.9)
    out = bdr.denoise(tex, rad, moments_of(rad, variance, 4), iterations=1)
    assert np.abs(out[cov][:, :3].astype(np.float64) / rad[cov][:, :3] - 1).max() <= 74 * 2.0 ** -24


def test_uncovered_texels_are_never_read():
    W, H = 37, 21
    tex = flat_surface(W, H, holes(W, H))
    cov = tex["covered"] != 0
    rs = np.random.RandomState(3)
    rad = rs.uniform(0, 2, (H, W, 4)).astype(f32)
    mom = moments_of(rad, 0.05, 4)
    want = bdr.denoise(tex, np.where(cov[..., None], rad, 0), np.where(cov[..., None], mom, 0), dilate=2)
    for junk in (np.nan, 1e30):
        r, m, t = rad.copy(), mom.copy(), tex.copy()
        r[~cov], m[~cov] = junk, junk
        t["position"][~cov], t["normal"][~cov] = junk, junk
        got = bdr.denoise(t, r, m, dilate=2)
        assert np.array_equal(bits(got), bits(want)), junk
    assert np.isfinite(want).all() and (want[..., 3] == 2).any()


@pytest.mark.parametrize("case", ["a", "b"])
def test_no_bleed_between_charts_that_touch_in_the_atlas(case):
    tex, right = two_charts(case)
    rad, mom = two_chart_planes(right)
    out = bdr.denoise(tex, rad, mom, iterations=3)
    within_chart_constants(out, tex, right)
    # the same records without the offset are one chart, and then the two halves do mix: the filter is not idle
    flat, _ = two_charts("a")
    flat["position"][right] -= (1.0, 0, 0)
    mixed = bdr.denoise(flat, rad, mom, iterations=3)
    assert mixed[:, right.shape[1] // 2 - 1, 0].min() > 1.1      # 10^4 times the bound above


def test_a_nan_and_a_firefly_stay_where_they_are():
    W, H = 24, 16
    tex = flat_surface(W, H)
    rs = np.random.RandomState(5)
    rad = rs.uniform(0.2, 0.8, (H, W, 4)).astype(f32)
    mom = moments_of(rad, 0.01, 4)
    rad[5, 7, :3], rad[9, 15, :3] = np.nan, 1e30
    out = bdr.denoise(tex, rad, mom)
    bad = ~np.isfinite(out[..., :3]).all(axis=-1)
    assert bad.sum() == 1 and bad[5, 7]
    assert out[9, 15, 0] > 1e29 and out[9, 14, 0] < 2 and out[8, 15, 0] < 2


def test_footprint_and_isolated_texels():
    """the footprint is the nearer of the covered 4-neighbours; an isolated texel has none and keeps its value"""
    W, H = 9, 7
    cov = np.zeros((H, W), bool)
    cov[1:4, 1:5] = True
    cov[5, 7] = True
    tex = flat_surface(W, H, cov, spacing=0.25)
    tex["position"][2, 2] += (0.125, 0, 0)                       # nearer to its right neighbour: 0.125
    rs = np.random.RandomState(9)
    rad = rs.uniform(0, 2, (H, W, 4)).astype(f32)
    gn, gp, cv = bdr.prepass(tex, rad, moments_of(rad, 0.5))
    assert gn[2, 2, 3] == f32(0.125) and gn[1, 1, 3] == f32(0.25) and gn[5, 7, 3] == 0 and not gn[~cov].any() and not gp[~cov].any()
    assert (gp[cov][:, 3] == 1).all() and np.array_equal(bits(cv[cov][:, :3]), bits(rad[cov][:, :3]))
    out = bdr.denoise(tex, rad, moments_of(rad, 0.5))
    assert np.array_equal(bits(out[5, 7]), bits(np.append(rad[5, 7, :3], f32(1))))


# ---- quality ---------------------------------------------------------------------------------------------------------------------
def test_model_cleans_a_cornell_bake_and_backs_off(oracle, scene_factory):
    sc = scene_factory("cornell")
    tex = quality_surface()
    assert (tex["covered"] != 0).sum() == 4 * 28 * 28
    bakes = oracle_bake(oracle, sc, tex, QTRUTH, keep=(QFRAMES, QTRUTH))
    (raw4, mom4), (raw1024, mom1024) = bakes[QFRAMES], bakes[QTRUTH]
    den4, den1024 = bdr.denoise(tex, raw4, mom4), bdr.denoise(tex, raw1024, mom1024)
    assert np.isfinite(den4).all() and np.isfinite(den1024).all()
    k, backoff = quality_measures(tex, raw4, den4, raw1024, den1024)
    print("K = mse(raw) / mse(filtered) = %.3f, back-off ratio = %.4f" % (k, backoff))
    assert k > K and backoff < BACKOFF, (k, backoff)


# ---- the ABI surface -------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_listed(tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    L = native.load()
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(L, f) and f in native.EXPORTS
    assert L.ptmi_abi_version() == 4 == native.ABI_VERSION
    buf = np.zeros(16, f32)
    assert L.ptmi_bake_denoise(None, None, None, 0) == -1 and L.ptmi_write_moments(None, native._p(buf), buf.size) == -1
    assert L.ptmi_bake_denoised_device_ptr(None) is None
    for m in ("bake_denoise", "bake_denoised_device_ptr", "write_moments"):
        assert hasattr(native.Context, m)
    fields = ("iterations", "dilate", "phi_color", "phi_normal", "phi_position", "reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu", sizeof(ptmi_bake_denoise_params));\n' +
                   "".join('printf(" %%zu", offsetof(ptmi_bake_denoise_params, %s));\n' % f for f in fields) + 'return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    dt = layout.BAKE_DENOISE_PARAMS
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in fields] == [32, 0, 4, 8, 12, 16, 20]
    assert ctypes.sizeof(native.BakeDenoiseParams) == 32
    assert [getattr(native.BakeDenoiseParams, f).offset for f in fields] == got[1:]
