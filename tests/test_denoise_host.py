"""Sample moments and the denoiser (include/ptmi.h ptmi_set_moments, ptmi_denoise) without a GPU: the header and the library agree
on the entry points, each refuses a NULL context, and the plain reference of tests/denoise_ref.py keeps edges, keeps a NaN where it
is and cleans an oracle render of the Cornell box."""
import ctypes
import os
import re

import numpy as np

import aov_ref
import denoise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["ptmi_set_moments", "ptmi_get_moments", "ptmi_read_moments", "ptmi_moments_device_ptr", "ptmi_denoise",
         "ptmi_denoised_device_ptr", "ptmi_blit_denoised"]
# The reference's denoised 4-spp 64x64 Cornell box (default parameters: 5 passes, demodulated) has 1/4.37 of the raw image's MSE
# against a 1024-spp oracle render (measured with this module's _cornell); the bar is half of that. tests/test_gpu_denoise.py
# uses the same bar.
K_MEASURED = 4.37
K = K_MEASURED / 2


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)


def test_header_declares_the_entry_points():
    h = _header()
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, h), f
    assert "ptmi_denoise_params" in h
    assert re.search(r"#define PTMI_ABI_VERSION 4\b", h)
    assert "PTMI_AOV_MOMENTS" not in h


def test_library_exports_them_and_the_binding_lists_them():
    from ptmi import native
    L = native.load()
    for f in FUNCS:
        assert hasattr(L, f), f
        assert f in native.EXPORTS
    assert set(native.AOVS) == {"albedo", "normal", "id"}
    assert ctypes.sizeof(native.DenoiseParams) == 32


def test_null_context_is_refused():
    from ptmi import native
    L = native.load()
    on = ctypes.c_uint32(7)
    buf = np.zeros(64, np.float32)
    u8 = np.zeros(64, np.uint8)
    assert L.ptmi_set_moments(None, 0) == -1 and L.ptmi_set_moments(None, 1) == -1
    assert L.ptmi_get_moments(None, ctypes.byref(on)) == -1 and on.value == 7
    assert L.ptmi_read_moments(None, native._p(buf), buf.size) == -1
    assert L.ptmi_moments_device_ptr(None) is None
    prm = native.DenoiseParams()
    assert L.ptmi_denoise(None, None, None, 0) == -1
    assert L.ptmi_denoise(None, ctypes.byref(prm), native._p(buf), buf.size) == -1
    assert L.ptmi_denoised_device_ptr(None) is None
    assert L.ptmi_blit_denoised(None, native._p(buf), buf.size, native._p(u8), u8.size) == -1


def _flat_scene(H=16, W=24):
    """two planes facing different ways, split at column W / 2, both at depth 1; noisy colour, unit variance"""
    rng = np.random.default_rng(1)
    normal = np.zeros((H, W, 4), np.float32)
    normal[:, : W // 2, 2] = 1
    normal[:, W // 2:, 0] = 1
    normal[..., 3] = 1
    rad = np.zeros((H, W, 4), np.float32)
    rad[:, : W // 2, :3] = 0.2
    rad[:, W // 2:, :3] = 0.8
    rad[..., :3] += rng.normal(0, 0.05, (H, W, 3)).astype(np.float32)
    mom = np.zeros((H, W, 4), np.float32)
    l = denoise_ref.lum(rad[..., 0], rad[..., 1], rad[..., 2])
    mom[..., 0], mom[..., 1], mom[..., 2] = l, l * l + np.float32(0.01), 4
    albedo = np.ones((H, W, 4), np.float32)
    return rad, normal, albedo, mom


def test_reference_keeps_a_normal_edge():
    rad, normal, albedo, mom = _flat_scene()
    W = rad.shape[1]
    # the same colour on both sides: only the normals tell them apart
    rad[:, W // 2:, :3] = rad[:, : W // 2, :3][:, ::-1] + np.float32(0.6)
    out = denoise_ref.denoise(rad, normal, albedo, mom, iterations=5, demodulate=False, phi_color=1e6)
    left, right = out[:, : W // 2, :3], out[:, W // 2:, :3]
    assert left.max() < 0.5 < right.min(), (left.max(), right.min())
    assert np.all(out[..., 3] == 0)
    # the noise went down on both sides
    assert left.std() < 0.5 * rad[:, : W // 2, :3].std()
    assert right.std() < 0.5 * rad[:, W // 2:, :3].std()
    # one normal everywhere: the two sides do mix
    normal[:] = 0
    normal[..., 2] = normal[..., 3] = 1
    mixed = denoise_ref.denoise(rad, normal, albedo, mom, iterations=5, demodulate=False, phi_color=1e6)
    assert mixed[:, W // 2 - 1, 0].mean() > out[:, W // 2 - 1, 0].mean() + 0.05


def test_reference_keeps_a_nan_where_it_is():
    rad, normal, albedo, mom = _flat_scene()
    rad[5, 7, :3] = np.nan
    rad[9, 15, :3] = 1e30
    for dm in (False, True):
        out = denoise_ref.denoise(rad, normal, albedo, mom, iterations=5, demodulate=dm)
        bad = ~np.isfinite(out[..., :3]).all(axis=-1)
        assert bad.sum() == 1 and bad[5, 7]
        assert np.isnan(out[5, 7, :3]).all()
        # the huge pixel stays huge, its neighbours do not pick it up
        assert out[9, 15, 0] > 1e29 and out[9, 14, 0] < 2 and out[8, 15, 0] < 2


def test_reference_misses_keep_their_value():
    rad, normal, albedo, mom = _flat_scene()
    normal[3:6, 3:6] = 0                                   # a hole of misses
    out = denoise_ref.denoise(rad, normal, albedo, mom, iterations=3, demodulate=False)
    assert np.array_equal(out[3:6, 3:6, :3].view(np.uint32), rad[3:6, 3:6, :3].view(np.uint32))


def test_moments_fold_definition():
    rng = np.random.default_rng(2)
    L = [rng.uniform(0, 4, (50, 3)).astype(np.float32) for _ in range(3)]
    L[1][0] = np.nan                                       # fmin(NaN, 2.5) = 2.5
    m = denoise_ref.fold_moments(L, [0, 1, 2])
    c = [np.fmin(x, np.float32(2.5)).astype(np.float64) for x in L]
    l = [0.2126 * x[:, 0] + 0.7152 * x[:, 1] + 0.0722 * x[:, 2] for x in c]
    assert np.allclose(m[:, 0], np.mean(l, axis=0), rtol=1e-5)
    assert np.allclose(m[:, 1], np.mean(np.square(l), axis=0), rtol=1e-5)
    assert (m[:, 2] == 3).all() and (m[:, 3] == 0).all()
    # a second dispatch continues the fold bit for bit
    m2 = denoise_ref.fold_moments(L[2:], [2], acc=denoise_ref.fold_moments(L[:2], [0, 1]))
    assert np.array_equal(m.view(np.uint32), m2.view(np.uint32))


def _cornell(oracle, sc, W, H, frames):
    """the 64x64 planes a context with every plane on would hold after `frames` frames: radiance (the oracle's render), albedo and
    normal (tests/aov_ref.py), moments folded from the per-path radiance (Oracle.trace_path)"""
    from ptmi import layout
    cam = layout.make_camera(W, H)
    raw, _ = oracle.render(sc, cam, frames, max_bounces=8, do_mis=1)
    s = [aov_ref.samples(oracle, sc, cam, f) for f in range(frames)]
    a, n, _, _ = aov_ref.fold(s, list(range(frames)))
    Ls = []
    for f in range(frames):
        L = np.zeros((W * H, 3), np.float32)
        for y in range(H):
            for x in range(W):
                L[y * W + x] = oracle.trace_path(sc, cam, x, y, f)[0]
        Ls.append(L)
    mom = denoise_ref.fold_moments(Ls, list(range(frames)))
    return cam, raw, a.reshape(H, W, 4), n.reshape(H, W, 4), mom.reshape(H, W, 4), Ls


def test_reference_cleans_the_cornell_box(oracle, scene_factory):
    sc = scene_factory("cornell")
    W = H = 64
    cam, raw, albedo, normal, mom, Ls = _cornell(oracle, sc, W, H, 4)
    # the per-path radiance folds to the oracle's running mean, clamped as the kernels clamp
    acc = np.fmin(Ls[0], np.float32(2.5))
    for f in range(1, 4):
        acc = aov_ref._mix(acc, np.fmin(Ls[f], np.float32(2.5)), np.float32(1) / np.float32(f + 1))
    assert np.array_equal(acc.view(np.uint32), raw.reshape(-1, 4)[:, :3].copy().view(np.uint32))
    gt, _ = oracle.render(sc, cam, 1024, max_bounces=8, do_mis=1)
    den = denoise_ref.denoise(raw, normal, albedo, mom)
    assert np.isfinite(den).all()

    def mse(a):
        return float(np.mean((a[..., :3].astype(np.float64) - gt[..., :3]) ** 2))

    assert mse(den) * K < mse(raw), (mse(den), mse(raw))
