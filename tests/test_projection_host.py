"""Camera projections without a GPU (include/ptmi.h ptmi_set_projections): the numpy model of the orthographic and the equirectangular
ray (tests/projection_ref.py) against the CPU oracle, bit for bit. The oracle knows the pinhole only, and needs nothing else: a
pinhole camera with fov = 0 sends every pixel along normalize3(forward) from position, so each model ray (org0, raw) is pixel
(x, y, frame) of the oracle camera with position = org0, forward = raw, fov = 0 and everything else equal - the same seed, the same
jitter draws, the same lens. Also here: the ABI surface of the feature (the word offsets, the helpers, the NULL-handle answers)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import projection_ref as pr
from oracle_lib import Oracle
from ptmi import layout, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZES = ((7, 5), (64, 3))
FRAMES = (0, 1, 1 << 20)
APERTURES = (0.0, 0.05)
YMAG = 1.25


def rotated_basis(yaw=0.37, pitch=-0.21, roll=0.13):
    """forward, right, up of a camera turned about all three axes: orthonormal to float32 rounding, no component a zero"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    R = Ry @ Rx @ Rz
    fw, rt, up = R @ [0.0, 0.0, -1.0], R @ [1.0, 0.0, 0.0], R @ [0.0, 1.0, 0.0]
    return dict(forward=tuple(fw), right=tuple(rt), up=tuple(up))


def camera(W, H, projection, aperture=0.0, **kw):
    return layout.make_camera(W, H, position=(0.11, 1.03, 2.6), aperture=aperture, focus_distance=2.75, projection=projection, ymag=YMAG,
                              **rotated_basis(), **kw)


def all_pixels(W, H, frames=FRAMES):
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    return (np.tile(xs, len(frames)), np.tile(ys, len(frames)), np.repeat(np.asarray(frames, np.uint32), W * H))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def test_the_basis_has_no_zero_component_and_is_orthonormal():
    b = {k: np.asarray(v, f32) for k, v in rotated_basis().items()}
    for v in b.values():
        assert (v != 0).all() and abs(float(v.astype(np.float64) @ v.astype(np.float64)) - 1.0) < 1e-6
    assert abs(float(b["forward"] @ b["right"])) < 1e-6 and abs(float(b["forward"] @ b["up"])) < 1e-6 and abs(float(b["right"] @ b["up"])) < 1e-6
    assert np.allclose(np.cross(b["right"], b["up"]), -b["forward"], atol=1e-6)       # right-handed: forward = up x right


def test_a_pinhole_with_fov_zero_sends_every_pixel_along_forward(oracle):
    """the equivalence everything below rests on, on the oracle alone"""
    cam = camera(7, 5, "perspective", fov=0.0)
    xs, ys, fr = all_pixels(7, 5)
    o, d, _ = oracle.raygen(cam, xs, ys, fr)
    want = pr.normalize3(np.asarray(cam["forward"], f32)[None, :])[0]
    assert (bits(d) == bits(want)[None, :]).all() and (bits(o) == bits(np.asarray(cam["position"], f32))[None, :]).all()


@pytest.mark.parametrize("aperture", APERTURES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("projection", ["orthographic", "equirect"])
def test_model_rays_are_fov0_oracle_rays(oracle, projection, size, aperture):
    W, H = size
    cam = camera(W, H, projection, aperture)
    xs, ys, fr = all_pixels(W, H)
    m = pr.rays(oracle, cam, xs, ys, fr)
    assert (m["raw"] != 0).all() and (np.asarray(cam["forward"]) != 0).all()      # no ray is left out: none has a zero component
    cams = pr.fov0_cameras(cam, m["org0"], m["raw"])
    o, d, rng = (np.concatenate(a) for a in zip(*(oracle.raygen(cams[i:i + 1], xs[i:i + 1], ys[i:i + 1], fr[i:i + 1]) for i in range(len(xs)))))
    assert np.array_equal(bits(o), bits(m["o"])) and np.array_equal(bits(d), bits(m["d"])) and np.array_equal(rng, m["rng"])
    # the rays are what the projection says: unit directions; orthographic origins on the camera plane inside the half extents,
    # all along forward; equirect directions covering both hemispheres
    assert np.allclose((m["d"].astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6)
    fw, rt, up, pos = (np.asarray(cam[k], np.float64) for k in ("forward", "right", "up", "position"))
    if projection == "orthographic":
        rel = m["org0"].astype(np.float64) - pos
        # (float32 rounding of offsets up to |rel| ~ ymag * aspect = 27 units: a few ulps of 27, 2^-24 * 27 * 4 < 1e-5)
        assert np.abs(rel @ fw).max() < 1e-5 and np.abs(rel @ up).max() <= YMAG + 1e-5 and np.abs(rel @ rt).max() <= YMAG * W / H + 1e-5
        assert (bits(m["raw"]) == bits(np.asarray(cam["forward"], f32))[None, :]).all()
        if aperture == 0.0:
            assert np.array_equal(bits(m["o"]), bits(m["org0"]))
    else:
        assert (m["d"] @ fw.astype(f32) > 0).any() and (m["d"] @ fw.astype(f32) < 0).any()
        assert (bits(m["org0"]) == bits(np.asarray(cam["position"], f32))[None, :]).all()


@pytest.mark.parametrize("projection", ["orthographic", "equirect"])
def test_centre_rays_are_the_formula_at_the_pixel_centre(oracle, projection):
    """float64 restatement of the two formulas at (x + 0.5, y + 0.5): the model's float32 rays lie within rounding of it, the corner
    pixels of the equirectangular frame half a pixel from lon = +-pi, lat = +-pi / 2"""
    W, H = 64, 3
    cam = camera(W, H, projection)
    ys, xs = np.divmod(np.arange(W * H), W)
    m = pr.rays(oracle, cam, xs, ys)
    uvx, uvy = (xs + 0.5) / W * 2 - 1, (ys + 0.5) / H * 2 - 1
    fw, rt, up, pos = (np.asarray(cam[k], np.float64) for k in ("forward", "right", "up", "position"))
    if projection == "orthographic":
        o = pos + rt * (uvx * YMAG * float(cam["aspect"]))[:, None] + up * (uvy * YMAG)[:, None]
        d = np.broadcast_to(fw / np.linalg.norm(fw), (W * H, 3))
    else:
        lon, lat = uvx * np.pi, uvy * np.pi / 2
        d = fw * (np.cos(lat) * np.cos(lon))[:, None] + rt * (np.cos(lat) * np.sin(lon))[:, None] + up * np.sin(lat)[:, None]
        d /= np.linalg.norm(d, axis=1)[:, None]
        o = np.broadcast_to(pos, (W * H, 3))
    # origins: four float32 roundings at the magnitude of the farthest origin; unit directions: 2e-6 as for the pinhole's centre rays
    assert np.abs(m["o"] - o).max() <= 4 * 2.0 ** -23 * np.abs(o).max() and np.abs(m["d"] - d).max() < 2e-6 and (m["rng"] == 0).all()


def test_word_offsets_helpers_and_packing(tmp_path):
    """the two words sit at 88 and 92 as a C compiler lays out include/ptmi_layout.h, the helpers round-trip, and the binding packs
    the same bytes"""
    src = tmp_path / "words.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   '  ptmi_camera c; memset(&c, 0, sizeof c); ptmi_camera_set_projection(&c, PTMI_PROJ_ORTHOGRAPHIC, 1.25f);\n'
                   '  printf("%zu %zu %u %u %u %u %u %g\\n", offsetof(ptmi_camera, _p3), sizeof(ptmi_camera), PTMI_CAMERA_PROJECTION_OFFSET,\n'
                   '         PTMI_CAMERA_YMAG_OFFSET, PTMI_PROJ_PERSPECTIVE, PTMI_PROJ_EQUIRECT, ptmi_camera_projection(&c), ptmi_camera_ymag(&c));\n'
                   '  fwrite(&c, 1, sizeof c, stderr); return 0; }\n')
    exe = tmp_path / "words"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True)
    assert r.stdout.decode().split() == ["88", "96", "88", "92", "0", "2", "1", "1.25"]
    cam = np.zeros((), layout.CAMERA)
    layout.set_projection(cam, "orthographic", 1.25)
    assert cam.tobytes() == r.stderr
    assert layout.CAMERA.fields["_p3"][1] == 88 and layout.CAMERA.names == layout.make_camera(4, 4).dtype.names
    assert bits(layout.make_camera(4, 4)["_p3"]).tolist() == [0, 0]
    assert pr.projection_of(layout.make_camera(4, 4, projection="equirect", ymag=2.0)) == (2, f32(2.0))


def test_entries_are_exported_and_answer_a_null_handle():
    L = native.load()
    on = ctypes.c_uint32(7)
    for name in ("ptmi_set_projections", "ptmi_multi_set_projections"):
        assert name in native.EXPORTS and getattr(L, name)(None, 1) == -1
    for name in ("ptmi_get_projections", "ptmi_multi_get_projections"):
        assert name in native.EXPORTS and getattr(L, name)(None, ctypes.byref(on)) == -1
    assert L.ptmi_abi_version() == 4
    for cls in (native.Context, native.MultiContext):
        assert hasattr(cls, "set_projections") and hasattr(cls, "projections")
