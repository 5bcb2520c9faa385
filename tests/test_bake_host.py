"""Lightmap baking without a GPU (include/ptmi.h ptmi_upload_bake_surface, ptmi_dispatch_bake, ptmi_bake_dilate): the numpy model of
tests/bake_ref.py against the CPU oracle and against hand-written cases, the two hosts' rasterisers against the model and against each
other, and the ABI surface of the feature.

The oracle knows the pinhole only, and needs nothing else: a pinhole with fov = 0 and aperture = 0 sends pixel (x, y, frame) along
normalize3(forward) from position after exactly two draws, the jitter's, which are the two a cosine-weighted direction takes. So the
model's bake ray (org, raw) of texel (x, y) at frame f is pixel (x, y, f) of the oracle camera with position = org, forward = raw,
fov = 0 (projection_ref.fov0_cameras): origin, direction and RNG state, bit for bit."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bake_ref
import projection_ref as pr
from oracle_lib import Oracle
from ptmi import bake, layout, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
f32 = np.float32
AXES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
TILTED = ((0.31, 0.82, -0.48), (-0.95, 0.2, 0.24))       # the second has |n.x| > 0.9 once normalised: constructTBN's other branch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ray_surface(W, H, tilted_only=False):
    """(H, W) texel records for the ray tests: by texel index i, kind i % 9 = a normal along +-x, +-y, +-z (0 - 5), a tilted normal
    of length 0.5 (6) or 3 (7), or an uncovered texel (8) that holds garbage; tilted_only: kinds 6 and 7 alone, every texel covered"""
    t = np.zeros((H, W), layout.BAKE_TEXEL)
    for i in range(W * H):
        y, x = divmod(i, W)
        k = 6 + i % 2 if tilted_only else i % 9
        t[y, x]["position"] = (0.11 + 0.07 * x, 0.93 - 0.05 * y, -0.4 + 0.013 * i)
        if k < 6:
            t[y, x]["normal"], t[y, x]["covered"] = AXES[k], 1
        elif k < 8:
            n = np.asarray(TILTED[(i // 2) % 2], np.float64)
            t[y, x]["normal"], t[y, x]["covered"] = n / np.linalg.norm(n) * (0.5 if k == 6 else 3.0), 1 + i
        else:
            t[y, x]["normal"], t[y, x]["position"], t[y, x]["_pad"] = (np.nan, 0, 0), (np.inf, 1, 2), 0xDEADBEEF
    return t


def texel_grid(W, H, frames):
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    return np.tile(xs, len(frames)), np.tile(ys, len(frames)), np.repeat(np.asarray(frames, np.uint32), W * H)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


# ---- the model's rays ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [0.0, 1e-6, 0.25])
def test_model_rays_are_fov0_oracle_rays(oracle, bias):
    W, H = 7, 5
    tex = ray_surface(W, H, tilted_only=True)
    xs, ys, fr = texel_grid(W, H, (0, 1, 1000))
    m = bake_ref.rays(oracle, tex, xs, ys, fr, bias)
    assert m["covered"].all()
    cam = layout.make_camera(W, H, aperture=0.0)
    cams = pr.fov0_cameras(cam, m["org"], m["raw"])          # asserts that no component of raw is a zero
    o, d, rng = (np.concatenate(a) for a in zip(*(oracle.raygen(cams[i:i + 1], xs[i:i + 1], ys[i:i + 1], fr[i:i + 1]) for i in range(len(xs)))))
    assert np.array_equal(bits(o), bits(m["org"])) and np.array_equal(bits(d), bits(m["d"])) and np.array_equal(rng, m["rng"])
    # the origin is the position pushed along the raw direction by bias; with bias 0 it is the position's bits
    pos = tex[ys.astype(int), xs.astype(int)]["position"]
    if bias == 0.0:
        assert np.array_equal(bits(m["org"]), bits(pos))
    assert np.abs(m["org"].astype(np.float64) - (pos + np.float64(f32(bias)) * m["raw"])).max() <= 2.0 ** -23 * 2


def test_model_rays_follow_the_cosine_law(oracle):
    """4 096 rays of one texel: the mean of d . n is 2 / 3 under the cosine law (a uniform hemisphere gives 1 / 2), one draw's standard
    deviation is sqrt(1 / 18), and no ray leaves below the surface"""
    tex = ray_surface(7, 5, tilted_only=True)
    n_rays = 4096
    x, y = 3, 2
    m = bake_ref.rays(oracle, tex, np.full(n_rays, x), np.full(n_rays, y), np.arange(n_rays))
    n = tex[y, x]["normal"].astype(np.float64)
    n /= np.linalg.norm(n)
    cos = m["d"].astype(np.float64) @ n
    assert (cos > 0).all()
    se = np.sqrt(1.0 / 18.0) / np.sqrt(n_rays)
    print("mean d.n = %.5f, 2/3 +- 3 se = [%.5f, %.5f]" % (cos.mean(), 2 / 3 - 3 * se, 2 / 3 + 3 * se))
    assert abs(cos.mean() - 2.0 / 3.0) <= 3 * se
    assert np.abs((m["d"].astype(np.float64) ** 2).sum(axis=1) - 1).max() < 1e-6


def test_model_axis_normals_take_both_frames(oracle):
    """normals along +-x take constructTBN's second start vector, the others its first; every frame is orthonormal and right-handed"""
    n = np.array(AXES + TILTED, f32)
    nn = pr.normalize3(n)
    T, B = bake_ref.construct_tbn(nn)
    assert (np.abs(nn[:, 0]) > 0.9).tolist() == [True, True, False, False, False, False, False, True]
    for a, b in ((T, B), (T, nn), (B, nn)):
        assert np.abs((a.astype(np.float64) * b).sum(axis=1)).max() < 1e-6
    assert np.abs(np.cross(T.astype(np.float64), B) - nn).max() < 1e-6


def test_covered_list_is_ascending():
    tex = ray_surface(7, 5)
    got = bake_ref.covered_list(tex)
    assert got.tolist() == [i for i in range(35) if i % 9 != 8] and got.dtype == np.uint32


# ---- the dilate model, by hand -------------------------------------------------------------------------------------------------------
def plane(rows):
    """(H, W, 4) output buffer and (H, W) mask from rows of values (None: uncovered); rgb = (v, 2 v, -v)"""
    H, W = len(rows), len(rows[0])
    out, cov = np.full((H, W, 4), 77.0, f32), np.zeros((H, W), bool)
    for y, row in enumerate(rows):
        for x, v in enumerate(row):
            if v is not None:
                out[y, x], cov[y, x] = (v, 2 * v, -v, 9.0), True
    return out, cov


def test_dilate_a_corner_texel():
    out, cov = plane([[3.0, None, None], [None, None, None], [None, None, None]])
    r0 = bake_ref.dilate(out, cov, 0)
    assert r0[0, 0].tolist() == [3.0, 6.0, -3.0, 1.0] and not r0[cov == 0].any()          # the masked copy: w is the state, not out.w
    r1 = bake_ref.dilate(out, cov, 1)
    for y, x in ((0, 1), (1, 0), (1, 1)):                       # the corner's three neighbours, each from one texel
        assert r1[y, x].tolist() == [3.0, 6.0, -3.0, 2.0]
    assert r1[0, 0].tolist() == [3.0, 6.0, -3.0, 1.0]
    assert not r1[2].any() and not r1[:, 2].any()


def test_dilate_two_passes_reach_two_rings():
    out, cov = plane([[1.0, None, None, None, 5.0]])
    r1 = bake_ref.dilate(out, cov, 1)
    assert r1[0, :, 0].tolist() == [1.0, 1.0, 0.0, 5.0, 5.0] and r1[0, :, 3].tolist() == [1.0, 2.0, 0.0, 2.0, 1.0]
    r2 = bake_ref.dilate(out, cov, 2)
    assert r2[0, :, 0].tolist() == [1.0, 1.0, 3.0, 5.0, 5.0] and r2[0, :, 3].tolist() == [1.0, 2.0, 2.0, 2.0, 1.0]
    assert np.array_equal(bits(bake_ref.dilate(out, cov, 40)), bits(r2))                   # nothing is left to fill


def test_dilate_a_pass_never_reads_what_it_wrote():
    """in a 5 x 1 row with one covered end, a pass that read its own writes would fill the whole row at once"""
    out, cov = plane([[4.0, None, None, None, None]])
    for k in range(5):
        r = bake_ref.dilate(out, cov, k)
        assert r[0, :, 3].tolist() == [1.0] + [2.0] * k + [0.0] * (4 - k) and r[0, :k + 1, 0].tolist() == [4.0] * (k + 1)


def test_dilate_sums_in_neighbour_order_and_divides_once():
    """three neighbours whose float32 sum depends on the order: (1e8 + 1) - 1e8 = 0 left to right, 1 any other way"""
    out, cov = plane([[1e8, 1.0, -1e8], [None, None, None]])
    r = bake_ref.dilate(out, cov, 1)
    want = (f32(1e8) + f32(1.0) + f32(-1e8)) / f32(3)
    assert r[1, 1, 0] == want == 0.0 and r[1, 1, 3] == 2.0
    assert r[1, 0, 0] == (f32(1e8) + f32(1.0)) / f32(2)


# ---- the rasteriser ------------------------------------------------------------------------------------------------------------------
def mesh():
    """a unit quad split along the diagonal through the texel centres of a square map, a sliver that misses every centre, and a tilted
    triangle that overlaps the quad and so loses every texel it shares with it"""
    rs = np.random.RandomState(7)
    uv = np.array([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)],
                   [(0.15, 0.15), (0.3, 0.15), (0.15, 0.3)],
                   [(0.05, 0.2), (1.3, 0.45), (0.4, 1.2)]], f32)
    uv[:2] *= f32(0.5)                                         # the quad covers [0, 0.5]^2 (a power of two: the barycentrics on its diagonal are
                                                               # exact zeros); texels beyond it belong to the tilted triangle or to nobody
    return rs.uniform(-2, 2, (4, 3, 3)).astype(f32), rs.normal(size=(4, 3, 3)).astype(f32), uv


def test_rasteriser_shared_edge_goes_to_the_first_triangle():
    pos, nrm, uv = mesh()
    W = H = 8
    cov, _, _, tri = bake_ref.rasterise(pos, nrm, uv, W, H)
    diag = [tri[i, i] for i in range(4)]                       # centres (i + 0.5) / 8 < 0.5 lie on the shared diagonal
    assert diag == [0] * 4
    assert (tri[3, :3] == 1).all() and (tri[:3, 3] == 0).all() and tri[0, 0] == 0
    cov2, _, _, tri2 = bake_ref.rasterise(pos[[1, 0, 2, 3]], nrm[[1, 0, 2, 3]], uv[[1, 0, 2, 3]], W, H)
    assert [tri2[i, i] for i in range(4)] == [0] * 4 and np.array_equal(cov, cov2)          # the other order: the other triangle, still the first
    assert (tri == 3).any() and not cov.all()                   # the tilted triangle keeps what the quad leaves; some texels are nobody's


def test_rasteriser_a_sliver_between_centres_covers_nothing():
    pos, nrm, uv = mesh()
    for W, H in ((4, 4), (2, 2)):                               # legs of 0.15, texels of 0.25 and 0.5; the nearest centres, 0.125 and 0.375, miss it
        cov, _, _, tri = bake_ref.rasterise(pos[2:3], nrm[2:3], uv[2:3], W, H)
        assert not cov.any() and (tri == -1).all()
    cov, _, _, _ = bake_ref.rasterise(pos[2:3], nrm[2:3], uv[2:3], 64, 64)
    assert cov.any()                                            # it is there: a finer map finds it


@pytest.mark.parametrize("size", [(8, 8), (7, 5), (33, 16)], ids=lambda s: "%dx%d" % s)
def test_python_rasteriser_matches_the_model(size):
    W, H = size
    pos, nrm, uv = mesh()
    cov, p, n, _ = bake_ref.rasterise(pos, nrm, uv, W, H)
    rec = bake.rasterise(pos, nrm, uv, W, H)
    assert rec.dtype == layout.BAKE_TEXEL and rec.shape == (H, W)
    assert np.array_equal(rec["covered"] != 0, cov) and 0 < cov.sum() < W * H
    assert np.array_equal(bits(rec["position"]), bits(p)) and np.array_equal(bits(rec["normal"]), bits(n))
    assert not rec["_pad"].any() and not bits(rec["position"][~cov]).any() and not bits(rec["normal"][~cov]).any()


@pytest.mark.skipif(NODE is None, reason="node is not installed")
@pytest.mark.parametrize("size", [(8, 8), (7, 5), (33, 16)], ids=lambda s: "%dx%d" % s)
def test_js_rasteriser_matches_the_python_one(tmp_path, size):
    W, H = size
    pos, nrm, uv = mesh()
    for name, a in (("pos", pos), ("nrm", nrm), ("uv", uv)):
        a.tofile(str(tmp_path / (name + ".f32")))
    script = ("const fs = require('fs'), bake = require(%r);\n"
              "const rd = (n) => { const b = fs.readFileSync(process.argv[1] + '/' + n + '.f32');"
              " return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };\n"
              "const r = bake.rasterise(rd('pos'), rd('nrm'), rd('uv'), %d, %d);\n"
              "fs.writeFileSync(process.argv[1] + '/out.bin', Buffer.from(r.texels));\n"
              "console.log(r.covered);\n" % (os.path.join(HOST, "bake.js"), W, H))
    out = subprocess.run([NODE, "-e", script, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = np.fromfile(str(tmp_path / "out.bin"), layout.BAKE_TEXEL).reshape(H, W)
    want = bake.rasterise(pos, nrm, uv, W, H)
    assert int(out.stdout) == int((want["covered"] != 0).sum())
    assert got.tobytes() == want.tobytes()


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------------
NEW = ("ptmi_upload_bake_surface", "ptmi_dispatch_bake", "ptmi_bake_status", "ptmi_bake_dilate", "ptmi_debug_bake_rays")


def test_entries_are_declared_exported_and_listed(tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    L = native.load()
    for f in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % f, hdr), f
        assert hasattr(L, f) and f in native.EXPORTS
    assert L.ptmi_abi_version() == 4 == native.ABI_VERSION
    assert L.ptmi_dispatch_bake(None, None, 1) == -1 and L.ptmi_bake_status(None, None) == -1
    assert L.ptmi_upload_bake_surface(None, None, 0, 0) == -1 and L.ptmi_bake_dilate(None, 0, None, 0) == -1
    for m in ("upload_bake_surface", "dispatch_bake", "bake_status", "bake_dilate", "debug_bake_rays"):
        assert hasattr(native.Context, m)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(ptmi_bake_texel), offsetof(ptmi_bake_texel, covered),\n'
                   '       offsetof(ptmi_bake_texel, normal), sizeof(ptmi_bake_params), offsetof(ptmi_bake_params, bias),\n'
                   '       sizeof(struct ptmi_bake_status), PTMI_ABI_VERSION);\nreturn 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 12, 16, 16, 4, 16, 4]
    assert layout.BAKE_TEXEL.itemsize == 32 and layout.BAKE_TEXEL.fields["covered"][1] == 12 and layout.BAKE_TEXEL.fields["normal"][1] == 16
    assert ctypes.sizeof(native.BakeParams) == 16 and ctypes.sizeof(native.BakeStatus) == 16
