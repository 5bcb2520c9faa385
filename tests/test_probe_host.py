"""Light probes without a GPU (include/ptmi.h ptmi_upload_probes, ptmi_dispatch_probes, ptmi_probe_sh, ptmi_probe_irradiance): the numpy
model of tests/probe_ref.py against the CPU oracle, the library's host-built tables against the model bit for bit, the quadrature the
tables stand for against analytic SH9 and irradiance, the two hosts' lattice helpers against each other, and the ABI surface.

The oracle knows the pinhole only, and needs nothing else: a pinhole with fov = 0 and aperture = 0 sends pixel (x, y, frame) along
normalize3(forward) from position after exactly two draws, the jitter's, which are the two the octahedral point of a probe texel takes.
So the model's probe ray (org, raw) of texel (x, y) at frame f is pixel (x, y, f) of the oracle camera with position = org, forward =
raw, fov = 0 (projection_ref.fov0_cameras): origin, direction and RNG state, bit for bit."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import probe_ref
import projection_ref as pr
from oracle_lib import Oracle
from ptmi import layout, native, probes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def atlas_probes(W, H, N, disabled=()):
    """one probe per tile of a W x H atlas, at positions that differ in every component; `disabled`: indices switched off"""
    n = (W // N) * (H // N)
    rec = np.zeros(n, layout.PROBE)
    i = np.arange(n)
    rec["position"] = np.stack([0.11 + 0.07 * i, 0.93 - 0.05 * i, -0.4 + 0.013 * i], axis=1)
    rec["enabled"] = 1 + i                                        # any non-zero word
    rec["enabled"][list(disabled)] = 0
    return rec


def texel_grid(W, H, frames):
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    return np.tile(xs, len(frames)), np.tile(ys, len(frames)), np.repeat(np.asarray(frames, np.uint32), W * H)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


# ---- the model's rays ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 8, 64])
def test_model_rays_are_fov0_oracle_rays(oracle, N):
    W, H = 2 * N, N                                               # two tiles: x % N differs from x in the second
    rec = atlas_probes(W, H, N)
    xs, ys, fr = texel_grid(W, H, (0, 1, 7))
    if N == 64:                                                   # every texel of one tile, the second
        keep = xs >= N
        xs, ys, fr = xs[keep], ys[keep], fr[keep]
    m = probe_ref.rays(oracle, rec, N, W, xs, ys, fr)
    assert m["enabled"].all()
    assert (m["raw"] != 0).all()                                  # no component is a zero: the pinhole adds +0 to each
    cam = layout.make_camera(W, H, aperture=0.0)
    cams = pr.fov0_cameras(cam, m["org"], m["raw"])
    o, d, rng = (np.concatenate(a) for a in zip(*(oracle.raygen(cams[i:i + 1], xs[i:i + 1], ys[i:i + 1], fr[i:i + 1]) for i in range(len(xs)))))
    assert np.array_equal(bits(o), bits(m["org"])) and np.array_equal(bits(d), bits(m["d"])) and np.array_equal(rng, m["rng"])
    assert np.array_equal(bits(m["org"]), bits(rec["position"][probe_ref.probe_of(N, W, xs.astype(int), ys.astype(int))]))
    # the upper hemisphere and all four folded quadrants of the lower one
    raw = m["raw"]
    below = raw[:, 2] < 0
    for sx in (-1, 1):
        for sy in (-1, 1):
            assert (below & (np.sign(raw[:, 0]) == sx) & (np.sign(raw[:, 1]) == sy)).any(), (sx, sy)
    assert (~below).any()
    l1 = np.abs(raw.astype(np.float64)).sum(axis=1)               # the octahedron |x| + |y| + |z| = 1
    assert np.abs(l1 - 1).max() < 1e-6
    assert np.abs((m["d"].astype(np.float64) ** 2).sum(axis=1) - 1).max() < 1e-6


def test_model_rays_of_disabled_and_absent_probes_are_zeros(oracle):
    N, W, H = 4, 8, 8                                             # four tiles, three probes, the middle one off
    rec = atlas_probes(W, H, N, disabled=(1,))[:3]
    xs, ys, fr = texel_grid(W, H, (3,))
    m = probe_ref.rays(oracle, rec, N, W, xs, ys, fr)
    idx = probe_ref.probe_of(N, W, xs.astype(int), ys.astype(int))
    assert np.array_equal(m["enabled"], (idx == 0) | (idx == 2))
    off = ~m["enabled"]
    assert not m["org"][off].any() and not m["d"][off].any() and not m["rng"][off].any()
    lst = probe_ref.texel_list(rec, N, W, H)
    assert np.array_equal(lst, np.flatnonzero(m["enabled"])) and (np.diff(lst.astype(np.int64)) > 0).all() and lst.dtype == np.uint32
    assert len(lst) == 2 * N * N


def test_model_rays_cover_the_sphere_evenly(oracle):
    """the map's Jacobian is what dw states: weighting each ray of a tile by the solid angle per unit of the square at its point
    gives 4 pi and a zero mean direction"""
    N, W = 8, 8
    rec = atlas_probes(W, N, N)
    xs, ys, fr = texel_grid(W, N, range(16))
    m = probe_ref.rays(oracle, rec, N, W, xs, ys, fr)
    raw = m["raw"].astype(np.float64)
    jac = 4.0 / np.linalg.norm(raw, axis=1) ** 3                  # solid angle per unit area of [-1, 1]^2, whose area is 4
    print("mean Jacobian * 4 = %.4f (4 pi = %.4f)" % (jac.mean(), 4 * np.pi))
    assert abs(jac.mean() - 4 * np.pi) < 0.15
    assert np.abs((m["d"] * jac[:, None]).mean(axis=0)).max() < 0.15


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 4, 8, 16, 32, 64])
def test_library_tables_match_the_model(N):
    dir_dw, basis = native.probe_tables(N)
    want_d, want_b = probe_ref.tables(N)
    assert np.array_equal(bits(dir_dw), bits(want_d))
    assert np.array_equal(bits(basis), bits(want_b))
    assert abs(float(dir_dw[:, 3].astype(np.float64).sum()) - 4 * np.pi) < 1e-5
    assert np.abs((dir_dw[:, :3].astype(np.float64) ** 2).sum(axis=1) - 1).max() < 1e-6


def test_bad_table_sizes_are_refused():
    L = native.load()
    for tile in (0, 1, 3, 12, 128):
        assert L.ptmi_debug_probe_tables(tile, None, None) == -1, tile
    assert L.ptmi_debug_probe_tables(8, None, None) == 0


def analytic_sh(u, band_factors):
    """band_factors[l] * Y_lm(u), the SH9 of a function that is a zonal kernel about the unit vector u"""
    x, y, z = u
    Y = np.array([probe_ref.Y0, probe_ref.C1 * y, probe_ref.C1 * z, probe_ref.C1 * x, probe_ref.C2 * x * y, probe_ref.C2 * y * z,
                  probe_ref.C20 * (3 * z * z - 1), probe_ref.C2 * x * z, probe_ref.C22 * (x * x - y * y)])
    return Y * np.repeat(band_factors, [1, 3, 5])


def quadrature_errors(N):
    """absolute errors of the float64 rule at tile N: the largest over the SH9 of a constant, the largest over the SH9 of a clamped
    cosine about u = (0.3, -0.5, 0.81) normalised, and the irradiance of a constant at the normal u"""
    d, dw, Y = probe_ref.tables64(N)
    basis = Y * dw[:, None]
    const = np.abs(basis.sum(axis=0) - analytic_sh((0.0, 0.0, 1.0), [2 * np.sqrt(np.pi) / probe_ref.Y0, 0, 0])).max()
    u = np.array([0.3, -0.5, 0.81])
    u /= np.linalg.norm(u)
    cosine = np.abs((basis * np.maximum(d @ u, 0)[:, None]).sum(axis=0) - analytic_sh(u, [np.pi, 2 * np.pi / 3, np.pi / 4])).max()
    irr = abs((np.maximum(d @ u, 0) * dw).sum() - np.pi)          # E = pi under constant radiance, at the normal u
    return const, cosine, irr


def test_quadrature_is_second_order():
    sizes = (8, 16, 32, 64)
    err = {N: quadrature_errors(N) for N in sizes}
    for N in (4,) + sizes:
        print("N = %2d: constant %.5f, cosine %.5f, irradiance %.5f" % ((N,) + (err[N] if N in err else quadrature_errors(N))))
    for lo, hi in zip(sizes, sizes[1:]):
        for k, what in enumerate(("constant", "cosine", "irradiance")):
            assert err[lo][k] >= 3 * err[hi][k], (what, lo, hi, err[lo][k], err[hi][k])
    assert err[16][0] <= 0.03
    # the analytic constant: c_00 = 2 sqrt(pi), every other coefficient 0
    assert abs(analytic_sh((0, 0, 1), [2 * np.sqrt(np.pi) / probe_ref.Y0, 0, 0])[0] - 2 * np.sqrt(np.pi)) < 1e-12


def test_wave_sum_is_the_stated_order():
    """(1e8 + 1) - 1e8: lanes 0 and 32 meet at the butterfly's first step, lane 0's second texel (64) comes before it"""
    t = np.zeros((1, 128, 1), f32)
    t[0, 0], t[0, 64], t[0, 32] = 1e8, 1.0, -1e8
    assert probe_ref.wave_sum(t)[0, 0] == (f32(1e8) + f32(1.0)) + f32(-1e8) == 0.0
    t[0, 64], t[0, 1] = 0.0, 1.0                                  # lane 1 joins at the last step: 1 survives
    assert probe_ref.wave_sum(t)[0, 0] == 1.0


# ---- the hosts' lattice helpers ------------------------------------------------------------------------------------------------------
CASES = [((-1.0, 0.25, -3.5), (2.0, 1.75, 0.3), (3, 2, 4)), ((0.1, 0.2, 0.3), (0.7, 0.9, 1.1), (1, 1, 1)),
         ((-0.999, -0.999, -0.999), (0.999, 1.999, 0.999), (7, 3, 5))]


def test_grid_is_cell_centres():
    g = probes.grid((0, 0, 0), (4, 2, 8), (4, 1, 2))
    assert g.dtype == f32 and g.shape == (8, 3)
    assert g[:4, 0].tolist() == [0.5, 1.5, 2.5, 3.5] and (g[:, 1] == 1.0).all() and g[::4, 2].tolist() == [2.0, 6.0]
    rec = probes.records(g, enabled=[1, 0, 1, 1, 0, 0, 1, 1])
    assert rec.dtype == layout.PROBE and rec["enabled"].tolist() == [1, 0, 1, 1, 0, 0, 1, 1] and np.array_equal(rec["position"], g)


def test_atlas_size_is_the_most_nearly_square():
    assert [probes.atlas_size(n, 8) for n in (1, 2, 3, 4, 5, 9, 10, 4096)] == [(8, 8), (16, 8), (16, 16), (16, 16), (24, 16), (24, 24),
                                                                              (32, 24), (512, 512)]
    for n in range(1, 200):
        w, h = probes.atlas_size(n, 4)
        cols, rows = w // 4, h // 4
        assert cols * rows >= n > cols * (rows - 1) and 0 <= cols - rows <= 1


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_js_helpers_match_the_python_ones(tmp_path):
    script = ("const fs = require('fs'), probes = require(%r);\n"
              "const cases = %s;\n"
              "const parts = [], sizes = [];\n"
              "for (const c of cases) { const g = probes.grid(c[0], c[1], c[2]); parts.push(Buffer.from(g.buffer));\n"
              "  const en = Array.from({length: g.length / 3}, (_, i) => i %% 3 !== 1); parts.push(Buffer.from(probes.records(g, en))); }\n"
              "for (let n = 1; n < 300; n++) { const s = probes.atlasSize(n, 8); sizes.push(s.width, s.height); }\n"
              "fs.writeFileSync(process.argv[1] + '/out.bin', Buffer.concat(parts));\n"
              "console.log(JSON.stringify(sizes));\n" % (os.path.join(HOST, "probes.js"), repr([list(map(list, c)) for c in CASES])))
    out = subprocess.run([NODE, "-e", script, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    want = b""
    for lo, hi, counts in CASES:
        g = probes.grid(lo, hi, counts)
        want += g.tobytes() + probes.records(g, np.arange(len(g)) % 3 != 1).tobytes()
    assert open(str(tmp_path / "out.bin"), "rb").read() == want
    sizes = [v for n in range(1, 300) for v in probes.atlas_size(n, 8)]
    assert eval(out.stdout) == sizes


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------------
NEW = ("ptmi_upload_probes", "ptmi_dispatch_probes", "ptmi_probe_status", "ptmi_probe_sh", "ptmi_probe_irradiance",
       "ptmi_debug_probe_rays", "ptmi_debug_probe_tables")


def test_entries_are_declared_exported_and_listed(tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    L = native.load()
    for f in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % f, hdr), f
        assert hasattr(L, f) and f in native.EXPORTS
    assert L.ptmi_abi_version() == 4 == native.ABI_VERSION
    assert L.ptmi_dispatch_probes(None, None, 1) == -1 and L.ptmi_probe_status(None, None) == -1
    assert L.ptmi_upload_probes(None, None, 0, 0) == -1 and L.ptmi_probe_sh(None, None, 0) == -1
    assert L.ptmi_probe_irradiance(None, 2, None, 0) == -1
    for m in ("upload_probes", "dispatch_probes", "probe_status", "probe_sh", "probe_irradiance", "debug_probe_rays"):
        assert hasattr(native.Context, m)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(ptmi_probe), offsetof(ptmi_probe, enabled), sizeof(ptmi_probe_params),\n'
                   '       offsetof(ptmi_probe_params, _reserved), sizeof(struct ptmi_probe_status), PTMI_ABI_VERSION);\nreturn 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [16, 12, 16, 4, 20, 4]
    assert layout.PROBE.itemsize == 16 and layout.PROBE.fields["enabled"][1] == 12
    assert ctypes.sizeof(native.ProbeParams) == 16 and ctypes.sizeof(native.ProbeStatus) == 20
