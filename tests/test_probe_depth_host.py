"""Probe visibility without a GPU (include/ptmi.h ptmi_set_probe_depth, ptmi_probe_visibility): the numpy model of
tests/probe_depth_ref.py against float64, the lobe's locality, the border table against the octahedral map's own wrap, the two hosts'
helpers against each other, and the ABI surface.

Every case fails without the feature: the hosts have no such helpers and the binding no such calls."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import probe_depth_ref as pdr
import probe_ref
from ptmi import layout, native, probes
from test_probe_host import CASES, atlas_probes, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
f32 = np.float32


def one_probe(N):
    return atlas_probes(N, N, N)


# ---- the model against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m", [(4, 2), (4, 4), (8, 8), (16, 4), (16, 16), (64, 2), (64, 16)], ids=lambda v: str(v))
def test_a_constant_plane_filters_to_itself(N, m):
    """every weight sum normalises away: (c, c * c, 1) comes back. A sum of T = N * N terms, each a rounded product, through
    T / 64 + 6 rounded additions a lane, then one division: (N * N + 16) roundings of 2^-24 relative bound the lot, and the third
    component is exact (wgt * 1 is wgt, so a2 and a3 are the same sum)."""
    rec = one_probe(N)
    for c in (f32(1.7), f32(0.013), f32(23.5)):
        plane = np.zeros((N, N, 4), f32)
        plane[..., 0], plane[..., 1], plane[..., 2] = c, c * c, 1
        for s in (0, 1, 6):
            got = pdr.visibility(plane, rec, N, m, s)[0].reshape(-1, 4).astype(np.float64)
            tol = (N * N + 16) * 2.0 ** -24
            assert np.abs(got[:, 0] / np.float64(c) - 1).max() <= tol, (c, s)
            assert np.abs(got[:, 1] / (np.float64(c) * np.float64(c)) - 1).max() <= tol, (c, s)
            assert (got[:, 2] == 1).all() and (got[:, 3] == 1).all()


@pytest.mark.parametrize("N", [4, 8, 16, 32, 64])
def test_the_weight_sum_is_positive(N):
    """what include/ptmi.h argues for m <= N, at the sharpest lobe: every output texel's a3 is a normal float32"""
    rec = one_probe(N)
    ones = np.ones((N, N, 4), f32)
    for m in (2, 4, 8, 16):
        if m <= N:
            a3 = pdr.sums(ones, rec, N, m, 6)[0, :, 3]
            assert a3.min() > 1e-30, (N, m, a3.min())
            # ... because the nearest tile texel has a cosine above 0.5 to the output texel's direction
            d, n = probe_ref.tables64(N)[0], probe_ref.tables64(m)[0]
            assert (n @ d.T).max(axis=1).min() > 0.5, (N, m)


@pytest.mark.parametrize("N", [8, 16])
def test_the_sharpest_lobe_is_local(N):
    """s = 6, m = N: a plane that is 1 in one texel and 0 elsewhere filters to a tile that peaks at that texel"""
    rec = one_probe(N)
    for t0 in (0, 3, N * N // 2 + N // 2 - 1, N * (N - 1), N * N - 1, 2 * N + 5):
        plane = np.zeros((N, N, 4), f32)
        plane.reshape(-1, 4)[t0, 0] = 1
        got = pdr.visibility(plane, rec, N, N, 6)[0].reshape(-1, 4)
        assert int(np.argmax(got[:, 0])) == t0 and 0 < got[t0, 0] <= 1
        assert (np.delete(got[:, 0], t0) < got[t0, 0]).all() and not got[:, 1:3].any()


# ---- the border ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 4, 8, 16])
def test_the_border_table_is_the_maps_own_wrap(m):
    """The map folds every edge of the square onto itself about its midpoint: the edge a = +-1 lands on an arc in the plane y = 0
    (b' = copysign(1 - |a|, b) = 0 there), the edge b = +-1 on one in the plane x = 0. Past an edge the sphere therefore continues as
    the mirror image, in that plane, of what lies before it: the direction half a texel outside the tile is the direction of the
    point reflected back in (a -> +-2 - a), mirrored in y for an a-edge and in x for a b-edge, in both past a corner. That direction
    is the direction of the interior texel the table names."""
    d = probe_ref.tables64(m)[0].reshape(m, m, 3)
    step = 2.0 / m
    ring = 0
    for y in range(-1, m + 1):
        for x in range(-1, m + 1):
            a, b = (x + 0.5) * step - 1.0, (y + 0.5) * step - 1.0
            out_a, out_b = abs(a) > 1, abs(b) > 1
            if not (out_a or out_b):
                assert pdr.border_source(x, y, m) == (x, y)
                continue
            ring += 1
            ra = np.float64(np.copysign(2.0, a) - a if out_a else a)
            rb = np.float64(np.copysign(2.0, b) - b if out_b else b)
            pa, pb, w = probe_ref.fold_octahedral(np.array([ra]), np.array([rb]))
            p = np.array([pa[0], pb[0], w[0]])
            p /= np.sqrt((p * p).sum())
            if out_a:
                p[1] = -p[1]
            if out_b:
                p[0] = -p[0]
            sx, sy = pdr.border_source(x, y, m)
            assert 0 <= sx < m and 0 <= sy < m
            assert np.abs(p - d[sy, sx]).max() < 4e-16, (x, y, sx, sy)
    assert ring == 4 * m + 4


def test_add_border_is_the_table():
    rs = np.random.RandomState(5)
    for m in (2, 4, 8, 16):
        t = rs.uniform(-1, 1, (3, m, m, 4)).astype(f32)
        got = probes.add_border(t, m)
        assert got.dtype == f32 and got.flags.c_contiguous
        assert np.array_equal(bits(got), bits(pdr.add_border(t, m)))
        assert np.array_equal(bits(got[:, 1:-1, 1:-1]), bits(t))


def test_max_distance_is_one_and_a_half_cell_diagonals():
    v = probes.max_distance((0, 0, 0), (4, 2, 8), (4, 1, 2))
    assert isinstance(v, f32) and v == f32(1.5 * np.sqrt(1.0 + 4.0 + 16.0))
    assert probes.max_distance((-1, -1, -1), (1, 1, 1), (1, 1, 1)) == f32(1.5 * np.sqrt(12.0))


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_js_helpers_match_the_python_ones(tmp_path):
    rs = np.random.RandomState(11)
    sizes = (2, 4, 8, 16)
    tiles = [rs.uniform(-3, 3, (5, m, m, 4)).astype(f32) for m in sizes]
    for t in tiles:
        t.reshape(-1)[::7] = [-0.0, 1e-40, 2.5][len(t) % 3]
    np.concatenate([t.reshape(-1) for t in tiles]).tofile(str(tmp_path / "in.bin"))
    script = ("const fs = require('fs'), probes = require(%r);\n"
              "const raw = fs.readFileSync(process.argv[1] + '/in.bin');\n"
              "const all = new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4);\n"
              "const parts = []; let at = 0;\n"
              "for (const m of %s) { const n = 5 * m * m * 4; parts.push(Buffer.from(probes.addBorder(all.subarray(at, at + n), m).buffer)); at += n; }\n"
              "fs.writeFileSync(process.argv[1] + '/out.bin', Buffer.concat(parts));\n"
              "const cases = %s;\n"
              "console.log(JSON.stringify(cases.map(c => Array.from(new Uint32Array(new Float32Array([probes.maxDistance(c[0], c[1], c[2])]).buffer))[0])));\n"
              % (os.path.join(HOST, "probes.js"), repr(list(sizes)), repr([list(map(list, c)) for c in CASES])))
    out = subprocess.run([NODE, "-e", script, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    want = b"".join(probes.add_border(t, m).tobytes() for t, m in zip(tiles, sizes))
    assert open(str(tmp_path / "out.bin"), "rb").read() == want
    assert eval(out.stdout) == [int(bits(np.array([probes.max_distance(*c)], f32))[0]) for c in CASES]


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------------
NEW = ("ptmi_set_probe_depth", "ptmi_get_probe_depth", "ptmi_read_probe_depth", "ptmi_write_probe_depth", "ptmi_probe_visibility")


def test_entries_are_declared_exported_and_listed(tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    L = native.load()
    for f in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % f, hdr), f
        assert hasattr(L, f) and f in native.EXPORTS
    assert re.search(r"\bvoid\s*\*\s*ptmi_probe_depth_device_ptr\s*\(", hdr) and "ptmi_probe_depth_device_ptr" in native.EXPORTS
    assert L.ptmi_abi_version() == 4 == native.ABI_VERSION
    assert L.ptmi_set_probe_depth(None, None) == -1 and L.ptmi_get_probe_depth(None, None, None) == -1
    assert L.ptmi_read_probe_depth(None, None, 0) == -1 and L.ptmi_write_probe_depth(None, None, 0) == -1
    assert L.ptmi_probe_visibility(None, None, None, 0) == -1 and L.ptmi_probe_depth_device_ptr(None) is None
    for m in ("set_probe_depth", "get_probe_depth", "read_probe_depth", "write_probe_depth", "probe_visibility"):
        assert hasattr(native.Context, m)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(ptmi_probe_depth_params), offsetof(ptmi_probe_depth_params, _reserved),\n'
                   '       sizeof(ptmi_probe_visibility_params), offsetof(ptmi_probe_visibility_params, border),\n'
                   '       offsetof(ptmi_probe_visibility_params, _reserved), PTMI_ABI_VERSION);\nreturn 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [16, 4, 16, 8, 12, 4]
    assert ctypes.sizeof(native.ProbeDepthParams) == 16 and ctypes.sizeof(native.ProbeVisibilityParams) == 16
    assert layout.PROBE.itemsize == 16
