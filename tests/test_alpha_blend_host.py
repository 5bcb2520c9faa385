"""Alpha blending at the C ABI (include/ptmi.h ptmi_set_alpha_blend), its numpy model (tests/alpha_blend_ref.py) and the JS loader's
table, without a GPU: the model's hash is a second implementation's in plain Python integers, on literal rays; alpha 0 is never there
and alpha 1 always; the calls are exported and listed by the binding, the two structs are laid out as the binding mirrors them, a
NULL handle is refused; host/scene_prep.js makes the table glTF's alphaMode BLEND asks for, and leaves everything as it was with
alphaCutout alone."""
import ctypes
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import alpha_blend_ref as B
import alpha_ref as A
from ptmi import glb_io, native, scenes
from test_alpha_host import LIB, PKG, ROOT
from test_node_medium import HOST, NODE, ensure_addon

SHARED = ("set_alpha_blend", "alpha_blend_status")
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", PKG, "all"], stdout=subprocess.DEVNULL)
    return ctypes.CDLL(LIB)


# ---- the hash ------------------------------------------------------------------------------------------------------------------------
def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def xi_int(o, d, tri, seed):
    """include/ptmi.h's definition in Python integers, one ray at a time: (h, xi as an exact fraction of 2^24)"""
    h = 0x9E3779B9
    for w in [bits(c) for c in o] + [bits(c) for c in d] + [tri & M32, seed & M32]:
        x = h ^ w
        x ^= x >> 16
        x = (x * 0x7FEB352D) & M32
        x ^= x >> 15
        x = (x * 0x846CA68B) & M32
        x ^= x >> 16
        h = x
    return h, (h >> 8) / float(1 << 24)


DENORMAL = 1e-45                    # the smallest float32 denormal: bits 0x00000001
RAYS = [
    ((0.0, 1.0, 2.8), (0.0, 0.0, -1.0), 0, 0),
    ((0.0, 1.0, 2.8), (-0.0, 0.0, -1.0), 0, 0),                            # -0.0 is another word than 0.0
    ((-0.0, -0.0, -0.0), (0.6, -0.8, 0.0), 1132, 7),
    ((DENORMAL, 1.0, -DENORMAL), (0.0, 1.0, 0.0), 5, 1),
    ((float("inf"), 0.25, float("-inf")), (1.0, 0.0, 0.0), 0xFFFFFFFF, 0xFFFFFFFF),
    ((200.0, 200.0, 200.0), (0.26726124, 0.5345225, 0.80178374), 4096, 0x80000000),
    ((1.5, -2.25, 3.125), (0.0, 0.0, 1.0), 17, 123456789),
]


def test_xi_is_the_definition_in_plain_integers():
    assert bits(-0.0) == 0x80000000 and bits(DENORMAL) == 1 and bits(float("inf")) == 0x7F800000
    seen = set()
    for o, d, tri, seed in RAYS:
        h, x = xi_int(o, d, tri, seed)
        got_h = B.hash_words(np.float32([o]), np.float32([d]), np.array([tri], np.uint32), seed)
        got = B.xi(np.float32([o]), np.float32([d]), np.array([tri], np.uint32), seed)
        assert int(got_h[0]) == h, (o, d, tri, seed)
        assert got.dtype == np.float32 and float(got[0]) == x and 0.0 <= x < 1.0            # h >> 8 is exact in float32
        seen.add(h)
    assert len(seen) == len(RAYS)
    # all rays at once give what they give one by one, and every word matters
    o, d = np.float32([r[0] for r in RAYS]), np.float32([r[1] for r in RAYS])
    tri = np.array([r[2] for r in RAYS], np.uint32)
    together = B.hash_words(o, d, tri, 11)
    assert [int(v) for v in together] == [xi_int(r[0], r[1], r[2], 11)[0] for r in RAYS]
    base = xi_int((0.5, 0.5, 0.5), (0.0, 0.0, 1.0), 3, 4)[0]
    for k in range(8):
        oo, dd, tri1, seed1 = [0.5, 0.5, 0.5], [0.0, 0.0, 1.0], 3, 4
        if k < 3:
            oo[k] = 0.75
        elif k < 6:
            dd[k - 3] = 0.125
        elif k == 6:
            tri1 = 2
        else:
            seed1 = 5
        assert xi_int(oo, dd, tri1, seed1)[0] != base, k
    # the largest word gives the largest threshold below 1
    assert ((np.uint32(M32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)) == np.float32(1.0 - 2.0 ** -24)


def test_the_hash_is_uniform_enough():
    """camera-like rays: one origin, jittered directions; and the triangle alone varying"""
    rng = np.random.default_rng(1)
    n = 40000
    d = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.4, 0.4, n), np.full(n, -1.0)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(np.float32([0.0, 1.0, 2.8]), (n, 1))
    x = B.xi(o, d.astype(np.float32), np.zeros(n, np.uint32), 0)
    for a in (0.25, 0.5, 0.75, 64 / 255, 128 / 255):
        there = (np.float32(a) > x).mean()
        assert abs(there - a) < 4.0 * np.sqrt(a * (1 - a) / n), (a, there)
    x = B.xi(o[:4096], np.tile(np.float32([0.0, 0.0, -1.0]), (4096, 1)), np.arange(4096, dtype=np.uint32), 0)
    assert abs((x < 0.5).mean() - 0.5) < 4.0 * np.sqrt(0.25 / 4096)


def test_the_ends_need_no_hash():
    """alpha = 0 is never there and alpha = 1 always, whatever the ray and the seed; a factor of 0 removes what the texel shows; the
    cutoff rule comes first and its holes are no tests; a material that is not blended is never asked"""
    alpha = np.stack([np.zeros((8, 8)), np.ones((8, 8)), np.full((8, 8), 0.5)]).astype(np.float32)
    sc = scenes.cornell_fence(alpha, z=(0.4, 0.3, 0.2))
    mats = sc.info["fence_materials"]
    rng = np.random.default_rng(2)
    n = 4096
    o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    u = v = np.full(n, 0.25, np.float32)
    table = B.blend_table(sc, 1.0)
    by_fence = [np.flatnonzero(sc.tris["material_index"] == m) for m in mats]
    for seed in (0, 7, 0xFFFFFFFF):
        for f, want in ((0, True), (1, False)):
            tri = rng.choice(by_fence[f], n)
            gone, tested = B.absent(sc, table, seed, o, d, tri, u, v)
            assert tested.all() and np.all(gone == want), (seed, f)
        tri = rng.choice(by_fence[2], n)
        gone, tested = B.absent(sc, table, seed, o, d, tri, u, v)
        assert tested.all() and 0.4 < gone.mean() < 0.6
        assert np.array_equal(gone, np.float32(0.5) <= B.xi(o, d, tri, seed))
    tri = rng.choice(by_fence[1], n)
    gone, tested = B.absent(sc, B.blend_table(sc, 0.0), 0, o, d, tri, u, v)
    assert tested.all() and gone.all()                                      # factor 0: alpha 0 whatever the texel
    gone, tested = B.absent(sc, B.blend_table(sc, 1.0, fences=[0]), 0, o, d, tri, u, v)
    assert not tested.any() and not gone.any()                              # fence 1 is not in this table
    cutoff = np.zeros(len(sc.mats), np.float32)
    cutoff[mats[2]] = 0.75
    gone, tested = B.absent(sc, table, 0, o, d, rng.choice(by_fence[2], n), u, v, cutoff=cutoff)
    assert gone.all() and not tested.any()                                  # 0.5 < 0.75: MASK holes, no test
    plain = np.flatnonzero(~np.isin(sc.tris["material_index"], mats))[:n]
    gone, tested = B.absent(sc, table, 0, o[:len(plain)], d[:len(plain)], plain, u[:len(plain)], v[:len(plain)])
    assert not gone.any() and not tested.any()


def test_the_loops_without_a_blended_material_are_alpha_refs(oracle):
    """with no entry >= 0 the model's loops are the cutoff model's, on the CPU oracle's probe"""
    sc, cutoff = A.fence_scene(A.checker(2), z=(0.4, 0.3))
    rng = np.random.default_rng(3)
    n = 1000
    o = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(0.1, 1.9, n), rng.uniform(1.2, 3.0, n)], 1).astype(np.float32)
    t = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 2.0, n), np.full(n, 0.3)], 1)
    d = t - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    probe = lambda oo, dd: oracle.intersect(sc, oo, dd)[:4]
    none = np.full(len(sc.mats), -1.0, np.float32)
    want, got = A.resolve(probe, sc, cutoff, o, d), B.resolve(probe, sc, none, o, d, cutoff=cutoff)
    assert all(np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(want, got))
    dist = rng.uniform(0.3, 6.0, n).astype(np.float32)
    dist[::3] = -1.0
    want, got = A.occluded(probe, sc, cutoff, o, d, dist), B.occluded(probe, sc, none, o, d, dist, cutoff=cutoff)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    # all fences at alpha 0 under factor 1: every ray ends on what the scene without the fences shows
    sc0 = scenes.cornell_fence(np.zeros((2, 8, 8), np.float32), z=(0.4, 0.3))
    bare = scenes.cornell_fence(None, z=(0.4, 0.3), drop=np.ones((2, 8, 8), bool))
    counts = {}
    t0, tri0, layers = B.resolve(lambda oo, dd: oracle.intersect(sc0, oo, dd)[:4], sc0, B.blend_table(sc0), o, d, counts=counts)
    wt = oracle.intersect(bare, o, d)[0]
    assert np.array_equal(t0.view(np.uint32), wt.view(np.uint32)) and layers.max() == 2
    assert counts["tests"] == counts["passes"] == int(layers.sum())


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_exported(lib):
    for prefix in ("ptmi_", "ptmi_multi_"):
        for n in SHARED:
            assert hasattr(lib, prefix + n), prefix + n
            assert prefix + n in native.EXPORTS
    for n in SHARED:
        assert n in native._SHARED and hasattr(native._Handle, n)
    assert lib.ptmi_abi_version() == 4                  # new calls only: the version stays
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert "BLEND stays opaque without ptmi_set_alpha_blend" in header
    for word in ("0x7feb352d", "0x846ca68b", "0x9E3779B9", "alpha <= xi"):
        assert word in header, word


def test_structs_match_the_header(tmp_path):
    pairs = (("ptmi_alpha_blend_params", native.AlphaBlendParams, 16), ("struct ptmi_alpha_blend_status", native.AlphaBlendStatus, 56))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ptmi.h"', 'int main(void) {']
    for k, (st, cls, _) in enumerate(pairs):
        lines.append(f'printf("size{k} %zu\\n", sizeof({st}));')
        lines += [f'printf("{k}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines += ['printf("alpha %zu\\n", sizeof(struct ptmi_alpha_status)); printf("stats %zu\\n", sizeof(ptmi_stats));', 'return 0; }']
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for k, (_, cls, size) in enumerate(pairs):
        assert int(got[f"size{k}"]) == ctypes.sizeof(cls) == size
        for f, _ in cls._fields_:
            assert int(got[f"{k}.{f}"]) == getattr(cls, f).offset, f
    # the structs every caller already has did not grow
    assert int(got["alpha"]) == ctypes.sizeof(native.AlphaStatus) == 48 and int(got["stats"]) == ctypes.sizeof(native.Stats)


def test_refusals_without_a_device(lib):
    """a NULL handle is refused before anything is touched"""
    one = (ctypes.c_float * 1)(0.5)
    st = native.AlphaBlendStatus()
    prm = native.AlphaBlendParams(0, 3, (ctypes.c_uint32 * 2)(0, 0))
    for prefix in ("ptmi_", "ptmi_multi_"):
        assert getattr(lib, prefix + "set_alpha_blend")(None, one, 1, None) != 0
        assert getattr(lib, prefix + "set_alpha_blend")(None, None, 0, ctypes.byref(prm)) != 0
        assert getattr(lib, prefix + "alpha_blend_status")(None, ctypes.byref(st)) != 0
        assert getattr(lib, prefix + "alpha_blend_status")(None, None) != 0


# ---- the JS loader's table -----------------------------------------------------------------------------------------------------------
SCRIPT = """
var prep = require(%(prep)s), gltf = require(%(gltf)s);
function run(opts) {
  var s = prep.prepareScene(gltf.loadGLB(%(glb)s), opts), a = s.atlas;
  return { blend: s.alphaBlend === undefined ? 'undefined' : s.alphaBlend === null ? null : Array.from(s.alphaBlend),
           cutoff: s.alphaCutoff ? Array.from(s.alphaCutoff) : null,
           blobs: Object.keys(s.blobs).map(function (k) { return Buffer.from(s.blobs[k]).toString('base64'); }),
           rgba8: Buffer.from(a.rgba8.buffer, a.rgba8.byteOffset, a.rgba8.byteLength).toString('base64') };
}
var info = { none: run(), cut: run({ alphaCutout: true }), blend: run({ alphaBlend: true }), both: run({ alphaCutout: true, alphaBlend: true }) };
info.opaqueOnly = prep.prepareScene(gltf.loadGLB(%(plain)s), { alphaBlend: true }).alphaBlend;
info.of = [undefined, {}, { alphaMode: 'MASK' }, { alphaMode: 'BLEND' },
           { alphaMode: 'BLEND', pbrMetallicRoughness: { baseColorFactor: [1, 1, 1, 0.25] } }].map(prep.alphaBlendOf);
console.log(JSON.stringify(info));
"""


def blend_glb(path, modes=True):
    """six quads; materials: OPAQUE, MASK at 0.6 over an RGBA image, BLEND with factor 0.5 over the same image, BLEND with factor 0,
    BLEND without a factor, and a primitive without a material. modes=False: the same file with every alphaMode left out."""
    rng = np.random.default_rng(4)
    img = rng.integers(64, 256, (16, 16, 4), dtype=np.uint8)
    img[:8, :, 3], img[8:, :, 3] = 255, 64

    def mesh_of(k, material):
        t = scenes._quad((k, 0, 0), (k + 0.9, 0, 0), (k + 0.9, 1, 0), (k, 1, 0), (0, 0, 1), 0)
        pos = np.stack([t["v0"], t["v1"], t["v2"]], 1).reshape(-1, 3)
        nrm = np.stack([t["n0"], t["n1"], t["n2"]], 1).reshape(-1, 3)
        uv = np.tile(np.float32([[0.1, 0.1], [0.9, 0.1], [0.9, 0.9]]), (2, 1))
        m = {"positions": pos, "normals": nrm, "uvs": uv, "indices": np.arange(len(pos))}
        if material is not None:
            m["material"] = material
        return m
    pbr = lambda a, tex=False: {"pbrMetallicRoughness": dict({"baseColorFactor": [0.8, 0.7, 0.6, a], "metallicFactor": 0, "roughnessFactor": 0.7},
                                                               **({"baseColorTexture": {"index": 0}} if tex else {}))}
    materials = [pbr(1), dict(pbr(1, True), alphaMode="MASK", alphaCutoff=0.6), dict(pbr(0.5, True), alphaMode="BLEND"),
                 dict(pbr(0), alphaMode="BLEND"), {"alphaMode": "BLEND"}]
    if not modes:
        materials = [{k: v for k, v in m.items() if k not in ("alphaMode", "alphaCutoff")} for m in materials]
    meshes = [mesh_of(k, m) for k, m in enumerate([0, 1, 2, 3, 4, None])]
    glb_io.write_glb(str(path), meshes, [{"mesh": k} for k in range(len(meshes))], materials, images=[glb_io.encode_png(img)], textures=[0])


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_the_loaders_table(tmp_path):
    ensure_addon()
    blend_glb(tmp_path / "blend.glb")
    blend_glb(tmp_path / "plain.glb", modes=False)
    script = tmp_path / "table.js"
    script.write_text(SCRIPT % dict(prep=json.dumps(os.path.join(HOST, "scene_prep.js")), gltf=json.dumps(os.path.join(HOST, "gltf.js")),
                                    glb=json.dumps(str(tmp_path / "blend.glb")), plain=json.dumps(str(tmp_path / "plain.glb"))))
    info = json.loads(subprocess.check_output([NODE, str(script)], text=True).strip().splitlines()[-1])
    # one entry per primitive's material: baseColorFactor[3] (default 1) for BLEND, -1 otherwise
    assert info["blend"]["blend"] == info["both"]["blend"] == [-1, -1, 0.5, 0, 1, -1]
    assert info["of"] == [-1, -1, -1, 1, 0.25]
    assert info["opaqueOnly"] is None                                       # no BLEND material: no table
    # alphaCutout alone: today's table, today's opaque BLEND, and no blend table at all
    assert info["cut"]["blend"] == info["none"]["blend"] == "undefined"
    cutoff = np.float32(info["cut"]["cutoff"])
    assert np.array_equal(cutoff, np.float32([0, 0.6, 0, 0, 0, 0])) and info["both"]["cutoff"] == info["cut"]["cutoff"]
    assert info["none"]["cutoff"] is None and info["blend"]["cutoff"] is None
    # the blobs never change; the atlas keeps albedo alpha when either option is set, and is opaque without
    for k in ("cut", "blend", "both"):
        assert info[k]["blobs"] == info["none"]["blobs"], k
    assert info["blend"]["rgba8"] == info["cut"]["rgba8"] == info["both"]["rgba8"] != info["none"]["rgba8"]
    import base64
    none8 = np.frombuffer(base64.b64decode(info["none"]["rgba8"]), np.uint8).reshape(-1, 4)
    kept8 = np.frombuffer(base64.b64decode(info["blend"]["rgba8"]), np.uint8).reshape(-1, 4)
    assert (none8[:, 3] == 255).all() and np.array_equal(none8[:, :3], kept8[:, :3])
    assert set(np.unique(kept8[:, 3]).tolist()) >= {64, 255}
