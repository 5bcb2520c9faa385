"""Lightmap baking through the Node host: Renderer.bake on a small .glb with TEXCOORD_1 gives the bits of the ctypes path with
ptmi.bake.rasterise of the same mesh, before and after dilate: 2. Also here: the loader carries TEXCOORD_1 through the builder's
reorder, the frame takes the lightmap's size, and a bake with a first-hit plane on throws."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ptmi import bake, glb_io, layout, native, scenes
from test_gltf_host import mesh_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES, GRID = 24, 20, 3, 6

SCRIPT = """
var fs = require('fs');
var host = require(%(renderer)s);
var dir = %(dir)s;
function dump(name, a) { fs.writeFileSync(dir + '/' + name, Buffer.from(a.buffer || a, a.byteOffset || 0, a.byteLength)); }
var info = {};
var r = new host.Renderer({ width: 32, height: 16, options: { maxBounces: 4, doMis: 1 } });
r.loadModel(%(glb)s).then(function () {
  var b = r.sceneInfo.blobs;
  dump('triangles.bin', b.triangles); dump('materials.bin', b.materials); dump('nodes.bin', b.bvhNodes); dump('lights.bin', b.lights);
  dump('lightmap.f32', r.lightmapUvs);
  r.renderFrame(2);
  dump('plain.f32', r.bake({ width: %(W)d, height: %(H)d, frames: %(F)d }));
  info.first = r.lastBake; info.size = [r.width, r.height]; info.frameIndex = r.frameIndex;
  dump('dilated.f32', r.bake({ frames: %(F)d, dilate: 2 }));
  info.second = r.lastBake;
  r.setAovs(['id']);
  try { r.bake({ frames: 1 }); } catch (e) { info.threw = String(e); }
  r.setAovs([]);
  r.renderFrame(1);                          // the camera renders again afterwards
  info.frameAfter = r.frameIndex;
  r.destroy();
  console.log(JSON.stringify(info));
});
"""


def ensure_addon():
    if not os.path.exists(os.path.join(HOST, "addon", "ptmi_napi.node")):             # normally built by the project's build step
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "wgpu-path-tracing_amd"), "all"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(HOST, "addon")], stdout=subprocess.DEVNULL)


def lightmapped_glb(path):
    """a floor, an emissive panel above it and a box, every triangle with a cell of its own in a GRID x GRID lightmap (TEXCOORD_1: the
    lower-left half of the cell, inset); TEXCOORD_0 is something else. Returns {vertex positions' bytes: the triangle's TEXCOORD_1}."""
    parts = [scenes._quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0), 0),
             scenes._quad((-0.4, 1.6, -0.4), (0.4, 1.6, -0.4), (0.4, 1.6, 0.4), (-0.4, 1.6, 0.4), (0, -1, 0), 0),
             scenes._box((0.2, 0.3, -0.1), (0.5, 0.6, 0.5), 0)]
    materials = [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1], "metallicFactor": 0, "roughnessFactor": 0.6}},
                 {"emissiveFactor": [1, 0.9, 0.7], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 8.0}},
                  "pbrMetallicRoughness": {"metallicFactor": 0, "roughnessFactor": 0.5}},
                 {"pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.3, 0.2, 1], "metallicFactor": 0, "roughnessFactor": 0.4}}]
    meshes, expect, t = [], {}, 0
    for k, tris in enumerate(parts):
        m = mesh_of(tris, k)
        uv1 = np.zeros((len(tris) * 3, 2), np.float32)
        for j in range(len(tris)):
            cx, cy = (t % GRID) / GRID, (t // GRID) / GRID
            uv1[3 * j:3 * j + 3] = [(cx + 0.01, cy + 0.01), (cx + 0.15, cy + 0.01), (cx + 0.01, cy + 0.15)]
            expect[m["positions"][3 * j:3 * j + 3].astype(np.float32).tobytes()] = uv1[3 * j:3 * j + 3].copy()
            t += 1
        m["uvs1"] = uv1
        meshes.append(m)
    assert t <= GRID * GRID
    glb_io.write_glb(path, meshes, [{"mesh": i} for i in range(len(meshes))], materials)
    return expect


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_renderer_bake_matches_the_c_abi(tmp_path):
    ensure_addon()
    expect = lightmapped_glb(str(tmp_path / "room.glb"))
    script = tmp_path / "bake.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), dir=json.dumps(str(tmp_path)),
                                    glb=json.dumps(str(tmp_path / "room.glb")), W=W, H=H, F=FRAMES))
    out = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dt)
    sc = scenes.Scene("room", rd("triangles.bin", layout.TRIANGLE), rd("materials.bin", layout.MATERIAL), rd("nodes.bin", layout.BVH_NODE),
                      rd("lights.bin", layout.LIGHT), None)
    uvs = rd("lightmap.f32", np.float32).reshape(-1, 3, 2)
    # the loader: every uploaded triangle carries the TEXCOORD_1 of the triangle it was, whatever the builder did to the order
    assert len(uvs) == len(sc.tris) == len(expect)
    for i, t in enumerate(sc.tris):
        key = np.stack([t["v0"], t["v1"], t["v2"]]).astype(np.float32).tobytes()
        assert same(uvs[i], expect[key]), i
    assert not same(uvs, np.stack([sc.tris["uv0"], sc.tris["uv1"], sc.tris["uv2"]], axis=1))      # and not TEXCOORD_0
    pos, nrm, _ = bake.scene_arrays(sc)
    tex = bake.rasterise(pos, nrm, uvs, W, H)
    covered = int((tex["covered"] != 0).sum())
    assert 0 < covered < W * H
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=4, do_mis=1)
        ctx.upload_bake_surface(tex)
        ctx.dispatch_bake(FRAMES)
        want, want_dilated = ctx.read_output(), ctx.bake_dilate(2)
    got, got_dilated = rd("plain.f32", np.float32).reshape(H, W, 4), rd("dilated.f32", np.float32).reshape(H, W, 4)
    assert same(got, want) and same(got_dilated, want_dilated)
    assert want[..., :3].max() > 0.05 and (want_dilated[..., 3] == 2).any() and not same(got, got_dilated)
    assert info["first"] == dict(width=W, height=H, frames=FRAMES, covered=covered) and info["second"] == info["first"]
    assert info["size"] == [W, H] and info["frameIndex"] == 0 and info["frameAfter"] == 1
    assert "first-hit planes" in info.get("threw", "")
