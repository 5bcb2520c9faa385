"""The lightmap filter through the Node host: Renderer.bake({denoise, dilate: 2}) on tests/test_node_bake.py's small .glb gives the
bytes the ctypes path gives for the same surface and parameters, records lastBake.denoised, and leaves the renderer's moments switch
as it was - off where it was off, on where adaptive sampling had it on."""
import json
import os
import subprocess

import numpy as np
import pytest

from ptmi import bake, layout, native, scenes
from test_node_bake import FRAMES, H, HOST, NODE, W, ensure_addon, lightmapped_glb, same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

PARAMS = dict(iterations=3, phiColor=2.0, phiNormal=16.0, phiPosition=1.5)

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
  info.momentsBefore = r.addon.getMoments(r.ctx);
  dump('defaults.f32', r.bake({ width: %(W)d, height: %(H)d, frames: %(F)d, denoise: true, dilate: 2 }));
  info.first = r.lastBake; info.momentsAfter = r.addon.getMoments(r.ctx);
  dump('chosen.f32', r.bake({ frames: %(F)d, denoise: %(params)s, dilate: 2 }));
  dump('plain.f32', r.bake({ frames: %(F)d, dilate: 2 }));
  info.plain = r.lastBake;
  r.addon.setMoments(r.ctx, true);            // a switch that is on stays on
  dump('again.f32', r.bake({ frames: %(F)d, denoise: true, dilate: 2 }));
  info.momentsKept = r.addon.getMoments(r.ctx);
  r.destroy();
  console.log(JSON.stringify(info));
});
"""


def test_renderer_bake_denoise_matches_the_c_abi(tmp_path):
    ensure_addon()
    lightmapped_glb(str(tmp_path / "room.glb"))
    script = tmp_path / "bake.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), dir=json.dumps(str(tmp_path)),
                                    glb=json.dumps(str(tmp_path / "room.glb")), W=W, H=H, F=FRAMES, params=json.dumps(PARAMS)))
    out = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dt)
    sc = scenes.Scene("room", rd("triangles.bin", layout.TRIANGLE), rd("materials.bin", layout.MATERIAL), rd("nodes.bin", layout.BVH_NODE),
                      rd("lights.bin", layout.LIGHT), None)
    pos, nrm, _ = bake.scene_arrays(sc)
    tex = bake.rasterise(pos, nrm, rd("lightmap.f32", np.float32).reshape(-1, 3, 2), W, H)
    covered = int((tex["covered"] != 0).sum())
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.set_moments(True)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=4, do_mis=1)
        ctx.upload_bake_surface(tex)
        ctx.dispatch_bake(FRAMES)
        want = ctx.bake_denoise(dilate=2)
        want_chosen = ctx.bake_denoise(iterations=3, dilate=2, phi_color=2.0, phi_normal=16.0, phi_position=1.5)
        want_plain = ctx.bake_dilate(2)
    got = {k: rd(k + ".f32", np.float32).reshape(H, W, 4) for k in ("defaults", "chosen", "plain", "again")}
    assert same(got["defaults"], want) and same(got["chosen"], want_chosen) and same(got["plain"], want_plain)
    assert same(got["again"], want)
    assert not same(want, want_plain) and not same(want, want_chosen) and (want[..., 3] == 2).any()
    assert info["first"] == dict(width=W, height=H, frames=FRAMES, covered=covered, denoised=True)
    assert info["plain"] == dict(width=W, height=H, frames=FRAMES, covered=covered)
    assert info["momentsBefore"] is False and info["momentsAfter"] is False and info["momentsKept"] is True
