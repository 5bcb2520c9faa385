"""The participating medium through the Node host: Renderer.setMedium gives the bits of the C ABI's render of the same medium,
setMedium(null) the bits of the plain render, and `render_cli.js --fog` fills the scene's root box."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ptmi import layout, native, scene_io, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 64, 48, 4
FOG = dict(sigma_t=0.5, albedo=(0.9, 0.8, 0.7), g=0.3)

SCRIPT = """
var fs = require('fs');
var host = require(%(renderer)s);
var r = new host.Renderer({ width: %(W)d, height: %(H)d, options: { maxBounces: 8, doMis: 1 } });
function render(path) {
  while (r.frameIndex < %(F)d) r.renderFrame(2);
  fs.writeFileSync(path, Buffer.from(r.readOutput().buffer));
}
r.loadModel(%(scene)s).then(function () {
  r.setMedium({ sigmaT: 0.5, albedo: [0.9, 0.8, 0.7], g: 0.3, bounds: 'scene' });
  render(%(fog)s);
  r.setMedium({ sigmaT: 0.5, albedo: [0.9, 0.8, 0.7], g: 0.3, bounds: { min: %(lo)s, max: %(hi)s } });
  render(%(fog_box)s);
  var threw = false;
  try { r.setMedium({ sigmaT: -1, bounds: 'scene' }); } catch (e) { threw = /ptmi_set_medium failed \\(-1\\)/.test(String(e)); }
  r.frameIndex = 0;
  render(%(kept)s);
  r.setMedium(null);
  render(%(clear)s);
  console.log(JSON.stringify({ threw: threw }));
  r.destroy();
});
"""


def ensure_addon():
    if not os.path.exists(os.path.join(HOST, "addon", "ptmi_napi.node")):             # normally built by the project's build step
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "wgpu-path-tracing_amd"), "all"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(HOST, "addon")], stdout=subprocess.DEVNULL)


def reference_renders(sc, box):
    cam = layout.make_camera(W, H)
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=8, do_mis=1)
        ctx.set_medium(box=box, **FOG)
        ctx.dispatch(cam, FRAMES)
        fog = ctx.read_output()
        ctx.set_medium(None)
        ctx.dispatch(cam, FRAMES)
        clear = ctx.read_output()
    return fog, clear


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_set_medium_gives_the_bits_of_the_c_abi(tmp_path):
    ensure_addon()
    sc = scenes.make("cornell")
    scene_io.save_ptscene(sc, str(tmp_path / "cornell.ptscene"))
    lo, hi = [float(v) for v in sc.nodes[0]["aabb_min"]], [float(v) for v in sc.nodes[0]["aabb_max"]]
    paths = {k: str(tmp_path / (k + ".f32")) for k in ("fog", "fog_box", "kept", "clear")}
    script = tmp_path / "fog.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), W=W, H=H, F=FRAMES,
                                    scene=json.dumps(str(tmp_path / "cornell.ptscene")), lo=json.dumps(lo), hi=json.dumps(hi),
                                    **{k: json.dumps(v) for k, v in paths.items()}))
    out = subprocess.check_output([NODE, str(script)], text=True, timeout=300)
    info = json.loads(out.strip().splitlines()[-1])
    got = {k: np.fromfile(v, np.float32).reshape(H, W, 4) for k, v in paths.items()}
    fog, clear = reference_renders(sc, (tuple(lo), tuple(hi)))
    assert info["threw"]                                     # a bad field is the library's error ...
    assert same(got["kept"], fog)                            # ... and the medium in place stays
    assert same(got["fog"], fog) and same(got["fog_box"], fog)
    assert same(got["clear"], clear)                         # setMedium(null): the plain render's bits
    assert not same(fog, clear)


def test_cli_fog_fills_the_scenes_box(tmp_path):
    ensure_addon()
    sc = scenes.make("cornell")
    scene_io.save_ptscene(sc, str(tmp_path / "cornell.ptscene"))
    subprocess.check_output([NODE, os.path.join(HOST, "render_cli.js"), str(tmp_path / "cornell.ptscene"), str(tmp_path / "out.f32"),
                             "--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--batch", "2", "--fog", "0.5,0.75,0.3"],
                            text=True, timeout=300)
    got = np.fromfile(tmp_path / "out.f32", np.float32).reshape(H, W, 4)
    cam = layout.make_camera(W, H)
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=8, do_mis=1)
        ctx.set_medium(sigma_t=0.5, albedo=0.75, g=0.3, box=(tuple(sc.nodes[0]["aabb_min"]), tuple(sc.nodes[0]["aabb_max"])))
        ctx.dispatch(cam, FRAMES)
        want = ctx.read_output()
    assert same(got, want)
