"""ptmi_rebuild_tree through the Node host: Renderer.rebuildTree() returns the status and renders what the C ABI renders after the same
update and rebuild; the opt-in constructor option rebuildAbove triggers exactly one rebuild when an edit leaves the cost ratio above it,
and none when it is left unset."""
import json
import os
import subprocess

import numpy as np
import pytest

import scene_update_ref as ref
from ptmi import layout, native, scene_io, scenes
from test_node_scene_update import HOST, NODE, ensure_addon, same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 64, 48, 4

SCRIPT = """
var fs = require('fs');
var host = require(%(renderer)s);
function bytes(path) { var b = fs.readFileSync(path); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); }
function render(r, path) {
  while (r.frameIndex < %(F)d) r.renderFrame(2);
  fs.writeFileSync(path, Buffer.from(r.readOutput().buffer));
}
function make(extra) {
  var o = { width: %(W)d, height: %(H)d, options: { maxBounces: 8, doMis: 1, leaves: 2, treeBuilder: 1 } };
  for (var k in extra) o[k] = extra[k];
  return new host.Renderer(o);
}
var info = {};
var r = make({});
r.loadModel(%(scene)s).then(function () {
  try { r.rebuildTree({ builder: 3 }); } catch (e) { info.threw = /ptmi_rebuild_tree failed \\(-1\\)/.test(String(e)); }
  info.none = r.rebuildStatus();
  r.updateTriangles(0, bytes(%(tris)s));
  info.update = r.sceneUpdateStatus();
  info.unset = r.rebuildStatus();
  render(r, %(refitted)s);
  info.framesBefore = r.frameIndex;
  info.status = r.rebuildTree();
  info.framesAfter = r.frameIndex;
  info.updateAfter = r.sceneUpdateStatus();
  r.resetOutputBuffer(false);
  render(r, %(rebuilt)s);
  r.destroy();
  var a = make({ rebuildAbove: %(below)s });
  return a.loadModel(%(scene)s).then(function () {
    a.updateTriangles(0, bytes(%(tris)s));
    info.auto = a.rebuildStatus();
    info.autoUpdate = a.sceneUpdateStatus();
    render(a, %(auto)s);
    a.destroy();
    var b = make({ rebuildAbove: %(above)s });
    return b.loadModel(%(scene)s).then(function () {
      b.updateTriangles(0, bytes(%(tris)s));
      info.notYet = b.rebuildStatus();
      b.destroy();
      console.log(JSON.stringify(info));
    });
  });
});
"""


def test_rebuild_through_the_renderer(tmp_path):
    ensure_addon()
    sc = scenes.make("cornell_spheres")
    moved = ref.deformed(sc.tris, "wobble")
    cam = layout.make_camera(W, H)
    with native.Context(0) as ctx:                               # the C ABI's renders of the same edit, and the ratio it produces
        ctx.set_options(max_bounces=8, do_mis=1, leaves=2, tree_builder=1)
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.update_triangles(0, moved)
        up = ctx.scene_update_status()
        ratio = up.cost_now / up.cost_built
        assert ratio > 1.0, "the edit must degrade the refitted tree for rebuildAbove to have something to decide"
        ctx.dispatch(cam, FRAMES)
        want_refitted = ctx.read_output()
        st = ctx.rebuild_tree()
        ctx.write_output(np.zeros((H, W, 4), np.float32))
        ctx.dispatch(cam, FRAMES)
        want_rebuilt = ctx.read_output()
    scene_io.save_ptscene(sc, str(tmp_path / "scene.ptscene"))
    moved.tofile(tmp_path / "tris.bin")
    paths = {k: str(tmp_path / (k + ".f32")) for k in ("refitted", "rebuilt", "auto")}
    script = tmp_path / "rebuild.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), W=W, H=H, F=FRAMES,
                                    scene=json.dumps(str(tmp_path / "scene.ptscene")), tris=json.dumps(str(tmp_path / "tris.bin")),
                                    below=repr(1.0 + (ratio - 1.0) / 2), above=repr(ratio * 1.5),
                                    **{k: json.dumps(v) for k, v in paths.items()}))
    out = subprocess.check_output([NODE, str(script)], text=True, timeout=300)
    info = json.loads(out.strip().splitlines()[-1])
    got = {k: np.fromfile(v, np.float32).reshape(H, W, 4) for k, v in paths.items()}
    assert info["threw"] and info["none"]["rebuilds"] == 0 and info["unset"]["rebuilds"] == 0       # left unset: no rebuild
    assert info["update"]["costNow"] == up.cost_now and info["update"]["costBuilt"] == up.cost_built
    s = info["status"]
    assert s["rebuilds"] == 1 and s["builderUsed"] == st.builder_used == 1 and s["buildMs"] > 0
    assert s["costBefore"] == st.cost_before == up.cost_now and s["costAfter"] == st.cost_after
    assert info["updateAfter"]["costBuilt"] == info["updateAfter"]["costNow"] == st.cost_after and info["updateAfter"]["updates"] == 1
    assert info["framesBefore"] == info["framesAfter"] == FRAMES       # the hits do not depend on the tree: accumulation continues
    # the same radiance as the ctypes path; a rebuild changes the tree, not the bits
    assert same(got["refitted"], want_refitted) and same(got["rebuilt"], want_rebuilt) and same(got["rebuilt"], got["refitted"])
    # rebuildAbove below the ratio the edit produces: exactly one rebuild; above it: none
    assert info["auto"]["rebuilds"] == 1 and info["auto"]["costAfter"] == st.cost_after
    assert info["autoUpdate"]["costBuilt"] == info["autoUpdate"]["costNow"] == st.cost_after
    assert same(got["auto"], want_rebuilt)
    assert info["notYet"]["rebuilds"] == 0
