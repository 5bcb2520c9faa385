"""Triangle groups through the Node host: Renderer.setTriangleGroups / transformGroups give the output bytes of the Python path (the
C ABI through ptmi.native), with normalMatrix omitted (derived through ptmi_normal_matrix) and with it passed from the model of
tests/transform_ref.py; several devices behind one Renderer give the same frame; a refused call throws and changes nothing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import transform_ref as ref
from ptmi import layout, native, scene_io, scenes
from test_node_scene_update import ensure_addon, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 64, 48, 4

SCRIPT = """
var fs = require('fs');
var host = require(%(renderer)s);
var ops = %(ops)s, groups = new Uint32Array(%(groups)s);
function render(r, path) {
  while (r.frameIndex < %(F)d) r.renderFrame(2);
  fs.writeFileSync(path, Buffer.from(r.readOutput().buffer));
}
function strip(list) { return list.map(function (o) { return { group: o.group, matrix: o.matrix }; }); }
var info = {};
var r = new host.Renderer({ width: %(W)d, height: %(H)d, options: { maxBounces: 8, doMis: 1 } });
r.loadModel(%(scene)s).then(function () {
  try { r.transformGroups(ops); } catch (e) { info.noTable = /ptmi_transform_groups failed \\(-4\\)/.test(String(e)); }
  render(r, %(base)s);
  r.setTriangleGroups(groups);
  r.transformGroups(strip(ops));                       // normalMatrix derived
  info.frameAfter = r.frameIndex;
  info.bounds = r.sceneBounds;
  info.status = r.transformStatus();
  info.updates = r.sceneUpdateStatus().updates;
  render(r, %(derived)s);
  r.transformGroups(ops);                              // the same matrices with the model's normalMatrix: absolute, so the same bytes
  render(r, %(passed)s);
  try { r.transformGroups([{ group: 99, matrix: ops[0].matrix }]); } catch (e) { info.threw = /ptmi_transform_groups failed \\(-1\\)/.test(String(e)); }
  info.statusAfterRefusal = r.transformStatus();
  r.destroy();
  var m = new host.Renderer({ width: %(W)d, height: %(H)d, devices: [0, 0], loopback: true, options: { maxBounces: 8, doMis: 1 } });
  return m.loadModel(%(scene)s).then(function () {
    m.setTriangleGroups(groups);
    m.transformGroups(strip(ops));
    info.multiStatus = m.transformStatus();
    render(m, %(multi)s);
    m.destroy();
    console.log(JSON.stringify(info));
  });
});
"""


def test_transforms_through_node_render_what_the_python_path_renders(tmp_path):
    ensure_addon()
    sc = scenes.make("cornell")
    groups = np.random.default_rng(11).integers(0, 5, len(sc.tris)).astype(np.uint32)
    ops = [ref.op(1, ref.affine(ref.rot_y(0.4), shift=(0.05, 0.02, -0.03))), ref.op(3, ref.affine(scale=(3, 0.5, 1)))]
    js_ops = [dict(group=g, matrix=[float(x) for x in m], normalMatrix=[float(x) for x in nm]) for g, m, nm in ops]
    scene_io.save_ptscene(sc, str(tmp_path / "cornell.ptscene"))
    paths = {k: str(tmp_path / (k + ".f32")) for k in ("base", "derived", "passed", "multi")}
    script = tmp_path / "transform.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), W=W, H=H, F=FRAMES, ops=json.dumps(js_ops),
                                    groups=json.dumps(groups.tolist()), scene=json.dumps(str(tmp_path / "cornell.ptscene")),
                                    **{k: json.dumps(v) for k, v in paths.items()}))
    out = subprocess.check_output([NODE, str(script)], text=True, timeout=300)
    info = json.loads(out.strip().splitlines()[-1])
    got = {k: np.fromfile(v, np.float32).reshape(H, W, 4) for k, v in paths.items()}
    cam = layout.make_camera(W, H)
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=8, do_mis=1)
        ctx.set_triangle_groups(groups)
        ctx.transform_groups(native.group_ops(ops))
        ctx.dispatch(cam, FRAMES)
        want = ctx.read_output()
        st = ctx.transform_status()
        root = ctx.scene_update_status()
    assert same(got["derived"], want) and same(got["passed"], want) and same(got["multi"], want)
    assert not same(got["base"], want)
    assert info["noTable"] and info["threw"] and info["frameAfter"] == 0 and info["updates"] == 1
    assert info["status"] == dict(present=1, nGroups=5, transforms=1, lastMoved=st.last_moved, firstBad=0xFFFFFFFF,
                                  transformMs=info["status"]["transformMs"])
    assert info["statusAfterRefusal"]["transforms"] == 2 and info["multiStatus"]["transforms"] == 1
    assert np.array_equal(np.float32(info["bounds"]["min"]), np.array(root.root_min, np.float32))
    assert np.array_equal(np.float32(info["bounds"]["max"]), np.array(root.root_max, np.float32))
