"""Morph targets through the Node host: Renderer.poseAt on the file of tests/gltf_morph_scene.py (a skinned bar with two targets, a
collar with one under a rotated, scaled node, weights channels) poses the morph first and the skin second, and renders what the Python
path (the C ABI through ptmi.native) renders with the model's weights and joint matrices at the same key; Renderer.setMorph /
poseMorph by hand give the same bytes, a pose the host checks refuse throws and changes nothing (the refusals of the device's check pass
are tests/test_gpu_morph.py's: no weight takes this file's small deltas out of float32), and two devices behind one Renderer give the same
frame."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import gltf_morph_scene as face
import gltf_skin_scene as bar
import morph_ref as mref
import skin_ref as sref
import transform_ref as tref
from ptmi import glb_io, layout, native
from test_node_scene_update import ensure_addon, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 64, 48, 4

POSE_AT = """
var fs = require('fs');
var host = require(%(renderer)s);
function render(r, path) {
  while (r.frameIndex < %(F)d) r.renderFrame(2);
  fs.writeFileSync(path, Buffer.from(r.readOutput().buffer));
}
var info = {};
var r = new host.Renderer({ width: %(W)d, height: %(H)d, options: { maxBounces: 8, doMis: 1 } });
r.loadModel(%(glb)s).then(function () {
  info.loaded = r.morphStatus();
  r.poseAt(0, 1.0);
  info.posed = r.morphStatus();
  info.skin = r.skinStatus();
  info.updates = r.sceneUpdateStatus().updates;
  info.frameAfter = r.frameIndex;
  render(r, %(at)s);
  // the same pose by hand: absolute, so the same bytes
  var weights = %(weights)s;
  r.poseMorph(weights);
  info.stale = r.morphStatus().skinStale;
  r.poseAt(0, 1.0);
  render(r, %(again)s);
  var before = r.morphStatus();
  try { r.poseMorph(weights.slice(1)); } catch (e) { info.threw = /ptmi_pose_morph failed \\(-1\\)/.test(String(e)); }
  try { r.poseMorph([0.5, NaN, 0.5]); } catch (e) { info.threwOnNaN = /ptmi_pose_morph failed \\(-1\\)/.test(String(e)); }
  info.statusKept = JSON.stringify(r.morphStatus()) === JSON.stringify(before);
  r.resetOutputBuffer(false);
  render(r, %(kept)s);
  r.setMorph(null, null, null, 0);
  info.removed = r.morphStatus();
  r.destroy();
  var m = new host.Renderer({ width: %(W)d, height: %(H)d, devices: [0, 0], loopback: true, options: { maxBounces: 8, doMis: 1 } });
  return m.loadModel(%(glb)s).then(function () {
    m.poseAt(0, 1.0);
    info.multi = m.morphStatus();
    render(m, %(multi)s);
    m.destroy();
    console.log(JSON.stringify(info));
  });
});
"""


def test_pose_at_renders_what_the_python_path_renders_with_the_models_weights(tmp_path):
    ensure_addon()
    face.write_face(tmp_path / "face.glb")
    os.makedirs(tmp_path / "out")
    subprocess.check_call([NODE, os.path.join(HOST, "prepare_cli.js"), str(tmp_path / "face.glb"), str(tmp_path / "out")], stdout=subprocess.DEVNULL)
    sc = glb_io.load_blob_dir(str(tmp_path / "out"))
    s_list = np.fromfile(tmp_path / "out" / "skin_triangles.bin", np.uint32)
    corners = np.fromfile(tmp_path / "out" / "skin_corners.bin", layout.SKIN_CORNER)
    m_list = np.fromfile(tmp_path / "out" / "morph_triangles.bin", np.uint32)
    rows = np.fromfile(tmp_path / "out" / "morph_rows.bin", np.uint32)
    deltas = np.fromfile(tmp_path / "out" / "morph_deltas.bin", layout.MORPH_DELTA)
    # the animation at its key at 1 s, from the files' float64 models: exact factors, so the float32 records are the host's
    weights = np.array(face.BAR_KEYS[1] + face.COLLAR_KEYS[1], np.float32)
    joints = [(m, None) for m in bar.joint_matrices(bar.KEY_T[1], bar.Q120, [1.0, 1.5, 1.0])]
    paths = {k: str(tmp_path / (k + ".f32")) for k in ("at", "again", "kept", "multi")}
    script = tmp_path / "pose_at.js"
    script.write_text(POSE_AT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), W=W, H=H, F=FRAMES,
                                     glb=json.dumps(str(tmp_path / "face.glb")), weights=json.dumps([float(w) for w in weights]),
                                     **{k: json.dumps(v) for k, v in paths.items()}))
    info = json.loads(subprocess.check_output([NODE, str(script)], text=True, timeout=300).strip().splitlines()[-1])
    got = {k: np.fromfile(v, np.float32).reshape(H, W, 4) for k, v in paths.items()}
    in_skin = int(np.isin(m_list, s_list).sum())
    assert in_skin == len(s_list) == 64 and len(m_list) == 64 + 12
    loaded = dict(present=1, nTargets=face.N_TARGETS, nMorphed=len(m_list), nRecords=len(deltas), nInSkin=in_skin, poses=0, activeTargets=0,
                  firstBad=0xFFFFFFFF, skinStale=0, poseMs=0)
    assert info["loaded"] == loaded
    assert info["posed"] == dict(loaded, poses=1, activeTargets=3, poseMs=info["posed"]["poseMs"]) and info["posed"]["poseMs"] > 0
    assert info["skin"]["poses"] == 1 and info["updates"] == 2 and info["frameAfter"] == 0 and info["stale"] == 1
    assert info["threw"] and info["threwOnNaN"] and info["statusKept"]
    assert info["removed"] == dict(present=0, nTargets=0, nMorphed=0, nRecords=0, nInSkin=0, poses=0, activeTargets=0, firstBad=0,
                                   skinStale=0, poseMs=0)
    assert info["multi"]["poses"] == 1 and info["multi"]["nMorphed"] == len(m_list)
    cam = layout.make_camera(W, H)
    rest = tref.rest_of(sc.tris)
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=8, do_mis=1)
        ctx.dispatch(cam, FRAMES)
        unposed = ctx.read_output()
        ctx.set_skin(s_list, corners, 2)
        ctx.set_morph(m_list, rows, deltas, face.N_TARGETS)
        ctx.pose_morph(weights)
        ctx.pose_skin(native.joint_ops(joints))
        moved = ctx.read_triangles()
        ctx.dispatch(cam, FRAMES)
        want = ctx.read_output()
    morphed = mref.morphed(sc.tris, rest, m_list, rows, deltas, weights)
    assert moved.tobytes() == sref.skinned(morphed, tref.rest_of(morphed), s_list, corners, joints).tobytes()
    assert morphed[m_list].tobytes() != sc.tris[m_list].tobytes()
    assert same(got["at"], want) and same(got["again"], want) and same(got["kept"], want) and same(got["multi"], want)
    assert not same(unposed, want)
