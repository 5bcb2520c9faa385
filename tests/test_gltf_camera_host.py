"""The glTF loader's cameras (host/gltf.js, host/scene_prep.js sceneCameras, host/renderer.js lookThrough, host/pack.js packCamera)
without a GPU: the two cameras of tests/gltf_camera_scene.py, under rotated, translated, nested nodes, come back with the world
position and basis of the float64 matrices composed in numpy, with the file's yfov / aspectRatio / znear and xmag / ymag, and pack
into the 96-byte camera record with the projection words include/ptmi_layout.h defines."""
import json
import os
import subprocess

import numpy as np
import pytest

import gltf_camera_scene as G
from ptmi import layout
from test_gltf_host import HOST, NODE, _build, prepare

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

W, H = 48, 32
SCRIPT = """
var host = require(%(renderer)s), prep = require(%(prep)s), gltf = require(%(gltf)s).loadGLB(%(glb)s);
var s = prep.prepareScene(gltf);
var info = { cameras: s.cameras, nGltfCameras: gltf.cameras.length, nodeCamera: gltf.nodes.map(function (n) { return n.camera ? n.camera.type : null; }) };
info.packed = s.cameras.map(function (c) {
  var cam = { position: [0, 1, 2.8], forward: [0, 0, -1], right: [1, 0, 0], up: [0, 1, 0], fov: Math.PI / 3, aspect: %(w)d / %(h)d,
              width: %(w)d, height: %(h)d, frameIndex: 3, focusDistance: 5.0, aperture: 0.001 };
  var kind = host.lookThrough(cam, c);
  return { kind: kind, hex: Buffer.from(host.pack.packCamera(cam)).toString('hex') };
});
info.plain = Buffer.from(host.pack.packCamera({ position: [0, 1, 2.8], forward: [0, 0, -1], right: [1, 0, 0], up: [0, 1, 0], fov: 1, aspect: 1.5,
  width: 3, height: 2, frameIndex: 0, focusDistance: 5.0, aperture: 0.001 })).toString('hex');
try { host.pack.packCamera({ position: [0, 0, 0], forward: [0, 0, -1], right: [1, 0, 0], up: [0, 1, 0], projection: 'fisheye' }); info.unknown = 'no error'; }
catch (e) { info.unknown = String(e.message); }
console.log(JSON.stringify(info));
"""


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    _build()
    d = tmp_path_factory.mktemp("cams")
    world = G.write_scene(d / "cams.glb")
    script = d / "cams.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), prep=json.dumps(os.path.join(HOST, "scene_prep.js")),
                                    gltf=json.dumps(os.path.join(HOST, "gltf.js")), glb=json.dumps(str(d / "cams.glb")), w=W, h=H))
    js = json.loads(subprocess.check_output([NODE, str(script)], text=True).strip().splitlines()[-1])
    return d, world, js


def test_cameras_are_listed_with_their_world_basis(loaded):
    d, world, js = loaded
    cams = js["cameras"]
    assert js["nGltfCameras"] == 2 and [c["type"] for c in cams] == ["perspective", "orthographic"]
    assert [c["name"] for c in cams] == ["hero", "elevation"] and [c["node"] for c in cams] == [G.PERSPECTIVE_NODE, G.ORTHO_NODE]
    assert [c["camera"] for c in cams] == [0, 1]
    assert js["nodeCamera"] == [None, None, None, "perspective", None, None, "orthographic"]
    for c in cams:
        pos, fw, rt, up = G.basis_of(world[c["camera"]])
        # the host composes in float32 (three nested matrices): a few float32 roundings of values up to ~4
        for got, want in ((c["position"], pos), (c["forward"], fw), (c["right"], rt), (c["up"], up)):
            assert np.abs(np.asarray(got) - want).max() < 4e-6, (c["name"], got, want)
        B = np.array([c["forward"], c["right"], c["up"]])
        assert np.abs(B @ B.T - np.eye(3)).max() < 1e-6                  # orthonormal: what projections 1 and 2 expect
        assert np.allclose(np.cross(c["right"], c["up"]), -np.asarray(c["forward"]), atol=1e-6)
    p, o = cams
    assert (p["yfov"], p["aspectRatio"], p["znear"]) == (G.YFOV, G.ASPECT, G.ZNEAR) and "ymag" not in p
    assert (o["xmag"], o["ymag"], o["znear"], o["zfar"]) == (G.XMAG, G.YMAG, G.ZNEAR, 50.0) and "yfov" not in o


def test_prepare_cli_reports_the_cameras(loaded):
    d, world, js = loaded
    sc, info = prepare(d / "cams.glb", d / "out")
    assert info["cameras"] == js["cameras"]
    assert info["counts"]["triangles"] == 2 + 2 + 12                    # the camera nodes add no geometry


def test_scene_cameras_pack_into_the_record(loaded):
    d, world, js = loaded
    f32 = np.float32
    for c, packed in zip(js["cameras"], js["packed"]):
        rec = np.frombuffer(bytes.fromhex(packed["hex"]), layout.CAMERA)[0]
        for k in ("position", "forward", "right", "up"):
            assert np.array_equal(rec[k], np.asarray(c[k], f32)), k
        # the frame's aspect, not the file's: the vertical extent is what is kept
        assert (rec["width"], rec["height"], rec["frame_index"]) == (W, H, 3) and rec["aspect"] == f32(W / H)
        assert rec["aperture"] == f32(0.001) and rec["focus_distance"] == f32(5.0)
        words = rec["_p3"]
        if c["type"] == "orthographic":
            assert packed["kind"] == "orthographic" and words[0] == layout.PROJ_ORTHOGRAPHIC
            assert words[1:2].view(f32)[0] == f32(G.YMAG) and rec["fov"] == f32(np.pi / 3)          # fov is left alone
            assert rec.tobytes() == layout.set_projection(rec.copy(), "orthographic", G.YMAG).tobytes()
        else:
            assert packed["kind"] == "perspective" and words.tolist() == [0, 0] and rec["fov"] == f32(G.YFOV)
    plain = np.frombuffer(bytes.fromhex(js["plain"]), layout.CAMERA)[0]
    want = layout.make_camera(3, 2, fov=1.0, aspect=1.5)
    assert plain.tobytes() == want.tobytes()                            # a camera without the two fields packs zero words, as before
    assert "unknown projection fisheye" in js["unknown"]
