"""Alpha cutouts through the Node host: new Renderer({alphaCutout: true}) loads a .glb with one alphaMode "MASK" material, keeps the
albedo map's alpha in the atlas, sets that material's cutoff, and renders the bits the C ABI renders from the same blobs and table;
with the option off, which is the default, the atlas and the output are what they are without this feature; and
`render_cli.js --alpha-cutout` runs."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import atlas_ref
from ptmi import glb_io, layout, native, scenes
from test_node_medium import HOST, ensure_addon, same

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 64, 48, 4

SCRIPT = """
var fs = require('fs'), path = require('path');
var host = require(%(renderer)s), prep = require(%(prep)s), gltf = require(%(gltf)s);
var dir = %(dir)s, glb = %(glb)s;
function dump(name, s) {
  Object.keys(s.blobs).forEach(function (k) { fs.writeFileSync(path.join(dir, name + '_' + k + '.bin'), Buffer.from(s.blobs[k])); });
  var a = s.atlas;
  fs.writeFileSync(path.join(dir, name + '_atlas.bin'), Buffer.from(a.data.buffer, a.data.byteOffset, a.data.byteLength));
  fs.writeFileSync(path.join(dir, name + '_rgba8.bin'), Buffer.from(a.rgba8.buffer, a.rgba8.byteOffset, a.rgba8.byteLength));
  return { width: a.width, height: a.height, cutoff: s.alphaCutoff ? Array.from(s.alphaCutoff) : null };
}
var info = { on: dump('on', prep.prepareScene(gltf.loadGLB(glb), { alphaCutout: true })), off: dump('off', prep.prepareScene(gltf.loadGLB(glb))) };
function run(opts, name, next) {
  var r = new host.Renderer(Object.assign({ width: %(W)d, height: %(H)d, options: { maxBounces: 8, doMis: 1 } }, opts));
  r.loadModel(glb).then(function () {
    function render(tag) {
      r.frameIndex = 0;
      while (r.frameIndex < %(F)d) r.renderFrame(2);
      fs.writeFileSync(path.join(dir, name + tag + '.f32'), Buffer.from(r.readOutput().buffer));
      return r.alphaStatus();
    }
    info[name] = render('');
    if (opts.alphaCutout) {
      r.setAlphaCutoff(null);
      info[name + 'Removed'] = render('_removed');
      try { r.setAlphaCutoff(new Float32Array(1)); } catch (e) { info[name + 'Threw'] = /set_alpha_cutoff failed \\(-1\\)/.test(String(e)); }
      r.setAlphaCutoff(new Float32Array(info.on.cutoff), { maxLayers: 2 });
      info[name + 'Again'] = render('_again');
    }
    r.destroy();
    next();
  });
}
run({ alphaCutout: true }, 'cut', function () {
  run({}, 'plain', function () {
    run({ alphaCutout: true, devices: [0, 0], loopback: true }, 'two', function () { console.log(JSON.stringify(info)); });
  });
});
"""


def mask_glb(path):
    """a floor, a back wall and a light panel, and in front of the wall a card whose material is alphaMode MASK over an RGBA image
    whose alpha is 0 in two of its four quadrants and 255 / 128 in the others (cutoff 0.6: the 128 quadrant is a hole too)"""
    rng = np.random.default_rng(3)
    img = rng.integers(64, 256, (16, 16, 4), dtype=np.uint8)
    img[:8, :8, 3], img[:8, 8:, 3], img[8:, :8, 3], img[8:, 8:, 3] = 255, 0, 128, 0
    quad = lambda a, b, c, d, n: scenes._quad(a, b, c, d, n, 0)

    def mesh_of(tris, material):
        pos = np.stack([tris["v0"], tris["v1"], tris["v2"]], 1).reshape(-1, 3)
        nrm = np.stack([tris["n0"], tris["n1"], tris["n2"]], 1).reshape(-1, 3)
        uv = np.stack([tris["uv0"], tris["uv1"], tris["uv2"]], 1).reshape(-1, 2)
        return {"positions": pos, "normals": nrm, "uvs": uv, "indices": np.arange(len(pos)), "material": material}

    floor = quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0))
    back = quad((-1, 0, -1), (-1, 2, -1), (1, 2, -1), (1, 0, -1), (0, 0, 1))
    panel = quad((-0.3, 1.9, -0.3), (0.3, 1.9, -0.3), (0.3, 1.9, 0.3), (-0.3, 1.9, 0.3), (0, -1, 0))
    card = quad((-0.8, 0.1, 0.2), (0.8, 0.1, 0.2), (0.8, 1.7, 0.2), (-0.8, 1.7, 0.2), (0, 0, 1))
    card["uv0"], card["uv1"], card["uv2"] = [[0.05, 0.1], [0.05, 0.1]], [[0.95, 0.1], [0.95, 0.9]], [[0.95, 0.9], [0.05, 0.9]]
    white = {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1], "metallicFactor": 0, "roughnessFactor": 0.7}}
    materials = [
        white,
        dict(white, alphaMode="BLEND"),                                      # a limit: stays opaque
        {"pbrMetallicRoughness": {"baseColorFactor": [1, 1, 1, 1]}, "emissiveFactor": [1, 1, 1],
         "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 12.0}}},
        {"pbrMetallicRoughness": {"baseColorFactor": [1, 1, 1, 1], "metallicFactor": 0, "roughnessFactor": 0.6,
                                  "baseColorTexture": {"index": 0}}, "alphaMode": "MASK", "alphaCutoff": 0.6},
    ]
    glb_io.write_glb(str(path), [mesh_of(floor, 0), mesh_of(back, 1), mesh_of(panel, 2), mesh_of(card, 3)],
                     [{"mesh": 0}, {"mesh": 1}, {"mesh": 2}, {"mesh": 3}], materials, images=[glb_io.encode_png(img)], textures=[0])
    return img


def load(tmp_path, name, size):
    rd = lambda n, dt: np.fromfile(tmp_path / ("%s_%s.bin" % (name, n)), dt)
    atlas = rd("atlas", np.float16).reshape(size, size, 4)
    return scenes.Scene(name, rd("triangles", layout.TRIANGLE), rd("materials", layout.MATERIAL), rd("bvhNodes", layout.BVH_NODE),
                        rd("lights", layout.LIGHT), atlas), rd("rgba8", np.uint8).reshape(size, size, 4)


def test_alpha_cutout_option_gives_the_bits_of_the_c_abi(tmp_path):
    ensure_addon()
    glb = tmp_path / "mask.glb"
    img = mask_glb(glb)
    script = tmp_path / "alpha.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), prep=json.dumps(os.path.join(HOST, "scene_prep.js")),
                                    gltf=json.dumps(os.path.join(HOST, "gltf.js")), dir=json.dumps(str(tmp_path)), glb=json.dumps(str(glb)),
                                    W=W, H=H, F=FRAMES))
    info = json.loads(subprocess.check_output([NODE, str(script)], text=True, timeout=300).strip().splitlines()[-1])
    # the table: one entry per primitive's material, MASK alone cut at its alphaCutoff; without the option there is none
    assert info["off"]["cutoff"] is None
    cutoff = np.float32(info["on"]["cutoff"])
    assert np.array_equal(cutoff, np.float32([0, 0, 0, 0.6]))
    size = info["on"]["width"]
    assert size == info["on"]["height"] == info["off"]["width"]
    on, on8 = load(tmp_path, "on", size)
    off, off8 = load(tmp_path, "off", size)
    # option off: the atlas is the restatement's (tests/atlas_ref.py), opaque everywhere; option on: only the alpha bytes differ, and
    # only inside the card's albedo rect, where they are the image's alpha through the 2 x 2 box filter
    _, canvas, atlas16 = atlas_ref.build([{}, {}, {}, {"albedo": 0}], [img])
    assert np.array_equal(off8, canvas) and np.array_equal(off.atlas.view(np.uint16), atlas16.view(np.uint16)) and (off8[..., 3] == 255).all()
    assert np.array_equal(on8[..., :3], off8[..., :3])
    x, y, w, h = (int(on.mats[3]["albedo_map"][k]) for k in "xywh")
    assert (w, h) == (8, 8)
    src = img[..., 3].astype(np.float64)
    mean = (src[0::2, 0::2] + src[1::2, 0::2] + src[0::2, 1::2] + src[1::2, 1::2]) / 4
    assert np.array_equal(on8[y:y + h, x:x + w, 3], np.floor(mean + 0.5).astype(np.uint8))
    outside = np.ones((size, size), bool)
    outside[y:y + h, x:x + w] = False
    assert (on8[..., 3][outside] == 255).all()
    for k in ("tris", "mats", "nodes", "lights"):
        assert getattr(on, k).tobytes() == getattr(off, k).tobytes(), k

    def out(name):
        return np.fromfile(tmp_path / (name + ".f32"), np.float32).reshape(H, W, 4)
    cam = layout.make_camera(W, H)
    with native.Context(0) as ctx:
        ctx.set_options(max_bounces=8, do_mis=1)

        def render(sc, table, **kw):
            ctx.upload_scene(sc)
            ctx.resize(W, H)
            if table is not None:
                ctx.set_alpha_cutoff(table, **kw)
            ctx.reset_stats()
            ctx.dispatch(cam, FRAMES)
            return ctx.read_output(), ctx.alpha_status().as_dict()
        want_cut, st_cut = render(on, cutoff)
        want_opaque, _ = render(on, None)
        want_plain, _ = render(off, None)
        want_again, st_again = render(on, cutoff, max_layers=2)
    assert st_cut["path_passes"] > 0 and st_cut["shadow_passes"] > 0 and st_cut["path_exhausted"] == 0 and not same(want_cut, want_plain)
    assert same(want_opaque, want_plain)                                    # nothing but a cutoff reads the alpha channel
    assert same(out("cut"), want_cut) and same(out("two"), want_cut)
    assert same(out("plain"), want_plain)
    assert same(out("cut_removed"), want_plain) and same(out("two_removed"), want_plain)
    assert same(out("cut_again"), want_again) and same(want_again, want_cut)
    for name in ("cut", "two"):
        got = info[name]
        assert (got["present"], got["materials"], got["cutout"], got["maxLayers"]) == (1, 4, 1, 4), name
        assert info[name + "Removed"]["present"] == 0 and info[name + "Threw"] is True and info[name + "Again"]["maxLayers"] == 2
    assert info["plain"]["present"] == 0


def test_cli_alpha_cutout(tmp_path):
    ensure_addon()
    glb = tmp_path / "mask.glb"
    mask_glb(glb)
    outs = {}
    for name, extra in (("cut", ["--alpha-cutout", "--alpha-layers", "3"]), ("plain", [])):
        txt = subprocess.check_output([NODE, os.path.join(HOST, "render_cli.js"), str(glb), str(tmp_path / (name + ".f32")), "--width", str(W),
                                       "--height", str(H), "--frames", str(FRAMES), "--batch", "2"] + extra, text=True, timeout=300)
        outs[name] = json.loads(txt.strip().splitlines()[-1]), np.fromfile(tmp_path / (name + ".f32"), np.float32).reshape(H, W, 4)
    st = outs["cut"][0]["alpha"]
    assert (st["present"], st["cutout"], st["maxLayers"]) == (1, 1, 3) and st["pathPasses"] > 0 and "alpha" not in outs["plain"][0]
    assert not same(outs["cut"][1], outs["plain"][1])
