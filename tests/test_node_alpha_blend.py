"""Alpha blending through the Node host: new Renderer({alphaBlend: true}) loads a .glb with alphaMode "BLEND" materials, keeps the
albedo map's alpha in the atlas, sets the blend table from baseColorFactor[3], and renders the bits the C ABI renders from the same
blobs and table; setAlphaBlend replaces and removes it; and `render_cli.js --alpha-blend` runs."""
import json
import os
import subprocess

import numpy as np
import pytest

from ptmi import glb_io, layout, native, scenes
from test_node_alpha import NODE, load
from test_node_medium import HOST, ensure_addon, same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 64, 48, 4

SCRIPT = """
var fs = require('fs'), path = require('path');
var host = require(%(renderer)s), prep = require(%(prep)s), gltf = require(%(gltf)s);
var dir = %(dir)s, glb = %(glb)s;
var s = prep.prepareScene(gltf.loadGLB(glb), { alphaBlend: true });
Object.keys(s.blobs).forEach(function (k) { fs.writeFileSync(path.join(dir, 'on_' + k + '.bin'), Buffer.from(s.blobs[k])); });
fs.writeFileSync(path.join(dir, 'on_atlas.bin'), Buffer.from(s.atlas.data.buffer, s.atlas.data.byteOffset, s.atlas.data.byteLength));
fs.writeFileSync(path.join(dir, 'on_rgba8.bin'), Buffer.from(s.atlas.rgba8.buffer, s.atlas.rgba8.byteOffset, s.atlas.rgba8.byteLength));
var info = { width: s.atlas.width, table: Array.from(s.alphaBlend) };
function run(opts, name, next) {
  var r = new host.Renderer(Object.assign({ width: %(W)d, height: %(H)d, options: { maxBounces: 8, doMis: 1 } }, opts));
  r.loadModel(glb).then(function () {
    function render(tag) {
      r.frameIndex = 0;
      while (r.frameIndex < %(F)d) r.renderFrame(2);
      fs.writeFileSync(path.join(dir, name + tag + '.f32'), Buffer.from(r.readOutput().buffer));
      return r.alphaBlendStatus();
    }
    info[name] = render('');
    if (opts.alphaBlend) {
      r.setAlphaBlend(null);
      info[name + 'Removed'] = render('_removed');
      try { r.setAlphaBlend(new Float32Array(1)); } catch (e) { info[name + 'Threw'] = /set_alpha_blend failed \\(-1\\)/.test(String(e)); }
      r.setAlphaBlend(new Float32Array(info.table), { maxLayers: 2, seed: 9 });
      info[name + 'Again'] = render('_again');
    }
    r.destroy();
    next();
  });
}
run({ alphaBlend: true, alphaBlendSeed: 5 }, 'blend', function () {
  run({}, 'plain', function () {
    run({ alphaBlend: true, alphaBlendSeed: 5, devices: [0, 0], loopback: true }, 'two', function () { console.log(JSON.stringify(info)); });
  });
});
"""


def blend_glb(path):
    """a floor, a back wall and a light panel, and in front of the wall two cards: one alphaMode BLEND with factor 0.5 over an RGBA
    image whose alpha is 255 in its upper half and 128 below, one BLEND with factor 0 (never there)"""
    rng = np.random.default_rng(3)
    img = rng.integers(64, 256, (16, 16, 4), dtype=np.uint8)
    img[:8, :, 3], img[8:, :, 3] = 255, 128
    quad = lambda a, b, c, d, n: scenes._quad(a, b, c, d, n, 0)

    def mesh_of(tris, material):
        pos = np.stack([tris["v0"], tris["v1"], tris["v2"]], 1).reshape(-1, 3)
        nrm = np.stack([tris["n0"], tris["n1"], tris["n2"]], 1).reshape(-1, 3)
        uv = np.stack([tris["uv0"], tris["uv1"], tris["uv2"]], 1).reshape(-1, 2)
        return {"positions": pos, "normals": nrm, "uvs": uv, "indices": np.arange(len(pos)), "material": material}

    floor = quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0))
    back = quad((-1, 0, -1), (-1, 2, -1), (1, 2, -1), (1, 0, -1), (0, 0, 1))
    panel = quad((-0.3, 1.9, -0.3), (0.3, 1.9, -0.3), (0.3, 1.9, 0.3), (-0.3, 1.9, 0.3), (0, -1, 0))
    card = quad((-0.8, 0.1, 0.2), (0.1, 0.1, 0.2), (0.1, 1.7, 0.2), (-0.8, 1.7, 0.2), (0, 0, 1))
    card["uv0"], card["uv1"], card["uv2"] = [[0.05, 0.1], [0.05, 0.1]], [[0.95, 0.1], [0.95, 0.9]], [[0.95, 0.9], [0.05, 0.9]]
    ghost = quad((0.2, 0.1, 0.3), (0.8, 0.1, 0.3), (0.8, 1.7, 0.3), (0.2, 1.7, 0.3), (0, 0, 1))
    white = {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1], "metallicFactor": 0, "roughnessFactor": 0.7}}
    materials = [
        white,
        {"pbrMetallicRoughness": {"baseColorFactor": [1, 1, 1, 1]}, "emissiveFactor": [1, 1, 1],
         "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 12.0}}},
        {"pbrMetallicRoughness": {"baseColorFactor": [1, 1, 1, 0.5], "metallicFactor": 0, "roughnessFactor": 0.6,
                                  "baseColorTexture": {"index": 0}}, "alphaMode": "BLEND"},
        {"pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.1, 0.1, 0], "metallicFactor": 0, "roughnessFactor": 0.6}, "alphaMode": "BLEND"},
    ]
    glb_io.write_glb(str(path), [mesh_of(floor, 0), mesh_of(back, 0), mesh_of(panel, 1), mesh_of(card, 2), mesh_of(ghost, 3)],
                     [{"mesh": k} for k in range(5)], materials, images=[glb_io.encode_png(img)], textures=[0])


def test_alpha_blend_option_gives_the_bits_of_the_c_abi(tmp_path):
    ensure_addon()
    glb = tmp_path / "blend.glb"
    blend_glb(glb)
    script = tmp_path / "blend.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), prep=json.dumps(os.path.join(HOST, "scene_prep.js")),
                                    gltf=json.dumps(os.path.join(HOST, "gltf.js")), dir=json.dumps(str(tmp_path)), glb=json.dumps(str(glb)),
                                    W=W, H=H, F=FRAMES))
    info = json.loads(subprocess.check_output([NODE, str(script)], text=True, timeout=300).strip().splitlines()[-1])
    table = np.float32(info["table"])
    assert np.array_equal(table, np.float32([-1, -1, -1, 0.5, 0]))          # one entry per primitive's material
    on, on8 = load(tmp_path, "on", info["width"])
    assert set(np.unique(on8[..., 3]).tolist()) >= {128, 255}               # the card's alpha is in the atlas

    def out(name):
        return np.fromfile(tmp_path / (name + ".f32"), np.float32).reshape(H, W, 4)
    cam = layout.make_camera(W, H)
    with native.Context(0) as ctx:
        ctx.set_options(max_bounces=8, do_mis=1)

        def render(tab, **kw):
            ctx.upload_scene(on)
            ctx.resize(W, H)
            if tab is not None:
                ctx.set_alpha_blend(tab, **kw)
            ctx.reset_stats()
            ctx.dispatch(cam, FRAMES)
            return ctx.read_output(), ctx.alpha_blend_status().as_dict()
        want, st = render(table, seed=5)
        want_plain, _ = render(None)
        want_again, st_again = render(table, seed=9, max_layers=2)
    assert st["path_passes"] > 0 and st["shadow_passes"] > 0 and st["path_tests"] > st["path_passes"]
    assert not same(want, want_plain) and not same(want, want_again)
    assert same(out("blend"), want) and same(out("two"), want)
    assert same(out("plain"), want_plain)
    assert same(out("blend_removed"), want_plain) and same(out("two_removed"), want_plain)
    assert same(out("blend_again"), want_again) and same(out("two_again"), want_again)
    for name in ("blend", "two"):
        got = info[name]
        assert (got["present"], got["materials"], got["blend"], got["maxLayers"], got["seed"]) == (1, 5, 2, 4, 5), name
        assert (got["pathTests"], got["pathPasses"], got["shadowTests"], got["shadowPasses"]) == \
            (st["path_tests"], st["path_passes"], st["shadow_tests"], st["shadow_passes"]), name
        assert info[name + "Removed"]["present"] == 0 and info[name + "Threw"] is True
        assert (info[name + "Again"]["maxLayers"], info[name + "Again"]["seed"]) == (2, 9)
    assert info["plain"]["present"] == 0


def test_cli_alpha_blend(tmp_path):
    ensure_addon()
    glb = tmp_path / "blend.glb"
    blend_glb(glb)
    outs = {}
    for name, extra in (("blend", ["--alpha-blend", "--alpha-seed", "3", "--alpha-layers", "3"]), ("plain", [])):
        txt = subprocess.check_output([NODE, os.path.join(HOST, "render_cli.js"), str(glb), str(tmp_path / (name + ".f32")), "--width", str(W),
                                       "--height", str(H), "--frames", str(FRAMES), "--batch", "2"] + extra, text=True, timeout=300)
        outs[name] = json.loads(txt.strip().splitlines()[-1]), np.fromfile(tmp_path / (name + ".f32"), np.float32).reshape(H, W, 4)
    st = outs["blend"][0]["alphaBlend"]
    assert (st["present"], st["blend"], st["maxLayers"], st["seed"]) == (1, 2, 3, 3) and st["pathPasses"] > 0
    assert "alphaBlend" not in outs["plain"][0] and not same(outs["blend"][1], outs["plain"][1])
