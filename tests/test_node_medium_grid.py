"""The medium's density grid through the Node host: Renderer.setMediumDensity gives the bits of the C ABI's render of the same grid, on
one context and on two loopback contexts (the multi call); `normalise` divides by the maximum and multiplies sigmaT by it;
setMediumDensity(null) gives the homogeneous medium's bits back; and `render_cli.js --fog-density` runs."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import medium_grid_ref as R
from ptmi import layout, native, scene_io, scenes
from test_node_medium import H, HOST, W, ensure_addon, same

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

FRAMES = 4
FOG = dict(sigma_t=0.5, albedo=(0.9, 0.8, 0.7), g=0.3)
DIMS = (3, 5, 2)

SCRIPT = """
var fs = require('fs');
var host = require(%(renderer)s);
var raw = fs.readFileSync(%(grid)s);
var rho = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length));
var times8 = rho.map(function (v) { return 8 * v; }),
    times16 = rho.map(function (v) { return 16 * v; });
function run(opts, name, next) {
  var r = new host.Renderer(Object.assign({ width: %(W)d, height: %(H)d, options: { maxBounces: 8, doMis: 1 } }, opts));
  function render(path) {
    r.frameIndex = 0;
    while (r.frameIndex < %(F)d) r.renderFrame(2);
    if (opts.devices) r.gather();
    fs.writeFileSync(path, Buffer.from(r.readOutput().buffer));
  }
  var info = {};
  try { r.setMediumDensity(rho, %(dims)s); } catch (e) { info.needsMedium = /needs a medium/.test(String(e)); }
  r.loadModel(%(scene)s).then(function () {
    r.setMedium({ sigmaT: 0.5, albedo: [0.9, 0.8, 0.7], g: 0.3, bounds: 'scene' });
    r.setMediumDensity(rho, %(dims)s, { filter: 'linear' });
    render(%(dir)s + '/' + name + '_linear.f32');
    r.setMediumDensity(rho, %(dims)s);
    render(%(dir)s + '/' + name + '_nearest.f32');
    try { r.setMediumDensity(times8, %(dims)s); } catch (e) { info.threw = /upload_medium_density failed \\(-1\\)/.test(String(e)); }
    render(%(dir)s + '/' + name + '_kept.f32');
    r.setMediumDensity(times16, %(dims)s, { normalise: true });            // maximum 4: rho / 4 under 4 sigmaT
    render(%(dir)s + '/' + name + '_normalised.f32');
    // what the library would refuse is refused before `normalise` changes anything: the grid and sigmaT in place stay
    var nan = times16.slice(), deep = rho.map(function (v) { return 4e4 * v; });
    nan[3] = NaN;
    info.refused = 0;
    [nan, deep].forEach(function (bad) {
      try { r.setMediumDensity(bad, %(dims)s, { normalise: true }); } catch (e) { if (e instanceof RangeError) info.refused++; }
    });
    render(%(dir)s + '/' + name + '_kept_normalised.f32');
    r.setMediumDensity(null);
    render(%(dir)s + '/' + name + '_homogeneous.f32');
    r.destroy();
    next(info);
  });
}
run({}, 'one', function (a) {
  run({ devices: [0, 0], loopback: true }, 'two', function (b) { console.log(JSON.stringify({ one: a, two: b })); });
});
"""


def grid():
    """densities whose quotient by 4 and product with 4 are exact"""
    return np.round(R.probe_grid(DIMS) * 64) / np.float32(256)               # multiples of 1 / 256 up to 0.25


def reference_renders(sc):
    cam = layout.make_camera(W, H)
    box = (tuple(sc.nodes[0]["aabb_min"]), tuple(sc.nodes[0]["aabb_max"]))
    g = grid()
    out = {}
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=8, do_mis=1)
        ctx.set_medium(box=box, **FOG)
        for name, filt in (("linear", 1), ("nearest", 0)):
            ctx.upload_medium_density(g, filter=filt)
            ctx.dispatch(cam, FRAMES)
            out[name] = ctx.read_output()
        ctx.set_medium(box=box, **dict(FOG, sigma_t=2.0))                    # 16 rho has the maximum 4: it moves into sigma_t
        ctx.upload_medium_density(g * np.float32(4))
        ctx.dispatch(cam, FRAMES)
        out["normalised"] = ctx.read_output()
        ctx.set_medium(box=box, **FOG)
        ctx.upload_medium_density(None)
        ctx.dispatch(cam, FRAMES)
        out["homogeneous"] = ctx.read_output()
    return out


def test_set_medium_density_gives_the_bits_of_the_c_abi(tmp_path):
    ensure_addon()
    sc = scenes.make("cornell")
    scene_io.save_ptscene(sc, str(tmp_path / "cornell.ptscene"))
    g = grid()
    assert g.max() == 0.25 and g.min() == 0.0
    g.tofile(tmp_path / "grid.f32")
    script = tmp_path / "smoke.js"
    script.write_text(SCRIPT % dict(renderer=json.dumps(os.path.join(HOST, "renderer.js")), W=W, H=H, F=FRAMES, dims=json.dumps(list(DIMS)),
                                    scene=json.dumps(str(tmp_path / "cornell.ptscene")), grid=json.dumps(str(tmp_path / "grid.f32")),
                                    dir=json.dumps(str(tmp_path))))
    out = subprocess.check_output([NODE, str(script)], text=True, timeout=300)
    info = json.loads(out.strip().splitlines()[-1])
    want = reference_renders(sc)
    assert not same(want["linear"], want["nearest"]) and not same(want["nearest"], want["normalised"])
    assert not same(want["nearest"], want["homogeneous"])
    for name in ("one", "two"):
        got = {k: np.fromfile(tmp_path / ("%s_%s.f32" % (name, k)), np.float32).reshape(H, W, 4)
               for k in ("linear", "nearest", "kept", "normalised", "kept_normalised", "homogeneous")}
        assert info[name] == {"needsMedium": True, "threw": True, "refused": 2}, name    # values above 1 without `normalise`: the library's error
        assert same(got["kept"], want["nearest"]), name                      # ... and the grid in place stays
        assert same(got["kept_normalised"], want["normalised"]), name        # a NaN, and a maximum past the optical-depth limit
        for k in ("linear", "nearest", "normalised", "homogeneous"):
            assert same(got[k], want[k]), (name, k)


@pytest.mark.parametrize("peak", [2.0, 0.5])
def test_cli_fog_density(tmp_path, peak):
    """a file with values above 1 is divided by its maximum; one within [0, 1] is taken as it is"""
    ensure_addon()
    sc = scenes.make("cornell")
    scene_io.save_ptscene(sc, str(tmp_path / "cornell.ptscene"))
    g = grid()
    (g * np.float32(4 * peak)).tofile(tmp_path / "density.f32")              # sigma_t stays 0.5 either way
    subprocess.check_output([NODE, os.path.join(HOST, "render_cli.js"), str(tmp_path / "cornell.ptscene"), str(tmp_path / "out.f32"),
                             "--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--batch", "2", "--fog", "0.5,0.75,0.3",
                             "--fog-density", str(tmp_path / "density.f32"), "--fog-grid", "3,5,2", "--fog-filter", "linear"],
                            text=True, timeout=300)
    got = np.fromfile(tmp_path / "out.f32", np.float32).reshape(H, W, 4)
    cam = layout.make_camera(W, H)
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=8, do_mis=1)
        ctx.set_medium(sigma_t=0.5, albedo=0.75, g=0.3, box=(tuple(sc.nodes[0]["aabb_min"]), tuple(sc.nodes[0]["aabb_max"])))
        ctx.upload_medium_density(g * np.float32(4 if peak > 1 else 4 * peak), filter=1)
        ctx.dispatch(cam, FRAMES)
        want = ctx.read_output()
        ctx.upload_medium_density(None)
        ctx.dispatch(cam, FRAMES)
        plain = ctx.read_output()
    assert same(got, want) and not same(want, plain)
