"""Probe visibility through the Node host: `render_cli.js --probes nx,ny,nz --probe-visibility M --probe-border`
(Renderer.bakeProbes with `visibility`) on cornell gives the bytes of the ctypes path for the same lattice: the bordered visibility
tiles and the bordered irradiance tiles, with the clamp both hosts derive from the lattice; and Renderer.bakeProbes returns the depth
plane of the ctypes path beside them."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ptmi import native, probes, scene_io, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

COUNTS, TILE, M, FRAMES, SHARP = (3, 1, 2), 8, 4, 3, 5


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_node_visibility_gives_the_bytes_of_the_ctypes_path(tmp_path):
    if not os.path.exists(os.path.join(HOST, "addon", "ptmi_napi.node")):             # normally built by the project's build step
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "wgpu-path-tracing_amd"), "all"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(HOST, "addon")], stdout=subprocess.DEVNULL)
    sc = scenes.make("cornell")
    scene_io.save_ptscene(sc, str(tmp_path / "cornell.ptscene"))
    out = subprocess.check_output([NODE, os.path.join(HOST, "render_cli.js"), str(tmp_path / "cornell.ptscene"), str(tmp_path / "out.f32"),
                                   "--frames", str(FRAMES), "--bounces", "4", "--probes", ",".join(map(str, COUNTS)),
                                   "--probe-tile", str(TILE), "--probe-irradiance", str(M), "--probe-visibility", str(M),
                                   "--probe-sharpness", str(SHARP), "--probe-border"], text=True, timeout=300)
    st = json.loads(out.strip().splitlines()[-1])
    root = np.frombuffer(sc.nodes[:1].tobytes(), np.float32)                          # the root box: the scene's bounds
    lo, hi = root[0:3], root[4:7]
    pos = probes.grid(lo, hi, COUNTS)
    n = len(pos)
    W, H = probes.atlas_size(n, TILE)
    assert st["probes"] == dict(width=W, height=H, count=n, tile=TILE)
    far = probes.max_distance(lo, hi, COUNTS)
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=4, do_mis=1)
        ctx.upload_probes(probes.records(pos), TILE)
        ctx.set_probe_depth(far)
        ctx.write_output(np.zeros((H, W, 4), np.float32))
        ctx.dispatch_probes(FRAMES)
        want, want_depth = ctx.read_output(), ctx.read_probe_depth()
        want_irr = probes.add_border(ctx.probe_irradiance(M), M)
        want_vis, plain = ctx.probe_visibility(M, SHARP, border=True), ctx.probe_visibility(M, SHARP)
    side = M + 2
    assert os.path.getsize(tmp_path / "out.vis.f32") == n * side * side * 16
    got = np.fromfile(tmp_path / "out.f32", np.float32).reshape(H, W, 4)
    got_irr = np.fromfile(tmp_path / "out.irr.f32", np.float32).reshape(n, side, side, 4)
    got_vis = np.fromfile(tmp_path / "out.vis.f32", np.float32).reshape(n, side, side, 4)
    assert same(got, want) and same(got_irr, want_irr) and same(got_vis, want_vis)
    assert same(want_vis, probes.add_border(plain, M)) and (want_vis[..., 3] == 1).all()
    assert 0 < want_vis[..., 0].min() and want_vis[..., 0].max() <= far * np.float32(1.000001) and want_depth[..., 0].max() > 0
    # Renderer.bakeProbes itself, without a border: the depth plane and the plain tiles
    script = ("const host = require(%r), fs = require('fs');\n"
              "const r = new host.Renderer({ width: 8, height: 8, options: { maxBounces: 4, doMis: 1 } });\n"
              "r.loadModel(process.argv[1] + '/cornell.ptscene').then(function () {\n"
              "  const p = r.bakeProbes({ grid: { min: r.sceneBounds.min, max: r.sceneBounds.max, counts: %s }, tile: %d, frames: %d,\n"
              "                           visibility: { tile: %d, sharpness: %d } });\n"
              "  fs.writeFileSync(process.argv[1] + '/depth.f32', Buffer.from(p.depth.buffer));\n"
              "  fs.writeFileSync(process.argv[1] + '/vis.f32', Buffer.from(p.visibility.buffer));\n"
              "  r.destroy();\n"
              "}).catch(function (e) { console.error(e); process.exit(1); });\n"
              % (os.path.join(HOST, "renderer.js"), list(COUNTS), TILE, FRAMES, M, SHARP))
    run = subprocess.run([NODE, "-e", script, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert same(np.fromfile(tmp_path / "depth.f32", np.float32).reshape(H, W, 4), want_depth)
    assert same(np.fromfile(tmp_path / "vis.f32", np.float32).reshape(n, M, M, 4), plain)
