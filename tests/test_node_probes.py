"""Light probes through the Node host: `render_cli.js --probes nx,ny,nz` (Renderer.bakeProbes) on cornell gives the bytes of the ctypes
path with ptmi.probes.grid over the same bounds: the radiance atlas, the SH9 coefficients and the irradiance tiles."""
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

COUNTS, TILE, M, FRAMES = (3, 1, 2), 8, 4, 3


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_cli_probes_give_the_bytes_of_the_ctypes_path(tmp_path):
    if not os.path.exists(os.path.join(HOST, "addon", "ptmi_napi.node")):             # normally built by the project's build step
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "wgpu-path-tracing_amd"), "all"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(HOST, "addon")], stdout=subprocess.DEVNULL)
    sc = scenes.make("cornell")
    scene_io.save_ptscene(sc, str(tmp_path / "cornell.ptscene"))
    out = subprocess.check_output([NODE, os.path.join(HOST, "render_cli.js"), str(tmp_path / "cornell.ptscene"), str(tmp_path / "out.f32"),
                                   "--frames", str(FRAMES), "--bounces", "4", "--probes", ",".join(map(str, COUNTS)),
                                   "--probe-tile", str(TILE), "--probe-irradiance", str(M)], text=True, timeout=300)
    st = json.loads(out.strip().splitlines()[-1])
    root = np.frombuffer(sc.nodes[:1].tobytes(), np.float32)                          # the root box: the scene's bounds
    pos = probes.grid(root[0:3], root[4:7], COUNTS)
    n = len(pos)
    W, H = probes.atlas_size(n, TILE)
    assert st["probes"] == dict(width=W, height=H, count=n, tile=TILE) and (W, H) == (24, 16)
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_options(max_bounces=4, do_mis=1)
        ctx.upload_probes(probes.records(pos), TILE)
        ctx.write_output(np.zeros((H, W, 4), np.float32))
        ctx.dispatch_probes(FRAMES)
        want, want_sh, want_irr = ctx.read_output(), ctx.probe_sh(), ctx.probe_irradiance(M)
    got = np.fromfile(tmp_path / "out.f32", np.float32).reshape(H, W, 4)
    got_sh = np.fromfile(tmp_path / "out.sh.f32", np.float32).reshape(n, 9, 3)
    got_irr = np.fromfile(tmp_path / "out.irr.f32", np.float32).reshape(n, M, M, 4)
    assert same(got, want) and same(got_sh, want_sh) and same(got_irr, want_irr)
    assert want[..., :3].max() > 0.05 and want_sh[:, 0].min() > 0 and (want_irr[..., 3] == 1).all()
    assert st["paths"] == n * TILE * TILE * FRAMES
