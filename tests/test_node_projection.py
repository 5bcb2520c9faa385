"""Camera projections through the Node host (host/render_cli.js --camera / --projection / --ymag / --hdr; Renderer.useSceneCamera,
setProjection): the orthographic camera of tests/gltf_camera_scene.py's file renders the bits the C ABI renders from the same blobs
and the same packed camera, and a panorama written with --hdr is an environment map that --env loads back."""
import json
import os
import subprocess

import numpy as np
import pytest

import gltf_camera_scene as G
from ptmi import layout, native
from test_gltf_host import prepare
from test_node_medium import HOST, NODE, ensure_addon, same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 48, 32, 4
PW, PH = 64, 32


def cli(*args):
    out = subprocess.check_output([NODE, os.path.join(HOST, "render_cli.js")] + [str(a) for a in args], text=True, timeout=300)
    return json.loads(out.strip().splitlines()[-1])


def c_abi_render(sc, cam, frames):
    with native.Context(0) as ctx:
        ctx.set_options(max_bounces=8, do_mis=1)
        ctx.upload_scene(sc)
        ctx.resize(int(cam["width"]), int(cam["height"]))
        ctx.set_projections(True)
        ctx.dispatch(cam, frames)
        return ctx.read_output()


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    ensure_addon()
    d = tmp_path_factory.mktemp("proj")
    G.write_scene(d / "cams.glb")
    sc, info = prepare(d / "cams.glb", d / "blobs")
    return d, sc, info


def test_cli_renders_the_files_orthographic_camera(scene):
    d, sc, info = scene
    st = cli(d / "cams.glb", d / "ortho.f32", "--camera", 1, "--width", W, "--height", H, "--frames", FRAMES)
    assert st["projection"] == {"kind": "orthographic", "ymag": G.YMAG}
    got = np.fromfile(d / "ortho.f32", np.float32).reshape(H, W, 4)
    c = info["cameras"][1]
    cam = layout.make_camera(W, H, position=c["position"], forward=c["forward"], right=c["right"], up=c["up"],
                             projection="orthographic", ymag=c["ymag"])
    want = c_abi_render(sc, cam, FRAMES)
    assert want[..., :3].max() > 0.05 and same(got, want)
    # ... and it is not the picture of the pinhole from the same place
    assert not same(got, c_abi_render(sc, layout.set_projection(cam.copy(), "perspective"), FRAMES))
    # the perspective camera of the file: its yfov, the frame's aspect
    st = cli(d / "cams.glb", d / "persp.f32", "--camera", 0, "--width", W, "--height", H, "--frames", FRAMES)
    assert st["projection"]["kind"] == "perspective"
    p = info["cameras"][0]
    cam = layout.make_camera(W, H, position=p["position"], forward=p["forward"], right=p["right"], up=p["up"], fov=p["yfov"])
    assert same(np.fromfile(d / "persp.f32", np.float32).reshape(H, W, 4), c_abi_render(sc, cam, FRAMES))


def rgbe(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"\n\n", 1)
    res, body = body.split(b"\n", 1)
    assert head.startswith(b"#?RADIANCE") and b"FORMAT=32-bit_rle_rgbe" in head
    _, h, _, w = res.split()
    px = np.frombuffer(body, np.uint8).reshape(int(h), int(w), 4).astype(np.float64)
    return px[..., :3] * np.where(px[..., 3:] == 0, 0.0, 2.0 ** (px[..., 3:] - 136))


def test_a_panorama_is_an_environment_map(scene):
    d, sc, info = scene
    st = cli(d / "cams.glb", d / "pano.f32", "--projection", "panorama", "--width", PW, "--height", PH, "--frames", FRAMES, "--hdr", d / "pano.hdr")
    assert st["projection"]["kind"] == "equirect"
    got = np.fromfile(d / "pano.f32", np.float32).reshape(PH, PW, 4)
    cam = layout.make_camera(PW, PH, projection="equirect")
    assert same(got, c_abi_render(sc, cam, FRAMES))
    # the file: top row first, turned by a quarter of the width, every channel within RGBE's 8 bits of the largest one
    env = np.roll(got[::-1, :, :3], -PW // 4, axis=1).astype(np.float64)
    file = rgbe(d / "pano.hdr")
    assert file.shape == (PH, PW, 3)
    peak = env.max(axis=2, keepdims=True)
    assert (np.abs(file - env) <= peak / 128 + 1e-30).all() and file.max() > 0.05
    # ... and --env takes it: the box lit by what the camera saw differs from the box alone
    lit = cli(d / "cams.glb", d / "lit.f32", "--width", W, "--height", H, "--frames", FRAMES, "--env", d / "pano.hdr")
    dark = cli(d / "cams.glb", d / "dark.f32", "--width", W, "--height", H, "--frames", FRAMES)
    a, b = (np.fromfile(d / n, np.float32).reshape(H, W, 4) for n in ("lit.f32", "dark.f32"))
    assert np.isfinite(a).all() and a[..., :3].sum() > b[..., :3].sum() and lit["segments"] > 0 and dark["segments"] > 0
