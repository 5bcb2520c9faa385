"""Reprojection through the Node host (wgpu-path-tracing_amd/host): the addon's reproject gives the bytes of the ctypes path, and a
Renderer with setReproject keeps its samples across a camera change where one without restarts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ptmi import layout, native, scene_io, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 70, 37, 8


@pytest.fixture(scope="module")
def ptscene(tmp_path_factory):
    if not os.path.exists(os.path.join(HOST, "addon", "ptmi_napi.node")):             # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "wgpu-path-tracing_amd"), "all"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(HOST, "addon")], stdout=subprocess.DEVNULL)
    path = tmp_path_factory.mktemp("reproject") / "cornell.ptscene"
    scene_io.save_ptscene(scenes.make("cornell"), str(path))
    return str(path)


def node(js):
    return json.loads(subprocess.check_output([NODE, "-e", js], text=True, timeout=300).strip().splitlines()[-1])


def test_addon_reproject_gives_the_bytes_of_the_ctypes_path(ptscene, tmp_path):
    cam_from = layout.make_camera(W, H)
    cam_to = layout.make_camera(W, H, position=(0.3, 1.0, 2.8))
    params = dict(max_history=6, depth_tolerance=0.05)
    (tmp_path / "from.bin").write_bytes(cam_from.tobytes())
    (tmp_path / "to.bin").write_bytes(cam_to.tobytes())
    js = ("var fs=require('fs'),h=require(%r);var r=new h.Renderer({width:%d,height:%d});r.loadModel(%r).then(function(){"
          "var a=r.addon,from=fs.readFileSync(%r),to=fs.readFileSync(%r);a.setAovs(r.ctx,7);a.setMoments(r.ctx,true);"
          "a.dispatch(r.ctx,from,%d);a.reproject(r.ctx,from,to,{maxHistory:6,depthTolerance:0.05});var st=a.reprojectStatus(r.ctx);"
          "fs.writeFileSync(%r,Buffer.from(r.readOutput().buffer));"
          "fs.writeFileSync(%r,Buffer.from(a.readMoments(r.ctx,new Float32Array(%d)).buffer));"
          "fs.writeFileSync(%r,Buffer.from(r.readAov('normal').buffer));r.destroy();console.log(JSON.stringify(st));})"
          % (os.path.join(HOST, "renderer.js"), W, H, ptscene, str(tmp_path / "from.bin"), str(tmp_path / "to.bin"), FRAMES,
             str(tmp_path / "out.f32"), str(tmp_path / "mom.f32"), W * H * 4, str(tmp_path / "nrm.f32")))
    st = node(js)
    with native.Context(0) as ctx:
        ctx.upload_scene(scenes.make("cornell"))
        ctx.resize(W, H)
        ctx.set_aovs("albedo", "normal", "id")
        ctx.set_moments(True)
        ctx.dispatch(cam_from, FRAMES)
        ctx.reproject(cam_from, cam_to, **params)
        want = ctx.read_output(), ctx.read_moments(), ctx.read_aov("normal")
        assert st == ctx.reproject_status().as_dict() and st["carried"] > 0 and st["disoccluded"] > 0 and st["missed"] > 0
    for name, w in zip(("out", "mom", "nrm"), want):
        got = np.fromfile(tmp_path / f"{name}.f32", np.float32).reshape(H, W, 4)
        assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), name


def test_renderer_keeps_its_samples_across_a_camera_change(ptscene):
    js = ("var h=require(%r);var res={};var run=function(name,reproject){var r=new h.Renderer({width:%d,height:%d,"
          "adaptive:{threshold:0.05,minFrames:16,step:4}});if(reproject)r.setReproject({});"
          "return r.loadModel(%r).then(function(){r.renderAdaptive(2);var before=r.adaptiveStatus().samples;r.moveCamera(0,0.3,0);"
          "var kept=reproject?r.reprojectFrom!==null:null;r.renderAdaptive(1);var st=r.adaptiveStatus();"
          "res[name]={before:before,kept:kept,frameIndex:r.frameIndex,samples:st.samples,minCount:st.minCount,maxCount:st.maxCount,"
          "reprojected:reproject?r.reprojectStatus():null};r.destroy();});};"
          "run('with',true).then(function(){return run('without',false)}).then(function(){console.log(JSON.stringify(res))})"
          % (os.path.join(HOST, "renderer.js"), W, H, ptscene))
    res = node(js)
    n = W * H
    a, b = res["with"], res["without"]
    assert a["before"] == b["before"] == n * 8
    # without: the camera change restarted at frame 0, and the round after it gave every pixel its first 4 frames
    assert b["frameIndex"] == 1 and b["samples"] == n * 4 and b["minCount"] == b["maxCount"] == 4
    # with: the carried pixels kept their 8 samples and went on to 12; the others restarted
    assert a["kept"] is True and a["frameIndex"] == 3
    rp = a["reprojected"]
    assert rp["carried"] > 0 and rp["samples"] == rp["carried"] * 8 > 0
    assert a["samples"] == rp["samples"] + n * 4 and a["minCount"] == 4 and a["maxCount"] == 12


def test_set_reproject_throws_with_several_devices():
    js = ("var h=require(%r);var r=new h.Renderer({width:16,height:8,devices:[0,0],loopback:true});var out;"
          "try{r.setReproject({});out='no error'}catch(e){out=e.message}r.destroy();console.log(JSON.stringify(out))"
          % os.path.join(HOST, "renderer.js"))
    assert "not supported with several devices" in node(js)
