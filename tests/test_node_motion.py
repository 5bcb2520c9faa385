"""Motion through the Node host (wgpu-path-tracing_amd/host): the addon's reproject with motion on gives the bytes of the ctypes path
after the same triangle update, and a Renderer with setReproject and setMotion keeps its samples across updateTriangles where one
without setMotion restarts at frame 0."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import scene_update_ref as sur
from ptmi import layout, native, scene_io, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H, FRAMES = 70, 37, 8


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(the scene file, the scene, the first triangle of the edit, the file of its records): the short box of cornell turned and moved"""
    if not os.path.exists(os.path.join(HOST, "addon", "ptmi_napi.node")):             # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "wgpu-path-tracing_amd"), "all"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(HOST, "addon")], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("motion")
    sc = scenes.make("cornell")
    scene_io.save_ptscene(sc, str(d / "cornell.ptscene"))
    sel = sc.tris["material_index"] == 5
    idx = np.flatnonzero(sel)
    first, end = int(idx.min()), int(idx.max()) + 1
    moved = sur.move_part(sc.tris, sel, sur.rot_y(0.5), (-0.4, 0.0, 0.3))
    (d / "tris.bin").write_bytes(moved[first:end].tobytes())
    return str(d / "cornell.ptscene"), sc, first, moved[first:end], str(d / "tris.bin")


def node(js):
    return json.loads(subprocess.check_output([NODE, "-e", js], text=True, timeout=300).strip().splitlines()[-1])


def test_addon_reproject_with_motion_gives_the_bytes_of_the_ctypes_path(case, tmp_path):
    ptscene, sc, first, records, blob = case
    cam_from = layout.make_camera(W, H)
    cam_to = layout.make_camera(W, H, position=(0.3, 1.0, 2.8))
    (tmp_path / "from.bin").write_bytes(cam_from.tobytes())
    (tmp_path / "to.bin").write_bytes(cam_to.tobytes())
    js = ("var fs=require('fs'),h=require(%r);var r=new h.Renderer({width:%d,height:%d});r.loadModel(%r).then(function(){"
          "var a=r.addon,from=fs.readFileSync(%r),to=fs.readFileSync(%r);a.setAovs(r.ctx,7);a.setMoments(r.ctx,true);r.setMotion(true);"
          "a.dispatch(r.ctx,from,%d);a.updateTriangles(r.ctx,%d,fs.readFileSync(%r));var dirty=a.motionStatus(r.ctx);"
          "a.reproject(r.ctx,from,to,{maxHistory:6});var st=a.reprojectStatus(r.ctx),ms=a.motionStatus(r.ctx);"
          "var prev=a.debugMotionPrev(r.ctx,%d,2,new Float32Array(18));"
          "fs.writeFileSync(%r,Buffer.from(r.readOutput().buffer));"
          "fs.writeFileSync(%r,Buffer.from(a.readMoments(r.ctx,new Float32Array(%d)).buffer));"
          "fs.writeFileSync(%r,Buffer.from(r.readMotion().buffer));r.destroy();"
          "console.log(JSON.stringify({st:st,ms:ms,dirty:dirty,prev:Array.from(prev)}));})"
          % (os.path.join(HOST, "renderer.js"), W, H, ptscene, str(tmp_path / "from.bin"), str(tmp_path / "to.bin"), FRAMES, first, blob,
             first, str(tmp_path / "out.f32"), str(tmp_path / "mom.f32"), W * H * 4, str(tmp_path / "mot.f32")))
    res = node(js)
    assert (res["dirty"]["dirtyFirst"], res["dirty"]["dirtyCount"], res["dirty"]["epochs"]) == (first, len(records), 0)
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(W, H)
        ctx.set_aovs("albedo", "normal", "id")
        ctx.set_moments(True)
        ctx.set_motion(True)
        ctx.dispatch(cam_from, FRAMES)
        ctx.update_triangles(first, records)
        ctx.reproject(cam_from, cam_to, max_history=6)
        want = ctx.read_output(), ctx.read_moments(), ctx.read_motion()
        ms = ctx.motion_status().as_dict()
        assert res["st"] == ctx.reproject_status().as_dict()
        assert res["ms"] == dict(on=1, epochs=1, dirtyFirst=0, dirtyCount=0, moved=ms["moved"], movedCarried=ms["moved_carried"])
        assert ms["moved_carried"] > 0
        prev = ctx.debug_motion_prev(first, 2)
    assert np.array_equal(np.array(res["prev"], np.float32).view(np.uint32), prev.reshape(-1).view(np.uint32))     # committed: the new ones
    for name, w in zip(("out", "mom", "mot"), want):
        got = np.fromfile(tmp_path / f"{name}.f32", np.float32).reshape(H, W, 4)
        assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), name


def test_renderer_keeps_its_samples_across_update_triangles(case):
    ptscene, _, first, _, blob = case
    js = ("var fs=require('fs'),h=require(%r);var res={};var run=function(name,motion){var r=new h.Renderer({width:%d,height:%d,"
          "adaptive:{threshold:0.05,minFrames:16,step:4}});r.setReproject({});if(motion)r.setMotion(true);"
          "return r.loadModel(%r).then(function(){r.renderAdaptive(2);var before=r.adaptiveStatus().samples;"
          "r.updateTriangles(%d,fs.readFileSync(%r));var after=r.frameIndex;r.renderAdaptive(1);var st=r.adaptiveStatus();"
          "res[name]={before:before,after:after,frameIndex:r.frameIndex,samples:st.samples,minCount:st.minCount,maxCount:st.maxCount,"
          "reprojected:r.reprojectStatus(),motion:motion?r.motionStatus():null,"
          "plane:motion?Array.from(r.readMotion()).some(function(x){return x!==0}):null};r.destroy();});};"
          "run('with',true).then(function(){return run('without',false)}).then(function(){console.log(JSON.stringify(res))})"
          % (os.path.join(HOST, "renderer.js"), W, H, ptscene, first, blob))
    res = node(js)
    n = W * H
    a, b = res["with"], res["without"]
    assert a["before"] == b["before"] == n * 8
    # without motion: the edit restarted at frame 0, and the round after it gave every pixel its first 4 frames
    assert b["after"] == 0 and b["frameIndex"] == 1 and b["samples"] == n * 4 and b["minCount"] == b["maxCount"] == 4
    assert b["reprojected"]["carried"] == 0
    # with: the rounds continue; the carried pixels kept their 8 samples and went on to 12, the others started over, none is without samples
    assert a["after"] == 2 and a["frameIndex"] == 3
    rp, ms = a["reprojected"], a["motion"]
    assert rp["carried"] > 0 and rp["samples"] == rp["carried"] * 8
    assert a["samples"] == rp["samples"] + n * 4 and a["minCount"] == 4 > 0 and a["maxCount"] == 12
    assert ms["moved"] > 0 and ms["movedCarried"] > 0 and ms["dirtyCount"] == 0 and a["plane"] is True
    assert ms["epochs"] == 2                                  # the restart at frame 0 committed, and so did the reprojection


def test_set_motion_throws_with_several_devices():
    js = ("var h=require(%r);var r=new h.Renderer({width:16,height:8,devices:[0,0],loopback:true});var out;"
          "try{r.setMotion(true);out='no error'}catch(e){out=e.message}r.destroy();console.log(JSON.stringify(out))"
          % os.path.join(HOST, "renderer.js"))
    assert "not supported with several devices" in node(js)
