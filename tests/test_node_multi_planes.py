"""The planes, adaptive rounds and the denoiser over several devices through the Node host (wgpu-path-tracing_amd/host):
new Renderer({devices: [0, 0], loopback: true}) gives what the single-device Renderer gives, bit for bit; reprojection still throws."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ptmi import scene_io, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]

W, H = 48, 32


@pytest.fixture(scope="module")
def ptscene(tmp_path_factory):
    if not os.path.exists(os.path.join(HOST, "addon", "ptmi_napi.node")):             # normally built by __graft_entry__.build()
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "wgpu-path-tracing_amd"), "all"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(HOST, "addon")], stdout=subprocess.DEVNULL)
    path = tmp_path_factory.mktemp("multi_planes") / "cornell.ptscene"
    scene_io.save_ptscene(scenes.make("cornell"), str(path))
    return str(path)


def node(js):
    return json.loads(subprocess.check_output([NODE, "-e", js], text=True, timeout=300).strip().splitlines()[-1])


# one script, run for both Renderers: planes after 3 uniform frames, then adaptive rounds with their counts, then the denoiser
JS = ("var fs=require('fs'),h=require(%(host)r);var res={};var dump=function(name,a){fs.writeFileSync(%(dir)r+'/'+name,Buffer.from(a.buffer,a.byteOffset,a.byteLength))};"
      "var run=function(tag,opt){opt.width=%(W)d;opt.height=%(H)d;var r=new h.Renderer(opt);r.setAovs(['albedo','normal','id']);"
      "return r.loadModel(%(scene)r).then(function(){r.renderFrame(3);['albedo','normal','id'].forEach(function(k){dump(tag+'_'+k,r.readAov(k))});"
      "dump(tag+'_out',r.readOutput());"
      "r.setDenoise(true);r.setAdaptive({threshold:0.35,floor:0.05,minFrames:4,maxFrames:64,step:4,neighbourhood:1});var act=[];"
      "for(var i=0;i<4;i++){r.renderAdaptive(1);act.push(r.adaptiveStatus().active)}"
      "dump(tag+'_counts',r.sampleCounts());dump(tag+'_adaptive',r.readOutput());dump(tag+'_denoised',r.denoise());dump(tag+'_canvas',r.blitDenoised());"
      "res[tag]={active:act,status:r.adaptiveStatus()};r.destroy();});};"
      "run('one',{}).then(function(){return run('two',{devices:[0,0],loopback:true})}).then(function(){console.log(JSON.stringify(res))})")


def test_renderer_over_two_loopback_devices_equals_the_single_device_renderer(ptscene, tmp_path):
    res = node(JS % dict(host=os.path.join(HOST, "renderer.js"), dir=str(tmp_path), W=W, H=H, scene=ptscene))
    assert res["one"] == res["two"]
    act = res["one"]["active"]
    assert act[0] == W * H and 0 < act[-1] < W * H                   # the rounds made progress and did not finish: counts differ
    for name in ("albedo", "normal", "id", "out", "counts", "adaptive", "denoised", "canvas"):
        a, b = (np.fromfile(tmp_path / f"{tag}_{name}", np.uint8) for tag in ("one", "two"))
        assert a.size and np.array_equal(a, b), name
    counts = np.fromfile(tmp_path / "two_counts", np.float32)
    assert counts.size == W * H and counts.min() < counts.max()
    assert np.fromfile(tmp_path / "two_albedo", np.float32).any() and np.fromfile(tmp_path / "two_denoised", np.float32).any()


def test_set_reproject_still_throws_with_several_devices():
    js = ("var h=require(%r);var r=new h.Renderer({width:16,height:8,devices:[0,0],loopback:true});var out;"
          "try{r.setReproject({});out='no error'}catch(e){out=e.message}r.destroy();console.log(JSON.stringify(out))"
          % os.path.join(HOST, "renderer.js"))
    assert "not supported with several devices" in node(js)
