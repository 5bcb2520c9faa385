"""First-hit planes on the GPU (include/ptmi.h ptmi_set_aovs): the radiance keeps its bits with them on, one frame's planes against
the oracle's closest hits and tests/aov_ref.py, many frames folded across batches and dispatches, depth of field, row bands and
strips, the planes' life cycle and errors, perf mode, and the Node host's binding of them."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import aov_ref
from ptmi import layout, native, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("albedo", "normal", "id")
E_INVALID, E_STATE = -1, -4


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the planes and options it sets never reach the session's shared context"""
    c = native.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def setup(ctx, sc, W, H, aovs=ALL, **opt):
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=0,
             overlap=2, perf_mode=0, leaves=0, timing=0)
    o.update(opt)
    ctx.set_aovs()
    ctx.set_options(**o)
    ctx.upload_scene(sc)
    ctx.resize(W, H)
    ctx.set_aovs(*aovs)


def run(ctx, cam, dispatches):
    """dispatches: frame counts of consecutive dispatches starting at frame 0"""
    f0 = 0
    for n in dispatches:
        c = cam.copy()
        c["frame_index"] = f0
        ctx.dispatch(c, n)
        f0 += n
    return ctx.read_output()


def planes(ctx):
    return {n: ctx.read_aov(n) for n in ctx.aovs()}


def err(fn, *a):
    with pytest.raises(native.PtmiError) as e:
        fn(*a)
    return e.value.code


# 1 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "feature_box", "cornell_spheres"])
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("leaves", [1, 2])
def test_radiance_unchanged(ctx, oracle, scene_factory, name, overlap, leaves):
    sc = scene_factory(name)
    W, H = 40, 30
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H, aovs=(), overlap=overlap, leaves=leaves, frames_per_batch=2)
    off = run(ctx, cam, [3, 2])
    setup(ctx, sc, W, H, overlap=overlap, leaves=leaves, frames_per_batch=2)
    on = run(ctx, cam, [3, 2])
    assert np.array_equal(bits(on), bits(off)), f"{name}: radiance changes with the AOV planes on"
    ref, _ = oracle.render(sc, cam, 5, max_bounces=8, do_mis=1)
    assert np.array_equal(bits(on), bits(ref)), f"{name}: radiance differs from the oracle"
    p = planes(ctx)
    assert p["albedo"][..., 3].max() == 1.0            # the planes were written
    ctx.set_aovs()


# 2 -----------------------------------------------------------------------------------------------------------------------------------
def check_one_frame(sc, s, p, W, H, normal_tol=2e-6, mapped_tol=1e-4, albedo_bits=True):
    hit = s["hit"]
    ids = p["id"].reshape(-1, 2)
    assert np.array_equal(ids[:, 0], s["tri"]), "ID: triangle differs from the oracle's closest hit"
    assert np.array_equal(ids[:, 1], s["mat"]), "ID: material differs"
    a = p["albedo"].reshape(-1, 4)
    n = p["normal"].reshape(-1, 4)
    assert np.array_equal(bits(n[:, 3]), bits(s["t"])), "NORMAL.w differs from the oracle's t"
    assert np.array_equal(a[:, 3], hit.astype(np.float32)), "ALBEDO.w is not the coverage"
    assert not a[~hit].any() and not n[~hit].any()
    mats = sc.mats[np.where(hit, s["mat"], 0)]
    untextured = hit & ((mats["albedo_map"]["w"] == 0) | (mats["albedo_map"]["h"] == 0))
    base = mats["base_color"].astype(np.float32)
    assert np.array_equal(bits(a[untextured, :3]), bits(base[untextured])), "untextured albedo is not the base colour"
    ex = hit & s["albedo_exact"]
    if albedo_bits:
        assert np.array_equal(bits(a[ex, :3]), bits(s["albedo"][ex])), "textured albedo differs from the texel x base colour"
    else:
        assert np.abs(a[ex, :3] - s["albedo"][ex]).max(initial=0) < 1e-5
    plain = hit & ~s["normal_mapped"] & s["normal_exact"]
    mapped = hit & s["normal_mapped"] & s["normal_exact"]
    assert np.abs(n[plain, :3] - s["normal"][plain]).max(initial=0) < normal_tol
    assert np.abs(n[mapped, :3] - s["normal"][mapped]).max(initial=0) < mapped_tol
    return int(hit.sum()), int(mapped.sum())


@pytest.mark.parametrize("name", ["cornell", "feature_box"])
@pytest.mark.parametrize("leaves", [1, 2])
def test_one_frame_exact(ctx, oracle, scene_factory, name, leaves):
    sc = scene_factory(name)
    W, H = 48, 36
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H, leaves=leaves)
    run(ctx, cam, [1])
    p = planes(ctx)
    s = aov_ref.samples(oracle, sc, cam, 0)
    n_hit, n_mapped = check_one_frame(sc, s, p, W, H)
    assert n_hit > 0.5 * W * H
    if name == "feature_box":
        assert n_mapped > 0, "no normal-mapped pixel in view"
    ctx.set_aovs()


# 3 -----------------------------------------------------------------------------------------------------------------------------------
# Tolerances of the 16-frame fold: albedo and coverage 2 ulp-scale (1e-6: the per-sample albedo is exact, the fold emulation rounds
# the FMA twice); t 1e-6 relative; normals 1e-5 unmapped (per-sample 2e-6 plus the fold), 2e-4 where a normal map bent them.
@pytest.mark.parametrize("name", ["cornell", "feature_box"])
@pytest.mark.parametrize("leaves", [1, 2])
def test_many_frames_fold(ctx, oracle, scene_factory, name, leaves):
    sc = scene_factory(name)
    W, H = 32, 24
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H, leaves=leaves, frames_per_batch=4, overlap=1)
    run(ctx, cam, [8, 8])                                   # 16 frames, four batches, two dispatches
    p = planes(ctx)
    per = [aov_ref.samples(oracle, sc, cam, f) for f in range(16)]
    ra, rn, rid, exact = aov_ref.fold(per, list(range(16)))
    assert exact.mean() > 0.9
    a, n = p["albedo"].reshape(-1, 4), p["normal"].reshape(-1, 4)
    assert np.array_equal(p["id"].reshape(-1, 2), rid), "ID is not the last frame's"
    assert np.abs(a[exact] - ra[exact]).max() < 1e-6
    t_err = np.abs(n[:, 3] - rn[:, 3]) / np.maximum(np.abs(rn[:, 3]), 1e-30)
    assert t_err[exact & (rn[:, 3] != 0)].max() < 1e-6 and (n[rn[:, 3] == 0, 3] == 0).all()
    mapped = np.zeros(W * H, bool)
    for s in per:
        mapped |= s["normal_mapped"]
    assert np.abs(n[exact & ~mapped, :3] - rn[exact & ~mapped, :3]).max() < 1e-5
    assert np.abs(n[exact & mapped, :3] - rn[exact & mapped, :3]).max(initial=0) < 2e-4
    # the raw mean of unit normals: not unit length where the samples disagree (the caller normalises)
    ctx.set_aovs()


# 4 -----------------------------------------------------------------------------------------------------------------------------------
def test_depth_of_field_measures_from_the_lens(ctx, oracle, scene_factory):
    sc = scene_factory("cornell")
    W, H = 40, 30
    cam = layout.make_camera(W, H, aperture=0.2, focus_distance=2.0)
    setup(ctx, sc, W, H, aovs=("normal", "id"))
    run(ctx, cam, [1])
    n = ctx.read_aov("normal").reshape(-1, 4)
    s = aov_ref.samples(oracle, sc, cam, 0)
    assert np.array_equal(bits(n[:, 3]), bits(s["t"]))
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    o, d, _ = oracle.raygen(cam, xs, ys, np.zeros(W * H, np.uint32))
    lens = np.linalg.norm(o - np.asarray(cam["position"], np.float32), axis=1)
    assert lens.max() > 0.05                                # the rays start on the lens, not at the pinhole
    hit = s["hit"]
    p_hit = o[hit] + d[hit] * n[hit, 3:4]
    pin = np.linalg.norm(p_hit - np.asarray(cam["position"], np.float32), axis=1)
    assert np.abs(pin - n[hit, 3]).max() > 1e-3            # ... and t is measured from there
    ctx.set_aovs()


# 5 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [1, 2])
def test_row_bands_and_strips_leave_other_rows(ctx, oracle, scene_factory, leaves):
    sc = scene_factory("cornell")
    W, H = 32, 24
    cam = layout.make_camera(W, H)
    # a band of rows on zero-filled planes
    setup(ctx, sc, W, H, leaves=leaves, tile_y0=5, tile_y1=17)
    run(ctx, cam, [2])
    p = planes(ctx)
    rows = np.zeros(H, bool)
    rows[5:17] = True
    for k in ALL:
        assert not p[k][~rows].any(), f"{k}: rows outside the band were written"
    s1 = aov_ref.samples(oracle, sc, cam, 1)
    assert np.array_equal(p["id"][rows].reshape(-1, 2)[:, 0], s1["tri"].reshape(H, W)[rows].ravel())
    # interleaved strips over planes that hold a whole frame
    setup(ctx, sc, W, H, leaves=leaves)
    run(ctx, cam, [1])
    before = planes(ctx)
    ctx.set_options(tile_parts=3, tile_part=1, tile_strip=2)
    c = cam.copy()
    c["frame_index"] = 1
    ctx.dispatch(c, 1)
    after = planes(ctx)
    mine = np.array([((y // 2) % 3) == 1 for y in range(H)])
    for k in ALL:
        assert np.array_equal(after[k][~mine].view(np.uint32), before[k][~mine].view(np.uint32)), k
    assert np.array_equal(after["id"][mine][..., 0], s1["tri"].reshape(H, W)[mine])
    assert not np.array_equal(after["albedo"][mine].view(np.uint32), before["albedo"][mine].view(np.uint32))
    ctx.set_options(tile_parts=0, tile_part=0, tile_strip=0)
    ctx.set_aovs()


# 6 -----------------------------------------------------------------------------------------------------------------------------------
def test_life_cycle_and_errors(ctx, scene_factory):
    sc = scene_factory("cornell")
    W, H = 24, 16
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H, aovs=())
    L, h = ctx.L, ctx.h
    assert ctx.aovs() == ()
    assert L.ptmi_aov_device_ptr(h, native.AOV_ALBEDO) is None
    assert err(ctx.read_aov, "albedo") == E_STATE
    assert err(ctx.set_aovs, 8) == E_INVALID and ctx.aovs() == ()          # bad bits leave the mask as it was
    ctx.set_aovs("albedo", "id")
    assert ctx.aovs() == ("albedo", "id")
    assert L.ptmi_aov_device_ptr(h, native.AOV_ALBEDO) and L.ptmi_aov_device_ptr(h, native.AOV_ID)
    assert L.ptmi_aov_device_ptr(h, native.AOV_NORMAL) is None and L.ptmi_aov_device_ptr(h, 3) is None
    assert not ctx.read_aov("albedo").any() and not ctx.read_aov("id").any()        # zero-filled
    run(ctx, cam, [2])
    a = ctx.read_aov("albedo")
    assert a[..., 3].max() == 1.0
    # which must be one bit, the size exact
    buf = np.zeros(W * H * 16, np.uint8)
    assert L.ptmi_read_aov(h, 3, native._p(buf), buf.nbytes) == E_INVALID
    assert L.ptmi_read_aov(h, 0, native._p(buf), buf.nbytes) == E_INVALID
    assert L.ptmi_read_aov(h, native.AOV_ALBEDO, native._p(buf), buf.nbytes - 16) == E_INVALID
    assert L.ptmi_read_aov(h, native.AOV_ID, native._p(buf), buf.nbytes) == E_INVALID
    assert L.ptmi_read_aov(h, native.AOV_ID, native._p(buf), W * H * 8) == 0
    # turning another plane on keeps the planes already on
    ctx.set_aovs("albedo", "normal", "id")
    assert np.array_equal(ctx.read_aov("albedo").view(np.uint32), a.view(np.uint32))
    assert not ctx.read_aov("normal").any()
    # off, then read: E_STATE
    ctx.set_aovs("normal")
    assert err(ctx.read_aov, "albedo") == E_STATE and err(ctx.read_aov, "id") == E_STATE
    # resize zero-fills the planes that are on
    ctx.set_aovs(*ALL)
    run(ctx, cam, [1])
    assert ctx.read_aov("normal").any()
    ctx.resize(W, H)
    for k in ALL:
        assert not ctx.read_aov(k).any(), k
    ctx.resize(W + 8, H + 4)
    assert ctx.read_aov("id").shape == (H + 4, W + 8, 2)
    ctx.set_aovs()
    assert err(ctx.read_aov, "normal") == E_STATE


def test_empty_scene(ctx):
    full = scenes.make("cornell")
    empty = scenes.Scene("empty", np.zeros(0, layout.TRIANGLE), full.mats, np.zeros(0, layout.BVH_NODE),
                         np.zeros(0, layout.LIGHT), None)
    W, H = 17, 9
    setup(ctx, empty, W, H)
    run(ctx, layout.make_camera(W, H), [3])
    p = planes(ctx)
    assert not p["albedo"].any() and not p["normal"].any()
    assert (p["id"] == 0xFFFFFFFF).all()
    ctx.set_aovs()


def test_perf_mode_planes(ctx, oracle, scene_factory):
    sc = scene_factory("feature_box")
    W, H = 40, 30
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H, perf_mode=1)
    run(ctx, cam, [1])
    p = planes(ctx)
    s = aov_ref.samples(oracle, sc, cam, 0)
    # the traversal is the same kernel (t and ids exact); shade's fast reciprocal / square root move normals by a few ulp
    check_one_frame(sc, s, p, W, H, normal_tol=2e-5, mapped_tol=2e-4, albedo_bits=False)
    ctx.set_aovs()


# 7 -----------------------------------------------------------------------------------------------------------------------------------
def test_node_host_read_aov_and_pick(ctx, scene_factory, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "wgpu-path-tracing_amd", "host", "addon", "ptmi_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    sc = scene_factory("cornell")
    W, H = 32, 24
    blobs = tmp_path / "scene"
    blobs.mkdir()
    for k in ("tris", "mats", "nodes", "lights"):
        getattr(sc, k).tofile(blobs / f"{k}.bin")
    script = tmp_path / "aov.js"
    script.write_text(r"""
const fs = require('fs');
const { Renderer } = require(process.argv[2]);
const dir = process.argv[3], W = 32, H = 24;
const buf = (k) => { const b = fs.readFileSync(dir + '/' + k + '.bin'); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length); };
const r = new Renderer({ device: 0, width: W, height: H });
r.loadModel({ blobs: { triangles: buf('tris'), materials: buf('mats'), bvhNodes: buf('nodes'), lights: buf('lights') } }).then(() => {
  r.setAovs(['albedo', 'normal', 'id']);
  r.renderFrame(2);
  const alb = r.readAov('albedo'), ids = r.readAov('id');
  const picks = [];
  for (const [x, y] of [[0, 0], [16, 12], [5, 20], [31, 23]]) picks.push(r.pick(x, y));
  let bad = null;
  try { r.readAov('depth'); } catch (e) { bad = String(e.message); }
  process.stdout.write(JSON.stringify({ alb: Array.from(alb.slice(0, 64)), albLen: alb.length, idsType: ids.constructor.name,
                                        ids: Array.from(ids.slice(0, 64)), picks, bad }));
  r.destroy();
});
""")
    pkg = os.path.join(ROOT, "wgpu-path-tracing_amd", "host", "renderer.js")
    out = subprocess.run([node, str(script), pkg, str(blobs)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    setup(ctx, sc, W, H)
    run(ctx, layout.make_camera(W, H), [2])
    alb, ids, nrm = ctx.read_aov("albedo"), ctx.read_aov("id"), ctx.read_aov("normal")
    assert got["albLen"] == W * H * 4 and got["idsType"] == "Uint32Array"
    assert np.array_equal(np.asarray(got["alb"], np.float32), alb.ravel()[:64])
    assert np.array_equal(np.asarray(got["ids"], np.uint32), ids.ravel()[:64])
    for (x, y), pk in zip([(0, 0), (16, 12), (5, 20), (31, 23)], got["picks"]):
        tri, mat = ids[H - 1 - y, x]                        # pick() takes canvas rows (0 = top); the planes' row 0 is the bottom
        if tri == 0xFFFFFFFF:
            assert pk is None
        else:
            assert pk["triangle"] == tri and pk["material"] == mat
            assert np.float32(pk["depth"]) == nrm[H - 1 - y, x, 3]
    assert got["bad"]
    ctx.set_aovs()
