"""The shading inputs on the GPU: the atlas lookup at its edges (both formats, non-square atlases, rects at and past the last
row and column, f16 specials, emissive maps), the atlas's life through the C ABI (uploads before the scene, swaps, removal,
rejected uploads) and bounce depths up to the ABI's 64 with the per-bounce counters. Renders are compared with the oracle
bit for bit; the emissive probe wall also with the plain float64 reference of tests/texture_ref.py."""
import copy

import numpy as np
import pytest

import texture_ref
from ptmi import layout, native, scenes

pytestmark = pytest.mark.gpu

SHAPES = [(67, 29), (3, 517), (65537, 3)]
_cache = {}


def edges(shape=(67, 29), fmt="f16"):
    if (shape, fmt) not in _cache:
        _cache[(shape, fmt)] = scenes.texture_edges(shape, fmt)
    return _cache[(shape, fmt)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_floats(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
    if bad.any():
        idx = np.argwhere(bad)[:5]
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} floats differ; first at {idx.tolist()}: "
                             f"gpu={a[tuple(idx[0])]!r} oracle={b[tuple(idx[0])]!r}")


def with_atlas(sc, atlas):
    s = copy.copy(sc)
    s.atlas = atlas
    return s


def upload_blobs(ctx, sc):
    """ptmi_upload_scene alone: the context's atlas stays as it is"""
    ctx._ck(ctx.L.ptmi_upload_scene(ctx.h, native._p(sc.tris), len(sc.tris), native._p(sc.mats), len(sc.mats),
                                    native._p(sc.nodes), len(sc.nodes), native._p(sc.lights), len(sc.lights)))


def upload_atlas(ctx, atlas, fmt=None, w=None, h=None):
    if atlas is None:
        return ctx._ck(ctx.L.ptmi_upload_atlas(ctx.h, None, 0, 0, 0))
    fmt = fmt if fmt is not None else (native.ATLAS_RGBA16F if atlas.dtype == np.float16 else native.ATLAS_RGBA32F)
    ctx._ck(ctx.L.ptmi_upload_atlas(ctx.h, native._p(atlas), atlas.shape[1] if w is None else w,
                                    atlas.shape[0] if h is None else h, fmt))


def render(ctx, sc, cam, frames, upload=True, **opt):
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, frames_per_batch=0, cull=1, traversal=0, overlap=2)
    o.update(opt)
    if upload:
        ctx.upload_scene(sc)
    ctx.resize(int(cam["width"]), int(cam["height"]))
    ctx.set_options(**o)
    ctx.reset_stats()
    ctx.dispatch(cam, frames)
    return ctx.read_output(), ctx.stats()


def restore(ctx):
    ctx.set_options(max_bounces=8, do_mis=1, overlap=2, traversal=0, frames_per_batch=0)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("bounces,mis", [(1, 0), (8, 1)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", ["f16", "f32"])
def test_texture_edges_render_parity(gpu_ctx, oracle, fmt, shape, bounces, mis, overlap):
    sc = edges(shape, fmt)
    cam = layout.make_camera(64, 48)
    frames = 3
    ref, ost = oracle.render(sc, cam, frames, max_bounces=bounces, do_mis=mis)
    got, st = render(gpu_ctx, sc, cam, frames, max_bounces=bounces, do_mis=mis, overlap=overlap)
    restore(gpu_ctx)
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got, ref, f"radiance {sc.name} b{bounces} mis{mis} overlap{overlap}")
    assert (got[..., :3] > 0).mean() > 0.3


def test_texture_edges_global_traversal(gpu_ctx, oracle):
    """the memory-walking traversal: its radiance buffer has the 16-byte stride"""
    sc = edges((67, 29), "f32")
    cam = layout.make_camera(64, 48)
    ref, ost = oracle.render(sc, cam, 2, max_bounces=8, do_mis=1)
    got, st = render(gpu_ctx, sc, cam, 2, traversal=native.TRAVERSAL_GLOBAL, overlap=1)
    restore(gpu_ctx)
    assert st.radiance_stride_bytes == 16 and st.traversal_used == native.TRAVERSAL_GLOBAL
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got, ref, "radiance, global traversal")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", ["f16", "f32"])
def test_emissive_probe_matches_the_plain_reference(gpu_ctx, fmt, shape):
    sc = edges(shape, fmt)
    W, H = 64, 48
    cam = layout.make_camera(W, H)
    got, _ = render(gpu_ctx, sc, cam, 1, max_bounces=1, do_mis=0)
    restore(gpu_ctx)
    ys, xs = np.mgrid[0:H, 0:W]
    o, d, _ = gpu_ctx.debug_raygen(cam, xs.ravel(), ys.ravel(), np.zeros(W * H, np.uint32))
    t, tri, u, v = gpu_ctx.debug_intersect(o, d)
    n_probe, n_exact = texture_ref.check(sc, got[..., :3].reshape(-1, 3), t, tri, u, v)
    assert n_probe > 0.4 * W * H and n_exact >= 0.95 * n_probe


def test_atlas_format_is_live(gpu_ctx, oracle):
    """the f32 atlas and the same atlas rounded to f16 (uploaded as RGBA16F) give different frames, each its oracle's"""
    sc32 = edges((67, 29), "f32")
    with np.errstate(over="ignore"):
        sc16 = with_atlas(sc32, np.ascontiguousarray(sc32.atlas.astype(np.float16)))
    cam = layout.make_camera(64, 48)
    outs = []
    for sc in (sc32, sc16):
        ref, _ = oracle.render(sc, cam, 2, max_bounces=8, do_mis=1)
        got, _ = render(gpu_ctx, sc, cam, 2)
        assert_same_floats(got, ref, f"radiance, {sc.atlas.dtype} atlas")
        outs.append(got)
    restore(gpu_ctx)
    assert (bits(outs[0]) != bits(outs[1])).mean() > 0.2


def test_atlas_lifecycle(gpu_ctx, oracle):
    """The atlas through the ABI, each step resumed from the last output (frame_index): uploaded before the scene, kept
    while the scene is replaced, swapped f16 -> f32 between two dispatches with no read in between, then removed - after
    which textured lookups read zero, not the fallback."""
    s16, s32 = edges((67, 29), "f16"), edges((67, 29), "f32")
    other = scenes.make("feature_box")                       # its rects partly cover the 67 x 29 atlas
    W, H = 48, 36
    cam = lambda f: layout.make_camera(W, H, frame_index=f)
    gpu_ctx.resize(W, H)
    gpu_ctx.set_options(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, frames_per_batch=0, overlap=1)
    upload_atlas(gpu_ctx, s16.atlas)
    upload_blobs(gpu_ctx, s16)
    gpu_ctx.dispatch(cam(0), 2)
    ref, _ = oracle.render(s16, cam(0), 2)
    assert_same_floats(gpu_ctx.read_output(), ref, "atlas uploaded before the scene")

    upload_blobs(gpu_ctx, other)
    gpu_ctx.dispatch(cam(2), 2)
    ref, _ = oracle.render(with_atlas(other, s16.atlas), cam(2), 2, out=ref.copy())
    assert_same_floats(gpu_ctx.read_output(), ref, "scene replaced, atlas kept")

    upload_blobs(gpu_ctx, s16)
    gpu_ctx.dispatch(cam(4), 1)
    upload_atlas(gpu_ctx, s32.atlas)
    gpu_ctx.dispatch(cam(5), 1)
    ref, _ = oracle.render(s16, cam(4), 1, out=ref.copy())
    ref, _ = oracle.render(s32, cam(5), 1, out=ref)
    assert_same_floats(gpu_ctx.read_output(), ref, "atlas swapped f16 -> f32 between dispatches")

    upload_atlas(gpu_ctx, None)
    gpu_ctx.dispatch(cam(6), 1)
    ref, _ = oracle.render(with_atlas(s32, None), cam(6), 1, out=ref.copy())
    assert_same_floats(gpu_ctx.read_output(), ref, "atlas removed")

    # without an atlas a textured lookup reads zero: the probes go dark, except the w = 0 / h = 0 rects (the fallback)
    got, _ = render(gpu_ctx, s32, cam(0), 1, upload=False, max_bounces=1, do_mis=0)
    ys, xs = np.mgrid[0:H, 0:W]
    o, d, _ = gpu_ctx.debug_raygen(cam(0), xs.ravel(), ys.ravel(), np.zeros(W * H, np.uint32))
    t, tri, _, _ = gpu_ctx.debug_intersect(o, d)
    mat = np.where(t > 0, s32.tris["material_index"][np.minimum(tri, len(s32.tris) - 1)], -1)
    rects = s32.mats["emissive_map"]
    rgb = got[..., :3].reshape(-1, 3)
    for m in texture_ref.probe_materials(s32):
        sel = mat == m
        assert sel.any()
        if rects[m]["w"] == 0 or rects[m]["h"] == 0:
            assert (rgb[sel] > 0).all(), f"material {m}: the fallback"
        else:
            assert not rgb[sel].any(), f"material {m}: no atlas reads zero"
    gpu_ctx.upload_scene(s16)
    restore(gpu_ctx)


def test_rejected_atlas_upload_changes_nothing(gpu_ctx, oracle):
    """an atlas of unknown format is refused, and the context keeps the atlas it had (include/ptmi.h)"""
    sc = edges((67, 29), "f16")
    cam = layout.make_camera(64, 48)
    gpu_ctx.upload_scene(sc)
    with pytest.raises(native.PtmiError) as e:
        upload_atlas(gpu_ctx, edges((67, 29), "f32").atlas, fmt=7)
    assert e.value.code == -1
    ref, ost = oracle.render(sc, cam, 2)
    got, st = render(gpu_ctx, sc, cam, 2, upload=False)
    restore(gpu_ctx)
    assert (st.segments, st.shadow_rays) == (ost.segments, ost.shadow_rays)
    assert_same_floats(got, ref, "radiance after a rejected atlas upload")


def test_rejected_atlas_upload_changes_no_shard(oracle):
    sc = edges((67, 29), "f16")
    W, H = 64, 48
    cam = layout.make_camera(W, H)
    ref, ost = oracle.render(sc, cam, 2)
    with native.MultiContext([0] * 3, loopback=True) as m:
        m.upload_scene(sc)
        a = edges((67, 29), "f32").atlas
        with pytest.raises(native.PtmiError) as e:
            m._ck(m.L.ptmi_multi_upload_atlas(m.h, native._p(a), a.shape[1], a.shape[0], 7))
        assert e.value.code == -1
        m.resize(W, H)
        m.set_options(max_bounces=8, do_mis=1)
        m.dispatch(cam, 2)
        got = m.read_output()
        st = m.stats()
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got, ref, "frame of three shards after a rejected atlas upload")


def test_atlas_size_overflow_is_rejected(gpu_ctx):
    """w * h * texel bytes past size_t is refused before anything is allocated or read (no dispatch here)"""
    one = np.zeros((1, 1, 4), np.float32)
    try:
        for fmt in (native.ATLAS_RGBA32F, native.ATLAS_RGBA16F):
            with pytest.raises(native.PtmiError) as e:
                upload_atlas(gpu_ctx, one, fmt=fmt, w=1 << 31, h=1 << 31)
            assert e.value.code == -1
        with native.MultiContext([0] * 2, loopback=True) as m:
            with pytest.raises(native.PtmiError) as e:
                m._ck(m.L.ptmi_multi_upload_atlas(m.h, native._p(one), 1 << 31, 1 << 31, native.ATLAS_RGBA32F))
            assert e.value.code == -1
    finally:
        gpu_ctx.upload_scene(edges((67, 29), "f16"))


def test_loopback_shards_with_an_f32_atlas(oracle):
    sc = edges((67, 29), "f32")
    W, H = 64, 48
    cam = layout.make_camera(W, H)
    ref, ost = oracle.render(sc, cam, 3, max_bounces=8, do_mis=1)
    with native.MultiContext([0] * 3, loopback=True) as m:
        m.upload_scene(sc)
        m.resize(W, H)
        m.set_options(max_bounces=8, do_mis=1, frames_per_batch=2)
        m.dispatch(cam, 2)
        m.dispatch(layout.make_camera(W, H, frame_index=2), 1)
        got = m.read_output()
        st = m.stats()
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got, ref, "frame assembled from 3 shards, f32 atlas")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("bounces", [9, 16, 63, 64])
@pytest.mark.parametrize("name", ["cornell_enclosed", "cornell_glass"])
def test_bounce_depths_past_8(gpu_ctx, oracle, scene_factory, name, bounces, overlap):
    """max_bounces up to the ABI's 64: per-bounce queue lengths and counters, and the overlap's event parity at the end of a
    batch. On 64 bounces the per-bounce segment counts are checked too: they sum to the segments, slot 0 is the paths, they
    never grow, nothing is counted past the limit, and slot k - 1 is what one more bounce adds in the oracle (the first
    k - 1 bounces do not depend on the limit)."""
    sc = scene_factory(name)
    W, H, frames = 32, 24, 2
    cam = layout.make_camera(W, H)
    ref, ost = oracle.render(sc, cam, frames, max_bounces=bounces, do_mis=1)
    got, st = render(gpu_ctx, sc, cam, frames, max_bounces=bounces, do_mis=1, overlap=overlap)
    restore(gpu_ctx)
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got, ref, f"radiance {name}, {bounces} bounces, overlap {overlap}")
    sb = np.array(st.segments_by_bounce[:], np.uint64)
    assert int(sb.sum()) == st.segments and int(sb[0]) == st.paths
    assert (np.diff(sb.astype(np.int64)) <= 0).all()
    assert not sb[bounces:].any()
    if bounces == 64:
        seg = {0: 0}
        for k in (1, 2, 3, 4, 8, 9, 32, 33, 63, 64):
            seg[k] = oracle.render(sc, cam, frames, max_bounces=k, do_mis=1)[1].segments
        for k in (1, 2, 3, 4, 9, 33, 64):
            assert int(sb[k - 1]) == seg[k] - seg[k - 1], (k, int(sb[k - 1]), seg[k] - seg[k - 1])
