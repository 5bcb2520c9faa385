"""The library's own leaves (ptmi_options.leaves = 2, csrc/traverse_own.hip) on the GPU, through the C ABI.

The kernels descend a SAH hierarchy over the triangles themselves — a quarter of the triangle tests the reference's leaves
(src/renderer/bvh.ts:86-127) cost — and must still return what the reference's traversal returns (src/shader/pt.wgsl:248-291): the
winner is verified against the box of its reference leaf, and a ray the padded boxes are not proven for is traced over the tree as
uploaded. Checked here: every memory variant of both kernels against the oracle's (t, triangle, u, v) and shadow predicates on rays
of every kind; renders against the oracle bit for bit; and, at BASELINE.json's full sizes, the image of leaves = 2 against the image
of leaves = 1 (the mode every other parity test of this suite pins to the oracle) — more than 10^8 rays per configuration, with the
number of rays that had to be traced again reported."""
import os

import numpy as np
import pytest

from ptmi import layout, native
from test_gpu_parity import _test_rays, assert_same_floats, bits

pytestmark = pytest.mark.gpu

# PT_VARIANT_OWN_* x 10 + workgroups per CU (csrc/pt_device.h), as ptmi_stats.extend_variant / shadow_variant report them
VARIANTS = {"lds": 41, "lds_nodes2": 52, "lds_nodes1": 51, "qlds": 61, "qlds_nodes2": 72, "qlds_nodes1": 71, "qglobal": 81, "global": 91,
            "lds16_nodes2": 102,          # exact nodes with 16-bit references and stack entries (scenes up to 4 096 triangles)
            "qlds16_nodes2": 112}         # quantised nodes with 16-bit references, 8 - 15 16-bit entries per lane, the node stack spills


@pytest.fixture()
def own_ctx(gpu_ctx):
    before = gpu_ctx.options()
    gpu_ctx.set_options(leaves=2, leaf_tris=0, keep_reference_tree=0, traversal=native.TRAVERSAL_AUTO, cull=1)
    yield gpu_ctx
    for k in ("PTMI_OWN_EXTEND", "PTMI_OWN_SHADOW", "PTMI_OWN_Q16_ENTRIES"):
        os.environ.pop(k, None)
    gpu_ctx.set_options(leaves=before.leaves, leaf_tris=before.leaf_tris, keep_reference_tree=0, traversal=native.TRAVERSAL_AUTO, cull=1,
                        max_bounces=8, do_mis=1, frames_per_batch=0, tile_y0=0, tile_y1=0)


def force(kind, code):
    """PTMI_OWN_EXTEND / PTMI_OWN_SHADOW = variant + 10 for two workgroups per CU, 20 for the compact-reference variant
    (csrc/traverse_pick.hip traverse_config)"""
    os.environ["PTMI_OWN_EXTEND" if kind == "extend" else "PTMI_OWN_SHADOW"] = {102: "20", 112: "21"}.get(code) or str(code // 10 + (10 if code % 10 == 2 else 0))


def more_rays(sc, n, seed):
    """_test_rays + origins far outside the scene and directions with a tiny or a huge component: the rays that take the slow way"""
    o, d = _test_rays(sc, n, seed)
    rng = np.random.default_rng(seed + 1)
    k = n // 10
    d[-k:, rng.integers(0, 3)] = np.float32(1e-20)
    far = slice(n - 2 * k, n - k)
    o[far] = (o[far] - d[far] * np.float32(500.0)).astype(np.float32)
    d[n - 3 * k:n - 2 * k, rng.integers(0, 3)] = np.float32(3e25)      # a component beyond 2^60: the reference's business too
    return o, d


@pytest.mark.parametrize("name", ["cornell", "feature_box", "cornell_spheres", "grid_1m"])
def test_every_memory_variant_returns_the_oracles_hits(own_ctx, oracle, scene_factory, name):
    sc = scene_factory(name)
    own_ctx.upload_scene(sc)
    o, d = more_rays(sc, 200_000, 41)
    ot, otri, ou, ov, _ = oracle.intersect(sc, o, d)
    rng = np.random.default_rng(9)
    dist = (rng.random(len(o)) * 2.5).astype(np.float32)
    dist[::5] = -1.0
    sel = (ot > 0) & (np.arange(len(o)) % 7 == 0)
    dist[sel] = ot[sel]                                        # the t < dist - 2e-6 edge
    occ_ref = oracle.occluded(sc, o, d, dist)
    ran = set()
    for tag, code in VARIANTS.items():
        for cull in (1, 0):
            own_ctx.set_options(cull=cull)
            force("extend", code)
            gt, gtri, gu, gv = own_ctx.debug_intersect(o, d)
            used = own_ctx.stats().extend_variant
            assert np.array_equal(gtri, otri), f"{name} {tag} (ran {used}) cull {cull}: {(gtri != otri).sum()} triangle ids differ"
            assert_same_floats(gt, ot, f"t ({tag})"); assert_same_floats(gu, ou, f"u ({tag})"); assert_same_floats(gv, ov, f"v ({tag})")
            force("shadow", code)
            g = own_ctx.debug_occluded(o, d, dist)
            assert np.array_equal(g, occ_ref), f"{name} {tag} cull {cull}: {(g != occ_ref).sum()} shadow predicates differ"
            ran.add((used, own_ctx.stats().shadow_variant))
    st = own_ctx.stats()
    assert st.leaves_used == 2
    # the variants that fit this scene really ran (the others fell back to the library's choice)
    # (Cornell: 634 nodes — 40 KB exact, 20 KB quantised — and 48 KB of triangles beside 60 / 64 KB of stacks)
    # (cornell_spheres: 2 038 nodes — 64 KB quantised: 8 16-bit entries per lane beside them in half a CU's LDS, in a tree 19 levels deep)
    want = {"cornell": {41, 51, 61, 72, 71, 81, 91, 102, 112}, "feature_box": {81, 91, 102, 112}, "cornell_spheres": {71, 81, 91, 112}, "grid_1m": {81, 91}}[name]
    assert want <= {u for u, _ in ran}, (name, sorted(ran))
    assert want <= {s for _, s in ran}, (name, sorted(ran))



@pytest.mark.parametrize("code", [41, 71, 102, 112])
def test_override_takes_the_reported_code(own_ctx, oracle, scene_factory, code):
    """PTMI_OWN_EXTEND / PTMI_OWN_SHADOW also take the code ptmi_stats reports (variant * 10 + workgroups per CU): the kernels run as
    that variant and still return the oracle's hits and verdicts"""
    sc = scene_factory("cornell")
    own_ctx.upload_scene(sc)
    os.environ["PTMI_OWN_EXTEND"] = os.environ["PTMI_OWN_SHADOW"] = str(code)
    o, d = more_rays(sc, 20_000, 3)
    ot, otri, _, _, _ = oracle.intersect(sc, o, d)
    gt, gtri, _, _ = own_ctx.debug_intersect(o, d)
    assert own_ctx.stats().extend_variant == code
    assert np.array_equal(gtri, otri); assert_same_floats(gt, ot, f"t ({code})")
    dist = (np.random.default_rng(4).random(len(o)) * 2.5).astype(np.float32)
    assert np.array_equal(own_ctx.debug_occluded(o, d, dist), oracle.occluded(sc, o, d, dist))
    assert own_ctx.stats().shadow_variant == code


RENDERS = [("cornell", 96, 64, 6, 8, 1, 0.001), ("cornell", 64, 64, 4, 4, 0, 0.001), ("cornell_glass", 80, 60, 5, 8, 1, 0.0),
           ("feature_box", 72, 72, 6, 8, 1, 0.05), ("cornell_spheres", 64, 48, 3, 8, 1, 0.001), ("grid_1m", 96, 54, 2, 8, 1, 0.001),
           ("deep_chain", 64, 48, 2, 8, 1, 0.0), ("cornell_enclosed", 64, 48, 3, 8, 1, 0.001)]


@pytest.mark.parametrize("case", RENDERS, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-b{c[4]}-mis{c[5]}")
@pytest.mark.parametrize("leaf_tris", [0, 1, 4, 8])
def test_render_parity_with_own_leaves(own_ctx, oracle, scene_factory, case, leaf_tris):
    name, W, H, frames, bounces, mis, ap = case
    sc = scene_factory(name)
    cam = layout.make_camera(W, H, aperture=ap, focus_distance=2.8)
    ref, ost = oracle.render(sc, cam, frames, max_bounces=bounces, do_mis=mis)
    own_ctx.set_options(leaf_tris=leaf_tris)
    own_ctx.upload_scene(sc)
    own_ctx.resize(W, H)
    own_ctx.set_options(max_bounces=bounces, do_mis=mis, tile_y0=0, tile_y1=0, frames_per_batch=0, cull=1)
    own_ctx.reset_stats()
    own_ctx.dispatch(cam, frames)
    got = own_ctx.read_output()
    st = own_ctx.stats()
    assert st.leaves_used == 2 and st.leaf_tris_used <= (leaf_tris or 32)
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got, ref, f"radiance {name} (own leaves of <= {leaf_tris or 'default'} triangles)")
    assert st.verify_failed <= 1e-4 * (st.segments + st.shadow_traced) + 2


@pytest.mark.parametrize("name,W,H,frames", [("deep_chain", 64, 48, 2), ("cornell", 96, 64, 4), ("cornell_spheres", 96, 64, 3), ("feature_box", 72, 72, 4)])
def test_spilling_short_stacks(own_ctx, oracle, scene_factory, name, W, H, frames):
    """The two-workgroup kernels over quantised nodes with compact references keep 8 - 15 16-bit entries per lane (node stack from one
    end, filed leaves from the other) and move the node stack to memory when the two meet: forced to 8 entries on trees 14 - 58 levels
    deep, renders and ray tables must still be the oracle's."""
    sc = scene_factory(name)
    os.environ["PTMI_OWN_Q16_ENTRIES"] = "8"
    force("extend", 112); force("shadow", 112)
    own_ctx.upload_scene(sc)
    o, d = more_rays(sc, 100_000, 5)
    ot, otri, ou, ov, _ = oracle.intersect(sc, o, d)
    gt, gtri, gu, gv = own_ctx.debug_intersect(o, d)
    assert own_ctx.stats().extend_variant == 112
    assert np.array_equal(gtri, otri); assert_same_floats(gt, ot, "t"); assert_same_floats(gu, ou, "u"); assert_same_floats(gv, ov, "v")
    dist = (np.random.default_rng(2).random(len(o)) * 2.5).astype(np.float32)
    assert np.array_equal(own_ctx.debug_occluded(o, d, dist), oracle.occluded(sc, o, d, dist))
    cam = layout.make_camera(W, H, aperture=0.001, focus_distance=2.8)
    ref, ost = oracle.render(sc, cam, frames, max_bounces=8, do_mis=1)
    own_ctx.resize(W, H)
    own_ctx.set_options(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, frames_per_batch=0, cull=1)
    own_ctx.reset_stats()
    own_ctx.dispatch(cam, frames)
    got, st = own_ctx.read_output(), own_ctx.stats()
    assert (st.extend_variant, st.shadow_variant) == (112, 112)
    assert (st.segments, st.shadow_rays) == (ost.segments, ost.shadow_rays)
    assert_same_floats(got, ref, f"radiance {name}, 8-entry spilling stacks")


def test_random_scene_fuzz_with_own_leaves(own_ctx, oracle):
    """Seeded random scenes (degenerate triangles, zero normals, every lobe, textures, an axis-aligned directional light): both leaf
    modes, LDS and memory variants, against the oracle."""
    from ptmi import scenes
    for seed in range(6):
        sc = scenes.random_soup(seed, n_tris=400 + 150 * (seed % 4))
        W, H, frames = 96, 64, 3
        cam = layout.make_camera(W, H, aperture=0.03 * (seed % 3), focus_distance=2.5, frame_index=seed * 7)
        ref, ost = oracle.render(sc, cam, frames, max_bounces=8, do_mis=seed % 4 != 3)
        for trav in (native.TRAVERSAL_AUTO, native.TRAVERSAL_GLOBAL, native.TRAVERSAL_GLOBAL_EXACT):
            own_ctx.set_options(traversal=trav)
            own_ctx.upload_scene(sc); own_ctx.resize(W, H)
            own_ctx.set_options(max_bounces=8, do_mis=int(seed % 4 != 3), tile_y0=0, tile_y1=0, frames_per_batch=[0, 2][seed % 2])
            own_ctx.reset_stats()
            own_ctx.dispatch(cam, frames)
            got, st = own_ctx.read_output(), own_ctx.stats()
            assert (st.segments, st.shadow_rays) == (ost.segments, ost.shadow_rays), (seed, trav)
            assert_same_floats(got, ref, f"soup {seed} traversal {trav}")


FULL = [  # BASELINE.json configs[1..3] as written (frames reduced where the config has 512 / the scene is 1 M triangles: stated)
    ("cornell", 1920, 1080, 64, 0.001, 5.0), ("cornell_spheres", 1920, 1080, 32, 0.001, 5.0), ("grid_1m", 1920, 1080, 16, 0.001, 5.0),
    ("cornell", 3840, 2160, 8, 0.05, 2.8)]


@pytest.mark.parametrize("case", FULL, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}")
def test_full_size_images_are_equal_between_the_leaf_modes(own_ctx, scene_factory, case, record_property):
    """BASELINE.json's configurations at full resolution: the frame rendered over the library's own leaves equals, bit for bit, the
    frame rendered over the reference's leaves — every one of the >= 10^8 rays of the render found the same (t, triangle) / verdict,
    or a pixel would differ — and the counters agree. (Rows of the leaves = 1 image are pinned to the oracle in test_gpu_full_size.py.)"""
    name, W, H, frames, ap, focus = case
    sc = scene_factory(name)
    cam = layout.make_camera(W, H, aperture=ap, focus_distance=focus)
    imgs, stats = [], []
    for leaves in (1, 2):
        own_ctx.set_options(leaves=leaves, leaf_tris=0)
        own_ctx.upload_scene(sc)
        own_ctx.resize(W, H)
        own_ctx.set_options(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, frames_per_batch=0, cull=1)
        own_ctx.reset_stats()
        own_ctx.dispatch(cam, frames)
        imgs.append(own_ctx.read_output())
        stats.append(own_ctx.stats())
    a, b = stats
    assert (a.leaves_used, b.leaves_used) == (1, 2)
    assert (a.segments, a.shadow_rays, a.shadow_traced) == (b.segments, b.shadow_rays, b.shadow_traced)
    rays = b.segments + b.shadow_traced
    diff = (bits(imgs[0]) != bits(imgs[1])) & ~(np.isnan(imgs[0]) & np.isnan(imgs[1]))
    record_property("rays", int(rays)); record_property("retraced", int(b.verify_failed)); record_property("differing_floats", int(diff.sum()))
    print(f"{name} {W}x{H}x{frames}: {rays} rays, {b.verify_failed} traced again after a failed verification, {int(diff.sum())} differing floats")
    assert rays >= (1e8 if frames >= 16 else 5e7)
    assert not diff.any(), f"{int(diff.sum())} floats differ between the leaf modes"
    assert b.verify_failed <= 1e-5 * rays
