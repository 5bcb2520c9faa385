"""ptmi_options.tree_builder = 2: the traversal hierarchy over the uploaded leaves is built on the GPU (csrc/gpu_tree.hip: Morton-order
linear BVH — radix sort, Karras' radix tree, bottom-up fit) instead of by the host's SAH builder. The leaves (triangle ranges, exact boxes)
are the reference's either way and inner boxes are exact unions, so every (t, triangle, u, v), every shadow predicate and every radiance
bit must equal the oracle's — through the LDS kernels, the quantised image and the exact image in global memory, with rays of every kind.
Reference: src/renderer/bvh.ts:53-157 builds the leaves; src/shader/pt.wgsl:248-291 walks them.

Parity cannot fail because of the builder alone: a device build that fails falls back to the host's, and a wrong decision that still
yields a tree over exact unions gives right hits at another cost per ray. So beside parity this file pins the builder itself:
  * every case that asks the device to build asserts ptmi_stats.tree_builder_used == 2 (and the reporting contract of include/ptmi.h
    for the cases where nobody or the host builds);
  * the image a device build left (Context.read_image()) equals tests/lbvh_ref.py — a plain numpy model that finds the same unique
    tree by another algorithm — word for word: no tolerance, every comparison is equality of 32-bit words or small integers;
  * three uploads of one scene leave three identical images (k_fit hands boxes from the first thread at a node to the second).
Scenes of the image comparison (lbvh_ref.IMAGE_SCENES; their coverage is asserted on the CPU in tests/test_lbvh_ref_host.py):
cornell, cornell_spheres, feature_box (cornell: 4 of 321 leaves share a code), random_soup(80..83) (coincident triangle centroids, but
the leaves' codes come out distinct: 143 / 138 / 139 / 140 leaves), deep_chain (367 leaves, 31 distinct codes: the index bits decide;
the image that is not quantised), exactly 2, 3, 255, 256, 257 and 513 leaves (hand-written node arrays, one quad per leaf), a flat scene
(no extent in y and z), concentric quads (all 30 code bits equal), grid_320 and grid_1m.

Cost of the model on grid_1m (334 174 leaves, 26 levels), measured on the CPU: 0.46 s, beside 3.5 s to make the scene (once per
session) and 0.06 s for the oracle.intersect + oracle.occluded calls of this file's grid_1m parity case, timed in the same run (a
multi-threaded C library against single-threaded numpy). The model is therefore the dearer of the two, and the rule of this file is then
a smaller grid with more than 65 536 leaves: grid_320 = scenes.grid_1m(n=320), 203 532 triangles, 66 164 leaves, 22 levels, model 0.07 s
(n = 316 gives 64 162 leaves, too few). The full scene is compared as well, since half a second is no price for the one scene the
builder exists for. Both cases print their seconds.

Not checked here: the quantised plane qn of a device-built image. Its nodes are renumbered (top levels first), so decoding it needs a
joint walk of both images, not one containment loop; pt_quantize_tree runs on the host on whatever hierarchy it is given and
tests/test_traversal_image.py covers it. The wn equality is the core.

Found by the equality and three-upload cases (MI355X, 2026-10-16): equal on all scenes, three uploads identical. k_fit's ordering
(box stores, __threadfence(), the atomic on `arrived`, __threadfence(), volatile loads) stands as it is."""
import time

import numpy as np
import pytest

import lbvh_ref
from ptmi import layout
from test_gpu_edge_cases import tiny_scene
from test_gpu_parity import _test_rays, assert_same_floats

pytestmark = pytest.mark.gpu


@pytest.fixture()
def tb_ctx(gpu_ctx):
    from ptmi import native
    before = gpu_ctx.options().leaves
    gpu_ctx.set_options(tree_builder=2, keep_reference_tree=0, leaves=1)        # the builder of the hierarchy over the REFERENCE's leaves
    yield gpu_ctx
    gpu_ctx.set_options(leaves=before, tree_builder=0, traversal=native.TRAVERSAL_AUTO, cull=1, keep_reference_tree=0, overlap=2, frames_per_batch=0,
                        max_bounces=8, do_mis=1)


def upload_built_on_device(ctx, sc):
    """upload_scene, and the proof that the device built the hierarchy the rays will walk (a failed device build falls back silently)"""
    ctx.upload_scene(sc)
    st = ctx.stats()
    assert st.tree_builder_used == 2, f"{sc.name}: tree_builder = 2 was asked for, ptmi_stats.tree_builder_used is {st.tree_builder_used}"
    assert st.leaves_used == 1
    return st


@pytest.mark.parametrize("name", ["cornell", "cornell_spheres", "feature_box", "grid_1m"])
def test_gpu_built_tree_extend_and_shadow_parity(tb_ctx, oracle, scene_factory, name):
    from ptmi import native
    sc = scene_factory(name)
    upload_built_on_device(tb_ctx, sc)
    n = 120_000 if name == "grid_1m" else 200_000
    o, d = _test_rays(sc, n, 33)
    d[::23, 1] = 0.0                                           # irregular rays walk the uploaded tree beside the others
    d[::31] *= np.float32(3.0)
    t0 = time.perf_counter()
    ot, otri, ou, ov, _ = oracle.intersect(sc, o, d)
    t_oracle = time.perf_counter() - t0
    rng = np.random.default_rng(5)
    dist = (rng.random(len(o)) * 2.5).astype(np.float32)
    dist[::5] = -1.0
    t0 = time.perf_counter()
    occ_ref = oracle.occluded(sc, o, d, dist)
    print(f"{name}: oracle.intersect + oracle.occluded {t_oracle + time.perf_counter() - t0:.3f} s")
    for trav in (native.TRAVERSAL_AUTO, native.TRAVERSAL_GLOBAL, native.TRAVERSAL_GLOBAL_EXACT):
        for cull in (1, 0):
            tb_ctx.set_options(traversal=trav, cull=cull)
            gt, gtri, gu, gv = tb_ctx.debug_intersect(o, d)
            assert np.array_equal(gtri, otri), f"{(gtri != otri).sum()} triangle ids differ (traversal {trav}, cull {cull})"
            assert_same_floats(gt, ot, "t"); assert_same_floats(gu, ou, "u"); assert_same_floats(gv, ov, "v")
            assert np.array_equal(tb_ctx.debug_occluded(o, d, dist), occ_ref)


@pytest.mark.parametrize("name,W,H,frames", [("cornell", 160, 100, 4), ("cornell_spheres", 96, 64, 3), ("feature_box", 72, 72, 4)])
def test_gpu_built_tree_render_parity(tb_ctx, oracle, scene_factory, name, W, H, frames):
    sc = scene_factory(name)
    cam = layout.make_camera(W, H, aperture=0.01, focus_distance=2.8)
    ref, ost = oracle.render(sc, cam, frames, max_bounces=8, do_mis=1)
    upload_built_on_device(tb_ctx, sc)
    tb_ctx.resize(W, H)
    tb_ctx.reset_stats()
    tb_ctx.dispatch(cam, frames)
    got = tb_ctx.read_output()
    st = tb_ctx.stats()
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got, ref, f"radiance ({name}, hierarchy built on the GPU)")


@pytest.mark.parametrize("seed", range(4))
def test_gpu_built_tree_random_scene_fuzz(tb_ctx, oracle, seed):
    from ptmi import scenes
    sc = scenes.random_soup(80 + seed)                      # degenerate triangles, coincident centroids: equal Morton codes
    W, H, frames = 64, 48, 3
    cam = layout.make_camera(W, H, aperture=0.02 if seed % 2 else 0.0, focus_distance=2.5)
    ref, ost = oracle.render(sc, cam, frames, max_bounces=8, do_mis=1)
    upload_built_on_device(tb_ctx, sc)
    tb_ctx.resize(W, H)
    tb_ctx.reset_stats()
    tb_ctx.dispatch(cam, frames)
    st = tb_ctx.stats()
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(tb_ctx.read_output(), ref, f"radiance (seed {seed})")


# ---- who built: the reporting contract of ptmi_stats.tree_builder_used (include/ptmi.h), each time with the device asked for ----------
def test_kept_reference_tree_reports_no_builder(tb_ctx, scene_factory):
    tb_ctx.set_options(keep_reference_tree=1)
    tb_ctx.upload_scene(scene_factory("cornell"))
    assert tb_ctx.stats().tree_builder_used == 0
    tb_ctx.set_options(keep_reference_tree=0)                       # ... and the same scene without it: the device builds
    upload_built_on_device(tb_ctx, scene_factory("cornell"))


def test_empty_scene_reports_no_builder(tb_ctx):
    tb_ctx.upload_scene(tiny_scene(0))
    assert tb_ctx.stats().tree_builder_used == 0


@pytest.mark.parametrize("n_tris", [1, 4])
def test_single_leaf_reports_no_builder(tb_ctx, n_tris):
    """The uploaded root is a leaf: there is no hierarchy to build (build_image asks for two leaves), the root leaf is walked as it is"""
    sc = tiny_scene(n_tris)
    assert len(sc.nodes) == 1 and sc.nodes[0]["triangle_count"] == n_tris
    tb_ctx.upload_scene(sc)
    assert tb_ctx.stats().tree_builder_used == 0
    info = tb_ctx.read_image()[0]
    assert info.n_wnodes == 0 and info.root_ref == (lbvh_ref.REF_LEAF | (n_tris - 1) << lbvh_ref.LEAF_OFF_BITS)


@pytest.mark.parametrize("builder", [1, 0])
def test_host_builder_reports_itself(tb_ctx, scene_factory, builder):
    tb_ctx.set_options(tree_builder=builder)                        # 0: the library default, the host
    tb_ctx.upload_scene(scene_factory("cornell"))
    st = tb_ctx.stats()
    assert st.tree_builder_used == 1 and st.leaves_used == 1


# ---- the image itself against the model -------------------------------------------------------------------------------------------------
def device_image(ctx, sc):
    upload_built_on_device(ctx, sc)
    info, wn, qn, tp, lb = ctx.read_image()
    assert info.leaves_used == 1 and lb is None
    return info, wn


@pytest.mark.parametrize("name", lbvh_ref.IMAGE_SCENES)
def test_gpu_built_image_equals_the_model(tb_ctx, scene_factory, name):
    sc = lbvh_ref.image_scene(name, scene_factory)
    n_leaves = int((sc.nodes["triangle_count"] > 0).sum())
    if name.startswith("row"):
        assert n_leaves == int(name[3:])                            # the exact counts around the builder's block of 256 threads
    t0 = time.perf_counter()
    model = lbvh_ref.build(sc)
    print(f"{name}: {n_leaves} leaves, {model.depth} levels, model {time.perf_counter() - t0:.3f} s")
    info, wn = device_image(tb_ctx, sc)
    assert wn.shape == (n_leaves - 1, 16)
    msg = lbvh_ref.describe_mismatch(model, wn)
    assert msg is None, f"{name}: {msg}"
    assert np.array_equal(wn.view(np.uint32), model.wnodes.view(np.uint32))
    assert (info.n_wnodes, info.root_ref, info.depth) == (model.n_wnodes, model.root_ref, model.depth)
    if name == "deep_chain":
        assert not info.quantised                                   # the image whose exact nodes are the only ones


@pytest.mark.parametrize("name", ["cornell_spheres", "soup81"])
def test_three_uploads_build_the_same_image(tb_ctx, scene_factory, name):
    """Three, fixed. A difference would be a box word the second thread at a node read before the first had published it."""
    sc = lbvh_ref.image_scene(name, scene_factory)
    images = [device_image(tb_ctx, sc)[1].view(np.uint32).copy() for _ in range(3)]
    for k in (1, 2):
        differ = np.flatnonzero((images[k] != images[0]).any(axis=1))
        assert not len(differ), f"{name}: upload {k + 1} differs from the first in {len(differ)} nodes, first node {differ[0]}, words {np.flatnonzero(images[k][differ[0]] != images[0][differ[0]]).tolist()}"
    assert lbvh_ref.describe_mismatch(lbvh_ref.build(sc), images[0].view(np.float32)) is None
