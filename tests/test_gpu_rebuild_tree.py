"""ptmi_rebuild_tree (include/ptmi.h; csrc/scene_rebuild.hip): the walked own-leaf tree rebuilt in place on the device.

The rule of every case, as in tests/test_gpu_scene_update.py: context A uploads scene S, is UPDATED with edited triangles and then
REBUILDS its walked tree; context B freshly UPLOADS the edited scene with the nodes refitted by tests/scene_update_ref.py refit_nodes,
under tree_builder = the rebuild's builder. A was uploaded under the OTHER builder, so a rebuild that left the tree alone could not
pass. Both builders are deterministic and read the same values, so A's image must be B's: references, triangle words and quantised
nodes by bits, boxes and header floats by value (which of -0 / +0 a tie returns is open), and A must trace and render B's bits, which
are the CPU oracle's. No tolerance anywhere. A ray on which B itself differs from the oracle would be the documented grazing freedom of
own leaves and call for another ray seed, not for a tolerance; with seed 71 none occurs.

grid48 (4 428 triangles) is the smallest scene the device builder accepts: its cases assert builder_used == 2, so a scene that slips
under the 4 096-triangle threshold fails loudly. grid80 is the device case with more than a handful of PLOC passes; cornell_spheres
takes the host builder with the 16-bit and quantised images.

Every case fails without the feature: the binding has no rebuild_tree."""
import dataclasses

import numpy as np
import pytest

import alpha_ref as A
import scene_update_ref as ref
from ptmi import layout
from test_gpu_parity import assert_same_floats
from test_gpu_scene_update import camera_for, edited, rays_for, render, same_image, same_trace, scene, trace

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -5
SCENES = ("grid48", "grid80", "cornell_spheres", "cornell", "tiny5")
CASES = [(n, k, b) for n in SCENES for k in ref.DEFORMATIONS for b in (1, 2)]
_oracle = {}


@pytest.fixture(scope="module")
def ctx_b():
    from ptmi import native
    with native.Context(0) as c:
        yield c


@pytest.fixture()
def ctx_a(gpu_ctx):
    from ptmi import native
    before = gpu_ctx.options().leaves
    yield gpu_ctx
    gpu_ctx.set_options(leaves=before, tree_builder=0, traversal=native.TRAVERSAL_AUTO, cull=1, keep_reference_tree=0, overlap=2,
                        frames_per_batch=0, max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0)


def expected_builder(s, builder):
    return 2 if builder == 2 and len(s.tris) > 4096 else 1


def rebuilt_and_fresh(ctx_a, ctx_b, name, kind, builder):
    """A: uploaded under the other builder, updated, rebuilt with `builder`. B: the edited scene freshly uploaded under `builder`."""
    from ptmi import native
    s = scene(name)
    moved, fresh = edited(s, kind)
    ctx_a.set_options(leaves=2, tree_builder=3 - builder, keep_reference_tree=0, traversal=native.TRAVERSAL_AUTO, cull=1)
    ctx_b.set_options(leaves=2, tree_builder=builder, keep_reference_tree=0, traversal=native.TRAVERSAL_AUTO, cull=1)
    ctx_a.upload_scene(s)
    assert ctx_a.stats().tree_builder_used == expected_builder(s, 3 - builder)
    ctx_a.update_triangles(0, moved)
    st = ctx_a.rebuild_tree(builder)
    assert st.builder_used == expected_builder(s, builder) == ctx_a.stats().tree_builder_used, (name, st.as_dict())
    ctx_b.upload_scene(fresh)
    assert ctx_b.stats().tree_builder_used == st.builder_used
    return s, moved, fresh


def same_images(a, b, what):
    """two read_image() results: references, triangle words, quantised nodes by bits; boxes and header floats by value"""
    (ia, wa, qa, ta, la), (ib, wb, qb, tb, lb) = a, b
    for f in ("leaves_used", "n_wnodes", "n_tris", "root_ref", "depth", "n_leaves", "max_leaf_tris", "quantised", "ref_depth"):
        assert getattr(ia, f) == getattr(ib, f), f"{what}: {f} {getattr(ia, f)} against {getattr(ib, f)}"
    for f in ("root_min", "root_max", "q_origin", "q_scale"):
        assert np.array_equal(np.array(getattr(ia, f), np.float32), np.array(getattr(ib, f), np.float32)), f"{what}: {f}"
    assert (ia.pad, ia.safe_origin) == (ib.pad, ib.safe_origin), what
    assert wa.shape == wb.shape and np.array_equal(wa[:, :12], wb[:, :12]), f"{what}: boxes"
    assert np.array_equal(wa.view(np.uint32)[:, 12:], wb.view(np.uint32)[:, 12:]), f"{what}: references"
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), f"{what}: triangle words"
    assert (qa is None) == (qb is None) and (qa is None or np.array_equal(qa, qb)), f"{what}: quantised nodes"
    assert np.array_equal(la, lb), f"{what}: leaf boxes"


def image_bytes(img):
    return b"".join(a.tobytes() for a in img[1:] if a is not None)


# ---- 1. the image is the fresh upload's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,builder", CASES)
def test_rebuilt_image_is_the_fresh_uploads(ctx_a, ctx_b, name, kind, builder):
    _, moved, _ = rebuilt_and_fresh(ctx_a, ctx_b, name, kind, builder)
    what = f"{name} {kind} builder {builder}"
    a, b = ctx_a.read_image(), ctx_b.read_image()
    assert a[0].leaves_used == 2
    same_images(a, b, what)
    if kind == "squash":
        assert int(ref.slivers(moved).sum()) > 0


# ---- 2. the bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,builder", CASES)
def test_rebuilt_context_traces_and_renders_the_fresh_uploads_bits(ctx_a, ctx_b, oracle, name, kind, builder):
    from ptmi import native
    _, _, fresh = rebuilt_and_fresh(ctx_a, ctx_b, name, kind, builder)
    cam, frames = camera_for(name)
    if (name, kind) not in _oracle:                                   # once per edited scene: both builders compare with it
        o, d, dist = rays_for(fresh)
        ot, otri, ou, ov, _ = oracle.intersect(fresh, o, d)
        _oracle[(name, kind)] = ((o, d, dist), (ot, otri, ou, ov, oracle.occluded(fresh, o, d, dist)),
                                 oracle.render(fresh, cam, frames, max_bounces=8, do_mis=1))
    (o, d, dist), want, (ref_img, ost) = _oracle[(name, kind)]
    what = f"{name} {kind} builder {builder}"
    for trav in (native.TRAVERSAL_AUTO, native.TRAVERSAL_GLOBAL, native.TRAVERSAL_GLOBAL_EXACT):
        for cull in (1, 0):
            ctx_a.set_options(traversal=trav, cull=cull)
            ctx_b.set_options(traversal=trav, cull=cull)
            a, b = trace(ctx_a, o, d, dist), trace(ctx_b, o, d, dist)
            same_trace(a, b, f"{what} traversal {trav} cull {cull}: rebuilt against fresh")
            same_trace(b, want, f"{what} traversal {trav} cull {cull}: fresh against the oracle")
            assert ctx_a.stats().extend_variant == ctx_b.stats().extend_variant, what     # the variant follows the new node count
    ctx_a.set_options(traversal=native.TRAVERSAL_AUTO, cull=1)
    ctx_b.set_options(traversal=native.TRAVERSAL_AUTO, cull=1)
    got_a, st_a = render(ctx_a, cam, frames)
    got_b, st_b = render(ctx_b, cam, frames)
    assert st_a == st_b == (ost.segments, ost.shadow_rays, ost.paths), what
    assert_same_floats(got_a, got_b, f"{what}: radiance, rebuilt against fresh")
    assert_same_floats(got_a, ref_img, f"{what}: radiance against the oracle")


# ---- 3. no edit, the upload's builder: the image byte for byte -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", [("grid80", 2), ("cornell_spheres", 1)])
def test_rebuild_without_an_edit_reproduces_the_image(ctx_a, name, builder):
    s = scene(name)
    ctx_a.set_options(leaves=2, tree_builder=builder, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    before = ctx_a.read_image()
    assert ctx_a.rebuild_status().rebuilds == 0 and ctx_a.rebuild_status().builder_used == 0
    st = ctx_a.rebuild_tree(builder)
    after = ctx_a.read_image()
    assert st.rebuilds == 1 and st.builder_used == builder and st.cost_after == st.cost_before > 0.0
    assert bytes(before[0]) == bytes(after[0])
    for x, y in zip(before[1:], after[1:]):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), name
    up = ctx_a.scene_update_status()
    assert up.updates == 0 and up.cost_built == up.cost_now == st.cost_after
    ctx_a.upload_scene(s)                                             # an upload zeroes the status
    z = ctx_a.rebuild_status()
    assert (z.rebuilds, z.builder_used, z.build_ms, z.cost_before, z.cost_after) == (0, 0, 0.0, 0.0, 0.0)


# ---- 4. the status, and the plan re-made for the new topology ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", [("grid48", 2), ("cornell_spheres", 1)])
def test_status_and_the_update_after_a_rebuild(ctx_a, ctx_b, name, builder):
    s = scene(name)
    moved, _ = edited(s, "wobble")
    ctx_a.set_options(leaves=2, tree_builder=3 - builder, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.update_triangles(0, moved)
    up0 = ctx_a.scene_update_status()
    st = ctx_a.rebuild_tree(builder)
    img = ctx_a.read_image()
    up = ctx_a.scene_update_status()
    print(f"{name} builder {builder}: cost {st.cost_before:.4f} -> {st.cost_after:.4f} (built {up0.cost_built:.4f}), {st.build_ms:.2f} ms")
    assert st.rebuilds == 1 and st.build_ms > 0.0 and st.cost_before == up0.cost_now
    # the project's reorder bound of at most 1e6 double additions: 1e-9 relative
    assert st.cost_after == pytest.approx(ref.image_cost(*img[:2]), rel=1e-9)
    assert up.cost_built == up.cost_now == st.cost_after
    assert up.updates == 1 and up.plan_ms > 0.0 and up.refit_ms == up0.refit_ms
    assert up.quantised_kept == (1 if img[0].quantised else 0)
    assert tuple(up.root_min) == tuple(up0.root_min) and tuple(up.root_max) == tuple(up0.root_max)
    stats = ctx_a.stats()
    assert stats.tree_builder_used == st.builder_used == builder and stats.leaf_tris_used == img[0].max_leaf_tris
    # a further edit: the refit walks the NEW topology
    moved2 = ref.deformed(moved, "move")
    model = ref.refit_image(*img, moved2, s.nodes)
    ctx_a.update_triangles(0, moved2)
    same_image(ctx_a.read_image(), model, f"{name}: the update after the rebuild")
    up2 = ctx_a.scene_update_status()
    assert up2.updates == 2 and up2.cost_built == st.cost_after and up2.cost_now == pytest.approx(model.cost, rel=1e-9)
    assert ctx_a.rebuild_status().rebuilds == 1
    fresh2 = dataclasses.replace(s, tris=moved2, nodes=ref.refit_nodes(s.nodes, moved2))
    ctx_b.set_options(leaves=2, tree_builder=builder, keep_reference_tree=0)
    ctx_b.upload_scene(fresh2)
    o, d, dist = rays_for(fresh2)
    same_trace(trace(ctx_a, o, d, dist), trace(ctx_b, o, d, dist), f"{name}: updated after the rebuild against a fresh upload")
    assert ctx_a.rebuild_tree(builder).rebuilds == 2


# ---- 5. what survives ----------------------------------------------------------------------------------------------------------------------
def test_alpha_motion_and_the_planes_survive_a_rebuild(ctx_a):
    zs = (0.4, 0.3)
    sc, cutoff = A.fence_scene(A.checker(2), z=zs)
    W, H = 48, 32
    cam = layout.make_camera(W, H, position=(0.0, 1.0, 2.8))
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(sc)
    assert ctx_a.read_image()[0].leaves_used == 2
    ctx_a.resize(W, H)
    try:
        ctx_a.set_aovs("normal")
        ctx_a.set_alpha_cutoff(cutoff, max_layers=3)
        ctx_a.set_motion(True)
        ctx_a.dispatch(cam, 3)
        first, count = len(sc.tris) // 4, len(sc.tris) // 3
        moved = ref.deformed(sc.tris, "wobble")
        ctx_a.update_triangles(first, moved[first:first + count])
        rng = np.random.default_rng(5)
        o = np.stack([rng.uniform(-0.9, 0.9, 4096), rng.uniform(0.1, 1.9, 4096), rng.uniform(1.2, 3.0, 4096)], 1).astype(np.float32)
        t = np.stack([rng.uniform(-1.1, 1.1, 4096), rng.uniform(-0.1, 2.1, 4096), rng.choice(zs, 4096)], 1)
        d = (t - o) / np.linalg.norm(t - o, axis=1, keepdims=True)
        d = d.astype(np.float32)
        hits = ctx_a.debug_alpha_intersect(o, d)
        assert hits[2].max() >= 1                                      # some rays pass holes
        before = (ctx_a.alpha_status().as_dict(), ctx_a.motion_status().as_dict(), ctx_a.debug_motion_prev(0, len(sc.tris)).tobytes(),
                  ctx_a.read_output().tobytes(), ctx_a.read_aov("normal").tobytes(), ctx_a.read_image()[4].tobytes())
        assert before[1]["on"] == 1 and (before[1]["dirty_first"], before[1]["dirty_count"]) == (first, count)
        assert before[0]["present"] == 1 and before[0]["n_cutout"] > 0 and np.frombuffer(before[3], np.float32).any()
        assert ctx_a.rebuild_tree().rebuilds == 1
        after = (ctx_a.alpha_status().as_dict(), ctx_a.motion_status().as_dict(), ctx_a.debug_motion_prev(0, len(sc.tris)).tobytes(),
                 ctx_a.read_output().tobytes(), ctx_a.read_aov("normal").tobytes(), ctx_a.read_image()[4].tobytes())
        assert before == after
        again = ctx_a.debug_alpha_intersect(o, d)
        assert np.array_equal(again[1], hits[1]) and np.array_equal(again[2], hits[2])
        assert_same_floats(again[0], hits[0], "debug_alpha_intersect across the rebuild")
    finally:
        ctx_a.set_motion(False)
        ctx_a.set_alpha_cutoff(None)
        ctx_a.set_aovs()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def state(c):
    return (bytes(c.read_image()[0]), image_bytes(c.read_image()), bytes(c.scene_update_status()), bytes(c.rebuild_status()))


def test_refusals_leave_the_context_unchanged(ctx_a):
    from ptmi import native
    from test_gpu_edge_cases import tiny_scene
    with native.Context(0) as empty:                                   # no scene loaded
        with pytest.raises(native.PtmiError) as e:
            empty.rebuild_tree()
        assert e.value.code == E_INVALID and empty.rebuild_status().rebuilds == 0
    s = scene("cornell")
    moved, _ = edited(s, "wobble")
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.update_triangles(0, moved)
    before = state(ctx_a)
    for kw in (dict(builder=3), dict(builder=0xFFFFFFFF), dict(reserved=(0, 0, 0, 0, 0, 0, 1)), dict(builder=1, reserved=(7, 0, 0, 0, 0, 0, 0))):
        with pytest.raises(native.PtmiError) as e:
            ctx_a.rebuild_tree(**kw)
        assert e.value.code == E_INVALID, kw
        assert state(ctx_a) == before, kw
    # images without own leaves
    single = tiny_scene(1)
    assert len(single.nodes) == 1
    for opts, sc, word in ((dict(leaves=1, keep_reference_tree=0), s, "leaves = 1"), (dict(leaves=2, keep_reference_tree=1), s, "keep_reference_tree"),
                           (dict(leaves=2, keep_reference_tree=0), single, "single leaf")):
        ctx_a.set_options(tree_builder=1, **opts)
        ctx_a.upload_scene(sc)
        if sc is s:
            ctx_a.update_triangles(0, moved)
        before = state(ctx_a)
        with pytest.raises(native.PtmiError) as e:
            ctx_a.rebuild_tree()
        assert e.value.code == E_UNSUPPORTED and word in str(e.value), (word, str(e.value))
        assert state(ctx_a) == before, word


# ---- 7. three fresh contexts -------------------------------------------------------------------------------------------------------------
def test_three_contexts_rebuild_identical_bytes():
    from ptmi import native
    s = scene("grid48")
    moved, _ = edited(s, "wobble")
    images = []
    for _ in range(3):
        with native.Context(0) as c:
            c.set_options(leaves=2, tree_builder=1)
            c.upload_scene(s)
            c.update_triangles(0, moved)
            st = c.rebuild_tree(2)
            assert st.builder_used == 2
            img = c.read_image()
            images.append((image_bytes(img), bytes(img[0]), st.cost_before, st.cost_after))
    assert images[0] == images[1] == images[2]


# ---- 8. several devices --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_rebuild_on_every_shard_assembles_the_single_device_frame(ctx_a, n):
    from ptmi import native
    s = scene("cornell")
    moved, _ = edited(s, "move")
    W, H, frames = 80, 50, 3
    cam = layout.make_camera(W, H)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.update_triangles(0, moved)
    one = ctx_a.rebuild_tree()
    single, _ = render(ctx_a, cam, frames)
    with native.MultiContext([0] * n, loopback=True) as m:
        m.upload_scene(s)
        m.resize(W, H)
        m.set_options(max_bounces=8, do_mis=1)
        m.update_triangles(0, moved)
        with pytest.raises(native.PtmiError) as e:                     # checked once, before any device changes
            m.rebuild_tree(builder=5)
        assert e.value.code == E_INVALID and m.rebuild_status().rebuilds == 0
        st = m.rebuild_tree()
        assert st.rebuilds == 1 and st.builder_used == one.builder_used
        assert (st.cost_before, st.cost_after) == (one.cost_before, one.cost_after)
        for i in range(n):
            same_images(m.read_image(i), ctx_a.read_image(), f"device {i} of {n}")
        m.dispatch(cam, frames)
        m.gather()
        assert_same_floats(m.read_output(), single, f"{n} rebuilt shards against one rebuilt device")
