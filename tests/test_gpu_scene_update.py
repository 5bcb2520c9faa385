"""ptmi_update_triangles / _materials / _lights (include/ptmi.h; csrc/scene_update.hip): a loaded scene edited in place.

The rule of every case: context A uploads scene S and is then UPDATED with edited records; context B freshly UPLOADS the edited scene
with the nodes refitted by tests/scene_update_ref.py refit_nodes (tight boxes over the same topology). A, B and the CPU oracle must then
agree bit for bit: (t, triangle, u, v) and the shadow predicate on 100 000 rays (tests/test_gpu_parity.py _test_rays, with zeroed
direction components and scaled directions sprinkled in as tests/test_gpu_tree_builder.py does), and a small render with equal
segment and shadow-ray counts. No tolerance anywhere: any conservative hierarchy over the reference's leaves gives the same bits
(DESIGN.md §3.2), and a refit is one.

leaves = 1 is exact unconditionally. leaves = 2 carries the documented grazing-ray freedom of own leaves: a ray
within ~1e-3 rad of a non-sliver triangle's plane may differ from the oracle in a fresh upload as well. The comparison therefore asks
A == B on every ray first (that is this feature's claim) and then B == oracle; a ray on which B itself differs from the oracle is not
this feature's fault and calls for another ray seed (RAY_SEED), not for a tolerance. With seed 71 no such ray occurs in any case.

The image: after an update Context.read_image() equals scene_update_ref.refit_image(the image read before, the new triangles) -
references and triangle words by bits, boxes and header floats by value (which of -0 / +0 a tie returns is open), the quantised nodes
word for word. Three fresh contexts leave identical bytes; an update with the unmoved triangles leaves the image as it was.

Every case fails without the feature: the binding has no update_triangles."""
import dataclasses

import numpy as np
import pytest

import scene_update_ref as ref
from ptmi import layout, scenes
from test_gpu_edge_cases import tiny_scene
from test_gpu_parity import _test_rays, assert_same_floats

pytestmark = pytest.mark.gpu

RAY_SEED = 71
N_RAYS = 100_000
E_INVALID, E_UNSUPPORTED = -1, -5
_made = {}


def scene(name):
    if name not in _made:
        if name.startswith("soup"):
            _made[name] = scenes.random_soup(int(name[4:]))
        elif name.startswith("tiny"):
            _made[name] = tiny_scene(int(name[4:]))
        elif name.startswith("grid"):
            _made[name] = scenes.grid_1m(n=int(name[4:]))
        else:
            _made[name] = scenes.make(name)
    return _made[name]


def edited(s, kind):
    """(the deformed triangles, the scene a fresh upload gets: those triangles with the nodes refitted)"""
    key = (s.name, len(s.tris), kind)
    if key not in _made:
        moved = ref.deformed(s.tris, kind)
        _made[key] = (moved, dataclasses.replace(s, tris=moved, nodes=ref.refit_nodes(s.nodes, moved)))
    return _made[key]


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


def rays_for(sc):
    o, d = _test_rays(sc, N_RAYS, RAY_SEED)
    d[::23, 1] = 0.0                                           # irregular rays walk the uploaded tree beside the others
    d[::31] *= np.float32(3.0)
    dist = (np.random.default_rng(RAY_SEED + 1).random(len(o)) * 2.5).astype(np.float32)
    dist[::5] = -1.0
    return o, d, dist


def trace(ctx, o, d, dist):
    return ctx.debug_intersect(o, d) + (ctx.debug_occluded(o, d, dist),)


def same_trace(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: {(got[1] != want[1]).sum()} triangle ids differ"
    for k, n in ((0, "t"), (2, "u"), (3, "v")):
        assert_same_floats(got[k], want[k], f"{what}: {n}")
    assert np.array_equal(got[4], want[4]), f"{what}: {(got[4] != want[4]).sum()} shadow predicates differ"


def update(ctx, moved, two_ranges):
    if two_ranges:
        cut = max(1, len(moved) // 3)
        ctx.update_triangles(cut, moved[cut:])
        ctx.update_triangles(0, moved[:cut])
    else:
        ctx.update_triangles(0, moved)


def render(ctx, cam, frames):
    ctx.resize(int(cam["width"]), int(cam["height"]))
    ctx.reset_stats()
    ctx.dispatch(cam, frames)
    out, st = ctx.read_output(), ctx.stats()
    return out, (st.segments, st.shadow_rays, st.paths)


def camera_for(name):
    if name == "cornell":
        return layout.make_camera(160, 100, aperture=0.01, focus_distance=2.8), 4
    if name.startswith("tiny"):
        return layout.make_camera(40, 30, position=(0, 1.0, 1.5), aperture=0.0), 4
    return layout.make_camera(96, 64, aperture=0.01, focus_distance=2.8), 3


# (leaves, tree_builder, keep_reference_tree)
UPLOADS = [(2, 1, 0), (2, 2, 0), (1, 1, 0), (1, 2, 0), (2, 1, 1)]
PARITY = [(n, k) for n in ("cornell", "cornell_spheres", "feature_box", "soup80", "tiny4", "tiny5", "grid80") for k in ref.DEFORMATIONS]


@pytest.mark.parametrize("name,kind", PARITY)
def test_updated_context_traces_what_a_fresh_upload_traces(ctx_a, ctx_b, oracle, name, kind):
    from ptmi import native
    s = scene(name)
    moved, fresh = edited(s, kind)
    o, d, dist = rays_for(fresh)
    ot, otri, ou, ov, _ = oracle.intersect(fresh, o, d)
    want = (ot, otri, ou, ov, oracle.occluded(fresh, o, d, dist))
    cam, frames = camera_for(name)
    ref_img, ost = oracle.render(fresh, cam, frames, max_bounces=8, do_mis=1)
    for leaves, builder, keep in UPLOADS:
        what = f"{name} {kind} leaves {leaves} builder {builder} keep {keep}"
        for c in (ctx_a, ctx_b):
            c.set_options(leaves=leaves, tree_builder=builder, keep_reference_tree=keep, traversal=native.TRAVERSAL_AUTO, cull=1)
        ctx_a.upload_scene(s)
        update(ctx_a, moved, two_ranges=False)
        assert ctx_a.scene_update_status().updates == 1
        ctx_b.upload_scene(fresh)
        assert ctx_a.stats().leaves_used == ctx_b.stats().leaves_used
        if len(s.nodes) > 1:
            assert ctx_a.stats().leaves_used == (1 if keep else leaves)
        for trav in (native.TRAVERSAL_AUTO, native.TRAVERSAL_GLOBAL, native.TRAVERSAL_GLOBAL_EXACT):
            for cull in (1, 0):
                ctx_a.set_options(traversal=trav, cull=cull)
                ctx_b.set_options(traversal=trav, cull=cull)
                a, b = trace(ctx_a, o, d, dist), trace(ctx_b, o, d, dist)
                same_trace(a, b, f"{what} traversal {trav} cull {cull}: updated against fresh")
                same_trace(b, want, f"{what} traversal {trav} cull {cull}: fresh against the oracle")
        ctx_a.set_options(traversal=native.TRAVERSAL_AUTO, cull=1)
        ctx_b.set_options(traversal=native.TRAVERSAL_AUTO, cull=1)
        if builder == 1 or len(s.tris) > 4096:                     # (the device builder only differs above 4 096 triangles)
            got_a, st_a = render(ctx_a, cam, frames)
            got_b, st_b = render(ctx_b, cam, frames)
            assert st_a == st_b == (ost.segments, ost.shadow_rays, ost.paths), what
            assert_same_floats(got_a, got_b, f"{what}: radiance, updated against fresh")
            assert_same_floats(got_a, ref_img, f"{what}: radiance against the oracle")
        # the same edit in two ranges, the later range first: the same image, the same hits
        whole = ctx_a.read_image()
        ctx_a.upload_scene(s)
        update(ctx_a, moved, two_ranges=True)
        assert ctx_a.scene_update_status().updates == 2
        parts = ctx_a.read_image()
        for x, y in zip(whole[1:], parts[1:]):
            assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), what
        same_trace(trace(ctx_a, o, d, dist), want, f"{what}: two ranges against the oracle")


def test_large_grid_updated_under_auto_traversal(ctx_a, ctx_b, oracle):
    """scenes.grid_1m(n=320): 203 532 triangles, the device builder's own-leaf tree, the plain images"""
    from ptmi import native
    s = scene("grid320")
    moved, fresh = edited(s, "wobble")
    o, d, dist = rays_for(fresh)
    ot, otri, ou, ov, _ = oracle.intersect(fresh, o, d)
    want = (ot, otri, ou, ov, oracle.occluded(fresh, o, d, dist))
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=2, keep_reference_tree=0, traversal=native.TRAVERSAL_AUTO, cull=1)
    ctx_a.upload_scene(s)
    assert ctx_a.stats().tree_builder_used == 2
    update(ctx_a, moved, two_ranges=False)
    ctx_b.upload_scene(fresh)
    a, b = trace(ctx_a, o, d, dist), trace(ctx_b, o, d, dist)
    same_trace(a, b, "grid320: updated against fresh")
    same_trace(b, want, "grid320: fresh against the oracle")
    st = ctx_a.scene_update_status()
    print(f"grid320: plan {st.plan_ms:.2f} ms, refit {st.refit_ms:.2f} ms, cost {st.cost_built:.4f} -> {st.cost_now:.4f}")


# ---- the image ----------------------------------------------------------------------------------------------------------------------------
def same_image(got, model, what):
    info, wn, qn, tp, lb = got
    assert np.array_equal(wn[:, :12], model.wn[:, :12]), f"{what}: {(wn[:, :12] != model.wn[:, :12]).any(axis=1).sum()} nodes differ in a box"
    assert np.array_equal(wn.view(np.uint32)[:, 12:], model.wn.view(np.uint32)[:, 12:]), f"{what}: references"
    assert np.array_equal(tp.view(np.uint32), model.tp.view(np.uint32)), f"{what}: triangle words"
    assert (lb is None) == (model.lb is None) and (lb is None or np.array_equal(lb, model.lb)), f"{what}: leaf boxes"
    assert (qn is None) == (model.qn is None), f"{what}: quantised nodes present {qn is not None}, model {model.qn is not None}"
    if qn is not None:
        assert np.array_equal(qn, model.qn), f"{what}: {(qn != model.qn).any(axis=1).sum()} quantised nodes differ"
        assert np.array_equal(np.array(info.q_origin, np.float32), model.q_origin) and np.array_equal(np.array(info.q_scale, np.float32), model.q_scale)
    assert np.array_equal(np.array(info.root_min, np.float32), model.root_min) and np.array_equal(np.array(info.root_max, np.float32), model.root_max), what
    if info.leaves_used == 2:
        assert (info.pad, info.safe_origin) == (model.pad, model.safe_origin), what


IMAGES = [("cornell", 2, 1, 0), ("cornell_spheres", 2, 1, 0), ("feature_box", 2, 1, 0), ("soup81", 2, 1, 0), ("deep_chain", 2, 1, 0),
          ("tiny4", 2, 1, 0), ("grid80", 2, 2, 0), ("cornell", 2, 1, 1), ("cornell_spheres", 1, 1, 0), ("grid80", 1, 2, 0)]


@pytest.mark.parametrize("kind", ref.DEFORMATIONS)
@pytest.mark.parametrize("name,leaves,builder,keep", IMAGES)
def test_updated_image_equals_the_model(ctx_a, name, leaves, builder, keep, kind):
    s = scene(name)
    moved, _ = edited(s, kind)
    ctx_a.set_options(leaves=leaves, tree_builder=builder, keep_reference_tree=keep)
    ctx_a.upload_scene(s)
    if builder == 2:
        assert ctx_a.stats().tree_builder_used == 2
    before = ctx_a.read_image()
    assert ctx_a.scene_update_status().updates == 0 and ctx_a.scene_update_status().cost_built == 0.0
    model = ref.refit_image(*before, moved, s.nodes)
    ctx_a.update_triangles(0, moved)
    after = ctx_a.read_image()
    what = f"{name} {kind} leaves {leaves} builder {builder} keep {keep}"
    same_image(after, model, what)
    st = ctx_a.scene_update_status()
    # the reorder bound of at most 1e6 double additions: 1e-9 relative
    assert st.cost_built == pytest.approx(ref.image_cost(before[0], before[1]), rel=1e-9), what
    assert st.cost_now == pytest.approx(model.cost, rel=1e-9) and st.cost_now == pytest.approx(ref.image_cost(after[0], after[1]), rel=1e-9), what
    assert st.updates == 1 and st.plan_ms > 0.0 and st.refit_ms > 0.0
    assert st.quantised_kept == (1 if after[0].quantised else 0)
    if before[0].leaves_used == 1:
        assert st.quantised_kept == 0 and after[2] is None           # the stream of leaves = 1 is dropped, the exact nodes are walked
    if kind == "squash" and before[0].leaves_used == 2:
        assert model.n_slivers > 0
    # the root box of the tree as uploaded
    fresh_nodes = ref.refit_nodes(s.nodes, moved)
    assert np.array_equal(np.array(st.root_min, np.float32), fresh_nodes[0]["aabb_min"]) and np.array_equal(np.array(st.root_max, np.float32), fresh_nodes[0]["aabb_max"])


@pytest.mark.parametrize("name,leaves,builder", [("cornell_spheres", 2, 1), ("grid80", 2, 2), ("soup81", 1, 1)])
def test_identity_update_leaves_the_image_and_the_cost(ctx_a, name, leaves, builder):
    s = scene(name)
    ctx_a.set_options(leaves=leaves, tree_builder=builder, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    before = ctx_a.read_image()
    ctx_a.update_triangles(0, s.tris)
    ctx_a.update_triangles(len(s.tris) // 2, s.tris[len(s.tris) // 2:])
    ctx_a.update_triangles(3, s.tris[:0])                              # count = 0 is fine
    after = ctx_a.read_image()
    assert np.array_equal(after[1][:, :12], before[1][:, :12]) and np.array_equal(after[1].view(np.uint32)[:, 12:], before[1].view(np.uint32)[:, 12:])
    assert after[3].tobytes() == before[3].tobytes()
    if leaves == 2:
        assert np.array_equal(after[4], before[4]) and after[2].tobytes() == before[2].tobytes()
        assert (after[0].pad, after[0].safe_origin, tuple(after[0].q_scale)) == (before[0].pad, before[0].safe_origin, tuple(before[0].q_scale))
    st = ctx_a.scene_update_status()
    assert st.updates == 3 and st.cost_now == st.cost_built


@pytest.mark.parametrize("name,builder", [("cornell_spheres", 1), ("grid80", 2)])
def test_three_contexts_leave_identical_bytes(name, builder):
    from ptmi import native
    s = scene(name)
    moved, _ = edited(s, "wobble")
    images = []
    for _ in range(3):
        with native.Context(0) as c:
            c.set_options(leaves=2, tree_builder=builder)
            c.upload_scene(s)
            c.update_triangles(0, moved)
            img = c.read_image()
            st = c.scene_update_status()
            images.append((b"".join(a.tobytes() for a in img[1:] if a is not None), bytes(img[0]), st.cost_now))
    assert images[0] == images[1] == images[2]


# ---- materials and lights ---------------------------------------------------------------------------------------------------------------
def test_material_and_light_edits_render_what_a_fresh_upload_renders(ctx_a, ctx_b, oracle):
    s = scene("feature_box")
    cam, frames = layout.make_camera(72, 72, aperture=0.01, focus_distance=2.8), 3
    mats, lights = s.mats.copy(), s.lights.copy()
    mats["base_color"][1] = (0.1, 0.7, 0.3)
    emitter = int(np.flatnonzero(mats["emissive_strength"] * mats["emission"].max(axis=1) > 0)[0])
    mats["emission"][emitter] = (1.0, 0.4, 0.2)
    mats["emissive_strength"][emitter] *= 0.5
    point = int(np.flatnonzero(lights["light_type"] == layout.LIGHT_POINT)[0])
    lights["position"][point] += np.float32(0.2)
    lights["intensity"][point] *= np.float32(1.5)
    em = np.flatnonzero(lights["light_type"] == layout.LIGHT_EMISSIVE)
    assert len(em) > 1
    lights["triangle_index"][em[0]] = lights["triangle_index"][em[-1]]     # retargeted to another light's triangle
    fresh = dataclasses.replace(s, mats=mats, lights=lights)
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    base, _ = render(ctx_a, cam, frames)
    ctx_a.update_materials(0, mats)
    ctx_a.update_lights(point, lights[point:point + 1])
    ctx_a.update_lights(int(em[0]), lights[em[0]:em[0] + 1])
    assert ctx_a.scene_update_status().updates == 0                 # neither touches a tree
    ctx_b.upload_scene(fresh)
    got_a, st_a = render(ctx_a, cam, frames)
    got_b, st_b = render(ctx_b, cam, frames)
    assert st_a == st_b
    assert_same_floats(got_a, got_b, "materials and lights: updated against fresh")
    assert not np.array_equal(got_a, base)
    ref_img, ost = oracle.render(fresh, cam, frames, max_bounces=8, do_mis=1)
    assert st_a == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got_a, ref_img, "materials and lights: against the oracle")
    # light checks as at upload
    from ptmi import native
    bad = lights[em[0]:em[0] + 1].copy()
    bad["triangle_index"] = len(s.tris)
    with pytest.raises(native.PtmiError) as e:
        ctx_a.update_lights(int(em[0]), bad)
    assert e.value.code == E_INVALID
    bad["light_type"] = 9
    with pytest.raises(native.PtmiError) as e:
        ctx_a.update_lights(int(em[0]), bad)
    assert e.value.code == E_INVALID
    assert_same_floats(render(ctx_a, cam, frames)[0], got_a, "a refused light edit changes nothing")


def test_moved_emissive_triangles_light_the_scene_from_their_new_place(ctx_a, ctx_b, oracle):
    s = scene("cornell")
    cam, frames = layout.make_camera(96, 64, aperture=0.0), 4
    lit = np.unique(s.lights["triangle_index"][s.lights["light_type"] == layout.LIGHT_EMISSIVE])
    moved = ref.move_part(s.tris, lit, np.eye(3), (0.35, -0.5, 0.2))
    fresh = dataclasses.replace(s, tris=moved, nodes=ref.refit_nodes(s.nodes, moved))
    for c in (ctx_a, ctx_b):
        c.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    base, _ = render(ctx_a, cam, frames)
    ctx_a.update_triangles(int(lit.min()), moved[lit.min():lit.max() + 1])
    ctx_b.upload_scene(fresh)
    got_a, st_a = render(ctx_a, cam, frames)
    got_b, st_b = render(ctx_b, cam, frames)
    ref_img, ost = oracle.render(fresh, cam, frames, max_bounces=8, do_mis=1)
    assert st_a == st_b == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got_a, got_b, "moved light: updated against fresh")
    assert_same_floats(got_a, ref_img, "moved light: against the oracle")
    assert not np.array_equal(got_a, base)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_updates_leave_the_context_unchanged(ctx_a):
    from ptmi import native
    s = scene("cornell")
    cam, frames = layout.make_camera(64, 40), 2
    with native.Context(0) as empty:                                   # no scene loaded
        with pytest.raises(native.PtmiError) as e:
            empty.update_triangles(0, s.tris[:1])
        assert e.value.code == E_INVALID
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    base, _ = render(ctx_a, cam, frames)
    image = ctx_a.read_image()
    nan = s.tris[10:12].copy()
    nan["v1"][1, 2] = np.nan
    inf = s.tris[:1].copy()
    inf["v0"][0, 0] = np.inf
    for first, records in ((len(s.tris) - 1, s.tris[:2]), (len(s.tris) + 1, s.tris[:0]), (10, nan), (0, inf)):
        with pytest.raises(native.PtmiError) as e:
            ctx_a.update_triangles(first, records)
        assert e.value.code == E_INVALID
        assert ctx_a.scene_update_status().updates == 0
        again = ctx_a.read_image()
        assert all(x is None or x.tobytes() == y.tobytes() for x, y in zip(image[1:], again[1:]))
        assert_same_floats(render(ctx_a, cam, frames)[0], base, "render after a refused update")
    # a tree that is not nested is walked as uploaded: a refit would change what its boxes mean
    loose = s.nodes.copy()
    inner = int(np.flatnonzero(loose["triangle_count"] == 0)[1])
    loose["aabb_min"][inner] += np.float32(0.01)                       # no longer contains its children
    odd = dataclasses.replace(s, nodes=loose)
    ctx_a.upload_scene(odd)
    base, _ = render(ctx_a, cam, frames)
    with pytest.raises(native.PtmiError) as e:
        ctx_a.update_triangles(0, s.tris)
    assert e.value.code == E_UNSUPPORTED and "nested" in str(e.value)
    assert_same_floats(render(ctx_a, cam, frames)[0], base, "render after the unsupported update")


# ---- several devices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_update_on_every_shard_assembles_the_single_device_frame(ctx_a, n):
    from ptmi import native
    s = scene("cornell")
    moved, _ = edited(s, "move")
    W, H, frames = 80, 50, 3
    cam = layout.make_camera(W, H)
    ctx_a.set_options(leaves=2, tree_builder=1, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.update_triangles(0, moved)
    single, _ = render(ctx_a, cam, frames)
    with native.MultiContext([0] * n, loopback=True) as m:
        m.upload_scene(s)
        m.resize(W, H)
        m.set_options(max_bounces=8, do_mis=1)
        m.update_triangles(0, moved)
        st = m.scene_update_status()
        assert st.updates == 1 and st.cost_now == ctx_a.scene_update_status().cost_now
        m.dispatch(cam, frames)
        assert_same_floats(m.read_output(), single, f"{n} updated shards against one updated device")
        with pytest.raises(native.PtmiError) as e:
            m.update_triangles(len(s.tris), s.tris[:1])
        assert e.value.code == E_INVALID
