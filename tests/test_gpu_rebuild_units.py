"""The unit list of ptmi_rebuild_tree (csrc/scene_rebuild.hip k_flag_leaves / k_flag_root, k_unit_tile_sums, k_unit_scatter; DESIGN.md
§16) on uploaded trees whose list is NOT the identity, whose leaves hold up to 32 triangles and whose ballot words fill more than one
tile of 1 024.

tests/test_gpu_rebuild_tree.py rebuilds trees straight from scene_host.build_bvh: every triangle listed (which[i] = i, every word
full), at most 4 triangles per leaf, at most 201 words. A scatter without a scan, a wrong exclusive offset, a dropped empty-word skip,
the two-word shifts of a wide leaf and everything a second tile runs (the sum of the tiles in front, w0, the count's writer) pass it
untouched. The scenes here are scenes.grid_1m trees operated on by tests/unit_list_ref.py (widen, drop), all legal uploads; the
census conditions that put each on its path are asserted on the host by tests/test_unit_list_host.py. One measurement of them:

  scene                    there for (csrc/scene_rebuild.hip)                                        census
  grid48/wide              flag_range's m << lo and m >> (64 - lo) with 17 .. 32 bits, lo in 33 .. 63,   4 428 units of 4 428, largest leaf 32,
                           under both builders                                                        68 leaves across a word edge, 63 of >= 17
  grid48/sparse            words that all have holes: the scan's offsets, not 64 * word; more than     1 755 units of 4 428, 70 of 70 words
                           4 096 triangles but at most 2 048 units, so own_leaves takes the host       partly filled
                           builder whichever is asked for
  grid182/wide+holes       exactly one full tile: thread 1023 of tile 0 holds a live word and writes   59 124 of 65 532, 1 024 words, the last
                           the count                                                                  with 60 bits, 360 partly filled
  grid183/plain            the smallest second tile: pre / tile_base / w0 with tile = 1, the count     66 258 of 66 258, 1 036 words, tiles
                           written by the last tile; all words full                                   [65 536, 722], 1 leaf across the tile edge
  grid183/edge             a tile total that is not 65 536 in front of tile 1; a leaf whose two        66 133, tiles [65 473, 660], 1 leaf across
                           atomicOr land in different tiles                                           the tile edge
  grid183/wide+holes       varying popcounts on both sides of the tile edge, wide straddles            59 604, tiles [58 904, 700], 794 straddles
                                                                                                      of >= 17
  grid320/empty-tile       three tiles in front; a tile whose total is 0; 1 024 empty words running    124 265 of 203 532, tiles [58 958, 0,
                           (the jm == 0 skip, a whole wave with nothing to write)                      59 178, 6 129], 1 024 empty words
  grid320/wide+empty-tile  the same with 32-triangle leaves, two of them across tile edges             124 284, tiles [59 076, 17, 59 082, 6 109]

The rule of every case is that of tests/test_gpu_rebuild_tree.py: context A uploads the operated scene, receives update_triangles(0,
moved) and rebuilds; context B freshly uploads `moved` with the operated nodes refitted (scene_update_ref.refit_nodes). `moved` is the
"wobble" deformation with POISON: every unlisted triangle is carried 64 scene extents away, in A's edit and in B's upload alike, so a
list that leaks one shows in the root box, the padding and the traces instead of cancelling between A and B. No tolerance anywhere.

  1. the list itself, against the independent model unit_list_ref.units: n_tris of the image and the original-triangle words of
     tripos, for A (the device's list) and for B (an upload's host-built list; under builder 2 the device builder's use of a
     non-identity `which`)
  2. A is B: same_images; builder_used agrees
  3. the bits: 20 000 rays, A against B and B against the CPU oracle, which walks the same operated nodes; no hit on an unlisted triangle
  4. the update plan re-made over a list with holes: a further update equals scene_update_ref.refit_image of the rebuilt image
  5. grid183/plain rebuilt without an edit reproduces the upload's image byte for byte

Which builder: own_leaves (csrc/scene_image.hip) takes the device builder for tree_builder = 2 above 4 096 triangles AND above 2 048
units; grid48/sparse therefore reports builder 1 whichever is asked for. The grid48 scenes run both builders with A uploaded under the
other one. From grid182 up the rebuild uses builder 2 only; A would be uploaded under builder 2 as well if an upload under the host
builder took more than about two seconds, but it takes 0.03 s for the 66 258 triangles of grid183 and 0.08 s for the 203 532 of
grid320 (UPLOAD_S below, measured on the parent commit), so A is uploaded under builder 1 everywhere. Either way A's image read
before the rebuild must differ from the one read after, so a rebuild that left the tree alone cannot pass.

Measured on the MI355X (parent commit's library): a device rebuild 5 ms (grid182, grid183) to 9 ms (grid320), the oracle 0.002 s per
scene, scene_update_ref.refit_image 0.05 s (grid182) and 0.12 s (grid320); the slowest case takes 0.6 s, most of it reading images."""
import dataclasses
import time

import numpy as np
import pytest

import scene_update_ref as ref
import unit_list_ref as U
from test_gpu_parity import _test_rays
from test_gpu_rebuild_tree import ctx_a, ctx_b, image_bytes, same_images  # noqa: F401  (the fixtures)
from test_gpu_scene_update import RAY_SEED, same_image, same_trace, scene, trace

pytestmark = pytest.mark.gpu

# 20 000 rays reach every tile of the floor. The oracle walks the uploaded nodes on all cores: 0.002 s for intersect + occluded on the
# 203 532 triangles of grid320, so the rays are not what a case's time goes to (that is the upload, the image reads and the models)
N_RAYS = 20_000
# seconds of upload_scene under tree_builder = 1 (the host builder and everything else an upload does), measured on the parent commit
# with the plain trees (under tree_builder = 2: 0.008, 0.009, 0.020)
UPLOAD_S = {"grid182": 0.035, "grid183": 0.029, "grid320": 0.076}

CASES = [(n, b) for n in U.SCENES for b in ((1, 2) if n.startswith("grid48") else (2,))]
_case, _oracle = {}, {}


def case(name):
    """(the operated scene, the poisoned wobble, the scene a fresh upload gets, who is listed [n_tris] bool, the model's unit list)"""
    if name not in _case:
        s = U.operated(name, scene)
        moved = U.poisoned(ref.deformed(s.tris, "wobble"), s.nodes, U.extent(s.tris))
        fresh = dataclasses.replace(s, tris=moved, nodes=ref.refit_nodes(s.nodes, moved))
        who = U.listed(s.nodes, len(s.tris))
        if not who.all():                                              # the poison is outside everything a ray can reach
            far = np.stack([moved[f][~who] for f in ("v0", "v1", "v2")]).reshape(-1, 3)
            assert np.abs(far).max() > 16 * U.extent(s.tris) and np.isfinite(far).all()
            assert np.abs(fresh.nodes[0]["aabb_max"]).max() < 2 * U.extent(s.tris)
        _case[name] = (s, moved, fresh, who, U.units(s.nodes, len(s.tris)))
    return _case[name]


def expected_builder(s, n_units, builder):
    """csrc/scene_image.hip own_leaves: the device builder above 4 096 triangles and above 2 048 units"""
    return 2 if builder == 2 and len(s.tris) > 4096 and n_units > 2048 else 1


def upload_builder(name, builder):
    """the builder A is uploaded under: the other one wherever the host builder is quick enough (everywhere: UPLOAD_S)"""
    return 3 - builder if name.startswith("grid48") or UPLOAD_S[name.split("/")[0]] < 2.0 else builder


def rays_for(sc):
    """tests/test_gpu_scene_update.py rays_for with N_RAYS rays"""
    o, d = _test_rays(sc, N_RAYS, RAY_SEED)
    d[::23, 1] = 0.0
    d[::31] *= np.float32(3.0)
    dist = (np.random.default_rng(RAY_SEED + 1).random(len(o)) * 2.5).astype(np.float32)
    dist[::5] = -1.0
    return o, d, dist


def rebuilt_and_fresh(ctx_a, ctx_b, name, builder):
    """A: uploaded, updated with the poisoned wobble, rebuilt with `builder`. B: the edited scene freshly uploaded under `builder`."""
    from ptmi import native
    s, moved, fresh, who, want = case(name)
    up = upload_builder(name, builder)
    ctx_a.set_options(leaves=2, tree_builder=up, keep_reference_tree=0, traversal=native.TRAVERSAL_AUTO, cull=1)
    ctx_b.set_options(leaves=2, tree_builder=builder, keep_reference_tree=0, traversal=native.TRAVERSAL_AUTO, cull=1)
    t0 = time.perf_counter()
    ctx_a.upload_scene(s)
    t_up = time.perf_counter() - t0
    assert ctx_a.stats().tree_builder_used == expected_builder(s, len(want), up)
    ctx_a.update_triangles(0, moved)
    before = ctx_a.read_image()
    st = ctx_a.rebuild_tree(builder)
    print(f"{name}: upload under builder {up} {t_up:.2f} s, rebuild with builder {builder} {st.build_ms:.2f} ms, "
          f"cost {st.cost_before:.4f} -> {st.cost_after:.4f}")
    assert st.builder_used == expected_builder(s, len(want), builder) == ctx_a.stats().tree_builder_used, (name, st.as_dict())
    assert image_bytes(before) != image_bytes(ctx_a.read_image()), f"{name}: the rebuild left the image as it was"
    ctx_b.upload_scene(fresh)
    assert ctx_b.stats().tree_builder_used == st.builder_used
    return s, moved, fresh, who, want


def assert_lists(img, want, n_triangles, what):
    info, tp = img[0], img[3]
    assert info.leaves_used == 2 and info.n_tris == len(want), f"{what}: {info.n_tris} units, the model lists {len(want)} of {n_triangles}"
    got = np.sort(tp.view(np.uint32)[:, 3])
    assert len(got) == len(want) and np.array_equal(got, want), f"{what}: {(got != want).sum() if len(got) == len(want) else '?'} entries differ"


# ---- 1, 2. the list, and the image of the fresh upload ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", CASES)
def test_rebuilt_list_is_the_models_and_the_image_the_fresh_uploads(ctx_a, ctx_b, name, builder):
    s, _, _, _, want = rebuilt_and_fresh(ctx_a, ctx_b, name, builder)
    what = f"{name} builder {builder}"
    a, b = ctx_a.read_image(), ctx_b.read_image()
    assert_lists(a, want, len(s.tris), f"{what}: rebuilt")
    assert_lists(b, want, len(s.tris), f"{what}: fresh")
    same_images(a, b, what)
    assert ctx_a.rebuild_status().builder_used == ctx_a.stats().tree_builder_used == ctx_b.stats().tree_builder_used


# ---- 3. the bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", CASES)
def test_rebuilt_context_traces_the_fresh_uploads_bits(ctx_a, ctx_b, oracle, name, builder):
    from ptmi import native
    s, _, fresh, who, _ = rebuilt_and_fresh(ctx_a, ctx_b, name, builder)
    if name not in _oracle:                                            # once per scene: both builders compare with it
        o, d, dist = rays_for(fresh)
        t0 = time.perf_counter()
        ot, otri, ou, ov, _ = oracle.intersect(fresh, o, d)
        _oracle[name] = ((o, d, dist), (ot, otri, ou, ov, oracle.occluded(fresh, o, d, dist)))
        print(f"{name}: the oracle on {N_RAYS} rays {time.perf_counter() - t0:.2f} s")
    (o, d, dist), want = _oracle[name]
    hit = want[0] > 0
    assert hit.mean() > 0.5 and who[want[1][hit]].all()
    what = f"{name} builder {builder}"
    for trav, cull in ((native.TRAVERSAL_AUTO, 1), (native.TRAVERSAL_AUTO, 0), (native.TRAVERSAL_GLOBAL_EXACT, 1)):
        ctx_a.set_options(traversal=trav, cull=cull)
        ctx_b.set_options(traversal=trav, cull=cull)
        a, b = trace(ctx_a, o, d, dist), trace(ctx_b, o, d, dist)
        same_trace(a, b, f"{what} traversal {trav} cull {cull}: rebuilt against fresh")
        same_trace(b, want, f"{what} traversal {trav} cull {cull}: fresh against the oracle")
        for got in (a, b):
            h = got[0] > 0
            assert (got[1][h] < len(s.tris)).all() and who[got[1][h]].all(), f"{what}: a ray hit an unlisted triangle"


# ---- 4. the plan re-made over a list with holes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid182/wide+holes", "grid320/empty-tile"])
def test_update_after_a_rebuild_over_a_list_with_holes(ctx_a, name):
    s, moved, _, _, want = case(name)
    ctx_a.set_options(leaves=2, tree_builder=upload_builder(name, 2), keep_reference_tree=0)
    ctx_a.upload_scene(s)
    ctx_a.update_triangles(0, moved)
    up0 = ctx_a.scene_update_status()
    st = ctx_a.rebuild_tree(2)
    img = ctx_a.read_image()
    up = ctx_a.scene_update_status()
    assert st.rebuilds == 1 and st.builder_used == 2 and st.build_ms > 0.0 and st.cost_before == up0.cost_now
    assert_lists(img, want, len(s.tris), name)
    # the project's reorder bound of at most 1e6 double additions: 1e-9 relative
    assert st.cost_after == pytest.approx(ref.image_cost(*img[:2]), rel=1e-9)
    assert up.cost_built == up.cost_now == st.cost_after
    assert up.updates == 1 and up.plan_ms > 0.0 and up.refit_ms == up0.refit_ms
    assert up.quantised_kept == (1 if img[0].quantised else 0)
    # further edits: the refit walks the NEW topology, over units that are not the triangles. "move" takes triangles n/3 .. n/2, which
    # in grid320/empty-tile are all unlisted (the image must then stay as it is); "squash" makes every third triangle a sliver
    changed = 0
    for k, kind in enumerate(("move", "squash")):
        moved = ref.deformed(moved, kind)
        t0 = time.perf_counter()
        model = ref.refit_image(*img, moved, s.nodes)
        print(f"{name}: refit_image {time.perf_counter() - t0:.2f} s")
        ctx_a.update_triangles(0, moved)
        after = ctx_a.read_image()
        same_image(after, model, f"{name}: the {kind} after the rebuild")
        assert_lists(after, want, len(s.tris), f"{name}: after the {kind}")
        up2 = ctx_a.scene_update_status()
        assert up2.updates == 2 + k and up2.cost_built == st.cost_after and up2.cost_now == pytest.approx(model.cost, rel=1e-9)
        changed += image_bytes(after) != image_bytes(img)
        img = after
    assert changed >= 1 and model.n_slivers > 0
    assert ctx_a.rebuild_status().rebuilds == 1


# ---- 5. no edit, the upload's builder, two tiles: the image byte for byte ----------------------------------------------------------------
def test_rebuild_without_an_edit_reproduces_a_two_tile_image(ctx_a):
    s, _, _, _, want = case("grid183/plain")
    ctx_a.set_options(leaves=2, tree_builder=2, keep_reference_tree=0)
    ctx_a.upload_scene(s)
    before = ctx_a.read_image()
    assert ctx_a.stats().tree_builder_used == 2 and ctx_a.rebuild_status().rebuilds == 0
    st = ctx_a.rebuild_tree(2)
    after = ctx_a.read_image()
    assert st.rebuilds == 1 and st.builder_used == 2 and st.cost_after == st.cost_before > 0.0
    assert_lists(after, want, len(s.tris), "grid183/plain")
    assert bytes(before[0]) == bytes(after[0])
    for x, y in zip(before[1:], after[1:]):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes())
