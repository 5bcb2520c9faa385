"""The own-leaf kernels (csrc/traverse_own.hip) on sliver triangles and grazing rays (tests/grazing_ref.py), through the C ABI.

Every memory variant of both kernels, with cull 1 and 0, and the reference's leaves (leaves = 1) beside them, must return the oracle's
(t, triangle, u, v) and shadow verdicts bit for bit. The retrace count of a closest-hit call (ptmi_stats.verify_failed, which also
counts a lane that ran out of stack and reported its hit unverified) must equal the CPU replay's over the image read back from the
device: which winner gets verified does not depend on the traversal order, and the replay's stack never runs out. The device-built
own tree (tree_builder = 2) is checked the same way, and a render of the strip floor seen from a few degrees above it must be the
oracle's and the leaves = 1 render's."""
import os

import numpy as np
import pytest

import grazing_ref as g
from test_gpu_own_leaves import VARIANTS, force, own_ctx  # noqa: F401  (own_ctx: the fixture, with its cleanup of the environment)
from test_gpu_parity import assert_same_floats

pytestmark = pytest.mark.gpu

QUANTISED = {6, 7, 8, 11}            # variant numbers (code // 10) that walk the quantised nodes
_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = {"fan300": lambda: g.sliver_fan(seed=2, n=300), "fan": lambda: g.sliver_fan(), "strip": lambda: g.sliver_strip(),
                        "fan_far": lambda: g.sliver_fan(transform="far"), "strip_far": lambda: g.sliver_strip(transform="far"),
                        "fan5000": lambda: g.sliver_fan(seed=7, n=5000)}[name]()
    return _cache[name]


def rays(oracle, sc, safe_origin, n=80_000):
    """grazing rays and a quarter as many control rays, the oracle's results, and the closest-hit records for the replay"""
    parts = [g.rays(sc, n, 200, "grazing", safe_origin), g.rays(sc, n // 4, 201, "control", safe_origin)]
    o = np.concatenate([p[0] for p in parts]); d = np.concatenate([p[1] for p in parts]); dist = np.concatenate([p[2] for p in parts])
    rec, ref = g.records(oracle, sc, o, d, dist)
    return o, d, dist, np.ascontiguousarray(rec[:len(o)]), ref


def check_call(ctx, L, sc, o, d, dist, rec, ref, what, cull):
    """one closest-hit and one any-hit call against the oracle; the closest-hit call's retrace count against the replay's"""
    ot, otri, ou, ov, occ = ref
    ctx.reset_stats()
    gt, gtri, gu, gv = ctx.debug_intersect(o, d)
    st = ctx.stats()
    assert np.array_equal(gtri, otri), f"{what}: {(gtri != otri).sum()} triangle ids differ"
    assert_same_floats(gt, ot, f"t ({what})"); assert_same_floats(gu, ou, f"u ({what})"); assert_same_floats(gv, ov, f"v ({what})")
    if st.leaves_used == 2:
        img = g.gate.Image(sc, 2, arrays=ctx.read_image())
        sums = g.replay(L, img, rec, 1 if st.extend_variant // 10 in QUANTISED else 0, cull, 0)[0]
        assert int(sums[8]) == 0
        assert st.verify_failed == int(sums[11]), f"{what}: {st.verify_failed} retraced on the device, {int(sums[11])} in the replay"
    g_occ = ctx.debug_occluded(o, d, dist)
    assert np.array_equal(g_occ, occ), f"{what}: {(g_occ != occ).sum()} shadow verdicts differ"
    # (a shadow ray stops at the first occluder it meets, which depends on the order: the verified one may differ from the replay's,
    # so its retraces are only bounded — by one per ray; the count is printed)
    shadow_redo = ctx.stats().verify_failed - st.verify_failed
    assert 0 <= shadow_redo <= len(o)
    print(f"{what}: {st.verify_failed} closest-hit and {shadow_redo} shadow rays retraced of {len(o)}")
    return st


def test_every_variant_returns_the_oracles_results_on_grazing_rays(own_ctx, oracle):
    L = g.gate.sim_lib()
    ran = set()
    for name in ("fan300", "fan", "strip", "fan_far", "strip_far"):
        sc = scene(name)
        own_ctx.set_options(leaves=2)
        own_ctx.upload_scene(sc)
        o, d, dist, rec, ref = rays(oracle, sc, own_ctx.read_image()[0].safe_origin, 40_000 if name != "strip" else 80_000)
        for tag, code in VARIANTS.items():
            for cull in (1, 0):
                own_ctx.set_options(cull=cull)
                force("extend", code); force("shadow", code)
                st = check_call(own_ctx, L, sc, o, d, dist, rec, ref, f"{name} {tag} cull {cull}", cull)
                assert st.leaves_used == 2
                ran.add(st.extend_variant); ran.add(own_ctx.stats().shadow_variant)
        for k in ("PTMI_OWN_EXTEND", "PTMI_OWN_SHADOW"):
            os.environ.pop(k, None)
        own_ctx.set_options(leaves=1)
        own_ctx.upload_scene(sc)
        for cull in (1, 0):
            own_ctx.set_options(cull=cull)
            assert check_call(own_ctx, L, sc, o, d, dist, rec, ref, f"{name} leaves 1 cull {cull}", cull).leaves_used == 1
    assert set(VARIANTS.values()) <= ran, sorted(ran)


def test_device_built_tree_on_a_large_sliver_scene(own_ctx, oracle):
    sc = scene("fan5000")
    L = g.gate.sim_lib()
    own_ctx.set_options(leaves=2, tree_builder=2)
    try:
        own_ctx.upload_scene(sc)
        assert own_ctx.stats().tree_builder_used == 2
        o, d, dist, rec, ref = rays(oracle, sc, own_ctx.read_image()[0].safe_origin, 100_000)
        for cull in (1, 0):
            own_ctx.set_options(cull=cull)
            check_call(own_ctx, L, sc, o, d, dist, rec, ref, f"fan5000 device tree cull {cull}", cull)
    finally:
        own_ctx.set_options(tree_builder=0)


def test_strip_floor_render_from_a_few_degrees_above(own_ctx, oracle):
    sc = scene("strip")
    W, H, frames = 96, 64, 4
    cam = g.strip_camera(W, H)
    ref, ost = oracle.render(sc, cam, frames, max_bounces=8, do_mis=1)
    imgs = []
    for leaves in (2, 1):
        own_ctx.set_options(leaves=leaves, leaf_tris=0)
        own_ctx.upload_scene(sc)
        own_ctx.resize(W, H)
        own_ctx.set_options(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, frames_per_batch=0, cull=1)
        own_ctx.reset_stats()
        own_ctx.dispatch(cam, frames)
        imgs.append(own_ctx.read_output())
        st = own_ctx.stats()
        assert st.leaves_used == leaves and (st.segments, st.shadow_rays) == (ost.segments, ost.shadow_rays)
    assert (ref[..., :3] > 0).mean() > 0.1                        # the floor is lit and seen (the lower part of the picture)
    assert_same_floats(imgs[0], ref, "strip floor, leaves = 2")
    assert_same_floats(imgs[0], imgs[1], "strip floor, leaves = 2 against leaves = 1")
