"""The gauntlet scenes (tests/gauntlet_scenes.py) on the GPU against the oracle: scenes built to take `shade` through the branches
the ordinary parity renders never reach (tests/test_shade_census_host.py proves on the CPU that they do, at every bounce class).
Radiance is compared bit for bit, NaN equal to NaN; paths, segments and shadow rays with the oracle's counters; and, new here,
ptmi_stats.segments_by_bounce and shadow_traced with figures derived from the oracle's branch census (G.gpu_figures has the
derivation) — both were only ever compared GPU against GPU. Options cover both sides of `shade`'s emit_records (overlap 0 / 2),
both traversal picks, bounce limits below, at and above the repack, the bounce-0 instantiation with first-hit planes, one frame
and many per batch, and a row range that ends the bounce-0 queue in a partial wave."""
import numpy as np
import pytest

import gauntlet_scenes as G
from test_gpu_parity import assert_same_floats

pytestmark = pytest.mark.gpu

_cache = {}


def reference(oracle, name, max_bounces, tile):
    """scene, and the oracle's image, stats and census of one render — computed once, shared, never written to"""
    if name not in _cache:
        _cache[name] = G.SCENES[name]()
    key = (name, max_bounces, tile)
    if key not in _cache:
        out, st, cen = G.render_census(oracle, _cache[name], max_bounces, tile)
        out.setflags(write=False)
        _cache[key] = (out, st, cen)
    return (_cache[name],) + _cache[key]


def case_id(c):
    return "b%d-overlap%d-trav%d-%s-fpb%d%s" % (c["max_bounces"], c["overlap"], c["traversal"], "planes" if c["planes"] else "plain",
                                                 c["frames_per_batch"], "-rows" if c["tile"] else "")


@pytest.mark.parametrize("case", G.gpu_cases(), ids=case_id)
@pytest.mark.parametrize("name", list(G.SCENES))
def test_gauntlet_render_and_counters(gpu_ctx, oracle, name, case):
    sc, ref, ost, cen = reference(oracle, name, case["max_bounces"], case["tile"])
    if case["tile"]:
        W, H, (y0, y1) = G.TILE_CASE["width"], G.TILE_CASE["height"], G.TILE_CASE["rows"]
        assert ((y1 - y0) * W) % 64 != 0
    else:
        (W, H), (y0, y1) = G.SIZE, (0, 0)
    cam = G.camera(W, H)
    want = G.gpu_figures(cen, case["max_bounces"])
    saved = gpu_ctx.options()
    try:
        gpu_ctx.upload_scene(sc)
        gpu_ctx.resize(W, H)
        if case["planes"]:
            gpu_ctx.set_aovs("albedo", "normal", "id")
            gpu_ctx.set_moments(True)
        gpu_ctx.set_options(max_bounces=case["max_bounces"], do_mis=1, tile_y0=y0, tile_y1=y1, tile_parts=0,
                            frames_per_batch=case["frames_per_batch"], cull=1, traversal=case["traversal"],
                            overlap=case["overlap"], perf_mode=0)
        gpu_ctx.reset_stats()
        gpu_ctx.dispatch(cam, G.FRAMES)
        got, st = gpu_ctx.read_output(), gpu_ctx.stats()
    finally:
        gpu_ctx.set_aovs()
        gpu_ctx.set_moments(False)
        gpu_ctx.set_options(**{k: getattr(saved, k) for k in ("max_bounces", "do_mis", "tile_y0", "tile_y1", "tile_parts",
                                                             "frames_per_batch", "cull", "traversal", "overlap", "perf_mode")})
    by_bounce = [int(v) for v in st.segments_by_bounce]
    print(name, case_id(case), "segments", st.segments, ost.segments, "shadow_rays", st.shadow_rays, ost.shadow_rays,
          "shadow_traced", st.shadow_traced, want["shadow_traced"], "by bounce", by_bounce[:8], want["segments_by_bounce"][:8])
    assert (st.paths, st.segments, st.shadow_rays) == (ost.paths, ost.segments, ost.shadow_rays)
    assert st.shadow_rays == want["shadow_rays"]
    nb = min(case["max_bounces"], 64)
    assert by_bounce[:nb] == want["segments_by_bounce"] and not any(by_bounce[nb:])
    assert st.shadow_traced == want["shadow_traced"]
    assert_same_floats(got, ref, f"radiance {name} {case_id(case)}")
