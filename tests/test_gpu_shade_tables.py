"""The shade tables: `shade` serves materials, lights and the lights' triangles from LDS when they fit its budget, from memory when
they do not, and neither may change a float or a counter.

The tables are raw copies made at upload (csrc/pt_device.h): (n_mats + 1) x 128 B of materials (the last one zeros), and per light
48 + 128 B (the light, and at the same index the triangle an emissive light names). ptmi_stats.shade_tables reports the budget and
which tables the last dispatch staged. Every case renders 72 x 40, three frames, against the oracle bit for bit with equal
counters: the three parity scenes on the LDS path (all light types, MIS on and off, one and two streams, first-hit planes), scenes
padded with unused materials and further lights to one record under, at and one record over each threshold of the budget,
out-of-range material indices, no light and a single light, and a second upload into a context that has rendered another scene.

Left out: an emissive light whose triangle_index is >= n_tris. ptmi_upload_scene refuses it (checked here), so the kernel's zero
triangle for it cannot be reached through the ABI; n_lights = 0 with MIS on is kept (the oracle renders it)."""
import dataclasses

import numpy as np
import pytest

import gauntlet_scenes
from ptmi import layout, native

pytestmark = pytest.mark.gpu

W, H, FRAMES = 72, 40, 3
COUNTERS = ("paths", "segments", "shadow_rays", "shadow_traced", "frames", "dispatches")
MATS, LIGHTS = 1, 2                     # bits of the staged mask
MAT_B, LIGHT_B = 128, 48 + 128          # bytes of the tables per material / per light


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS) + tuple(int(v) for v in st.segments_by_bounce)


def budget_of(st):
    return int(st.shade_tables) & 0xFFFFFF


def staged_of(st):
    return (int(st.shade_tables) >> 28) & 3


def expected_stage(budget, n_mats, n_lights):
    """which tables fit: both, else the materials, else the lights"""
    m, l = (n_mats + 1) * MAT_B, n_lights * LIGHT_B
    if m + l <= budget:
        return MATS | (LIGHTS if n_lights else 0)
    if m <= budget:
        return MATS
    return LIGHTS if l <= budget and n_lights else 0


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: its uploads and options never reach the session's shared context"""
    c = native.Context(0)
    yield c
    c.close()


def render(ctx, sc, opt, aov=False, upload=True):
    o = dict(max_bounces=8, do_mis=1, overlap=2, traversal=0, tile_y0=0, tile_y1=0, frames_per_batch=0, perf_mode=0)
    o.update(opt)
    ctx.set_aovs()
    ctx.set_options(**o)
    if upload:
        ctx.upload_scene(sc)
    ctx.resize(W, H)
    if aov:
        ctx.set_aovs("albedo", "normal", "id")
    ctx.reset_stats()
    ctx.dispatch(layout.make_camera(W, H), FRAMES)
    out = ctx.read_output()
    planes = [ctx.read_aov(n) for n in ("albedo", "normal", "id")] if aov else []
    st = ctx.stats()
    ctx.set_aovs()
    return out, planes, st


_oracle_cache = {}


def oracle_render(oracle, key, sc, bounces=8, mis=1):
    """one oracle render per (scene, options), shared by the cases that need it and never written to"""
    k = (key, bounces, mis)
    if k not in _oracle_cache:
        ref, ost = oracle.render(sc, layout.make_camera(W, H), FRAMES, max_bounces=bounces, do_mis=mis)
        ref.setflags(write=False)
        _oracle_cache[k] = (ref, (ost.segments, ost.shadow_rays))
    return _oracle_cache[k]


def check(oracle, key, sc, got, st, mis=1, oracle_scene=None):
    """oracle_scene: sc without its unused materials (the same picture; one oracle render serves every padding)"""
    ref, cnt = oracle_render(oracle, key, oracle_scene or sc, mis=mis)
    print(f"{key}: n_mats {len(sc.mats)} n_lights {len(sc.lights)} budget {budget_of(st)} staged {staged_of(st)} "
          f"segments {st.segments} shadow rays {st.shadow_rays}")
    assert (st.segments, st.shadow_rays) == cnt
    assert same(got, ref), f"{key}: output differs from the oracle"
    assert staged_of(st) == expected_stage(budget_of(st), len(sc.mats), len(sc.lights))


# ---- the LDS path ----------------------------------------------------------------------------------------------------------------
LDS_CASES = [   # scene, do_mis, overlap, first-hit planes
    ("cornell", 1, 2, False), ("cornell", 1, 0, True), ("cornell", 0, 2, False), ("cornell", 0, 0, False),
    ("cornell_spheres", 1, 2, False), ("cornell_spheres", 1, 0, False), ("cornell_spheres", 0, 0, False),
    ("feature_box", 1, 2, False), ("feature_box", 1, 0, False), ("feature_box", 0, 2, False),
]


@pytest.mark.parametrize("name,mis,overlap,aov", LDS_CASES)
def test_parity_scenes_from_lds(ctx, oracle, scene_factory, name, mis, overlap, aov):
    sc = scene_factory(name)
    got, planes, st = render(ctx, sc, dict(do_mis=mis, overlap=overlap), aov)
    check(oracle, name, sc, got, st, mis=mis)
    assert staged_of(st) == MATS | LIGHTS and 0 < budget_of(st) <= 16384
    got2, planes2, st2 = render(ctx, sc, dict(do_mis=mis, overlap=overlap), aov, upload=False)
    assert same(got, got2) and counters(st) == counters(st2), "a second dispatch gave other bits or counters"
    for a, b in zip(planes, planes2):
        assert same(a, b)
    if aov:
        assert planes[0][..., 3].max() == 1.0                  # the planes were written


# ---- at the budget ---------------------------------------------------------------------------------------------------------------
def padded(sc, n_mats, n_lights):
    """sc with unused materials appended (copies of material 0: no triangle names them, the picture stays) and further lights
    (copies of its own, in turn: these are sampled, the picture changes with n_lights)"""
    assert n_mats >= len(sc.mats) and n_lights >= len(sc.lights) > 0
    mats = np.concatenate([sc.mats, np.repeat(sc.mats[:1], n_mats - len(sc.mats))])
    lights = np.concatenate([sc.lights, sc.lights[np.arange(n_lights - len(sc.lights)) % len(sc.lights)]])
    return dataclasses.replace(sc, mats=np.ascontiguousarray(mats), lights=np.ascontiguousarray(lights))


def budget(ctx, scene_factory):
    _, _, st = render(ctx, scene_factory("cornell"), {})
    return budget_of(st)


@pytest.mark.parametrize("which", ["both_under", "both_at", "both_over", "mats_at", "mats_over"])
def test_materials_around_the_budget(ctx, oracle, scene_factory, which):
    """feature_box with 8 lights and unused materials up to each threshold: the same picture whatever was staged"""
    B = budget(ctx, scene_factory)
    base = scene_factory("feature_box")
    nl = 8
    assert (B - nl * LIGHT_B) % MAT_B == 0 and B % MAT_B == 0, "the budget is not reachable to the byte with 8 lights"
    both_at, mats_at = (B - nl * LIGHT_B) // MAT_B - 1, B // MAT_B - 1
    n_mats, want = {"both_under": (both_at - 1, MATS | LIGHTS), "both_at": (both_at, MATS | LIGHTS), "both_over": (both_at + 1, MATS),
                    "mats_at": (mats_at, MATS), "mats_over": (mats_at + 1, LIGHTS)}[which]
    sc = padded(base, n_mats, nl)
    got, planes, st = render(ctx, sc, {}, aov=True)
    check(oracle, "feature_box_8_lights", sc, got, st, oracle_scene=padded(base, len(base.mats), nl))
    assert staged_of(st) == want
    first = _oracle_cache.setdefault("planes_8_lights", planes)
    for a, b in zip(planes, first):
        assert same(a, b), "the first-hit planes depend on what was staged"


@pytest.mark.parametrize("which", ["lights_under", "lights_over"])
def test_lights_around_the_budget(ctx, oracle, scene_factory, which):
    """materials past the budget, and lights one record under / over it (176 B records do not reach it to the byte)"""
    B = budget(ctx, scene_factory)
    base = scene_factory("feature_box")
    n_mats = B // MAT_B
    nl, want = {"lights_under": (B // LIGHT_B, LIGHTS), "lights_over": (B // LIGHT_B + 1, 0)}[which]
    sc = padded(base, n_mats, nl)
    got, _, st = render(ctx, sc, {})
    check(oracle, f"feature_box_{nl}_lights", sc, got, st)
    assert staged_of(st) == want
    got0, _, st0 = render(ctx, sc, dict(overlap=0), upload=False)
    assert same(got, got0) and counters(st) == counters(st0)


# ---- edge records ----------------------------------------------------------------------------------------------------------------
def test_material_index_past_the_table(ctx, oracle, scene_factory):
    """gauntlet_materials names materials n_mats and n_mats + 7: zeros, from LDS (the record behind the last) and from memory"""
    sc = gauntlet_scenes.gauntlet_materials()
    nm = len(sc.mats)
    assert (sc.tris["material_index"] >= nm).sum() > 20
    got, _, st = render(ctx, sc, {})
    check(oracle, "gauntlet_materials", sc, got, st)
    assert staged_of(st) & MATS
    # the same picture with the table past the budget: unused materials appended, the out-of-range indices moved behind them
    B = budget_of(st)
    big = padded(sc, B // MAT_B, len(sc.lights))
    tris = big.tris.copy()
    oob = tris["material_index"] >= nm
    tris["material_index"][oob] = np.where(tris["material_index"][oob] == nm, len(big.mats), 0xFFFFFFFF)
    big = dataclasses.replace(big, tris=tris)
    got2, _, st2 = render(ctx, big, {})
    assert not staged_of(st2) & MATS
    assert same(got2, got) and counters(st2) == counters(st)


def test_no_light_and_one_light(ctx, oracle, scene_factory):
    base = scene_factory("feature_box")
    none = dataclasses.replace(base, lights=np.zeros(0, layout.LIGHT))
    got, _, st = render(ctx, none, dict(do_mis=1))
    check(oracle, "feature_box_no_light", none, got, st)
    assert staged_of(st) == MATS and st.shadow_rays == 0
    for k in range(len(base.lights)):                          # each light alone: every type, rng_int(0, 0) still drawn
        one = dataclasses.replace(base, lights=np.ascontiguousarray(base.lights[k:k + 1]))
        got, _, st = render(ctx, one, dict(do_mis=1, overlap=k & 1))
        check(oracle, f"feature_box_light_{k}", one, got, st)
        assert staged_of(st) == MATS | LIGHTS


def test_emissive_light_without_a_triangle_is_refused(ctx, scene_factory):
    base = scene_factory("cornell")
    lights = base.lights.copy()
    assert lights[0]["light_type"] == layout.LIGHT_EMISSIVE
    lights[0]["triangle_index"] = len(base.tris)
    with pytest.raises(native.PtmiError):
        ctx.upload_scene(dataclasses.replace(base, lights=lights))


# ---- a second upload -------------------------------------------------------------------------------------------------------------
def test_reupload_rebuilds_the_tables(ctx, oracle, scene_factory):
    """scene B after scene A in one context = scene B in a fresh one: other materials in the same slots, other lights, and a table
    that moves between LDS and memory"""
    a = scene_factory("cornell")
    mats = a.mats.copy()
    mats["base_color"] = mats["base_color"][:, ::-1] * np.float32(0.9)
    mats["roughness"] = np.float32(0.3)
    mats["metallic"][0] = np.float32(0.5)
    lights = a.lights.copy()
    lights["color"] = lights["color"] * np.float32([0.5, 1.0, 0.25])
    b = dataclasses.replace(a, mats=mats, lights=lights[::-1].copy())
    B = budget(ctx, scene_factory)
    b_big = padded(b, B // MAT_B, len(b.lights))                # B with its materials past the budget
    fresh = {}
    for key, sc in (("b", b), ("b_big", b_big)):
        with native.Context(0) as c:
            fresh[key] = render(c, sc, {})
    check(oracle, "cornell_b", b, fresh["b"][0], fresh["b"][2])
    assert same(fresh["b"][0], fresh["b_big"][0])
    for first, then in ((a, "b"), (b_big, "b"), (a, "b_big"), (scene_factory("feature_box"), "b")):
        render(ctx, first, {})
        got, _, st = render(ctx, b if then == "b" else b_big, {})
        assert same(got, fresh[then][0]), "the second upload renders with records of the first"
        assert counters(st) == counters(fresh[then][2]) and staged_of(st) == staged_of(fresh[then][2])
