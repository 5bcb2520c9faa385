"""The branch census of the oracle (Oracle.render_census, oracle/pt_oracle.h): which branches of the bounce loop a render takes,
per bounce. Whole-frame parity with the oracle proves the `shade` kernel only on the branches the compared frames take; these
tests say which those are, on the CPU alone:
  * coverage: the gauntlet renders (tests/gauntlet_scenes.py; the GPU test compares exactly these) reach every event in every
    bounce class at least 16 times, but for the cells listed as impossible;
  * equivalence: the census changes nothing render() returns;
  * golden: the tables of the gauntlet renders, of the fog / sky gauntlet's (the oracle's extras; their coverage condition is in
    tests/test_oracle_extras_host.py) and of the ordinary parity renders are pinned (tests/golden/shade_census.json), so a change
    of the oracle's control flow shows."""
import json
import os

import numpy as np
import pytest

import gauntlet_scenes as G
from ptmi import layout, native, scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_census.json")
MIN_COUNT = 16

# Cells no scene can reach, each with its reason. Classes: A bounce 0; B bounces 1 .. rb; C bounce rb + 1; D later bounces
# (rb = G.repack_bounce(), the first bounce with Russian roulette).
EXEMPT = {
    ("miss_nonfinite", "A"): "the camera ray's throughput is 1",
    ("emissive_nonfinite", "A"): "the camera ray's throughput is 1",
    ("roulette_kill", "A"): "roulette is played from bounce rb on",
    ("roulette_survival", "A"): "roulette is played from bounce rb on",
    ("cs_roulette", "A"): "roulette is played from bounce rb on",
    # sampleBSDF returns the reflection when eta * sin_t > 1, which is k < 0 up to rounding; a negative eta, which would separate
    # the two tests, makes the Fresnel term >= 1 (or NaN with k = cos^2 >= 0), so refract() is not reached with k < 0
    ("refract_k_negative", "A"): "k < 0 is the total-internal-reflection test, taken first",
    ("refract_k_negative", "B"): "k < 0 is the total-internal-reflection test, taken first",
    ("refract_k_negative", "C"): "k < 0 is the total-internal-reflection test, taken first",
    ("refract_k_negative", "D"): "k < 0 is the total-internal-reflection test, taken first",
}


def extras_events(names):
    """the census events of pto_extras (oracle/pt_oracle.h), a contiguous run of the table"""
    return names[names.index("med_no_interval"):names.index("env_weight_at_scatter") + 1]


def classes(row):
    rb = G.repack_bounce()
    row = np.asarray(row, np.int64)
    return {"A": int(row[0]), "B": int(row[1:rb + 1].sum()), "C": int(row[rb + 1]), "D": int(row[rb + 2:].sum())}


@pytest.fixture(scope="module")
def gauntlet(oracle):
    """{(scene, max_bounces, tile): (image, stats, census)} of every render the GPU test compares"""
    out = {}
    for name, make in G.SCENES.items():
        sc = make()
        for mb, tile in G.oracle_renders():
            out[name, mb, tile] = G.render_census(oracle, sc, mb, tile)
    return out


def test_gauntlet_reaches_every_branch_in_every_bounce_class(oracle, gauntlet):
    names = oracle.census_events()
    total = {n: np.zeros(64, np.int64) for n in names}
    for _, _, cen in gauntlet.values():
        for n in names:
            total[n] += cen[n].astype(np.int64)
    # the events of the oracle's extras (the sky and the fog) are counted only with extras in place: never here; their own coverage
    # condition, over the fog / sky gauntlet, is in tests/test_oracle_extras_host.py
    extras = extras_events(names)
    assert len(extras) == 23 and not any(total[n].any() for n in extras)
    names = [n for n in names if n not in extras]
    assert {e for e, _ in EXEMPT} <= set(names)
    short = []
    for n in names:
        for cls, count in classes(total[n]).items():
            if (n, cls) in EXEMPT:
                assert count == 0, f"{n} in class {cls} is listed as impossible but happened {count} times"
            elif count < MIN_COUNT:
                short.append((n, cls, count))
    assert not short, f"cells reached fewer than {MIN_COUNT} times: {short}"


def test_gauntlet_scenes_are_small():
    for make in G.SCENES.values():
        assert len(make().tris) <= 400
    assert G.SIZE[0] * G.SIZE[1] <= 64 * 48 and G.FRAMES <= 8 and len(G.SCENES) <= 3


@pytest.mark.parametrize("name", list(G.SCENES) + ["feature_box"])
def test_census_changes_nothing(oracle, scene_factory, name):
    sc = G.SCENES[name]() if name in G.SCENES else scene_factory(name)
    cam = G.camera() if name in G.SCENES else layout.make_camera(48, 36)
    for mb in (8, 64):
        ref, rst = oracle.render(sc, cam, 3, max_bounces=mb, threads=1)
        tables = []
        for threads in (1, 4):
            out, st, cen = oracle.render_census(sc, cam, 3, max_bounces=mb, threads=threads)
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
            for k in ("paths", "segments", "shadow_rays", "nodes_visited", "tris_tested", "closest_hits", "max_stack"):
                assert getattr(st, k) == getattr(rst, k), k
            assert st.threads == threads
            fig = G.gpu_figures(cen, mb)
            assert int(cen["segment"].sum()) == st.segments and sum(fig["segments_by_bounce"]) == st.segments
            assert fig["shadow_rays"] == st.shadow_rays
            assert not cen["segment"][mb:].any()
            tables.append(np.stack([cen[n] for n in oracle.census_events()]))
        assert np.array_equal(tables[0], tables[1])              # per-thread tables, summed: no count lost or doubled


def parity_renders():
    """the renders of tests/test_gpu_parity.py whose branch coverage the golden records: (key, scene, camera, frames)"""
    out = []
    for name, W, H, frames, ap in (("feature_box", 72, 72, 6, 0.05), ("cornell", 96, 64, 6, 0.001),
                                   ("cornell_glass", 80, 60, 5, 0.0), ("cornell_spheres", 64, 48, 3, 0.001)):
        out.append((name, lambda n=name: scenes.make(n), layout.make_camera(W, H, aperture=ap, focus_distance=2.8), frames))
    for seed in range(8):
        cam = layout.make_camera(64, 48, aperture=0.02 if seed % 2 else 0.0, focus_distance=2.5)
        out.append(("random_soup_%d" % seed, lambda s=seed: scenes.random_soup(s), cam, 4))
    return out


def census_tables(oracle):
    """{render: {event: counts per bounce, trailing zeros cut}} — what tests/golden/make_golden.py writes"""
    def rows(cen):
        return {n: [int(v) for v in np.trim_zeros(r, "b")] for n, r in cen.items()}
    tables = {}
    for name, make in G.SCENES.items():
        sc = make()
        for mb, tile in G.oracle_renders():
            tables["%s-b%d%s" % (name, mb, "-rows" if tile else "")] = rows(G.render_census(oracle, sc, mb, tile)[2])
    fog = G.gauntlet_fog()                                       # the fog / sky gauntlet through the oracle's extras, every state
    for state in G.FOG_STATES:
        for mb, tile in G.fog_oracle_renders():
            cen = G.render_fog(oracle, fog, state, native.env_table, mb, tile)[3]
            tables["gauntlet_fog-%s-b%d%s" % (state, mb, "-rows" if tile else "")] = rows(cen)
    for key, make, cam, frames in parity_renders():
        tables[key] = rows(oracle.render_census(make(), cam, frames, max_bounces=8)[2])
    return tables


def test_census_tables_match_the_golden(oracle):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = census_tables(oracle)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_what_the_parity_scenes_do_not_reach():
    """The claims the docstrings of scenes.feature_box and scenes.random_soup make, from the golden tables: feature_box takes
    every lobe and light type but none of the degenerate branches; the soups take the NaN branches but few late bounces."""
    with open(GOLDEN) as f:
        t = json.load(f)
    fb = t["feature_box"]
    for ev in ("lobe_diffuse", "lobe_specular", "lobe_transmit_front", "lobe_transmit_back", "total_internal_reflection",
               "refraction", "normal_map", "nee_directional", "nee_point", "nee_emissive", "contribution_zero"):
        assert sum(fb[ev]) > 0, ev
    for ev in ("point_light_beyond_100", "material_out_of_range", "emissive_nonfinite", "miss_nonfinite", "nan_normal",
               "transmission_fractional", "normal_map_zero_det", "sample_pdf_not_positive", "contribution_nonfinite"):
        assert sum(fb[ev]) == 0, ev
    soups = [t["random_soup_%d" % s] for s in range(8)]
    assert all(sum(s["nan_normal"]) > 0 for s in soups)
    for ev in ("point_light_beyond_100", "material_out_of_range", "emissive_nonfinite"):
        assert all(sum(s[ev]) == 0 for s in soups), ev
