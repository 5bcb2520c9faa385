"""The licence of tests/test_gpu_alpha_per_sample.py, without a GPU ("A hole is an absent triangle, sample for sample").

The resolve loops of csrc/alpha.hip draw no random number and never touch a path's O / D, and a ray that passed holes reports the triangle
test's t from its own origin. A render under a cutoff table should therefore be, float for float, the render of the GHOST scene: the same
triangles, nodes, materials and lights with every hole triangle collapsed to a point, and no table (alpha_ref.ghost). Whether that holds
is decided here by what no kernel had a part in: the numpy model's two loops over the oracle's closest-hit probe on the cutout scene,
replayed on every ray of the oracle's render of the ghost scene (alpha_ref.replay). At the origin no ray may disagree, in any case of the
table the GPU test runs; a deliberately wrong model must disagree; 200 units out, where the triangle test leaks by itself, the rows that
hold a disagreeing ray are set aside, at most a quarter of them."""
import itertools

import numpy as np
import pytest

import alpha_ref as A
import gauntlet_scenes as G

CASES = A.per_sample_cases(G.repack_bounce())
SCENES = ("stripes", "checker2")
ROWS_ASIDE_CAP = 0.25


def test_the_case_table_covers_every_pair():
    rb = G.repack_bounce()
    plain = [c for c in CASES if not c["tile"]]
    assert len(CASES) == 12 and sum(c["tile"] for c in CASES) == 2
    assert {c["max_bounces"] for c in CASES} == {1, rb, rb + 1, rb + 2, 8}
    factors = dict(A._FACTORS)
    for k, vals in factors.items():                         # every value of every factor at every bounce limit
        assert {(c["max_bounces"], c[k]) for c in plain} == set(itertools.product((1, rb, rb + 1, rb + 2, 8), vals)), k
    for a, b in itertools.combinations(factors, 2):         # every pair of values of two factors
        assert {(c[a], c[b]) for c in plain} == set(itertools.product(factors[a], factors[b])), (a, b)
    W, (y0, y1) = A.TILE["width"], A.TILE["rows"]
    assert (y1 - y0) * W % 64 != 0 and (y1 - y0) * W * A.FRAMES % 64 != 0


def layers_of(case, n_fences):
    return n_fences if case["fence_layers"] else A.DEFAULT_LAYERS


def figures(what, r):
    print("%-44s rays %7d (closest %7d, shadow %7d), through holes %6d, path passes %6d, shadow passes %6d (lit side %6d of %6d samples)"
          % (what, r.n_rays, r.n_closest, r.n_shadow, r.through_holes, r.path_passes, r.shadow_passes, r.shadow_passes_lit, r.shadow_lit))


@pytest.mark.parametrize("name", SCENES)
def test_zero_disagreements_at_the_origin(oracle, name):
    """every (bounce limit, MIS, rows, layer limit) of the case table: no ray disagrees, none runs out of layers, rays pass holes; and
    the replay's reading of the tap is the oracle's own count: as many closest-hit rays as segments, as many shadow rays as the
    reference traces, as many on the lit side of their surface as samples that would leave a record, none of them grazing"""
    cut, cutoff, n_fences = A.case_scene(name)
    ghost, hole = A.ghost(cut, cutoff)
    assert 0 < hole.sum() < np.isin(cut.tris["material_index"], cut.info["fence_materials"]).sum()
    total = through = 0
    for mb, mis, tile, layers in sorted({(c["max_bounces"], c["do_mis"], c["tile"], layers_of(c, n_fences)) for c in CASES}):
        cam, rows = A.case_view(dict(tile=tile))
        r = A.replay(oracle, cut, cutoff, ghost, cam, A.FRAMES, rows, mb, mis, layers)
        figures("%s b%d mis%d%s layers %d:" % (name, mb, mis, " rows" if tile else "", layers), r)
        assert (r.disagreeing_closest, r.disagreeing_shadow, r.exhausted) == (0, 0, 0)
        assert r.path_passes > 0 and (r.shadow_passes > 0) == (mis == 1)
        _, st, census = oracle.render_census(ghost, cam, A.FRAMES, max_bounces=mb, do_mis=mis, y0=rows[0], y1=rows[1])
        want = G.gpu_figures(census, mb)
        assert (r.n_closest, r.n_shadow) == (st.segments, st.shadow_rays) and want["shadow_rays"] == st.shadow_rays
        assert r.shadow_grazing == 0 and r.shadow_lit == want["shadow_traced"]
        if mis:
            assert 0 < r.shadow_passes_lit <= r.shadow_passes and r.shadow_lit < r.n_shadow
        total, through = total + r.n_rays, through + r.through_holes
    print(name, "in all: %d rays, %d through holes" % (total, through))


@pytest.mark.parametrize("mis", [0, 1])
def test_zero_disagreements_on_the_edited_fence(oracle, mis):
    """the stripes fence moved, tilted and mirrored in u (alpha_ref.edited_fence), the nodes refitted: zero as well"""
    cut, cutoff, _ = A.case_scene("stripes")
    _, edited = A.edited_fence(cut)
    ghost, hole = A.ghost(edited, cutoff)
    assert hole.sum() == A.ghost(cut, cutoff)[1].sum()
    assert not np.array_equal(hole, A.ghost(cut, cutoff)[1])                # mirrored: other cells are holes now
    r = A.replay(oracle, edited, cutoff, ghost, A.case_camera(), A.FRAMES, (0, 0), 8, mis)
    figures("edited stripes b8 mis%d:" % mis, r)
    assert (r.disagreeing_closest, r.disagreeing_shadow, r.exhausted) == (0, 0, 0) and r.path_passes > 0 and r.shadow_grazing == 0


def test_the_check_can_fail(oracle, monkeypatch):
    """a replay that compared nothing would report zero for a wrong model too: the distance travelled in place of the test from the
    ray's own origin, and a step of PT_EPS alone 200 units out, must each disagree"""
    cut, cutoff, _ = A.case_scene("stripes")
    ghost, _ = A.ghost(cut, cutoff)
    cam = A.case_camera(A.FAR["size"])
    right = A.replay(oracle, cut, cutoff, ghost, cam, A.FAR["frames"], (0, 0), 8, 1)
    assert (right.disagreeing_closest, right.disagreeing_shadow) == (0, 0)
    with monkeypatch.context() as m:
        m.setattr(A, "hit_t", lambda scene, tri, o0, d, fallback: np.asarray(fallback, A.F))
        wrong = A.replay(oracle, cut, cutoff, ghost, cam, A.FAR["frames"], (0, 0), 8, 1)
    print("travelled + t for the distance: %d closest-hit rays disagree, %d shadow rays" % (wrong.disagreeing_closest, wrong.disagreeing_shadow))
    assert wrong.disagreeing_closest > 0 and wrong.path_passes == right.path_passes

    # On the tilted fence of the edit: a hit point on an axis-aligned plane z = const rounds onto the plane itself, where the triangle
    # test's t > PT_EPS rejects the triangle whatever the step is, and the wrong step would go unnoticed.
    far, far_cutoff, _ = A.case_scene("stripes", A.FAR["offset"])
    _, far = A.edited_fence(far, A.FAR["offset"])
    far_ghost, _ = A.ghost(far, far_cutoff)
    far_cam = A.case_camera(A.FAR["size"], A.FAR["offset"])

    def eps_step(o, d, t):
        o, d, t = np.asarray(o, A.F), np.asarray(d, A.F), np.asarray(t, A.F)
        p = A.fmaf(d, t[:, None], o)
        return A.fmaf(d, A.PT_EPS, p), (t + A.PT_EPS).astype(A.F)
    honest = A.replay(oracle, far, far_cutoff, far_ghost, far_cam, A.FAR["frames"], (0, 0), 8, 1)
    with monkeypatch.context() as m:
        m.setattr(A, "step", eps_step)
        wrong = A.replay(oracle, far, far_cutoff, far_ghost, far_cam, A.FAR["frames"], (0, 0), 8, 1)
    print("a step of PT_EPS at 200 units: %d + %d rays disagree, %d exhausted (the model's own step: %d + %d, %d)"
          % (wrong.disagreeing_closest, wrong.disagreeing_shadow, wrong.exhausted, honest.disagreeing_closest, honest.disagreeing_shadow,
             honest.exhausted))
    assert wrong.disagreeing_closest + wrong.disagreeing_shadow > 10 * (honest.disagreeing_closest + honest.disagreeing_shadow) + 10
    assert wrong.exhausted > 0 and honest.exhausted == 0


@pytest.mark.parametrize("mis", [0, 1])
def test_rows_set_aside_200_units_out(oracle, mis):
    """at (200, 200, 200) an ulp of a coordinate is 15 PT_EPS and the triangle test leaks by itself (test_alpha_host names those rays):
    a row is set aside when it holds a disagreeing ray, found by tapping one row at a time; at most a quarter of the rows"""
    aside, rays = A.far_rows_aside(oracle, mis)
    print("200 units out, do_mis %d: %d of %d rows set aside (%s), %d disagreeing rays" % (mis, aside.sum(), len(aside), np.flatnonzero(aside).tolist(), rays))
    assert aside.mean() <= ROWS_ASIDE_CAP


def test_where_a_collapsed_triangle_sits_does_not_matter(oracle):
    cut, cutoff, _ = A.case_scene("checker2")
    cam = A.case_camera(A.FAR["size"])
    at_v0, hole = A.ghost(cut, cutoff)
    at_v1, hole1 = A.ghost(cut, cutoff, at="v1")
    assert np.array_equal(hole, hole1) and not np.array_equal(at_v0.tris["v0"][hole], at_v1.tris["v0"][hole])
    for k in ("nodes", "mats", "lights", "atlas"):
        assert getattr(at_v0, k) is getattr(cut, k)
    assert np.array_equal(at_v0.tris[~hole], cut.tris[~hole])
    for k in ("v1", "v2"):
        assert np.array_equal(at_v0.tris[k][hole], at_v0.tris["v0"][hole])
    opaque, _ = oracle.render(cut, cam, A.FAR["frames"])
    a, sa = oracle.render(at_v0, cam, A.FAR["frames"])
    b, sb = oracle.render(at_v1, cam, A.FAR["frames"])
    assert not np.array_equal(a.view(np.uint32), opaque.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (sa.segments, sa.shadow_rays) == (sb.segments, sb.shadow_rays)
