"""Alpha cutouts per sample (csrc/alpha.hip inside the bounce loop): a render under a cutoff table is, float for float, the
oracle's render of the GHOST scene - the same triangles, nodes, materials and lights with every hole triangle collapsed to a point, and
no table (alpha_ref.ghost). tests/test_alpha_replay_host.py is the licence for the `==`: on the CPU, the model's loops replayed on every
ray of the oracle's ghost render disagree with it on no ray, in any case run here. What this pins and the probes cannot (they run the
resolve kernels without a queue): queue[i] / queue[slot] / sq[i] / S.SO[rec] / the path of a shadow record, the write of hits[slot] from
a later round into a queue repacked after roulette, the rotation of the control words over eight bounces, and the order of the additions
to L[path].

Per case (alpha_ref.per_sample_cases, shared with the host test): output, moments, first-hit planes and every counter against the ghost
scene's; the hole counters against the replay. ptmi_alpha_status.shadow_passes counts the holes passed by the shadow rays the device
traces, which are the reference's shadow rays but for the samples `shade` counts without tracing (contribution zero: the light on the far
side of the surface, ndl = 0), so: shadow_traced == the tap's shadow rays on the lit side of their surface (== the census's records), and
shadow_passes == the holes THOSE pass (replay.shadow_passes_lit); it equals replay.shadow_passes only where no far-side sample passes
a hole (the one-fence scene), and is smaller on the two-fence scene.

A failure names the first differing pixel, the frame (from one-frame dispatches) and prints Oracle.trace_path's log."""
import numpy as np
import pytest

import adaptive_ref
import alpha_ref as A
import aov_ref
import gauntlet_scenes as G
from ptmi import native
from test_gpu_alpha import at, prepare
from test_gpu_parity import assert_same_floats, bits

pytestmark = pytest.mark.gpu

CASES = A.per_sample_cases(G.repack_bounce())
SCENES = ("stripes", "checker2")
PLANES = ("albedo", "normal", "id")
ROWS_ASIDE_CAP = 0.25
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the table, planes and options it sets never reach the session's shared context"""
    with native.Context(0) as c:
        yield c


def case_id(c):
    return "b%d-mis%d-leaves%d-trav%d-overlap%d-fpb%d-%s-%s%s" % (
        c["max_bounces"], c["do_mis"], c["leaves"], c["traversal"], c["overlap"], c["frames_per_batch"],
        "planes" if c["planes"] else "plain", "fencelayers" if c["fence_layers"] else "layers4", "-rows" if c["tile"] else "")


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def scene_set(name):
    """(cutout scene, cutoff, number of fences, ghost, hole mask)"""
    def make():
        cut, cutoff, n = A.case_scene(name)
        return (cut, cutoff, n) + A.ghost(cut, cutoff)
    return cached(("scene", name), make)


def rows_of(cam, rows):
    return slice(rows[0], rows[1] or int(cam["height"]))


def reference(oracle, key, ghost, cam, rows, frames, mb, mis):
    """the oracle's side of one render of a ghost scene, computed once and shared: image, statistics, what ptmi_stats must say"""
    def make():
        out, st, census = oracle.render_census(ghost, cam, frames, max_bounces=mb, do_mis=mis, y0=rows[0], y1=rows[1])
        out.setflags(write=False)
        return dict(out=out, stats=st, figures=G.gpu_figures(census, mb))
    return cached(("ref", key, rows, frames, mb, mis), make)


def moments_reference(oracle, key, ghost, cam, rows, frames, mb, mis):
    """the moments plane folded from the oracle's per-path radiance, as tests/adaptive_ref.py folds it"""
    def make():
        W, H = int(cam["width"]), int(cam["height"])
        ys, xs = np.mgrid[rows_of(cam, rows), 0:W]
        xs, ys = xs.ravel(), ys.ravel()
        rgb, mom = np.zeros((len(xs), 3), np.float32), np.zeros((len(xs), 4), np.float32)
        for f in range(frames):
            rad, _ = oracle.trace_paths(ghost, cam, xs, ys, np.full(len(xs), f), max_bounces=mb, do_mis=mis)
            rgb, mom = adaptive_ref.fold_listed(rgb, mom, rad, np.full(len(xs), f, np.uint32))
        plane = np.zeros((H, W, 4), np.float32)
        plane[ys, xs] = mom
        return plane
    return cached(("moments", key, rows, frames, mb, mis), make)


def planes_reference(oracle, key, ghost, cam, rows, frames):
    """the first-hit planes tests/aov_ref.py gives for the rendered rows of the ghost scene, folded over the frames"""
    def make():
        ys = np.arange(int(cam["height"]))[rows_of(cam, rows)]
        per = [aov_ref.samples(oracle, ghost, cam, f, rows=ys) for f in range(frames)]
        return aov_ref.fold(per, list(range(frames))) + (np.any([s["normal_mapped"] for s in per], axis=0),)
    return cached(("planes", key, rows, frames), make)


def render(c, cam, frames):
    c.reset_stats()
    c.write_output(np.zeros((c.height, c.width, 4), np.float32))
    c.dispatch(at(cam, 0), frames)
    r = dict(output=c.read_output(), stats=c.stats(), alpha=c.alpha_status().as_dict())
    if c.moments():
        r["moments"] = c.read_moments()
    for a in c.aovs():
        r[a] = c.read_aov(a)
    return r


def options_of(case, rows):
    return dict(max_bounces=case["max_bounces"], do_mis=case["do_mis"], leaves=case["leaves"], traversal=case["traversal"],
                overlap=case["overlap"], frames_per_batch=case["frames_per_batch"], tile_y0=rows[0], tile_y1=rows[1])


def explain(c, oracle, ghost, cam, frames, got, want, mb, mis, what, keep=None):
    """the first differing pixel, the frame (one-frame dispatches onto a zeroed output: min(sample, 2.5) / (frame + 1), one float32
    product, against Oracle.trace_path folded the same way) and the oracle's log of that path"""
    bad = (bits(got) != bits(want)).any(axis=-1)
    if keep is not None:
        bad &= keep[:, None]
    y, x = (int(v) for v in np.argwhere(bad)[0])
    lines = ["%s: %d pixels differ; first at (x %d, y %d): gpu %s oracle %s" % (what, bad.sum(), x, y, got[y, x], want[y, x])]
    for f in range(frames):
        c.write_output(np.zeros((c.height, c.width, 4), np.float32))
        c.dispatch(at(cam, f), 1)
        one = c.read_output()[y, x, :3]
        rad, log = oracle.trace_path(ghost, cam, x, y, f, max_bounces=mb, do_mis=mis)
        fold = np.minimum(rad, np.float32(2.5)) * (np.float32(1.0) / np.float32(f + 1))
        if not np.array_equal(bits(one), bits(fold)):
            lines.append("frame %d: gpu sample %s oracle %s; the oracle's path (o, d, throughput, radiance, rng, t, tri, alive):" % (f, one, fold))
            lines += ["   " + " ".join("%.9g" % v for v in rec[:12]) + " rng %08x t %.9g tri %d alive %d"
                      % (rec[12:13].view(np.uint32)[0], rec[13], rec[14:15].view(np.uint32)[0], rec[15]) for rec in log]
            break
    else:
        lines.append("every one-frame dispatch of that pixel agrees with the oracle: the frames differ only when folded together")
    return "\n".join(lines)


def same_image(c, oracle, ghost, cam, frames, got, want, mb, mis, what, keep=None):
    g, w = (got, want) if keep is None else (got[keep], want[keep])
    if not np.array_equal(bits(g), bits(w)):
        raise AssertionError(explain(c, oracle, ghost, cam, frames, got, want, mb, mis, what, keep))
    assert_same_floats(g, w, what)


def check_planes(r, ref, rows, what):
    """the bars of tests/test_gpu_aov.py::test_many_frames_fold on the rendered rows, zeros outside them; ids exact (the numbering is
    the cutout scene's)"""
    ra, rn, rid, exact, mapped = ref
    outside = np.ones(r["id"].shape[0], bool)
    outside[rows] = False
    for k in PLANES:
        assert not r[k][outside].any(), what + ": " + k + " written outside the rows"
    a, n = r["albedo"][rows].reshape(-1, 4), r["normal"][rows].reshape(-1, 4)
    assert exact.mean() > 0.9 and not mapped.any()
    assert np.array_equal(r["id"][rows].reshape(-1, 2), rid), what + ": ID is not the last frame's first hit in the ghost scene"
    assert np.abs(a[exact] - ra[exact]).max() < 1e-6, what
    t_err = np.abs(n[:, 3] - rn[:, 3]) / np.maximum(np.abs(rn[:, 3]), 1e-30)
    assert t_err[exact & (rn[:, 3] != 0)].max() < 1e-6 and (n[rn[:, 3] == 0, 3] == 0).all(), what
    assert np.abs(n[exact, :3] - rn[exact, :3]).max() < 1e-5, what


def check_counters(r, ref, rp, what):
    st, ost, want = r["stats"], ref["stats"], ref["figures"]
    print(what, "segments", st.segments, "shadow rays", st.shadow_rays, "traced", st.shadow_traced, "of the tap's", rp.n_shadow, "|", r["alpha"],
          "| replay: path passes", rp.path_passes, "shadow passes", rp.shadow_passes, "on the lit side", rp.shadow_passes_lit)
    assert (st.paths, st.segments, st.shadow_rays) == (ost.paths, ost.segments, ost.shadow_rays), what
    nb = len(want["segments_by_bounce"])
    by_bounce = [int(v) for v in st.segments_by_bounce]
    assert by_bounce[:nb] == want["segments_by_bounce"] and not any(by_bounce[nb:]), what
    assert (rp.n_closest, rp.n_shadow) == (ost.segments, ost.shadow_rays) and rp.shadow_grazing == 0, what
    assert st.shadow_traced == want["shadow_traced"] == rp.shadow_lit, what
    assert r["alpha"]["path_exhausted"] == 0 and r["alpha"]["shadow_exhausted"] == 0, what
    assert r["alpha"]["path_passes"] == rp.path_passes > 0, what
    assert r["alpha"]["shadow_passes"] == rp.shadow_passes_lit, what


# ---- 1. every case of the table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("name", SCENES)
def test_a_render_under_the_table_is_the_ghost_scenes(ctx, oracle, name, case):
    cut, cutoff, n_fences, ghost, hole = scene_set(name)
    cam, rows = A.case_view(case)
    W, H = int(cam["width"]), int(cam["height"])
    mb, mis = case["max_bounces"], case["do_mis"]
    layers = n_fences if case["fence_layers"] else 0
    if case["tile"]:
        assert ((rows[1] - rows[0]) * W) % 64 != 0 and ((rows[1] - rows[0]) * W * A.FRAMES) % 64 != 0
    what = "%s %s" % (name, case_id(case))
    ref = reference(oracle, name, ghost, cam, rows, A.FRAMES, mb, mis)
    rp = cached(("replay", name, rows, mb, mis, layers),
                lambda: A.replay(oracle, cut, cutoff, ghost, cam, A.FRAMES, rows, mb, mis, layers or A.DEFAULT_LAYERS))
    assert (rp.disagreeing_closest, rp.disagreeing_shadow, rp.exhausted) == (0, 0, 0)
    aovs = PLANES if case["planes"] else ()
    try:
        prepare(ctx, cut, W, H, aovs=aovs, moments=case["planes"], **options_of(case, rows))
        ctx.set_alpha_cutoff(cutoff, max_layers=layers)
        r = render(ctx, cam, A.FRAMES)
        assert ctx.options().overlap == case["overlap"]                     # the stored option is left alone
        assert r["alpha"]["max_layers"] == (layers or A.DEFAULT_LAYERS) and r["alpha"]["n_cutout"] == n_fences
        same_image(ctx, oracle, ghost, cam, A.FRAMES, r["output"], ref["out"], mb, mis, what)
        check_counters(r, ref, rp, what)
        if case["planes"]:
            assert_same_floats(r["moments"], moments_reference(oracle, name, ghost, cam, rows, A.FRAMES, mb, mis), what + ": moments")
            check_planes(r, planes_reference(oracle, name, ghost, cam, rows, A.FRAMES), rows_of(cam, rows), what)
        # the ghost on the device: the cutout scene without a table, its hole triangles collapsed through ptmi_update_triangles
        prepare(ctx, cut, W, H, **options_of(case, rows))
        ctx.update_triangles(0, ghost.tris)
        assert ctx.alpha_status().present == 0
        g = render(ctx, cam, A.FRAMES)
        same_image(ctx, oracle, ghost, cam, A.FRAMES, g["output"], ref["out"], mb, mis, what + ", the ghost made on the device")
        assert (g["stats"].segments, g["stats"].shadow_rays, g["stats"].shadow_traced) == \
               (r["stats"].segments, r["stats"].shadow_rays, r["stats"].shadow_traced)
        assert g["alpha"]["path_passes"] == 0 and g["alpha"]["shadow_passes"] == 0
    finally:
        ctx.set_aovs()
        ctx.set_moments(False)
        ctx.set_alpha_cutoff(None)


# ---- 2. a triangle edit under the table --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [1, 2])
def test_a_triangle_edit_leaves_the_table_in_place(ctx, oracle, leaves):
    """include/ptmi.h: the ptmi_update_* calls leave the table alone. The fence is moved, tilted and mirrored in u under the table; the
    render is the oracle's of the edited scene's ghost (other cells are holes now), nodes refitted as tests/test_gpu_scene_update.py's
    edited() refits them"""
    cut, cutoff, n_fences, _, hole = scene_set("stripes")
    moved, edited = cached("edited", lambda: A.edited_fence(cut))
    ghost, edited_hole = cached("edited ghost", lambda: A.ghost(edited, cutoff))
    assert not np.array_equal(hole, edited_hole)
    cam, rows = A.case_camera(), (0, 0)
    W, H = A.SIZE
    what = "edited stripes, leaves %d" % leaves
    ref = reference(oracle, "edited", ghost, cam, rows, A.FRAMES, 8, 1)
    rp = cached(("replay", "edited"), lambda: A.replay(oracle, edited, cutoff, ghost, cam, A.FRAMES, rows, 8, 1))
    assert (rp.disagreeing_closest, rp.disagreeing_shadow, rp.exhausted) == (0, 0, 0)
    try:
        prepare(ctx, cut, W, H, leaves=leaves)
        ctx.set_alpha_cutoff(cutoff, max_layers=3)
        before = render(ctx, cam, A.FRAMES)
        ctx.update_triangles(0, moved)
        st = ctx.alpha_status().as_dict()
        assert (st["present"], st["n_materials"], st["n_cutout"], st["max_layers"]) == (1, len(cut.mats), n_fences, 3)
        r = render(ctx, cam, A.FRAMES)
        assert not np.array_equal(bits(r["output"]), bits(before["output"]))
        same_image(ctx, oracle, ghost, cam, A.FRAMES, r["output"], ref["out"], 8, 1, what)
        check_counters(r, ref, rp, what)
    finally:
        ctx.set_alpha_cutoff(None)


# ---- 3. 200 units out --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", [0, 1])
def test_far_from_the_origin_outside_the_rows_set_aside(ctx, oracle, mis):
    """at (200, 200, 200) the triangle test leaks by itself: the rows in which the CPU replay finds a disagreeing ray are set aside (at
    most a quarter, the host test's condition); every float of every other row is the ghost scene's"""
    cut, cutoff, ghost, cam = A.far_scene()
    aside, n_bad = A.far_rows_aside(oracle, mis)
    W, H = A.FAR["size"]
    print("200 units out, do_mis %d: %d of %d rows set aside (%.1f %%), %d disagreeing rays" % (mis, aside.sum(), H, 100 * aside.mean(), n_bad))
    assert aside.mean() <= ROWS_ASIDE_CAP
    ref = reference(oracle, "far", ghost, cam, (0, 0), A.FAR["frames"], 8, mis)
    try:
        prepare(ctx, cut, W, H, do_mis=mis)
        ctx.set_alpha_cutoff(cutoff)
        r = render(ctx, cam, A.FAR["frames"])
        assert r["alpha"]["path_passes"] > 0 and r["alpha"]["path_exhausted"] == 0 and r["alpha"]["shadow_exhausted"] == 0
        same_image(ctx, oracle, ghost, cam, A.FAR["frames"], r["output"], ref["out"], 8, mis, "200 units out, do_mis %d" % mis, keep=~aside)
        differ = (bits(r["output"]) != bits(ref["out"])).any(axis=-1)
        print("   pixels that differ in the rows set aside:", int(differ.sum()))
    finally:
        ctx.set_alpha_cutoff(None)
