"""`shade`'s ENV and MED instantiations against the oracle's extras (oracle/pt_oracle.h pto_extras), per sample: the fog / sky gauntlet
(tests/gauntlet_scenes.py gauntlet_fog; tests/test_oracle_extras_host.py proves on the CPU which branches its renders reach and
measures what may differ) rendered with the sky looked up, the sky sampled, the fog alone, and both.

  * ENV alone: the sky lookup never changes a path's geometry, so paths, segments, shadow rays and segments by bounce equal the
    oracle's and the radiance is the oracle's bit for bit, but on the pixels one of whose paths looked the sky up within
    env_ref.BORDER_BAND of a texel border (atan2f / acosf are outside the arithmetic contract); shadow_traced within that many paths.
  * MED alone, ENV + MED: logf / expf move the scatter point by ulps. Outside the pixels where a path of the oracle's own -2 .. 2 ulp
    variants takes another branch (G.nudge_study), the image is within medium_ref.TOL_SHADE of the reference but for 0.2 % of pixels; paths equal, segments and
    shadow rays within 1e-3; the first-hit planes are those without a medium, bit for bit.
  * the same per path, on (x, y, frame) triples from one-frame dispatches: a failure names the path, and Oracle.trace_path_ext's log
    explains it.
Options: both sides of `shade`'s emit_records, both traversal picks, bounce limits around the repack, the bounce-0 instantiation
with planes, one frame and many per batch, a row range that ends the bounce-0 queue in a partial wave (G.fog_gpu_cases)."""
import numpy as np
import pytest

import env_ref
import gauntlet_scenes as G
import medium_ref
from ptmi import native
from test_golden import same
from test_gpu_environment import at
from test_gpu_parity import assert_same_floats

pytestmark = pytest.mark.gpu

ASIDE_CAP, OUTSIDE_CAP, COUNTER_RTOL = 0.01, 0.002, 1e-3
OPTIONS = ("max_bounces", "do_mis", "tile_y0", "tile_y1", "tile_parts", "frames_per_batch", "cull", "traversal", "overlap", "perf_mode")
PLANES = ("albedo", "normal", "id")
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the session's stays without a map and without a medium"""
    with native.Context(0) as c:
        yield c


def scene():
    if "scene" not in _cache:
        _cache["scene"] = G.gauntlet_fog()
    return _cache["scene"]


def reference(oracle, state, max_bounces, tile):
    """the oracle's side of one render, computed once and shared: G.nudge_study for a state with fog, else the plain reference"""
    key = (state, max_bounces, tile)
    if key not in _cache:
        if G.FOG_STATES[state]["fog"]:
            _cache[key] = G.nudge_study(oracle, scene(), state, native.env_table, max_bounces, tile)
        else:
            out, st, border, cen = G.render_fog(oracle, scene(), state, native.env_table, max_bounces, tile)
            out.setflags(write=False)
            _cache[key] = dict(ref=out, stats=st, border=border, census=cen)
    return _cache[key]


def put_in_place(c, state):
    s = G.FOG_STATES[state]
    if s["sky"]:
        c.upload_environment(G.fog_sky(), intensity=G.FOG_SKY_INTENSITY, rotation=G.FOG_SKY_ROTATION, sample=int(s["sky"] == "lookup"))
        assert c.environment_status().sampled == int(s["sky"] == "sampled")
    if s["fog"]:
        c.set_medium(**s["fog"])


def render(c, state, case, fog=True, frames=None, cam=None):
    """(image, stats, planes) of one case on the GPU; fog = False leaves the medium out (for the planes)"""
    if case["tile"]:
        W, H, (y0, y1) = G.TILE_CASE["width"], G.TILE_CASE["height"], G.TILE_CASE["rows"]
        assert ((y1 - y0) * W) % 64 != 0
    else:
        (W, H), (y0, y1) = G.SIZE, (0, 0)
    c.upload_scene(scene())
    c.resize(W, H)
    c.set_aovs(*(PLANES if case["planes"] else ()))
    c.set_moments(bool(case["planes"]))
    c.set_options(max_bounces=case["max_bounces"], do_mis=1, tile_y0=y0, tile_y1=y1, tile_parts=0, frames_per_batch=case["frames_per_batch"],
                  cull=1, traversal=case["traversal"], overlap=case["overlap"], perf_mode=0)
    try:
        put_in_place(c, state)
        if not fog:
            c.set_medium(None)
        c.write_output(np.zeros((H, W, 4), np.float32))
        c.reset_stats()
        c.dispatch(G.fog_camera(state, W, H) if cam is None else cam, G.FOG_FRAMES if frames is None else frames)
        out, st = c.read_output(), c.stats()
        planes = {a: c.read_aov(a) for a in PLANES} if case["planes"] else {}
    finally:
        c.set_medium(None)
        c.upload_environment(None)
        c.set_aovs()
        c.set_moments(False)
    return out, st, planes


def case_id(c):
    return "b%d-overlap%d-trav%d-%s-fpb%d%s" % (c["max_bounces"], c["overlap"], c["traversal"], "planes" if c["planes"] else "plain",
                                                 c["frames_per_batch"], "-rows" if c["tile"] else "")


# ---- a) the sky alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.fog_gpu_cases(), ids=case_id)
@pytest.mark.parametrize("state", ["sky_lookup", "sky_sampled"])
def test_sky_alone_is_the_oracle_bit_for_bit(ctx, oracle, state, case):
    r = reference(oracle, state, case["max_bounces"], case["tile"])
    ost, want = r["stats"], G.gpu_figures_ext(r["census"], case["max_bounces"])
    got, st, _ = render(ctx, state, case)
    rows = G.rendered_rows(case["tile"])
    aside = r["border"] < env_ref.BORDER_BAND
    # the paths behind the set-aside pixels: at most FOG_FRAMES each
    aside_paths = int(aside[rows].sum()) * G.FOG_FRAMES
    by_bounce = [int(v) for v in st.segments_by_bounce]
    print(state, case_id(case), "segments", st.segments, ost.segments, "shadow_rays", st.shadow_rays, ost.shadow_rays, "shadow_traced",
          st.shadow_traced, want["shadow_traced"], "set aside %.3f %% of pixels" % (100 * aside[rows].mean()))
    assert aside[rows].mean() <= ASIDE_CAP
    assert (st.paths, st.segments, st.shadow_rays) == (ost.paths, ost.segments, ost.shadow_rays)
    assert st.shadow_rays == want["shadow_rays"]
    nb = min(case["max_bounces"], 64)
    assert by_bounce[:nb] == want["segments_by_bounce"] and not any(by_bounce[nb:])
    assert abs(st.shadow_traced - want["shadow_traced"]) <= aside_paths
    assert_same_floats(got[~aside], r["ref"][~aside], f"radiance {state} {case_id(case)}")
    differ = (got.view(np.uint32) != r["ref"].view(np.uint32)).any(axis=-1)
    print("   pixels that differ inside the band:", int(differ.sum()), "of", int(aside.sum()))


# ---- b), c) the fog alone, and with the sky sampled ---------------------------------------------------------------------------------
def compare_within_tolerance(got, r, rows, what):
    """the GPU image against the reference outside the pixels set aside; prints what it measured"""
    aside = r["flips"]
    assert np.isfinite(got[..., :3]).all()
    dev = G.pixel_deviation(got, r["ref"])
    keep = ~aside[rows]
    outside = dev[rows][keep] > medium_ref.TOL_SHADE
    within = dev[rows][keep][~outside]
    print(what, "largest deviation within tolerance %.3g (limit %.3g, the oracle's own drift %.3g); %.3f %% of pixels set aside; %.3f %% outside (largest %.3g)"
          % (within.max() if within.size else 0.0, medium_ref.TOL_SHADE, r["drift"], 100 * aside[rows].mean(), 100 * outside.mean(),
             dev[rows][keep].max()))
    assert aside[rows].mean() <= ASIDE_CAP, what
    assert outside.mean() <= OUTSIDE_CAP, what
    assert not got[..., 3].any()


@pytest.mark.parametrize("case", G.fog_gpu_cases(), ids=case_id)
@pytest.mark.parametrize("state", ["fog", "fog_sky_sampled"])
def test_fog_is_the_oracle_within_the_measured_tolerance(ctx, oracle, state, case):
    r = reference(oracle, state, case["max_bounces"], case["tile"])
    ost = r["stats"]
    got, st, planes = render(ctx, state, case)
    rows = G.rendered_rows(case["tile"])
    print(state, case_id(case), "segments", st.segments, ost.segments, "shadow_rays", st.shadow_rays, ost.shadow_rays)
    assert st.paths == ost.paths
    assert abs(st.segments / ost.segments - 1) < COUNTER_RTOL and abs(st.shadow_rays / max(ost.shadow_rays, 1) - 1) < COUNTER_RTOL
    assert st.segments_by_bounce[0] == ost.paths            # every path traces its camera ray, scatter or not
    compare_within_tolerance(got, r, rows, f"{state} {case_id(case)}:")
    if case["planes"]:                                      # the planes record the camera ray's surface hit, fog or not
        _, _, clear = render(ctx, state, case, fog=False)
        for a in PLANES:
            assert same(planes[a], clear[a]), a
        assert (clear["id"][rows] != 0xFFFFFFFF).any() and (clear["id"][rows] == 0xFFFFFFFF).any()


# ---- d) per path ------------------------------------------------------------------------------------------------------------------------
N_PER_FRAME = 250
PATH_CASE = dict(max_bounces=8, overlap=2, traversal=0, planes=False, frames_per_batch=0, tile=False)


@pytest.mark.parametrize("state", G.FOG_GPU_STATES)
def test_single_samples_are_the_oracles_paths(ctx, oracle, state):
    """8 x 250 (x, y, frame) triples: the GPU's sample from a one-frame dispatch at that frame index onto a zeroed output, which
    is mix(0, min(sample, 2.5), 1 / (frame + 1)) = one float32 product; the oracle's from trace_paths_ext, folded the same way"""
    W, H = G.SIZE
    rng = np.random.default_rng(41)
    cam = G.fog_camera(state)
    env, fog = G.fog_env(state, native.env_table), G.FOG_STATES[state]["fog"]
    xs, ys, fr, got = [], [], [], []
    for f in range(G.FRAMES):
        out, _, _ = render(ctx, state, PATH_CASE, frames=1, cam=at(cam, f))
        pick = rng.choice(W * H, N_PER_FRAME, replace=False)
        y, x = np.divmod(pick, W)
        xs.append(x); ys.append(y); fr.append(np.full(N_PER_FRAME, f)); got.append(out[y, x, :3])
    xs, ys, fr, got = (np.concatenate(a) for a in (xs, ys, fr, got))
    fold = lambda rad: np.minimum(rad, np.float32(2.5)) * (np.float32(1.0) / (fr + 1).astype(np.float32))[:, None]
    rad, seg, border = oracle.trace_paths_ext(scene(), cam, xs, ys, fr, oracle.extras(env, fog), max_bounces=8)
    want = fold(rad)
    assert np.isfinite(want).all()
    aside = border < env_ref.BORDER_BAND
    name = lambda i: "path (x %d, y %d, frame %d): gpu %s oracle %s, %d segments" % (xs[i], ys[i], fr[i], got[i], want[i], seg[i])
    if not fog:
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1) & ~aside)
        print(state, "%d paths, %.3f %% set aside, %d differ" % (len(xs), 100 * aside.mean(), len(bad)))
        assert aside.mean() <= ASIDE_CAP
        assert not len(bad), name(bad[0])
        return
    scale = (fr + 1)[:, None] / np.maximum(np.abs(want.astype(np.float64)) * (fr + 1)[:, None], 1.0)     # to the sample's own scale
    deviation = lambda a: (np.abs(a.astype(np.float64) - want) * scale).max(axis=1)
    branches = oracle.last_branches
    flips = np.zeros(len(xs), bool)
    drift = 0.0
    for k in G.NUDGES:                                       # the paths that take another branch under a 1 - 2 ulp library, on the oracle
        d = deviation(fold(oracle.trace_paths_ext(scene(), cam, xs, ys, fr, oracle.extras(env, fog, k), max_bounces=8)[0]))
        now = oracle.last_branches != branches
        flips |= now
        drift = max(drift, float(d[~now].max()))
    aside |= flips
    dev = deviation(got)
    outside = np.flatnonzero((dev > medium_ref.TOL_SHADE) & ~aside)
    print(state, "%d paths: largest deviation %.3g (limit %.3g, the oracle's own drift %.3g); %.3f %% set aside; %.3f %% outside"
          % (len(xs), dev[~aside].max(), medium_ref.TOL_SHADE, drift, 100 * aside.mean(), 100 * len(outside) / (~aside).sum()))
    for i in outside[:5]:
        print("   outside:", name(i), "deviation %.3g" % dev[i])
    assert aside.mean() <= ASIDE_CAP
    assert len(outside) <= OUTSIDE_CAP * (~aside).sum(), name(outside[0])
