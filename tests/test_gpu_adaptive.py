"""Adaptive sampling on the GPU (include/ptmi.h ptmi_dispatch_adaptive) against tests/adaptive_ref.py, bit for bit: radiance and the
moments plane (hence the counts) against the model fed the oracle's per-path radiance; the first-hit planes against what a plain
dispatch of count[pixel] frames leaves at each pixel (tests/aov_ref.py restates the normals in float64, so the bit-exact reference
for a plane folded per pixel in frame order is the plain dispatch; that reference is this code base itself, but k_fold_aov<DensePixels> and
k_fold_aov<ListedPixels> are one body (fold_aov in csrc/pipeline.hip) over two pixel sources: what tests/test_gpu_aov.py pins for the plain
fold against tests/aov_ref.py holds for both walks, and this test pins the listed source). Also the counters, the batch and
round splits, bands and strips, the life cycle and errors, and the Node binding."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref
from ptmi import layout, native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the planes and options it sets never reach the session's shared context"""
    c = native.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def setup(ctx, sc, W, H, aovs=(), moments=True, **opt):
    o = dict(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=0,
             overlap=2, perf_mode=0, leaves=0, timing=0)
    o.update(opt)
    ctx.set_aovs()
    ctx.set_moments(False)
    ctx.set_options(**o)
    ctx.upload_scene(sc)
    ctx.resize(W, H)
    ctx.set_aovs(*aovs)
    ctx.set_moments(moments)
    ctx.reset_stats()


def at(cam, frame):
    c = cam.copy()
    c["frame_index"] = frame
    return c


def err(fn, *a, **kw):
    with pytest.raises(native.PtmiError) as e:
        fn(*a, **kw)
    return e.value.code


# step 4 from 4 frames on: the counts of a 6-round run spread over 4 .. 24. The threshold is chosen so that the model ends between
# 10 % and 90 % converged on all three scenes (asserted on the model below).
P = dict(threshold=0.35, floor=0.05, min_frames=4, max_frames=64, step=4, neighbourhood=1)
ROUNDS = 6


def converged_share(st, p, rows=None):
    act = adaptive_ref.select(st.moments, p, rows)
    inside = adaptive_ref.rows_mask(st.image.shape[0], rows)
    return 1.0 - act[inside].mean()


def check_partly_converged(st, p, rows=None):
    share = converged_share(st, p, rows)
    print("converged share", share, "active per round", st.active)
    assert 0.10 <= share <= 0.90, share
    assert st.active[-1] < st.active[0]                     # the list shrank


@pytest.mark.parametrize("name,leaves,overlap,dof", [("cornell", 2, 2, False), ("cornell", 1, 0, False), ("cornell_spheres", 2, 1, True),
                                                     ("feature_box", 1, 1, False), ("feature_box", 2, 0, False)])
def test_matches_the_model(ctx, oracle, scene_factory, name, leaves, overlap, dof):
    sc = scene_factory(name)
    W, H = 24, 20
    cam = layout.make_camera(W, H, aperture=0.05, focus_distance=2.5) if dof else layout.make_camera(W, H)
    want = adaptive_ref.run(oracle, sc, cam, P, ROUNDS)
    check_partly_converged(want, P)
    setup(ctx, sc, W, H, aovs=("albedo", "normal", "id"), leaves=leaves, overlap=overlap)
    ctx.dispatch_adaptive(at(cam, 0), ROUNDS, **P)
    got, mom = ctx.read_output(), ctx.read_moments()
    planes = {k: ctx.read_aov(k) for k in ("albedo", "normal", "id")}
    st, ast = ctx.stats(), ctx.adaptive_status()
    assert same(mom, want.moments)
    assert same(got, want.image)
    # the list compaction did not leak into the counters
    assert st.segments == want.segments and st.paths == want.paths and st.dispatches == 1 and st.frames == 0
    assert ast.as_dict() == adaptive_ref.status(want)
    # first-hit planes: per pixel what a plain dispatch of count[pixel] frames holds
    counts = want.counts
    by_n = {k: {} for k in planes}
    for n in sorted(set(counts.ravel().tolist())):
        ctx.dispatch(at(cam, 0), n)
        for k in planes:
            by_n[k][n] = ctx.read_aov(k)
    for k in ("albedo", "normal"):
        assert same(planes[k], adaptive_ref.planes_at_counts(counts, by_n[k])), k
    assert np.array_equal(planes["id"], adaptive_ref.planes_at_counts(counts, by_n["id"]))


def test_nothing_converges_equals_plain_dispatch(ctx, scene_factory):
    sc = scene_factory("cornell")
    W, H = 32, 32
    cam = layout.make_camera(W, H)
    # a pixel whose first frames are all black has variance 0 and meets any threshold: min_frames keeps those in the list too
    p = dict(P, threshold=1e-9, neighbourhood=0, min_frames=ROUNDS * P["step"])
    setup(ctx, sc, W, H, aovs=("albedo", "normal", "id"))
    ctx.dispatch(at(cam, 0), ROUNDS * p["step"])
    want = ctx.read_output(), ctx.read_moments(), ctx.read_aov("albedo"), ctx.read_aov("normal"), ctx.read_aov("id")
    seg = ctx.stats().segments
    ctx.reset_stats()
    ctx.dispatch_adaptive(at(cam, 0), ROUNDS, **p)
    got = ctx.read_output(), ctx.read_moments(), ctx.read_aov("albedo"), ctx.read_aov("normal"), ctx.read_aov("id")
    for g, w in zip(got[:4], want[:4]):
        assert same(g, w)
    assert np.array_equal(got[4], want[4])
    st = ctx.stats()
    assert st.segments == seg and st.paths == W * H * ROUNDS * p["step"]


def test_independent_of_batches_and_round_splits(ctx, scene_factory):
    sc = scene_factory("cornell_spheres")
    W, H = 32, 24
    cam = layout.make_camera(W, H)
    outs = []
    for fpb, split in ((0, False), (1, False), (3, False), (0, True)):
        setup(ctx, sc, W, H, frames_per_batch=fpb)
        if split:
            for r in range(ROUNDS):
                ctx.dispatch_adaptive(at(cam, 0 if r == 0 else 7), 1, **P)
        else:
            ctx.dispatch_adaptive(at(cam, 0), ROUNDS, **P)
        outs.append((ctx.read_output(), ctx.read_moments(), ctx.stats().segments, ctx.adaptive_status().as_dict()))
    c = outs[0][1][..., 2]
    assert c.min() < c.max()                                # some pixels stopped early
    for o in outs[1:]:
        assert same(o[0], outs[0][0]) and same(o[1], outs[0][1]) and o[2] == outs[0][2] and o[3] == outs[0][3]


def test_uniform_frames_then_adaptive_rounds(ctx, oracle, scene_factory):
    sc = scene_factory("cornell")
    W, H = 24, 20
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H)
    ctx.dispatch(at(cam, 0), 4)
    start = adaptive_ref.State(H, W, ctx.read_output(), ctx.read_moments())
    want = adaptive_ref.run(oracle, sc, cam, P, 4, state=start, restart=False)
    check_partly_converged(want, P)
    ctx.dispatch_adaptive(at(cam, 4), 4, **P)
    assert same(ctx.read_moments(), want.moments) and same(ctx.read_output(), want.image)
    # ... and frame_index 0 restarts: the same planes as a fresh run
    fresh = adaptive_ref.run(oracle, sc, cam, P, 3)
    ctx.dispatch_adaptive(at(cam, 0), 3, **P)
    assert same(ctx.read_moments(), fresh.moments) and same(ctx.read_output(), fresh.image)
    assert ctx.adaptive_status().rounds == 3


@pytest.mark.parametrize("tile", [dict(tile_y0=5, tile_y1=14), dict(tile_parts=3, tile_part=1, tile_strip=2),
                                  dict(tile_y0=2, tile_y1=19, tile_parts=2, tile_part=0, tile_strip=3)])
def test_bands_and_strips(ctx, oracle, scene_factory, tile):
    sc = scene_factory("cornell")
    W, H = 24, 20
    cam = layout.make_camera(W, H)
    rows = adaptive_ref.band_rows(H, tile.get("tile_y0", 0), tile.get("tile_y1", 0), tile.get("tile_parts", 1), tile.get("tile_part", 0),
                                  tile.get("tile_strip", 1))
    want = adaptive_ref.run(oracle, sc, cam, P, ROUNDS, rows=rows)
    check_partly_converged(want, P, rows)
    # the 3x3 rule stops at the band: with the whole image as the band, some pixel of these rows is chosen differently
    whole = adaptive_ref.run(oracle, sc, cam, P, ROUNDS)
    assert not np.array_equal(whole.counts[rows], want.counts[rows])
    setup(ctx, sc, W, H, aovs=("albedo", "normal", "id"), **tile)
    ctx.dispatch_adaptive(at(cam, 0), ROUNDS, **P)
    got, mom = ctx.read_output(), ctx.read_moments()
    assert same(mom, want.moments) and same(got, want.image)          # rows outside: zeros in both
    for k in ("albedo", "normal", "id"):
        assert not ctx.read_aov(k)[~rows].any(), k
        assert ctx.read_aov(k)[rows].any(), k
    assert ctx.adaptive_status().as_dict() == adaptive_ref.status(want, rows)
    st = ctx.stats()
    assert st.segments == want.segments and st.paths == want.paths


def test_plain_dispatch_keeps_its_bits(ctx):
    """radiance of a plain ptmi_dispatch against a stored fixture, with the feature compiled in and its buffers live"""
    from test_golden import load
    z, sc, cam = load(os.path.join(ROOT, "tests", "golden", "cornell_64x48_4spp_mis.npz"))
    W, H = int(cam["width"]), int(cam["height"])
    setup(ctx, sc, W, H, max_bounces=int(z["bounces"]), do_mis=int(z["mis"]))
    ctx.dispatch_adaptive(at(cam, 0), 2, **P)                       # the adaptive buffers exist
    ctx.reset_stats()
    ctx.dispatch(at(cam, 0), int(z["frames"]))
    assert same(ctx.read_output(), z["image"])
    assert ctx.stats().segments == int(z["segments"])


def write_moments(ctx, plane):
    """the caller's way to write the moments plane: a copy to ptmi_moments_device_ptr"""
    import ctypes
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    plane = np.ascontiguousarray(plane, np.float32)
    ctx.synchronize()
    assert hip.hipMemcpy(ctx.moments_device_ptr(), plane.ctypes.data, plane.nbytes, 1) == 0          # host to device


def same_or_both_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


@pytest.mark.parametrize("neighbourhood", [0, 1])
def test_nan_moments_end_at_max_frames(ctx, oracle, scene_factory, neighbourhood):
    """The folds clamp with fmin, so no render puts a NaN into the moments plane; a caller can, through ptmi_moments_device_ptr.
    Such a pixel stays listed until max_frames (NOT var <= bound, max(a, b) keeping a NaN first operand) - and with neighbourhood = 1
    so do its eight neighbours - while everything finite stops at min_frames under this threshold."""
    sc = scene_factory("cornell")
    W, H = 24, 20
    cam = layout.make_camera(W, H)
    p = dict(threshold=1e9, floor=0.05, min_frames=4, max_frames=20, step=4, neighbourhood=neighbourhood)
    setup(ctx, sc, W, H)
    ctx.dispatch(at(cam, 0), 4)
    mom = ctx.read_moments()
    assert np.isfinite(mom).all() and (mom[..., 2] == 4).all()
    poisoned = [(3, 4, (0,)), (9, 15, (1,)), (15, 8, (0, 1))]           # (y, x, which of m1 / m2)
    for y, x, ch in poisoned:
        for c in ch:
            mom[y, x, c] = np.nan
    write_moments(ctx, mom)
    assert same_or_both_nan(ctx.read_moments(), mom)
    want = adaptive_ref.State(H, W, ctx.read_output(), mom)
    listed = np.zeros((H, W), bool)
    for y, x, _ in poisoned:
        if neighbourhood:
            listed[y - 1:y + 2, x - 1:x + 2] = True
        else:
            listed[y, x] = True
    for r in range(6):
        before = want.counts.copy()
        adaptive_ref.run(oracle, sc, cam, p, 1, state=want, restart=False)
        ctx.dispatch_adaptive(at(cam, 4), 1, **p)
        assert want.active[-1] == (int(listed.sum()) if r < 4 else 0)            # four rounds take 4 to 20 = max_frames, not fewer
        assert ctx.adaptive_status().active == want.active[-1]
        assert np.array_equal(want.counts - before, np.where(listed & (r < 4), 4, 0))
        got = ctx.read_moments()
        assert same_or_both_nan(got, want.moments), r
        assert same(ctx.read_output(), want.image), r
    got = ctx.read_moments()
    assert (got[..., 2][listed] == 20).all() and (got[..., 2][~listed] == 4).all()
    for y, x, ch in poisoned:
        assert all(np.isnan(got[y, x, c]) for c in ch)


def test_life_cycle_and_errors(ctx, scene_factory):
    sc = scene_factory("cornell")
    W, H = 16, 12
    cam = layout.make_camera(W, H)
    fresh = native.Context(0)
    try:
        assert err(fresh.dispatch_adaptive, cam, 1, **P) == E_STATE                  # no scene
        fresh.upload_scene(sc)
        assert err(fresh.dispatch_adaptive, cam, 1, **P) == E_STATE                  # no size
        fresh.resize(W, H)
        assert err(fresh.dispatch_adaptive, cam, 1, **P) == E_STATE                  # no moments plane
        assert err(fresh.adaptive_status) == E_STATE
    finally:
        fresh.close()
    setup(ctx, sc, W, H)
    for bad in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(reserved=(0, 1)), dict(reserved=(2, 0)),
                dict(min_frames=9, max_frames=8), dict(max_frames=(1 << 24) + 1), dict(neighbourhood=2), dict(floor=-1.0)):
        assert err(ctx.dispatch_adaptive, cam, 1, **dict(P, **bad)) == E_INVALID, bad
    assert err(ctx.dispatch_adaptive, layout.make_camera(W + 1, H), 1, **P) == E_INVALID
    assert ctx.adaptive_status().as_dict() == dict(active=0, samples=0, min_count=0, max_count=0, rounds=0)
    ctx.dispatch_adaptive(at(cam, 0), 0, **P)                                        # no rounds: nothing
    assert ctx.stats().dispatches == 0 and not ctx.read_moments().any()
    ctx.dispatch_adaptive(at(cam, 0), 2, **P)
    a = ctx.read_output(), ctx.read_moments()
    assert ctx.adaptive_status().rounds == 2
    # set_moments(0) between dispatches: an error, then a fresh plane
    ctx.set_moments(False)
    assert err(ctx.dispatch_adaptive, at(cam, 0), 1, **P) == E_STATE
    ctx.set_moments(True)
    assert ctx.adaptive_status().as_dict() == dict(active=0, samples=0, min_count=0, max_count=0, rounds=0)      # a fresh plane
    ctx.dispatch_adaptive(at(cam, 0), 2, **P)
    assert same(ctx.read_output(), a[0]) and same(ctx.read_moments(), a[1])
    # resize between dispatches: planes at the new size, the round counter back to 0, then the same result again
    ctx.resize(W + 8, H + 4)
    assert ctx.adaptive_status().as_dict() == dict(active=0, samples=0, min_count=0, max_count=0, rounds=0)
    ctx.dispatch_adaptive(at(layout.make_camera(W + 8, H + 4), 0), 1, **P)
    assert ctx.adaptive_status().samples == (W + 8) * (H + 4) * P["step"]
    ctx.resize(W, H)
    ctx.dispatch_adaptive(at(cam, 0), 2, **P)
    assert same(ctx.read_output(), a[0]) and same(ctx.read_moments(), a[1])
    # defaults: zeros pick them
    ctx.dispatch_adaptive(at(cam, 0), 1, threshold=0.5)
    d = adaptive_ref.DEFAULTS
    assert ctx.adaptive_status().as_dict() == dict(active=W * H, samples=W * H * d["step"], min_count=d["step"], max_count=d["step"], rounds=1)
    assert not hasattr(native.MultiContext, "dispatch_adaptive")


def test_node_render_cli_adaptive(ctx, scene_factory, tmp_path):
    """render_cli.js --adaptive on a small scene equals the Python handle's output bit for bit"""
    host = os.path.join(ROOT, "wgpu-path-tracing_amd", "host")
    if not shutil.which("node") or not os.path.exists(os.path.join(host, "addon", "ptmi_napi.node")):
        pytest.skip("node or the N-API addon is not available")           # as tests/test_gpu_denoise.py's Node test
    from ptmi import scene_io
    sc = scene_factory("cornell")
    W, H = 32, 24
    path = tmp_path / "cornell.ptscene"
    scene_io.save_ptscene(sc, str(path))
    raw = tmp_path / "out.f32"
    out = subprocess.check_output(["node", os.path.join(host, "render_cli.js"), str(path), str(raw), "--width", str(W), "--height", str(H),
                                   "--adaptive", "0.35", "--max-frames", "64", "--rounds", "6"], text=True, timeout=300)
    info = json.loads(out.strip().splitlines()[-1])
    p = dict(threshold=0.35, max_frames=64)
    setup(ctx, sc, W, H)
    ctx.dispatch_adaptive(at(layout.make_camera(W, H), 0), 6, **p)
    assert same(np.fromfile(raw, np.float32).reshape(H, W, 4), ctx.read_output())
    ast = ctx.adaptive_status()
    assert info["adaptive"]["samples"] == ast.samples and info["adaptive"]["minCount"] == ast.min_count
    assert info["adaptive"]["maxCount"] == ast.max_count
