"""tests/reproject_ref.py, the numpy model of ptmi_reproject (include/ptmi.h), on its own: no GPU. The planes of the camera moved
from are rendered with the CPU oracle and folded with tests/aov_ref.py / tests/adaptive_ref.py; the first hits of the camera moved
to come from Oracle.intersect on the float64 centre rays."""
import numpy as np
import pytest

import adaptive_ref
import aov_ref
import reproject_ref
from ptmi import layout

f32 = np.float32
W, H, FRAMES = 24, 32, 3
MISS = reproject_ref.MISS


def snapshot(oracle, scene, cam, frames):
    """the planes `frames` frames of a plain dispatch leave: output, moments, normal, albedo, id, each (H, W, C)"""
    w, h = int(cam["width"]), int(cam["height"])
    ys, xs = np.divmod(np.arange(w * h, dtype=np.uint32), np.uint32(w))
    rgb, mom = np.zeros((w * h, 3), f32), np.zeros((w * h, 4), f32)
    per_frame = []
    for f in range(frames):
        L, _ = oracle.trace_paths(scene, cam, xs, ys, np.full(w * h, f, np.uint32))
        rgb, mom = adaptive_ref.fold_listed(rgb, mom, L, np.full(w * h, f, np.uint32))
        per_frame.append(aov_ref.samples(oracle, scene, cam, f))
    alb, nrm, ids, _ = aov_ref.fold(per_frame, range(frames))
    out = np.zeros((h, w, 4), f32)
    out[..., :3] = rgb.reshape(h, w, 3)
    return dict(output=out, moments=mom.reshape(h, w, 4), normal=nrm.reshape(h, w, 4), albedo=alb.reshape(h, w, 4),
                id=ids.reshape(h, w, 2))


def first_hits(oracle, scene, cam):
    o, d = (a.astype(f32) for a in reproject_ref.center_rays64(cam))
    t, tri, _, _, _ = oracle.intersect(scene, o, d)
    return o, d, t, np.where(t < 0, MISS, tri).astype(np.uint32)


def tan_half_fov(oracle, cam):
    s, c = oracle.sincos(float(f32(cam["fov"]) * f32(0.5)))
    return f32(s) / f32(c)


@pytest.fixture(scope="module")
def case(oracle, scene_factory):
    sc = scene_factory("cornell")
    cam_from = layout.make_camera(W, H)
    cam_to = layout.make_camera(W, H, position=(0.3, 1.0, 2.8))
    snap = snapshot(oracle, sc, cam_from, FRAMES)
    o, d, t, tri = first_hits(oracle, sc, cam_to)
    args = dict(cam_from=cam_from, o=o, d=d, t=t, tri=tri, tri_material=sc.tris["material_index"], th=tan_half_fov(oracle, cam_from))
    return sc, snap, args


def bits_equal(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def test_a_sideways_move_carries_most_pixels(case):
    _, snap, args = case
    planes, st = reproject_ref.reproject(snap, **args)
    assert st["carried"] + st["disoccluded"] + st["missed"] == W * H
    assert st["carried"] > W * H // 2 and st["disoccluded"] > 0
    n = planes["moments"][..., 2]
    assert np.array_equal(n, np.floor(n)) and n.max() == FRAMES and st["samples"] == int(n.sum())
    carried = n > 0
    assert not planes["output"][~carried].any() and not planes["normal"][~carried].any() and not planes["albedo"][~carried].any()
    assert np.array_equal(planes["normal"][..., 3][carried], args["t"].reshape(H, W)[carried])
    assert np.isfinite(planes["output"]).all() and not planes["output"][..., 3].any() and not planes["moments"][..., 3].any()
    hit = args["tri"].reshape(H, W) != MISS
    assert np.array_equal(planes["id"][..., 0], args["tri"].reshape(H, W))
    assert (planes["id"][..., 1][hit] < 64).all() and (planes["id"][..., 1][~hit] == MISS).all()
    # a carried value is a convex combination of snapshot values: inside their range
    assert planes["output"][..., :3].max() <= snap["output"][..., :3].max() and planes["output"].min() >= 0


def test_looking_away_carries_nothing(case):
    _, snap, args = case
    away = args["cam_from"].copy()
    away["forward"] = -away["forward"]
    planes, st = reproject_ref.reproject(snap, **dict(args, cam_from=away))
    assert st["carried"] == 0 and st["samples"] == 0 and st["disoccluded"] + st["missed"] == W * H
    for k in ("output", "moments", "normal", "albedo"):
        assert not planes[k].any(), k


@pytest.mark.parametrize("max_history", [1, 2, 0])
def test_counts_are_integers_up_to_the_cap(case, max_history):
    _, snap, args = case
    snap = dict(snap, moments=snap["moments"].copy())
    snap["moments"][..., 2] = 40                                # far above the default cap of 32
    planes, st = reproject_ref.reproject(snap, max_history=max_history, **args)
    n = planes["moments"][..., 2]
    cap = max_history or 32
    assert st["carried"] > 0 and set(np.unique(n).tolist()) == {0.0, float(cap)}
    assert st["carried"] == int((n > 0).sum()) and st["samples"] == int(n.sum())


def test_identity_move_keeps_the_picture_where_the_depth_agrees(case, oracle):
    """from == to: the hit point projects onto its own pixel centre (fx = x up to rounding), so a carried pixel whose own tap is
    valid is, nearly, its own snapshot value (one whose own tap fails the depth test takes a neighbour's)"""
    sc, snap, args = case
    o, d, t, tri = first_hits(oracle, sc, args["cam_from"])
    planes, st = reproject_ref.reproject(snap, **dict(args, o=o, d=d, t=t, tri=tri))
    carried = planes["moments"][..., 2] > 0
    assert st["carried"] > 0.75 * (W * H - st["missed"])        # the rest: mean depths of jittered samples across an edge
    close = np.abs(planes["output"][carried] - snap["output"][carried]).max(axis=1) <= 2e-3
    assert close.mean() > 0.9


def test_taps_without_samples_or_with_a_nan_are_never_used(case):
    _, snap, args = case
    rng = np.random.default_rng(7)
    no_samples = rng.random((H, W)) < 0.15
    nan_at = (rng.random((H, W)) < 0.15) & ~no_samples
    a = {k: v.copy() for k, v in snap.items()}
    a["moments"][no_samples, 2] = 0
    for n, (y, x) in enumerate(zip(*np.nonzero(nan_at))):        # a NaN or an infinity in one float of one plane, in turn
        plane, ch = (("output", 0), ("output", 2), ("moments", 0), ("moments", 1), ("normal", 1), ("albedo", 3), ("albedo", 0))[n % 7]
        a[plane][y, x, ch] = (np.nan, np.inf, -np.inf)[n % 3]
    b = {k: v.copy() for k, v in a.items()}
    poisoned = no_samples | nan_at
    for k, ch in (("output", 3), ("moments", 2), ("albedo", 4)):     # whatever else such a pixel holds must not matter
        vals = b[k][poisoned]
        sub = vals[:, :ch]
        sub[np.isfinite(sub)] = f32(1e30)
        b[k][poisoned] = vals
    assert not bits_equal(a, b)
    pa, sa = reproject_ref.reproject(a, **args)
    pb, sb = reproject_ref.reproject(b, **args)
    assert sa == sb and bits_equal(pa, pb)
    for k in ("output", "moments", "normal", "albedo"):
        assert np.isfinite(pa[k]).all(), k
    clean, sc_ = reproject_ref.reproject(snap, **args)
    assert sa["carried"] < sc_["carried"] and sa["carried"] > 0


def test_a_band_reads_and_writes_only_its_rows(case):
    _, snap, args = case
    rows = adaptive_ref.band_rows(H, 5, 29)
    junk = {k: v.copy() for k, v in snap.items()}
    for k in ("output", "normal", "albedo"):
        junk[k][~rows] = 123.0
    junk["moments"][~rows] = (9.0, 9.0, 7.0, 0.0)
    junk["normal"][~rows, :, 3] = snap["normal"][~rows, :, 3]       # depths that would pass the test
    junk["id"][~rows] = snap["id"][~rows]
    pa, sa = reproject_ref.reproject(snap, rows=rows, **args)
    pb, sb = reproject_ref.reproject(junk, rows=rows, **args)
    assert sa == sb and sa["carried"] + sa["disoccluded"] + sa["missed"] == int(rows.sum()) * W
    for k in pa:
        assert np.array_equal(pa[k][rows].view(np.uint32), pb[k][rows].view(np.uint32)), k
        assert np.array_equal(pa[k][~rows].view(np.uint32), snap[k][~rows].view(np.uint32)), k      # untouched
        assert np.array_equal(pb[k][~rows].view(np.uint32), junk[k][~rows].view(np.uint32)), k
    # ... and the band's own edge rows lose the taps that fall outside: fewer carried pixels than the same rows of the whole frame
    whole, _ = reproject_ref.reproject(snap, **args)
    assert (pa["moments"][rows][..., 2] > 0).sum() <= (whole["moments"][rows][..., 2] > 0).sum()


def test_material_ids_gate_the_taps(case):
    _, snap, args = case
    other = dict(snap, id=snap["id"].copy())
    other["id"][..., 1] ^= 1 << 30                                   # no tap's material matches any more
    _, st = reproject_ref.reproject(other, **args)
    assert st["carried"] == 0
    _, st1 = reproject_ref.reproject(other, match_ids=1, **args)
    _, st0 = reproject_ref.reproject(snap, **args)
    _, off = reproject_ref.reproject(dict(other, id=None), **args)
    assert st1["carried"] == off["carried"] >= st0["carried"] > 0
    with pytest.raises(AssertionError):
        reproject_ref.reproject(dict(snap, id=None), match_ids=2, **args)


def test_center_rays64_are_the_pinhole_rays(oracle):
    """against the oracle's ray generation: without a lens, its ray through (x + jx, y + jy); the centre ray differs from it by the
    jitter only, so both lie within half a pixel's angle"""
    cam = layout.make_camera(W, H, aperture=0.0)
    o, d = reproject_ref.center_rays64(cam)
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    oo, dd, _ = oracle.raygen(cam, xs, ys, np.zeros(W * H, np.uint32))
    assert np.array_equal(o.astype(f32), oo)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1).max() < 1e-12
    pixel = 2 * np.tan(np.pi / 6) / H
    assert np.abs(d - dd).max() < pixel
