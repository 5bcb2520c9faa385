"""The frame scissor on the host (csrc/scene/frame_scissor.cpp): pt_frame_scissor answers a pixel rectangle outside which
every camera ray misses the box, or "whole frame". No GPU.

Set A: deterministic cameras around the Cornell box, every one with the whole inflated box strictly in front and itself outside it — the
premise is checked first, with the inflation restated here from the rule in DESIGN.md, and for such a camera the function may not answer
"whole frame". Each ray of the check is built as pipeline.hip camera_ray builds it, in float64 from the float32 camera record: the four
jitter corners and the centre of a pixel, each through the pinhole and through eight points of the lens rim. Every such ray of every
pixel outside the rectangle must miss the box (the box as handed in: un-inflated). For aperture 0 the rectangle is at most 3 pixels
wider per side than the bounding rectangle of the pixels one of whose rays hits: 2 of margin, and 1 because a corner of the box may poke
into a pixel without reaching one of its sampled points.

Set B: the cases that must answer "whole frame".

Set C: boxes and bases beyond Cornell — flat, line, point, tiny, long and far from the origin; scaled, left-handed and skewed bases; frames
of one column and of one row; fov from 0.05 to 3; lenses focused in front of and behind the box; aspect != W / H; cameras as near as 1.05
box radii. No premise is checked here: the function may answer "whole frame" (then it must leave the whole frame), but not often, and
whenever it answers a rectangle the same rays as in set A must miss outside it.
"""
import ctypes
import itertools

import numpy as np
import pytest

from ptmi import layout, scene_host, scenes

RECT, NOT_FINITE, PROJECTION, INSIDE, BEHIND, DEGENERATE = range(6)
FRAMES = ((96, 54), (64, 64))
FOVS = (0.6, np.pi / 3, 1.4)
LENSES = ((0.0, 5.0), (0.001, 2.8), (0.05, 2.8), (0.3, 2.8), (0.001, 5.0), (0.05, 5.0), (0.3, 5.0))     # (aperture, focus)
RADII = (3.0, 4.5, 6.0)
# look-at offsets from the box centre, as shares of the camera's distance: the box goes partly off the frame
OFFSETS = ((0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (0.0, -0.25, 0.1), (-0.2, 0.2, 0.0), (0.1, 0.1, -0.3), (-0.3, -0.1, 0.2))
N_DIRS = 210
JITTER = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.5))


@pytest.fixture(scope="module")
def fn():
    f = scene_host.lib().pt_frame_scissor
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.POINTER(ctypes.c_uint32)] * 4
    return f


@pytest.fixture(scope="module")
def box():
    """the Cornell box's bounds, padded the way a root box is (a relative 2^-16 of the largest coordinate)"""
    t = scenes.make("cornell").tris
    v = np.concatenate([t[k][:, :3] for k in ("v0", "v1", "v2")]).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    pad = np.abs(np.concatenate([lo, hi])).max() / 65536.0
    return (lo - pad).astype(np.float32), (hi + pad).astype(np.float32)


def scissor(fn, cam, box):
    lo, hi = (np.ascontiguousarray(b, np.float32) for b in box)
    r = [ctypes.c_uint32(7) for _ in range(4)]
    why = fn(cam.ctypes.data, lo.ctypes.data, hi.ctypes.data, *[ctypes.byref(v) for v in r])
    return why, tuple(int(v.value) for v in r)


def look_at(pos, target):
    f = np.asarray(target, np.float64) - pos
    f /= np.linalg.norm(f)
    world_up = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.99 else np.array([0.0, 0.0, 1.0])
    r = np.cross(f, world_up)
    r /= np.linalg.norm(r)
    return f, r, np.cross(r, f)


def cameras(box):
    """N_DIRS directions on a Fibonacci sphere; direction i sits on sphere i % 3 and takes one frame size, fov, lens and offset each
    by strides that are coprime to each other, so every value of every list and a spread of their pairs occur"""
    centre = (box[0].astype(np.float64) + box[1]) * 0.5
    golden = np.pi * (3.0 - np.sqrt(5.0))
    for i in range(N_DIRS):
        y = 1.0 - 2.0 * (i + 0.5) / N_DIRS
        rad = np.sqrt(1.0 - y * y)
        d = np.array([np.cos(golden * i) * rad, y, np.sin(golden * i) * rad])
        radius = RADII[i % 3]
        pos = centre + radius * d
        for rep in range(2):
            (w, h), fov, (ap, focus) = FRAMES[rep], FOVS[(i // 3) % 3], LENSES[(2 * i + rep) % 7]
            off = np.array(OFFSETS[(i // 9 + 3 * rep) % 6]) * radius
            f, r, u = look_at(pos, centre + off)
            yield layout.make_camera(w, h, position=pos, forward=f, right=r, up=u, fov=fov, aperture=ap, focus_distance=focus)


def cam_f64(cam):
    g = lambda k: np.asarray(cam[k], np.float64)
    return g("position"), g("forward"), g("right"), g("up")


def inflated(cam, box):
    """the rounding margin, then the lens: A max(1, (D - f) / (f - A)) with D the farthest corner's distance"""
    lo, hi = box[0].astype(np.float64), box[1].astype(np.float64)
    grow = np.abs(np.concatenate([lo, hi])).max() / 65536.0
    pos, _, rt, up = cam_f64(cam)
    ap, f = float(cam["aperture"]), float(cam["focus_distance"])
    if ap > 0.0:
        A = ap * np.sqrt(max(rt @ rt, up @ up) + abs(rt @ up))
        assert f > A
        corners = np.array(list(itertools.product(*zip(lo - grow, hi + grow))))
        D = np.linalg.norm(corners - pos, axis=1).max()
        grow += A * max(1.0, (D - f) / (f - A))
    return lo - grow, hi + grow


def premise(cam, box):
    lo, hi = inflated(cam, box)
    pos, fw, _, _ = cam_f64(cam)
    outside = bool(np.any(pos < lo) or np.any(pos > hi))
    corners = np.array(list(itertools.product(*zip(lo, hi))))
    q = corners - pos
    return outside and bool(np.all(q @ fw > 1e-3 * np.linalg.norm(q, axis=1)))


def rays_hit(cam, box):
    """(H, W) bool: some sampled ray of the pixel meets the box. pipeline.hip camera_dir / camera_ray in float64."""
    W, H = int(cam["width"]), int(cam["height"])
    pos, fw, rt, up = cam_f64(cam)
    th, aspect = np.tan(float(cam["fov"]) * 0.5), float(cam["aspect"])
    ap, focus = float(cam["aperture"]), float(cam["focus_distance"])
    lo, hi = box[0].astype(np.float64), box[1].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    hit = np.zeros((H, W), bool)
    lens = [None] + ([(ap * np.cos(a), ap * np.sin(a)) for a in np.arange(8) * np.pi / 4] if ap > 0.0 else [])
    for jx, jy in JITTER:
        uvx = ((xs + jx) / W) * 2.0 - 1.0
        uvy = ((ys + jy) / H) * 2.0 - 1.0
        d = fw + rt * (uvx * th * aspect)[..., None] + up * (uvy * th)[..., None]
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        for pt in lens:
            o, dd = pos, d
            if pt is not None:
                o = pos + up * pt[1] + rt * pt[0]
                dd = (pos + d * focus) - o
                dd = dd / np.linalg.norm(dd, axis=-1, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                t1, t2 = (lo - o) / dd, (hi - o) / dd
            par = dd == 0.0                                      # parallel to a slab: inside it for all t, or never
            inside = (o >= lo) & (o <= hi)
            tn = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
            tf = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
            hit |= tf.min(-1) >= np.maximum(tn.max(-1), 0.0)
    return hit


def test_set_a_rectangles_hold_and_are_tight(fn, box):
    cams = list(cameras(box))
    assert len(cams) == 2 * N_DIRS
    bad = [i for i, c in enumerate(cams) if not premise(c, box)]
    assert not bad, f"cameras {bad[:8]} of the list break the premise: fix the list"
    skipped_share = []
    for i, cam in enumerate(cams):
        why, (x0, x1, y0, y1) = scissor(fn, cam, box)
        assert why == RECT, (i, why)
        W, H = int(cam["width"]), int(cam["height"])
        assert 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H
        hit = rays_hit(cam, box)
        outside = np.ones((H, W), bool)
        outside[y0:y1, x0:x1] = False
        assert not (hit & outside).any(), (i, (x0, x1, y0, y1), np.argwhere(hit & outside)[:4])
        skipped_share.append(outside.mean())
        if float(cam["aperture"]) == 0.0 and hit.any():
            yy, xx = np.nonzero(hit)
            assert x0 >= xx.min() - 3 and x1 <= xx.max() + 1 + 3 and y0 >= yy.min() - 3 and y1 <= yy.max() + 1 + 3, \
                (i, (x0, x1, y0, y1), (xx.min(), xx.max() + 1, yy.min(), yy.max() + 1))
    assert max(skipped_share) > 0.5 and min(skipped_share) == 0.0       # the list has both: most of a frame spared, and none


def test_set_a_covers_every_listed_value(box):
    cams = list(cameras(box))
    assert {(int(c["width"]), int(c["height"])) for c in cams} == set(FRAMES)
    assert {float(c["fov"]) for c in cams} == {float(np.float32(f)) for f in FOVS}
    assert {(float(c["aperture"]), float(c["focus_distance"])) for c in cams} == {(float(np.float32(a)), float(np.float32(f))) for a, f in LENSES}
    centre = (box[0].astype(np.float64) + box[1]) * 0.5
    radii = {round(float(np.linalg.norm(np.asarray(c["position"], np.float64) - centre)), 2) for c in cams}
    assert radii == set(RADII)


def test_default_camera_spares_about_half_the_frame(fn, box):
    """the headline framing: the box covers about 54 % of the width and 96 % of the height of a 16:9 frame"""
    why, (x0, x1, y0, y1) = scissor(fn, layout.make_camera(1920, 1080), box)
    assert why == RECT
    assert 0.40 < 1.0 - (x1 - x0) * (y1 - y0) / (1920 * 1080) < 0.50


def test_set_b_whole_frame(fn, box):
    W, H = 96, 54
    whole = (0, W, 0, H)
    lo, hi = box[0].astype(np.float64), box[1].astype(np.float64)
    centre = (lo + hi) * 0.5
    cases = {
        "inside": (layout.make_camera(W, H, position=centre), INSIDE),
        "on a face": (layout.make_camera(W, H, position=(centre[0], centre[1], float(box[1][2]))), INSIDE),
        # looking along the front face from beside it: the far corners are ahead, the near ones behind
        "corner behind": (layout.make_camera(W, H, position=(hi[0] + 1.0, centre[1], centre[2]), forward=(0.0, 0.0, -1.0)), BEHIND),
        "orthographic": (layout.make_camera(W, H, projection=layout.PROJ_ORTHOGRAPHIC, ymag=2.0), PROJECTION),
        "equirect": (layout.make_camera(W, H, projection=layout.PROJ_EQUIRECT), PROJECTION),
    }
    nan = layout.make_camera(W, H)
    nan["forward"][1] = np.nan
    cases["nan"] = (nan, NOT_FINITE)
    for name, (cam, want) in cases.items():
        why, rect = scissor(fn, cam, box)
        assert why == want and rect == whole, (name, why, rect)
    for field in ("position", "right", "up"):
        cam = layout.make_camera(W, H)
        cam[field][0] = np.inf
        assert scissor(fn, cam, box) == (NOT_FINITE, whole), field
    for field in ("fov", "aspect", "aperture", "focus_distance"):
        cam = layout.make_camera(W, H)
        cam[field] = np.nan
        assert scissor(fn, cam, box) == (NOT_FINITE, whole), field
    nan_box = (box[0].copy(), box[1].copy())
    nan_box[1][2] = np.nan
    assert scissor(fn, layout.make_camera(W, H), nan_box) == (NOT_FINITE, whole)
    # what the argument does not cover: a lens as wide as its focus distance, a fov past 3, a singular basis
    assert scissor(fn, layout.make_camera(W, H, aperture=3.0, focus_distance=2.8), box) == (DEGENERATE, whole)
    assert scissor(fn, layout.make_camera(W, H, fov=3.1), box) == (DEGENERATE, whole)
    assert scissor(fn, layout.make_camera(W, H, up=(1.0, 0.0, 0.0)), box) == (DEGENERATE, whole)


def test_a_box_off_the_frame_leaves_no_pixel(fn, box):
    why, rect = scissor(fn, layout.make_camera(96, 54, position=(30.0, 1.0, 2.8)), box)
    assert why == RECT and rect == (0, 0, 0, 0)


# ---- set C -----------------------------------------------------------------------------------------------------------------------------
C_BOXES = {
    "flat in y": ((-1.0, 0.0, -1.0), (1.0, 0.0, 1.0)),
    "flat in z": ((-1.0, -1.0, 0.0), (1.0, 1.0, 0.0)),
    "line": ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
    "point": ((0.25, 0.5, -0.75), (0.25, 0.5, -0.75)),
    "1e-3 cube": ((-5e-4, -5e-4, -5e-4), (5e-4, 5e-4, 5e-4)),
    "beam": ((-50.0, -0.1, -0.1), (50.0, 0.1, 0.1)),
    "far cube": ((999.0, -2001.0, 499.0), (1001.0, -1999.0, 501.0)),
}
C_DISTANCES = (1.05, 1.5, 3.0, 10.0)                            # in box radii (half the diagonal; the point: 1)
C_BASES = ("orthonormal", "scaled", "left-handed", "skewed")
C_FRAMES = ((96, 54), (64, 64), (1, 37), (200, 1), (33, 97))
C_FOVS = (0.05, 0.6, 1.4, 2.5, 3.0)
C_LENSES = ((0.0, 1.0), (0.01, 0.5), (0.05, 2.0))               # (aperture, focus), both in camera distances
# look-at offsets from the box centre, in box radii
C_OFFSETS = ((0.0, 0.0, 0.0), (0.2, 0.0, 0.0), (0.0, -0.15, 0.1), (-0.1, 0.1, 0.0), (0.05, 0.05, -0.2))
C_N = 420                                                       # = 7 * 4 * 5 * 3: box x distance x frame x lens, each combination once


def c_box(name):
    lo, hi = (np.array(v, np.float32) for v in C_BOXES[name])
    return lo, hi


def c_cameras():
    """(camera, box, (box, distance, basis, frame, fov, lens)) for i < C_N. Box, distance, frame and lens go by i modulo their lists'
    lengths, which are pairwise coprime; the basis and the fov by strides of their own; the direction by a seeded generator."""
    rng = np.random.default_rng(25)
    names = list(C_BOXES)
    for i in range(C_N):
        name, dist, basis = names[i % 7], C_DISTANCES[i % 4], C_BASES[(i // 7) % 4]
        (w, h), fov, (ap, focus) = C_FRAMES[i % 5], C_FOVS[(i // 4) % 5], C_LENSES[i % 3]
        lo, hi = (b.astype(np.float64) for b in c_box(name))
        radius = np.linalg.norm(hi - lo) * 0.5 or 1.0
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        r = dist * radius
        centre = (lo + hi) * 0.5
        pos = centre + r * d
        fw, rt, up = look_at(pos, centre + np.array(C_OFFSETS[(i // 3) % 5]) * radius)
        if basis == "scaled":
            fw, rt, up = fw * 2.5, rt * 0.4, up * 1.7
        elif basis == "left-handed":
            rt = -rt
        elif basis == "skewed":
            rt = rt + 0.3 * up
            up = up + 0.2 * fw
        cam = layout.make_camera(w, h, position=pos, forward=fw, right=rt, up=up, fov=fov, aperture=ap * r, focus_distance=focus * r,
                                 aspect=0.7 if (i + i // 7) % 7 == 6 else None)     # one in seven, on another box each time
        yield cam, c_box(name), (name, dist, basis, (w, h), fov, (ap, focus))


def edge_pixels(cam, box, n=20001):
    """(H, W) bool: the pinhole image of a point of one of the box's twelve edges falls in the pixel, n points per edge, in float64. An
    image thinner than a pixel (a line, a beam, a plate seen edge-on) slips between the sampled rays of rays_hit; its outline does not
    slip through here, and the bounds of a convex image on the frame are reached on its outline or where rays_hit finds them."""
    W, H = int(cam["width"]), int(cam["height"])
    pos, fw, rt, up = cam_f64(cam)
    th, aspect = np.tan(float(cam["fov"]) * 0.5), float(cam["aspect"])
    lo, hi = box[0].astype(np.float64), box[1].astype(np.float64)
    c = np.array(list(itertools.product(*zip(lo, hi))))
    t = np.linspace(0.0, 1.0, n)[:, None]
    out = np.zeros((H, W), bool)
    for a in range(8):
        for k in (1, 2, 4):
            if a & k:
                continue
            q = c[a] + t * (c[a | k] - c[a]) - pos
            s, u, v = np.linalg.solve(np.stack([fw, rt, up], axis=1), q.T)
            ok = s > 0.0
            px, py = (u[ok] / s[ok] / (th * aspect) + 1.0) * 0.5 * W, (v[ok] / s[ok] / th + 1.0) * 0.5 * H
            on = (px >= 0.0) & (px < W) & (py >= 0.0) & (py < H)
            out[py[on].astype(int), px[on].astype(int)] = True
    return out


def test_set_c_rectangles_hold_beyond_cornell(fn):
    answers = {}
    seen = [set() for _ in range(6)]
    aspects = tight = 0
    for i, (cam, box, what) in enumerate(c_cameras()):
        W, H = int(cam["width"]), int(cam["height"])
        why, (x0, x1, y0, y1) = scissor(fn, cam, box)
        answers[why] = answers.get(why, 0) + 1
        if why != RECT:
            assert (x0, x1, y0, y1) == (0, W, 0, H), (i, what, why)
            continue
        assert 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H
        for s, v in zip(seen, what):
            s.add(v)
        aspects += float(cam["aspect"]) == float(np.float32(0.7))
        hit = rays_hit(cam, box)
        outside = np.ones((H, W), bool)
        outside[y0:y1, x0:x1] = False
        assert not (hit & outside).any(), (i, what, (x0, x1, y0, y1), np.argwhere(hit & outside)[:4])
        if what[5][0] == 0.0 and what[2] == "orthonormal":
            # against the box the function projects: far from the origin its 2^-16 margin is many pixels, by design
            big = inflated(cam, box)
            near = rays_hit(cam, big) | edge_pixels(cam, big)
            if near.any():
                yy, xx = np.nonzero(near)
                assert x0 >= xx.min() - 3 and x1 <= xx.max() + 1 + 3 and y0 >= yy.min() - 3 and y1 <= yy.max() + 1 + 3, \
                    (i, what, (x0, x1, y0, y1), (xx.min(), xx.max() + 1, yy.min(), yy.max() + 1))
                tight += 1
    print("set C answers:", answers)
    assert answers.get(RECT, 0) >= 0.85 * C_N, answers
    assert set(answers) <= {RECT, INSIDE, BEHIND}, answers
    # ... and those that answered a rectangle cover every listed value
    assert seen[0] == set(C_BOXES) and seen[1] == set(C_DISTANCES) and seen[2] == set(C_BASES)
    assert seen[3] == set(C_FRAMES) and seen[4] == set(C_FOVS) and seen[5] == set(C_LENSES)
    assert aspects > 0 and tight > 0


def test_set_c_aspect_is_0_7_on_every_seventh_camera():
    a = [float(c["aspect"]) for c, _, _ in c_cameras()]
    assert len(a) == C_N and sum(v == float(np.float32(0.7)) for v in a) == C_N // 7


def test_the_widest_frame_that_is_promised(fn, box):
    """65 536 pixels a side is the last size with a rectangle; one more answers "whole frame" """
    W, H = 65536, 2
    cam = layout.make_camera(W, H, aperture=0.0)
    why, (x0, x1, y0, y1) = scissor(fn, cam, box)
    assert why == RECT and 0 < x0 < x1 < W and (y0, y1) == (0, H)
    hit = rays_hit(cam, box)
    assert hit.any() and not hit[:, :x0].any() and not hit[:, x1:].any()
    assert scissor(fn, layout.make_camera(W + 1, H, aperture=0.0), box) == (DEGENERATE, (0, W + 1, 0, H))
    assert scissor(fn, layout.make_camera(H, W + 1, aperture=0.0), box) == (DEGENERATE, (0, H, 0, W + 1))
