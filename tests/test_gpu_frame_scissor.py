"""The frame scissor on the GPU (include/ptmi.h ptmi_scissor_status): a plain dispatch that traces only the pixels inside
the scissor leaves the output and every counter of a dispatch that traces them all, bit for bit. The reference is this library with
the scissor off: a second context created under PTMI_SCISSOR=0 in the same process. What the full dispatch computes is pinned against
the oracle elsewhere (tests/test_gpu_parity.py and the files beside it).

Cornell, 96 x 54, 5 frames in batches of 2 (three batches, the last one short), 3 bounces, MIS on. Then everything that must switch
the scissor off, one at a time, with the reason the status gives, and the same frames again."""
import os

import numpy as np
import pytest

from ptmi import layout, native, scenes

pytestmark = pytest.mark.gpu

W, H, FRAMES = 96, 54, 5


@pytest.fixture(scope="module")
def pair():
    """(scissored, full): two contexts, the second created with the scissor switched off"""
    old = os.environ.pop("PTMI_SCISSOR", None)
    on = native.Context(0)
    os.environ["PTMI_SCISSOR"] = "0"
    try:
        off = native.Context(0)
    finally:
        if old is None:
            del os.environ["PTMI_SCISSOR"]
        else:
            os.environ["PTMI_SCISSOR"] = old
    yield on, off
    on.close()
    off.close()


@pytest.fixture(scope="module")
def cornell():
    return scenes.make("cornell")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def render(ctx, scene, cam, dispatch=None, **opt):
    o = dict(max_bounces=3, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=2, timing=0)
    o.update(opt)
    ctx.set_options(**o)
    if getattr(ctx, "_scissor_scene", None) is not scene:
        ctx.upload_scene(scene)
        ctx._scissor_scene = scene
    ctx.resize(W, H)
    ctx.write_output(np.full((H, W, 4), 0.25, np.float32))      # rows of another part keep this; frame 0 overwrites the rest
    ctx.reset_stats()
    (dispatch or (lambda: ctx.dispatch(cam, FRAMES)))()
    st = ctx.stats()
    counters = (int(st.paths), int(st.segments), [int(v) for v in st.segments_by_bounce], int(st.shadow_rays), int(st.frames_per_batch_used))
    return ctx.read_output(), counters, ctx.scissor_status().as_dict()


def both(pair, scene, cam, **kw):
    """renders on both contexts; asserts equal frames and counters; returns the scissored context's status and counters"""
    on, off = pair
    a, ca, sa = render(on, scene, cam, **kw)
    b, cb, sb = render(off, scene, cam, **kw)
    assert sb["applied"] == 0 and sb["reason"] == native.SCISSOR_OFF and sb["skipped"] == 0
    assert (sb["x0"], sb["x1"], sb["y0"], sb["y1"]) == (0, W, 0, H)
    assert ca == cb, (ca, cb)
    assert np.array_equal(bits(a), bits(b)), np.argwhere((bits(a) != bits(b)).any(-1))[:8]
    return sa, ca, a


def rolled(yaw, roll):
    cy, sy, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    fw, r0, u0 = np.array([sy, 0.0, -cy]), np.array([cy, 0.0, sy]), np.array([0.0, 1.0, 0.0])
    return dict(forward=fw, right=cr * r0 + sr * u0, up=-sr * r0 + cr * u0)


CAMERAS = {
    "default": dict(),
    "far, 17 pixels a row": dict(position=(0.07, 1.0, 9.0)),
    "cut by the left and top edges": dict(position=(0.9, 0.3, 2.8)),
    "aperture 0.3": dict(position=(0.0, 1.0, 6.0), aperture=0.3, focus_distance=5.0),
    "rotated": dict(position=(0.5, 1.2, 5.0), **rolled(0.25, 0.5)),
}


@pytest.mark.parametrize("name", list(CAMERAS))
def test_scissored_dispatch_equals_the_full_one(pair, cornell, name):
    cam = layout.make_camera(W, H, **CAMERAS[name])
    st, (paths, segments, by_bounce, _, fpb), img = both(pair, cornell, cam)
    assert st["applied"] == 1 and st["reason"] == native.SCISSOR_APPLIED
    x0, x1, y0, y1 = st["x0"], st["x1"], st["y0"], st["y1"]
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
    assert st["skipped"] == (W * H - (x1 - x0) * (y1 - y0)) * FRAMES > 0
    assert paths == by_bounce[0] == W * H * FRAMES and fpb == 2
    outside = np.ones((H, W), bool)
    outside[y0:y1, x0:x1] = False
    assert not bits(img)[outside].any()                         # folded zeros, over the 0.25 the buffer held
    assert img[..., :3].max() > 0.0
    if name.startswith("far"):
        assert x1 - x0 == 17
    if name.startswith("cut"):
        assert x0 == 0 and y1 == H and x1 < W and y0 > 0


@pytest.mark.parametrize("part", (0, 1))
def test_interleaved_strips(pair, cornell, part):
    """two parts of 4-row strips: the band's rows inside the scissor are one range of local rows, part by part"""
    cam = layout.make_camera(W, H, position=(0.07, 1.0, 9.0))      # rows 19 .. 34: the range starts and ends inside a strip
    st, (paths, _, by_bounce, _, _), img = both(pair, cornell, cam, tile_parts=2, tile_part=part, tile_strip=4)
    rows = [y for y in range(H) if (y // 4) % 2 == part]
    assert paths == by_bounce[0] == len(rows) * W * FRAMES
    inside = sum(1 for y in rows if st["y0"] <= y < st["y1"])
    assert st["applied"] == 1 and st["skipped"] == (len(rows) * W - inside * (st["x1"] - st["x0"])) * FRAMES > 0
    other = [y for y in range(H) if y not in rows]
    assert np.all(img[other] == 0.25) and not np.any(img[rows][..., :3] == 0.25)


def test_what_a_miss_can_reach_switches_it_off(pair, cornell):
    on, off = pair
    cam = layout.make_camera(W, H)
    sky = np.full((4, 8, 4), 0.5, np.float32)
    fog = dict(sigma_t=0.4, albedo=0.8, g=0.2, box=((-3.0, -1.0, -3.0), (3.0, 3.0, 3.0)))

    def each(f):
        for c in pair:
            f(c)

    try:
        each(lambda c: c.upload_environment(sky, sample=0))
        st, _, _ = both(pair, cornell, cam)
        assert (st["applied"], st["reason"], st["skipped"]) == (0, native.SCISSOR_ENVIRONMENT, 0)
        each(lambda c: c.set_environment(sample=1))                 # looked up only
        assert both(pair, cornell, cam)[0]["reason"] == native.SCISSOR_ENVIRONMENT
        each(lambda c: c.upload_environment(None))

        each(lambda c: c.set_medium(**fog))
        st, _, _ = both(pair, cornell, cam)
        assert (st["applied"], st["reason"]) == (0, native.SCISSOR_MEDIUM)
        each(lambda c: c.set_medium(None))

        each(lambda c: c.set_aovs("normal"))
        st, _, _ = both(pair, cornell, cam)
        assert (st["applied"], st["reason"]) == (0, native.SCISSOR_AOV)
        each(lambda c: c.set_aovs())

        each(lambda c: c.set_moments(True))
        st, _, _ = both(pair, cornell, cam)
        assert (st["applied"], st["reason"]) == (0, native.SCISSOR_MOMENTS)
        a, b = (render(c, cornell, cam, dispatch=lambda c=c: c.dispatch_adaptive(cam, rounds=2, threshold=0.2, min_frames=2, step=2))
                for c in pair)
        assert a[2]["applied"] == 0 and a[2]["reason"] == native.SCISSOR_NOT_PLAIN and b[2]["reason"] == native.SCISSOR_OFF
        assert a[1] == b[1] and np.array_equal(bits(a[0]), bits(b[0]))
        each(lambda c: c.set_moments(False))

        # an active cutoff table (inert here: every alpha is 1, tests/test_gpu_alpha.py): the resolve loops run on bounce 0's hits
        each(lambda c: c.set_alpha_cutoff(np.full(len(cornell.mats), 0.5, np.float32)))
        st, _, _ = both(pair, cornell, cam)
        assert (st["applied"], st["reason"], st["skipped"]) == (0, native.SCISSOR_ALPHA, 0)
        each(lambda c: c.set_alpha_cutoff(None))

        st, _, _ = both(pair, cornell, cam)                         # ... and with all of it gone it is back
        assert st["applied"] == 1 and st["skipped"] > 0
    finally:
        for c in pair:
            c.upload_environment(None)
            c.set_medium(None)
            c.set_aovs()
            c.set_moments(False)
            c.set_alpha_cutoff(None)


def test_box_off_the_frame(pair, cornell):
    """the empty rectangle: no entry, no path traced, the fold walks the band with zeros alone"""
    st, (paths, segments, by_bounce, shadow_rays, _), img = both(pair, cornell, layout.make_camera(W, H, position=(30.0, 1.0, 2.8)))
    assert (st["applied"], st["reason"]) == (1, native.SCISSOR_APPLIED)
    assert (st["x0"], st["x1"], st["y0"], st["y1"]) == (0, 0, 0, 0)
    assert st["skipped"] == paths == segments == by_bounce[0] == W * H * FRAMES and shadow_rays == 0 and not any(by_bounce[1:])
    assert not bits(img).any()


def test_camera_inside_the_scene(pair):
    room = scenes.make("cornell_enclosed")
    st, (paths, _, by_bounce, _, _), _ = both(pair, room, layout.make_camera(W, H))
    assert (st["applied"], st["reason"], st["skipped"]) == (0, native.SCISSOR_NO_PROMISE, 0)
    assert (st["x0"], st["x1"], st["y0"], st["y1"]) == (0, W, 0, H)
    assert paths == by_bounce[0] == W * H * FRAMES


def test_skipped_counts_since_reset(pair, cornell):
    on, _ = pair
    cam = layout.make_camera(W, H)
    _, _, st = render(on, cornell, cam)
    on.dispatch(cam, 3)
    assert on.scissor_status().skipped == st["skipped"] // FRAMES * (FRAMES + 3)
    on.reset_stats()
    assert on.scissor_status().skipped == 0 and on.scissor_status().applied == 1
