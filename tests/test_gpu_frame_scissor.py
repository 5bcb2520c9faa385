"""The frame scissor on the GPU (include/ptmi.h ptmi_scissor_status): a plain dispatch that traces only the pixels inside
the scissor leaves the output and every counter of a dispatch that traces them all, bit for bit. The reference is this library with
the scissor off: a second context created under PTMI_SCISSOR=0 in the same process. What the full dispatch computes is pinned against
the oracle elsewhere (tests/test_gpu_parity.py and the files beside it).

Cornell, 96 x 54, 5 frames in batches of 2 (three batches, the last one short), 3 bounces, MIS on. Then everything that must switch
the scissor off, one at a time, with the reason the status gives, and the same frames again.

Further down, what only the benchmark or nothing reached: accumulation resumed at frame_index > 0 under a camera that moves (outside
pixels decay, by a float32 model of pipeline.hip fold), one 1600 x 900 frame whose pixels and whose rectangle both exceed one round of
the n_cu * 8 * 256-thread grids, contiguous row bands (tile_y0 / tile_y1) above, below and across the rectangle, rectangles of 5 x 5
pixels, of every row and cut by the right and bottom edges, every option an upload or a dispatch reads, and — the one check whose
reference is not this library's dispatch — ptmi_debug_raygen's rays of the ring just outside the rectangle against the bounds of the
device's triangles. The pair of contexts and the comparison are in tests/scissor_pair.py; the edits of a loaded scene in
tests/test_gpu_frame_scissor_edits.py; multi-device handles in tests/test_gpu_multi_scissor.py."""
import numpy as np
import pytest

from ptmi import layout, native, scenes
from scissor_pair import FRAMES, H, W, bits, both, contains, forget_scene, host_rect, make_pair, rect, render, slab_hits, triangle_bounds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pair():
    """(scissored, full): two contexts, the second created with the scissor switched off"""
    on, off = make_pair()
    yield on, off
    on.close()
    off.close()


@pytest.fixture(scope="module")
def cornell():
    return scenes.make("cornell")


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


# ---- accumulation that goes on, more than one round of the grid, row bands, thin rectangles, options, the device's own rays ----------

FAR = CAMERAS["far, 17 pixels a row"]
CUT = CAMERAS["cut by the left and top edges"]


def decayed(v, frames):
    """pipeline.hip fold with x = 0 at each frame f > 0 of `frames`: mix1(acc, 0, t) = fma(0, t, acc * (1 - t)), t = 1 / (f + 1)"""
    acc = np.asarray(v, np.float32)
    for f in frames:
        t = np.float32(1.0) / np.float32(f + 1)
        acc = acc * (np.float32(1.0) - t) + np.float32(0.0)
    return acc


def test_resumed_accumulation_under_a_camera_that_moves(pair, cornell):
    """frames 0 .. 2, 3 .. 5 and 6 .. 7 under three cameras with no write to the output in between: from frame 1 on a pixel outside the
    rectangle is a decay of what the buffer holds, and pixels change sides mid-accumulation"""
    s1, _, a1 = both(pair, cornell, layout.make_camera(W, H, **FAR), frames=3)
    s2, _, a2 = both(pair, cornell, layout.make_camera(W, H, frame_index=3, **CUT), frames=3, fill=None)
    s3, _, a3 = both(pair, cornell, layout.make_camera(W, H, frame_index=6), frames=2, fill=None)
    assert s1["applied"] == s2["applied"] == s3["applied"] == 1 and len({rect(s) for s in (s1, s2, s3)}) == 3
    in1 = np.zeros((H, W), bool)
    in1[s1["y0"]:s1["y1"], s1["x0"]:s1["x1"]] = True
    out2 = np.ones((H, W), bool)
    out2[s2["y0"]:s2["y1"], s2["x0"]:s2["x1"]] = False
    moved_out = in1 & out2 & (a1[..., :3] > 0.0).any(-1)         # traced in step 1, zero-folded in step 2, and holding something
    assert moved_out.any(), (rect(s1), rect(s2))
    want = decayed(a1[moved_out][:, :3], (3, 4, 5))
    assert np.array_equal(bits(a2[moved_out][:, :3]), bits(want)), (bits(a2[moved_out][:, :3])[:4], bits(want)[:4])
    assert (want > 0.0).any() and (a3[..., :3] > 0.0).any()
    # ... and the pixels outside both of the first two rectangles went from the fill to zero at frame 0 and stayed there
    assert not bits(a2)[~in1 & out2].any()


def test_more_than_one_round_of_the_grid(pair, cornell):
    """raygen and the fold launch n_cu * 8 blocks of 256 threads: a frame with more pixels than that, and a rectangle with more
    entries, take ScissoredPixels::pixel, fold_entry and the index k * n + e through further rounds of the grid-stride loops"""
    from test_gpu_edit_edges import device_cus               # torch's multi_processor_count of device 0, asked in a child process
    n_cu = device_cus()
    threads = n_cu * 8 * 256
    w, h = 1600, 900
    hint = f"this device launches {threads} threads: choose a frame whose default-camera rectangle holds more pixels than that"
    assert w * h > threads, hint
    st, (paths, _, by_bounce, _, fpb), img = both(pair, cornell, layout.make_camera(w, h), frames=2, frames_per_batch=1, max_bounces=2)
    assert st["applied"] == 1 and fpb == 1
    entries = (st["x1"] - st["x0"]) * (st["y1"] - st["y0"])
    assert threads < entries < w * h, (hint, rect(st))
    assert st["skipped"] == (w * h - entries) * 2 and paths == by_bounce[0] == w * h * 2
    outside = np.ones((h, w), bool)
    outside[st["y0"]:st["y1"], st["x0"]:st["x1"]] = False
    assert not bits(img)[outside].any() and img[..., :3].max() > 0.0


@pytest.mark.parametrize("y0,y1,where", [(2, 12, "above"), (40, 50, "below"), (30, 45, "across the lower edge"), (25, 26, "one row inside")])
def test_row_bands(pair, cornell, y0, y1, where):
    """tile_y0 / tile_y1, what a multi-device handle gives each device: a band wholly above or below the rectangle has no entry while
    the column range is not empty"""
    cam = layout.make_camera(W, H, **FAR)                       # rows 19 .. 34
    st, (paths, segments, by_bounce, shadow_rays, _), img = both(pair, cornell, cam, tile_y0=y0, tile_y1=y1)
    rows = y1 - y0
    assert st["applied"] == 1 and st["reason"] == native.SCISSOR_APPLIED and st["x0"] < st["x1"] and st["y0"] < st["y1"]
    inside = len([y for y in range(y0, y1) if st["y0"] <= y < st["y1"]])
    assert inside == {"above": 0, "below": 0, "across the lower edge": st["y1"] - 30, "one row inside": 1}[where]
    assert st["skipped"] == (rows * W - inside * (st["x1"] - st["x0"])) * FRAMES
    assert paths == by_bounce[0] == rows * W * FRAMES
    other = [y for y in range(H) if not y0 <= y < y1]
    assert np.all(img[other] == 0.25)
    if not inside:
        assert segments == paths and shadow_rays == 0 and not any(by_bounce[1:])
        assert not bits(img[y0:y1]).any()
    else:
        assert img[y0:y1, :, :3].max() > 0.0 and segments > paths


def test_thin_rectangles(pair, cornell):
    # 400 units away the box is a fraction of a pixel, and the camera is set half a pixel off both ways so that the fraction lies
    # inside one pixel: that pixel and the margin of 2 on every side
    st, _, _ = both(pair, cornell, layout.make_camera(W, H, position=(4.3, 5.3, 400.0)))
    assert st["applied"] == 1 and (st["x1"] - st["x0"], st["y1"] - st["y0"]) == (5, 5), rect(st)
    # a frame of 5 rows: every row, not every column
    st, _, img = both(pair, cornell, layout.make_camera(W, 5))
    assert st["applied"] == 1 and (st["y0"], st["y1"]) == (0, 5) and 0 < st["x0"] < st["x1"] < W, rect(st)
    assert img[..., :3].max() > 0.0
    # the mirror of the camera cut by the left and top edges: the right and the bottom edge
    st, _, img = both(pair, cornell, layout.make_camera(W, H, position=(-0.9, 1.7, 2.8)))
    assert st["applied"] == 1 and st["x1"] == W and st["y0"] == 0 and st["x0"] > 0 and st["y1"] < H, rect(st)
    assert img[:, W - 1, :3].max() > 0.0 and img[0, :, :3].max() > 0.0      # something is seen in the last column and in row 0


def upload_options(pair, **opt):
    for c in pair:
        c.set_options(**opt)
    forget_scene(pair)


@pytest.mark.parametrize("leaves,builder", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_options_read_at_upload(pair, cornell, leaves, builder):
    on, _ = pair
    upload_options(pair, leaves=leaves, tree_builder=builder)
    try:
        for name in ("default", "cut by the left and top edges"):
            st, _, _ = both(pair, cornell, layout.make_camera(W, H, **CAMERAS[name]))
            assert st["applied"] == 1 and st["skipped"] > 0, name
            stats = on.stats()
            assert stats.leaves_used == leaves
            # the device builds over the uploaded leaves; own leaves of a scene of at most 4 096 triangles keep the host builder
            assert stats.tree_builder_used == (builder if leaves == 1 else 1)
            if leaves == 2:
                # own leaves: the walked root is padded and differs from the uploaded tree's, and the rectangle holds both boxes'
                info = on.read_image()[0]
                lo, hi = triangle_bounds(on.read_triangles())
                assert tuple(info.root_min) != tuple(lo) or tuple(info.root_max) != tuple(hi)
                cam = layout.make_camera(W, H, **CAMERAS[name])
                for box in ((lo, hi), (np.array(info.root_min, np.float32), np.array(info.root_max, np.float32))):
                    why, r = host_rect(cam, *box)
                    assert why == 0 and contains(rect(st), r), (name, rect(st), r)
    finally:
        upload_options(pair, leaves=0, tree_builder=0)


@pytest.mark.parametrize("opt,value", [("traversal", native.TRAVERSAL_GLOBAL), ("traversal", native.TRAVERSAL_LDS),
                                       ("traversal", native.TRAVERSAL_GLOBAL_EXACT), ("overlap", 0), ("overlap", 1),
                                       ("perf_mode", 0), ("perf_mode", 1), ("do_mis", 0), ("do_mis", 1), ("max_bounces", 1)])
def test_options_read_at_dispatch(pair, cornell, opt, value):
    on, _ = pair
    before = {k: getattr(on.options(), k) for k in ("traversal", "overlap", "perf_mode")}
    try:
        for name in ("default", "cut by the left and top edges"):
            st, (paths, segments, by_bounce, shadow_rays, _), _ = both(pair, cornell, layout.make_camera(W, H, **CAMERAS[name]), **{opt: value})
            assert st["applied"] == 1 and st["skipped"] > 0, name
            stats = on.stats()
            assert getattr(on.options(), opt) == value
            if opt == "traversal":
                assert stats.traversal_used == (native.TRAVERSAL_LDS if value == native.TRAVERSAL_LDS else native.TRAVERSAL_GLOBAL)
                if value != native.TRAVERSAL_LDS:                # csrc/pt_device.h kPtVariants: 8 walks the quantised nodes from memory, 9 the exact
                    quantised = on.read_image()[0].quantised and value == native.TRAVERSAL_GLOBAL
                    assert stats.extend_variant // 10 == (8 if quantised else 9)
                    assert stats.radiance_stride_bytes == (16 if quantised else 12)
            if opt == "do_mis":
                assert (shadow_rays > 0) == bool(value)
            if opt == "max_bounces":
                assert segments == by_bounce[0] == paths and not any(by_bounce[1:])
            else:
                assert by_bounce[2] > 0
    finally:
        for c in pair:
            c.set_options(**before)


EXTRA_LENS = dict(position=(0.3, 0.8, 7.0), aperture=0.3, focus_distance=3.0)     # focused in front of the box: the lens rays fan out behind


@pytest.mark.parametrize("name", list(CAMERAS) + ["aperture 0.3, focused short"])
def test_no_ray_of_the_device_from_the_ring_outside_meets_the_box(pair, cornell, name):
    """the one check here whose reference is not this library's own dispatch: the rays ptmi_debug_raygen returns for the pixels of the
    one-pixel ring just outside the reported rectangle, frames 0 .. 15, against the exact bounds of the device's triangles in float64"""
    on, _ = pair
    cam = layout.make_camera(W, H, **(CAMERAS.get(name) or EXTRA_LENS))
    _, _, st = render(on, cornell, cam)
    assert st["applied"] == 1
    x0, x1, y0, y1 = rect(st)
    ring = [(x, y) for y in range(y0 - 1, y1 + 1) for x in range(x0 - 1, x1 + 1)
            if (x in (x0 - 1, x1) or y in (y0 - 1, y1)) and 0 <= x < W and 0 <= y < H]
    assert len(ring) >= min(x1 - x0, y1 - y0)                 # (a rectangle cut by the frame has no ring on that side)
    xs, ys = (np.repeat(np.array(v, np.uint32), 16) for v in zip(*ring))
    frames = np.tile(np.arange(16, dtype=np.uint32), len(ring))
    o, d, _ = on.debug_raygen(cam, xs, ys, frames)
    assert np.isfinite(o).all() and np.isfinite(d).all() and (np.abs(d).max(-1) > 0.5).all()
    if float(cam["aperture"]) >= 0.3:
        assert np.ptp(o, axis=0).max() > 0.1                   # the lens is sampled: origins spread
    lo, hi = triangle_bounds(on.read_triangles())
    hit = slab_hits(o, d, lo, hi)
    assert not hit.any(), (name, rect(st), [(int(xs[i]), int(ys[i]), int(frames[i])) for i in np.flatnonzero(hit)[:8]])
