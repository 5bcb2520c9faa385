"""The frame scissor after an edit of the loaded scene (§13, §16 - §19 for the edits): the rectangle is worked out from
the context's root boxes, and five entry points rewrite those after the upload — update_triangles, transform_groups, pose_skin,
pose_morph (all through scene_update.hip refit_written) and rebuild_tree. A box that is stale or half updated crops the moved geometry,
and the counters still add up.

The idiom of tests/test_gpu_frame_scissor.py (tests/scissor_pair.py): two contexts, the second with the scissor off, every call given to
both in the same order. Per case: render, edit, render again from frame 0, and
  (i)   the scissored frame and counters are the full dispatch's, bit for bit;
  (ii)  the scissor applied;
  (iii) the reported rectangle contains pt_frame_scissor's answer for the exact bounds of the triangles read back from the device — a
        reference that does not pass through root_min / root_max — and, with own leaves, its answer for the walked image's padded
        root box as ptmi_debug_read_image reports it (the union of dispatch.hip frame_scissor);
  (iv)  the case is not vacuous: the rectangle grew where the geometry went, and a pixel beyond the old rectangle is lit.
Tried on mutated builds: a refit that leaves the walked root stale keeps (i) and (iii) — both contexts cull the block at the stale root,
and the refitted uploaded root is in the union — and fails (iv); a walked root that only ever grows fails the shrink step's "the first
rectangle again"; a dispatch that reads the uploaded tree's root alone fails the pixel-boundary case at the end of this file and
nothing else.

The edit moves the short block (12 triangles, material 5) by (0.6, 0, 1.4): out of the room to the front right, where the lamp
reaches its top face through the open front. (Moved along +x alone it would stand behind the red wall in the dark, and (iv) would
have nothing to see.) Cornell, 96 x 54, 3 bounces, MIS, 4 frames in batches of 2."""
import numpy as np
import pytest

from ptmi import layout, native, scenes
from scissor_pair import H, W, bits, both, contains, forget_scene, host_rect, make_pair, rect, triangle_bounds

pytestmark = pytest.mark.gpu

FRAMES = 4
SHIFT = (0.6, 0.0, 1.4)
E_UNSUPPORTED = -5
# (leaves, keep_reference_tree): the reference's leaves, own leaves, and own leaves asked for beside the tree walked as uploaded
MODES = ((1, 0), (2, 0), (2, 1))
ENTRIES = ("update_triangles", "transform_groups", "pose_skin", "pose_morph")


@pytest.fixture(scope="module")
def pair():
    on, off = make_pair()
    yield on, off
    on.close()
    off.close()


@pytest.fixture(scope="module")
def cornell():
    return scenes.make("cornell")


def block_of(scene):
    b = np.flatnonzero(scene.tris["material_index"] == 5).astype(np.uint32)
    assert len(b) == 12
    return b


def affine(shift):
    m = np.zeros((3, 4), np.float32)
    m[:, :3] = np.eye(3, dtype=np.float32)
    m[:, 3] = shift
    return m


class Edit:
    """one entry point's way of moving the block by `shift` from where the upload put it; shift (0, 0, 0) moves it back"""

    def __init__(self, entry, scene):
        self.entry, self.scene, self.block = entry, scene, block_of(scene)

    def prepare(self, c):
        n, b = len(self.scene.tris), self.block
        if self.entry == "transform_groups":                     # one group holding the block, the rest in another
            g = np.zeros(n, np.uint32)
            g[b] = 1
            c.set_triangle_groups(g)
        elif self.entry == "pose_skin":                          # one joint, weight 1
            corners = np.zeros(3 * len(b), layout.SKIN_CORNER)
            corners["weight"][:, 0] = 1.0
            c.set_skin(b, corners, n_joints=1)
        elif self.entry == "pose_morph":                         # one target, weight 1: a row of one record per triangle
            d = np.zeros(len(b), layout.MORPH_DELTA)
            for k in ("dv0", "dv1", "dv2"):
                d[k] = np.array(SHIFT, np.float32)
            c.set_morph(b, np.arange(len(b) + 1, dtype=np.uint32), d, n_targets=1)

    def apply(self, c, shift):
        if self.entry == "update_triangles":
            moved = self.scene.tris[self.block].copy()
            for k in ("v0", "v1", "v2"):
                moved[k] += np.array(shift, np.float32)
            lo, hi = int(self.block.min()), int(self.block.max()) + 1      # one call: the range that holds the block, mostly unchanged
            rec = self.scene.tris[lo:hi].copy()
            rec[self.block - lo] = moved
            c.update_triangles(lo, rec)
        elif self.entry == "transform_groups":
            c.transform_groups([(1, affine(shift))])
        elif self.entry == "pose_skin":
            c.pose_skin([(affine(shift), None)])
        elif self.entry == "pose_morph":
            c.pose_morph([1.0 if any(shift) else 0.0])


def upload(pair, scene, leaves, keep, builder=1):
    for c in pair:
        c.set_options(leaves=leaves, keep_reference_tree=keep, tree_builder=builder, traversal=native.TRAVERSAL_AUTO, cull=1)
    forget_scene(pair)


def restore(pair):
    for c in pair:
        c.set_options(leaves=0, keep_reference_tree=0, tree_builder=0)
    forget_scene(pair)


def check_rectangle(on, cam, st, what):
    """(ii) and (iii); returns the rectangle of the device's triangles"""
    assert st["applied"] == 1 and st["reason"] == native.SCISSOR_APPLIED, (what, st)
    why, tight = host_rect(cam, *triangle_bounds(on.read_triangles()))
    assert why == 0 and contains(rect(st), tight), (what, "the device's triangles", rect(st), tight)
    info = on.read_image()[0]
    if info.leaves_used == 2:
        why, padded = host_rect(cam, np.array(info.root_min, np.float32), np.array(info.root_max, np.float32))
        assert why == 0 and contains(rect(st), padded), (what, "the walked image's root box", rect(st), padded)
    return tight


@pytest.mark.parametrize("leaves,keep", MODES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_grow_then_shrink(pair, cornell, entry, leaves, keep):
    on, off = pair
    what = f"{entry} leaves {leaves} keep {keep}"
    cam = layout.make_camera(W, H)
    edit = Edit(entry, cornell)
    upload(pair, cornell, leaves, keep)
    try:
        st0, c0, img0 = both(pair, cornell, cam, frames=FRAMES)
        assert on.stats().leaves_used == (2 if leaves == 2 and not keep else 1)     # (keep: the tree is walked as uploaded, no own leaves)
        tight0 = check_rectangle(on, cam, st0, what + ": as uploaded")
        for c in pair:
            edit.prepare(c)
            edit.apply(c, SHIFT)
        # grow
        st1, c1, img1 = both(pair, cornell, cam, frames=FRAMES)
        tight1 = check_rectangle(on, cam, st1, what + ": grown")
        assert tight1[1] > tight0[1] and st1["x1"] > st0["x1"], (what, rect(st0), rect(st1))
        lit = np.argwhere(bits(img1)[:, st0["x1"]:, :3].any(-1))
        assert len(lit), f"{what}: no lit pixel in a column >= {st0['x1']}"
        assert not np.array_equal(bits(img0), bits(img1))
        # shrink: the inverse edit through the same entry point
        for c in pair:
            edit.apply(c, (0.0, 0.0, 0.0))
        assert on.read_triangles().tobytes() == cornell.tris.tobytes(), what
        st2, c2, img2 = both(pair, cornell, cam, frames=FRAMES)
        check_rectangle(on, cam, st2, what + ": shrunk")
        assert rect(st2) == rect(st0), (what, rect(st0), rect(st2))
        assert c2 == c0 and np.array_equal(bits(img2), bits(img0)), (what, np.argwhere((bits(img2) != bits(img0)).any(-1))[:8])
    finally:
        restore(pair)


@pytest.mark.parametrize("builder", (1, 2))
def test_rebuild_tree_after_a_grow(pair, cornell, builder):
    on, off = pair
    what = f"rebuild_tree builder {builder}"
    cam = layout.make_camera(W, H)
    edit = Edit("update_triangles", cornell)
    upload(pair, cornell, 2, 0)
    try:
        st0, _, _ = both(pair, cornell, cam, frames=FRAMES)
        for c in pair:
            edit.apply(c, SHIFT)
        st1, c1, img1 = both(pair, cornell, cam, frames=FRAMES)
        check_rectangle(on, cam, st1, what + ": grown")
        assert st1["x1"] > st0["x1"]
        for c in pair:
            assert c.rebuild_tree(builder).rebuilds == 1
        st2, c2, img2 = both(pair, cornell, cam, frames=FRAMES)
        check_rectangle(on, cam, st2, what + ": rebuilt")
        assert rect(st2) == rect(st1), (what, rect(st1), rect(st2))
        assert len(np.argwhere(bits(img2)[:, st0["x1"]:, :3].any(-1)))
    finally:
        restore(pair)


@pytest.mark.parametrize("leaves,keep", ((1, 0), (2, 1)))
def test_rebuild_tree_is_refused_without_own_leaves(pair, cornell, leaves, keep):
    """... and the refused call leaves the scissor what it was"""
    on, off = pair
    cam = layout.make_camera(W, H)
    upload(pair, cornell, leaves, keep)
    try:
        st0, c0, img0 = both(pair, cornell, cam, frames=FRAMES)
        for c in pair:
            with pytest.raises(native.PtmiError) as e:
                c.rebuild_tree(1)
            assert e.value.code == E_UNSUPPORTED
        st1, c1, img1 = both(pair, cornell, cam, frames=FRAMES)
        assert rect(st1) == rect(st0) and st1["applied"] == 1 and c1 == c0 and np.array_equal(bits(img1), bits(img0))
    finally:
        restore(pair)


def rect_at(x, box):
    return host_rect(layout.make_camera(W, H, position=(float(x), 1.0, 2.8)), *box)[1]


def test_the_padded_root_box_counts_on_a_pixel_boundary(pair, cornell):
    """Own leaves pad the walked root by a few ulp, far less than a pixel, so the two boxes of dispatch.hip frame_scissor nearly always
    give one rectangle and a dispatch that read only one of them would pass (iii). Here the camera is walked to the right, by bisection
    over float32 positions on the host, until an edge of the tight box's image sits on a pixel boundary: between two neighbouring
    positions its rectangle changes, and at one of the two the padded box's rectangle is already, or still, the other one. There the
    reported rectangle must hold both."""
    on, off = pair
    upload(pair, cornell, 2, 0)
    try:
        both(pair, cornell, layout.make_camera(W, H), frames=FRAMES)
        for c in pair:
            Edit("update_triangles", cornell).apply(c, SHIFT)
        info = on.read_image()[0]
        assert info.leaves_used == 2 and info.pad > 0.0
        tight = triangle_bounds(on.read_triangles())
        padded = (np.array(info.root_min, np.float32), np.array(info.root_max, np.float32))
        assert np.all(padded[0] < tight[0]) and np.all(padded[1] > tight[1])
        a, b = np.float32(0.0), np.float32(0.5)
        first = rect_at(a, tight)
        assert rect_at(b, tight) != first
        while True:
            m = np.float32((np.float64(a) + np.float64(b)) * 0.5)
            if m == a or m == b:
                break
            a, b = (m, b) if rect_at(m, tight) == first else (a, m)
        apart = [x for x in (a, b) if rect_at(x, tight) != rect_at(x, padded)]
        assert apart, ("no float32 camera position tells the boxes apart", float(a), float(b), float(info.pad))
        cam = layout.make_camera(W, H, position=(float(apart[0]), 1.0, 2.8))
        st, _, _ = both(pair, cornell, cam, frames=FRAMES)
        assert st["applied"] == 1
        for name, box in (("the device's triangles", tight), ("the walked image's root box", padded)):
            assert contains(rect(st), host_rect(cam, *box)[1]), (name, rect(st), host_rect(cam, *box)[1])
    finally:
        restore(pair)
