"""tests/lbvh_ref.py, the plain model of the device LBVH builder (csrc/gpu_tree.hip), checked by itself on the CPU: hand cases whose tree
can be written down, the properties any such tree has (every inner box the union of the leaves below it, every leaf once, n - 1 inner
nodes numbered in left-first preorder) on real scenes, and the coverage the GPU comparison of tests/test_gpu_tree_builder.py relies on
(equal codes, all codes equal, an axis without extent, the exact leaf counts around the builder's block size), asserted from the
model alone so that a change to ptmi.scenes cannot quietly remove it."""
import numpy as np
import pytest

import lbvh_ref
from lbvh_ref import REF_LEAF

F = np.float32


def leaves_at(centres, half):
    """cubes of the given half sizes around the given centres, with made-up reference words (leaf k: one triangle, number 7 k)"""
    c, h = np.array(centres, F), np.array(half, F).reshape(-1, 1)
    return c - h, c + h, (np.uint32(REF_LEAF) | (np.arange(len(c), dtype=np.uint32) * np.uint32(7))).astype(np.uint32)


def children(m):
    return m.wnodes.view(np.uint32)[:, 12:14].tolist()


def leaf(k):
    return REF_LEAF | 7 * k


def test_two_leaves():
    mn, mx, ref = leaves_at([(4, 0, 0), (1, 0, 0)], [0.5, 0.25])              # given in descending x: the sort must swap them
    m = lbvh_ref.build_from_leaves(mn, mx, ref)
    assert (m.root_ref, m.depth, m.n_wnodes) == (0, 2, 1)
    assert children(m) == [[leaf(1), leaf(0)]]
    want = [0.75, -0.25, -0.25, 1.25, 0.25, 0.25, 3.5, -0.5, -0.5, 4.5, 0.5, 0.5]      # left min, left max, right min, right max
    assert m.wnodes[0, :12].tolist() == want and not m.wnodes.view(np.uint32)[0, 14:].any()
    assert m.codes.tolist() == [0b100100100100100100100100100100, 0]           # x = 1023 and 0: every third bit from bit 2 up


def test_three_leaves():
    # centroids x = 10, 0, 1 -> 1023, 0, 102 of 1024: the top x bit separates {0, 1} from {10}, then bit 6 of x (102 = 0b1100110) splits them
    mn, mx, ref = leaves_at([(10, 0, 0), (0, 0, 0), (1, 0, 0)], [0.5, 0.5, 0.5])
    m = lbvh_ref.build_from_leaves(mn, mx, ref)
    assert (m.root_ref, m.depth, m.n_wnodes) == (0, 3, 2)
    assert children(m) == [[1, leaf(0)], [leaf(1), leaf(2)]]
    assert m.wnodes[0, :12].tolist() == [-0.5, -0.5, -0.5, 1.5, 0.5, 0.5, 9.5, -0.5, -0.5, 10.5, 0.5, 0.5]    # left: the union below node 1
    assert m.wnodes[1, :12].tolist() == [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5, 0.5, -0.5, -0.5, 1.5, 0.5, 0.5]
    assert m.range_size.tolist() == [3, 2]


def test_four_leaves_two_with_one_code():
    # leaves 0 and 1 share the centroid (code 0; their indices order them), leaf 2 is the far end (1023), leaf 3 sits at 4 / 10 (409)
    mn, mx, ref = leaves_at([(0, 0, 0), (0, 0, 0), (10, 0, 0), (4, 0, 0)], [0.5, 2.0, 0.5, 0.5])
    m = lbvh_ref.build_from_leaves(mn, mx, ref)
    assert m.codes[0] == m.codes[1] == 0 and len(set(m.codes.tolist())) == 3
    assert (m.depth, m.n_wnodes) == (4, 3)
    assert children(m) == [[1, leaf(2)], [2, leaf(3)], [leaf(0), leaf(1)]]
    assert m.wnodes[1, :6].tolist() == [-2, -2, -2, 2, 2, 2] and m.wnodes[0, :6].tolist() == [-2, -2, -2, 4.5, 2, 2]
    assert m.wnodes[2, :12].tolist() == [-0.5] * 3 + [0.5] * 3 + [-2.0] * 3 + [2.0] * 3


def test_all_codes_equal_gives_the_radix_tree_of_the_indices():
    mn, mx, ref = leaves_at([(3, 3, 3)] * 5, [1, 2, 3, 4, 5])
    m = lbvh_ref.build_from_leaves(mn, mx, ref)
    assert not m.codes.any() and not m.extent.any()
    # indices 000 001 010 011 | 100, then 00x | 01x
    assert children(m) == [[1, leaf(4)], [2, 3], [leaf(0), leaf(1)], [leaf(2), leaf(3)]]
    assert (m.depth, m.range_size.tolist()) == (4, [5, 4, 2, 2])
    assert m.wnodes[0, :12].tolist() == [-1.0] * 3 + [7.0] * 3 + [-2.0] * 3 + [8.0] * 3


def test_clamp_and_signed_zero():
    # the largest centroid lands on 1024 and is clamped to 1023; a box face at -0 stays -0 through a union with +0
    mn, mx, ref = leaves_at([(0, 0, 0), (1, 1, 1)], [0.0, 0.0])
    mn[0, 1] = F(-0.0)
    m = lbvh_ref.build_from_leaves(mn, mx, ref)
    assert m.codes.tolist() == [0, (1 << 30) - 1]
    assert np.signbit(lbvh_ref.fmin32(np.array([0.0, -0.0], F), np.array([-0.0, 0.0], F))).all()
    assert not np.signbit(lbvh_ref.fmax32(np.array([0.0, -0.0], F), np.array([-0.0, 0.0], F))).any()


def test_refusals_are_errors():
    mn, mx, ref = leaves_at([(0, 0, 0)], [1.0])
    with pytest.raises(ValueError):
        lbvh_ref.build_from_leaves(mn, mx, ref)                                     # one leaf: build_image builds no hierarchy
    mn, mx, ref = leaves_at([(0, 0, 0), (5, 0, 0)], [1.0, 1.0])
    mx[1, 0] = np.inf
    with pytest.raises(ValueError):
        lbvh_ref.build_from_leaves(mn, mx, ref)                                     # a centroid is not finite


def walk(m):
    """The tree read back from the model's array alone, by a plain recursive walk: (visit order of the inner nodes, leaf words in
    left-first order, levels), checking on the way that each child box is the leaf's own or the union of the leaves below"""
    wu = m.wnodes.view(np.uint32)
    box_of = {int(r): (m.leaf_min[k], m.leaf_max[k]) for k, r in enumerate(m.leaf_refs)}
    order, leaves = [], []

    def below(ref, level):                   # -> (min, max, levels) of the subtree
        if ref & REF_LEAF:
            leaves.append(ref)
            return box_of[ref][0], box_of[ref][1], level
        order.append(ref)
        w, deepest = m.wnodes[ref], level
        lo, hi = [], []
        for c in range(2):
            cmn, cmx, d = below(int(wu[ref, 12 + c]), level + 1)
            assert np.array_equal(w[6 * c:6 * c + 3], cmn) and np.array_equal(w[6 * c + 3:6 * c + 6], cmx), f"node {ref} child {c}"
            lo.append(cmn); hi.append(cmx); deepest = max(deepest, d)
        return np.minimum(lo[0], lo[1]), np.maximum(hi[0], hi[1]), deepest

    _, _, levels = below(m.root_ref, 1)
    return order, leaves, levels


@pytest.mark.parametrize("name", ["cornell", "feature_box", "soup81"])
def test_model_is_a_sound_tree_on_real_scenes(scene_factory, name):
    sc = lbvh_ref.image_scene(name, scene_factory)
    m = lbvh_ref.build(sc)
    n = int((sc.nodes["triangle_count"] > 0).sum())
    assert m.wnodes.shape == (n - 1, 16) and m.n_wnodes == n - 1 and m.root_ref == 0
    order, leaves, levels = walk(m)
    assert order == list(range(n - 1)), "inner nodes are not numbered in left-first preorder"
    assert sorted(leaves) == sorted(m.leaf_refs.tolist()) and len(set(leaves)) == n, "a leaf is missing or appears twice"
    assert levels == m.depth
    # the leaves' words and boxes are the reference nodes' own
    lf = sc.nodes[sc.nodes["triangle_count"] > 0]
    assert np.array_equal(m.leaf_refs & np.uint32(0x03FFFFFF), lf["triangle_offset"]) and np.array_equal((m.leaf_refs >> 26) & 31, lf["triangle_count"] - 1)
    assert np.array_equal(m.leaf_min, lf["aabb_min"]) and np.array_equal(m.leaf_max, lf["aabb_max"])


def test_scene_list_covers_what_the_gpu_comparison_is_for(scene_factory):
    """From the model alone: among the scenes compared image for image there is a tree with two leaves of equal 30-bit code (but not
    all), one whose codes are all equal, one with an axis of zero extent, and the six exact leaf counts around the block of 256."""
    some_equal = all_equal = zero_axis = False
    counts = set()
    for name in lbvh_ref.SMALL_SCENES:
        sc = lbvh_ref.image_scene(name, scene_factory)
        m = lbvh_ref.build(sc)
        n, distinct = len(m.codes), len(np.unique(m.codes))
        assert n == int((sc.nodes["triangle_count"] > 0).sum()) == m.n_wnodes + 1
        some_equal |= 1 < distinct < n
        all_equal |= distinct == 1 and n > 2
        zero_axis |= bool((m.extent == 0).any() and (m.extent > 0).any())
        if name.startswith("row"):
            assert n == int(name[3:]), "the hand-written node array must give exactly that many leaves"
            counts.add(n)
    assert some_equal and all_equal and zero_axis
    assert counts == set(lbvh_ref.EDGE_LEAF_COUNTS) == {2, 3, 255, 256, 257, 513}
    assert set(lbvh_ref.IMAGE_SCENES) >= {"cornell", "cornell_spheres", "feature_box", "soup80", "soup81", "soup82", "soup83", "deep_chain",
                                          "grid_1m", "flat", "concentric"}


def test_mismatch_report_tells_a_box_word_from_a_child_word():
    mn, mx, ref = leaves_at([(0, 0, 0), (0, 0, 0), (10, 0, 0), (4, 0, 0)], [0.5, 2.0, 0.5, 0.5])
    m = lbvh_ref.build_from_leaves(mn, mx, ref)
    assert lbvh_ref.describe_mismatch(m, m.wnodes.copy()) is None
    assert "shape" in lbvh_ref.describe_mismatch(m, m.wnodes[:2])
    w = m.wnodes.copy()
    w[1, 4] = F(1.5)                                                # a box that lost a child's extent
    msg = lbvh_ref.describe_mismatch(m, w)
    assert "the same tree" in msg and "node 1 (3 leaves below it in the model), word 4, a box word" in msg and "child word:" not in msg
    w = m.wnodes.copy()
    w[2, 12:14] = w[2, [13, 12]]; w[2, 0:6], w[2, 6:12] = m.wnodes[2, 6:12], m.wnodes[2, 0:6]         # children swapped, boxes with them
    msg = lbvh_ref.describe_mismatch(m, w)
    assert "another tree" in msg and "node 2 (2 leaves below it in the model), word 12, a child word" in msg
