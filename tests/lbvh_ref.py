"""A plain model of the device LBVH builder (csrc/gpu_tree.hip; ptmi_options.leaves = 1, tree_builder = 2, keep_reference_tree = 0):
numpy on the CPU, no GPU and no library call. From a scene's triangles and reference nodes it states the one value the builder's
`wnodes` array, root reference and depth can have, so that Context.read_image() after a device build can be compared word for word.

Why one value: the sort keys are unique (30-bit Morton code of the leaf's centroid above the leaf's index), the binary radix tree over
sorted unique keys is unique, inner boxes are exact minima / maxima, the host renumbers in left-first preorder, and the library is
compiled without contraction or fast-math, so numpy's float32 arithmetic restates its float32 arithmetic operation for operation.

What is restated from the code, and what is deliberately done another way:
  leaves   as build_image (csrc/scene_image.hip) collects them: the reachable reference nodes with triangle_count > 0 in node-array order
  keys     the host prologue of pt_build_fast_tree_gpu and k_morton, same float32 operations in the same order; the 10 -> 30 bit spread
           is a bit-by-bit loop here, not the multiply-and-mask of expand10
  tree     NOT Karras' per-node search: top-down, a range of sorted keys splits where the highest bit in which its first and last key
           differ changes value (one searchsorted per level); the preorder index of a node follows from the sizes of the ranges
  boxes    bottom-up, level by level, with a minimum / maximum that orders -0 below +0 as the device's v_min_f32 / v_max_f32 do
"""
from dataclasses import dataclass

import numpy as np

from ptmi import layout, scene_host, scenes

# csrc/pt_device.h, copied by value: PT_REF_LEAF, PT_LEAF_OFF_BITS, PT_LEAF_MAX_TRIS (a leaf reference is
# PT_REF_LEAF | (count - 1) << PT_LEAF_OFF_BITS | first triangle: leaf_ref, csrc/scene_image.hip)
REF_LEAF = 0x80000000
LEAF_OFF_BITS = 26
LEAF_MAX_TRIS = 32
MAX_LEVELS = 60                       # pt_build_fast_tree_gpu refuses a deeper tree (the host builder then builds)

F = np.float32


@dataclass
class Model:
    wnodes: np.ndarray               # [n_leaves - 1, 16] float32: what read_image() returns as wnodes; compare .view(uint32)
    root_ref: int
    depth: int                       # levels, the leaves included
    n_wnodes: int
    range_size: np.ndarray           # [n_leaves - 1] leaves below each inner node (preorder index)
    codes: np.ndarray                # [n_leaves] the 30-bit Morton code of each leaf, in leaf order
    extent: np.ndarray               # [3] float32 extent of the centroid bounds (0: that axis does not enter the codes)
    leaf_refs: np.ndarray            # [n_leaves] uint32 reference words, in leaf order
    leaf_min: np.ndarray             # [n_leaves, 3] float32
    leaf_max: np.ndarray


# ------------------------------------------------------------------------------------------------------------------ leaves --
def reachable(nodes):
    """mask of the nodes a left-first walk from node 0 reaches (level by level; the tree is assumed to be one)"""
    seen = np.zeros(len(nodes), bool)
    front = np.array([0], np.int64)
    for _ in range(64):
        if not len(front):
            return seen
        assert not seen[front].any() and len(np.unique(front)) == len(front), "a node is reachable twice"
        seen[front] = True
        inner = front[nodes["triangle_count"][front] == 0]
        front = np.concatenate([nodes["left"][inner], nodes["right"][inner]]).astype(np.int64)
    raise ValueError("reference tree deeper than 64 levels")


def scene_leaves(nodes):
    """(min [n, 3], max [n, 3], reference word [n]) of the leaves the builder is given, in its order"""
    seen = reachable(nodes)
    inner = np.flatnonzero(seen & (nodes["triangle_count"] == 0))
    # build_image only rebuilds a hierarchy over a nested tree with finite boxes: say so instead of modelling another path
    assert np.isfinite(nodes["aabb_min"][seen]).all() and np.isfinite(nodes["aabb_max"][seen]).all(), "non-finite box: no rebuild"
    for side in ("left", "right"):
        ch = nodes[side][inner]
        assert (nodes["aabb_min"][ch] >= nodes["aabb_min"][inner]).all() and (nodes["aabb_max"][ch] <= nodes["aabb_max"][inner]).all(), \
            "reference tree is not nested: no rebuild"
    leaf = np.flatnonzero(seen & (nodes["triangle_count"] > 0))
    cnt = nodes["triangle_count"][leaf].astype(np.uint32)
    assert (cnt <= LEAF_MAX_TRIS).all()
    ref = np.uint32(REF_LEAF) | ((cnt - np.uint32(1)) << np.uint32(LEAF_OFF_BITS)) | nodes["triangle_offset"][leaf].astype(np.uint32)
    return (np.ascontiguousarray(nodes["aabb_min"][leaf], F), np.ascontiguousarray(nodes["aabb_max"][leaf], F), ref.astype(np.uint32))


# -------------------------------------------------------------------------------------------------------------------- keys --
def spread10(v):
    """10 bits -> every third bit (bit b of v becomes bit 3 b), one bit at a time"""
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_codes(mn, mx):
    """(30-bit codes [n] uint64, extent [3] float32) — float32 throughout, one rounding per operation as the library's build flags
    (-ffp-contract=off -fno-fast-math) leave it"""
    half = F(0.5)
    c = half * mn + half * mx                                   # two products, one sum
    if not np.isfinite(c).all():
        raise ValueError("a centroid is not finite: the device builder refuses")
    lo, hi = c.min(axis=0), c.max(axis=0)
    e = (hi - lo).astype(F)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        r = (F(1.0) / e).astype(F)
        inv = np.where((e > 0) & np.isfinite(r), r, F(0.0)).astype(F)
        v = ((c - lo).astype(F) * inv).astype(F)
        v = (v * F(1024.0)).astype(F)
    q = np.where(v < 0, F(0.0), np.where(v > F(1023.0), F(1023.0), v))      # NaN passes both comparisons ...
    q = np.where(np.isnan(q), F(0.0), q).astype(np.uint64)                    # ... and converts to 0; the rest truncates
    return (spread10(q[:, 0]) << np.uint64(2)) | (spread10(q[:, 1]) << np.uint64(1)) | spread10(q[:, 2]), e


# ------------------------------------------------------------------------------------------------------------------- boxes --
def fmin32(a, b):
    """minimum of finite float32 with -0 below +0 (v_min_f32; fminf of equal zeros of opposite sign is otherwise unspecified)"""
    return np.where((a < b) | ((a == b) & np.signbit(a)), a, b)


def fmax32(a, b):
    return np.where((a > b) | ((a == b) & ~np.signbit(a)), a, b)


def top_bit(x):
    """index of the highest set bit of each (non-zero) uint64"""
    x = x.copy()
    p = np.zeros(len(x), np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> np.uint64(s)) != 0
        p[big] += np.uint64(s)
        x[big] >>= np.uint64(s)
    return p


# -------------------------------------------------------------------------------------------------------------------- tree --
def build_from_leaves(mn, mx, ref):
    n = len(ref)
    if n < 2:
        raise ValueError("fewer than two leaves: no hierarchy is built")
    codes, extent = morton_codes(mn, mx)
    keys = np.sort((codes << np.uint64(32)) | np.arange(n, dtype=np.uint64))
    order = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)                 # sorted position -> leaf
    smn, smx, sref = mn[order], mx[order], ref[order]

    # top-down: one pass per level over the inner nodes of that level (first, last sorted position; preorder index)
    levels = []
    a, b, idx = np.array([0], np.int64), np.array([n - 1], np.int64), np.array([0], np.int64)
    while len(a):
        if len(levels) + 2 > MAX_LEVELS:
            raise ValueError("more than %d levels: the device builder refuses" % MAX_LEVELS)
        p = top_bit(keys[a] ^ keys[b])
        m = np.searchsorted(keys, ((keys[a] >> p) | np.uint64(1)) << p, side="left").astype(np.int64)   # first key with bit p set
        assert ((a < m) & (m <= b)).all()
        l_inner, r_inner = m - 1 > a, b > m
        l_idx, r_idx = idx + 1, idx + 1 + (m - 1 - a)            # a subtree over k leaves has k - 1 inner nodes, left subtree first
        levels.append((a, b, m, idx, l_inner, r_inner, l_idx, r_idx))
        a, b, idx = (np.concatenate([a[l_inner], m[r_inner]]), np.concatenate([(m - 1)[l_inner], b[r_inner]]),
                     np.concatenate([l_idx[l_inner], r_idx[r_inner]]))

    w = np.zeros((n - 1, 16), F)
    wu = w.view(np.uint32)
    nmin, nmax = np.zeros((n - 1, 3), F), np.zeros((n - 1, 3), F)
    size = np.zeros(n - 1, np.int64)
    for a, b, m, idx, l_inner, r_inner, l_idx, r_idx in reversed(levels):
        li, ri = np.where(l_inner, l_idx, 0), np.where(r_inner, r_idx, 0)
        lmn = np.where(l_inner[:, None], nmin[li], smn[a]); lmx = np.where(l_inner[:, None], nmax[li], smx[a])
        rmn = np.where(r_inner[:, None], nmin[ri], smn[b]); rmx = np.where(r_inner[:, None], nmax[ri], smx[b])
        w[idx, 0:3], w[idx, 3:6], w[idx, 6:9], w[idx, 9:12] = lmn, lmx, rmn, rmx
        wu[idx, 12] = np.where(l_inner, l_idx.astype(np.uint32), sref[a])
        wu[idx, 13] = np.where(r_inner, r_idx.astype(np.uint32), sref[b])
        nmin[idx], nmax[idx] = fmin32(lmn, rmn), fmax32(lmx, rmx)
        size[idx] = b - a + 1
    return Model(w, 0, len(levels) + 1, n - 1, size, codes, extent, ref, mn, mx)


def build(sc):
    """The model for a scene as ptmi.scenes makes them (sc.tris is only counted: the leaves carry their boxes)"""
    mn, mx, ref = scene_leaves(sc.nodes)
    first, cnt = ref & np.uint32((1 << LEAF_OFF_BITS) - 1), ((ref >> np.uint32(LEAF_OFF_BITS)) & np.uint32(LEAF_MAX_TRIS - 1)) + 1
    assert (first.astype(np.int64) + cnt <= len(sc.tris)).all()
    return build_from_leaves(mn, mx, ref)


def describe_mismatch(model, wn):
    """None when wn equals the model's array word for word; else a message that names the first differing node, whether it differs in
    a child word or only in box words, and how many leaves lie below it in the model. A tree that differs in box words alone is what a
    lost update in the bottom-up fit looks like (it may change from run to run); a child word is a decision of the builder (stable),
    and the box words above it then differ as a consequence — so a child word is named whenever one differs."""
    got, want = np.ascontiguousarray(wn, F).view(np.uint32), model.wnodes.view(np.uint32)
    if got.shape != want.shape:
        return "wnodes has shape %s, the model %s" % (got.shape, want.shape)
    bad = got != want
    if not bad.any():
        return None

    def first(cols, kind):
        node = int(np.flatnonzero(bad[:, cols].any(axis=1))[0])
        word = int(np.flatnonzero(bad[node, cols])[0]) + cols.start
        return "node %d (%d leaves below it in the model), word %d, a %s: device 0x%08x, model 0x%08x" % (
            node, model.range_size[node], word, kind, got[node, word], want[node, word])

    box, child, pad = slice(0, 12), slice(12, 14), slice(14, 16)
    n_box, n_child = int(bad[:, box].sum()), int(bad[:, child].sum())
    if n_child:
        verdict = "another tree (a decision of the builder: stable from run to run); first " + first(child, "child word")
        if n_box:
            verdict += "; first differing box word: " + first(box, "box word")
    elif n_box:
        verdict = "the same tree with other boxes (an update lost in the bottom-up fit? may change from run to run); first " + first(box, "box word")
    else:
        verdict = "padding words are not zero; first " + first(pad, "padding word")
    return "%d of %d nodes differ, in %d child words and %d box words: %s" % (bad.any(axis=1).sum(), len(want), n_child, n_box, verdict)


# ------------------------------------------------------------------------------------------------------------------ scenes --
def quad_leaf_scene(name, quads):
    """One leaf per quad (4 corners each), the node array written by hand: a balanced tree over the quads in their order, node 0 the
    root, children after their parent, exact boxes. The reference builder would cut leaves of up to four triangles where it likes;
    here the leaf count is the quad count."""
    tris = np.ascontiguousarray(np.concatenate([scenes._quad(*q, np.cross(np.subtract(q[1], q[0]), np.subtract(q[2], q[0])), 0)
                                                for q in quads]))
    v = np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1).reshape(len(quads), 6, 3)
    qmn, qmx = v.min(axis=1), v.max(axis=1)
    nodes = np.zeros(2 * len(quads) - 1, layout.BVH_NODE)
    used, depth = 0, 0

    def make(a, b, level):                      # quads [a, b)
        nonlocal used, depth
        i = used
        used += 1
        depth = max(depth, level)
        nodes[i]["aabb_min"], nodes[i]["aabb_max"] = qmn[a:b].min(axis=0), qmx[a:b].max(axis=0)
        if b - a == 1:
            nodes[i]["triangle_offset"], nodes[i]["triangle_count"] = 2 * a, 2
        else:
            mid = (a + b + 1) // 2
            nodes[i]["left"] = make(a, mid, level + 1)
            nodes[i]["right"] = make(mid, b, level + 1)
        return i

    make(0, len(quads), 1)
    assert used == len(nodes)
    mats = np.array([scenes._material()], layout.MATERIAL)
    return scenes.Scene(name, tris, mats, nodes, scene_host.emissive_lights(tris, mats), None, depth)


def row_scene(n_leaves):
    """n_leaves well-separated unit quads in a row along x, stepping in y and z as well so that every axis enters the codes"""
    quads = []
    for i in range(n_leaves):
        x, y, z = 3.0 * i, 0.75 * (i % 7), 1.25 * (i % 5)
        quads.append(((x, y, z), (x + 1, y, z), (x + 1, y, z + 1), (x, y, z + 1)))
    return quad_leaf_scene("row%d" % n_leaves, quads)


def concentric_scene(n_leaves=41):
    """Quads of growing size around one point, in the three coordinate planes in turn: every leaf box is symmetric about the origin,
    so every centroid is exactly (0, 0, 0), every extent 0, and all 30 code bits are equal — the index bits alone decide the tree."""
    quads = []
    for i in range(n_leaves):
        s = 0.25 * (i + 1)
        c = [(-s, -s), (s, -s), (s, s), (-s, s)]
        quads.append(tuple(tuple(np.insert(np.array(p, np.float64), i % 3, 0.0)) for p in c))
    return quad_leaf_scene("concentric", quads)


def flat_scene():
    """All triangles in the plane y = 0 (tests/test_traversal_image.py::test_flat_scene_quantises_with_a_zero_scale): the centroid
    bounds have no extent in y, the builder's inverse extent is 0 there"""
    t = scenes._quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0), 0)
    parts = []
    for i in range(6):
        q = t.copy()
        for k in ("v0", "v1", "v2"):
            q[k][:, 0] += 3.0 * i
        parts.append(q)
    return scenes._finish("flat", parts, [scenes._material()])


EDGE_LEAF_COUNTS = (2, 3, 255, 256, 257, 513)                # around the builder's block of 256 threads: n leaves, n - 1 inner nodes
SMALL_SCENES = ("cornell", "cornell_spheres", "feature_box", "soup80", "soup81", "soup82", "soup83", "deep_chain") \
    + tuple("row%d" % n for n in EDGE_LEAF_COUNTS) + ("flat", "concentric")
# what tests/test_gpu_tree_builder.py compares image for image. grid_320: the construction of grid_1m at 203 532 triangles, 66 164 leaves
# (more than 65 536: beyond 16-bit indices and 256 blocks of the builder's kernels)
IMAGE_SCENES = SMALL_SCENES + ("grid_320", "grid_1m")
_made = {}


def image_scene(name, make=scenes.make):
    """The scene of that name in IMAGE_SCENES; `make` builds the named scenes of ptmi.scenes (the suite's cached factory)"""
    if name.startswith("soup") or name.startswith("row") or name in ("flat", "concentric"):
        if name not in _made:
            _made[name] = (scenes.random_soup(int(name[4:])) if name.startswith("soup") else row_scene(int(name[3:])) if name.startswith("row")
                           else flat_scene() if name == "flat" else concentric_scene())
        return _made[name]
    if name.startswith("grid_") and name != "grid_1m":
        if name not in _made:
            _made[name] = scenes.grid_1m(n=int(name[5:]))
        return _made[name]
    return make(name)
