"""A plain model of ptmi_update_triangles (csrc/scene_update.hip; include/ptmi.h): numpy on the CPU, vectorised per level, no GPU and no
library call. From a traversal image as Context.read_image() / native.build_image() return it, the uploaded node array and NEW triangle
records it states the image a refit must leave: the topology (references, triangle order) stays, every box, triangle word and header
value is recomputed from the triangles.

  refit_nodes   the 48-byte reference nodes with tight boxes, bottom-up: leaf = min / max over the vertices of its triangle range,
                inner = union of its children (src/renderer/bvh.ts:14-28 stores exactly that for every node it builds)
  refit_image   leaves_used = 1 (and keep_reference_tree): leaf child = its range's tight box, inner child = union; tripos in original
                order. leaves_used = 2: unit boxes as csrc/fast_tree.hip pt_build_own_tree computes them (a, b, c, a + (b - a),
                a + (c - a); a sliver grown by its NEW reference leaf's box), pad / safe_origin from the largest coordinate, exact unions
                up the tree, every stored box padded with lower / upper, tripos in leaf order with the original index kept, the 16-bit
                grid of csrc/quantise.hip pt_quant_grid over the padded bounds and every child through wide_node.h pt_quantise_child
                (float32 fma restated exactly: product and sum in float64 with the rounding error carried, ties repaired)
  wobble / move_part / squash   the deformations the tests apply

Minima and maxima are exact, so only which of -0 / +0 a tie returns is open: boxes are compared by value, everything else by bits."""
import math
import time
from dataclasses import dataclass

import numpy as np

REF_LEAF = 0x80000000
REF_NONE = 0xFFFFFFFF
LEAF_OFF_BITS = 26
LEAF_OFF_MASK = (1 << LEAF_OFF_BITS) - 1
LEAF_MAX_TRIS = 32
OWN_PAD_LOG2 = -16                    # csrc/pt_box.h PT_OWN_PAD_LOG2
OWN_SLIVER = 16.0                     # csrc/fast_tree.h PT_OWN_SLIVER
F = np.float32
D = np.float64
FLT_MIN = np.finfo(F).tiny
INF32 = F(np.inf)


def _verts(tris):
    """[n, 3 vertices, 3 axes] float32"""
    return np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1).astype(F, copy=False)


def _range_boxes(tri_min, tri_max, first, count):
    """min / max over rows [first, first + count) of per-item boxes, for arrays of ranges (count >= 1)"""
    first, count = np.asarray(first, np.int64), np.asarray(count, np.int64)
    mn = np.full((len(first), 3), np.inf, F)
    mx = np.full((len(first), 3), -np.inf, F)
    for k in range(int(count.max()) if len(count) else 0):
        sel = np.flatnonzero(count > k)
        mn[sel] = np.minimum(mn[sel], tri_min[first[sel] + k])
        mx[sel] = np.maximum(mx[sel], tri_max[first[sel] + k])
    return mn, mx


# ---------------------------------------------------------------------------------------------------- the 48-byte reference nodes --
def node_levels(nodes):
    """the nodes a walk from node 0 reaches, as one index array per depth (root first)"""
    levels, front = [], np.array([0], np.int64)
    while len(front):
        assert len(levels) < 64, "reference tree deeper than 64 levels"
        levels.append(front)
        inner = front[nodes["triangle_count"][front] == 0]
        front = np.concatenate([nodes["left"][inner], nodes["right"][inner]]).astype(np.int64)
    return levels


def refit_nodes(nodes, tris):
    """a copy of `nodes` whose reachable boxes are tight over `tris`; everything else (links, ranges, padding words) as it was"""
    t0 = time.perf_counter()
    out = nodes.copy()
    if not len(nodes) or not len(tris):
        return out
    v = _verts(tris)
    tmin, tmax = v.min(axis=1), v.max(axis=1)
    for lvl in reversed(node_levels(nodes)):
        cnt = nodes["triangle_count"][lvl]
        leaf, inner = lvl[cnt > 0], lvl[cnt == 0]
        if len(leaf):
            mn, mx = _range_boxes(tmin, tmax, nodes["triangle_offset"][leaf], nodes["triangle_count"][leaf])
            out["aabb_min"][leaf], out["aabb_max"][leaf] = mn, mx
        if len(inner):
            l, r = nodes["left"][inner], nodes["right"][inner]
            out["aabb_min"][inner] = np.minimum(out["aabb_min"][l], out["aabb_min"][r])
            out["aabb_max"][inner] = np.maximum(out["aabb_max"][l], out["aabb_max"][r])
    print(f"refit_nodes: {len(nodes)} nodes, {time.perf_counter() - t0:.3f} s")
    return out


def leaf_boxes(nodes, n_tris):
    """[n_tris, 8] float32: per triangle (min.xyz, 0, max.xyz, 0) of the reachable leaf that lists it (zeros: no leaf does)"""
    lb = np.zeros((n_tris, 8), F)
    reach = np.concatenate(node_levels(nodes)) if len(nodes) else np.zeros(0, np.int64)
    leaf = reach[nodes["triangle_count"][reach] > 0]
    for k in range(int(nodes["triangle_count"][leaf].max()) if len(leaf) else 0):
        sel = leaf[nodes["triangle_count"][leaf] > k]
        at = nodes["triangle_offset"][sel].astype(np.int64) + k
        lb[at, 0:3], lb[at, 4:7] = nodes["aabb_min"][sel], nodes["aabb_max"][sel]
    return lb


# ------------------------------------------------------------------------------------------------------------- float32 arithmetic --
def fmaf(a, b, c):
    """float32 fma(a, b, c), correctly rounded once: the product of two float32 is exact in float64, the sum's rounding error is carried
    (TwoSum) and decides the one case where rounding twice goes wrong, a float64 sum that sits exactly between two float32 values"""
    a, b, c = np.asarray(a, F).astype(D), np.asarray(b, F).astype(D), np.asarray(c, F).astype(D)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    f = s.astype(F)
    d = s - f.astype(D)
    up, dn = np.nextafter(f, INF32), np.nextafter(f, -INF32)
    with np.errstate(invalid="ignore", over="ignore"):
        tie_up = (d > 0) & (d == (up.astype(D) - f.astype(D)) / 2) & (err > 0)
        tie_dn = (d < 0) & (-d == (f.astype(D) - dn.astype(D)) / 2) & (err < 0)
    return np.where(tie_up, up, np.where(tie_dn, dn, f)).astype(F)


def lower(x, pad):
    x = np.asarray(x, F)
    y = (x - F(pad)).astype(F)
    return np.where(y < x, y, np.nextafter(x, -INF32)).astype(F)


def upper(x, pad):
    x = np.asarray(x, F)
    y = (x + F(pad)).astype(F)
    return np.where(y > x, y, np.nextafter(x, INF32)).astype(F)


def box_area(lo, hi):
    """wide_node.h pt_box_area, float64"""
    e = np.asarray(hi, F).astype(D) - np.asarray(lo, F).astype(D)
    return 2.0 * (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0])


def slivers(tris):
    """csrc/fast_tree.h pt_own_sliver per triangle: float64 throughout, no contraction"""
    a, b, c = tris["v0"].astype(D), tris["v1"].astype(D), tris["v2"].astype(D)
    e1, e2, e3 = b - a, c - a, c - b
    x = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    y = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    z = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    l1 = e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1] + e1[:, 2] * e1[:, 2]
    l2 = e2[:, 0] * e2[:, 0] + e2[:, 1] * e2[:, 1] + e2[:, 2] * e2[:, 2]
    l3 = e3[:, 0] * e3[:, 0] + e3[:, 1] * e3[:, 1] + e3[:, 2] * e3[:, 2]
    longest = np.where(l1 > l2, np.where(l1 > l3, l1, l3), np.where(l2 > l3, l2, l3))
    return longest * longest > (OWN_SLIVER * OWN_SLIVER) * (x * x + y * y + z * z)


# -------------------------------------------------------------------------------------------------------- the 16-bit grid and qn --
def quant_grid(mn, mx):
    """csrc/quantise.hip pt_quant_grid: (origin [3], scale [3]) float32, or None where the bounds are not finite"""
    origin, scale = np.asarray(mn, F).copy(), np.zeros(3, F)
    for k in range(3):
        ext = float(D(mx[k]) - D(mn[k]))
        s = F(ext / 65535.0)
        if not np.isfinite(s):
            return None
        if ext > 0.0:
            if not s > 0:
                s = np.nextafter(F(0), INF32)
            guard = 0
            while fmaf(s, F(65535.0), origin[k]) < mx[k] and guard < 64:
                s, guard = np.nextafter(s, INF32), guard + 1
            if fmaf(s, F(65535.0), origin[k]) < mx[k]:
                return None
        scale[k] = s
    return origin, scale


def _plane_numbers(origin, scale, v, low):
    """wide_node.h pt_plane_lo (low) / pt_plane_hi for one axis: the quotient in float64 rounded outward, then moved outward while the
    decoded plane is on the wrong side of v"""
    v = np.asarray(v, F)
    if not scale > 0:
        return np.zeros(len(v), np.uint32)
    q = (v.astype(D) - D(origin)) / D(scale)
    q = np.floor(q) if low else np.ceil(q)
    u = np.clip(np.nan_to_num(q, nan=0.0), 0.0, 65535.0).astype(np.int64)
    for _ in range(70000):
        plane = fmaf(scale, u.astype(F), origin)
        move = (u > 0) & (plane > v) if low else (u < 65535) & (plane < v)
        if not move.any():
            break
        u = u - move if low else u + move
    return u.astype(np.uint32)


def quantise_children(origin, scale, lo, hi):
    """[n, 3] uint32 words (lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16) of the boxes lo / hi [n, 3]"""
    ql = [_plane_numbers(origin[k], scale[k], lo[:, k], True) for k in range(3)]
    qh = [_plane_numbers(origin[k], scale[k], hi[:, k], False) for k in range(3)]
    return np.stack([ql[0] | (ql[1] << 16), ql[2] | (qh[0] << 16), qh[1] | (qh[2] << 16)], axis=1).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ the image --
@dataclass
class Refit:
    wn: np.ndarray                    # [n_wnodes, 16] float32
    qn: np.ndarray                    # [n_wnodes, 8] uint32, or None (leaves_used = 1: dropped; an image that had none)
    tp: np.ndarray                    # [n_tris, 12] float32
    lb: np.ndarray                    # [n_triangles, 8] float32, or None
    root_min: np.ndarray
    root_max: np.ndarray
    pad: float
    safe_origin: float
    q_origin: np.ndarray              # the grid (None with qn None)
    q_scale: np.ndarray
    cost: float                       # sum of the child boxes' areas / the root box's area
    n_slivers: int


def wide_levels(refs, root):
    """the nodes of a wide-node image by depth (root first); refs: [n, 2] uint32 child references"""
    levels = []
    if root & REF_LEAF or not len(refs):
        return levels
    front = np.array([root], np.int64)
    seen = 0
    while len(front):
        assert len(levels) < 70
        levels.append(front)
        seen += len(front)
        ch = refs[front].reshape(-1)
        front = ch[(ch & REF_LEAF) == 0].astype(np.int64)
    assert seen == len(refs), "the image is not a tree over all of its nodes"
    return levels


def _ref_parts(ref):
    ref = np.asarray(ref, np.uint32)
    return (ref & LEAF_OFF_MASK).astype(np.int64), (((ref >> LEAF_OFF_BITS) & (LEAF_MAX_TRIS - 1)) + 1).astype(np.int64)


def _tripos(t, w_bits=None):
    tp = np.zeros((len(t), 12), F)
    tp[:, 0:3] = t["v0"]
    tp[:, 4:7] = (t["v1"] - t["v0"]).astype(F)
    tp[:, 8:11] = (t["v2"] - t["v0"]).astype(F)
    if w_bits is not None:
        tp[:, 3] = np.asarray(w_bits, np.uint32).view(F)
    return tp


def refit_image(info, wn, qn, tp, lb, tris, nodes=None):
    """The image (info, wn, qn, tp, lb) refitted over `tris`. nodes: the uploaded node array, needed for leaves_used = 2 (the new
    leaf boxes come from its leaf ranges; its boxes are not read)."""
    t0 = time.perf_counter()
    own = info.leaves_used == 2
    n = len(wn)
    refs = wn.view(np.uint32)[:, 12:14].copy() if n else np.zeros((0, 2), np.uint32)
    new_lb = None
    n_sl = 0
    if own:
        assert nodes is not None
        new_lb = leaf_boxes(refit_nodes(nodes, tris), len(tris))
        orig = tp.view(np.uint32)[:, 3].astype(np.int64)
        t = tris[orig]
        a, b, c = t["v0"].astype(F), t["v1"].astype(F), t["v2"].astype(F)
        b2, c2 = (a + (b - a).astype(F)).astype(F), (a + (c - a).astype(F)).astype(F)
        five = np.stack([a, b, c, b2, c2], axis=0)
        umin, umax = five.min(axis=0), five.max(axis=0)
        sl = slivers(t)
        n_sl = int(sl.sum())
        umin[sl] = np.minimum(umin[sl], new_lb[orig[sl], 0:3])
        umax[sl] = np.maximum(umax[sl], new_lb[orig[sl], 4:7])
        biggest = float(max(np.abs(umin).max(), np.abs(umax).max()))
        pad = max(F(math.ldexp(biggest, OWN_PAD_LOG2)), FLT_MIN)
        safe_origin = F(min(8.0 * biggest, 3.0e38))
        new_tp = _tripos(t, orig.astype(np.uint32))
        item_min, item_max = umin, umax
    else:
        v = _verts(tris)
        item_min, item_max = v.min(axis=1), v.max(axis=1)
        pad, safe_origin = F(0), F(info.safe_origin)
        new_tp = _tripos(tris)
    # exact child boxes, bottom-up
    exact_min, exact_max = np.zeros((n, 2, 3), F), np.zeros((n, 2, 3), F)
    for lvl in reversed(wide_levels(refs, info.root_ref)):
        for side in range(2):
            r = refs[lvl, side]
            is_leaf = (r & REF_LEAF) != 0
            lf, inn = lvl[is_leaf], lvl[~is_leaf]
            if len(lf):
                first, cnt = _ref_parts(r[is_leaf])
                exact_min[lf, side], exact_max[lf, side] = _range_boxes(item_min, item_max, first, cnt)
            if len(inn):
                ch = r[~is_leaf].astype(np.int64)
                exact_min[inn, side] = exact_min[ch].min(axis=1)
                exact_max[inn, side] = exact_max[ch].max(axis=1)
    if n and not info.root_ref & REF_LEAF:
        root_min, root_max = exact_min[info.root_ref].min(axis=0), exact_max[info.root_ref].max(axis=0)
    elif own:
        root_min, root_max = item_min.min(axis=0), item_max.max(axis=0)
    else:
        first, cnt = _ref_parts(np.array([info.root_ref], np.uint32))
        mn, mx = _range_boxes(item_min, item_max, first, cnt)
        root_min, root_max = mn[0], mx[0]
    if own:
        exact_min, exact_max = lower(exact_min, pad), upper(exact_max, pad)
        root_min, root_max = lower(root_min, pad), upper(root_max, pad)
    new_wn = wn.copy()
    if n:
        new_wn[:, 0:3], new_wn[:, 3:6] = exact_min[:, 0], exact_max[:, 0]
        new_wn[:, 6:9], new_wn[:, 9:12] = exact_min[:, 1], exact_max[:, 1]
    # the quantised nodes: kept by own leaves only
    new_qn = q_origin = q_scale = None
    if own and qn is not None and n:
        grid = quant_grid(exact_min.reshape(-1, 3).min(axis=0), exact_max.reshape(-1, 3).max(axis=0))
        if grid is not None:
            q_origin, q_scale = grid
            qnum = np.full(n, -1, np.int64)
            qnum[info.root_ref] = 0                                   # the root stays node 0; a child's number is its reference in qn
            for lvl in wide_levels(refs, info.root_ref):
                for side in range(2):
                    r = refs[lvl, side]
                    inner = (r & REF_LEAF) == 0
                    qnum[r[inner].astype(np.int64)] = qn[qnum[lvl[inner]], 4 * side + 3]
            assert sorted(qnum.tolist()) == list(range(n))
            new_qn = qn.copy()
            for side in range(2):
                new_qn[qnum, 4 * side:4 * side + 3] = quantise_children(q_origin, q_scale, exact_min[:, side], exact_max[:, side])
    cost = _cost(new_wn, root_min, root_max)
    print(f"refit_image: {n} nodes, {len(new_tp)} triangle images, {time.perf_counter() - t0:.3f} s")
    return Refit(new_wn, new_qn, new_tp, new_lb, root_min, root_max, float(pad), float(safe_origin), q_origin, q_scale, cost, n_sl)


def _cost(wn, root_min, root_max):
    if not len(wn):
        return 0.0
    area = float(box_area(np.asarray(root_min, F), np.asarray(root_max, F)))
    boxes = box_area(wn[:, [0, 1, 2, 6, 7, 8]].reshape(-1, 2, 3), wn[:, [3, 4, 5, 9, 10, 11]].reshape(-1, 2, 3))
    return float(boxes.sum() / area) if area > 0.0 else 0.0


def image_cost(info, wn):
    """the cost of an image as it stands (include/ptmi.h ptmi_scene_update_status), float64"""
    return _cost(wn, np.array(info.root_min, F), np.array(info.root_max, F))


# ------------------------------------------------------------------------------------------------------------ deformations --
def wobble(tris, amp):
    """every vertex moved by amp * a smooth function of its own position: vertices that coincide keep coinciding"""
    out = tris.copy()
    for f in ("v0", "v1", "v2"):
        p = tris[f].astype(D)
        d = np.stack([np.sin(3.1 * p[:, 1] + 1.7 * p[:, 2] + 0.3), np.sin(2.3 * p[:, 2] + 2.9 * p[:, 0] + 1.1),
                      np.sin(3.7 * p[:, 0] + 1.3 * p[:, 1] + 2.0)], axis=1)
        out[f] = (p + amp * d).astype(F)
    return out


def move_part(tris, sel, rot, shift):
    """the triangles `sel` (a mask or indices) rotated by the 3 x 3 matrix rot about their centroid and shifted; normals rotate along"""
    out = tris.copy()
    rot, shift = np.asarray(rot, D), np.asarray(shift, D)
    part = tris[sel]
    centre = np.concatenate([part["v0"], part["v1"], part["v2"]]).astype(D).mean(axis=0)
    for f in ("v0", "v1", "v2"):
        part[f] = ((part[f].astype(D) - centre) @ rot.T + centre + shift).astype(F)
    for f in ("n0", "n1", "n2"):
        part[f] = (part[f].astype(D) @ rot.T).astype(F)
    out[sel] = part
    return out


def squash(tris, sel, ratio=1e-3):
    """v2 of the triangles `sel` pulled towards the line through v0 and v1 until `ratio` of its distance is left: ordinary triangles
    become slivers (csrc/fast_tree.h pt_own_sliver)"""
    out = tris.copy()
    part = tris[sel]
    a, b, c = part["v0"].astype(D), part["v1"].astype(D), part["v2"].astype(D)
    e = b - a
    l2 = np.maximum((e * e).sum(axis=1, keepdims=True), 1e-300)
    foot = a + e * (((c - a) * e).sum(axis=1, keepdims=True) / l2)
    part["v2"] = (foot + ratio * (c - foot)).astype(F)
    out[sel] = part
    return out


def rot_y(angle):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


DEFORMATIONS = ("wobble", "move", "squash")


def deformed(tris, kind):
    """the deformation `kind` of the tests, sized by the scene's extent"""
    v = _verts(tris).reshape(-1, 3).astype(D)
    ext = float((v.max(axis=0) - v.min(axis=0)).max())
    n = len(tris)
    if kind == "wobble":
        return wobble(tris, 0.03 * ext)
    if kind == "move":
        return move_part(tris, np.arange(n // 3, max(n // 3 + 1, n // 2)), rot_y(0.6), (0.1 * ext, 0.05 * ext, -0.02 * ext))
    if kind == "squash":
        return squash(tris, np.arange(0, n, 3), 1e-3)
    raise ValueError(kind)
