"""A numpy float32 model of the alpha cutouts (csrc/alpha.hip): the alpha lookup of a hit, the step past a hole, and the
two resolve loops run on top of a raw closest-hit probe. Every operation is the one float32 operation the kernel names, so the model
gives the device's bits; the texel itself is cross-checked against tests/texture_ref.py, which shares no code with either.

The constants of the step: eps = max(PT_EPS, 2^-18 * max(|p.x|, |p.y|, |p.z|)) with p = fma(d, t, o) the hit point; the next origin is
fma(d, eps, p); the distance travelled grows by step = t + eps (travelled' = travelled + step). The distance a ray that passed holes
reports for its last hit is the triangle test's t of that triangle from the ray's FIRST origin (what an unobstructed ray would report),
and travelled + t of the last leg only where that test rejects the hit.
"""
import numpy as np

import texture_ref
from ptmi import scenes
from scene_update_ref import fmaf

F = np.float32
PT_EPS = F(1e-6)
STEP_SCALE = F(2.0 ** -18)
DEFAULT_LAYERS = 4
NONE = 0xFFFFFFFF


# ---- the scene of the tests ---------------------------------------------------------------------------------------------------------
def checker(n_fences=1, phase=0):
    """alpha [fence, row, column]: 1 where row + column + fence + phase is even, else 0"""
    f, j, i = np.mgrid[0:n_fences, 0:scenes.FENCE_CELLS, 0:scenes.FENCE_CELLS]
    return ((f + j + i + phase) % 2 == 0).astype(np.float32)


def fence_scene(alpha=None, **kw):
    """scenes.cornell_fence, and the cutoff table that makes its fences' materials cutouts at 0.5"""
    sc = scenes.cornell_fence(alpha, **kw)
    cutoff = np.zeros(len(sc.mats), np.float32)
    cutoff[sc.info["fence_materials"]] = 0.5
    return sc, cutoff


# ---- the lookup ---------------------------------------------------------------------------------------------------------------------
def _f2u(f):
    """WGSL u32(f): truncating, saturating, NaN -> 0"""
    f = np.asarray(f, F)
    with np.errstate(invalid="ignore"):
        return np.where(f > 0, np.minimum(np.where(f > 0, f, 0).astype(np.float64), 4294967295.0), 0.0).astype(np.uint64)


def texel_of(scene, tri, u, v):
    """(ix, iy, mapped): the atlas texel the albedo lookup of each hit (triangle, u, v) reads, and whether its material has a map"""
    tri = np.asarray(tri, np.int64)
    u, v = np.asarray(u, F), np.asarray(v, F)
    T = scene.tris[tri]
    w = (F(1) - u) - v
    uvx = fmaf(T["uv2"][:, 0], v, fmaf(T["uv1"][:, 0], u, T["uv0"][:, 0] * w))
    uvy = fmaf(T["uv2"][:, 1], v, fmaf(T["uv1"][:, 1], u, T["uv0"][:, 1] * w))
    r = scene.mats[T["material_index"]]["albedo_map"]
    fx, fy = uvx - np.trunc(uvx), uvy - np.trunc(uvy)
    ax = r["x"].astype(F) + fx * r["w"].astype(F)
    ay = r["y"].astype(F) + fy * r["h"].astype(F)
    return _f2u(ax), _f2u(ay), (r["w"] != 0) & (r["h"] != 0)


def alpha_of(scene, tri, u, v):
    """the alpha of each hit as float32: the texel's fourth channel, 1 without a map, 0 outside the atlas or without an atlas"""
    ix, iy, mapped = texel_of(scene, tri, u, v)
    a = scene.atlas
    if a is None:
        tex = np.zeros(len(ix), F)
    else:
        H, W = a.shape[:2]
        inside = (ix < W) & (iy < H)
        tex = np.where(inside, a[np.minimum(iy, H - 1).astype(np.int64), np.minimum(ix, W - 1).astype(np.int64), 3].astype(F), F(0))
    return np.where(mapped, tex, F(1)).astype(F)


def is_hole(scene, cutoff, tri, u, v):
    """the MASK rule: the hit's material has cutoff > 0 and alpha < cutoff (a material index past the table: opaque)"""
    mi = scene.tris[np.asarray(tri, np.int64)]["material_index"].astype(np.int64)
    cutoff = np.asarray(cutoff, F)
    cut = np.where(mi < len(cutoff), cutoff[np.minimum(mi, len(cutoff) - 1)], F(0))
    return (cut > 0) & (alpha_of(scene, tri, u, v) < cut)


def texture_ref_texels(scene, tri, u, v):
    """what tests/texture_ref.py's float64 lookup says the albedo map's texel of one hit may be: (x candidates, y candidates)"""
    T = scene.tris[int(tri)]
    r = scene.mats[int(T["material_index"])]["albedo_map"]
    H, W = scene.atlas.shape[:2]
    bary = np.array([1.0 - float(u) - float(v), float(u), float(v)])
    uvs = np.array([T["uv0"], T["uv1"], T["uv2"]], np.float64)
    return (texture_ref._axis_indices(uvs[:, 0], bary, int(r["x"]), int(r["w"]), W),
            texture_ref._axis_indices(uvs[:, 1], bary, int(r["y"]), int(r["h"]), H))


# ---- the step -----------------------------------------------------------------------------------------------------------------------
def step(o, d, t):
    """past a hole at distance t of the rays (o, d): (next origins, step lengths)"""
    o, d, t = np.asarray(o, F), np.asarray(d, F), np.asarray(t, F)
    p = fmaf(d, t[:, None], o)
    eps = np.maximum(PT_EPS, STEP_SCALE * np.abs(p).max(axis=1)).astype(F)
    return fmaf(d, eps[:, None], p), (t + eps).astype(F)


# ---- the triangle test (csrc/pt_math.h tri_test) -------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([fmaf(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), fmaf(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])),
                     fmaf(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], 1).astype(F)


def _dot(a, b):
    return fmaf(a[:, 2], b[:, 2], fmaf(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))


def tri_t(scene, tri, o, d):
    """Moller-Trumbore as the kernels run it, operation for operation in float32: t (> 1e-6) of the rays (o, d) on the triangles
    `tri`, or -1"""
    T = scene.tris[np.asarray(tri, np.int64)]
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    v0 = T["v0"][:, :3].astype(F)
    e1, e2 = (T["v1"][:, :3] - v0).astype(F), (T["v2"][:, :3] - v0).astype(F)
    with np.errstate(all="ignore"):
        h = _cross(d, e2)
        a = _dot(e1, h)
        f = (F(1) / a).astype(F)
        sv = (o - v0).astype(F)
        u = f * _dot(sv, h)
        q = _cross(sv, e1)
        v = f * _dot(d, q)
        t = f * _dot(e2, q)
        reject = (np.abs(a) < PT_EPS) | (u < 0) | (u > 1) | (v < 0) | (u + v > 1)
        return np.where(~reject & (t > PT_EPS), t, F(-1)).astype(F)


def hit_t(scene, tri, o0, d, fallback):
    """the distance a ray that passed holes reports for its hit on `tri`: from its first origin o0, or `fallback` where that test rejects"""
    t = tri_t(scene, tri, o0, d)
    return np.where(t > 0, t, fallback).astype(F)


# ---- the loops, on a raw closest-hit probe ------------------------------------------------------------------------------------------
def resolve(intersect, scene, cutoff, o, d, max_layers=DEFAULT_LAYERS):
    """The path loop: intersect(o, d) -> (t, tri, u, v) is the raw probe (Context.debug_intersect). Returns (t along the given ray,
    triangle, layers) as ptmi_debug_alpha_intersect defines them."""
    o, d = np.asarray(o, F).reshape(-1, 3).copy(), np.asarray(d, F).reshape(-1, 3)
    o0 = o.copy()
    n = len(o)
    t_out, tri_out, layers = np.zeros(n, F), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    travelled = np.zeros(n, F)
    idx = np.arange(n)
    for r in range(max_layers + 1):
        if not len(idx):
            break
        t, tri, u, v = intersect(o[idx], d[idx])
        hit = ~(t < 0)
        hole = hit.copy()
        hole[hit] = is_hole(scene, cutoff, tri[hit], u[hit], v[hit])
        exhausted = hole & (r >= max_layers)
        go = hole & ~exhausted
        done = idx[~go]
        t_out[done] = t[~go]
        if r > 0:
            k = hit & ~go
            t_out[idx[k]] = hit_t(scene, tri[k], o0[idx[k]], d[idx[k]], travelled[idx[k]] + t[k])
        tri_out[done] = tri[~go]
        layers[done] = np.where(exhausted[~go], max_layers + 1, r)
        nxt = idx[go]
        o2, st = step(o[nxt], d[nxt], t[go])
        o[nxt] = o2
        travelled[nxt] = travelled[nxt] + st
        idx = nxt
    return t_out, tri_out, layers


def occluded(intersect, scene, cutoff, o, d, dist, max_layers=DEFAULT_LAYERS):
    """The shadow loop on the same probe: dist < 0 is a directional light (any hit that is there occludes), else a hit occludes when
    it is nearer than dist - 2e-6. Returns (occluded 0 / 1, layers) as ptmi_debug_alpha_occluded defines them."""
    o, d = np.asarray(o, F).reshape(-1, 3).copy(), np.asarray(d, F).reshape(-1, 3)
    o0 = o.copy()
    dist = np.asarray(dist, F)
    tlim_all = np.where(dist < 0, F(np.nan), dist - PT_EPS * F(2)).astype(F)
    n = len(o)
    occ, layers = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    travelled = np.zeros(n, F)
    idx = np.arange(n)
    for r in range(max_layers + 1):
        if not len(idx):
            break
        t, tri, u, v = intersect(o[idx], d[idx])
        hit = ~(t < 0)
        t_ray = t.copy()                                    # along the record's own ray
        if r > 0:
            t_ray[hit] = hit_t(scene, tri[hit], o0[idx[hit]], d[idx[hit]], travelled[idx[hit]] + t[hit])
        with np.errstate(invalid="ignore"):
            nearer = hit & ~(t_ray >= tlim_all[idx])
        hole = nearer.copy()
        hole[nearer] = is_hole(scene, cutoff, tri[nearer], u[nearer], v[nearer])
        exhausted = hole & (r >= max_layers)
        go = hole & ~exhausted
        done = idx[~go]
        occ[done] = nearer[~go]
        layers[done] = np.where(exhausted[~go], max_layers + 1, r)
        nxt = idx[go]
        o2, st = step(o[nxt], d[nxt], t[go])
        o[nxt] = o2
        travelled[nxt] = travelled[nxt] + st
        idx = nxt
    return occ, layers
