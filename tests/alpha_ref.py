"""A numpy float32 model of the alpha cutouts (csrc/alpha.hip): the alpha lookup of a hit, the step past a hole, and the
two resolve loops run on top of a raw closest-hit probe. Every operation is the one float32 operation the kernel names, so the model
gives the device's bits; the texel itself is cross-checked against tests/texture_ref.py, which shares no code with either.

The constants of the step: eps = max(PT_EPS, 2^-18 * max(|p.x|, |p.y|, |p.z|)) with p = fma(d, t, o) the hit point; the next origin is
fma(d, eps, p); the distance travelled grows by step = t + eps (travelled' = travelled + step). The distance a ray that passed holes
reports for its last hit is the triangle test's t of that triangle from the ray's FIRST origin (what an unobstructed ray would report),
and travelled + t of the last leg only where that test rejects the hit.

Below the loops: the ghost scene (every hole triangle collapsed to a point, nothing else moved), the replay of the loops on every ray of
the oracle's render of it, and the case table tests/test_alpha_replay_host.py and tests/test_gpu_alpha_per_sample.py share.
"""
import dataclasses
import types

import numpy as np

import texture_ref
from ptmi import layout, scenes
from scene_update_ref import fmaf, refit_nodes

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


# ---- the ghost scene: a hole is an absent triangle, sample for sample ----------------------------------------------
def ghost(scene, cutoff, at="v0"):
    """(the ghost of `scene` under the table `cutoff`, the hole mask over its triangles): a copy with the same triangle order, nodes,
    materials, lights and atlas in which every triangle whose albedo texel is below its material's cutoff is collapsed to the point
    `at` (one of its own corners), so the triangle test rejects it (|a| < PT_EPS) while the old boxes still enclose it; light order and
    triangle ids do not move. Asserts that every triangle of a cutout material reads one texel: the same verdict at its three corners
    and at its centroid."""
    cutoff = np.asarray(cutoff, F)
    mi = scene.tris["material_index"].astype(np.int64)
    cut = np.flatnonzero((mi < len(cutoff)) & (cutoff[np.minimum(mi, len(cutoff) - 1)] > 0))
    third = F(1.0 / 3.0)
    verdicts = [is_hole(scene, cutoff, cut, np.full(len(cut), u, F), np.full(len(cut), v, F))
                for u, v in ((0, 0), (1, 0), (0, 1), (third, third))]
    for k in verdicts[1:]:
        assert np.array_equal(k, verdicts[0]), "a triangle of a cutout material reads more than one texel"
    hole = np.zeros(len(scene.tris), bool)
    hole[cut] = verdicts[0]
    tris = scene.tris.copy()
    point = scene.tris[at][hole].copy()
    for k in ("v0", "v1", "v2"):
        tris[k][hole] = point
    return dataclasses.replace(scene, tris=tris), hole


def replay(oracle, cut, cutoff, ghost, cam, frames, rows, max_bounces, do_mis, max_layers=DEFAULT_LAYERS):
    """The model's two loops, over the oracle's closest-hit probe on the cutout scene `cut`, replayed on every ray the oracle's render
    of the ghost scene traces (rows = (y0, y1); Oracle.render_tap in tracing order). A closest-hit ray disagrees when the bits of t or the
    triangle differ from what the tap recorded for the ghost scene (two misses agree), a shadow ray when the verdict does. No kernel has
    a part in any of it. Returns a namespace:
      n_rays, n_closest, n_shadow       the rays replayed
      disagreeing_closest / _shadow     how many disagree
      path_passes, shadow_passes        holes passed: the sum of `layers` over the closest-hit / the shadow rays
      through_holes                     rays that passed at least one hole
      exhausted                         rays still on a hole after max_layers
      shadow_lit                        shadow rays whose sample lies on the lit side of its surface, cos > 0: the ones `shade` leaves a
                                        record for (a sample with ndl = 0 has contribution zero and is counted, not traced)
      shadow_passes_lit                 the holes those passed: what ptmi_alpha_status.shadow_passes counts
      shadow_grazing                    shadow rays with |cos| < 1e-5, whose side float64 and the kernels' float32 may see differently"""
    y0, y1 = rows
    W, H = int(cam["width"]), int(cam["height"])
    n_paths = ((y1 or H) - y0) * W * frames
    rec = oracle.render_tap(ghost, cam, frames, y0, y1, max(n_paths * (2 * max_bounces + 1), 1), max_bounces, do_mis, threads=1)
    o, d, dist = rec[:, 0:3], rec[:, 3:6], rec[:, 6]
    want_t, want_tri = rec[:, 7], np.ascontiguousarray(rec[:, 8]).view(np.uint32)
    probe = lambda oo, dd: oracle.intersect(cut, oo, dd)[:4]
    c, s = np.flatnonzero(dist == 0), np.flatnonzero(dist != 0)
    t, tri, layers = resolve(probe, cut, cutoff, o[c], d[c], max_layers)
    both_miss = (t < 0) & (want_t[c] < 0)
    same = (np.ascontiguousarray(t).view(np.uint32) == np.ascontiguousarray(want_t[c]).view(np.uint32)) & (tri == want_tri[c])
    occ, slayers = occluded(probe, cut, cutoff, o[s], d[s], dist[s], max_layers)
    wt, ds = want_t[s], dist[s]
    with np.errstate(invalid="ignore"):
        want_occ = np.where(ds < 0, wt > 0, (wt > 0) & (wt < (ds - PT_EPS * F(2)).astype(F)))
    # the side of its surface a light sample lies on: the shadow ray stands right behind the ray whose hit it starts from
    cos = np.zeros(len(s))
    if len(s):
        assert s[0] > 0 and np.all(dist[s - 1] == 0) and np.all(want_t[s - 1] > 0)
        pt, ptri, pu, pv = oracle.intersect(ghost, o[s - 1], d[s - 1])[:4]
        assert np.array_equal(ptri, want_tri[s - 1])
        T = ghost.tris[ptri.astype(np.int64)]
        u, v = pu.astype(np.float64)[:, None], pv.astype(np.float64)[:, None]
        w = (F(1) - pu - pv).astype(np.float64)[:, None]
        n = T["n0"][:, :3] * w + T["n1"][:, :3] * u + T["n2"][:, :3] * v
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        cos = (n * d[s].astype(np.float64)).sum(axis=1)
    lit = cos > 0
    return types.SimpleNamespace(
        n_rays=len(rec), n_closest=len(c), n_shadow=len(s),
        disagreeing_closest=int((~(same | both_miss)).sum()), disagreeing_shadow=int((occ.astype(bool) != want_occ).sum()),
        path_passes=int(np.minimum(layers, max_layers).sum()), shadow_passes=int(np.minimum(slayers, max_layers).sum()),
        through_holes=int((layers > 0).sum() + (slayers > 0).sum()),
        exhausted=int((layers > max_layers).sum() + (slayers > max_layers).sum()),
        shadow_lit=int(lit.sum()), shadow_passes_lit=int(np.minimum(slayers, max_layers)[lit].sum()),
        shadow_grazing=int((np.abs(cos) < 1e-5).sum()))


# ---- the cases of the per-sample comparison: tests/test_alpha_replay_host.py (the licence) and tests/test_gpu_alpha_per_sample.py -----
STRIPES = (np.add.outer(np.arange(8), np.arange(8)) % 3 != 1)[None]        # holes: two cells of every three, in diagonal stripes
SIZE, FRAMES = (96, 64), 8
TILE = dict(width=100, height=64, rows=(5, 42))           # 37 rows of 100: the bounce-0 queue ends in a partial wave, whole or frame by frame
FAR = dict(offset=(200.0, 200.0, 200.0), size=(64, 48), frames=4)
FENCE_EDIT = dict(dz=-0.07, tilt=0.05)


def case_scene(name, offset=(0.0, 0.0, 0.0)):
    """(the cutout scene, its cutoff table, the number of fences) of the case scenes 'stripes' and 'checker2'"""
    if name == "stripes":
        return fence_scene(1.0 - STRIPES, z=(0.4,), offset=offset) + (1,)
    assert name == "checker2"
    return fence_scene(checker(2), z=(0.4, 0.3), offset=offset) + (2,)


def case_camera(size=SIZE, offset=(0.0, 0.0, 0.0)):
    return layout.make_camera(size[0], size[1], position=tuple(F((0.0, 1.0, 2.8)) + F(offset)))


def edited_fence(scene, offset=(0.0, 0.0, 0.0)):
    """the edit of the triangle-update tests: (the records of the whole scene with the fences moved by dz, tilted by tilt * x in z (x
    from the scene's own offset) and u mirrored to 1 - u; the scene a fresh upload gets, those records with the nodes refitted over the
    same topology)"""
    moved = scene.tris.copy()
    fence = np.isin(moved["material_index"], scene.info["fence_materials"])
    for k in ("v0", "v1", "v2"):
        v = moved[k][fence]
        v[:, 2] = v[:, 2] + F(FENCE_EDIT["dz"]) + F(FENCE_EDIT["tilt"]) * (v[:, 0] - F(offset[0]))
        moved[k][fence] = v
    for k in ("uv0", "uv1", "uv2"):
        uv = moved[k][fence]
        uv[:, 0] = F(1) - uv[:, 0]
        moved[k][fence] = uv
    return moved, dataclasses.replace(scene, tris=moved, nodes=refit_nodes(scene.nodes, moved))


_FACTORS = (("do_mis", (0, 1)), ("leaves", (1, 2)), ("traversal", (0, 1)), ("overlap", (0, 2)), ("frames_per_batch", (0, 1)),
            ("planes", (False, True)), ("fence_layers", (False, True)))
# Five settings of the seven two-valued factors and their complements, one pair per bounce limit: every value of every factor meets
# every bounce limit, and, the columns of the last four rows being pairwise distinct, every pair of values of two factors occurs
# (tests/test_alpha_replay_host.py checks both).
_SETTINGS = ("0000000", "0101010", "0011001", "0110100", "0001111")


def per_sample_cases(repack_bounce):
    """Option sets of the per-sample comparison, the same for every scene: bounce limits 1, at the repack bounce, one and two above it
    and 8; do_mis; both leaf kinds; both traversal picks; overlap 0 and 2; one frame and many per batch; planes and moments on and
    off; max_layers at its default and equal to the number of fences (fence_layers); two row ranges of TILE."""
    cases = []
    for mb, bits in zip((1, repack_bounce, repack_bounce + 1, repack_bounce + 2, 8), _SETTINGS):
        for flip in (0, 1):
            c = dict(max_bounces=mb, tile=False)
            c.update({k: vals[int(b) ^ flip] for (k, vals), b in zip(_FACTORS, bits)})
            cases.append(c)
    cases.append(dict(max_bounces=8, do_mis=1, leaves=2, traversal=0, overlap=2, frames_per_batch=0, planes=False, fence_layers=False, tile=True))
    cases.append(dict(max_bounces=repack_bounce + 1, do_mis=0, leaves=1, traversal=1, overlap=0, frames_per_batch=1, planes=True,
                      fence_layers=True, tile=True))
    return cases


def case_view(case, offset=(0.0, 0.0, 0.0)):
    """(camera, (y0, y1)) of a case"""
    if case["tile"]:
        return case_camera((TILE["width"], TILE["height"]), offset), TILE["rows"]
    return case_camera(SIZE, offset), (0, 0)


_far = {}


def far_scene():
    """(cutout scene, cutoff, ghost, camera) of the stripes fence with everything offset by FAR['offset']"""
    if "scene" not in _far:
        cut, cutoff, _ = case_scene("stripes", FAR["offset"])
        _far["scene"] = (cut, cutoff, ghost(cut, cutoff)[0], case_camera(FAR["size"], FAR["offset"]))
    return _far["scene"]


def far_rows_aside(oracle, do_mis, max_bounces=8):
    """200 units out the triangle test leaks by itself: (the rows of the FAR render that hold a ray on which the replay disagrees, found
    by tapping one row at a time: (H,) bool; the number of such rays). Computed once per do_mis."""
    if do_mis not in _far:
        cut, cutoff, gh, cam = far_scene()
        bad = np.zeros(FAR["size"][1], np.int64)
        for y in range(len(bad)):
            r = replay(oracle, cut, cutoff, gh, cam, FAR["frames"], (y, y + 1), max_bounces, do_mis)
            assert r.exhausted == 0
            bad[y] = r.disagreeing_closest + r.disagreeing_shadow
        _far[do_mis] = (bad > 0, int(bad.sum()))
    return _far[do_mis]
