"""A numpy model of alpha blending as hashed stochastic transparency (include/ptmi.h ptmi_set_alpha_blend; csrc/alpha.hip; DESIGN.md
§20): the hash of a ray, the rule of a hit under both tables, and the two resolve loops of tests/alpha_ref.py with the hole rule
replaced. The lookup, the step past an absent hit and the distance along the original ray are alpha_ref's own; the loops are written
out again here because the blend rule asks about the ray of the leg, which alpha_ref's is_hole never sees.

The rule: a hit on a material with blend factor f >= 0 examines alpha = f * a_texel (one float32 multiply) and is NOT THERE iff
alpha <= xi, xi = float(h >> 8) * 2^-24, with
    mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          (uint32, wrapping)
    h = 0x9E3779B9;  for w in bits(o.x), bits(o.y), bits(o.z), bits(d.x), bits(d.y), bits(d.z), tri, seed:  h = mix(h ^ w)
(o, d) being the leg's ray: the caller's in round 0, the stepped origin and the same direction afterwards. The cutoff rule, where a
cutoff table is given too, is asked first; its holes are no blend tests.
"""
import numpy as np

import alpha_ref as A

F = np.float32
U = np.uint32
GOLDEN = 0x9E3779B9
M1, M2 = 0x7FEB352D, 0x846CA68B


def mix(x):
    x = np.asarray(x, U).copy()
    x ^= x >> U(16)
    x *= U(M1)
    x ^= x >> U(15)
    x *= U(M2)
    x ^= x >> U(16)
    return x


def hash_words(o, d, tri, seed):
    """h of each ray: o, d (n, 3) float32 taken by their bits, tri (n,) triangle indices, seed one word"""
    o = np.ascontiguousarray(np.asarray(o, F).reshape(-1, 3)).view(U)
    d = np.ascontiguousarray(np.asarray(d, F).reshape(-1, 3)).view(U)
    tri = np.asarray(tri).astype(U).reshape(-1)
    h = np.full(len(o), GOLDEN, U)
    with np.errstate(over="ignore"):
        for w in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tri, np.full(len(o), seed & 0xFFFFFFFF, U)):
            h = mix(h ^ w)
    return h


def xi(o, d, tri, seed):
    """the threshold of each ray on its hit triangle, float32 in [0, 1)"""
    return ((hash_words(o, d, tri, seed) >> U(8)).astype(F) * F(2.0 ** -24)).astype(F)


def absent(scene, blend, seed, o, d, tri, u, v, cutoff=None):
    """(the hit is not there, the blend rule was asked) for the hits (tri, u, v) of the legs (o, d)"""
    tri = np.asarray(tri, np.int64)
    n_mats = len(scene.mats)
    mi = scene.tris[tri]["material_index"].astype(np.int64)
    known = mi < n_mats
    mc = np.minimum(mi, n_mats - 1)
    blend = np.asarray(blend, F)
    f = np.where(known, blend[mc], F(-1))
    cut = np.zeros(len(tri), F) if cutoff is None else np.where(known, np.asarray(cutoff, F)[mc], F(0))
    texel = A.alpha_of(scene, tri, u, v)
    masked = (cut > 0) & (texel < cut)
    tested = ~masked & ~(f < 0)
    alpha = (f * texel).astype(F)
    with np.errstate(invalid="ignore"):
        gone = tested & (alpha <= xi(o, d, tri, seed))
    return masked | gone, tested


def _count(counts, tested, hole):
    if counts is not None:
        counts["tests"] = counts.get("tests", 0) + int(tested.sum())
        counts["passes"] = counts.get("passes", 0) + int((tested & hole).sum())


def resolve(intersect, scene, blend, o, d, max_layers=A.DEFAULT_LAYERS, seed=0, cutoff=None, counts=None):
    """alpha_ref.resolve under the blend rule: (t along the given ray, triangle, layers). counts (a dict, optional) gains 'tests' and
    'passes' as ptmi_alpha_blend_status counts them."""
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
        hole, tested = hit.copy(), np.zeros(len(idx), bool)
        hole[hit], tested[hit] = absent(scene, blend, seed, o[idx][hit], d[idx][hit], tri[hit], u[hit], v[hit], cutoff)
        _count(counts, tested, hole)
        exhausted = hole & (r >= max_layers)
        go = hole & ~exhausted
        done = idx[~go]
        t_out[done] = t[~go]
        if r > 0:
            k = hit & ~go
            t_out[idx[k]] = A.hit_t(scene, tri[k], o0[idx[k]], d[idx[k]], travelled[idx[k]] + t[k])
        tri_out[done] = tri[~go]
        layers[done] = np.where(exhausted[~go], max_layers + 1, r)
        nxt = idx[go]
        o2, st = A.step(o[nxt], d[nxt], t[go])
        o[nxt] = o2
        travelled[nxt] = travelled[nxt] + st
        idx = nxt
    return t_out, tri_out, layers


def occluded(intersect, scene, blend, o, d, dist, max_layers=A.DEFAULT_LAYERS, seed=0, cutoff=None, counts=None):
    """alpha_ref.occluded under the blend rule: (occluded 0 / 1, layers)"""
    o, d = np.asarray(o, F).reshape(-1, 3).copy(), np.asarray(d, F).reshape(-1, 3)
    o0 = o.copy()
    dist = np.asarray(dist, F)
    tlim_all = np.where(dist < 0, F(np.nan), dist - A.PT_EPS * F(2)).astype(F)
    n = len(o)
    occ, layers = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    travelled = np.zeros(n, F)
    idx = np.arange(n)
    for r in range(max_layers + 1):
        if not len(idx):
            break
        t, tri, u, v = intersect(o[idx], d[idx])
        hit = ~(t < 0)
        t_ray = t.copy()
        if r > 0:
            t_ray[hit] = A.hit_t(scene, tri[hit], o0[idx[hit]], d[idx[hit]], travelled[idx[hit]] + t[hit])
        with np.errstate(invalid="ignore"):
            nearer = hit & ~(t_ray >= tlim_all[idx])
        hole, tested = nearer.copy(), np.zeros(len(idx), bool)
        hole[nearer], tested[nearer] = absent(scene, blend, seed, o[idx][nearer], d[idx][nearer], tri[nearer], u[nearer], v[nearer], cutoff)
        _count(counts, tested, hole)
        exhausted = hole & (r >= max_layers)
        go = hole & ~exhausted
        done = idx[~go]
        occ[done] = nearer[~go]
        layers[done] = np.where(exhausted[~go], max_layers + 1, r)
        nxt = idx[go]
        o2, st = A.step(o[nxt], d[nxt], t[go])
        o[nxt] = o2
        travelled[nxt] = travelled[nxt] + st
        idx = nxt
    return occ, layers


def blend_table(scene, factor=1.0, fences=None):
    """-1 everywhere but at the fences' materials (all of them, or those listed by fence number), which get `factor`"""
    t = np.full(len(scene.mats), -1.0, F)
    mats = scene.info["fence_materials"]
    for k in (range(len(mats)) if fences is None else fences):
        t[mats[k]] = factor
    return t
