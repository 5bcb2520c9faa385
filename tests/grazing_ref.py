"""Adversarial geometry and rays for the own-leaf traversal (ptmi_options.leaves = 2).

The argument that the own leaves return the reference traversal's results rests on a bound: a ray that meets triangle T in
Moller-Trumbore's arithmetic also meets T's PADDED box. Where that bound is weakest the renders of the benchmark scenes never go:
long thin triangles (their (u, v) lose accuracy fastest), rays within 1e-7 ... 1e-2 rad of their plane, aimed at their edges and
vertices, and reference leaves much larger than the triangles they list. This module builds exactly that, deterministically from a
seed: the geometry in float64, everything handed to the library rounded to float32.

Scenes (ptmi.scenes._finish, material 0 the slivers, material 1 one emissive quad so that they render):
  sliver_fan      triangles of aspect 1e2 ... 1e6 at random orientations, exactly in axis planes (zero-thickness boxes), and tilted
                  1e-6 ... 1e-3 rad off them
  sliver_strip    a floor cut into long thin triangles that share edges: a disk of thin wedges (reference leaves pair wedges of
                  opposite slopes: boxes much larger than each wedge's) beside a band of strips tilted 3e-5 rad off the axis plane
  either of them translated far from the origin (coordinates ~1e4, extent ~1) or shrunk (extent ~3e-2, where the contract's
  determinant limit 1e-6 still lets most of them be hit): the padding (2^-16 of the largest coordinate) large and small against the
  geometry.
  mixed_fan       the fan's construction at aspect 1 ... 300: ordinary triangles, which keep their own padded boxes, and slivers
                  just above the threshold at which a triangle enters the own hierarchy with its reference leaf's box
Rays (rays()): aimed just inside an edge of a sliver, exactly on it, at a vertex, or outside by 1 ... 1e4 ulp of the barycentrics; at
10^U(-7, -2) rad to its plane (the grazing family) or 10^U(-2, 0) (the control family); along its long axis, across it, or anywhere in
its plane; from 1e-2 away up to just inside and just outside the safe origin (the cube of half-side 8 x the largest coordinate
within which the own tree takes a ray). Each ray is also a shadow ray: to the aim point +- a few ulp, and directional (-1)."""
import ctypes
import os
import sys

import numpy as np

from ptmi import layout, native, scenes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import own_leaf_gate as gate            # noqa: E402

SLIVER, EMISSIVE = 0, 1
FAR = (1.2e4, 0.9e4, -1.1e4)
TRANSFORMS = {"": (1.0, (0.0, 0.0, 0.0)), "far": (1.0, FAR), "shrunk": (3e-2, (0.0, 0.0, 0.0))}
SLIVER_RATIO = 16.0                  # fast_tree.h PT_OWN_SLIVER


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(rng, nrm):
    """random unit vectors perpendicular to the rows of nrm"""
    r = _unit(rng.standard_normal(nrm.shape))
    p = r - (r * nrm).sum(-1, keepdims=True) * nrm
    return _unit(p)


def _tris(v64, mat):
    v = v64.astype(np.float32)
    e = np.cross(v64[:, 1] - v64[:, 0], v64[:, 2] - v64[:, 0])
    ln = np.linalg.norm(e, axis=-1, keepdims=True)
    n = np.where(ln > 0, e / np.where(ln > 0, ln, 1.0), 0.0).astype(np.float32)
    return scenes._tri_array(v, np.repeat(n[:, None, :], 3, 1), np.zeros((len(v), 3, 2), np.float32), mat)


def _emitter(y):
    q = np.array([[-0.3, y, -0.3], [0.3, y, -0.3], [0.3, y, 0.3], [-0.3, y, 0.3]], np.float64)
    return np.stack([q[[0, 2, 1]], q[[0, 3, 2]]])                  # facing down


def _mats():
    return [scenes._material((0.8, 0.8, 0.8)), scenes._material((0.8, 0.8, 0.8), emission=(1, 1, 1), strength=8.0)]


def _finish(name, parts, transform):
    """parts: [(float64 [m, 3, 3] vertices, material)] in the unit frame; transform: a key of TRANSFORMS"""
    scale, offset = TRANSFORMS[transform]
    off = np.array(offset, np.float64)
    tris = [_tris(v * scale + off, m) for v, m in parts]
    return scenes._finish(name + (f"_{transform}" if transform else ""), tris, _mats())


def sliver_ratio(tris):
    """longest edge squared / |e1 x e2| of each triangle, as fast_tree.h pt_own_sliver compares it with PT_OWN_SLIVER"""
    v0, v1, v2 = (tris[k].astype(np.float64) for k in ("v0", "v1", "v2"))
    longest = np.maximum.reduce([((v1 - v0) ** 2).sum(1), ((v2 - v0) ** 2).sum(1), ((v2 - v1) ** 2).sum(1)])
    with np.errstate(divide="ignore", invalid="ignore"):
        return longest / np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)


def sliver_fan_geometry(seed, n, log_aspect=(2.0, 6.0)):
    """[n, 3, 3] float64 slivers inside about [-1, 1]^3 (aspect 10^U(log_aspect)), four kinds in turn: random orientation, exactly in an axis plane (random
    in-plane direction), exactly in an axis plane along an axis, tilted 1e-6 ... 1e-3 rad off an axis plane"""
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 4
    aspect = 10.0 ** rng.uniform(*log_aspect, n)
    L = rng.uniform(0.3, 1.5, n)
    c = rng.uniform(-0.8, 0.8, (n, 3))
    axis = rng.integers(0, 3, n)
    nrm = _unit(rng.standard_normal((n, 3)))
    ax_n = np.eye(3)[axis]
    nrm[kind > 0] = ax_n[kind > 0]
    a = _perp(rng, nrm)
    other = np.eye(3)[(axis + 1 + rng.integers(0, 2, n)) % 3]
    a[kind == 2] = other[kind == 2]
    b = np.cross(nrm, a)
    tilt = 10.0 ** rng.uniform(-6, -3, n)
    tk = kind == 3
    about_long = rng.random(n) < 0.5                               # tilt about the long axis (thickness w sin) or across it (L sin)
    ct, st = np.cos(tilt)[:, None], np.sin(tilt)[:, None]
    b2 = np.where(about_long[:, None], ct * b + st * nrm, b)
    a2 = np.where(about_long[:, None], a, ct * a + st * nrm)
    a[tk], b[tk] = a2[tk], b2[tk]
    w = L / aspect
    s = rng.uniform(0.05, 0.95, n)
    v = np.stack([c - a * (L / 2)[:, None], c + a * (L / 2)[:, None], c + a * (L * (s - 0.5))[:, None] + b * w[:, None]], 1)
    plane = kind == 1
    plane |= kind == 2
    rows = np.flatnonzero(plane)
    v[rows, :, axis[rows]] = c[rows, axis[rows]][:, None]           # exactly in the plane: zero-thickness boxes
    rot = rng.integers(0, 3, n)                                    # which vertex is v0, and the winding
    for r in range(1, 3):
        v[rot == r] = np.roll(v[rot == r], r, axis=1)
    flip = rng.random(n) < 0.5
    v[flip] = v[flip][:, [0, 2, 1]]
    return v


def sliver_fan(seed=1, n=500, transform=""):
    return _finish(f"sliver_fan{n}", [(sliver_fan_geometry(seed, n), SLIVER), (_emitter(2.0), EMISSIVE)], transform)


def mixed_fan(seed=4, n=3000):
    """the fan's construction at aspect 1 ... 300: ordinary triangles (ratio 1 ... 16, which keep their own boxes) and slivers just
    above the threshold (fast_tree.h pt_own_sliver), side by side"""
    return _finish(f"mixed_fan{n}", [(sliver_fan_geometry(seed, n, (0.0, 2.5)), SLIVER), (_emitter(2.0), EMISSIVE)], "")


def sliver_strip_geometry(n_wedges=1200, n_strips=700):
    """A disk of radius 1 at y = 0 cut into thin wedges around its centre (shared centre and rim vertices), and beside it the band
    x in [1.05, 3.05], z in [-1, 1] cut into strips along z, each split on its diagonal, tilted 3e-5 rad about the z axis"""
    ang = np.linspace(0.0, 2 * np.pi, n_wedges + 1)
    rim = np.stack([np.cos(ang), np.zeros_like(ang), np.sin(ang)], 1)
    rim[-1] = rim[0]
    ctr = np.zeros((n_wedges, 3))
    wedges = np.stack([ctr, rim[1:], rim[:-1]], 1)                 # winding: normal +y
    x = np.linspace(1.05, 3.05, n_strips + 1)
    y = (x - 1.05) * 3e-5
    p00 = np.stack([x[:-1], y[:-1], np.full(n_strips, -1.0)], 1)
    p10 = np.stack([x[1:], y[1:], np.full(n_strips, -1.0)], 1)
    p11 = np.stack([x[1:], y[1:], np.full(n_strips, 1.0)], 1)
    p01 = np.stack([x[:-1], y[:-1], np.full(n_strips, 1.0)], 1)
    strips = np.concatenate([np.stack([p00, p11, p10], 1), np.stack([p00, p01, p11], 1)])
    return np.concatenate([wedges, strips])


def sliver_strip(transform=""):
    return _finish("sliver_strip", [(sliver_strip_geometry(), SLIVER), (_emitter(1.5), EMISSIVE)], transform)


def strip_camera(W, H, transform="", degrees=4.0, frame_index=0):
    """a camera a few degrees above the strip floor, looking along +x over the wedge disk onto the strip band"""
    scale, offset = TRANSFORMS[transform]
    a = np.radians(degrees)
    fwd = np.array([np.cos(a), -np.sin(a), 0.0])
    pos = np.array([-1.6, 1.6 * np.tan(a) + 0.02, 0.05]) * scale + np.array(offset)
    up = np.array([np.sin(a), np.cos(a), 0.0])
    return layout.make_camera(W, H, position=tuple(pos), forward=tuple(fwd), right=(0.0, 0.0, 1.0), up=tuple(up),
                              fov=np.pi / 4, aperture=0.0, focus_distance=3.0, frame_index=frame_index)


def _solve_max_abs(P, d, S):
    """s > 0 with max_k |P_k - s d_k| = S (float64 bisection; the max is convex and grows without bound)"""
    lo = np.zeros(len(P))
    hi = np.full(len(P), 4.0 * (S + np.abs(P).max()))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        over = np.abs(P - mid[:, None] * d).max(1) > S
        hi = np.where(over, mid, hi)
        lo = np.where(over, lo, mid)
    return 0.5 * (lo + hi)


def rays(sc, n, seed, family, safe_origin, targets=None):
    """n rays at the triangles `targets` of sc (default: material 0, the slivers): (o [n, 3] f32, d [n, 3] f32, dist [n] f32 for the shadow use of the same ray,
    meta: dict of float64 arrays — the aim point, the angle to the plane, the chosen triangle, the kinds)"""
    assert family in ("grazing", "control")
    rng = np.random.default_rng(seed)
    idx = np.flatnonzero(sc.tris["material_index"] == SLIVER) if targets is None else np.asarray(targets)
    tri = idx[rng.integers(0, len(idx), n)]
    T = sc.tris[tri]
    v0, v1, v2 = (T[k].astype(np.float64) for k in ("v0", "v1", "v2"))
    e1, e2 = v1 - v0, v2 - v0
    # aim point P = v0 + u e1 + v e2
    aim = rng.integers(0, 5, n)                                    # 0 just inside an edge, 1 on it, 2 a vertex, 3 outside an edge, 4 beyond a vertex
    edge = rng.integers(0, 3, n)
    s = rng.random(n)
    delta = 10.0 ** rng.uniform(0, 4, n) * 2.0 ** -24
    base = np.where(edge[:, None] == 0, np.stack([s, 0 * s], 1), np.where(edge[:, None] == 1, np.stack([0 * s, s], 1), np.stack([s, 1 - s], 1)))
    inward = np.array([[0.0, 1.0], [1.0, 0.0], [-0.5, -0.5]])[edge]
    sign = np.choose(aim, [1.0, 0.0, 0.0, -1.0, 0.0])
    uv = base + (sign * delta)[:, None] * inward
    vert = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])[edge]
    uv[aim == 2] = vert[aim == 2]
    # beyond a vertex: outward from the triangle's barycentric centre, past the vertex (past the tip of a sliver: outside its box)
    out = vert - 1.0 / 3.0
    uv[aim == 4] = (vert + delta[:, None] * 16.0 * out / np.linalg.norm(out, axis=1, keepdims=True))[aim == 4]
    P = v0 + uv[:, :1] * e1 + uv[:, 1:] * e2
    # direction: theta off the plane, in-plane part along / across the long axis or anywhere
    nrm = np.cross(e1, e2)
    nl = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(nl > 0, nrm / np.where(nl > 0, nl, 1.0), np.array([0.0, 1.0, 0.0]))
    edges = np.stack([e1, e2, v2 - v1], 1)
    longest = edges[np.arange(n), np.linalg.norm(edges, axis=2).argmax(1)]
    along = _unit(longest)
    across = _unit(np.cross(nrm, along))
    dk = rng.integers(0, 3, n)
    phi = rng.uniform(0, 2 * np.pi, n)[:, None]
    inplane = np.where(dk[:, None] == 0, along, np.where(dk[:, None] == 1, across, np.cos(phi) * along + np.sin(phi) * across))
    inplane *= rng.choice([-1.0, 1.0], n)[:, None]
    # along / across an axis-aligned sliver the direction would have a zero component (the slow path from the start): turned off it
    # by 1e-6 ... 1e-2 rad in the plane for three rays in four
    turn = np.where((dk < 2) & (rng.random(n) < 0.75), 10.0 ** rng.uniform(-6, -2, n), 0.0)[:, None]
    inplane = _unit(np.cos(turn) * inplane + np.sin(turn) * np.cross(nrm, inplane))
    lo, hi = (-7.0, -2.0) if family == "grazing" else (-2.0, 0.0)
    theta = 10.0 ** rng.uniform(lo, hi, n)
    side = rng.choice([-1.0, 1.0], n)[:, None]
    d64 = np.cos(theta)[:, None] * inplane + np.sin(theta)[:, None] * side * nrm
    d = d64.astype(np.float32)
    # origin: P - s d, s from 1e-2 to a few scene extents, or just inside / just outside the safe origin
    ext = float(np.abs(sc.nodes[0]["aabb_max"].astype(np.float64) - sc.nodes[0]["aabb_min"]).max())
    sdist = 10.0 ** rng.uniform(-2, np.log10(4 * ext), n)
    edge_o = rng.random(n) < 0.2
    s_star = _solve_max_abs(P, d.astype(np.float64), float(safe_origin))
    beyond = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, -3, n)
    sdist = np.where(edge_o, s_star * (1 + beyond), sdist)
    o = (P - sdist[:, None] * d.astype(np.float64)).astype(np.float32)
    # shadow use: the float64 distance to P (along the float32 ray) +- a few ulp, or a directional light
    od, dd = o.astype(np.float64), d.astype(np.float64)
    tP = ((P - od) * dd).sum(1) / (dd * dd).sum(1)
    dist = tP.astype(np.float32)
    k = rng.integers(-4, 5, n)
    for step in range(1, 5):
        dist = np.where(k >= step, np.nextafter(dist, np.float32(np.inf)), dist)
        dist = np.where(k <= -step, np.nextafter(dist, np.float32(-np.inf)), dist)
    dist = np.where(rng.random(n) < 0.25, np.float32(-1.0), dist).astype(np.float32)
    meta = {"P": P, "theta": theta, "tri": tri, "aim": aim, "dir_kind": dk, "origin_edge": edge_o}
    return o, d, dist, meta


def classify(sc, pad, o, d, tri):
    """float64 verdict on a ray whose result differs, about the triangle the reference reported: did the ray really pass within the
    padding of its box (the padding argument would be broken), or did Moller-Trumbore's rounding accept a ray that misses the
    triangle (and its padded box) entirely?"""
    T = sc.tris[int(tri)]
    v = np.array([T["v0"], T["v1"], T["v2"]], np.float64)
    lo, hi = v.min(0) - pad, v.max(0) + pad
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    tmin, tmax = np.nanmax(np.minimum(t1, t2)), np.nanmin(np.maximum(t1, t2))
    in_box = bool(tmax >= tmin and tmax >= 0)
    e1, e2 = v[1] - v[0], v[2] - v[0]
    h = np.cross(d, e2)
    a = e1 @ h
    sv = o - v[0]
    u = (sv @ h) / a
    q = np.cross(sv, e1)
    vv = (d @ q) / a
    t = (e2 @ q) / a
    exact_hit = bool(u >= 0 and vv >= 0 and u + vv <= 1 and t > 0)
    return (f"triangle {int(tri)}: ray {'passes' if in_box else 'MISSES'} its padded box (pad {pad:.3g}); float64 "
            f"Moller-Trumbore: {'hit' if exact_hit else 'miss'} (u {u:.3g}, v {vv:.3g}, t {t:.6g})")


def records(oracle, sc, o, d, dist):
    """the rays as tools/own_sim.c takes them, with the oracle's results: closest-hit records (dist 0, the reference's t and
    triangle), shadow records (dist, the reference's closest t), and the oracle's (t, tri, u, v) and occlusion verdicts"""
    t, tri, u, v, _ = oracle.intersect(sc, o, d)
    occ = oracle.occluded(sc, o, d, dist)
    rec = np.zeros((2 * len(o), 9), np.float32)
    for h, dd in ((0, np.zeros(len(o), np.float32)), (1, dist)):
        r = rec[h * len(o):(h + 1) * len(o)]
        r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7], r[:, 8] = o, d, dd, t, tri.view(np.float32)
    return rec, (t, tri, u, v, occ)


def replay(L, img, rec, quant, cull, deferred):
    """own_sim over rec: (sums[12], per-ray result t / occluded, triangle, flags: 1 slow from the start, 2 retraced)"""
    n = len(rec)
    sums = np.zeros(12, np.uint64)
    out_t, out_tri, fl = np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    p = gate._p
    L.own_sim_run(ctypes.byref(img.s), n, p(rec), img.own, quant, cull, deferred, p(out_t), p(out_tri), p(fl), p(sums), None, 0, None)
    return sums, out_t, out_tri, fl


def shrunk_padding_image(sc, leaf_tris=0):
    """the own image with the padding shrunk to nothing (one ulp outward): the gate must be able to see the boundary"""
    os.environ["PTMI_OWN_PAD_EXTRA_LOG2"] = "-200"
    try:
        return gate.Image(sc, 2, leaf_tris)
    finally:
        os.environ.pop("PTMI_OWN_PAD_EXTRA_LOG2", None)
