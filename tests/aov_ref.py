"""A plain reference for the first-hit planes (include/ptmi.h ptmi_set_aovs): albedo, shading normal, depth and ids.

The camera rays and their closest hits (t, triangle, u, v) come from the CPU oracle (Oracle.raygen, Oracle.intersect), which agree
with the kernels bit for bit. Everything after that is written here from the definitions, in numpy, sharing no code with the
kernels or the oracle:
  albedo = base colour x albedo-map texel (float32 product; no map: the base colour itself),
  normal = normalize(n0 w + n1 u + n2 v), bent by the normal-map texel through the tangent frame of the UVs (pt.wgsl's hit
           shading; float64 here, so the kernels' float32 result is compared with a tolerance),
  depth  = t, ids = (triangle, its material_index), coverage 1 on a hit; zeros and 0xFFFFFFFF on a miss.
Texel lookups reuse tests/texture_ref.py's candidate sets: where float32 rounding may pick either of two texels the sample is
"ambiguous" and lists every value it may take.

fold() folds per-frame samples the way the output buffer is folded (frame 0 overwrites, frame f mixes with weight 1 / (f + 1)
through mix(a, b, t) = fma(b, t, a * (1 - t))), emulating the float32 FMA in float64.
"""
import numpy as np

import texture_ref

MISS = 0xFFFFFFFF


def _candidates(scene, rect, tri_rec, u, v):
    """RGB texels (float32) the lookup of `rect` at barycentrics (u, v) may return; None: the rect is empty (fallback)"""
    x0, y0, w, h = int(rect["x"]), int(rect["y"]), int(rect["w"]), int(rect["h"])
    if w == 0 or h == 0:
        return None
    atlas = scene.atlas
    if atlas is None:
        return [np.zeros(3, np.float32)]                   # no atlas bound: every lookup reads zero
    H, W = atlas.shape[:2]
    bary = np.array([1.0 - float(u) - float(v), float(u), float(v)])
    uvs = np.array([tri_rec["uv0"], tri_rec["uv1"], tri_rec["uv2"]], np.float64)
    xs = texture_ref._axis_indices(uvs[:, 0], bary, x0, w, W)
    ys = texture_ref._axis_indices(uvs[:, 1], bary, y0, h, H)
    out = []
    for ix in xs:
        for iy in ys:
            t = texture_ref._texel(atlas, ix, iy) if ix >= 0 and iy >= 0 else np.zeros(3, np.float32)
            if not any(np.array_equal(t.view(np.uint32), q.view(np.uint32)) for q in out):
                out.append(t)
    return out


def _unit(a):
    return a / np.sqrt(np.dot(a, a))


def _mapped_normal(tri_rec, u, v, n_i, texel):
    """the normal map's bend (float64): tangent from the UV derivatives, Gram-Schmidt against n_i, then TBN * (2 texel - 1)"""
    p0, p1, p2 = (np.asarray(tri_rec[k], np.float64) for k in ("v0", "v1", "v2"))
    t0, t1, t2 = (np.asarray(tri_rec[k], np.float64) for k in ("uv0", "uv1", "uv2"))
    e1, e2 = p1 - p0, p2 - p0
    d1, d2 = t1 - t0, t2 - t0
    r = 1.0 / (d1[0] * d2[1] - d1[1] * d2[0])
    tg = _unit((e1 * d2[1] - e2 * d1[1]) * r)
    Tn = _unit(tg - n_i * np.dot(n_i, tg))
    Bn = _unit(np.cross(n_i, Tn))
    m = np.asarray(texel, np.float64) * 2.0 - 1.0
    return _unit(Tn * m[0] + Bn * m[1] + n_i * m[2])


def samples(oracle, scene, cam, frame, rows=None):
    """One frame's first hits for every pixel, row-major (index y * W + x), or with `rows` (ascending row numbers) for the pixels of
    those rows only, row after row (index i * W + x for rows[i]: the texel candidates are a Python loop per pixel, and a large frame is
    sampled by rows). Returns a dict of arrays:
    albedo (n, 3) f32 (first candidate), normal (n, 3) f64, t (n,) f32 (0 on a miss), tri, mat (n,) u32, hit (n,) bool,
    albedo_exact / normal_exact (n,) bool: one texel decides the value, normal_mapped (n,) bool: a normal map bent it."""
    W, H = int(cam["width"]), int(cam["height"])
    rows = np.arange(H, dtype=np.uint32) if rows is None else np.asarray(rows, np.uint32)
    assert rows.ndim == 1 and (rows < H).all()
    ys, xs = np.repeat(rows, W), np.tile(np.arange(W, dtype=np.uint32), len(rows))
    n = len(ys)
    o, d, _ = oracle.raygen(cam, xs, ys, np.full(n, frame, np.uint32))
    t, tri, u, v, _ = oracle.intersect(scene, o, d)
    hit = ~(t < 0)
    out = dict(albedo=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float64),
               t=np.where(hit, t, np.float32(0)).astype(np.float32), tri=np.where(hit, tri, MISS).astype(np.uint32),
               mat=np.full(n, MISS, np.uint32), hit=hit, albedo_exact=np.ones(n, bool), normal_exact=np.ones(n, bool),
               normal_mapped=np.zeros(n, bool))
    one = [np.ones(3, np.float32)]
    for i in np.flatnonzero(hit):
        T = scene.tris[int(tri[i])]
        mi = int(T["material_index"])
        out["mat"][i] = mi
        m = scene.mats[mi] if mi < len(scene.mats) else None
        base = np.asarray(m["base_color"], np.float32)[:3] if m is not None else np.zeros(3, np.float32)
        alb = (_candidates(scene, m["albedo_map"], T, u[i], v[i]) if m is not None else None) or one
        out["albedo"][i] = alb[0] * base
        out["albedo_exact"][i] = len({tuple((a * base).view(np.uint32)) for a in alb}) == 1
        uu, vv = float(u[i]), float(v[i])
        w = float(np.float32(1) - u[i] - v[i])
        n_i = _unit(np.asarray(T["n0"], np.float64) * w + np.asarray(T["n1"], np.float64) * uu + np.asarray(T["n2"], np.float64) * vv)
        nm = _candidates(scene, m["normal_map"], T, u[i], v[i]) if m is not None else None
        flat = np.array([0.5, 0.5, 1.0], np.float32)
        nm = nm or [flat]
        normals = [n_i if np.array_equal(c, flat) else _mapped_normal(T, uu, vv, n_i, c) for c in nm]
        out["normal"][i] = normals[0]
        out["normal_mapped"][i] = not np.array_equal(nm[0], flat)
        out["normal_exact"][i] = len(nm) == 1
    return out


def _mix(a, b, t):
    """mix1(a, b, t) = fma(b, t, a * (1 - t)) in float32 (the FMA in float64, then rounded: the product b t is exact in float64)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    t = np.float32(t)
    p = a * (np.float32(1) - t)
    return (b.astype(np.float64) * np.float64(t) + p.astype(np.float64)).astype(np.float32)


def fold(per_frame, frames):
    """Folds per-frame samples (list of samples() dicts, for `frames` in ascending order) like the output buffer: returns
    albedo (n, 4) f32 = (albedo, coverage), normal (n, 4) f32 = (normal, t), ids (n, 2) u32 of the last frame, and
    exact (n,) bool: no sample of the pixel was ambiguous."""
    n = len(per_frame[0]["t"])
    acc_a, acc_n = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    exact = np.ones(n, bool)
    for s, f in zip(per_frame, frames):
        xa = np.concatenate([s["albedo"], s["hit"].astype(np.float32)[:, None]], axis=1)
        xn = np.concatenate([s["normal"].astype(np.float32), s["t"][:, None]], axis=1)
        if f == 0:
            acc_a, acc_n = xa.astype(np.float32), xn.astype(np.float32)
        else:
            w = np.float32(1) / np.float32(f + 1)
            acc_a, acc_n = _mix(acc_a, xa, w), _mix(acc_n, xn, w)
        exact &= s["albedo_exact"] & s["normal_exact"]
    last = per_frame[-1]
    return acc_a, acc_n, np.stack([last["tri"], last["mat"]], axis=1), exact
