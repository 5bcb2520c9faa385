"""A plain reference for what an emissive-mapped surface shows in a one-bounce, MIS-off, one-frame render.

Written from the lookup's definition (pt.wgsl getTextureColor: uv % 1.0 scales into the material's rect, the texel is read
from the row-major atlas, anything outside it reads zero; w or h = 0 gives the fallback), in numpy and float64, sharing no
code with the kernels or either oracle. Only the steps whose rounding decides the visible result are done in float32:
the texel itself, the attenuation 1 / (1 + t^2) and its product with the texel.

The texel index comes from the float64 texel coordinate. The kernels compute it in float32 (the UV interpolation, then
x + fract(uv) * w), so where the float64 value is too close to a texel boundary - or to a whole UV, where fract(uv) jumps -
for float32 to decide it the same way, the pixel is "ambiguous": it must show one of the few texels the interval of
coordinates reaches, and is left out of the exact check.
"""
import math

import numpy as np

F32_INT = 2.0 ** 23          # every float32 of at least this magnitude is a whole number
U32_MAX = 4294967295


def _ulp32(x):
    x = abs(float(x))
    if x < 2.0 ** -126:
        return 2.0 ** -149
    return 2.0 ** (math.floor(math.log2(x)) - 23)


def _u32(c):
    """WGSL u32(f) as the project defines it: truncating, saturating, NaN -> 0"""
    if not c > 0.0:
        return 0
    if c >= 4294967296.0:
        return U32_MAX
    return int(c)


def _axis_indices(uvs, bary, origin, size, limit):
    """Texel indices one axis of the lookup can reach: a sorted tuple of ints, -1 standing for 'outside the atlas'."""
    if not np.isfinite(uvs).all():
        return (0 if limit > 0 else -1,)                  # a non-finite UV makes fract(uv) NaN, whose u32 is 0
    uv = float(np.dot(uvs, bary))
    tol = 2.0 ** -21 * max(1.0, float(np.abs(uvs).max()))  # bound on the float32 interpolation's error
    lo, hi = uv - tol, uv + tol
    if min(abs(lo), abs(hi)) >= F32_INT and lo * hi > 0:
        pieces = [(0.0, 0.0)]                               # no fractional bits: fract = 0 exactly
    else:
        # fract(v) = v - trunc(v) is continuous between consecutive non-zero integers; split [lo, hi] there
        cuts = [n for n in range(math.floor(lo), math.ceil(hi) + 1) if n != 0 and lo <= n <= hi]
        pieces, a = [], lo
        for n in cuts:
            if a < n:
                T = math.trunc((a + n) / 2)
                pieces.append((a - T, n - T))
            pieces.append((0.0, 0.0))                       # v = n exactly
            a = n
        if a < hi or not cuts:
            T = math.trunc((a + hi) / 2)
            pieces.append((a - T, hi - T))
    out = set()
    for fa, fb in pieces:
        ca, cb = origin + fa * size, origin + fb * size
        if fa == fb == 0.0 and origin < 2 ** 24:
            m = 0.0                                         # x + 0 * w: no rounding anywhere
        else:                                               # the float32 product and sum round by half an ulp each
            m = max(1e-4, _ulp32(max(abs(fa), abs(fb)) * size) + _ulp32(max(abs(ca), abs(cb), 1.0)))
        ia, ib = _u32(min(ca, cb) - m), _u32(max(ca, cb) + m)
        if ia >= limit:
            out.add(-1)
            continue
        out.update(range(ia, min(ib, limit - 1) + 1))
        if ib >= limit:
            out.add(-1)
    return tuple(sorted(out))


def _texel(atlas, ix, iy):
    if ix < 0 or iy < 0:
        return np.zeros(3, np.float32)
    return atlas[iy, ix, :3].astype(np.float32)


def _shown(texel, t):
    """what the one-bounce frame holds for an emissive hit of emission texel * (1, 1, 1), strength 1, at distance t"""
    if not (texel > 0).any():
        return np.zeros(3, np.float32)
    t = np.float32(t)
    att = np.float32(1) / (np.float32(1) + t * t)
    with np.errstate(invalid="ignore", over="ignore"):
        radiance = np.float32(0) + texel * att               # the path's radiance starts at zero
    return np.fmin(radiance, np.float32(2.5))                # the accumulation's clamp


def probe_materials(scene):
    """indices of the materials the reference describes: emission (1, 1, 1), strength 1 and an emissive map"""
    m = scene.mats
    sel = (m["emission"] == 1.0).all(axis=1) & (m["emissive_strength"] == 1.0) & \
          ((m["emissive_map"]["w"] != 0) | (m["emissive_map"]["h"] != 0) | (m["emissive_map"]["x"] != 0))
    return np.flatnonzero(sel)


def predict(scene, t, tri, u, v):
    """For the closest hits (t, tri, u, v) of a frame's camera rays: (probe, exact, value, candidates).
    probe[i]: the ray hit a probe material; exact[i]: one texel decides the pixel, whose RGB is value[i];
    candidates[i]: for an ambiguous probe pixel, the list of RGB values it may show."""
    n = len(t)
    atlas = scene.atlas
    H, W = atlas.shape[:2]
    pm = set(probe_materials(scene).tolist())
    probe, exact = np.zeros(n, bool), np.zeros(n, bool)
    value = np.zeros((n, 3), np.float32)
    candidates = [None] * n
    for i in range(n):
        if not t[i] > 0:
            continue
        T = scene.tris[int(tri[i])]
        mi = int(T["material_index"])
        if mi not in pm:
            continue
        probe[i] = True
        r = scene.mats[mi]["emissive_map"]
        x0, y0, w, h = int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])
        if w == 0 or h == 0:
            outs = [_shown(np.ones(3, np.float32), t[i])]
        else:
            uu, vv = float(u[i]), float(v[i])
            bary = np.array([1.0 - uu - vv, uu, vv])
            uvs = np.array([T["uv0"], T["uv1"], T["uv2"]], np.float64)
            xs = _axis_indices(uvs[:, 0], bary, x0, w, W)
            ys = _axis_indices(uvs[:, 1], bary, y0, h, H)
            outs = []
            for ix in xs:
                for iy in ys:
                    o = _shown(_texel(atlas, ix, iy) if ix >= 0 and iy >= 0 else np.zeros(3, np.float32), t[i])
                    if not any(np.array_equal(o.view(np.uint32), q.view(np.uint32)) for q in outs):
                        outs.append(o)
        if len(outs) == 1:
            exact[i], value[i] = True, outs[0]
        else:
            candidates[i] = outs
    return probe, exact, value, candidates


def check(scene, rgb, t, tri, u, v, min_exact=0.95):
    """Asserts that the frame's RGB (n, 3) is what predict() says; returns (probe pixels, exactly checked pixels)."""
    probe, exact, value, cand = predict(scene, t, tri, u, v)
    rgb = np.ascontiguousarray(rgb, np.float32)
    bad = exact & (rgb.view(np.uint32) != value.view(np.uint32)).any(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{scene.name}: {int(bad.sum())} of {int(exact.sum())} exactly predicted probe pixels differ; "
                             f"first: pixel {i} (triangle {int(tri[i])}, u {u[i]!r}, v {v[i]!r}) shows {rgb[i]} where "
                             f"the reference has {value[i]}")
    for i in np.flatnonzero(probe & ~exact):
        assert any(np.array_equal(rgb[i].view(np.uint32), q.view(np.uint32)) for q in cand[i]), \
            f"{scene.name}: ambiguous pixel {i} shows {rgb[i]}, none of {cand[i]}"
    assert probe.sum() > 0.3 * len(t), f"{scene.name}: only {int(probe.sum())} probe pixels"
    assert exact.sum() >= min_exact * probe.sum(), f"{scene.name}: {int(exact.sum())} of {int(probe.sum())} exact"
    return int(probe.sum()), int(exact.sum())
