"""Lightmap baking on the host (include/ptmi.h ptmi_upload_bake_surface): a mesh's lightmap UVs rasterised into the texel records a bake
starts its paths from. host/bake.js states the same rule operation by operation and gives the same float32 bits.

The rule. Texel (x, y) of a W x H lightmap has its centre at p = ((x + 0.5) / W, (y + 0.5) / H). For a triangle with lightmap
coordinates a, b, c, in float64:
    den = (b.y - c.y) * (a.x - c.x) + (c.x - b.x) * (a.y - c.y)                        (0: the triangle has no area and covers nothing)
    w0  = ((b.y - c.y) * (p.x - c.x) + (c.x - b.x) * (p.y - c.y)) / den
    w1  = ((c.y - a.y) * (p.x - c.x) + (a.x - c.x) * (p.y - c.y)) / den
    w2  = (1 - w0) - w1
The texel is covered by the FIRST triangle in order with w0 >= 0, w1 >= 0 and w2 >= 0: a centre on an edge two triangles share goes to
the earlier one, and a triangle that contains no centre covers nothing. Its position and normal are (w0 * v0 + w1 * v1) + w2 * v2 of
the triangle's corners, in float64, rounded once to float32. The normal is not normalised here: the device does that.
"""
import numpy as np

from . import layout


def rasterise(positions, normals, lightmap_uvs, W, H):
    """positions, normals: (T, 3, 3); lightmap_uvs: (T, 3, 2), in [0, 1]^2 with v = 0 at the lightmap's bottom row. Returns the (H, W)
    layout.BAKE_TEXEL records of Context.upload_bake_surface; uncovered texels are all zeros."""
    P = np.asarray(positions, np.float64).reshape(-1, 3, 3)
    N = np.asarray(normals, np.float64).reshape(-1, 3, 3)
    UV = np.asarray(lightmap_uvs, np.float64).reshape(-1, 3, 2)
    assert len(P) == len(N) == len(UV)
    out = np.zeros((H, W), layout.BAKE_TEXEL)
    covered = np.zeros((H, W), bool)
    cx, cy = (np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H
    for t in range(len(UV)):
        (ax, ay), (bx, by), (cx_, cy_) = UV[t]
        den = (by - cy_) * (ax - cx_) + (cx_ - bx) * (ay - cy_)
        if den == 0.0 or not np.isfinite(den):
            continue
        # the texels whose centres can lie inside: a generous box, which decides nothing
        x0, x1 = int(np.clip(np.floor(min(ax, bx, cx_) * W) - 1, 0, W)), int(np.clip(np.ceil(max(ax, bx, cx_) * W) + 1, 0, W))
        y0, y1 = int(np.clip(np.floor(min(ay, by, cy_) * H) - 1, 0, H)), int(np.clip(np.ceil(max(ay, by, cy_) * H) + 1, 0, H))
        if x0 >= x1 or y0 >= y1:
            continue
        px, py = cx[None, x0:x1], cy[y0:y1, None]
        w0 = ((by - cy_) * (px - cx_) + (cx_ - bx) * (py - cy_)) / den
        w1 = ((cy_ - ay) * (px - cx_) + (ax - cx_) * (py - cy_)) / den
        w2 = (1.0 - w0) - w1
        take = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & ~covered[y0:y1, x0:x1]
        if not take.any():
            continue
        ys, xs = np.nonzero(take)
        a, b, c = w0[ys, xs][:, None], w1[ys, xs][:, None], w2[ys, xs][:, None]
        rec = out[y0:y1, x0:x1]
        rec["position"][ys, xs] = (a * P[t, 0] + b * P[t, 1]) + c * P[t, 2]
        rec["normal"][ys, xs] = (a * N[t, 0] + b * N[t, 1]) + c * N[t, 2]
        rec["covered"][ys, xs] = 1
        covered[y0:y1, x0:x1] |= take
    return out


def scene_arrays(scene, lightmap_uvs=None):
    """(positions, normals, lightmap_uvs) of a ptmi scene's triangles for rasterise; lightmap_uvs None: the triangles' own uv0..2"""
    t = scene.tris
    pos = np.stack([t["v0"], t["v1"], t["v2"]], axis=1)
    nrm = np.stack([t["n0"], t["n1"], t["n2"]], axis=1)
    uv = np.stack([t["uv0"], t["uv1"], t["uv2"]], axis=1) if lightmap_uvs is None else lightmap_uvs
    return pos, nrm, uv
