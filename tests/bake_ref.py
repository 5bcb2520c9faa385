"""Lightmap baking (include/ptmi.h ptmi_upload_bake_surface, ptmi_dispatch_bake, ptmi_bake_dilate) restated in numpy, sharing no code
with the kernels (csrc/pipeline.hip bake_ray, csrc/bake.hip) or with the hosts' rasterisers (ptmi/bake.py, host/bake.js):

  rays()        the first ray of a bake path, operation by operation in float32: the oracle's RNG (pto_seed, pto_rand) and sincos
                (pto_sincos), numpy's correctly rounded sqrt, the contract normalize3 and the fused cross3 / lincomb3 / madd3 as
                tests/projection_ref.py states them. Returns org, raw (the direction before normalize3), d and the RNG state.
                (org, raw) is the ray of the pinhole with position = org, forward = raw, fov = 0, aperture = 0
                (projection_ref.fov0_cameras), which is how a bake sample is pinned against the unchanged oracle.
  covered_list  the texels a bake walks, in the order it walks them
  dilate()      the gutter fill, pass by pass
  rasterise()   the hosts' rule, texel by texel and triangle by triangle in Python floats (float64)
"""
import numpy as np

from projection_ref import PI, _fma, _sincos, normalize3

f32 = np.float32
DEFAULT_BIAS = f32(1e-6)


def cross3(a, b):
    """(ay bz - az by, az bx - ax bz, ax by - ay bx), each fma(p, q, -(r * s))"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.stack([_fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), _fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])),
                     _fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], axis=1)


def construct_tbn(n):
    """pt.wgsl:624-634: T = x (y where |n.x| > 0.9), B = normalize(n x T), T = normalize(B x n)"""
    n = np.asarray(n, f32)
    T = np.where((np.abs(n[:, 0]) > f32(0.9))[:, None], np.array([0, 1, 0], f32)[None, :], np.array([1, 0, 0], f32)[None, :]).astype(f32)
    B = normalize3(cross3(n, T))
    return normalize3(cross3(B, n)), B


def lincomb3(a, s1, b, s2, c, s3):
    """fma(c, s3, fma(b, s2, a * s1)) per component"""
    return _fma(c, s3[:, None], _fma(b, s2[:, None], a * s1[:, None]))


def rays(oracle, texels, xs, ys, frames, bias=DEFAULT_BIAS):
    """texels: (H, W) BAKE_TEXEL records. The bake rays of texels (xs, ys) at `frames`: dict(org, raw, d: (n, 3) float32; rng: (n,)
    uint32; covered: (n,) bool). An uncovered texel's entries are zeros."""
    xs, ys, frames = (np.asarray(a, np.uint32).ravel() for a in (xs, ys, frames))
    n = len(xs)
    rec = texels[ys.astype(np.int64), xs.astype(np.int64)]
    pos, nrm, cov = np.asarray(rec["position"], f32), np.asarray(rec["normal"], f32), rec["covered"] != 0
    draws, states = np.zeros((n, 2), f32), np.zeros((n, 2), np.uint32)
    for i, (x, y, f) in enumerate(zip(xs, ys, frames)):
        states[i], _, draws[i] = oracle.rand(oracle.seed(int(x), int(y), int(f)), 2)
    r1, r2 = draws[:, 0], draws[:, 1]
    with np.errstate(all="ignore"):
        nn = normalize3(nrm)
        sp, cp = _sincos(oracle, (f32(2) * PI) * r1)
        z, sr = np.sqrt(f32(1) - r2), np.sqrt(r2)
        T, B = construct_tbn(nn)
        raw = lincomb3(T, cp * sr, B, sp * sr, nn, z)
        org = _fma(raw, f32(bias), pos)
        d = normalize3(raw)
    assert all(a.dtype == f32 for a in (nn, sp, z, sr, T, B, raw, org, d))
    zero = ~cov
    raw[zero], org[zero], d[zero] = 0, 0, 0
    return dict(org=org, raw=raw, d=d, rng=np.where(cov, states[:, 1], 0).astype(np.uint32), covered=cov)


def covered_list(texels):
    """texel indices y * W + x of the covered texels, ascending"""
    return np.flatnonzero(np.asarray(texels["covered"]).ravel() != 0).astype(np.uint32)


NEIGHBOURS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def dilate(out, covered, passes):
    """out: (H, W, 4) float32, the output buffer; covered: (H, W) bool. The (H, W, 4) result: rgb, and w = 1 covered, 2 filled, 0
    empty. A pass reads only what stood before it: state-0 texels sum the rgb of the neighbours whose state is non-zero, in the order
    NEIGHBOURS, in float32 from +0, and divide by their number."""
    out, covered = np.asarray(out, f32), np.asarray(covered, bool)
    H, W = covered.shape
    res = np.zeros((H, W, 4), f32)
    res[covered, :3], res[covered, 3] = out[covered, :3], 1
    for _ in range(passes):
        src = np.zeros((H + 2, W + 2, 4), f32)
        src[1:-1, 1:-1] = res
        total, count = np.zeros((H, W, 3), f32), np.zeros((H, W), np.uint32)
        for dy, dx in NEIGHBOURS:
            nb = src[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            take = nb[..., 3] != 0
            with np.errstate(all="ignore"):
                total = np.where(take[..., None], total + nb[..., :3], total).astype(f32)
            count += take
        fill = (res[..., 3] == 0) & (count > 0)
        with np.errstate(all="ignore"):
            mean = (total / np.maximum(count, 1).astype(f32)[..., None]).astype(f32)
        res[fill, :3], res[fill, 3] = mean[fill], 2
    return res


def rasterise(positions, normals, uvs, W, H):
    """(covered (H, W) bool, position (H, W, 3) float32, normal (H, W, 3) float32, triangle (H, W) int, -1 where uncovered): texel
    (x, y) belongs to the first triangle whose three barycentrics at ((x + 0.5) / W, (y + 0.5) / H) are all >= 0"""
    P, N, UV = (np.asarray(a, np.float64) for a in (positions, normals, uvs))
    cov, tri = np.zeros((H, W), bool), np.full((H, W), -1, np.int64)
    pos, nrm = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
    for y in range(H):
        for x in range(W):
            px, py = (x + 0.5) / W, (y + 0.5) / H
            for t in range(len(UV)):
                (ax, ay), (bx, by), (cx, cy) = ((float(u), float(v)) for u, v in UV[t])
                den = (by - cy) * (ax - cx) + (cx - bx) * (ay - cy)
                if den == 0.0:
                    continue
                w0 = ((by - cy) * (px - cx) + (cx - bx) * (py - cy)) / den
                w1 = ((cy - ay) * (px - cx) + (ax - cx) * (py - cy)) / den
                w2 = (1.0 - w0) - w1
                if w0 >= 0 and w1 >= 0 and w2 >= 0:
                    cov[y, x], tri[y, x] = True, t
                    pos[y, x] = [(w0 * float(P[t, 0, k]) + w1 * float(P[t, 1, k])) + w2 * float(P[t, 2, k]) for k in range(3)]
                    nrm[y, x] = [(w0 * float(N[t, 0, k]) + w1 * float(N[t, 1, k])) + w2 * float(N[t, 2, k]) for k in range(3)]
                    break
    return cov, pos, nrm, tri
