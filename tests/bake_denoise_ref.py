"""A plain float32 restatement of the lightmap filter (include/ptmi.h ptmi_bake_denoise), written from its definition in numpy and
sharing no code with the kernels (csrc/bake_denoise.hip). The gutter fill that follows the filter is bake_ref's dilate model.

Every float32 operation is written in the order the kernels' header gives, and the library builds without FMA contraction, so the
restatement differs from the kernels only where exp and pow round differently.

  prepass   uncovered: guides and cv are zero. Covered: n^ = normal / sqrt(nx nx + ny ny + nz nz) per component; the footprint f = the
            smallest non-zero |P - P_q| over the covered 4-neighbours inside the map (order x - 1, x + 1, y - 1, y + 1; 0 if none);
            guide N = (n^, f), guide P = (P, 1), cv = (R.rgb, max(0, M.y - M.x M.x) / max(M.z, 1)).
  pass i    a covered centre with a finite cv takes the 24 taps at offsets (dx, dy) 2^i, dy outer, that are inside the map, covered and
            finite: w = h_y h_x w_n w_x w_l, w_n = max(0, n^_p . n^_q)^phi_n, w_x = exp(-e / (phi_x f_p + 1e-6)) with
            e = max(|n^_p . D|, |D| - S off f_p), D = P_q - P_p, off = 2^i sqrt(dx dx + dy dy), S = 4,
            w_l = exp(-|l_p - l_q| / (phi_c sqrt(g3x3(var)_p) + 1e-6)); colour = sum w c / sum w, var = sum w^2 var / (sum w)^2, the
            centre weighing h0^2. g3x3 = (1/4, 1/8, 1/16) Gaussian over the covered finite in-map 3x3 texels / their weight sum.
            A covered centre that is not finite keeps its value; uncovered texels hold zeros throughout.
  last pass (rgb, 1) for covered texels, zeros for the others.
"""
import numpy as np

import bake_ref
from denoise_ref import H_B3, _finite4, _shift, lum

f32 = np.float32
STRETCH = f32(4)
DEFAULTS = dict(iterations=5, phi_color=4.0, phi_normal=128.0, phi_position=1.0)


def _len3(x, y, z):
    return np.sqrt(x * x + y * y + z * z)


def _nonzero3(g):
    return (g[..., 0] != 0) | (g[..., 1] != 0) | (g[..., 2] != 0)


def prepass(texels, radiance, moments):
    """texels: (H, W) BAKE_TEXEL records; radiance, moments: (H, W, 4) float32 -> guide N, guide P, cv, (H, W, 4) each. Nothing of an
    uncovered texel is used."""
    cov = np.asarray(texels["covered"]) != 0
    P = np.where(cov[..., None], np.asarray(texels["position"], f32), f32(0)).astype(f32)
    n = np.where(cov[..., None], np.asarray(texels["normal"], f32), f32(0)).astype(f32)
    H, W = cov.shape
    gn, gp, cv = (np.zeros((H, W, 4), f32) for _ in range(3))
    ln = _len3(n[..., 0], n[..., 1], n[..., 2])
    for k in range(3):
        gn[..., k][cov] = n[..., k][cov] / ln[cov]
    f = np.zeros((H, W), f32)
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        Pq, m = _shift(P, dy, dx)
        cq, _ = _shift(cov, dy, dx)
        d = _len3(P[..., 0] - Pq[..., 0], P[..., 1] - Pq[..., 1], P[..., 2] - Pq[..., 2])
        take = m & cq & cov & (d > 0) & ((f == 0) | (d < f))
        f = np.where(take, d, f)
    gn[..., 3] = f
    gp[..., :3], gp[..., 3] = P, cov
    c, mo = np.asarray(radiance, f32), np.asarray(moments, f32)
    var = np.fmax(f32(0), mo[..., 1] - mo[..., 0] * mo[..., 0]) / np.fmax(mo[..., 2], f32(1))
    for k in range(3):
        cv[..., k][cov] = c[..., k][cov]
    cv[..., 3][cov] = var[cov]
    return gn, gp, cv


def atrous_pass(gn, gp, src, step, phi_c, phi_n, phi_x, last=False):
    phi_c, phi_n, phi_x = f32(phi_c), f32(phi_n), f32(phi_x)
    cov = _nonzero3(gn)
    cp = src
    active = cov & _finite4(cp)
    sv, sk = np.zeros(cov.shape, f32), np.zeros(cov.shape, f32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            q, m = _shift(src, dy, dx)
            cq, _ = _shift(cov, dy, dx)
            ok = m & cq & _finite4(q)
            k = (f32(0.5) if dy == 0 else f32(0.25)) * (f32(0.5) if dx == 0 else f32(0.25))
            sv = np.where(ok, sv + k * q[..., 3], sv)
            sk = np.where(ok, sk + k, sk)
    lp = lum(cp[..., 0], cp[..., 1], cp[..., 2])
    den_l = phi_c * np.sqrt(sv / np.where(sk > 0, sk, f32(1))) + f32(1e-6)
    fp = gn[..., 3]
    den_x = phi_x * fp + f32(1e-6)
    w0 = H_B3[2] * H_B3[2]
    sw = np.full(cov.shape, w0, f32)
    s = [w0 * cp[..., k] for k in range(3)]
    s2 = w0 * w0 * cp[..., 3]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx == 0 and dy == 0:
                continue
            q, m = _shift(src, dy * step, dx * step)
            gq, _ = _shift(gn, dy * step, dx * step)
            pq, _ = _shift(gp, dy * step, dx * step)
            ok = active & m & _nonzero3(gq) & _finite4(q)
            wn = np.power(np.fmax(f32(0), gn[..., 0] * gq[..., 0] + gn[..., 1] * gq[..., 1] + gn[..., 2] * gq[..., 2]), phi_n)
            ex, ey, ez = pq[..., 0] - gp[..., 0], pq[..., 1] - gp[..., 1], pq[..., 2] - gp[..., 2]
            dist = _len3(ex, ey, ez)
            plane = np.abs(gn[..., 0] * ex + gn[..., 1] * ey + gn[..., 2] * ez)
            off = f32(step) * np.sqrt(f32(dx * dx + dy * dy))
            e = np.fmax(plane, dist - STRETCH * off * fp)
            wx = np.exp(-e / den_x)
            wl = np.exp(-np.abs(lp - lum(q[..., 0], q[..., 1], q[..., 2])) / den_l)
            w = H_B3[dy + 2] * H_B3[dx + 2] * wn * wx * wl
            sw = np.where(ok, sw + w, sw)
            for k in range(3):
                s[k] = np.where(ok, s[k] + w * q[..., k], s[k])
            s2 = np.where(ok, s2 + w * w * q[..., 3], s2)
    out = np.array(cp, f32)
    filt = np.stack([s[0] / sw, s[1] / sw, s[2] / sw, s2 / (sw * sw)], axis=-1)
    out[active] = filt[active]
    if last:
        out[..., 3] = 1
    out[~cov] = 0
    assert out.dtype == f32
    return out


def denoise(texels, radiance, moments, iterations=0, dilate=0, phi_color=0.0, phi_normal=0.0, phi_position=0.0):
    """ptmi_bake_denoise on an (H, W) surface and (H, W, 4) float32 planes; 0 picks a parameter's default. The (H, W, 4) result: rgb,
    and w = 1 covered, 2 filled by a gutter pass, 0 empty."""
    it = iterations or DEFAULTS["iterations"]
    pc = phi_color or DEFAULTS["phi_color"]
    pn = phi_normal or DEFAULTS["phi_normal"]
    px = phi_position or DEFAULTS["phi_position"]
    with np.errstate(all="ignore"):
        gn, gp, cv = prepass(texels, radiance, moments)
        for i in range(it):
            cv = atrous_pass(gn, gp, cv, 1 << i, pc, pn, px, last=i + 1 == it)
    cov = np.asarray(texels["covered"]) != 0
    return bake_ref.dilate(cv, cov, dilate) if dilate else cv
