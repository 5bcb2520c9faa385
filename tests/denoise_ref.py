"""A plain float32 restatement of the denoiser (include/ptmi.h ptmi_denoise) and of the sample-moments fold (ptmi_set_moments),
written from their definitions in numpy and sharing no code with the kernels.

Every float32 operation is written in the order the definitions give, the order csrc/denoise.hip evaluates them in (the library
builds without FMA contraction), so the restatement differs from the kernels only where exp and pow round differently.

  moments   per frame l = 0.2126 r + 0.7152 g + 0.0722 b of the radiance clamped at 2.5 per channel (fmin: NaN -> 2.5), folded with
            the output buffer's rule into (mean l, mean l^2, frames, 0); the FMA of mix() is emulated in float64.
  prepass   guide = (normal / |normal| or 0, depth = normal.w), grad = max |depth - neighbour depth| over the 4-neighbours inside the
            image, cv = (colour, max(0, E[l^2] - E[l]^2) / max(frames, 1)); demodulated where albedo.w > 0: colour / max(albedo,
            1e-3), variance / max(l(albedo), 1e-3)^2.
  pass i    5x5 taps h = (1/16, 1/4, 3/8, 1/4, 1/16) at offsets k 2^i; w = h_y h_x w_n w_z w_l, w_n = max(0, n_p . n_q)^phi_n,
            w_z = exp(-|z_p - z_q| / (phi_z |offset| grad_p + 1e-6)), w_l = exp(-|l_p - l_q| / (phi_c sqrt(g3x3(var)_p) + 1e-6)).
            Taps outside the image, non-finite or with a zero normal are skipped; the centre weighs h0^2; a non-finite or missed
            (zero-normal) centre keeps its value. g3x3 = (1/4, 1/8, 1/16) Gaussian over the finite in-image taps / their weight sum.
  last pass remodulates with max(albedo, 1e-3) where albedo.w > 0 and writes (rgb, 0).
"""
import numpy as np

f32 = np.float32
H_B3 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
DEFAULTS = dict(iterations=5, phi_color=4.0, phi_normal=128.0, phi_depth=1.0)


def lum(r, g, b):
    return f32(0.2126) * r + f32(0.7152) * g + f32(0.0722) * b


def _mix(a, b, t):
    """mix(a, b, t) = fma(b, t, a * (1 - t)) in float32, the FMA in float64 then rounded (b t is exact in float64)"""
    t = f32(t)
    p = a * (f32(1) - t)
    return (b.astype(np.float64) * np.float64(t) + p.astype(np.float64)).astype(np.float32)


def fold_moments(per_frame, frames, acc=None):
    """per_frame: list of (n, 3) float32 per-path radiances (unclamped), one per frame in `frames` (ascending).
    acc: the plane before (n, 4), or None for zeros. Returns the (n, 4) float32 moments plane."""
    acc = np.zeros((len(per_frame[0]), 4), np.float32) if acc is None else np.array(acc, np.float32)
    for L, f in zip(per_frame, frames):
        c = np.fmin(np.asarray(L, np.float32), f32(2.5))
        l = lum(c[:, 0], c[:, 1], c[:, 2])
        m1, m2 = l, l * l
        if f > 0:
            t = f32(1) / f32(f + 1)
            m1, m2 = _mix(acc[:, 0], m1, t), _mix(acc[:, 1], m2, t)
        acc = np.stack([m1, m2, np.full_like(m1, f32(f + 1)), np.zeros_like(m1)], axis=1).astype(np.float32)
    return acc


def _shift(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx] where inside the image (else 0) and the mask of where it is"""
    H, W = a.shape[:2]
    b = np.zeros_like(a)
    m = np.zeros((H, W), bool)
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[yd, xd] = a[ys, xs]
        m[yd, xd] = True
    return b, m


def _finite4(a):
    return np.isfinite(a).all(axis=-1)


def prepass(radiance, normal, albedo, moments):
    """(H, W, 4) float32 planes (albedo None: no demodulation) -> guide (H, W, 4), grad (H, W), cv (H, W, 4)"""
    n = np.asarray(normal, np.float32)
    len2 = n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2]
    g = np.zeros_like(n)
    g[..., 3] = n[..., 3]
    hit = len2 > 0
    ln = np.sqrt(len2[hit])
    for k in range(3):
        g[..., k][hit] = n[..., k][hit] / ln
    z = n[..., 3]
    dz = np.zeros_like(z)
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        zq, m = _shift(z, dy, dx)
        dz = np.where(m, np.fmax(dz, np.abs(z - zq)), dz)
    c = np.asarray(radiance, np.float32)
    mo = np.asarray(moments, np.float32)
    cv = np.empty_like(c)
    cv[..., :3] = c[..., :3]
    cv[..., 3] = np.fmax(f32(0), mo[..., 1] - mo[..., 0] * mo[..., 0]) / np.fmax(mo[..., 2], f32(1))
    if albedo is not None:
        a = np.asarray(albedo, np.float32)
        cov = a[..., 3] > 0
        for k in range(3):
            cv[..., k] = np.where(cov, cv[..., k] / np.fmax(a[..., k], f32(1e-3)), cv[..., k])
        la = np.fmax(lum(a[..., 0], a[..., 1], a[..., 2]), f32(1e-3))
        cv[..., 3] = np.where(cov, cv[..., 3] / (la * la), cv[..., 3])
    return g, dz, cv


def atrous_pass(guide, grad, src, step, phi_c, phi_n, phi_z, last=False, albedo=None):
    """one pass; last: remodulate with albedo (None: none) and write w = 0"""
    phi_c, phi_n, phi_z = f32(phi_c), f32(phi_n), f32(phi_z)
    cp, gp = src, guide
    active = _finite4(cp) & ((gp[..., 0] != 0) | (gp[..., 1] != 0) | (gp[..., 2] != 0))
    sv = np.zeros(cp.shape[:2], np.float32)
    sk = np.zeros(cp.shape[:2], np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            q, m = _shift(src, dy, dx)
            ok = m & _finite4(q)
            k = (f32(0.5) if dy == 0 else f32(0.25)) * (f32(0.5) if dx == 0 else f32(0.25))
            sv = np.where(ok, sv + k * q[..., 3], sv)
            sk = np.where(ok, sk + k, sk)
    lp = lum(cp[..., 0], cp[..., 1], cp[..., 2])
    den_l = phi_c * np.sqrt(sv / np.where(sk > 0, sk, f32(1))) + f32(1e-6)
    w0 = H_B3[2] * H_B3[2]
    sw = np.full(cp.shape[:2], w0, np.float32)
    s = [w0 * cp[..., k] for k in range(3)]
    s2 = w0 * w0 * cp[..., 3]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx == 0 and dy == 0:
                continue
            q, m = _shift(src, dy * step, dx * step)
            gq, _ = _shift(guide, dy * step, dx * step)
            ok = m & _finite4(q) & ((gq[..., 0] != 0) | (gq[..., 1] != 0) | (gq[..., 2] != 0))
            wn = np.power(np.fmax(f32(0), gp[..., 0] * gq[..., 0] + gp[..., 1] * gq[..., 1] + gp[..., 2] * gq[..., 2]), phi_n)
            off = f32(step) * np.sqrt(f32(dx * dx + dy * dy))
            wz = np.exp(-np.abs(gp[..., 3] - gq[..., 3]) / (phi_z * off * grad + f32(1e-6)))
            wl = np.exp(-np.abs(lp - lum(q[..., 0], q[..., 1], q[..., 2])) / den_l)
            w = H_B3[dy + 2] * H_B3[dx + 2] * wn * wz * wl
            ok &= active
            sw = np.where(ok, sw + w, sw)
            for k in range(3):
                s[k] = np.where(ok, s[k] + w * q[..., k], s[k])
            s2 = np.where(ok, s2 + w * w * q[..., 3], s2)
    out = np.array(cp, np.float32)
    filt = np.stack([s[0] / sw, s[1] / sw, s[2] / sw, s2 / (sw * sw)], axis=-1)
    out[active] = filt[active]
    if last:
        if albedo is not None:
            a = np.asarray(albedo, np.float32)
            cov = a[..., 3] > 0
            for k in range(3):
                out[..., k] = np.where(cov, out[..., k] * np.fmax(a[..., k], f32(1e-3)), out[..., k])
        out[..., 3] = 0
    return out.astype(np.float32)


def denoise(radiance, normal, albedo, moments, iterations=0, demodulate=True, phi_color=0.0, phi_normal=0.0, phi_depth=0.0):
    """ptmi_denoise on (H, W, 4) float32 planes; albedo is used only with demodulate. 0 picks a parameter's default."""
    it = iterations or DEFAULTS["iterations"]
    pc = phi_color or DEFAULTS["phi_color"]
    pn = phi_normal or DEFAULTS["phi_normal"]
    pz = phi_depth or DEFAULTS["phi_depth"]
    alb = albedo if demodulate else None
    with np.errstate(all="ignore"):
        guide, grad, cv = prepass(radiance, normal, alb, moments)
        for i in range(it):
            cv = atrous_pass(guide, grad, cv, 1 << i, pc, pn, pz, last=i + 1 == it, albedo=alb)
    return cv
