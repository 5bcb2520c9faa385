"""Light probes (include/ptmi.h ptmi_upload_probes, ptmi_dispatch_probes, ptmi_probe_sh, ptmi_probe_irradiance) restated in numpy,
sharing no code with the kernels (csrc/pipeline.hip probe_ray, csrc/probes.hip) or with the host's table builder:

  rays()         the first ray of a probe path, operation by operation in float32 with the oracle's RNG (pto_seed, pto_rand) and the
                 contract normalize3. Returns org, raw (the direction before normalize3), d and the RNG state. (org, raw) is the ray of
                 the pinhole with position = org, forward = raw, fov = 0, aperture = 0 (projection_ref.fov0_cameras), which is how a
                 probe sample is pinned against the unchanged oracle.
  texel_list()   the texels a probe dispatch walks, in the order it walks them
  tables64()     the octahedral map of the texel centres, the solid angles and the nine SH functions, in float64 with + - * / sqrt only
  tables()       ... rounded once to float32: (d, dw) and basis, as the device reads them
  sh()           SH9 of every probe's tile, in float32: 64 lanes take texels l, l + 64, ..., then the butterfly
  irradiance()   the m x m irradiance tile (E / pi) of every probe, likewise
"""
import numpy as np

from projection_ref import normalize3
from scene_update_ref import fmaf

f32, f64 = np.float32, np.float64
PI64 = 3.141592653589793
INV_PI = f32(0.318309886)
C1, C2, C20, C22 = 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
Y0 = 0.28209479177387814


def fold_octahedral(a, b):
    """(a', b', w) of the map: w = (1 - |a|) - |b|; below the fold (w < 0) a' = copysign(1 - |b|, a), b' = copysign(1 - |a|, b).
    Works in the dtype it is given."""
    one = a.dtype.type(1)
    fa, fb = np.abs(a), np.abs(b)
    w = (one - fa) - fb
    lower = w < 0
    return np.where(lower, np.copysign(one - fb, a), a), np.where(lower, np.copysign(one - fa, b), b), w


def probe_of(N, W, xs, ys):
    return (ys // N) * (W // N) + xs // N


def rays(oracle, probes, N, W, xs, ys, frames):
    """probes: layout.PROBE records of an atlas W texels wide with N x N tiles. The probe rays of texels (xs, ys) at `frames`:
    dict(org, raw, d: (n, 3) float32; rng: (n,) uint32; enabled: (n,) bool). A texel of a disabled probe, or of a tile past the last
    probe, has zeros."""
    xs, ys, frames = (np.asarray(a, np.uint32).ravel() for a in (xs, ys, frames))
    n = len(xs)
    idx = probe_of(N, W, xs.astype(np.int64), ys.astype(np.int64))
    inside = idx < len(probes)
    rec = probes[np.where(inside, idx, 0)]
    on = inside & (rec["enabled"] != 0)
    draws, states = np.zeros((n, 2), f32), np.zeros((n, 2), np.uint32)
    for i, (x, y, f) in enumerate(zip(xs, ys, frames)):
        states[i], _, draws[i] = oracle.rand(oracle.seed(int(x), int(y), int(f)), 2)
    s = f32(2) / f32(N)
    a = ((xs % N).astype(f32) + draws[:, 0]) * s - f32(1)
    b = ((ys % N).astype(f32) + draws[:, 1]) * s - f32(1)
    pa, pb, w = fold_octahedral(a, b)
    raw = np.stack([pa, pb, w], axis=1)
    org = np.array(rec["position"], f32)
    with np.errstate(all="ignore"):
        d = normalize3(raw)
    assert all(v.dtype == f32 for v in (a, b, raw, org, d))
    raw[~on], org[~on], d[~on] = 0, 0, 0
    return dict(org=org, raw=raw, d=d, rng=np.where(on, states[:, 1], 0).astype(np.uint32), enabled=on)


def texel_list(probes, N, W, H):
    """frame indices y * W + x of the texels of the enabled probes' tiles, ascending"""
    ys, xs = np.divmod(np.arange(W * H, dtype=np.int64), W)
    idx = probe_of(N, W, xs, ys)
    on = np.zeros(W * H, bool)
    inside = idx < len(probes)
    on[inside] = probes["enabled"][idx[inside]] != 0
    return np.flatnonzero(on).astype(np.uint32)


def tables64(N):
    """(d (N * N, 3), dw (N * N,), Y (N * N, 9)) in float64, texel t = ty * N + tx"""
    t = np.arange(N * N)
    step = 2.0 / f64(N)
    a, b = ((t % N).astype(f64) + 0.5) * step - 1.0, ((t // N).astype(f64) + 0.5) * step - 1.0
    pa, pb, w = fold_octahedral(a, b)
    ln = np.sqrt((pa * pa + pb * pb) + w * w)
    d = np.stack([pa / ln, pb / ln, w / ln], axis=1)
    dw = (4.0 / (f64(N) * f64(N))) / ((ln * ln) * ln)
    total = f64(0)
    for v in dw:                                                # ascending t, plain additions
        total = total + v
    dw = dw * ((4.0 * PI64) / total)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = np.stack([np.full(N * N, Y0), C1 * y, C1 * z, C1 * x, (C2 * x) * y, (C2 * y) * z, C20 * ((3.0 * z) * z - 1.0), (C2 * x) * z,
                  C22 * (x * x - y * y)], axis=1)
    return d, dw, Y


def tables(N):
    """(dir_dw (N * N, 4), basis (N * N, 9)) float32"""
    d, dw, Y = tables64(N)
    return np.concatenate([d, dw[:, None]], axis=1).astype(f32), (Y * dw[:, None]).astype(f32)


def tiles(out, probes, N):
    """(count, N * N, 3) float32: the rgb of every probe's tile of the (H, W, 4) frame, texel t = ty * N + tx"""
    out = np.asarray(out, f32)
    cols = out.shape[1] // N
    res = np.zeros((len(probes), N * N, 3), f32)
    for i in range(len(probes)):
        x0, y0 = (i % cols) * N, (i // cols) * N
        res[i] = out[y0:y0 + N, x0:x0 + N, :3].reshape(N * N, 3)
    return res


def wave_sum(terms):
    """terms: (..., T, C) float32, T texels. The sum a wave forms: lane l adds terms l, l + 64, ... to +0 in ascending order, then for
    s = 32 ... 1: v[l] = v[l] + v[l + s]. Returns (..., C)."""
    terms = np.asarray(terms, f32)
    T = terms.shape[-2]
    v = np.zeros(terms.shape[:-2] + (64, terms.shape[-1]), f32)
    with np.errstate(all="ignore"):
        for t0 in range(0, T, 64):
            k = min(64, T - t0)
            v[..., :k, :] = v[..., :k, :] + terms[..., t0:t0 + k, :]
        s = 32
        while s:
            v[..., :s, :] = v[..., :s, :] + v[..., s:2 * s, :]
            s //= 2
    assert v.dtype == f32
    return v[..., 0, :]


def sh(out, probes, N):
    """(count, 9, 3) float32; zeros for a disabled probe"""
    _, basis = tables(N)
    L = tiles(out, probes, N)
    res = np.zeros((len(probes), 9, 3), f32)
    with np.errstate(all="ignore"):
        for i in range(len(probes)):
            if probes["enabled"][i]:
                terms = basis[:, :, None] * L[i][:, None, :]                      # (T, 9, 3): rounded products
                res[i] = wave_sum(terms.reshape(N * N, 27)).reshape(9, 3)
    return res


def irradiance(out, probes, N, m):
    """(count, m, m, 4) float32; w = 1 for an enabled probe, whose disabled neighbours are all zeros"""
    dir_dw, _ = tables(N)
    nrm = tables(m)[0][:, :3]
    d, dw = dir_dw[:, :3], dir_dw[:, 3]
    L = tiles(out, probes, N)
    c = fmaf(nrm[:, None, 2], d[None, :, 2], fmaf(nrm[:, None, 1], d[None, :, 1], nrm[:, None, 0] * d[None, :, 0]))
    c = np.where(c > 0, c, f32(0)).astype(f32)
    wgt = c * dw[None, :]                                                           # (m * m, T)
    res = np.zeros((len(probes), m * m, 4), f32)
    with np.errstate(all="ignore"):
        for i in range(len(probes)):
            if probes["enabled"][i]:
                acc = wave_sum(wgt[:, :, None] * L[i][None, :, :])                  # (m * m, 3)
                res[i, :, :3], res[i, :, 3] = acc * INV_PI, 1
    assert wgt.dtype == f32
    return res.reshape(len(probes), m, m, 4)
