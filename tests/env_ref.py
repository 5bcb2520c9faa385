"""The environment map (include/ptmi.h ptmi_upload_environment) restated in numpy float64, sharing no code with the library: the
sampling weights and probabilities, c_t, the lookup of a direction and the sampling step on given uniforms."""
import numpy as np

EPS = 1e-6
# A direction whose u W or v H lies this close to a whole number, in texels, may read either texel: which one is the device's atan2f /
# acosf's to decide (outside the arithmetic contract). Tests set such lookups aside.
BORDER_BAND = 1e-4


def weights(texels):
    """(w_t, P_t, c_t, sum(w)) of an (H, W, >=3) map; P and c are zeros for an all-black map"""
    t = np.asarray(texels, np.float64)
    H, W = t.shape[:2]
    lum = 0.2126 * t[..., 0] + 0.7152 * t[..., 1] + 0.0722 * t[..., 2]
    edge = np.cos(np.pi * np.arange(H + 1) / H)
    w = lum * (edge[:-1] - edge[1:])[:, None]
    total = float(w.sum())
    P = w / total if total > 0 else np.zeros_like(w)
    return w, P, P * (W * H) / (2.0 * np.pi ** 2), total


def uv_of(d, rotation=0.0):
    """(u W-independent u in [0, 1), v in [0, 1]) of unit directions (n, 3)"""
    d = np.asarray(d, np.float64)
    u = (np.arctan2(d[:, 2], d[:, 0]) - float(np.float32(rotation))) / (2.0 * np.pi) + 0.5
    return u - np.floor(u), np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi


def lookup(texels, d, intensity=1.0, rotation=0.0):
    """(texel index, Le (n, 3) as float32 products, pdf (n,) float64, u W, v H) of unit directions (n, 3)"""
    t32 = np.asarray(texels).astype(np.float32)
    H, W = t32.shape[:2]
    d = np.asarray(d, np.float64)
    u, v = uv_of(d, rotation)
    x = np.minimum(np.floor(u * W).astype(np.int64), W - 1)
    y = np.minimum(np.floor(v * H).astype(np.int64), H - 1)
    c = weights(texels)[2]
    le = t32[y, x, :3] * np.float32(intensity)
    pdf = c[y, x] / np.maximum(np.sqrt(np.maximum(0.0, 1.0 - d[:, 1] ** 2)), EPS)
    return y * W + x, le, pdf, u * W, v * H


def sample(texels, prob, alias, r, rotation=0.0):
    """the sampling step on uniforms r (n, 4) float32 with the alias table (prob float32, alias) as given:
    (texel, direction (n, 3) float64, density (n,) float64)"""
    H, W = np.asarray(texels).shape[:2]
    N = W * H
    r32 = np.asarray(r, np.float32)
    k = np.minimum((r32[:, 0] * np.float32(N)).astype(np.int64), N - 1)      # the float32 product the kernel truncates
    t = np.where(r32[:, 1] < np.asarray(prob, np.float32)[k], k, np.asarray(alias, np.int64)[k])
    r = r32.astype(np.float64)
    u, v = (t % W + r[:, 2]) / W, (t // W + r[:, 3]) / H
    theta, phi = v * np.pi, (u - 0.5) * 2.0 * np.pi + float(np.float32(rotation))
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], -1)
    c = weights(texels)[2].reshape(-1)
    return t, d, c[t] / np.maximum(np.sin(theta), EPS)


def texel_centres(W, H, rotation=0.0):
    """the unit directions (H * W, 3) float32 of every texel's centre, in texel order"""
    y, x = np.divmod(np.arange(W * H), W)
    theta, phi = (y + 0.5) / H * np.pi, ((x + 0.5) / W - 0.5) * 2.0 * np.pi + float(np.float32(rotation))
    return np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], -1).astype(np.float32)
