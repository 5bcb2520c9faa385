"""Probe visibility (include/ptmi.h ptmi_set_probe_depth, ptmi_probe_visibility) restated in numpy, sharing no code with the kernels
(csrc/pipeline.hip fold_probe_depth, csrc/probes.hip k_probe_visibility). The tables, the tiles of an atlas and the sum a wave forms
are tests/probe_ref.py's; the running mean is tests/adaptive_ref.py's.

  fold()           one frame's first hits (t, triangle) into the listed texels of the depth plane
  fold_rays()      ... with the first hits taken from the oracle on the model's probe rays
  visibility()     the m x m visibility tile of every probe, in float32: 64 lanes take texels l, l + 64, ..., then the butterfly, then
                   the three divisions
  border_source()  the interior texel every texel of a bordered tile copies, from the table of include/ptmi.h, written out case by case
  add_border()     the bordered tiles by that table
"""
import numpy as np

import probe_ref
from adaptive_ref import _mix
from scene_update_ref import fmaf

f32 = np.float32
MISS = np.uint32(0xFFFFFFFF)


def fold(texels, t, tri, max_distance, frame):
    """texels: (n, 4) float32, the listed texels of the plane as they stand; t (n,) float32 and tri (n,) uint32: the first hit of each
    texel's path at `frame` (tri 0xFFFFFFFF: a miss). Returns the (n, 4) texels after the fold."""
    texels, t, md = np.asarray(texels, f32), np.asarray(t, f32), f32(max_distance)
    hit = np.asarray(tri, np.uint32) != MISS
    d = np.where(hit, np.fmin(t, md), md).astype(f32)
    x = np.stack([d, d * d, hit.astype(f32)], axis=1)
    assert x.dtype == f32
    if frame > 0:
        x = _mix(texels[:, :3], x, f32(1) / f32(frame + 1))
    out = np.zeros((len(t), 4), f32)
    out[:, :3] = x
    return out


def first_hits(oracle, scene, probes, N, W, H, frame):
    """(t, tri, list): Oracle.intersect on the model's probe ray of every listed texel at `frame`, ascending texels"""
    lst = probe_ref.texel_list(probes, N, W, H)
    ys, xs = np.divmod(lst, np.uint32(W))
    m = probe_ref.rays(oracle, probes, N, W, xs, ys, np.full(len(lst), frame, np.uint32))
    assert m["enabled"].all()
    t, tri = oracle.intersect(scene, m["org"], m["d"])[:2]
    return t, tri, lst.astype(np.int64)


def fold_rays(oracle, scene, probes, N, plane, max_distance, frame):
    """the (H, W, 4) plane after one frame of a probe dispatch; returns (plane, t, tri, list)"""
    H, W = plane.shape[:2]
    t, tri, lst = first_hits(oracle, scene, probes, N, W, H, frame)
    out = np.array(plane, f32).reshape(-1, 4)
    out[lst] = fold(out[lst], t, tri, max_distance, frame)
    return out.reshape(H, W, 4), t, tri, lst


def weights(N, m, s):
    """(m * m, N * N) float32: the lobe weight of tile texel t in output texel j"""
    dir_dw = probe_ref.tables(N)[0]
    nrm = probe_ref.tables(m)[0][:, :3]
    d, dw = dir_dw[:, :3], dir_dw[:, 3]
    c = fmaf(nrm[:, None, 2], d[None, :, 2], fmaf(nrm[:, None, 1], d[None, :, 1], nrm[:, None, 0] * d[None, :, 0]))
    p = np.where(c > 0, c, f32(0)).astype(f32)
    with np.errstate(all="ignore"):
        for _ in range(s):
            p = p * p
        wgt = p * dw[None, :]
    assert wgt.dtype == f32
    return wgt


def sums(plane, probes, N, m, s):
    """(count, m * m, 4) float32: a0 ... a3 of every output texel after the butterfly (zeros for a disabled probe)"""
    wgt = weights(N, m, s)
    D = probe_ref.tiles(plane, probes, N)
    res = np.zeros((len(probes), m * m, 4), f32)
    with np.errstate(all="ignore"):
        for i in range(len(probes)):
            if probes["enabled"][i]:
                terms = np.concatenate([wgt[:, :, None] * D[i][None, :, :], wgt[:, :, None]], axis=2)      # (m * m, T, 4)
                res[i] = probe_ref.wave_sum(terms)
    return res


def visibility(plane, probes, N, m, s, border=0):
    """(count, side, side, 4) float32, side = m + 2 * border"""
    a = sums(plane, probes, N, m, s)
    res = np.zeros((len(probes), m * m, 4), f32)
    with np.errstate(all="ignore"):
        for i in range(len(probes)):
            if probes["enabled"][i]:
                res[i, :, :3], res[i, :, 3] = a[i, :, :3] / a[i, :, 3:4], 1
    assert res.dtype == f32
    res = res.reshape(len(probes), m, m, 4)
    return add_border(res, m) if border else res


def border_source(x, y, m):
    """the interior texel (sx, sy) that texel (x, y) of the bordered tile copies; x, y in interior coordinates, -1 ... m"""
    e = m - 1
    if x == -1 and y == -1:
        return e, e
    if x == m and y == -1:
        return 0, e
    if x == -1 and y == m:
        return e, 0
    if x == m and y == m:
        return 0, 0
    if x == -1:
        return 0, e - y
    if x == m:
        return e, e - y
    if y == -1:
        return e - x, 0
    if y == m:
        return e - x, e
    return x, y


def add_border(tiles, m):
    tiles = np.asarray(tiles)
    out = np.zeros((len(tiles), m + 2, m + 2, 4), tiles.dtype)
    for y in range(-1, m + 1):
        for x in range(-1, m + 1):
            sx, sy = border_source(x, y, m)
            out[:, y + 1, x + 1] = tiles[:, sy, sx]
    return out
