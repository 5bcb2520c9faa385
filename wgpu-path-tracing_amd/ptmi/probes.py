"""Light probes on the host (include/ptmi.h ptmi_upload_probes): where the probes of a lattice stand and how large their atlas is.
host/probes.js states the same rules operation by operation and gives the same bytes.

grid(lo, hi, counts): probes at the cell centres of an nx x ny x nz lattice over the box [lo, hi]. Probe (ix, iy, iz) is record
(iz * ny + iy) * nx + ix, and along each axis, in float64 and rounded once to float32,
    position = lo + (hi - lo) * ((i + 0.5) / n)
atlas_size(count, tile): the most nearly square atlas that holds `count` tiles: cols = the smallest integer with cols * cols >= count,
rows = ceil(count / cols), in integers; (width, height) = (cols * tile, rows * tile). Probe i owns tile (i % cols, i // cols).
max_distance(lo, hi, counts): the default clamp of the probe depth plane (ptmi_set_probe_depth) for that lattice, 1.5 times the cell
diagonal (DDGI's convention): with c = (hi - lo) / n along each axis, in float64 and rounded once to float32,
    1.5 * sqrt((cx * cx + cy * cy) + cz * cz)
add_border(tiles, m): (count, m, m, 4) octahedral tiles (ptmi_probe_irradiance's, or ptmi_probe_visibility's with border = 0) with
the ring of texels a bilinear tap needs across the edge of the octahedral square: (count, m + 2, m + 2, 4), interior texel (x, y) at
(x + 1, y + 1). A pure index permutation, the table of include/ptmi.h: with e = m - 1,
    (-1, y) <- (0, e - y)    (m, y) <- (e, e - y)    (x, -1) <- (e - x, 0)    (x, m) <- (e - x, e)
    corners (-1, -1) <- (e, e)   (m, -1) <- (0, e)   (-1, m) <- (e, 0)   (m, m) <- (0, 0)
"""
import numpy as np

from . import layout


def grid(lo, hi, counts):
    """(nx * ny * nz, 3) float32 positions, x fastest"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    nx, ny, nz = (int(n) for n in counts)
    assert nx > 0 and ny > 0 and nz > 0
    axes = [lo[k] + (hi[k] - lo[k]) * ((np.arange(n, dtype=np.float64) + 0.5) / n) for k, n in enumerate((nx, ny, nz))]
    out = np.zeros((nz, ny, nx, 3), np.float32)
    out[..., 0], out[..., 1], out[..., 2] = axes[0][None, None, :], axes[1][None, :, None], axes[2][:, None, None]
    return out.reshape(-1, 3)


def atlas_size(count, tile):
    """(width, height) of the atlas for `count` probes with tile x tile tiles"""
    count, tile = int(count), int(tile)
    assert count > 0 and tile > 0
    cols = 1
    while cols * cols < count:
        cols += 1
    rows = (count + cols - 1) // cols
    return cols * tile, rows * tile


def records(positions, enabled=None):
    """layout.PROBE records of Context.upload_probes from (n, 3) positions; enabled: (n,) flags (None: every probe)"""
    p = np.asarray(positions, np.float32).reshape(-1, 3)
    rec = np.zeros(len(p), layout.PROBE)
    rec["position"] = p
    rec["enabled"] = 1 if enabled is None else (np.asarray(enabled).ravel() != 0)
    return rec


def max_distance(lo, hi, counts):
    """the float32 default max_distance of set_probe_depth for grid(lo, hi, counts)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    cx, cy, cz = ((hi[k] - lo[k]) / np.float64(int(n)) for k, n in enumerate(counts))
    return np.float32(1.5 * np.sqrt((cx * cx + cy * cy) + cz * cz))


def border_source(m):
    """(sy, sx), each (m + 2, m + 2): the interior texel every texel of a bordered tile copies (an interior texel itself)"""
    e = m - 1
    k = np.arange(-1, m + 1)
    y, x = np.meshgrid(k, k, indexing="ij")
    out_x, out_y = (x < 0) | (x > e), (y < 0) | (y > e)
    sx = np.where(out_x, np.where(x < 0, 0, e), x)
    sy = np.where(out_y, np.where(y < 0, 0, e), y)
    edge_x, edge_y = out_x & ~out_y, out_y & ~out_x
    sy = np.where(edge_x, e - y, sy)                    # (-1, y) <- (0, e - y), (m, y) <- (e, e - y)
    sx = np.where(edge_y, e - x, sx)                    # (x, -1) <- (e - x, 0), (x, m) <- (e - x, e)
    corner = out_x & out_y                              # a corner copies the interior's opposite corner
    sx = np.where(corner, np.where(x < 0, e, 0), sx)
    sy = np.where(corner, np.where(y < 0, e, 0), sy)
    return sy, sx


def add_border(tiles, m):
    """(count, m + 2, m + 2, 4) from (count, m, m, 4): the bytes move, none is computed"""
    t = np.asarray(tiles)
    m = int(m)
    assert t.ndim == 4 and t.shape[1] == m and t.shape[2] == m
    sy, sx = border_source(m)
    return np.ascontiguousarray(t[:, sy, sx, :])
