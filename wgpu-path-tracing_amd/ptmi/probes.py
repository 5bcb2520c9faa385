"""Light probes on the host (include/ptmi.h ptmi_upload_probes): where the probes of a lattice stand and how large their atlas is.
host/probes.js states the same rules operation by operation and gives the same bytes.

grid(lo, hi, counts): probes at the cell centres of an nx x ny x nz lattice over the box [lo, hi]. Probe (ix, iy, iz) is record
(iz * ny + iy) * nx + ix, and along each axis, in float64 and rounded once to float32,
    position = lo + (hi - lo) * ((i + 0.5) / n)
atlas_size(count, tile): the most nearly square atlas that holds `count` tiles: cols = the smallest integer with cols * cols >= count,
rows = ceil(count / cols), in integers; (width, height) = (cols * tile, rows * tile). Probe i owns tile (i % cols, i // cols).
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
