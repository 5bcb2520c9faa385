'use strict';
/**
 * probes.js — where the probes of a lattice stand and how large their atlas is (include/ptmi.h ptmi_upload_probes;
 * Renderer.bakeProbes). The rules are ptmi/probes.py's, operation by operation, and give the same bytes. No dependency.
 *
 * grid(lo, hi, counts) -> Float32Array, 3 per probe: the cell centres of an nx x ny x nz lattice over the box [lo, hi]. Probe
 *   (ix, iy, iz) is record (iz * ny + iy) * nx + ix; along each axis, in doubles, rounded once by the Float32Array store,
 *     position = lo + (hi - lo) * ((i + 0.5) / n)
 * atlasSize(count, tile) -> { width, height }: cols = the smallest integer with cols * cols >= count, rows = ceil(count / cols).
 * records(positions, enabled) -> ArrayBuffer of 16-byte ptmi_probe records; enabled: flags per probe (absent: every probe).
 */

function grid(lo, hi, counts) {
  var nx = counts[0], ny = counts[1], nz = counts[2];
  var out = new Float32Array(nx * ny * nz * 3);
  var at = function (k, i, n) { return lo[k] + (hi[k] - lo[k]) * ((i + 0.5) / n); };
  for (var iz = 0; iz < nz; iz++)
    for (var iy = 0; iy < ny; iy++)
      for (var ix = 0; ix < nx; ix++) {
        var p = 3 * ((iz * ny + iy) * nx + ix);
        out[p] = at(0, ix, nx); out[p + 1] = at(1, iy, ny); out[p + 2] = at(2, iz, nz);
      }
  return out;
}

function atlasSize(count, tile) {
  var cols = 1;
  while (cols * cols < count) cols++;
  var rows = Math.floor((count + cols - 1) / cols);
  return { width: cols * tile, height: rows * tile };
}

function records(positions, enabled) {
  var n = Math.floor(positions.length / 3);
  var buf = new ArrayBuffer(n * 16);
  var f = new Float32Array(buf), u = new Uint32Array(buf);
  for (var i = 0; i < n; i++) {
    f[4 * i] = positions[3 * i]; f[4 * i + 1] = positions[3 * i + 1]; f[4 * i + 2] = positions[3 * i + 2];
    u[4 * i + 3] = enabled ? (enabled[i] ? 1 : 0) : 1;
  }
  return buf;
}

module.exports = { grid: grid, atlasSize: atlasSize, records: records };
