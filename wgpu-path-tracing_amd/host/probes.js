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
 * maxDistance(lo, hi, counts) -> the default clamp of the probe depth plane (ptmi_set_probe_depth) for that lattice, 1.5 times the
 *   cell diagonal (DDGI's convention): with c = (hi - lo) / n along each axis, in doubles, rounded once by Math.fround,
 *     1.5 * sqrt((cx * cx + cy * cy) + cz * cz)
 * addBorder(tiles, m) -> Float32Array: count tiles of m x m x 4 floats (ptmi_probe_irradiance's, or ptmi_probe_visibility's with
 *   border = 0) with the ring of texels a bilinear tap needs across the edge of the octahedral square: (m + 2) x (m + 2) x 4 each,
 *   interior texel (x, y) at (x + 1, y + 1). A pure index permutation, the table of include/ptmi.h: with e = m - 1,
 *     (-1, y) <- (0, e - y)    (m, y) <- (e, e - y)    (x, -1) <- (e - x, 0)    (x, m) <- (e - x, e)
 *     corners (-1, -1) <- (e, e)   (m, -1) <- (0, e)   (-1, m) <- (e, 0)   (m, m) <- (0, 0)
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

function maxDistance(lo, hi, counts) {
  var cx = (hi[0] - lo[0]) / counts[0], cy = (hi[1] - lo[1]) / counts[1], cz = (hi[2] - lo[2]) / counts[2];
  return Math.fround(1.5 * Math.sqrt((cx * cx + cy * cy) + cz * cz));
}

// the interior texel that texel (x, y) of the bordered tile copies, x and y in interior coordinates (-1 ... m)
function borderSource(x, y, m) {
  var e = m - 1, outX = x < 0 || x > e, outY = y < 0 || y > e;
  if (outX && outY) return [x < 0 ? e : 0, y < 0 ? e : 0];
  if (outX) return [x < 0 ? 0 : e, e - y];
  if (outY) return [e - x, y < 0 ? 0 : e];
  return [x, y];
}

function addBorder(tiles, m) {
  var side = m + 2, count = Math.floor(tiles.length / (m * m * 4));
  var out = new Float32Array(count * side * side * 4);
  for (var i = 0; i < count; i++)
    for (var y = -1; y <= m; y++)
      for (var x = -1; x <= m; x++) {
        var s = borderSource(x, y, m);
        var from = ((i * m + s[1]) * m + s[0]) * 4, to = ((i * side + y + 1) * side + x + 1) * 4;
        out[to] = tiles[from]; out[to + 1] = tiles[from + 1]; out[to + 2] = tiles[from + 2]; out[to + 3] = tiles[from + 3];
      }
  return out;
}

module.exports = { grid: grid, atlasSize: atlasSize, records: records, maxDistance: maxDistance, addBorder: addBorder };
