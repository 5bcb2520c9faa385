'use strict';
/**
 * bake.js — a mesh's lightmap UVs rasterised into the texel records a bake starts its paths from (include/ptmi.h
 * ptmi_upload_bake_surface; Renderer.bake). The rule is ptmi/bake.py's, operation by operation, and gives the same float32 bits.
 * No dependency.
 *
 * rasterise(positions, normals, uvs, W, H) -> { texels: ArrayBuffer (W * H records of 32 bytes, ptmi_bake_texel), covered: count }
 *   positions, normals: 9 numbers per triangle (three corners, xyz); uvs: 6 per triangle (three corners, uv), in [0, 1]^2 with v = 0
 *   at the lightmap's bottom row.
 * Texel (x, y) has its centre at p = ((x + 0.5) / W, (y + 0.5) / H). For a triangle with lightmap coordinates a, b, c, in doubles:
 *   den = (b.y - c.y) * (a.x - c.x) + (c.x - b.x) * (a.y - c.y)                       (0: no area, covers nothing)
 *   w0  = ((b.y - c.y) * (p.x - c.x) + (c.x - b.x) * (p.y - c.y)) / den
 *   w1  = ((c.y - a.y) * (p.x - c.x) + (a.x - c.x) * (p.y - c.y)) / den
 *   w2  = (1 - w0) - w1
 * The texel belongs to the FIRST triangle in order with w0, w1, w2 all >= 0; its position and normal are
 * (w0 * v0 + w1 * v1) + w2 * v2 in doubles, rounded once to float32 (the Float32Array store). Uncovered records are all zeros.
 */

function rasterise(positions, normals, uvs, W, H) {
  var nTris = Math.floor(uvs.length / 6);
  var texels = new ArrayBuffer(W * H * 32);
  var f = new Float32Array(texels), u = new Uint32Array(texels);
  var covered = 0;
  for (var t = 0; t < nTris; t++) {
    var ax = uvs[6 * t], ay = uvs[6 * t + 1], bx = uvs[6 * t + 2], by = uvs[6 * t + 3], cx = uvs[6 * t + 4], cy = uvs[6 * t + 5];
    var den = (by - cy) * (ax - cx) + (cx - bx) * (ay - cy);
    if (den === 0 || !isFinite(den)) continue;
    // the texels whose centres can lie inside: a generous box, which decides nothing
    var clamp = function (v, hi) { return Math.max(0, Math.min(hi, v)); };
    var x0 = clamp(Math.floor(Math.min(ax, bx, cx) * W) - 1, W), x1 = clamp(Math.ceil(Math.max(ax, bx, cx) * W) + 1, W);
    var y0 = clamp(Math.floor(Math.min(ay, by, cy) * H) - 1, H), y1 = clamp(Math.ceil(Math.max(ay, by, cy) * H) + 1, H);
    for (var y = y0; y < y1; y++) {
      var py = (y + 0.5) / H;
      for (var x = x0; x < x1; x++) {
        var i = y * W + x;
        if (u[8 * i + 3]) continue;                                   // an earlier triangle has it
        var px = (x + 0.5) / W;
        var w0 = ((by - cy) * (px - cx) + (cx - bx) * (py - cy)) / den;
        var w1 = ((cy - ay) * (px - cx) + (ax - cx) * (py - cy)) / den;
        var w2 = (1 - w0) - w1;
        if (!(w0 >= 0 && w1 >= 0 && w2 >= 0)) continue;
        for (var k = 0; k < 3; k++) {
          f[8 * i + k] = (w0 * positions[9 * t + k] + w1 * positions[9 * t + 3 + k]) + w2 * positions[9 * t + 6 + k];
          f[8 * i + 4 + k] = (w0 * normals[9 * t + k] + w1 * normals[9 * t + 3 + k]) + w2 * normals[9 * t + 6 + k];
        }
        u[8 * i + 3] = 1;
        covered++;
      }
    }
  }
  return { texels: texels, covered: covered };
}

module.exports = { rasterise: rasterise };
