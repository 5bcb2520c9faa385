'use strict';
/**
 * hdr_encode.js — a Radiance .hdr (RGBE) writer, the counterpart of hdr_decode.js: what render_cli.js --hdr writes, and what
 * --env (Renderer.setEnvironment) reads back. No dependency.
 *
 * encodeHDR(rgba, width, height) -> Buffer: `#?RADIANCE`, FORMAT=32-bit_rle_rgbe, `-Y h +X w`, flat (uncompressed) scanlines,
 * row 0 of `rgba` (Float32Array, 4 floats per pixel, alpha ignored) on top. A texel is (r, g, b, e) with the largest channel's
 * exponent: value = mantissa * 2^(e - 136); a texel whose largest channel is below 1e-32, negative or not finite is written as zero.
 *
 * panoramaToEnvironment(rgba, width, height) -> Float32Array: an equirectangular render (Renderer.setProjection('equirect'): row 0 at
 * the bottom, forward in the middle column) in the layout of an environment map (include/ptmi.h ptmi_upload_environment: row 0 at
 * the +Y pole, u = atan2(z, x) / 2 pi + 1/2), for a camera with the default basis (forward -Z, right +X, up +Y): rows flipped, and
 * columns turned by a quarter of the width (forward, -Z, is u = 1/4 of the map and the middle of the render).
 */

function encodeHDR(rgba, width, height) {
  var head = Buffer.from('#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y ' + height + ' +X ' + width + '\n', 'latin1');
  var body = Buffer.alloc(width * height * 4);
  for (var i = 0; i < width * height; i++) {
    var r = rgba[4 * i], g = rgba[4 * i + 1], b = rgba[4 * i + 2];
    var m = Math.max(r, g, b);
    if (!(m >= 1e-32) || !isFinite(m)) continue;                       // zero texel: e = 0
    var e = Math.floor(Math.log2(m)) + 1;                              // m in [2^(e-1), 2^e)
    if (m / Math.pow(2, e) >= 1) e++;                                  // (log2's rounding at a power of two)
    var s = 256 / Math.pow(2, e);
    body[4 * i] = Math.max(0, Math.min(255, Math.floor(r * s)));
    body[4 * i + 1] = Math.max(0, Math.min(255, Math.floor(g * s)));
    body[4 * i + 2] = Math.max(0, Math.min(255, Math.floor(b * s)));
    body[4 * i + 3] = e + 128;
  }
  return Buffer.concat([head, body]);
}

function panoramaToEnvironment(rgba, width, height) {
  var out = new Float32Array(width * height * 4), turn = Math.round(width / 4);
  for (var y = 0; y < height; y++)
    for (var x = 0; x < width; x++) {
      var from = ((height - 1 - y) * width + (x + turn) % width) * 4, to = (y * width + x) * 4;
      out[to] = rgba[from]; out[to + 1] = rgba[from + 1]; out[to + 2] = rgba[from + 2]; out[to + 3] = 1;
    }
  return out;
}

module.exports = { encodeHDR: encodeHDR, panoramaToEnvironment: panoramaToEnvironment };
