'use strict';
/**
 * hdr_decode.js — a Radiance .hdr (RGBE) reader for environment maps (Renderer.setEnvironment, render_cli.js --env). No dependency.
 *
 * Handles the `#?RADIANCE` / `#?RGBE` header with FORMAT=32-bit_rle_rgbe, the `-Y h +X w` orientation (row 0 on top: what an
 * equirectangular map with the +Y pole in row 0 wants), flat scanlines and the new-style run-length scanlines (2 2 hi lo, then the
 * four channels one after another, each as runs (count > 128: count - 128 copies of the next byte) and literal spans).
 * A texel (r, g, b, e) is (r, g, b) * 2^(e - 136), and zero when e = 0.
 * decodeHDR(bytes) -> { width, height, data: Float32Array(width * height * 4) } with alpha 1; throws on a malformed or truncated file.
 */

function fail(msg) { throw new Error('hdr_decode: ' + msg); }

function decodeHDR(bytes) {
  var b = bytes instanceof Uint8Array ? bytes : new Uint8Array(bytes);
  var pos = 0;
  function line() {
    var s = '';
    for (;;) {
      if (pos >= b.length) fail('the header ends before the resolution line');
      var c = b[pos++];
      if (c === 10) return s;
      if (s.length > 4096) fail('a header line is too long');
      s += String.fromCharCode(c);
    }
  }
  var first = line();
  if (first.slice(0, 2) !== '#?') fail('not a Radiance file (no #? signature)');
  var format = null;
  for (;;) {
    var l = line();
    if (l === '') break;
    var m = /^FORMAT=(.*)$/.exec(l.trim());
    if (m) format = m[1].trim();
  }
  if (format !== null && format !== '32-bit_rle_rgbe') fail('unsupported FORMAT ' + format);
  var res = /^-Y\s+(\d+)\s+\+X\s+(\d+)\s*$/.exec(line());
  if (!res) fail('only the -Y h +X w orientation is supported');
  var h = parseInt(res[1], 10), w = parseInt(res[2], 10);
  if (!(w > 0 && h > 0) || w * h > (1 << 28)) fail('bad size ' + w + 'x' + h);
  var out = new Float32Array(w * h * 4);
  var scan = new Uint8Array(w * 4);
  for (var y = 0; y < h; y++) {
    if (pos + 4 > b.length) fail('truncated at scanline ' + y);
    var rle = w >= 8 && w < 32768 && b[pos] === 2 && b[pos + 1] === 2 && (b[pos + 2] & 0x80) === 0;
    if (rle) {
      if (((b[pos + 2] << 8) | b[pos + 3]) !== w) fail('scanline ' + y + ' has another width');
      pos += 4;
      for (var ch = 0; ch < 4; ch++) {
        var x = 0;
        while (x < w) {
          if (pos >= b.length) fail('truncated in scanline ' + y);
          var n = b[pos++];
          if (n > 128) {
            n -= 128;
            if (x + n > w) fail('a run overflows scanline ' + y);
            if (pos >= b.length) fail('truncated in scanline ' + y);
            var v = b[pos++];
            for (var i = 0; i < n; i++) scan[(x++) * 4 + ch] = v;
          } else {
            if (n === 0 || x + n > w) fail('a literal span overflows scanline ' + y);
            if (pos + n > b.length) fail('truncated in scanline ' + y);
            for (var j = 0; j < n; j++) scan[(x++) * 4 + ch] = b[pos++];
          }
        }
      }
    } else {
      if (pos + w * 4 > b.length) fail('truncated in scanline ' + y);
      scan.set(b.subarray(pos, pos + w * 4));
      pos += w * 4;
    }
    for (var k = 0; k < w; k++) {
      var e = scan[k * 4 + 3], o = (y * w + k) * 4;
      var f = e === 0 ? 0 : Math.pow(2, e - 136);
      out[o] = scan[k * 4] * f; out[o + 1] = scan[k * 4 + 1] * f; out[o + 2] = scan[k * 4 + 2] * f; out[o + 3] = 1;
    }
  }
  return { width: w, height: h, data: out };
}

module.exports = { decodeHDR: decodeHDR };
